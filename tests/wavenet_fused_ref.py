"""torch restatement of ONE coupling flow of the decoder (Start conv .. End conv + affine coupling, Modules.py:780-887) with the bf16 rounding
contract of the fused kernels (csrc/wavenet_fused.hip, csrc/wavenet_fused_bwd.hip) - forward, inverse and a HAND-WRITTEN
backward -, written from that contract and not from the kernels: plain torch, channel-first [B, channels, T] like the oracle, no GPU import.
A switchable rounding `r`: identity gives the reference's arithmetic (equal to oracle.glowtts_ref.coupling and, for the backward, to
torch.autograd of it: tests/test_wavenet_fused_ref_cpu.py), `rb` (bf16 nearest even and back) gives the contract.

THE CONTRACT.  Forward (H = 192 hidden channels, C2 = C / 2, L layers):
  * every conv weight is rounded after w = g v / ||v|| was formed in the run's dtype (End has a plain weight, rounded as well);
  * h_0 = r((Start(r(x_a)) + b) * mask);
  * the In_l pre-activation (+ bias), the dropout multiplier and the conditioning add stay in the run's dtype: pre = (In_l(h_l) + b) * keep + cond;
  * (t, s) = (tanh, sigmoid) of the unrounded pre; acts_l = r(t * s) from the unrounded pair; the KEPT gate pair is (r(t), r(s));
  * h_{l+1} = r((h_l + res_l + b) * mask) with h_l the already rounded state;
  * the skip sum is not rounded; skip = (sum_l (skip_l + b)) * mask is kept unrounded and enters the End conv as r(skip);
  * (m, logs) = End(r(skip)) + b, the coupling line x_b' = (m + exp(logs) x_b) * mask (inverse: (x_b - m) exp(-logs) * mask) and the log-determinant
    sum(logs * mask) are not rounded.
Backward (d = gradient of a scalar loss):
  * d(m, logs) is rounded to bf16: it is the operand of End^T and of the End conv's weight / bias gradient;
  * d skip = r((d(m, logs) W_end^T) * mask);
  * per layer, last to first: d acts = [d h_{l+1} | d skip] W_rs_l^T (last layer: d skip alone); (da, ds) = d acts * (s (1 - t^2), t s (1 - s)) from the KEPT
    rounded pair; the conditioning gradient is the per-utterance sum of (da, ds) over the frames, BEFORE the keep multiplier and unrounded;
    dins_l = r((da, ds) * keep); d h_l = (In_l^T(dins_l) + d h_{l+1}) * mask, rounded to bf16 for l >= 1;
  * d h_0 is kept in fp32 where C2 is no multiple of 8 and as bf16 where it is (the kernels' `dh0_bf16`: the bf16 copy of x_a exists only then); as an
    OPERAND - of Start^T and of the Start conv's weight gradient - it is bf16 either way (every product runs on bf16 MFMA inputs);
  * weight and bias gradients are plain products / row sums of the rounded tensors above: r(x_a), h_l, acts_l, r(skip), d h_0, dins_l, [d h_{l+1} | d skip],
    d(m, logs);  d x_a += r(d h_0) W_start^T and d x_b = d x_b' exp(logs) * mask are not rounded.
Dropout enters as injected keep multipliers (tests/dropout_masks.hip_keep_multipliers), conditioning as the per-utterance rows [B, L, 2H].

RUNS (`VARIANTS`):  ref64 = r identity, float64;  emu64 = the contract in float64;  emu32 = the contract in float32;  emu32b = the contract in float32 with the
k = 5 conv as five per-tap products added as ((tap0 + tap4) + (tap1 + tap3)) + tap2, tanh(x) = 1 - 2 / (exp(2x) + 1) and sigmoid(x) = 1 / (1 + exp(-x)) (the forms
csrc/device_common.h uses).  emu32 / emu32b differ from emu64 by what a correct fp32 implementation may differ by.

`decoder(...)` wraps the coupling in the oracle's own squeeze / ActNorm / invertible 1x1 / unsqueeze (oracle.glowtts_ref) so that F flows are compared
end to end; everything outside the coupling is differentiated by torch.autograd in the run's dtype, the coupling by the hand-written backward.
Shared by tests/test_wavenet_fused_ref_cpu.py and tests/test_gpu_wavenet_fused_contract.py."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import glowtts_ref as O  # noqa: E402


def rb(t):
    """round to bf16 (nearest even) and back"""
    return t.float().bfloat16().to(t.dtype)


def ident(t):
    return t


# name -> (dtype, rounding, the other summation order and the other tanh / sigmoid forms)
VARIANTS = {"ref64": (torch.float64, ident, False), "emu64": (torch.float64, rb, False), "emu32": (torch.float32, rb, False), "emu32b": (torch.float32, rb, True)}
KEYS = ("w_start", "b_start", "w_in", "b_in", "w_rs", "b_rs", "w_end", "b_end")


def flow_params(sd, p, n_layers):
    """The effective (weight-normalised, UNROUNDED) weights of the coupling at prefix `p` (`...Flows.f.layers.2`), differentiable in the state dict's entries."""
    q = p + ".layer_Dict."
    w = lambda n: O.eff_weight(sd, q + n)
    return {"w_start": w("Start"), "b_start": sd[q + "Start.bias"],
            "w_in": [w(f"WaveNet.layer_Dict.In_{l}") for l in range(n_layers)], "b_in": [sd[q + f"WaveNet.layer_Dict.In_{l}.bias"] for l in range(n_layers)],
            "w_rs": [w(f"WaveNet.layer_Dict.Res_Skip_{l}") for l in range(n_layers)], "b_rs": [sd[q + f"WaveNet.layer_Dict.Res_Skip_{l}.bias"] for l in range(n_layers)],
            "w_end": w("End"), "b_end": sd[q + "End.bias"]}


def _conv5(x, w, split):
    if not split:
        return F.conv1d(x, w, None, padding=2)
    T = x.shape[2]
    pad = F.pad(x, (2, 2))
    tap = [F.conv1d(pad[:, :, j:j + T], w[:, :, j:j + 1]) for j in range(5)]
    return ((tap[0] + tap[4]) + (tap[1] + tap[3])) + tap[2]


def _gate(pre, H, alt):
    a, b = pre[:, :H], pre[:, H:]
    if alt:
        return 1.0 - 2.0 / (torch.exp(2.0 * a) + 1.0), 1.0 / (1.0 + torch.exp(-b))
    return torch.tanh(a), torch.sigmoid(b)


def coupling_forward(P, x, mask, variant, reverse=False, cond=None, keep=None):
    """P: flow_params(...) in the run's dtype; x [B, C, T]; mask [B, 1, T]; cond None or [B, L, 2H]; keep None or a list of L keep multipliers [B, 2H, T].
    -> (out [B, C, T], logdet [B] or None, kept): kept holds what the kernels keep (hs, gates, acts, skip, m, logs) and what the backward needs."""
    _, r, alt = VARIANTS[variant]
    C2, H, L = x.shape[1] // 2, P["b_start"].shape[0], len(P["w_in"])
    xa, xb = x[:, :C2], x[:, C2:]
    xar = r(xa)
    h = r((F.conv1d(xar, r(P["w_start"])) + P["b_start"][None, :, None]) * mask)
    hs, gates, acts, total = [], [], [], 0
    for l in range(L):
        pre = _conv5(h, r(P["w_in"][l]), alt) + P["b_in"][l][None, :, None]
        if keep is not None:
            pre = pre * keep[l]
        if cond is not None:
            pre = pre + cond[:, l, :, None]
        t, s = _gate(pre, H, alt)
        a = r(t * s)
        hs.append(h)
        gates.append((r(t), r(s)))
        acts.append(a)
        rs = F.conv1d(a, r(P["w_rs"][l])) + P["b_rs"][l][None, :, None]
        if l < L - 1:
            h = r((h + rs[:, :H]) * mask)
            total = total + rs[:, H:]
        else:
            total = total + rs
    skip = total * mask
    skr = r(skip)
    outs = F.conv1d(skr, r(P["w_end"])) + P["b_end"][None, :, None]
    m, logs = outs[:, :C2], outs[:, C2:]
    if reverse:
        xbn, logdet = (xb - m) * torch.exp(-logs) * mask, None
    else:
        xbn, logdet = (m + torch.exp(logs) * xb) * mask, (logs * mask).sum((1, 2))
    kept = {"xar": xar, "xb": xb, "hs": hs, "gates": gates, "acts": acts, "skip": skip, "skr": skr, "m": m, "logs": logs, "mask": mask, "keep": keep}
    return torch.cat([xa, xbn], 1), logdet, kept


def coupling_backward(P, kept, dout, dlogdet, variant):
    """The hand-written backward of `coupling_forward` (reverse = False): dout [B, C, T] and dlogdet [B] -> (dx [B, C, T], gradients of P's entries in P's
    layout, dcond [B, L, 2H]).  With r = identity: the exact gradient."""
    _, r, _ = VARIANTS[variant]
    mask, keep = kept["mask"], kept["keep"]
    C2, H, L = kept["m"].shape[1], P["b_start"].shape[0], len(P["w_in"])
    wT = lambda w: w[:, :, 0].t()[:, :, None]                  # the 1x1 conv of the transposed matrix
    dxa, dxbn = dout[:, :C2], dout[:, C2:] * mask
    e = torch.exp(kept["logs"])
    dm, dlogs = dxbn, dxbn * e * kept["xb"] + dlogdet[:, None, None] * mask
    dxb = dxbn * e
    do = r(torch.cat([dm, dlogs], 1))
    G = {"w_end": torch.einsum("bot,bit->oi", do, kept["skr"])[:, :, None], "b_end": do.sum((0, 2)),
         "w_in": [None] * L, "b_in": [None] * L, "w_rs": [None] * L, "b_rs": [None] * L}
    dskip = r(F.conv1d(do, wT(r(P["w_end"]))) * mask)
    dcond = []
    dh = None                                                  # d h_{l+1}
    for l in range(L - 1, -1, -1):
        dy = dskip if l == L - 1 else torch.cat([dh, dskip], 1)
        G["w_rs"][l] = torch.einsum("bot,bit->oi", dy, kept["acts"][l])[:, :, None]
        G["b_rs"][l] = dy.sum((0, 2))
        da_ = F.conv1d(dy, wT(r(P["w_rs"][l])))
        t, s = kept["gates"][l]
        dpre = torch.cat([da_ * s * (1 - t * t), da_ * t * s * (1 - s)], 1)
        dcond.append(dpre.sum(2))
        dins = r(dpre * keep[l]) if keep is not None else r(dpre)
        hp = F.pad(kept["hs"][l], (2, 2))
        T = dins.shape[2]
        G["w_in"][l] = torch.stack([torch.einsum("bot,bit->oi", dins, hp[:, :, j:j + T]) for j in range(5)], 2)
        G["b_in"][l] = dins.sum((0, 2))
        dh_ = F.conv_transpose1d(dins, r(P["w_in"][l]), padding=2)
        if dh is not None:
            dh_ = dh_ + dh
        dh_ = dh_ * mask
        dh = r(dh_) if (l >= 1 or C2 % 8 == 0) else dh_
    dh0 = r(dh)
    G["w_start"] = torch.einsum("bot,bit->oi", dh0, kept["xar"])[:, :, None]
    G["b_start"] = dh.sum((0, 2))
    dxa = dxa + F.conv1d(dh0, wT(r(P["w_start"])))
    return torch.cat([dxa, dxb], 1), G, torch.stack(dcond[::-1], 1)


def _flatten(P):
    out = []
    for k in KEYS:
        out += list(P[k]) if isinstance(P[k], list) else [P[k]]
    return out


def _unflatten(flat, L):
    P, i = {}, 0
    for k in KEYS:
        if k in ("w_in", "b_in", "w_rs", "b_rs"):
            P[k] = list(flat[i:i + L])
            i += L
        else:
            P[k] = flat[i]
            i += 1
    return P


class Coupling(torch.autograd.Function):
    """coupling_forward with coupling_backward as its autograd: (out, logdet) = Coupling.apply(variant, L, sink, keep, mask, x, cond, *weights)."""

    @staticmethod
    def forward(ctx, variant, L, sink, keep, mask, x, cond, *flat):
        P = _unflatten(flat, L)
        out, logdet, kept = coupling_forward(P, x, mask, variant, False, cond, keep)
        ctx.P, ctx.kept, ctx.variant, ctx.has_cond = P, kept, variant, cond is not None
        if sink is not None:
            sink.append(kept)
        return out, logdet

    @staticmethod
    def backward(ctx, dout, dlogdet):
        if dout is None:
            dout = torch.zeros_like(ctx.kept["mask"]).expand(-1, 2 * ctx.kept["m"].shape[1], -1)
        if dlogdet is None:
            dlogdet = dout.new_zeros(dout.shape[0])
        dx, G, dcond = coupling_backward(ctx.P, ctx.kept, dout, dlogdet, ctx.variant)
        return (None, None, None, None, None, dx, dcond if ctx.has_cond else None) + tuple(_flatten(G))


def cast_sd(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def decoder(sd, x, mask, cfg, variant, reverse=False, cond=None, keep=None, sink=None, p="layer_Dict.Decoder"):
    """oracle.glowtts_ref.decoder with the coupling of every flow restated in the run `variant`.  x [B, Cm, Tm], mask [B, 1, Tm] and sd in the run's dtype;
    cond None or [B, F, L, 2H]; keep None or {(flow, layer): [B, 2H, T]}; sink: a list that receives, per flow in the order run, the kept tensors + "xout"
    (the flow's output).  -> (z or mel, logdet or None, mask)."""
    L = cfg.wn_layers
    x, sm = O.squeeze(x, mask, cfg.n_squeeze)
    logdets = []
    for f in (range(cfg.n_flows - 1, -1, -1) if reverse else range(cfg.n_flows)):
        q = f"{p}.layer_Dict.Flows.{f}.layers"
        P = flow_params(sd, q + ".2", L)
        cf = cond[:, f] if cond is not None else None
        if reverse:
            x, _, kept = coupling_forward(P, x, sm, variant, True, cf)
            x, _ = O.inv1x1(sd, q + ".1", x, sm, cfg, True)
            x, _ = O.actnorm(sd, q + ".0", x, sm, True)
        else:
            x, l0 = O.actnorm(sd, q + ".0", x, sm, False)
            x, l1 = O.inv1x1(sd, q + ".1", x, sm, cfg, False)
            kf = [keep[(f, l)] for l in range(L)] if keep is not None else None
            mine = [] if sink is not None else None
            x, l2 = Coupling.apply(variant, L, mine, kf, sm, x, cf, *_flatten(P))
            logdets += [l0, l1, l2]
            if sink is not None:
                mine[0]["xout"] = x.detach()
                sink.append(mine[0])
    x, m = O.unsqueeze(x, sm, cfg.n_squeeze)
    return x, (None if reverse else torch.stack(logdets).sum(0)), m
