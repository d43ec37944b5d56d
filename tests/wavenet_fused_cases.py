"""The cases and the bars of the fused coupling kernels' contract tests, shared by tests/test_wavenet_fused_ref_cpu.py (which holds the reference runs
emu32 / emu32b of tests/wavenet_fused_ref.py to the bars: the guard that the bars are what reference arithmetic satisfies) and
tests/test_gpu_wavenet_fused_contract.py (which holds the kernels to them).  Every reference is computed once per process and not modified.

CASES.  The fused kernels (csrc/wavenet_fused.hip, csrc/wavenet_fused_bwd.hip) admit 1 <= L <= 4 layers and 64 < C2 = C / 2 <= 96, C % 8 == 0: with
Num_Squeeze 2 that is Sound.Mel_Dim in {68, 72, .., 96}.  Configurations (L, Mel_Dim): (1, 68), (1, 96), (2, 72), (2, 96), (3, 88), (3, 92), (4, 68), (4, 96)
and the benchmarked (4, 80).  They reach: the K-padding zeroing (96 - C2) / 4 = 0 .. 7; column predicates at C2 no multiple of 16; the next-flow ActNorm / 1x1
epilogue at G = C2 / 2 = 34 .. 48; halo 2 (L - 1) and nvalid(L) = 64 - 4 (L - 1) = 64 / 60 / 56 / 52 owned rows per workgroup; L = 1 (no Res_Skip image, no residual
layer); d h_0 kept as fp32 (C2 % 8 != 0) and as bf16; 88 is the last C2 whose x_a staging fitted two rounds of the workgroup, 92 the first that needs three.
Per configuration ONE ragged batch of four, F = 2 flows: tm = 2 (nvalid - 3) frames, lengths [tm, tm - 9, 36, 2] - nvalid + 1 rows per utterance (212 .. 260 flat
rows, 4 - 5 workgroups), so the utterance boundaries fall 1, 2 and 3 rows behind a window seam, the longest utterance spans a seam with mask 1 on both sides, one
length is odd (the squeeze drops a frame), one window holds several utterances and one utterance is a single squeezed frame.  With nvalid + 1 rows per utterance
every seam of these batches falls on or next to pad rows (for L >= 2 no owned row with mask 1 sees the last four state rows of its window: the parent commit's unstaged
x_a rows at Mel_Dim 92 / 96 passed every ragged batch with L >= 2), so per configuration one more case ("span") is a single utterance of nvalid + 9 squeezed frames, whose
rows carry mask 1 on both sides of the seam at row nvalid (two workgroups).
Variants: speaker conditioning (256) with dropout 0.3 on (2, 96) and (3, 72); dropout 0.3 alone on (1, 68) and (4, 96).  Weights: helpers.full_width_state;
mels randn * 1.5 clamped to +-4; the loss is sum(z * wz) + sum(logdet * wl) with wz ~ N(0, 1), wl ~ N(0, 0.05^2).

NOTATION.  ref64 / ref32: the unrounded restatement in float64 / float32; emu64: the bf16 contract in float64; per tensor e_bf = max |emu64 - ref64|,
rms_bf = rms(emu64 - ref64), e32 = max |ref32 - ref64|, scale = max |ref64| (all over the frames the mask keeps).

THE BARS, per tensor:  max |got - emu64| <= a * e_bf  and  rms(got - emu64) <= b * rms_bf, with (a, b) per KEY = twice the worst value emu32 / emu32b reach on
that key over all twenty-two cases (tests/test_wavenet_fused_ref_cpu.py prints every ratio and asserts that the reference runs stay within three quarters of every bar - one half where
the tables were made; which element float32 flips depends on the host's summation order -; nothing is taken from the kernel).  Twice: the kernel is one more independent summation order and one more exp / rcp.  A key is a kept
tensor's name WITH its flow and layer, or a gradient's kind with its flow - because of what was measured:

MEASURED (`BARS` / `FRACS` below carry every value; python tests/wavenet_fused_cases.py prints them).  A bar separates the contracted rounding points from any other
bf16 scheme - which sits about sqrt(2) e_bf away - where a <= 0.75 and b <= 0.35.  The reference runs meet that only at the head of the chain:
    hs0.0 0.31 / 0.016 e_bf,  gates0.0 0.20 / 0.05,  acts0.0 0.26 / 0.05,  gates0.1 0.17 / 0.16,  acts0.1 0.27 / 0.15     (max / rms, emu32 or emu32b against emu64)
and drift apart behind it: every state h_l is STORED as bf16, so a value that float32 and float64 arithmetic put on different sides of a rounding midpoint differs by
a whole unit in the last place (e_bf is half of one), and each such flip moves every pre-activation of the next layer that sees it.  The fraction of kept elements
that differ by more than 1e-6 grows 0.15 % (hs0.0) -> 0.65 % (hs0.1) -> 6 % -> 13 % (hs0.3) -> 28 - 60 % in flow 1; skip0 / m0 / logs0 / x1 reach 0.36 / 0.44 / 0.52 / 0.52
e_bf in max and 0.26 - 0.37 in rms, every tensor of flow 1, z, the inverse and every gradient 0.47 - 1.8 e_bf in max and 0.48 - 1.34 in rms.  Those keys (all but `DISCRIMINATING`)
miss the condition: their bars are bounds that reference arithmetic itself needs, and they separate a wrong kernel - one wrong column, four wrong rows per window are
tens to hundreds of e_bf, e_bf being 0.1 - 4 % of a tensor's scale - but not another rounding scheme.  The tensors STORED as bf16 (`STORED_BF16`: hs, gates, acts) are
therefore ALSO held to the fraction-of-elements form `close` of tests/test_gpu_wavenet_fused.py - at most `FRACS[key]` of the elements off by more than 1e-6 (twice
the reference runs' worst fraction: the existing test's 2 % (l + 1) is what two fp32 paths keep, not what float32 against float64 keeps), none by more than 0.05
(hs: 0.1) - and the gradients to the envelope tier's cosine / norm form against the per-conv backward (tests/test_gpu_wavenet_fused_contract.py, tier b).
The log-determinant is four sums per case in which the bf16 errors average out and the fp32 ones do not: e_bf / e32 is 88 - 120 on these cases, depending on the
host's summation order, so the guard below cannot hold for it; it is held to the envelope's form |got - emu64| <= 2e-3 |emu64| + 0.05 and its summands (`logs`) to
ratio bars.  Every other tensor has e_bf > 2600 e32.
(For the record, not a source of any bar: on an MI355X the kernels' worst ratios equal the reference runs' - 0.2 - 0.3 e_bf at the head of flow 0, 0.7 - 1.4 in
flow 1 and the gradients - and use at most 0.73 of any bar.)
Guards on every tensor under a ratio bar: e_bf > 100 e32, scale > 1e-3, rms_bf > 0."""
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wavenet_fused_ref as E  # noqa: E402
from dropout_masks import hip_keep_multipliers  # noqa: E402
from helpers import full_width_state  # noqa: E402
from oracle import glowtts_ref as O  # noqa: E402

N_FLOWS, DROP_P, SPK_DIM, H = 2, 0.3, 256, 192
CONFIGS = [(1, 68), (1, 96), (2, 72), (2, 96), (3, 88), (3, 92), (4, 68), (4, 96), (4, 80)]
SPANS = [(L, m, "span") for L, m in CONFIGS]
CASES = [(L, m, "plain") for L, m in CONFIGS] + [(2, 96, "spk+drop"), (3, 72, "spk+drop"), (1, 68, "drop"), (4, 96, "drop")] + SPANS
RUNS = ("ref64", "ref32", "emu64", "emu32", "emu32b")
E.VARIANTS.setdefault("ref32", (torch.float32, E.ident, False))
_CASE, _REFS = {}, {}


def nvalid(L):
    """owned rows of a workgroup's 64-row window"""
    return 64 - 4 * (L - 1)


def lengths_of(L, variant="plain"):
    if variant == "span":                                    # one utterance of nvalid + 9 squeezed frames (an odd number of frames): rows 2 .. nvalid + 10 carry mask 1
        tm = 2 * (nvalid(L) + 10)
        return [tm - 1], tm
    tm = 2 * (nvalid(L) - 3)
    return [tm, tm - 9, 36, 2], tm


def case_id(c):
    return f"L{c[0]}-mel{c[1]}-{c[2]}"


def build(c):
    """The inputs of case c = (L, Mel_Dim, variant): weights, mels, lengths, loss weights, the inverse's input, conditioning rows, dropout word and multipliers."""
    if c in _CASE:
        return _CASE[c]
    L, mel, variant = c
    spk_dim = SPK_DIM if "spk" in variant else 0
    drop_p = DROP_P if "drop" in variant else 0.0
    g = torch.Generator().manual_seed(7000 + 100 * L + mel + (1 if spk_dim else 0) + (2 if drop_p else 0))
    cfg, sd = full_width_state(N_FLOWS, g, spk_dim=spk_dim, mel_dim=mel, n_layers=L)
    lengths, tm = lengths_of(L, variant)
    B, T = len(lengths), tm // 2
    mels = (torch.randn(B, mel, tm, generator=g) * 1.5).clamp(-4, 4)
    wz, wl = torch.randn(B, mel, tm, generator=g), torch.randn(B, generator=g) * 0.05
    zin = torch.randn(B, mel, tm, generator=g) * 0.6
    cond = None
    if spk_dim:                                              # cond[b, f, l] = Speaker_l(spk_b) (Modules.py:863-866), formed once in float64 and handed to every run as fp32 rows
        spk = torch.randn(B, spk_dim, generator=g)
        spk = (spk / spk.norm(dim=1, keepdim=True)).double()
        sd64 = E.cast_sd(sd, torch.float64)
        cond = torch.stack([torch.stack([O.conv(sd64, f"layer_Dict.Decoder.layer_Dict.Flows.{f}.layers.2.layer_Dict.WaveNet.layer_Dict.Speaker_{l}", spk.unsqueeze(2))[:, :, 0]
                                         for l in range(L)], 1) for f in range(N_FLOWS)], 1).float()
        sd = {k: v for k, v in sd.items() if ".Speaker_" not in k}
    word = 40000 + 7 * mel + L
    keep = {(f, l): hip_keep_multipliers(word, f, l, B, T, H, drop_p) for f in range(N_FLOWS) for l in range(L)} if drop_p else None
    out = dict(cfg=cfg, sd=sd, mels=mels, lengths=lengths, ml=torch.tensor(lengths), tm=tm, T=T, B=B, wz=wz, wl=wl, zin=zin, cond=cond, word=word, keep=keep,
               drop_p=drop_p, L=L, mel=mel, C2=mel)
    _CASE[c] = out
    return out


def kind_of(name):
    """Tensor name -> its kind (flow and layer numbers dropped)."""
    if name.startswith("grad/"):
        k = name.split("Flows.")[1].split(".", 1)[1]         # layers.2.layer_Dict.WaveNet.layer_Dict.In_3.weight_v
        k = k.replace("layer_Dict.", "").replace("layers.", "")
        return "grad/" + re.sub(r"_\d+\.", ".", k)
    return re.sub(r"[\d.]+$", "", name)


def key_of(name):
    """Tensor name -> the key of its bar: a kept tensor's own name (flow and layer: the reference runs drift apart from layer to layer and from flow to flow,
    see the docstring); a gradient's kind with its flow, the layers merged."""
    if name.startswith("grad/"):
        return "grad/f" + name.split("Flows.")[1].split(".", 1)[0] + "/" + kind_of(name)[5:]
    return name


def run(c, variant):
    """Every compared tensor of one run of case c: name -> float64 tensor (frames the mask drops are zero)."""
    K = build(c)
    dtype = E.VARIANTS[variant][0]
    cfg, L = K["cfg"], K["L"]
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    sd = {k: leaf(v) for k, v in K["sd"].items()}
    x = leaf(K["mels"])
    cond = leaf(K["cond"]) if K["cond"] is not None else None
    keep = {k: v.to(dtype) for k, v in K["keep"].items()} if K["keep"] is not None else None
    mask = O.mask_from_lengths(K["ml"], K["tm"]).to(dtype)
    sink = []
    z, ld, _ = E.decoder(sd, x, mask, cfg, variant, cond=cond, keep=keep, sink=sink)
    ((z * K["wz"].to(dtype)).sum() + (ld * K["wl"].to(dtype)).sum()).backward()
    out = {"z": z.detach(), "logdet": ld.detach(), "dmel": x.grad}
    if cond is not None:
        out["dcond"] = cond.grad
    for k, v in sd.items():
        out["grad/" + k] = v.grad
    for f, kept in enumerate(sink):
        sm = kept["mask"]
        for l in range(L):
            out[f"hs{f}.{l}"] = kept["hs"][l] * sm
            out[f"gates{f}.{l}"] = torch.cat(kept["gates"][l], 1) * sm
            out[f"acts{f}.{l}"] = kept["acts"][l] * sm
        out[f"skip{f}"], out[f"m{f}"], out[f"logs{f}"], out[f"x{f + 1}"] = kept["skip"], kept["m"] * sm, kept["logs"] * sm, kept["xout"]
    with torch.no_grad():
        sdd = {k: v.detach() for k, v in sd.items()}
        out["mel_inv"] = E.decoder(sdd, K["zin"].to(dtype), mask, cfg, variant, reverse=True, cond=cond.detach() if cond is not None else None)[0]
    if K["B"] == 1:
        del out["logdet"]                                    # (one number: its e_bf is one draw that may be next to nothing - `logs` carries the comparison)
    return {k: v.detach().double() for k, v in out.items()}


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def refs(c):
    """{run: tensors} of case c plus "stats": name -> (e_bf, rms_bf, e32, scale)."""
    if c not in _REFS:
        R = {v: run(c, v) for v in RUNS}
        R["stats"] = {n: (float((R["emu64"][n] - t).abs().max()), rms(R["emu64"][n] - t), float((R["ref32"][n] - t).abs().max()), float(t.abs().max()))
                      for n, t in R["ref64"].items()}
        _REFS[c] = R
    return _REFS[c]


def ratios(name, got, R):
    """(max |got - emu64| / e_bf, rms(got - emu64) / rms_bf) of one tensor"""
    e_bf, r_bf, _, _ = R["stats"][name]
    d = got.double().cpu() - R["emu64"][name]
    return float(d.abs().max()) / e_bf, rms(d) / r_bf


def close(a, b, what, atol=0.0, frac=0.0, big=None):
    """|a - b| <= atol everywhere except on at most `frac` of the elements (bf16 one-ulp flips), where it stays <= big (tests/test_gpu_wavenet_fused.py's form)."""
    d = (a.double() - b.double()).abs()
    bad = (d > atol).double().mean().item()
    assert bad <= frac, (what, "fraction above atol", bad, "max", d.max().item())
    if big is not None:
        assert d.max().item() <= big, (what, d.max().item())
    return bad, d.max().item()


def check(tag, name, got, R, bars=None, fracs=None):
    """One tensor against emu64 under the bar of its key; prints the ratios.  -> (max ratio, rms ratio, fraction of elements off by more than 1e-6 or None)"""
    bars, fracs = BARS if bars is None else bars, FRACS if fracs is None else fracs
    key, kind = key_of(name), kind_of(name)
    e_bf, r_bf, e32, scale = R["stats"][name]
    got = got.double().cpu()
    assert got.shape == R["emu64"][name].shape, (tag, name, got.shape, R["emu64"][name].shape)
    if name == "logdet":                                     # the envelope's form (see the docstring)
        want = R["emu64"][name]
        print(f"{tag} logdet: |got - emu64| {[round(v, 5) for v in (got - want).abs().tolist()]} of {[round(v, 2) for v in want.tolist()]}  (e_bf {e_bf:.2e}, e32 {e32:.2e})")
        assert bool(((got - want).abs() <= 2e-3 * want.abs() + 0.05).all()), (tag, name, got, want)
        return None
    assert e_bf > 100 * e32 > 0 and scale > 1e-3 and r_bf > 0, (tag, name, "the case tests nothing", e_bf, e32, scale)
    rm, rr = ratios(name, got, R)
    a, b = bars[key]
    bad = None
    line = f"{tag} {name}: e_bf / scale {e_bf / scale:.2e}  e32 / e_bf {e32 / e_bf:.1e}  max ratio {rm:.3f} (bar {a})  rms ratio {rr:.3f} (bar {b})"
    if kind in STORED_BF16:
        d = (got - R["emu64"][name]).abs()
        bad = float((d > 1e-6).double().mean())
        line += f"  fraction off {bad:.4f} (bar {fracs[key]})  max {float(d.max()):.3e} (bar {STORED_BF16[kind]})"
    print(line)
    assert rm <= a and rr <= b, (tag, name, rm, a, rr, b)
    if bad is not None:
        close(got, R["emu64"][name], f"{tag} {name}", atol=1e-6, frac=fracs[key], big=STORED_BF16[kind])
    return rm, rr, bad


def measure():
    """The worst (max ratio, rms ratio, fraction off) of emu32 / emu32b per key over all cases: what BARS / FRACS are twice of (python tests/wavenet_fused_cases.py
    prints the tables)."""
    worst = {}
    for c in CASES:
        R = refs(c)
        for name in R["ref64"]:
            if name == "logdet":
                continue
            for v in ("emu32", "emu32b"):
                rm, rr = ratios(name, R[v][name], R)
                bad = float(((R[v][name] - R["emu64"][name]).abs() > 1e-6).double().mean())
                w = worst.setdefault(key_of(name), [0.0, 0.0, 0.0])
                w[0], w[1], w[2] = max(w[0], rm), max(w[1], rr), max(w[2], bad)
    return worst


def up(x, digits=2):
    """x rounded up to `digits` decimals"""
    import math
    return math.ceil(x * 10 ** digits - 1e-9) / 10 ** digits


# tensors the kernels STORE as bf16 (value: the largest single difference the fraction form allows, as in tests/test_gpu_wavenet_fused.py)
STORED_BF16 = {"hs": 0.1, "gates": 0.05, "acts": 0.05}
# key: (a, b) = twice the worst (max, rms) ratio of emu32 / emu32b over the cases, rounded up; the measured values stand behind them
BARS = {
    "z": (2.27, 1.23),                                                 # measured 1.134, 0.615
    "dmel": (1.77, 1.48),                                              # measured 0.883, 0.738
    "grad/f0/0.logs": (1.91, 1.71),                                    # measured 0.954, 0.853
    "grad/f0/0.bias": (1.95, 1.63),                                    # measured 0.971, 0.812
    "grad/f0/1.weight": (3.6, 2.68),                                  # measured 1.797, 1.337
    "grad/f0/2.Start.weight_v": (1.65, 1.27),                          # measured 0.824, 0.632
    "grad/f0/2.Start.weight_g": (1.95, 1.5),                          # measured 0.971, 0.746
    "grad/f0/2.Start.bias": (1.52, 1.46),                              # measured 0.759, 0.729
    "grad/f0/2.WaveNet.In.weight_v": (1.17, 1.11),                     # measured 0.585, 0.551
    "grad/f0/2.WaveNet.In.weight_g": (1.59, 1.11),                     # measured 0.792, 0.551
    "grad/f0/2.WaveNet.In.bias": (1.82, 1.27),                         # measured 0.908, 0.631
    "grad/f0/2.WaveNet.Res_Skip.weight_v": (1.35, 1.21),               # measured 0.674, 0.603
    "grad/f0/2.WaveNet.Res_Skip.weight_g": (1.68, 1.31),               # measured 0.839, 0.651
    "grad/f0/2.WaveNet.Res_Skip.bias": (2.4, 1.86),                   # measured 1.198, 0.927
    "grad/f0/2.End.weight": (1.72, 1.18),                              # measured 0.857, 0.587
    "grad/f0/2.End.bias": (2.86, 1.92),                                # measured 1.430, 0.955
    "grad/f1/0.logs": (1.81, 1.6),                                    # measured 0.903, 0.795
    "grad/f1/0.bias": (2.58, 1.73),                                    # measured 1.285, 0.863
    "grad/f1/1.weight": (2.69, 2.27),                                  # measured 1.344, 1.130
    "grad/f1/2.Start.weight_v": (1.86, 1.68),                          # measured 0.926, 0.838
    "grad/f1/2.Start.weight_g": (2.62, 1.94),                          # measured 1.307, 0.969
    "grad/f1/2.Start.bias": (1.79, 1.84),                              # measured 0.891, 0.917
    "grad/f1/2.WaveNet.In.weight_v": (2.24, 1.66),                     # measured 1.117, 0.830
    "grad/f1/2.WaveNet.In.weight_g": (3.11, 1.77),                     # measured 1.553, 0.883
    "grad/f1/2.WaveNet.In.bias": (2.58, 1.87),                         # measured 1.289, 0.933
    "grad/f1/2.WaveNet.Res_Skip.weight_v": (2.22, 1.66),               # measured 1.107, 0.829
    "grad/f1/2.WaveNet.Res_Skip.weight_g": (2.33, 1.74),               # measured 1.163, 0.866
    "grad/f1/2.WaveNet.Res_Skip.bias": (2.39, 1.81),                   # measured 1.195, 0.905
    "grad/f1/2.End.weight": (2.23, 1.64),                              # measured 1.114, 0.816
    "grad/f1/2.End.bias": (3.04, 1.75),                                # measured 1.518, 0.873
    "hs0.0": (0.62, 0.04),                                             # measured 0.307, 0.016
    "gates0.0": (0.41, 0.11),                                          # measured 0.202, 0.051
    "acts0.0": (0.53, 0.11),                                           # measured 0.262, 0.052
    "skip0": (0.72, 0.53),                                             # measured 0.355, 0.261
    "m0": (0.89, 0.73),                                                # measured 0.442, 0.361
    "logs0": (1.03, 0.75),                                             # measured 0.511, 0.371
    "x1": (1.05, 0.73),                                                # measured 0.524, 0.363
    "hs1.0": (2.54, 1.32),                                             # measured 1.269, 0.657
    "gates1.0": (1.42, 1.34),                                          # measured 0.708, 0.669
    "acts1.0": (1.4, 1.36),                                           # measured 0.700, 0.676
    "skip1": (1.65, 1.48),                                             # measured 0.822, 0.738
    "m1": (1.81, 1.57),                                                # measured 0.905, 0.784
    "logs1": (1.96, 1.56),                                             # measured 0.979, 0.776
    "x2": (2.27, 1.23),                                                # measured 1.134, 0.615
    "mel_inv": (1.89, 1.44),                                           # measured 0.943, 0.719
    "hs0.1": (1.78, 0.17),                                             # measured 0.889, 0.084
    "gates0.1": (0.34, 0.32),                                          # measured 0.169, 0.157
    "acts0.1": (0.55, 0.3),                                           # measured 0.274, 0.150
    "hs1.1": (3.27, 1.48),                                             # measured 1.630, 0.735
    "gates1.1": (1.78, 1.5),                                          # measured 0.887, 0.748
    "acts1.1": (1.69, 1.5),                                           # measured 0.841, 0.749
    "hs0.2": (2.2, 0.4),                                             # measured 1.100, 0.196
    "gates0.2": (0.49, 0.56),                                          # measured 0.242, 0.276
    "acts0.2": (0.61, 0.57),                                           # measured 0.303, 0.281
    "hs1.2": (2.86, 1.56),                                             # measured 1.429, 0.779
    "gates1.2": (1.79, 1.56),                                          # measured 0.894, 0.777
    "acts1.2": (2.17, 1.58),                                           # measured 1.082, 0.786
    "hs0.3": (1.39, 0.6),                                             # measured 0.691, 0.295
    "gates0.3": (1.01, 0.73),                                          # measured 0.503, 0.365
    "acts0.3": (0.87, 0.74),                                           # measured 0.432, 0.368
    "hs1.3": (2.44, 1.63),                                             # measured 1.218, 0.812
    "gates1.3": (1.96, 1.61),                                          # measured 0.979, 0.801
    "acts1.3": (2.23, 1.62),                                           # measured 1.110, 0.806
    "dcond": (0.94, 0.95),                                             # measured 0.465, 0.474
}
FRACS = {
    "hs0.0": 0.003,               # measured 0.0013
    "gates0.0": 0.008,            # measured 0.0037
    "acts0.0": 0.012,             # measured 0.0056
    "hs1.0": 0.605,               # measured 0.3022
    "gates1.0": 0.555,            # measured 0.2774
    "acts1.0": 0.865,             # measured 0.4320
    "hs0.1": 0.013,               # measured 0.0062
    "gates0.1": 0.057,            # measured 0.0282
    "acts0.1": 0.094,             # measured 0.0466
    "hs1.1": 0.789,               # measured 0.3943
    "gates1.1": 0.672,            # measured 0.3356
    "acts1.1": 1.003,             # measured 0.5010
    "hs0.2": 0.123,               # measured 0.0610
    "gates0.2": 0.235,            # measured 0.1171
    "acts0.2": 0.4,             # measured 0.1997
    "hs1.2": 0.936,               # measured 0.4676
    "gates1.2": 0.769,            # measured 0.3842
    "acts1.2": 1.127,             # measured 0.5631
    "hs0.3": 0.259,               # measured 0.1293
    "gates0.3": 0.339,            # measured 0.1695
    "acts0.3": 0.568,             # measured 0.2839
    "hs1.3": 1.049,               # measured 0.5243
    "gates1.3": 0.833,            # measured 0.4163
    "acts1.3": 1.191,             # measured 0.5952
}
# the bars that separate the contracted rounding points from any other bf16 scheme (see the docstring)
DISCRIMINATING = sorted(k for k, (a, b) in BARS.items() if a <= 0.75 and b <= 0.35)


if __name__ == "__main__":
    for k, (rm, rr, bad) in measure().items():
        print(f"{k}: max ratio {rm:.3f}  rms ratio {rr:.3f}  fraction off by more than 1e-6 {bad:.4f}")
