"""The arithmetic contract of the multi-period discriminator's bf16 mode in torch, written from DESIGN.md ("The multi-period discriminator in bf16") and not
from the product code.  The network is tests/hifigan_disc_ref.py's; every middle convolution convs.1 .. convs.{n-1} is a custom autograd function:

    forward   conv2d(bf16(act), bf16(W)) + b            act = lrelu(kept pre-activation): the rounding is of the ACTIVATED rows
    backward  d act = conv2d_input(bf16(W), bf16(dy))   dy as it arrives, with whatever the layers above and the feature matching injected
              d W   = conv2d_weight(bf16(act), bf16(dy))
              d b   = dy.sum()                          the UNROUNDED dy

bf16(.) rounds to nearest even and returns to the working dtype, so every product is exact in it and every sum is the working dtype's.  Layer 0 (from the
waveform) and conv_post stay plain convolutions.  The LeakyReLU, its mask from the unrounded pre-activation, the reflect pad and the fold are autograd's.
The same code runs in float64 (`emu64`: the contract) and in float32 (`emu32`: one float32 realisation of it, whose distance from emu64 is what a summation
order is worth).  `rounding=False` is the unrounded network: tests/test_hifigan_disc_bf16_cpu.py shows it equal to hifigan_disc_ref.score_grads.
Shared by tests/hifigan_disc_bf16_cases.py, the CPU test and the GPU tests."""
import torch
import torch.nn.functional as F

import hifigan_disc_ref as HR

STRIDE = HR.STRIDE


def bf16(t):
    """round to bf16, nearest even, back in t's dtype"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class MiddleConv(torch.autograd.Function):
    """One middle convolution under the contract: act [B, Cin, H, p], W [Cout, Cin, 5, 1], b [Cout] -> [B, Cout, H', p]"""

    @staticmethod
    def forward(ctx, act, W, b, stride, rounding):
        r = bf16 if rounding else (lambda t: t)
        ctx.save_for_backward(act, W)
        ctx.stride, ctx.r = int(stride), r
        return F.conv2d(r(act), r(W), None, stride=(int(stride), 1), padding=(2, 0)) + b.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, dy):
        act, W = ctx.saved_tensors
        r, s = ctx.r, (ctx.stride, 1)
        dyr = r(dy)
        dact = torch.nn.grad.conv2d_input(act.shape, r(W), dyr, stride=s, padding=(2, 0))
        dW = torch.nn.grad.conv2d_weight(r(act), W.shape, dyr, stride=s, padding=(2, 0))
        return dact, dW, dy.sum((0, 2, 3)), None, None


def middle_conv(act, W, b, stride, rounding=True):
    return MiddleConv.apply(act, W, b, stride, rounding)


def period_forward(sd, i, x, p, n, slope, rounding=True):
    """hifigan_disc_ref.period_forward with the middle convolutions under the contract"""
    B, T = x.shape
    if T % p:
        x = F.pad(x[:, None], (0, p - T % p), mode="reflect")[:, 0]
    h, maps = x.view(B, 1, -1, p), []
    for j in range(n):
        W, b, s = sd[f"discriminators.{i}.convs.{j}.weight"], sd[f"discriminators.{i}.convs.{j}.bias"], STRIDE if j < n - 1 else 1
        pre = F.conv2d(h, W, b, stride=(s, 1), padding=(2, 0)) if j == 0 else middle_conv(h, W, b, s, rounding)
        h = F.leaky_relu(pre, slope)
        maps.append(h)
    h = F.conv2d(h, sd[f"discriminators.{i}.conv_post.weight"], sd[f"discriminators.{i}.conv_post.bias"], padding=(1, 0))
    maps.append(h)
    return h.flatten(1), maps


def forward(sd, wav, periods, n, slope, rounding=True):
    return [period_forward(sd, i, wav, p, n, slope, rounding) for i, p in enumerate(periods)]


def _leaves(sd, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def score_grads(sd, wav, periods, n, slope, value, dtype=torch.float64, rounding=True):
    """hifigan_disc_ref.score_grads under the contract: L = sum over the periods of mean((D_p(wav) - value)^2) -> dict(scores, maps, loss, dwav, grads)"""
    w, x = _leaves(sd, dtype), wav.detach().to(dtype).clone().requires_grad_(True)
    out = forward(w, x, periods, n, slope, rounding)
    loss = sum(((s - value) ** 2).mean() for s, _ in out)
    loss.backward()
    return {"scores": [s.detach() for s, _ in out], "maps": [[m.detach() for m in maps] for _, maps in out], "loss": loss.detach().reshape(1),
            "dwav": x.grad.detach(), "grads": {k: v.grad.detach() for k, v in w.items()}}


def pair_grads(sd, real, fake, periods, n, slope, dtype=torch.float64, rounding=True):
    """hifigan_disc_ref.pair_grads under the contract, as `score_pair` computes it: ONE forward over [real; fake]"""
    w = _leaves(sd, dtype)
    B = real.shape[0]
    out = forward(w, torch.cat([real.detach(), fake.detach()]).to(dtype), periods, n, slope, rounding)
    rt, ft = [((s[:B] - 1) ** 2).mean() for s, _ in out], [(s[B:] ** 2).mean() for s, _ in out]
    loss = sum(rt) + sum(ft)
    loss.backward()
    return {"loss": loss.detach().reshape(1), "real_terms": torch.stack(rt).detach(), "fake_terms": torch.stack(ft).detach(),
            "both": [s.detach() for s, _ in out], "grads": {k: v.grad.detach() for k, v in w.items()}}


def generator_term_grads(sd, real, fake, periods, n, slope, lambda_adv, lambda_fm, dtype=torch.float64, rounding=True):
    """hifigan_disc_ref.generator_term_grads under the contract; the parameters and the real rows' maps are constants"""
    w = {k: v.detach().to(dtype) for k, v in sd.items()}
    f = fake.detach().to(dtype).clone().requires_grad_(True)
    out_r, out_f = forward(w, real.detach().to(dtype), periods, n, slope, rounding), forward(w, f, periods, n, slope, rounding)
    adv = torch.stack([((s - 1) ** 2).mean() for s, _ in out_f])
    fm = torch.stack([HR.feature_matching(mr, mf) for (_, mr), (_, mf) in zip(out_r, out_f)])
    loss = lambda_adv * adv.sum() + lambda_fm * fm.sum()
    loss.backward()
    return {"loss": loss.detach().reshape(1), "adv_terms": adv.detach(), "fm_terms": fm.detach(), "l_fm": fm.sum().detach().reshape(1),
            "p_fake": [s.detach() for s, _ in out_f], "dfake": f.grad.detach()}


# ---- one operator at a time, in the kernels' layouts: activations [B, H p, C] with the flat row h p + c ------------------------------------------------
def _folded(t, p):
    """[B, H p, C] -> [B, C, H, p]"""
    return t.reshape(t.shape[0], -1, p, t.shape[2]).permute(0, 3, 1, 2)


def _flat(t):
    """[B, C, H, p] -> [B, H p, C]"""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1])


def op_conv(x, W, b, p, stride, slope, dtype=torch.float64):
    """hifigan_disc_conv_bf16: x [B, H p, Cin] kept pre-activations -> [B, H' p, Cout]"""
    return _flat(middle_conv(F.leaky_relu(_folded(x.to(dtype), p), slope), W.to(dtype), b.to(dtype), stride))


def op_conv_bwd(dy, W, x, p, stride, slope, inj=None, inj_scale=0.0, dtype=torch.float64):
    """hifigan_disc_conv_bwd_bf16: dy [B, H' p, Cout], x [B, H p, Cin] -> sum * lrelu'(x) + inj * inj_scale"""
    xf, Wd = _folded(x.to(dtype), p), W.to(dtype)
    d = torch.nn.grad.conv2d_input(xf.shape, bf16(Wd), bf16(_folded(dy.to(dtype), p)), stride=(stride, 1), padding=(2, 0))
    d = _flat(d) * torch.where(x > 0, 1.0, slope).to(dtype)
    return d + inj.to(dtype) * inj_scale if inj is not None else d


def op_wgrad(x, dy, Wshape, p, stride, slope, dtype=torch.float64):
    """hifigan_disc_wgrad_bf16 -> (dW [Cout, Cin, 5, 1], db [Cout])"""
    act, d = F.leaky_relu(_folded(x.to(dtype), p), slope), _folded(dy.to(dtype), p)
    return torch.nn.grad.conv2d_weight(bf16(act), Wshape, bf16(d), stride=(stride, 1), padding=(2, 0)), d.sum((0, 2, 3))
