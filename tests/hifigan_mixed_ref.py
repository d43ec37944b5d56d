"""torch restatement of the HiFi-GAN generator's mixed-precision training mode as DESIGN.md ("Training the HiFi-GAN generator: mixed precision") states it,
built on tests/hifigan_f16_ref.py and written from that statement, not from the product code.  One utterance at a time, rows channels-first ([C, T]).

THE CONTRACT.  The forward is the fp16 inference mode's rounded operator, imported from hifigan_f16_ref (`Emu.conv`, `Emu.upsample`): the same values, bit
for bit.  The backward of a convolution and of a transposed convolution is a `torch.autograd.Function`:
  data gradient    sum over taps and channels of bf16(dy) bf16(W), then * lrelu'(x) * scale - dy as it arrives, BEFORE any scale; the mask from the function's
                   own x (x > 0 ? 1 : slope, the slope at x == 0);
  weight gradient  sum over rows of bf16(lrelu(x)) bf16(dy), then * scale - lrelu in float32 on the float32 row, as the forward stages it;
  bias gradient    the column sum of the UNROUNDED dy, then * scale.
bf16 rounding is `.to(torch.bfloat16)`: nearest even, no clamp.  conv_post + tanh stay hifigan_ref's, unrounded, forward and backward.
`scale` is the 1 / nk of the MRF mean: the kernels round the stage's output gradient d acc itself and multiply the products by 1 / nk afterwards (bf16 rounding
does not commute with a division by 3).  So the mean's backward (`_Mean`) hands every block the UNSCALED d acc, the last step of a block multiplies what it
computes from it by 1 / nk (`scale` of its last convolution; `_scale_grad` on its skip branch, in the working precision), and everything before the last step
sees scaled gradients, as in the kernels' plan.  The whole generator's gradient under a given d wav then falls out of autograd.

Three realisations, as for f16:  emu64 = Emu(torch.float64);  emu32 = Emu(torch.float32): float32 sums in torch's order;  emu32b = Emu(torch.float32,
blocked=True): float32 sums in the kernels' order - the data gradient per (64-channel chunk of dy, tap) one partial sum from zero, added chunk by chunk and tap
by tap; the weight gradient per 64-row tile one partial sum from zero, the tiles added in ascending order (an utterance is one call here, so the order of the
splits ACROSS utterances is autograd's)."""
import torch
import torch.nn.functional as F

import hifigan_f16_ref as R
import hifigan_ref as H

CHUNK, TILE = 64, 64


def rb(x):
    """round to bf16 (nearest even), back to x.dtype"""
    return x.to(torch.bfloat16).to(x.dtype)


def staged(x, slope):
    """lrelu(x) as the weight gradient stages it: the float32 row, LeakyReLU in float32 (slope None: none), bf16 - in x.dtype"""
    v = x.to(torch.float32)
    if slope is not None:
        v = torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32))
    return v.to(torch.bfloat16).to(x.dtype)


def mask(x, slope):
    """lrelu'(x): 1 where x > 0, the (float32) slope elsewhere, at x == 0 as well"""
    if slope is None:
        return torch.ones_like(x)
    return torch.where(x > 0, torch.ones_like(x), torch.tensor(slope, dtype=torch.float32).to(x.dtype) * torch.ones_like(x))


class _Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emu, x, w, b, dilation, slope, scale):
        ctx.emu, ctx.args = emu, (dilation, slope, scale)
        ctx.save_for_backward(x, w)
        return R.Emu.conv(emu, x, w, b, dilation, slope)

    @staticmethod
    def backward(ctx, dy):
        (x, w), (d, slope, scale), dt, blocked = ctx.saved_tensors, ctx.args, ctx.emu.dtype, ctx.emu.blocked
        dy = dy.to(dt)
        dyb, wb, xr = rb(dy), rb(w.to(torch.float32)).to(dt), staged(x.to(dt), slope)
        Cout, Cin, taps = w.shape
        T, pad = x.shape[1], (taps - 1) // 2 * d
        dyp, xp = F.pad(dyb, (pad, pad)), F.pad(xr, (pad, pad))
        # y[t] = sum_j W_j x[t - pad + j d]  =>  dx[s] = sum_j W_j^T dy[s + pad - j d]; the kernel's tap m reads dy[s - pad + m d]: j = taps - 1 - m
        if blocked:
            dx = torch.zeros(Cin, T, dtype=dt)
            for c0 in range(0, Cout, CHUNK):
                for m in range(taps):
                    dx = dx + wb[c0:c0 + CHUNK, :, taps - 1 - m].T @ dyp[c0:c0 + CHUNK, m * d:m * d + T]
        else:
            dx = F.conv_transpose1d(dyb[None], wb, padding=pad, dilation=d)[0]
        dx = dx * mask(x.to(dt), slope) * scale
        dw = torch.zeros(Cout, Cin, taps, dtype=dt)
        for j in range(taps):
            xs = xp[:, j * d:j * d + T]
            if blocked:
                for t0 in range(0, T, TILE):
                    dw[:, :, j] = dw[:, :, j] + dyb[:, t0:t0 + TILE] @ xs[:, t0:t0 + TILE].T
            else:
                dw[:, :, j] = dyb @ xs.T
        return None, dx, dw * scale, dy.sum(1) * scale, None, None, None


class _Upsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emu, x, w, b, u, slope):
        ctx.emu, ctx.args = emu, (u, slope)
        ctx.save_for_backward(x, w)
        return R.Emu.upsample(emu, x, w, b, u, slope)

    @staticmethod
    def backward(ctx, dy):
        (x, w), (u, slope), dt, blocked = ctx.saved_tensors, ctx.args, ctx.emu.dtype, ctx.emu.blocked
        dy = dy.to(dt)
        dyb, wb, xr = rb(dy), rb(w.to(torch.float32)).to(dt), staged(x.to(dt), slope)
        Cin, Cout, k = w.shape
        T, p = x.shape[1], (k - u) // 2
        t = torch.arange(u * T)
        dx, dw = torch.zeros(Cin, T, dtype=dt), torch.zeros(Cin, Cout, k, dtype=dt)
        for j in range(k):                                                   # out[t] += W_j^T x[(t + p - j) / u] where u divides t + p - j
            n = t + p - j
            ok = (n % u == 0) & (n >= 0) & (n < u * T)
            src, tt = torch.div(n[ok], u, rounding_mode="floor"), t[ok]
            dx[:, src] += wb[:, :, j] @ dyb[:, tt]                           # (for one tap the source rows are distinct)
            if blocked:
                for t0 in range(0, len(tt), TILE):
                    dw[:, :, j] = dw[:, :, j] + xr[:, src[t0:t0 + TILE]] @ dyb[:, tt[t0:t0 + TILE]].T
            else:
                dw[:, :, j] = xr[:, src] @ dyb[:, tt].T
        return None, dx * mask(x.to(dt), slope), dw, dy.sum(1), None, None


class _Mean(torch.autograd.Function):
    """(r_0 + r_1 + ..) / nk as hifigan_f16_ref sums it; the backward hands every block the UNSCALED gradient (the blocks' last steps scale)"""

    @staticmethod
    def forward(ctx, *rs):
        ctx.n = len(rs)
        xs = None
        for r in rs:
            xs = r if xs is None else xs + r
        return xs / len(rs)

    @staticmethod
    def backward(ctx, g):
        return (g,) * ctx.n


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.scale, None


class Emu(R.Emu):
    """hifigan_f16_ref.Emu with the mixed mode's backward: `generator(sd, cfg, mel)` on leaves that require a gradient is differentiable"""

    def conv(self, x, w, b, dilation=1, slope=None, scale=1.0):
        return _Conv.apply(self, x, w, b, dilation, slope, scale)

    def upsample(self, x, w, b, u, slope=H.SLOPE):
        return _Upsample.apply(self, x, w, b, u, slope)

    def resblock(self, sd, cfg, n, x):
        """hifigan_f16_ref's resblock; the last step carries the 1 / nk of the mean in its backward"""
        nk = len(cfg["rk"])
        j = n % nk
        t = lambda k: sd["resblocks.{}.{}".format(n, k)]
        ds = cfg["rd"][j]
        for m, d in enumerate(ds):
            sc = 1.0 / nk if m == len(ds) - 1 else 1.0
            two = cfg["resblock"] == "1"
            y = self.conv(x, t("convs1.{}.weight".format(m)), t("convs1.{}.bias".format(m)), d, H.SLOPE, 1.0 if two else sc)
            if two:
                y = self.conv(y, t("convs2.{}.weight".format(m)), t("convs2.{}.bias".format(m)), 1, H.SLOPE, sc)
            x = y + (_ScaleGrad.apply(x, sc) if sc != 1.0 else x)
        return x

    def stage(self, sd, cfg, i, x):
        nk = len(cfg["rk"])
        x = self.upsample(x.to(self.dtype), sd["ups.{}.weight".format(i)], sd["ups.{}.bias".format(i)], cfg["rates"][i])
        return _Mean.apply(*[self.resblock(sd, cfg, i * nk + j, x) for j in range(nk)])


def emus(flush=False):
    """(emu64, emu32, emu32b)"""
    return Emu(torch.float64, False, flush), Emu(torch.float32, False, flush), Emu(torch.float32, True, flush)


def generator_grads(emu, sd, cfg, mels, functionals):
    """mels: list of [A, L_b]; functionals: list of d wav_b [L_b * hop].  The loss is sum_b <f_b, wav_b> -> (list of waveforms, {key: gradient}), in emu.dtype"""
    leaves = {k: v.detach().to(emu.dtype).clone().requires_grad_(True) for k, v in sd.items()}
    wavs = [emu.generator(leaves, cfg, mel)[0] for mel in mels]
    loss = sum((f.to(emu.dtype) * w).sum() for f, w in zip(functionals, wavs))
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return [w.detach() for w in wavs], {k: g.to(emu.dtype) for k, g in zip(leaves, grads)}


def conv_grads(emu, xs, w, b, dys, dilation, slope, scale=1.0):
    """The contract's gradients of one convolution for rows x_b [T_b, Cin] under dy_b [T_b, Cout] -> ([dx_b [T_b, Cin]], dw, db)"""
    w, b = w.detach().to(emu.dtype).clone().requires_grad_(True), b.detach().to(emu.dtype).clone().requires_grad_(True)
    xs = [x.detach().to(emu.dtype).clone().requires_grad_(True) for x in xs]
    loss = sum((dy.to(emu.dtype).T * emu.conv(x.T, w, b, dilation, slope, scale)).sum() for x, dy in zip(xs, dys))
    g = torch.autograd.grad(loss, xs + [w, b])
    return [t.to(emu.dtype) for t in g[:len(xs)]], g[-2].to(emu.dtype), g[-1].to(emu.dtype)


def upsample_grads(emu, xs, w, b, dys, u):
    """The same for the transposed convolution: x_b [T_b, Cin], dy_b [u T_b, Cout]"""
    w, b = w.detach().to(emu.dtype).clone().requires_grad_(True), b.detach().to(emu.dtype).clone().requires_grad_(True)
    xs = [x.detach().to(emu.dtype).clone().requires_grad_(True) for x in xs]
    loss = sum((dy.to(emu.dtype).T * emu.upsample(x.T, w, b, u)).sum() for x, dy in zip(xs, dys))
    g = torch.autograd.grad(loss, xs + [w, b])
    return [t.to(emu.dtype) for t in g[:len(xs)]], g[-2].to(emu.dtype), g[-1].to(emu.dtype)
