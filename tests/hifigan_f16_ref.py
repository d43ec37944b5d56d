"""torch restatement of the HiFi-GAN generator's fp16 inference mode as DESIGN.md ("HiFi-GAN generator: fp16 inference mode") states it, built on
tests/hifigan_ref.py and written from that statement, not from the product code.  One utterance at a time, rows channels-first ([C, T]) as in hifigan_ref.

THE CONTRACT.  Only the convolutions and transposed convolutions change (conv_pre included; conv_post + tanh is hifigan_ref's, unrounded).  In them the
OPERANDS are rounded: the row as float32, LeakyReLU in float32 (x > 0 ? x : x * float32(slope)), clamped to +-65504, rounded to fp16 nearest even; the weight
clamped and rounded the same way.  fp16 x fp16 products are exact; the sums start at the bias, the residual adds the UNROUNDED row, the MRF sum and mean and
every tensor between two operators stay in the working precision.  `flush`: fp16 subnormal operands count as zero (what the hardware was found to do is
recorded in hifigan_f16_cases.FLUSH_SUBNORMALS).

Three realisations:  emu64 = Emu(torch.float64): the contract in float64 arithmetic;  emu32 = Emu(torch.float32): the same in float32 (torch's CPU
convolution's summation order);  emu32b = Emu(torch.float32, blocked=True): float32 with the sums taken as the kernel takes them - per (64-channel chunk, tap)
one partial sum from zero, the partial sums added to the bias-initialised sum chunk by chunk and tap by tap."""
import numpy as np
import torch
import torch.nn.functional as F

import hifigan_ref as H

F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14
CHUNK = 64


def r16(x, flush=False):
    """clamp to +-65504, round to fp16 (nearest even, numpy's direct conversion: no double rounding from float64), back to x.dtype"""
    y = x.clamp(-F16_MAX, F16_MAX).numpy().astype(np.float16)
    if flush:
        y = np.where(np.abs(y) < np.float16(F16_MIN_NORMAL), np.float16(0), y)
    return torch.from_numpy(y.astype(np.float64)).to(x.dtype)


def operand(x, slope, flush=False):
    """The staged row: float32, LeakyReLU in float32 (slope None: none), clamp, fp16 - returned in x.dtype"""
    v = x.to(torch.float32)
    if slope is not None:
        v = torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32))
    return r16(v, flush).to(x.dtype)


class Emu:
    def __init__(self, dtype=torch.float64, blocked=False, flush=False):
        self.dtype, self.blocked, self.flush = dtype, blocked, flush

    def conv(self, x, w, b, dilation=1, slope=None):
        """x [Cin, T] -> [Cout, T] in self.dtype"""
        dt = self.dtype
        xr, wr, b = operand(x.to(dt), slope, self.flush), r16(w.to(torch.float32), self.flush).to(dt), b.to(dt)
        taps, pad = w.shape[2], (w.shape[2] - 1) // 2 * dilation
        if not self.blocked:
            return F.conv1d(xr[None], wr, b, padding=pad, dilation=dilation)[0]
        T = x.shape[1]
        xp = F.pad(xr, (pad, pad))
        y = b[:, None].repeat(1, T)
        for c0 in range(0, x.shape[0], CHUNK):
            for j in range(taps):
                y = y + wr[:, c0:c0 + CHUNK, j] @ xp[c0:c0 + CHUNK, j * dilation:j * dilation + T]
        return y

    def upsample(self, x, w, b, u, slope=H.SLOPE):
        """x [Cin, T] -> [Cout, u T]: hifigan_ref.upsample's index arithmetic on the rounded operands; per output row the taps ascend, as the kernel's phases
        walk them"""
        dt = self.dtype
        xr, wr = operand(x.to(dt), slope, self.flush), r16(w.to(torch.float32), self.flush).to(dt)
        Cin, T = xr.shape
        k = w.shape[2]
        p = (k - u) // 2
        assert k >= u and (k - u) % 2 == 0
        out = b.to(dt)[:, None].repeat(1, u * T)
        t = torch.arange(u * T)
        for c0 in range(0, Cin, CHUNK if self.blocked else Cin):
            c1 = c0 + (CHUNK if self.blocked else Cin)
            for j in range(k):
                n = t + p - j
                ok = (n % u == 0) & (n >= 0) & (n < u * T)
                src = torch.div(n[ok], u, rounding_mode="floor")
                out[:, t[ok]] += wr[c0:c1, :, j].T @ xr[c0:c1][:, src]
        return out

    def resblock(self, sd, cfg, n, x):
        j = n % len(cfg["rk"])
        t = lambda k: sd["resblocks.{}.{}".format(n, k)]
        for m, d in enumerate(cfg["rd"][j]):
            y = self.conv(x, t("convs1.{}.weight".format(m)), t("convs1.{}.bias".format(m)), d, H.SLOPE)
            if cfg["resblock"] == "1":
                y = self.conv(y, t("convs2.{}.weight".format(m)), t("convs2.{}.bias".format(m)), 1, H.SLOPE)
            x = y + x                                                         # the unrounded row
        return x

    def stage(self, sd, cfg, i, x):
        nk = len(cfg["rk"])
        x = self.upsample(x.to(self.dtype), sd["ups.{}.weight".format(i)], sd["ups.{}.bias".format(i)], cfg["rates"][i])
        xs = None
        for j in range(nk):
            r = self.resblock(sd, cfg, i * nk + j, x)
            xs = r if xs is None else xs + r
        return xs / nk

    def generator(self, sd, cfg, mel):
        """mel [A, L] -> (waveform [L * hop], the rows entering conv_post [c_last, L * hop]); conv_post + tanh: hifigan_ref's, in self.dtype"""
        x = self.conv(mel.to(self.dtype), sd["conv_pre.weight"], sd["conv_pre.bias"])
        for i in range(len(cfg["rates"])):
            x = self.stage(sd, cfg, i, x)
        y = torch.tanh(H.conv(x, sd["conv_post.weight"].to(self.dtype), sd["conv_post.bias"].to(self.dtype), 1, H.LAST_SLOPE))
        return y[0], x


def emus(flush=False):
    """(emu64, emu32, emu32b)"""
    return Emu(torch.float64, False, flush), Emu(torch.float32, False, flush), Emu(torch.float32, True, flush)
