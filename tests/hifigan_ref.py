"""torch restatement of the HiFi-GAN generator as DESIGN.md ("HiFi-GAN generator") states it, written from that statement and not from the product code:
float64 by default, `dtype=torch.float32` runs the very same code in single precision on the CPU (the yardstick of the error bar).  One utterance at a
time: mel [A, L] -> waveform [L * hop]; rows are channels-first here ([C, T]), as torch's convolutions take them.  Shared by tests/test_hifigan_cpu.py
and tests/test_gpu_hifigan.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F

DEFAULT = {"A": 80, "C0": 512, "rates": [8, 8, 2, 2], "kernels": [16, 16, 4, 4], "resblock": "1", "rk": [3, 7, 11], "rd": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}
NARROW = {"A": 8, "C0": 64, "rates": [2, 2], "kernels": [4, 4], "resblock": "2", "rk": [3, 5], "rd": [[1, 3], [1, 3]]}
ODD = {"A": 12, "C0": 64, "rates": [3, 5], "kernels": [7, 11], "resblock": "1", "rk": [3, 7, 11], "rd": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}   # u does not divide k
SLOPE, LAST_SLOPE = 0.1, 0.01


def hop(cfg):
    return math.prod(cfg["rates"])


def channels(cfg, i):
    """the width after stage i (i = -1: after conv_pre)"""
    return cfg["C0"] // 2 ** (i + 1)


def shapes(cfg):
    """state-dict key -> shape"""
    e = {"conv_pre.weight": (cfg["C0"], cfg["A"], 7), "conv_pre.bias": (cfg["C0"],)}
    nk = len(cfg["rk"])
    for i, k in enumerate(cfg["kernels"]):
        c = channels(cfg, i)
        e["ups.{}.weight".format(i)], e["ups.{}.bias".format(i)] = (channels(cfg, i - 1), c, k), (c,)
        for j, rk in enumerate(cfg["rk"]):
            for m in range(len(cfg["rd"][j])):
                for convs in (["convs1", "convs2"] if cfg["resblock"] == "1" else ["convs1"]):
                    q = "resblocks.{}.{}.{}.".format(i * nk + j, convs, m)
                    e[q + "weight"], e[q + "bias"] = (c, c, rk), (c,)
    e["conv_post.weight"], e["conv_post.bias"] = (1, channels(cfg, len(cfg["rates"]) - 1), 7), (1,)
    return e


def random_state_dict(cfg, seed):
    """torch's default Conv initialisation (uniform in +- 1 / sqrt(fan_in), weights and biases alike; fan_in = shape[1] * taps, for the transposed
    convolutions too) under a fixed seed, from a private generator."""
    g = torch.Generator().manual_seed(seed)
    sd, sh = {}, shapes(cfg)
    for k, shape in sh.items():
        wshape = shape if k.endswith(".weight") else sh[k[:-len("bias")] + "weight"]
        sd[k] = (torch.rand(shape, generator=g) * 2.0 - 1.0) / math.sqrt(int(np.prod(wshape[1:])))
    return sd


def conv(x, w, b, dilation=1, slope=None):
    """x [Cin, T] -> [Cout, T]: LeakyReLU(slope) (None: none), then the zero-padded dilated convolution."""
    if slope is not None:
        x = F.leaky_relu(x, slope)
    return F.conv1d(x[None], w.to(x.dtype), b.to(x.dtype), padding=(w.shape[2] - 1) // 2 * dilation, dilation=dilation)[0]


def upsample(x, w, b, u, slope=SLOPE):
    """x [Cin, T] -> [Cout, u T]: LeakyReLU, then by explicit index arithmetic the transposed convolution of stride u and padding p = (k - u) / 2:
    out[t] = sum over the taps j with (t + p - j) % u == 0 of w[:, :, j]^T x[(t + p - j) / u], zero outside [0, T)."""
    x = F.leaky_relu(x, slope)
    w = w.to(x.dtype)
    Cin, T = x.shape
    k = w.shape[2]
    p = (k - u) // 2
    assert k >= u and (k - u) % 2 == 0
    out = b.to(x.dtype)[:, None].repeat(1, u * T)
    t = torch.arange(u * T)
    for j in range(k):
        n = t + p - j
        ok = (n % u == 0) & (n >= 0) & (n < u * T)
        src = torch.div(n[ok], u, rounding_mode="floor")
        out[:, t[ok]] += w[:, :, j].T @ x[:, src]
    return out


def resblock(sd, cfg, n, x):
    """Resblock n (kernel rk_j, dilations D_j with j = n % nk) on x [c, T]"""
    j = n % len(cfg["rk"])
    t = lambda k: sd["resblocks.{}.{}".format(n, k)]
    for m, d in enumerate(cfg["rd"][j]):
        y = conv(x, t("convs1.{}.weight".format(m)), t("convs1.{}.bias".format(m)), d, SLOPE)
        if cfg["resblock"] == "1":
            y = conv(y, t("convs2.{}.weight".format(m)), t("convs2.{}.bias".format(m)), 1, SLOPE)
        x = y + x
    return x


def stage(sd, cfg, i, x):
    """Stage i on x [c_{i-1}, T] -> [c_i, u_i T]: LeakyReLU + transposed convolution, then the mean of the nk resblocks"""
    nk = len(cfg["rk"])
    x = upsample(x, sd["ups.{}.weight".format(i)], sd["ups.{}.bias".format(i)], cfg["rates"][i])
    xs = None
    for j in range(nk):
        r = resblock(sd, cfg, i * nk + j, x)
        xs = r if xs is None else xs + r
    return xs / nk


def generator(sd, cfg, mel, dtype=torch.float64):
    """mel [A, L] -> (waveform [L * hop], the rows entering conv_post [c_last, L * hop])"""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = conv(mel.to(dtype), sd["conv_pre.weight"], sd["conv_pre.bias"])
    for i in range(len(cfg["rates"])):
        x = stage(sd, cfg, i, x)
    y = torch.tanh(conv(x, sd["conv_post.weight"], sd["conv_post.bias"], 1, LAST_SLOPE))
    return y[0], x


def errors(got, ref64, ref32):
    """(err, e32): max |got - ref64| / max |ref64| and the same for the float32 run of the restatement"""
    scale = float(ref64.abs().max())
    return float((got.double() - ref64).abs().max()) / scale, float((ref32.double() - ref64).abs().max()) / scale


def uniform_mel(A, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(A, L, generator=g) * 8.0 - 4.0
