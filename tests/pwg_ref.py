"""torch restatement of the Parallel WaveGAN generator as DESIGN.md ("Neural vocoder") states it, written from that statement and not from the product
code: float64 by default, `dtype=torch.float32` runs the very same code in single precision on the CPU (the yardstick of the error bar).  One utterance
at a time: mel [A, L] and noise [T = L * hop] -> waveform [T].  Seeded noise comes from tests/prior_sample_ref.py's restatement of the counter hash
(integers bit for bit, the Gaussian in float64).  Shared by tests/test_pwg_cpu.py and tests/test_gpu_pwg.py."""
import hashlib
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prior_sample_ref as PS  # noqa: E402

DEFAULT = {"layers": 30, "stacks": 3, "R": 64, "G": 128, "S": 64, "A": 80, "ctx": 2, "scales": [4, 4, 4, 4]}
NARROW = {"layers": 4, "stacks": 2, "R": 32, "G": 64, "S": 32, "A": 20, "ctx": 2, "scales": [3, 5]}


def hop(cfg):
    return math.prod(cfg["scales"])


def dilation(cfg, i):
    return 2 ** (i % (cfg["layers"] // cfg["stacks"]))


def shapes(cfg):
    """state-dict key -> shape"""
    R, G, S, A, ctx = cfg["R"], cfg["G"], cfg["S"], cfg["A"], cfg["ctx"]
    e = {"first_conv.weight": (R, 1, 1), "first_conv.bias": (R,), "upsample_net.conv_in.weight": (A, A, 2 * ctx + 1)}
    for i, s in enumerate(cfg["scales"]):
        e["upsample_net.upsample.up_layers.{}.weight".format(2 * i + 1)] = (1, 1, 1, 2 * s + 1)
    for i in range(cfg["layers"]):
        q = "conv_layers.{}.".format(i)
        e[q + "conv.weight"], e[q + "conv.bias"] = (G, R, 3), (G,)
        e[q + "conv1x1_aux.weight"] = (G, A, 1)
        e[q + "conv1x1_out.weight"], e[q + "conv1x1_out.bias"] = (R, G // 2, 1), (R,)
        e[q + "conv1x1_skip.weight"], e[q + "conv1x1_skip.bias"] = (S, G // 2, 1), (S,)
    e["last_conv_layers.1.weight"], e["last_conv_layers.1.bias"] = (S, S, 1), (S,)
    e["last_conv_layers.3.weight"], e["last_conv_layers.3.bias"] = (1, S, 1), (1,)
    return e


def random_state_dict(cfg, seed):
    """torch's default Conv initialisation (uniform in +- 1 / sqrt(fan_in), weights and biases alike) under a fixed seed, from a private generator."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in shapes(cfg).items():
        if k.endswith(".weight"):
            bound = 1.0 / math.sqrt(int(np.prod(shape[1:])))
        else:
            bound = 1.0 / math.sqrt(int(np.prod(shapes(cfg)[k[:-len("bias")] + "weight"][1:])))
        sd[k] = (torch.rand(shape, generator=g) * 2.0 - 1.0) * bound
    return sd


def seeded_noise(s0, s1, T):
    """z[t] = gauss(s0, s1, 0, t, 1) in float64"""
    return torch.from_numpy(PS.gauss(s0, s1, 0, np.arange(T), 1))


def pwg_seed_words(seed, label, k=0):
    d = hashlib.blake2b("{}\0{}\0{}\0pwg".format(seed, label, k).encode()).digest()
    return int.from_bytes(d[:4], "little"), int.from_bytes(d[4:8], "little")


def condition(sd, cfg, mel, dtype=torch.float64):
    """mel [A, L] -> c [A, L * hop], by explicit index arithmetic"""
    m = mel.to(dtype)
    A, L = m.shape
    ctx = cfg["ctx"]
    w = sd["upsample_net.conv_in.weight"].to(dtype)                                          # [A, A, 2 ctx + 1]
    idx = (torch.arange(L)[:, None] + torch.arange(2 * ctx + 1)[None, :] - ctx).clamp(0, L - 1)  # replicate padding: the utterance's own first / last frame
    c = torch.einsum("oik,ilk->ol", w, m[:, idx])
    for i, s in enumerate(cfg["scales"]):
        fir = sd["upsample_net.upsample.up_layers.{}.weight".format(2 * i + 1)].to(dtype).reshape(-1)
        n = c.shape[1] * s
        rep = c[:, torch.arange(n) // s]                                                     # nearest neighbour
        pad = torch.zeros(A, n + 2 * s, dtype=dtype)
        pad[:, s:s + n] = rep
        c = sum(fir[j] * pad[:, j:j + n] for j in range(2 * s + 1))
    return c


def layer(sd, cfg, i, x, c, dtype=torch.float64):
    """x [R, T], c [A, T] -> (x', skip contribution [S, T])"""
    q, d = "conv_layers.{}.".format(i), dilation(cfg, i)
    t = lambda k: sd[q + k].to(dtype)
    x, c = x.to(dtype), c.to(dtype)
    h = F.conv1d(x[None], t("conv.weight"), t("conv.bias"), padding=d, dilation=d)[0] + F.conv1d(c[None], t("conv1x1_aux.weight"))[0]
    half = h.shape[0] // 2
    g = torch.tanh(h[:half]) * torch.sigmoid(h[half:])
    skip = F.conv1d(g[None], t("conv1x1_skip.weight"), t("conv1x1_skip.bias"))[0]
    xn = (F.conv1d(g[None], t("conv1x1_out.weight"), t("conv1x1_out.bias"))[0] + x) * math.sqrt(0.5)
    return xn, skip


def generator(sd, cfg, mel, noise, dtype=torch.float64):
    """mel [A, L], noise [L * hop] -> waveform [L * hop]"""
    c = condition(sd, cfg, mel, dtype)
    z = noise.to(dtype).reshape(1, 1, -1)
    assert z.shape[2] == c.shape[1]
    x = F.conv1d(z, sd["first_conv.weight"].to(dtype), sd["first_conv.bias"].to(dtype))[0]
    skips = 0
    for i in range(cfg["layers"]):
        x, s = layer(sd, cfg, i, x, c, dtype)
        skips = skips + s
    y = torch.relu(skips * math.sqrt(1.0 / cfg["layers"]))
    y = torch.relu(F.conv1d(y[None], sd["last_conv_layers.1.weight"].to(dtype), sd["last_conv_layers.1.bias"].to(dtype)))
    return F.conv1d(y, sd["last_conv_layers.3.weight"].to(dtype), sd["last_conv_layers.3.bias"].to(dtype))[0, 0]


def errors(got, ref64, ref32):
    """(err, e32): max |got - ref64| / max |ref64| and the same for the float32 run of the restatement"""
    scale = float(ref64.abs().max())
    return float((got.double() - ref64).abs().max()) / scale, float((ref32.double() - ref64).abs().max()) / scale


def uniform_mel(A, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(A, L, generator=g) * 8.0 - 4.0
