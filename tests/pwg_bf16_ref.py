"""torch restatement of the Parallel WaveGAN generator's bf16 inference mode as DESIGN.md ("Neural vocoder", "bf16 inference mode") states it: tests/pwg_ref.py
with the contract's rounding points, written from that statement and not from the kernel.  Inside a layer exactly these values are rounded to bf16 (nearest
even, `rb`): the gathered operand rows x(t - d), x(t), x(t + d), c(t); the four weight tensors conv / conv1x1_aux / conv1x1_out / conv1x1_skip; the gate
tanh(a) * sigmoid(b) before the second product.  Everything else is the dtype of the run: the sums and the biases, tanh / sigmoid, the residual (which adds the
UNROUNDED x), the skip sum, and all of the conditioning, first_conv and the head.

Three runs of the same statement:  emu64 (float64),  emu32 (float32),  emu32b (float32 with another summation order: the three taps and the aux 1x1 are four
separate products, added as ((tap0 + tap2) + tap1) + aux + bias).  The differences between them are what a correct implementation may differ by.
Shared by tests/test_pwg_bf16_cpu.py and tests/test_gpu_pwg_bf16.py."""
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pwg_ref as P  # noqa: E402

THIN = {"layers": 2, "stacks": 1, "R": 16, "G": 32, "S": 16, "A": 4, "ctx": 2, "scales": [3, 5]}       # GEMM 2 has K = 16, padded to 32
WIDE = {"layers": 2, "stacks": 1, "R": 96, "G": 192, "S": 48, "A": 36, "ctx": 2, "scales": [3, 5]}     # more column pairs than waves
VARIANTS = {"emu64": (torch.float64, False), "emu32": (torch.float32, False), "emu32b": (torch.float32, True)}


def rb(t):
    """round to bf16 (nearest even) and back"""
    return t.float().bfloat16().to(t.dtype)


def layer_emu(sd, cfg, i, x, c, variant="emu64"):
    """x [R, T], c [A, T] -> (x', skip contribution [S, T], the unrounded gate [R, T]) in the run `variant`"""
    dtype, split = VARIANTS[variant]
    q, d = "conv_layers.{}.".format(i), P.dilation(cfg, i)
    t = lambda k: sd[q + k].to(dtype)
    x, c = x.to(dtype), c.to(dtype)
    xr, cr, w, wa = rb(x), rb(c), rb(t("conv.weight")), rb(t("conv1x1_aux.weight"))
    if split:
        T = x.shape[1]
        pad = F.pad(xr, (d, d))
        tap = [F.conv1d(pad[None, :, j * d:j * d + T], w[:, :, j:j + 1])[0] for j in range(3)]
        h = ((tap[0] + tap[2]) + tap[1]) + F.conv1d(cr[None], wa)[0] + t("conv.bias")[:, None]
    else:
        h = F.conv1d(xr[None], w, t("conv.bias"), padding=d, dilation=d)[0] + F.conv1d(cr[None], wa)[0]
    half = h.shape[0] // 2
    gate = torch.tanh(h[:half]) * torch.sigmoid(h[half:])
    g = rb(gate)
    skip = F.conv1d(g[None], rb(t("conv1x1_skip.weight")), t("conv1x1_skip.bias"))[0]
    xn = (F.conv1d(g[None], rb(t("conv1x1_out.weight")), t("conv1x1_out.bias"))[0] + x) * math.sqrt(0.5)
    return xn, skip, gate


def generator_emu(sd, cfg, mel, noise, variant="emu64"):
    """mel [A, L], noise [L * hop] -> waveform [L * hop]: pwg_ref.generator with `layer_emu` for the layers"""
    dtype = VARIANTS[variant][0]
    c = P.condition(sd, cfg, mel, dtype)
    z = noise.to(dtype).reshape(1, 1, -1)
    assert z.shape[2] == c.shape[1]
    x = F.conv1d(z, sd["first_conv.weight"].to(dtype), sd["first_conv.bias"].to(dtype))[0]
    skips = 0
    for i in range(cfg["layers"]):
        x, s, _ = layer_emu(sd, cfg, i, x, c, variant)
        skips = skips + s
    y = torch.relu(skips * math.sqrt(1.0 / cfg["layers"]))
    y = torch.relu(F.conv1d(y[None], sd["last_conv_layers.1.weight"].to(dtype), sd["last_conv_layers.1.bias"].to(dtype)))
    return F.conv1d(y, sd["last_conv_layers.3.weight"].to(dtype), sd["last_conv_layers.3.bias"].to(dtype))[0, 0]
