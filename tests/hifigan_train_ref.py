"""Gradients of the torch restatement tests/hifigan_ref.py under autograd: the yardstick of the HiFi-GAN generator's backward (csrc/hifigan_train_ops.hip).
float64 by default; `dtype=torch.float32` runs the very same code in single precision on the CPU, which gives e32 of the error bar
max |hip - ref64| / max |ref64| <= 4 e32 + 1e-6 (guards 0 < e32 < 1e-3, max |ref64| > 1e-3).  Shared by tests/test_hifigan_train_cpu.py,
tests/test_gpu_hifigan_train.py and tests/test_gpu_hifigan_trainer.py."""
import torch

import hifigan_ref as H


def generator_grads(sd, cfg, mels, functionals, dtype=torch.float64):
    """mels: list of [A, L_b]; functionals: list of f_b [L_b * hop].  The loss is sum_b <f_b, wav_b> -> (list of waveforms, {key: gradient}) in `dtype`."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    wavs = [H.generator(leaves, cfg, mel, dtype)[0] for mel in mels]
    loss = sum((f.to(dtype) * w).sum() for f, w in zip(functionals, wavs))
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return [w.detach() for w in wavs], dict(zip(leaves, grads))


def conv_grads(xs, w, b, dys, dilation, slope, dtype=torch.float64):
    """Gradients of sum_b <dy_b, H.conv(x_b)> for rows x_b [T_b, Cin], dy_b [T_b, Cout] -> ([dx_b [T_b, Cin]], dw, db)"""
    w, b = w.detach().to(dtype).requires_grad_(True), b.detach().to(dtype).requires_grad_(True)
    xs = [x.detach().to(dtype).requires_grad_(True) for x in xs]
    loss = sum((dy.to(dtype).T * H.conv(x.T, w, b, dilation, slope)).sum() for x, dy in zip(xs, dys))
    g = torch.autograd.grad(loss, xs + [w, b])
    return list(g[:len(xs)]), g[-2], g[-1]


def upsample_grads(xs, w, b, dys, u, dtype=torch.float64):
    """Gradients of sum_b <dy_b, H.upsample(x_b)> for rows x_b [T_b, Cin], dy_b [u T_b, Cout] -> ([dx_b], dw, db)"""
    w, b = w.detach().to(dtype).requires_grad_(True), b.detach().to(dtype).requires_grad_(True)
    xs = [x.detach().to(dtype).requires_grad_(True) for x in xs]
    loss = sum((dy.to(dtype).T * H.upsample(x.T, w, b, u)).sum() for x, dy in zip(xs, dys))
    g = torch.autograd.grad(loss, xs + [w, b])
    return list(g[:len(xs)]), g[-2], g[-1]


def check(tag, got, ref64, ref32):
    """Prints the figures, then asserts the guards and the bar; -> err / e32"""
    err, e32 = H.errors(got.detach().cpu(), ref64, ref32)
    print(f"{tag}: err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}  max|ref| {float(ref64.abs().max()):.3e}")
    assert 0 < e32 < 1e-3 and float(ref64.abs().max()) > 1e-3, "degenerate case: " + tag
    assert err <= 4 * e32 + 1e-6, tag
    return err / e32
