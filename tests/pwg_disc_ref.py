"""Reference of the Parallel WaveGAN discriminator and the least-squares adversarial losses, written from DESIGN.md ("Training the Parallel WaveGAN
discriminator") and not from the product code: `F.conv1d` + `leaky_relu` over a state dict in a given dtype.  float64 by default; the same code in float32 on
the CPU is the yardstick of the error bar (`pwg_train_ref.check`, unchanged).  `kernel_form_backward`: a float64 numpy restatement of the backward in the
shape the kernels compute it - the LeakyReLU mask read from a layer's OUTPUT, the data gradient as a gather of dpre(t + d) | dpre(t) | dpre(t - d) against
the transposed taps, the weight gradients as row products with a shift per tap - with two switches that break it one way each.  Shared by
tests/test_pwg_disc_cpu.py, tests/test_gpu_pwg_disc.py and tests/test_gpu_pwg_gan_trainer.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def shapes(layers, C):
    e = {}
    for i in range(layers):
        e["conv_layers.{}.weight".format(i)] = (1 if i == layers - 1 else C, 1 if i == 0 else C, 3)
        e["conv_layers.{}.bias".format(i)] = (1 if i == layers - 1 else C,)
    return e


def dilation(layers, i):
    return 1 if i == 0 or i == layers - 1 else i


def random_state_dict(layers, C, seed, scale=1.0):
    """torch.nn.Conv1d's default rule (uniform in +- 1 / sqrt(fan_in)) in name order on a seeded host generator, times `scale`"""
    g, sh, sd = torch.Generator().manual_seed(seed), shapes(layers, C), {}
    for k, s in sh.items():
        fan_in = math.prod(sh[k.rsplit(".", 1)[0] + ".weight"][1:])
        sd[k] = (torch.rand(s, generator=g, dtype=torch.float32) * 2.0 - 1.0) / math.sqrt(fan_in) * scale
    return sd


def discriminator(sd, wav, slope=0.2, dtype=torch.float64, hidden=None):
    """wav [B, T] -> scores [B, T]; `hidden` (a list) receives every layer's output [B, C, T]"""
    layers = len(sd) // 2
    x = wav.to(dtype).unsqueeze(1)
    for i in range(layers):
        d = dilation(layers, i)
        x = F.conv1d(x, sd["conv_layers.{}.weight".format(i)].to(dtype), sd["conv_layers.{}.bias".format(i)].to(dtype), padding=d, dilation=d)
        if i < layers - 1:
            x = F.leaky_relu(x, slope)
        if hidden is not None:
            hidden.append(x)
    return x.squeeze(1)


def mse(scores, value):
    return ((scores - value) ** 2).mean()


def adversarial_loss(p_fake):
    """L_adv = mean((D(G(z)) - 1)^2)"""
    return mse(p_fake, 1.0)


def discriminator_loss(p_real, p_fake):
    """L_D = mean((D(y) - 1)^2) + mean(D(G(z))^2)"""
    return mse(p_real, 1.0) + mse(p_fake, 0.0)


def score_grads(sd, wav, value, slope=0.2, dtype=torch.float64, factor=1.0):
    """One backward of factor * mean((D(wav) - value)^2) -> dict(scores, loss (unscaled), dwav, grads {key: gradient})"""
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = wav.detach().to(dtype).clone().requires_grad_(True)
    p = discriminator(params, x, slope, dtype)
    loss = mse(p, value)
    (loss * factor).backward()
    return {"scores": p.detach(), "loss": loss.detach().reshape(1), "dwav": x.grad.detach(), "grads": {k: t.grad.detach() for k, t in params.items()}}


def functional_grads(sd, wav, dscores, slope=0.2, dtype=torch.float64):
    """One backward of <dscores, D(wav)> -> dict(scores, dwav, grads)"""
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = wav.detach().to(dtype).clone().requires_grad_(True)
    p = discriminator(params, x, slope, dtype)
    (p * dscores.to(dtype)).sum().backward()
    return {"scores": p.detach(), "dwav": x.grad.detach(), "grads": {k: t.grad.detach() for k, t in params.items()}}


def pair_grads(sd, real, fake, slope=0.2, dtype=torch.float64):
    """L_D on (real, fake): -> dict(loss, terms [2], grads)"""
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    pr, pf = discriminator(params, real, slope, dtype), discriminator(params, fake, slope, dtype)
    loss = discriminator_loss(pr, pf)
    loss.backward()
    return {"loss": loss.detach().reshape(1), "terms": torch.stack([mse(pr, 1.0), mse(pf, 0.0)]).detach(), "grads": {k: t.grad.detach() for k, t in params.items()}}


# ---- the kernels' form, float64 numpy --------------------------------------------------------------------------------------------------------
def shifted(a, s):
    """a [T, C] -> rows a[t + s], zero outside [0, T)"""
    T = a.shape[0]
    out = np.zeros_like(a)
    lo, hi = max(0, -s), min(T, T - s)
    if lo < hi:
        out[lo:hi] = a[lo + s:hi + s]
    return out


def kernel_form_backward(sd, wav, dscores, slope=0.2, mask_from_input=False, same_side_gather=False):
    """sd: float64 numpy arrays in torch's layout, wav [T], dscores [T] (ONE batch row) -> (scores, d wav, {key: gradient}) in the kernels' form.  The
    switches each break it: the mask is read from the layer's input in place of its output, the backward gathers from the forward's side (t - d for the
    first tap)."""
    layers = len(sd) // 2
    W = lambda i: sd["conv_layers.{}.weight".format(i)]
    bias = lambda i: sd["conv_layers.{}.bias".format(i)]
    lrelu = lambda v: np.where(v > 0, v, v * slope)
    outs, x = [], wav[:, None]
    for i in range(layers):                                                               # forward, rows [T, C]
        d = dilation(layers, i)
        rows = np.concatenate([shifted(x, (j - 1) * d) for j in range(3)], axis=1)        # [x(t - d) | x(t) | x(t + d)]
        image = W(i).transpose(2, 1, 0).reshape(-1, W(i).shape[0])                        # row = tap * Cin + input channel
        x = rows @ image + bias(i)[None, :]
        if i < layers - 1:
            x = lrelu(x)
        outs.append(x)
    grads, dout = {}, dscores[:, None]
    for i in reversed(range(layers)):
        d, xin = dilation(layers, i), (outs[i - 1] if i > 0 else wav[:, None])
        if i == layers - 1:
            dpre = dout
        else:
            carrier = xin if mask_from_input and xin.shape == dout.shape else outs[i]
            dpre = dout * np.where(carrier > 0, 1.0, slope)
        seen = dpre
        sign = 1 if same_side_gather else -1
        rows = np.concatenate([shifted(seen, sign * (j - 1) * d) for j in range(3)], axis=1)   # [dpre(t + d) | dpre(t) | dpre(t - d)]
        image_t = W(i).transpose(2, 0, 1).reshape(-1, W(i).shape[1])                      # row = tap * Cout + output channel
        grads["conv_layers.{}.weight".format(i)] = np.stack([shifted(xin, (j - 1) * d).T @ dpre for j in range(3)], axis=0).transpose(2, 1, 0)
        grads["conv_layers.{}.bias".format(i)] = dpre.sum(0)
        dout = rows @ image_t
    return outs[-1][:, 0], dout[:, 0], grads
