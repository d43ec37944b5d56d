"""Reference of the HiFi-GAN multi-scale discriminator, written from DESIGN.md ("The multi-scale discriminator") and not from the product code: the network
exactly as the contract states it - F.avg_pool1d(4, 2, padding 2) between the scales, F.conv1d(groups=) with zero padding k // 2, leaky_relu, autograd.
float64 by default; the same code in float32 on the CPU is the yardstick of the error bar.  Shared by tests/test_hifigan_msd_cpu.py and the GPU tests."""
import numpy as np
import torch
import torch.nn.functional as F

POST_TAPS = 3
DEFAULT = {"channels": [128, 128, 256, 512, 1024, 1024, 1024], "groups": [1, 4, 16, 16, 16, 16, 1], "strides": [1, 2, 2, 4, 4, 1, 1],
           "kernels": [15, 41, 41, 41, 41, 41, 5]}
NARROW = {"channels": [16, 32, 64, 32, 64], "groups": [1, 2, 4, 2, 1], "strides": [1, 2, 4, 1, 1], "kernels": [15, 41, 41, 41, 5]}


def shapes(scales, net):
    e = {}
    for i in range(scales):
        cin = 1
        for j, (c, g, k) in enumerate(zip(net["channels"], net["groups"], net["kernels"])):
            e[f"discriminators.{i}.convs.{j}.weight"], e[f"discriminators.{i}.convs.{j}.bias"] = (c, cin // g, k), (c,)
            cin = c
        e[f"discriminators.{i}.conv_post.weight"], e[f"discriminators.{i}.conv_post.bias"] = (1, cin, POST_TAPS), (1,)
    return e


def random_state_dict(scales, net, seed, scale=1.0):
    """uniform in +- scale / sqrt(fan_in), fan_in = (Cin / groups) k, weights and biases alike (torch's default rule times `scale`)"""
    g, sd, e = torch.Generator().manual_seed(seed), {}, shapes(scales, net)
    for k, shape in e.items():
        fan_in = int(np.prod(e[k.replace(".bias", ".weight")][1:]))
        sd[k] = (torch.rand(shape, generator=g, dtype=torch.float32) * 2.0 - 1.0) / np.sqrt(fan_in) * scale
    return sd


def scale_forward(sd, i, x, net, slope):
    """x [B, T_i] -> (scores [B, L_last], the n + 1 feature maps [B, C, L]: the activated outputs, then conv_post's)"""
    h, maps = x[:, None, :], []
    for j, (g, s, k) in enumerate(zip(net["groups"], net["strides"], net["kernels"])):
        h = F.leaky_relu(F.conv1d(h, sd[f"discriminators.{i}.convs.{j}.weight"], sd[f"discriminators.{i}.convs.{j}.bias"], stride=s, padding=k // 2, groups=g), slope)
        maps.append(h)
    h = F.conv1d(h, sd[f"discriminators.{i}.conv_post.weight"], sd[f"discriminators.{i}.conv_post.bias"], padding=POST_TAPS // 2)
    maps.append(h)
    return h.flatten(1), maps


def forward(sd, wav, scales, net, slope):
    """-> [(scores, maps) per scale]; scale i sees the waveform after i pools (zero padding counted: always divided by 4)"""
    out, x = [], wav
    for i in range(scales):
        if i:
            x = F.avg_pool1d(x[:, None, :], 4, 2, padding=2)[:, 0, :]
        out.append(scale_forward(sd, i, x, net, slope))
    return out


def _leaves(sd, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def score_grads(sd, wav, scales, net, slope, value, dtype=torch.float64):
    """L = sum over the scales of mean((D_i(wav) - value)^2) -> dict(scores, maps, loss [1], dwav, grads) by autograd"""
    w, x = _leaves(sd, dtype), wav.detach().to(dtype).clone().requires_grad_(True)
    out = forward(w, x, scales, net, slope)
    loss = sum(((s - value) ** 2).mean() for s, _ in out)
    loss.backward()
    return {"scores": [s.detach() for s, _ in out], "maps": [[m.detach() for m in maps] for _, maps in out], "loss": loss.detach().reshape(1),
            "dwav": x.grad.detach(), "grads": {k: v.grad.detach() for k, v in w.items()}}


def pair_grads(sd, real, fake, scales, net, slope, dtype=torch.float64):
    """L_D = sum_i [mean((D_i(real) - 1)^2) + mean(D_i(fake.detach())^2)] -> dict(loss [1], real_terms, fake_terms, both: scores over [real; fake] per scale, grads)"""
    w = _leaves(sd, dtype)
    out_r, out_f = forward(w, real.detach().to(dtype), scales, net, slope), forward(w, fake.detach().to(dtype), scales, net, slope)
    rt, ft = [((s - 1) ** 2).mean() for s, _ in out_r], [(s ** 2).mean() for s, _ in out_f]
    loss = sum(rt) + sum(ft)
    loss.backward()
    return {"loss": loss.detach().reshape(1), "real_terms": torch.stack(rt).detach(), "fake_terms": torch.stack(ft).detach(), "both": [torch.cat([r.detach(), f.detach()]) for (r, _), (f, _) in zip(out_r, out_f)],
            "grads": {k: v.grad.detach() for k, v in w.items()}}


def generator_term_grads(sd, real, fake, scales, net, slope, lambda_adv, lambda_fm, dtype=torch.float64):
    """L = lambda_adv sum_i mean((D_i(fake) - 1)^2) + lambda_fm sum_i sum_maps mean |map_real - map_fake| -> dict(loss [1], p_fake, adv_terms [scales],
    fm_terms [scales, n + 1], l_fm [1], dfake); the parameters and the real maps are constants"""
    w = {k: v.detach().to(dtype) for k, v in sd.items()}
    f = fake.detach().to(dtype).clone().requires_grad_(True)
    out_r, out_f = forward(w, real.detach().to(dtype), scales, net, slope), forward(w, f, scales, net, slope)
    adv = torch.stack([((s - 1) ** 2).mean() for s, _ in out_f])
    fm = torch.stack([torch.stack([(r.detach() - m).abs().mean() for r, m in zip(mr, mf)]) for (_, mr), (_, mf) in zip(out_r, out_f)])
    loss = lambda_adv * adv.sum() + lambda_fm * fm.sum()
    loss.backward()
    return {"loss": loss.detach().reshape(1), "p_fake": [s.detach() for s, _ in out_f], "adv_terms": adv.detach(), "fm_terms": fm.detach(),
            "l_fm": fm.sum().detach().reshape(1), "dfake": f.grad.detach()}
