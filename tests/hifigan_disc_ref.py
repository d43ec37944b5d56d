"""References of the HiFi-GAN multi-period discriminator, written from DESIGN.md ("Training the HiFi-GAN discriminator") and not from the product code.

`forward` / `score_grads` / `pair_grads` / `generator_term_grads`: the network exactly as the contract states it - F.pad(reflect) on the right to a multiple
of the period, .view(B, 1, -1, p), F.conv2d with kernels (5, 1) / (3, 1), leaky_relu, autograd; float64 by default, the same code in float32 on the CPU is
the yardstick of the error bar.  `kernel_form_backward`: a float64 numpy restatement of ONE period's backward in the shape the kernels compute it - the
polyphase data gradient of the strided convolutions (input row h takes tap m from output row (h + 2 - m) / s where s divides), the LeakyReLU mask from the
kept PRE-activation, the reflect fold as a gather, the strided weight-gradient sum - with switches that break it one way each
(tests/test_hifigan_disc_cpu.py shows each rejected).  Shared by tests/test_hifigan_disc_cpu.py and the GPU tests."""
import numpy as np
import torch
import torch.nn.functional as F

STRIDE, TAPS, POST_TAPS = 3, 5, 3
BROKEN = ("phase", "mask", "fold", "wgrad_stride")


def shapes(periods, channels):
    e = {}
    for i in range(len(periods)):
        cin = 1
        for j, c in enumerate(channels):
            e[f"discriminators.{i}.convs.{j}.weight"], e[f"discriminators.{i}.convs.{j}.bias"] = (c, cin, TAPS, 1), (c,)
            cin = c
        e[f"discriminators.{i}.conv_post.weight"], e[f"discriminators.{i}.conv_post.bias"] = (1, cin, POST_TAPS, 1), (1,)
    return e


def random_state_dict(periods, channels, seed, scale=1.0):
    """uniform in +- scale / sqrt(fan_in), weights and biases alike (torch's default rule times `scale`)"""
    g, sd, e = torch.Generator().manual_seed(seed), {}, shapes(periods, channels)
    for k, shape in e.items():
        fan_in = int(np.prod(e[k.replace(".bias", ".weight")][1:]))
        sd[k] = (torch.rand(shape, generator=g, dtype=torch.float32) * 2.0 - 1.0) / np.sqrt(fan_in) * scale
    return sd


def period_forward(sd, i, x, p, n, slope):
    """x [B, T] -> (scores [B, H_last p], the n + 1 feature maps [B, C, H, p]: the activated outputs, then conv_post's)"""
    B, T = x.shape
    if T % p:
        x = F.pad(x[:, None], (0, p - T % p), mode="reflect")[:, 0]
    h, maps = x.view(B, 1, -1, p), []
    for j in range(n):
        h = F.leaky_relu(F.conv2d(h, sd[f"discriminators.{i}.convs.{j}.weight"], sd[f"discriminators.{i}.convs.{j}.bias"], stride=(STRIDE if j < n - 1 else 1, 1),
                                  padding=(2, 0)), slope)
        maps.append(h)
    h = F.conv2d(h, sd[f"discriminators.{i}.conv_post.weight"], sd[f"discriminators.{i}.conv_post.bias"], padding=(1, 0))
    maps.append(h)
    return h.flatten(1), maps


def forward(sd, wav, periods, n, slope):
    """-> [(scores, maps) per period]"""
    return [period_forward(sd, i, wav, p, n, slope) for i, p in enumerate(periods)]


def _leaves(sd, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def score_grads(sd, wav, periods, n, slope, value, dtype=torch.float64):
    """L = sum over the periods of mean((D_p(wav) - value)^2) -> dict(scores, maps, loss [1], dwav, grads) by autograd"""
    w, x = _leaves(sd, dtype), wav.detach().to(dtype).clone().requires_grad_(True)
    out = forward(w, x, periods, n, slope)
    loss = sum(((s - value) ** 2).mean() for s, _ in out)
    loss.backward()
    return {"scores": [s.detach() for s, _ in out], "maps": [[m.detach() for m in maps] for _, maps in out], "loss": loss.detach().reshape(1),
            "dwav": x.grad.detach(), "grads": {k: v.grad.detach() for k, v in w.items()}}


def pair_grads(sd, real, fake, periods, n, slope, dtype=torch.float64):
    """L_D = sum_p [mean((D_p(real) - 1)^2) + mean(D_p(fake.detach())^2)] -> dict(loss [1], real_terms, fake_terms, grads, dfake: None - it does not reach it)"""
    w, f = _leaves(sd, dtype), fake.detach().to(dtype).clone().requires_grad_(True)
    out_r, out_f = forward(w, real.detach().to(dtype), periods, n, slope), forward(w, f.detach(), periods, n, slope)
    rt, ft = [((s - 1) ** 2).mean() for s, _ in out_r], [(s ** 2).mean() for s, _ in out_f]
    loss = sum(rt) + sum(ft)
    loss.backward()
    return {"loss": loss.detach().reshape(1), "real_terms": torch.stack(rt).detach(), "fake_terms": torch.stack(ft).detach(),
            "grads": {k: v.grad.detach() for k, v in w.items()}, "dfake": f.grad}


def feature_matching(maps_real, maps_fake):
    """-> terms [n + 1]: mean |real map - fake map|, the real maps constants"""
    return torch.stack([(r.detach() - f).abs().mean() for r, f in zip(maps_real, maps_fake)])


def generator_term_grads(sd, real, fake, periods, n, slope, lambda_adv, lambda_fm, dtype=torch.float64):
    """L = lambda_adv sum_p mean((D_p(fake) - 1)^2) + lambda_fm sum_p sum_maps mean |map_real - map_fake| -> dict(loss [1], adv_terms [periods], fm_terms
    [periods, n + 1], l_fm [1], dfake); the parameters are constants"""
    w = {k: v.detach().to(dtype) for k, v in sd.items()}
    f = fake.detach().to(dtype).clone().requires_grad_(True)
    out_r, out_f = forward(w, real.detach().to(dtype), periods, n, slope), forward(w, f, periods, n, slope)
    adv = torch.stack([((s - 1) ** 2).mean() for s, _ in out_f])
    fm = torch.stack([feature_matching(mr, mf) for (_, mr), (_, mf) in zip(out_r, out_f)])
    loss = lambda_adv * adv.sum() + lambda_fm * fm.sum()
    loss.backward()
    return {"loss": loss.detach().reshape(1), "adv_terms": adv.detach(), "fm_terms": fm.detach(), "l_fm": fm.sum().detach().reshape(1), "dfake": f.grad.detach()}


# ---- the kernels' form, float64 numpy --------------------------------------------------------------------------------------------------------
def _lrelu(v, slope):
    return np.where(v > 0, v, v * slope)


def kernel_form_backward(sd, i, wav, p, n, slope, dscores, broken=None):
    """One period's backward as the kernels compute it.  sd: the state dict; wav [B, T]; dscores [B, H_last p] -> (dwav [B, T], {name: gradient}), float64
    numpy.  Activations are [B][H][p][C]; what is kept are pre-activations.  broken: one of BROKEN - the data gradient with the wrong phase rule, no
    LeakyReLU mask, the reflect fold left out, the weight gradient blind to the stride."""
    assert broken in (None,) + BROKEN
    W = lambda name: sd[f"discriminators.{i}.{name}.weight"].double().numpy()[..., 0]          # [Cout, Cin, taps]
    bias = lambda name: sd[f"discriminators.{i}.{name}.bias"].double().numpy()
    x = wav.double().numpy()
    B, T = x.shape
    H0 = -(-T // p)
    idx = np.arange(H0 * p)
    a = x[:, np.where(idx < T, idx, 2 * T - 2 - idx)].reshape(B, H0, p, 1)                     # the padded, folded waveform: a gather
    strides = [STRIDE] * (n - 1) + [1]

    def taps_of(act, s, Hout, taps):                       # tap m of every output row: [taps][B, Hout, p, C], zero outside [0, H)
        pad = (taps - 1) // 2
        ap = np.pad(act, ((0, 0), (pad, pad), (0, 0), (0, 0)))
        return [ap[:, s * np.arange(Hout) + m] for m in range(taps)]

    acts, pres = [a], []                                   # acts[j]: the input of layer j (activated), pres[j]: its kept pre-activation output
    for j in range(n):
        H, s = acts[-1].shape[1], strides[j]
        Hout = (H - 1) // s + 1
        w = W(f"convs.{j}")
        pre = bias(f"convs.{j}") + sum(t @ w[:, :, m].T for m, t in enumerate(taps_of(acts[-1], s, Hout, TAPS)))
        pres.append(pre)
        acts.append(_lrelu(pre, slope))
    grads = {}
    H = acts[-1].shape[1]
    d = np.asarray(dscores, dtype=np.float64).reshape(B, H, p, 1)
    # conv_post: the weight gradient, then d pre of the last width
    w = W("conv_post")
    grads[f"discriminators.{i}.conv_post.weight"] = np.stack([np.einsum("bhpi,bhpo->oi", t, d) for t in taps_of(acts[-1], 1, H, POST_TAPS)], -1)[..., None]
    grads[f"discriminators.{i}.conv_post.bias"] = d.sum((0, 1, 2))
    dp = np.pad(d, ((0, 0), (1, 1), (0, 0), (0, 0)))
    da = sum(dp[:, np.arange(H) + 2 - m] @ w[:, :, m] for m in range(POST_TAPS))               # row h takes tap m from row h - (m - 1)
    for j in reversed(range(n)):
        mask = 1.0 if broken == "mask" else np.where(pres[j] > 0, 1.0, slope)
        d = da * mask                                      # d pre of layer j
        s, w, H = strides[j], W(f"convs.{j}"), acts[j].shape[1]
        Hout = d.shape[1]
        grads[f"discriminators.{i}.convs.{j}.weight"] = np.stack([np.einsum("bhpi,bhpo->oi", t, d)
                                                                  for t in taps_of(acts[j], 1 if broken == "wgrad_stride" else s, Hout, TAPS)], -1)[..., None]
        grads[f"discriminators.{i}.convs.{j}.bias"] = d.sum((0, 1, 2))
        da = np.zeros((B, H, p, w.shape[1]))
        hs = np.arange(H)
        for m in range(TAPS):                              # polyphase: input row h takes tap m from output row (h + 2 - m) / s where s divides
            t = hs + m - 2 if broken == "phase" else hs + 2 - m
            ok = (t >= 0) & (t % s == 0) & (t // s < Hout)
            da[:, hs[ok]] += d[:, (t // s)[ok]] @ w[:, :, m]
    dpad = da.reshape(B, H0 * p)
    t = np.arange(T)
    mirror = 2 * T - 2 - t
    dwav = dpad[:, :T].copy()
    if broken != "fold":
        ok = (mirror >= T) & (mirror < H0 * p)
        dwav[:, ok] += dpad[:, mirror[ok]]                 # the reflect pad folded back: a gather, no scatter
    return dwav, grads
