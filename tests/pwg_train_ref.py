"""References of vocoder training, written from DESIGN.md ("STFT loss") and not from the product code.

`stft_loss`: the multi-resolution STFT loss with torch.stft, exactly as the contract states it; float64 by default, the same code in float32 on the CPU is
the yardstick of the error bar.  `kernel_form_grad`: a float64 numpy restatement of the loss's closed-form gradient in the shape the kernels compute it -
dL/d|X| in closed form, times X / |X| (zero where the clamp is active), the transposed real DFT per frame, the window, the overlap-add as a GATHER over the
ceil(win / hop) frames that cover a padded position, the reflect padding folded back - with switches that break it one way each (tests/test_pwg_train_cpu.py
shows each rejected).  Shared by tests/test_pwg_train_cpu.py and tests/test_gpu_stft_loss.py."""
import numpy as np
import torch

RESOLUTIONS = [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)]               # (n_fft, hop, win)
CLAMP = 1e-7


def magnitude(x, n_fft, hop, win):
    """x [B, T] -> (|X| [B, F, frames], re^2 + im^2)"""
    X = torch.stft(x, n_fft, hop, win, torch.hann_window(win, periodic=True, dtype=x.dtype), center=True, pad_mode="reflect", return_complex=True)
    p = X.real ** 2 + X.imag ** 2
    return torch.sqrt(torch.clamp(p, min=CLAMP)), p


def stft_loss(pred, target, resolutions=RESOLUTIONS, dtype=torch.float64):
    """-> (L, terms [n, 2] = (L_sc, L_mag) per resolution, the smallest re^2 + im^2 over all resolutions of (the prediction, the target))"""
    pred, target = pred.to(dtype), target.to(dtype)
    terms, low = [], [float("inf"), float("inf")]
    for n_fft, hop, win in resolutions:
        mx, px = magnitude(pred, n_fft, hop, win)
        my, py = magnitude(target, n_fft, hop, win)
        sc = torch.norm(my - mx, p="fro") / torch.norm(my, p="fro")
        mag = (torch.log(my) - torch.log(mx)).abs().mean()
        terms.append(torch.stack([sc, mag]))
        low = [min(low[0], float(px.detach().min())), min(low[1], float(py.detach().min()))]
    terms = torch.stack(terms)
    return terms.sum() / len(resolutions), terms, low


def loss_and_grad(pred, target, resolutions=RESOLUTIONS, dtype=torch.float64):
    """-> {'L', 'terms', 'dpred', 'low' (of both signals), 'low_pred'} by autograd of `stft_loss`"""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    L, terms, low = stft_loss(p, target.detach(), resolutions, dtype)
    L.backward()
    return {"L": L.detach().reshape(1), "terms": terms.detach(), "dpred": p.grad.detach(), "low": min(low), "low_pred": low[0]}


def errors(got, ref64, ref32):
    scale = float(ref64.abs().max())
    return float((got.double().cpu() - ref64).abs().max()) / scale, float((ref32.double() - ref64).abs().max()) / scale, scale


def check(name, got, ref64, ref32):
    """The project's bar: err <= 4 e32 + 1e-6 with the guards 0 < e32 < 1e-3 and max |ref64| > 1e-3; the figures are printed before they are asserted."""
    err, e32, scale = errors(got, ref64, ref32)
    print("{}: err {:.3e}  e32 {:.3e}  ratio {:.3f}  max|ref| {:.3e}".format(name, err, e32, err / (4 * e32 + 1e-6), scale))
    assert 0 < e32 < 1e-3 and scale > 1e-3, (name, e32, scale)
    assert err <= 4 * e32 + 1e-6, (name, err, e32)


def signals(B, T, seed, amplitude=0.3):
    """(pred, target) [B, T] float32: unrelated white noise of the given amplitude - no bin of either comes near the clamp"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, generator=g) * amplitude).float(), (torch.randn(B, T, generator=g) * amplitude).float()


# ---- the kernels' form, float64 numpy --------------------------------------------------------------------------------------------------------
def reflect(s, T):
    """index of sample s under reflect padding (one reflection: -T < s < 2 T - 1)"""
    s = np.where(s < 0, -s, s)
    return np.where(s >= T, 2 * (T - 1) - s, s)


def frames_spectrum(x, n_fft, hop, win):
    """x [T] -> X [frames, F] complex: gather under reflect padding, the periodic Hann of `win` centred in n_fft, the real DFT"""
    T, M, lpad = len(x), n_fft // 2, (n_fft - win) // 2
    nf = 1 + T // hop
    w = np.zeros(n_fft)
    w[lpad:lpad + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    idx = reflect(np.arange(nf)[:, None] * hop + np.arange(n_fft)[None, :] - M, T)
    return np.fft.rfft(x[idx] * w[None, :], axis=1), w


def kernel_form_grad(pred, target, resolutions=RESOLUTIONS, drop_last_frame=False, unfolded=False, floor_cover=False):
    """pred, target [B, T] float64 numpy -> (L, d pred) in the kernels' form.  The three switches each break it: the gather forgets the last frame, the
    reflect padding is not folded back, win // hop frames are gathered in place of ceil(win / hop)."""
    B, T = pred.shape
    L, dpred = 0.0, np.zeros_like(pred)
    for n_fft, hop, win in resolutions:
        M, lpad, nf = n_fft // 2, (n_fft - win) // 2, 1 + T // hop
        X, Y = [], []
        for b in range(B):
            xs, w = frames_spectrum(pred[b], n_fft, hop, win)
            X.append(xs)
            Y.append(frames_spectrum(target[b], n_fft, hop, win)[0])
        X, Y = np.stack(X), np.stack(Y)
        px = X.real ** 2 + X.imag ** 2
        mx, my = np.sqrt(np.maximum(px, CLAMP)), np.sqrt(np.maximum(Y.real ** 2 + Y.imag ** 2, CLAMP))
        nd, ny, n = np.sqrt(((my - mx) ** 2).sum()), np.sqrt((my ** 2).sum()), mx.size
        L += (nd / ny + np.abs(np.log(my) - np.log(mx)).mean()) / len(resolutions)
        coef = 1.0 / (nd * ny) if nd > 0 else 0.0
        dmag = ((mx - my) * coef + np.sign(mx - my) / (n * mx)) / len(resolutions)
        G = np.where(px < CLAMP, 0.0, dmag / mx) * X                                     # dL/dre + i dL/dim
        full = np.zeros((B, nf, n_fft), dtype=np.complex128)
        full[:, :, :M + 1] = G                                                           # every bin once: no Hermitian doubling
        dfr = (np.fft.ifft(full, axis=2).real * n_fft * w[None, None, :])[:, :, lpad:lpad + win]    # Re sum_k G[k] exp(+2 pi i k n / n_fft), windowed
        cover = win // hop if floor_cover else -(-win // hop)
        last = nf - 2 if drop_last_frame else nf - 1

        def dpad(b, p):
            pp, acc = p - lpad, 0.0
            if pp < 0:
                return acc
            for t in range(pp // hop - cover + 1, pp // hop + 1):                        # ascending frame order
                j = pp - t * hop
                if 0 <= t <= last and j < win:
                    acc += dfr[b, t, j]
            return acc

        for b in range(B):
            for s in range(T):
                r = dpad(b, M + s)
                if not unfolded:
                    if 1 <= s <= M:
                        r += dpad(b, M - s)
                    if T - 1 - M <= s <= T - 2:
                        r += dpad(b, M + 2 * (T - 1) - s)
                dpred[b, s] += r
    return L, dpred


# ---- the generator under autograd ---------------------------------------------------------------------------------------------------------------
def generator_grads(sd, cfg, mels, noises, functionals, dtype=torch.float64):
    """One backward of the loss sum_b <functionals[b], wav_b> through tests/pwg_ref.py's generator: mels [A, L_b], noises [T_b], functionals [T_b] per
    utterance -> (wavs, {state-dict key: gradient})"""
    import pwg_ref as P
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    wavs, total = [], 0.0
    for mel, z, f in zip(mels, noises, functionals):
        wav = P.generator(params, cfg, mel, z, dtype)
        total = total + (wav * f.to(dtype)).sum()
        wavs.append(wav.detach())
    total.backward()
    return wavs, {k: torch.zeros_like(p) if p.grad is None else p.grad.detach() for k, p in params.items()}     # (nothing reads the last layer's x')


def layer_grads(sd, cfg, i, x, c, dxp, dskips, dtype=torch.float64):
    """Layer i alone: x [R, T], c [A, T], the gradients of its outputs dxp [R, T], dskips [S, T] -> {'dx', 'dc', conv.weight, ...} by autograd"""
    import pwg_ref as P
    q = "conv_layers.{}.".format(i)
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith(q)}
    x, c = x.detach().to(dtype).clone().requires_grad_(True), c.detach().to(dtype).clone().requires_grad_(True)
    xn, skip = P.layer(params, cfg, i, x, c, dtype)
    ((xn * dxp.to(dtype)).sum() + (skip * dskips.to(dtype)).sum()).backward()
    out = {k[len(q):]: p.grad.detach() for k, p in params.items()}
    out.update(dx=x.grad.detach(), dc=c.grad.detach())
    return out
