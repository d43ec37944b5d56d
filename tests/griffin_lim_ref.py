"""Float64 yardstick of the Griffin-Lim vocoder (glow_tts_amd/vocoder.py, csrc/vocoder_ops.hip): a numpy restatement of `stft`, `istft`, `mel_to_linear`
and `griffin_lim` with the identical update rule, floors and lengths, on `numpy.fft`.  The product never imports it.  Every function takes `dtype`
(default float64); with `numpy.float32` the same arithmetic runs in single precision - the tests use that copy to size their error bars (what fp32 costs on
this input with a different FFT factorisation), never as a reference.

Framing is `glow_tts_amd.audio.stft_magnitude`'s: center = True, reflect padding by n_fft / 2, a periodic Hann window of win_length centred in n_fft.
A T-frame spectrogram gives hop * (T - 1) samples.  Fast Griffin-Lim's momentum is applied to the SIGNAL (the STFT is linear):
    x_0 = x_-1 = istft(S exp(i phase0));    y = x_n + alpha (x_n - x_n-1);    x_n+1 = istft(S * Y / max(|Y|, 1e-8)),  Y = stft(y)."""
import numpy as np


def window(n_fft, win_length, dtype=np.float64):
    """Periodic Hann of win_length -> [win_length], and its offset inside the n_fft-point frame."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length, dtype=np.float64) / win_length)
    return w.astype(dtype), (n_fft - win_length) // 2


def _ctype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def stft(x, n_fft, hop, win_length, dtype=np.float64):
    """x [L] -> complex [1 + L // hop, n_fft / 2 + 1]"""
    w, lpad = window(n_fft, win_length, dtype)
    wf = np.zeros(n_fft, dtype)
    wf[lpad:lpad + win_length] = w
    y = np.pad(np.asarray(x, dtype), n_fft // 2, mode="reflect")
    n = 1 + (len(y) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n)[:, None]
    return np.fft.rfft(y[idx] * wf[None, :], axis=1).astype(_ctype(dtype))


def istft(spec, n_fft, hop, win_length, dtype=np.float64):
    """complex [T, n_fft / 2 + 1] -> [hop * (T - 1)]: inverse FFT, window again, overlap-add, divide by the summed squared window floored at 1e-8."""
    spec = np.asarray(spec, _ctype(dtype))
    T = spec.shape[0]
    w, lpad = window(n_fft, win_length, dtype)
    frames = np.fft.irfft(spec, n_fft, axis=1).astype(dtype)[:, lpad:lpad + win_length] * w[None, :]
    out = np.zeros(n_fft + hop * (T - 1), dtype)
    wss = np.zeros(n_fft + hop * (T - 1), dtype)
    for t in range(T):                                   # ascending frame order, as the gather of the kernel
        out[t * hop + lpad:t * hop + lpad + win_length] += frames[t]
        wss[t * hop + lpad:t * hop + lpad + win_length] += w * w
    out = out / np.maximum(wss, dtype(1e-8))
    return out[n_fft // 2:n_fft // 2 + hop * (T - 1)]


def mel_amplitude(mel, max_abs, dtype=np.float64):
    """Undo `audio.mel_generate`'s normalisation: [-max_abs, max_abs] -> amplitude (the 1e-7 of the log removed, floored at 0)."""
    m = np.clip(np.asarray(mel, dtype), -max_abs, max_abs)
    db = (m + dtype(max_abs)) / dtype(2 * max_abs) * dtype(100) - dtype(100)
    return np.maximum(np.power(dtype(10), db / dtype(20)) - dtype(1e-7), dtype(0))


def mel_basis_pinv(sample_rate, n_fft, n_mels, fmin, fmax):
    """[n_fft / 2 + 1, n_mels] float64: pseudo-inverse of the Slaney filterbank of the front end."""
    from glow_tts_amd import audio
    return np.linalg.pinv(audio.mel_filterbank(sample_rate, n_fft, n_mels, fmin, fmax).astype(np.float64))


def mel_to_linear(mel, basis, max_abs, dtype=np.float64):
    """mel [Mel, T] normalised, basis [F, Mel] -> magnitudes [T, F] clamped to >= 1e-10"""
    amp = mel_amplitude(mel, max_abs, dtype)
    return np.maximum(np.asarray(basis, dtype) @ amp, dtype(1e-10)).T


def griffin_lim(mag, phase0, n_fft, hop, win_length, iterations, momentum, dtype=np.float64):
    """mag [T, F], phase0 [T, F] (angles) -> waveform [hop * (T - 1)]"""
    mag = np.asarray(mag, dtype)
    ph = np.asarray(phase0, dtype)
    x = istft(mag * (np.cos(ph) + 1j * np.sin(ph)).astype(_ctype(dtype)), n_fft, hop, win_length, dtype)
    x_prev = x
    alpha = dtype(momentum)
    for _ in range(iterations):
        y = x + alpha * (x - x_prev)
        Y = stft(y, n_fft, hop, win_length, dtype)
        P = Y / np.maximum(np.abs(Y), dtype(1e-8))
        x_prev, x = x, istft(mag * P, n_fft, hop, win_length, dtype)
    return x


def spectral_convergence(x, mag, n_fft, hop, win_length):
    """|| |STFT64(x)| - S ||_F / || S ||_F in float64"""
    S = np.asarray(mag, np.float64)
    return float(np.linalg.norm(np.abs(stft(np.asarray(x, np.float64), n_fft, hop, win_length)) - S) / np.linalg.norm(S))


def make_signal(seed=0, sample_rate=24000, seconds=3.0):
    """The synthetic test input: a 39-harmonic tone whose f0 wanders 120 +- 60 Hz, a syllable-like on/off envelope, 2 % noise."""
    rng = np.random.default_rng(seed)
    n = int(sample_rate * seconds)
    t = np.arange(n) / sample_rate
    f0 = 120.0 + 60.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 2 * np.pi))
    phase = 2 * np.pi * np.cumsum(f0) / sample_rate
    amps = 1.0 / np.arange(1, 40) * rng.uniform(0.5, 1.0, 39)
    x = sum(a * np.sin(k * phase + rng.uniform(0, 2 * np.pi)) for k, a in zip(range(1, 40), amps))
    env = np.clip(1.5 * np.sin(2 * np.pi * 2.5 * t) + 0.5, 0.0, 1.0)
    x = x * env
    x = 0.5 * x / np.abs(x).max()
    return x + 0.02 * 0.5 * rng.standard_normal(n)
