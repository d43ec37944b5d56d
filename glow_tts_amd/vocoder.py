"""Waveform output: a Griffin-Lim vocoder on the HIP kernels of csrc/vocoder_ops.hip.  A BASELINE vocoder (no weights, audibly phasey), not a neural one:
it inverts exactly the front end `audio.py` restates (pre-emphasis, centred reflect-padded STFT, periodic Hann of Frame_Length zero-padded to n_fft, hop
Frame_Shift, Slaney mel filterbank, dB normalisation to +- Max_Abs_Mel), so a generated or converted mel can be listened to without a second project.

    mel [B, Mel, T] --mel_to_linear--> |S| [B, T, F] --(phase0)--> x_0 --`iterations` x (griffin_lim_step + overlap_add)--> wav [B, hop (T - 1)]

Fast Griffin-Lim with the momentum applied to the SIGNAL (the STFT is linear): y = x_n + alpha (x_n - x_n-1), x_n+1 = istft(|S| * Y / max(|Y|, 1e-8)) with
Y = stft(y); two signals are kept, never a previous spectrogram, and the complex spectrum of an iteration never leaves LDS.  The waveform is still
pre-emphasised: `audio.deemphasis` undoes that on the host before the samples are written."""
import numpy as np
import torch

from . import _lib, audio, ops

DEFAULT_ITERATIONS, DEFAULT_MOMENTUM = 60, 0.99
T_BUCKET = 64                                                       # frames: the work buffers are sized for T_max rounded up to a multiple of it


def geometry(hp):
    """(n_fft, win_length, hop) of hp.Sound; raises ValueError naming the offending Sound.* keys when the kernels do not support it."""
    s = hp.Sound
    n_fft, win, hop = (int(s.Spectrogram_Dim) - 1) * 2, int(s.Frame_Length), int(s.Frame_Shift)
    if n_fft < 256 or n_fft > 4096 or n_fft & (n_fft - 1):
        raise ValueError(f"Sound.Spectrogram_Dim = {s.Spectrogram_Dim}: the vocoder needs n_fft = 2 * (Spectrogram_Dim - 1) to be a power of two in [256, 4096], "
                         f"got {n_fft}")
    if win < 1 or win > n_fft:
        raise ValueError(f"Sound.Frame_Length = {win} must lie in [1, n_fft = {n_fft}] (Sound.Spectrogram_Dim = {s.Spectrogram_Dim})")
    if hop < 1 or win % hop:
        raise ValueError(f"Sound.Frame_Length = {win} must be a multiple of Sound.Frame_Shift = {hop} (the overlap-add gathers Frame_Length / Frame_Shift frames "
                         "per sample)")
    return n_fft, win, hop


def fft_tables(n_fft, win):
    """(twiddle [n_fft / 2, 2] = (cos, -sin)(2 pi k / n_fft), window [win] = periodic Hann) in float64: the tables of the LDS FFT, shared with
    `frontend.Analyzer`; the callers round them once to fp32."""
    k = np.arange(n_fft // 2, dtype=np.float64)
    tw = np.stack([np.cos(2.0 * np.pi * k / n_fft), -np.sin(2.0 * np.pi * k / n_fft)], axis=1)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win)                # periodic Hann (scipy get_window("hann", fftbins=True))
    return tw, w


def settings(hp):
    """(iterations, momentum) of the optional yaml block `Griffin_Lim: {Iterations: 60, Momentum: 0.99}`."""
    g = getattr(hp, "Griffin_Lim", None)
    return int(getattr(g, "Iterations", DEFAULT_ITERATIONS)), float(getattr(g, "Momentum", DEFAULT_MOMENTUM))


class GriffinLim:
    """GriffinLim(hp, device)(mels [B, Mel, T], mel_lengths) -> (wav [B, hop (T - 1)] fp32 on the device, wav_lengths [B] int64)."""

    def __init__(self, hp, device="cuda:0"):
        self.geo = geometry(hp)                                    # before anything touches the device
        self.iterations, self.momentum = settings(hp)
        s = hp.Sound
        n_fft, win, hop = self.geo
        self.device = torch.device(device)
        self.n_freq, self.n_mel, self.max_abs = n_fft // 2 + 1, int(s.Mel_Dim), float(s.Max_Abs_Mel)
        self.sample_rate, self.pre_emphasis = int(s.Sample_Rate), 0.97
        # tables in float64 on the host, rounded once to fp32
        tw, w = fft_tables(n_fft, win)
        fb = audio.mel_filterbank(self.sample_rate, n_fft, self.n_mel, s.Mel_F_Min, s.Mel_F_Max).astype(np.float64)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        self.twiddle, self.window, self.basis = to(tw), to(w), to(np.linalg.pinv(fb))
        self._capacity, self._buffers = 0, None

    def _work(self, B, T):
        """Work buffers of a call (two signals, the frames' overlap-add contributions, the magnitudes): views of ONE set that is sized for the largest
        bucket seen so far - B x T_max rounded up to T_BUCKET frames - and grows only when a call exceeds it, so batches of varying length allocate
        nothing and device memory is bounded by the largest batch (275 MB at B = 32 x 800 frames).  The kernels honour the lengths and every sample
        and magnitude of the views is rewritten by the call, so what an earlier call left behind is never read."""
        n_fft, win, hop = self.geo
        frames = B * (-(-T // T_BUCKET) * T_BUCKET)
        if frames > self._capacity:
            self._buffers = None                                   # the smaller set goes back to the allocator first
            f = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)
            self._buffers = {"x": [f(frames * hop), f(frames * hop)], "frames": f(frames * win), "mag": f(frames * self.n_freq)}
            self._capacity = frames
        L, bf = max(hop * (T - 1), 1), self._buffers
        return {"x": [v[:B * L].view(B, L) for v in bf["x"]], "frames": bf["frames"][:B * T * win].view(B, T, win),
                "mag": bf["mag"][:B * T * self.n_freq].view(B, T, self.n_freq)}

    def _lengths(self, lengths, B):
        return torch.as_tensor(lengths).to(device=self.device, dtype=torch.int32).reshape(B).contiguous()

    def mel_to_linear(self, mels, mel_lengths, out=None):
        """Normalised mels [B, Mel, T] -> linear magnitudes [B, T, F] (pseudo-inverse of the mel filterbank, clamped at 1e-10; padded frames zero)."""
        mels = mels.to(device=self.device, dtype=torch.float32).contiguous()
        B, Mel, T = mels.shape
        if Mel != self.n_mel:
            raise ValueError(f"mels have {Mel} channels, Sound.Mel_Dim = {self.n_mel}")
        mag = out if out is not None else torch.empty(B, T, self.n_freq, dtype=torch.float32, device=self.device)
        ops.mel_to_linear(mels, self._lengths(mel_lengths, B), self.basis, mag, self.max_abs)
        return mag

    def stft(self, wav, wav_lengths=None):
        """wav [B, L] (sample counts `wav_lengths`, default L) -> complex spectrogram [B, 1 + L // hop, F]."""
        wav = wav.to(device=self.device, dtype=torch.float32).contiguous()
        B, L = wav.shape
        lengths = self._lengths(wav_lengths if wav_lengths is not None else [L] * B, B)
        spec = torch.empty(B, 1 + L // self.geo[2], self.n_freq, 2, dtype=torch.float32, device=self.device)
        ops.stft(wav, lengths, self.window, self.twiddle, spec, self.geo)
        return torch.view_as_complex(spec)

    def istft(self, spec, frame_lengths=None):
        """complex [B, T, F] (frame counts `frame_lengths`, default T) -> wav [B, hop (T - 1)]"""
        spec = torch.view_as_real(spec.to(device=self.device, dtype=torch.complex64).contiguous())
        B, T = spec.shape[:2]
        n_fft, win, hop = self.geo
        lengths = self._lengths(frame_lengths if frame_lengths is not None else [T] * B, B)
        frames = torch.empty(B, T, win, dtype=torch.float32, device=self.device)
        wav = torch.empty(B, max(hop * (T - 1), 1), dtype=torch.float32, device=self.device)
        ops.istft(spec, lengths, self.window, self.twiddle, frames, wav, self.geo)
        return wav[:, :hop * (T - 1)]

    @torch.no_grad()
    def griffin_lim(self, mag, frame_lengths, iterations=None, momentum=None, initial_phase=None):
        """Magnitudes [B, T, F] -> (wav [B, hop (T - 1)], wav_lengths)."""
        if not mag.is_cuda:
            raise _lib.GlowTTSHipError("expected a device tensor (the HIP path has no CPU fallback)")
        B, T, F = mag.shape
        n_fft, win, hop = self.geo
        iterations = self.iterations if iterations is None else int(iterations)
        alpha = self.momentum if momentum is None else float(momentum)
        lengths = self._lengths(frame_lengths, B)
        wk = self._work(B, T)
        if initial_phase is None:                                  # torch's device generator: a seeded call is reproducible
            initial_phase = (torch.rand(B, T, F, dtype=torch.float32, device=self.device) * 2.0 - 1.0) * float(np.pi)
        ph = initial_phase.to(device=self.device, dtype=torch.float32)
        if tuple(ph.shape) != (B, T, F):
            raise ValueError(f"initial_phase has shape {tuple(ph.shape)}, expected {(B, T, F)}")
        mag = mag.contiguous()
        # the start spectrum |S| exp(i phase_0): the one allocation of a call besides the returned waveform, filled in place and handed back to torch's
        # caching allocator before the iterations
        spec = torch.empty(B, T, F, 2, dtype=torch.float32, device=self.device)
        torch.cos(ph, out=spec[..., 0])
        torch.sin(ph, out=spec[..., 1])
        spec.mul_(mag.unsqueeze(-1))
        x, xp = wk["x"]
        ops.istft(spec, lengths, self.window, self.twiddle, wk["frames"], x, self.geo)
        del spec
        for i in range(iterations):
            # the first iteration has no history: x_prev = x (y = x exactly)
            ops.griffin_lim_step(x, x if i == 0 else xp, mag, lengths, self.window, self.twiddle, alpha, wk["frames"], self.geo)
            ops.overlap_add(wk["frames"], lengths, self.window, xp, self.geo)      # x_n-1 is dead: its buffer takes x_n+1
            x, xp = xp, x
        # a copy: the work buffers belong to the next call
        return x[:, :hop * (T - 1)].clone(), (lengths.to(torch.int64) - 1).clamp_(min=0) * hop

    def __call__(self, mels, mel_lengths, iterations=None, momentum=None, initial_phase=None):
        B, _, T = mels.shape
        mag = self.mel_to_linear(mels, mel_lengths, out=self._work(B, T)["mag"])
        return self.griffin_lim(mag, mel_lengths, iterations, momentum, initial_phase)

    def to_host(self, wav, wav_lengths):
        """Device waveforms -> list of de-emphasised float32 numpy arrays (what `audio.write_wav` takes)."""
        wav, n = wav.cpu().numpy(), wav_lengths.cpu().tolist()
        return [audio.deemphasis(w[:m], self.pre_emphasis).astype(np.float32) for w, m in zip(wav, n)]
