"""Analysis front end on the HIP kernels of csrc/frontend_ops.hip: the device counterpart of `audio.mel_generate` and `audio.pitch_generate`, batched.

    wav [B, L] --mel_analysis (pre-emphasis, STFT, sparse mel filterbank, dB normalisation: one launch)--> mel [B, T, Mel]
    wav [B, L] --yin (difference function, cumulative-mean normalisation, decision: one launch)--> Hz [B, T] --min / max per utterance--> pitch in [0, 1]

What stays on the host: decoding, resampling, trimming and peak normalisation (`audio.audio_prep`; file-bound, and the trim decides the lengths before a
batch exists) and the optional Gaussian smoothing of the pitch track (the same scipy call as the host path, between the device YIN and the normalisation).
The tables (twiddles and window - shared with `vocoder.GriffinLim` - and the sparse filterbank) are built in float64 on the host and rounded once."""
import numpy as np
import torch

from . import audio, ops, vocoder

PRE_EMPHASIS, MIN_LEVEL_DB = 0.97, -100.0                           # audio.mel_generate's defaults, as `audio.pattern_from_wav` calls it
YIN_W_LEN, YIN_W_STEP, YIN_F0_MIN, YIN_F0_MAX = 1024, 256, 100, 500  # fixed in the reference whatever the yaml says (see audio.pitch_generate)
SAMPLE_BUDGET = 8 << 20                                             # padded samples per batch of `Analyzer.__call__` (32 x 800 frames at hop 256 is 6.5 M)


def geometry(hp, with_pitch=True):
    """(n_fft, win_length, hop) of hp.Sound; raises ValueError naming the offending Sound.* keys when the analysis kernels do not support it."""
    s = hp.Sound
    n_fft, win, hop = (int(s.Spectrogram_Dim) - 1) * 2, int(s.Frame_Length), int(s.Frame_Shift)
    if n_fft < 256 or n_fft > 4096 or n_fft & (n_fft - 1):
        raise ValueError(f"Sound.Spectrogram_Dim = {s.Spectrogram_Dim}: the front end needs n_fft = 2 * (Spectrogram_Dim - 1) to be a power of two in "
                         f"[256, 4096], got {n_fft}")
    if win < 1 or win > n_fft:
        raise ValueError(f"Sound.Frame_Length = {win} must lie in [1, n_fft = {n_fft}] (Sound.Spectrogram_Dim = {s.Spectrogram_Dim})")
    if hop < 1:
        raise ValueError(f"Sound.Frame_Shift = {hop} must be positive")
    if with_pitch and hop != YIN_W_STEP:
        raise ValueError(f"Sound.Frame_Shift = {hop}: the pitch track is always analysed every {YIN_W_STEP} samples, so mel and pitch have the same number "
                         f"of frames only at Sound.Frame_Shift = {YIN_W_STEP}")
    return n_fft, win, hop


def sparse_filterbank(fb):
    """Dense filterbank [Mel, F] -> (index [Mel, 3] int32 = (first bin, bin count, offset into the weights), weights [sum of counts]): row j is
    weights[offset_j:offset_j + count_j] at bins first_j ...; a row's support is one run of bins (a triangle), zeros inside a run are kept."""
    fb = np.asarray(fb)
    index, weights, off = np.zeros((fb.shape[0], 3), np.int32), [], 0
    for j, row in enumerate(fb):
        nz = np.flatnonzero(row)
        if nz.size:
            first, count = int(nz[0]), int(nz[-1] - nz[0] + 1)
            index[j] = (first, count, off)
            weights.append(row[first:first + count])
            off += count
        else:
            index[j] = (0, 0, off)
    w = np.concatenate(weights) if weights else np.zeros(0, fb.dtype)
    return index, np.ascontiguousarray(w if w.size else np.zeros(1, fb.dtype))      # never empty: the kernel takes a non-null table


def dense_filterbank(index, weights, n_freq):
    """Inverse of `sparse_filterbank`."""
    fb = np.zeros((index.shape[0], n_freq), weights.dtype)
    for j, (first, count, off) in enumerate(index):
        fb[j, first:first + count] = weights[off:off + count]
    return fb


def yin_frames(n, w_len=YIN_W_LEN, w_step=YIN_W_STEP):
    """Frames `audio.yin_pitch` makes of n samples."""
    if n < 1:
        return 0
    span = n + 2 * ((w_step + w_len - n % w_step) // 2) - w_len
    return max(0, -(-span // w_step))


class Analyzer:
    """Analyzer(hp, device)(list of float32 audio arrays) -> [(mel [T, Mel], pitch [T] or None)]; `mel` / `pitch` take padded batches on the device."""

    def __init__(self, hp, device="cuda:0", with_pitch=True):
        self.geo = geometry(hp, with_pitch)                         # before anything touches the device
        s = hp.Sound
        n_fft, win, hop = self.geo
        self.with_pitch = bool(with_pitch)
        self.device = torch.device(device)
        self.n_freq, self.n_mel, self.max_abs = n_fft // 2 + 1, int(s.Mel_Dim), float(s.Max_Abs_Mel)
        self.sample_rate = int(s.Sample_Rate)
        self.thresh = 1.0 - float(getattr(s, "Confidence_Threshold", 0.6))
        self.sigma = float(getattr(s, "Gaussian_Smoothing_Sigma", 0.0))
        self.tau_min, self.tau_max = int(self.sample_rate / YIN_F0_MAX), min(int(self.sample_rate / YIN_F0_MIN), YIN_W_LEN)
        # tables in float64 on the host, rounded once to fp32
        tw, w = vocoder.fft_tables(n_fft, win)
        index, weights = sparse_filterbank(audio.mel_filterbank(self.sample_rate, n_fft, self.n_mel, s.Mel_F_Min, s.Mel_F_Max))
        to = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        self.twiddle, self.window, self.fb_index, self.fb_weight = to(tw), to(w), to(index, np.int32), to(weights)
        self._capacity, self._buffers = (0, 0), None

    # ---- padded batches on the device ----
    def _wav(self, wav, wav_lengths):
        wav = torch.as_tensor(wav).to(device=self.device, dtype=torch.float32).contiguous()
        B, L = wav.shape
        lengths = torch.as_tensor(wav_lengths if wav_lengths is not None else [L] * B).to(device=self.device, dtype=torch.int32).reshape(B).contiguous()
        return wav, lengths

    def _mel_into(self, wav, lengths, out):
        ops.mel_analysis(wav, lengths, self.window, self.twiddle, self.fb_index, self.fb_weight, out, self.geo, PRE_EMPHASIS, MIN_LEVEL_DB, self.max_abs)

    def mel(self, wav, wav_lengths=None):
        """wav [B, L] (sample counts `wav_lengths`, default L) -> (mels [B, 1 + L // hop, Mel] padded with -Max_Abs_Mel, frame_lengths [B] int64)."""
        wav, lengths = self._wav(wav, wav_lengths)
        hop = self.geo[2]
        out = torch.empty(wav.shape[0], 1 + wav.shape[1] // hop, self.n_mel, dtype=torch.float32, device=self.device)
        self._mel_into(wav, lengths, out)
        n = lengths.to(torch.int64)
        return out, torch.where(n > 0, 1 + n // hop, torch.zeros_like(n))

    def yin(self, wav, wav_lengths=None, thresh=None, w_len=YIN_W_LEN, w_step=YIN_W_STEP, tau_min=None, tau_max=None, with_cmnd=False, out=None):
        """wav [B, L] -> (Hz [B, T] with T = frames of L samples, 0 where unvoiced or beyond the utterance, frame_lengths [B] int64, cmnd [B, T, tau_max] or
        None).  The defaults are the reference's fixed analysis (1024 / 256, 100 .. 500 Hz) at 1 - Sound.Confidence_Threshold."""
        wav, lengths = self._wav(wav, wav_lengths)
        B, L = wav.shape
        tau_min = self.tau_min if tau_min is None else int(tau_min)
        tau_max = self.tau_max if tau_max is None else int(tau_max)
        T = max(yin_frames(L, w_len, w_step), 1)
        hz = out if out is not None else torch.empty(B, T, dtype=torch.float32, device=self.device)
        cmnd = torch.empty(B, T, tau_max, dtype=torch.float32, device=self.device) if with_cmnd else None
        ops.yin(wav, lengths, hz, w_len, w_step, tau_min, tau_max, self.thresh if thresh is None else thresh, self.sample_rate, cmnd)
        n = lengths.to(torch.int64)
        pad = (w_step + w_len - n % w_step) // 2
        frames = torch.where(n > 0, (-(-(n + 2 * pad - w_len) // w_step)).clamp(min=0), torch.zeros_like(n))
        return hz, frames, cmnd

    def _normalise(self, hz, frames):
        """Hz [B, T] -> the track of `audio.pitch_generate`: optional host smoothing, then (p - min) / (max - min + 1e-7) over each utterance's frames."""
        # the kernel's Hz are sample_rate / tau rounded to fp32: recompute them in float64 from the integer tau, as the host has them
        voiced = hz > 0
        tau = torch.round(float(self.sample_rate) / torch.where(voiced, hz.double(), torch.ones_like(hz, dtype=torch.float64)))
        hz = torch.where(voiced, float(self.sample_rate) / tau, torch.zeros_like(tau))
        if self.sigma > 0.0:
            from scipy.ndimage import gaussian_filter1d
            host = hz.cpu().numpy()
            for b, n in enumerate(frames.cpu().tolist()):
                if n:
                    host[b, :n] = gaussian_filter1d(host[b, :n], sigma=self.sigma)
            p = torch.from_numpy(host).to(self.device)
        else:
            p = hz
        valid = torch.arange(p.shape[1], device=self.device)[None, :] < frames[:, None]
        inf = torch.full_like(p, float("inf"))
        lo, hi = torch.where(valid, p, inf).amin(1, keepdim=True), torch.where(valid, p, -inf).amax(1, keepdim=True)
        return torch.where(valid, (p - lo) / (hi - lo + 1e-7), torch.zeros_like(p)).to(torch.float32)

    def pitch(self, wav, wav_lengths=None):
        """wav [B, L] -> (normalised pitch track [B, T] in [0, 1], 0 beyond the utterance, frame_lengths [B] int64)."""
        hz, frames, _ = self.yin(wav, wav_lengths)
        return self._normalise(hz, frames), frames

    # ---- lists of utterances ----
    def _work(self, samples, frames):
        """One grow-only set of buffers - a pinned staging signal, its device copy and one flat output (mels, then the Hz track) - sized for the largest
        batch seen so far; every element a call reads is rewritten by that call."""
        cs, cf = self._capacity
        if samples > cs or frames > cf or self._buffers is None:
            cs, cf = max(cs, samples), max(cf, frames)
            self._buffers = None                                   # the smaller set goes back to the allocator first
            host = torch.zeros(cs, dtype=torch.float32)
            self._buffers = {"host": host.pin_memory() if self.device.type == "cuda" else host,
                             "wav": torch.zeros(cs, dtype=torch.float32, device=self.device),
                             "out": torch.zeros(cf * (self.n_mel + 1), dtype=torch.float32, device=self.device)}
            self._capacity = (cs, cf)
        return self._buffers

    def _batch(self, arrays, with_pitch):
        B, L = len(arrays), max(max(len(a) for a in arrays), 1)
        T = 1 + L // self.geo[2]
        bf = self._work(B * L, B * T)
        host = bf["host"][:B * L].view(B, L)
        hnp = host.numpy()
        for b, a in enumerate(arrays):
            hnp[b, :len(a)] = a
            hnp[b, len(a):] = 0.0
        wav = bf["wav"][:B * L].view(B, L)
        wav.copy_(host, non_blocking=True)                         # one padded upload
        lengths = torch.tensor([len(a) for a in arrays], dtype=torch.int32).to(self.device)
        mel = bf["out"][:B * T * self.n_mel].view(B, T, self.n_mel)
        self._mel_into(wav, lengths, mel)
        n_out = B * T * self.n_mel
        if with_pitch:                                             # hop = 256: the track has the mel's frame count
            hz = bf["out"][n_out:n_out + B * T].view(B, T)
            _, frames, _ = self.yin(wav, lengths, out=hz)
            hz.copy_(self._normalise(hz, frames))
            n_out += B * T
        flat = bf["out"][:n_out].cpu().numpy()                      # one download (synchronises: the staging buffer is free again)
        mels, pit = flat[:B * T * self.n_mel].reshape(B, T, self.n_mel), flat[B * T * self.n_mel:].reshape(B, -1)
        out = []
        for b, a in enumerate(arrays):
            n = 1 + len(a) // self.geo[2] if len(a) else 0
            out.append((mels[b, :n].copy(), pit[b, :n].copy() if with_pitch else None))
        return out

    @torch.no_grad()
    def __call__(self, audios, with_pitch=True, sample_budget=SAMPLE_BUDGET):
        """List of float32 audio arrays (what `audio.audio_prep` returns) -> [(mel [T, Mel], pitch [T] or None)] in the caller's order.  Utterances are
        sorted by length and batched so that a padded batch holds at most `sample_budget` samples."""
        if with_pitch and not self.with_pitch:
            raise ValueError("this Analyzer was built without the pitch track (with_pitch=False)")
        arrays = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in audios]
        order = sorted(range(len(arrays)), key=lambda i: -len(arrays[i]))
        results, i = [None] * len(arrays), 0
        while i < len(order):
            longest = max(len(arrays[order[i]]), 1)
            n = max(1, min(len(order) - i, sample_budget // longest, 65535))
            idx = order[i:i + n]
            for k, r in zip(idx, self._batch([arrays[k] for k in idx], with_pitch)):
                results[k] = r
            i += n
        return results
