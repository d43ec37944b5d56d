"""Waveform output.  Three vocoders: Griffin-Lim (below, the default) and - with the optional yaml block `Vocoder` and a checkpoint - the Parallel WaveGAN
generator `ParallelWaveGAN` on the kernels of csrc/pwg_ops.hip (second half of this file) or, with `Type: 'HiFiGAN'` in that block, the HiFi-GAN generator
`HiFiGAN` on the kernels of csrc/hifigan_ops.hip (the end of this file, with `make_vocoder`, the one place that chooses).

Griffin-Lim: a vocoder on the HIP kernels of csrc/vocoder_ops.hip.  A BASELINE vocoder (no weights, audibly phasey), not a neural one:
it inverts exactly the front end `audio.py` restates (pre-emphasis, centred reflect-padded STFT, periodic Hann of Frame_Length zero-padded to n_fft, hop
Frame_Shift, Slaney mel filterbank, dB normalisation to +- Max_Abs_Mel), so a generated or converted mel can be listened to without a second project.

    mel [B, Mel, T] --mel_to_linear--> |S| [B, T, F] --(phase0)--> x_0 --`iterations` x (griffin_lim_step + overlap_add)--> wav [B, hop (T - 1)]

Fast Griffin-Lim with the momentum applied to the SIGNAL (the STFT is linear): y = x_n + alpha (x_n - x_n-1), x_n+1 = istft(|S| * Y / max(|Y|, 1e-8)) with
Y = stft(y); two signals are kept, never a previous spectrogram, and the complex spectrum of an iteration never leaves LDS.  The waveform is still
pre-emphasised: `audio.deemphasis` undoes that on the host before the samples are written."""
import ctypes
import hashlib
import math

import numpy as np
import torch

from . import _lib, audio, ops
from .hparams import overlay_settings, plain_block  # noqa: F401 (plain_block: for the callers that look for it here)

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


# ================================================================================================================================================
# Neural vocoder: the Parallel WaveGAN generator (Yamamoto et al. 2020), f32: the frozen inference path and, with trainable=True, the training forward
# and backward (DESIGN.md "Neural vocoder", "Training the Parallel WaveGAN generator").  The network, the launch plan and the noise contract are written
# down there; the checkpoint layout restates the most widely used implementation's names and is UNPINNED (no such checkpoint was at hand when this was
# written).  The state-dict finder, the weight-norm fold, the checked load and the Conv1d-default initialiser just below serve the generator and the
# discriminator (further down) alike.
# ================================================================================================================================================
PWG_DEFAULTS = {"Type": "PWG", "Checkpoint_Path": None, "Layers": 30, "Stacks": 3, "Residual_Channels": 64, "Gate_Channels": 128, "Skip_Channels": 64,
                "Aux_Context_Window": 2, "Upsample_Scales": [4, 4, 4, 4], "Precision": "f32"}
PWG_PRECISIONS = ("f32", "bf16")
PWG_TILE, PWG_MAX_CHANNELS, PWG_MAX_DILATION, PWG_MAX_SCALE, PWG_MAX_SCALES, PWG_MAX_CTX, PWG_LDS = 64, 256, 1024, 16, 8, 16, 160 * 1024


def lds_row_stride(K):
    """The stride in floats of an LDS row of K floats whose quarter is odd (`lds_stride_of` of csrc/device_common.h)"""
    return K if (K // 4) % 2 else K + 4


def pad32(K):
    """K rounded up to a multiple of 32: the k step of the bf16 MFMA (`pad32` of csrc/pwg_bf16_ops.hip)"""
    return (K + 31) // 32 * 32


def pwg_pack_bf16(w):
    """w [K, N] float32 (K-major: row = input channel) -> the bf16 image [Kp / 8, N, 8] of csrc/pwg_bf16_ops.hip: rounded to nearest even, zero rows from K to
    Kp = pad32(K); element (k, n) lies at [k // 8, n, k % 8], so a lane's eight k values of one column are 16 consecutive bytes."""
    K, N = w.shape
    p = torch.zeros(pad32(K), N, dtype=torch.bfloat16, device=w.device)
    p[:K] = w.to(torch.float32).to(torch.bfloat16)
    return p.view(-1, 8, N).permute(0, 2, 1).contiguous()


def pwg_unpack_bf16(image):
    """The inverse of `pwg_pack_bf16`: image [Kp / 8, N, 8] bf16 -> [Kp, N] float32 (the rounded weights, then the zero rows)"""
    return image.permute(0, 2, 1).reshape(-1, image.shape[1]).to(torch.float32)


def find_state_dict(obj, paths, mine, error):
    """The first dict for which `mine` holds among those that the key paths `paths` reach inside `obj` (what torch.load returned); none: ValueError(error)."""
    for path in paths:
        d = obj
        for k in path:
            d = d.get(k) if isinstance(d, dict) else None
        if isinstance(d, dict) and mine(d):
            return d
    raise ValueError(error)


def fold_weight_norm(sd, noun):
    """Folds the weight-norm pairs (`weight_g` / `weight_v`) of the state dict `sd` in place into plain `weight`s, in float64"""
    for kg in [k for k in sd if k.endswith(".weight_g")]:
        base = kg[:-len("_g")]
        if base + "_v" not in sd:
            raise ValueError(f"{noun} checkpoint: {kg} has no {base}_v beside it")
        if base in sd:
            raise ValueError(f"{noun} checkpoint: {base} is given both plain and in weight-norm form")
        g, v = sd.pop(kg).double(), sd.pop(base + "_v").double()
        norm = v.reshape(v.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (v.dim() - 1))
        sd[base] = v * (g.reshape(norm.shape) / norm)


def checked_load(found, want, noun, model, block):
    """-> {key: float32 host tensor} with exactly the keys of `want` (key -> shape) from the state dict `found` of a `model` (weight-norm pairs are folded
    once); a missing, surplus or wrongly shaped tensor raises a ValueError naming the key.  `noun` names the checkpoint, `block` the yaml block of the sizes."""
    sd = dict(found)
    fold_weight_norm(sd, noun)
    for k in want:
        if k not in sd:
            raise ValueError(f"{noun} checkpoint: missing key {k}")
    for k in sd:
        if k not in want:
            raise ValueError(f"{noun} checkpoint: surplus key {k} (not part of a {model} of the {block} block's sizes)")
    out = {}
    for k, shape in want.items():
        t = sd[k]
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            raise ValueError(f"{noun} checkpoint: {k} has shape {tuple(getattr(t, 'shape', ()))}, the {block} block's sizes need {shape}")
        out[k] = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
    return out


def conv_default_init(shapes, seed, constant=lambda k, shape: None):
    """A fresh state dict of the names and shapes `shapes`: torch.nn.Conv1d's default rule per tensor - uniform in +- 1 / sqrt(fan_in), weights and biases
    alike - drawn in the order of `shapes` on a host generator seeded with `seed`; a tensor that `constant(key, shape)` gives is taken as it is, undrawn."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for k, shape in shapes.items():
        sd[k] = constant(k, shape)
        if sd[k] is None:
            fan_in = math.prod(shapes[k[:-len("bias")] + "weight"][1:]) if k.endswith(".bias") else math.prod(shape[1:])
            sd[k] = (torch.rand(shape, generator=g, dtype=torch.float32) * 2.0 - 1.0) / math.sqrt(fan_in)
    return sd


def pwg_settings(hp):
    """The `Vocoder` block of the yaml over PWG_DEFAULTS (an absent block: the defaults)."""
    v = getattr(hp, "Vocoder", None)
    return {k: getattr(v, k, d) if v is not None else d for k, d in PWG_DEFAULTS.items()}


def pwg_geometry(hp):
    """The generator's sizes as a dict (layers, stacks, R, G, S, A, ctx, scales, hop, dilations, precision); raises ValueError naming the offending yaml keys
    when the kernels do not support them - the idiom of `geometry`."""
    v = pwg_settings(hp)
    precision = v["Precision"]
    if precision not in PWG_PRECISIONS:
        raise ValueError(f"Vocoder.Precision = {precision!r} must be 'f32' or 'bf16' (bf16: the layer launches' operands only, inference only)")
    if v["Type"] != "PWG":
        raise ValueError(f"Vocoder.Type = {v['Type']!r}: the Parallel WaveGAN generator needs Vocoder.Type: 'PWG' (a 'HiFiGAN' block describes the HiFi-GAN "
                         "generator, `HiFiGAN`; `make_vocoder` chooses between them)")
    layers, stacks, R, G, S, ctx = (int(v[k]) for k in ("Layers", "Stacks", "Residual_Channels", "Gate_Channels", "Skip_Channels", "Aux_Context_Window"))
    scales = [int(s) for s in v["Upsample_Scales"]]
    A, hop = int(hp.Sound.Mel_Dim), int(hp.Sound.Frame_Shift)
    if G != 2 * R:
        raise ValueError(f"Vocoder.Gate_Channels = {G} must be 2 * Vocoder.Residual_Channels = {2 * R} (the gate halves feed 1x1s of Residual_Channels inputs)")
    if R < 16 or R % 16 or R > PWG_MAX_CHANNELS:
        raise ValueError(f"Vocoder.Residual_Channels = {R} must be a multiple of 16 in [16, {PWG_MAX_CHANNELS}]")
    if S < 16 or S % 16 or S > PWG_MAX_CHANNELS:
        raise ValueError(f"Vocoder.Skip_Channels = {S} must be a multiple of 16 in [16, {PWG_MAX_CHANNELS}]")
    if A < 4 or A % 4 or A > PWG_MAX_CHANNELS:
        raise ValueError(f"Sound.Mel_Dim = {A} must be a multiple of 4 in [4, {PWG_MAX_CHANNELS}] for the neural vocoder (Vocoder block)")
    if layers < 1 or stacks < 1 or layers % stacks:
        raise ValueError(f"Vocoder.Layers = {layers} must be a positive multiple of Vocoder.Stacks = {stacks}")
    dilations = [2 ** (i % (layers // stacks)) for i in range(layers)]
    if max(dilations) > PWG_MAX_DILATION:
        raise ValueError(f"Vocoder.Layers = {layers} / Vocoder.Stacks = {stacks} gives dilations up to {max(dilations)}; at most {PWG_MAX_DILATION} is supported")
    if not 0 <= ctx <= PWG_MAX_CTX:
        raise ValueError(f"Vocoder.Aux_Context_Window = {ctx} must lie in [0, {PWG_MAX_CTX}]")
    if not 1 <= len(scales) <= PWG_MAX_SCALES or any(s < 1 or s > PWG_MAX_SCALE for s in scales):
        raise ValueError(f"Vocoder.Upsample_Scales = {scales}: 1 to {PWG_MAX_SCALES} scales, each in [1, {PWG_MAX_SCALE}]")
    if math.prod(scales) != hop:
        raise ValueError(f"Vocoder.Upsample_Scales = {scales} multiply to {math.prod(scales)}, Sound.Frame_Shift is {hop}: the vocoder must produce one hop per frame")
    K = 3 * R + A
    lds = 4 * PWG_TILE * (lds_row_stride(K) + (0 if R <= 64 else R + 4))
    if lds > PWG_LDS:
        raise ValueError(f"Vocoder.Residual_Channels = {R} with Sound.Mel_Dim = {A}: a layer's tile of {lds} bytes exceeds the {PWG_LDS} bytes of LDS")
    geo = {"layers": layers, "stacks": stacks, "R": R, "G": G, "S": S, "A": A, "ctx": ctx, "scales": scales, "hop": hop, "dilations": dilations,
           "precision": precision}
    if precision == "bf16":
        pwg_bf16_geometry(geo)
    return geo


def pwg_bf16_geometry(geo):
    """Raises ValueError naming the yaml keys when the bf16 layer kernel's LDS tile (`layer_bf16_lds_bytes` of csrc/pwg_bf16_ops.hip) does not fit."""
    R, A = geo["R"], geo["A"]
    lds = 2 * PWG_TILE * (pad32(3 * R + A) + 8 + pad32(R) + 8)
    if lds > PWG_LDS:
        raise ValueError(f"Vocoder.Precision = 'bf16' with Vocoder.Residual_Channels = {R} and Sound.Mel_Dim = {A}: a layer's bf16 tile of {lds} bytes exceeds the "
                         f"{PWG_LDS} bytes of LDS")


def pwg_seed_words(seed, label, k=0):
    """The vocoder's two 32-bit seed words of sample `k` of the utterance `label` under the run seed `seed`: the first 8 bytes of blake2b of
    "<seed> NUL <label> NUL <k> NUL pwg", little endian - distinct from the mel's words (`inferencer.utterance_seed_words`), so the two streams are unrelated."""
    d = hashlib.blake2b("{}\0{}\0{}\0pwg".format(seed, label, k).encode()).digest()
    return int.from_bytes(d[:4], "little"), int.from_bytes(d[4:8], "little")


def pwg_expected_shapes(geo):
    """state-dict key -> shape of the generator with the sizes `geo`"""
    R, G, S, A, ctx = geo["R"], geo["G"], geo["S"], geo["A"], geo["ctx"]
    e = {"first_conv.weight": (R, 1, 1), "first_conv.bias": (R,), "upsample_net.conv_in.weight": (A, A, 2 * ctx + 1)}
    for i, s in enumerate(geo["scales"]):
        e[f"upsample_net.upsample.up_layers.{2 * i + 1}.weight"] = (1, 1, 1, 2 * s + 1)
    for i in range(geo["layers"]):
        q = f"conv_layers.{i}."
        e.update({q + "conv.weight": (G, R, 3), q + "conv.bias": (G,), q + "conv1x1_aux.weight": (G, A, 1), q + "conv1x1_out.weight": (R, G // 2, 1),
                  q + "conv1x1_out.bias": (R,), q + "conv1x1_skip.weight": (S, G // 2, 1), q + "conv1x1_skip.bias": (S,)})
    e.update({"last_conv_layers.1.weight": (S, S, 1), "last_conv_layers.1.bias": (S,), "last_conv_layers.3.weight": (1, S, 1), "last_conv_layers.3.bias": (1,)})
    return e


def pwg_find_state_dict(obj):
    """The generator's state dict inside what torch.load returned: at the top level or under `generator` / `Generator`, possibly inside `model`."""
    return find_state_dict(obj, ((), ("generator",), ("Generator",), ("model",), ("model", "generator"), ("model", "Generator")),
                           lambda d: any(str(k).startswith("first_conv.") for k in d),
                           "no Parallel WaveGAN generator state dict found (looked for `first_conv.*` at the top level, under generator / Generator and inside model)")


def pwg_load(obj, geo):
    """-> {key: float32 host tensor} with exactly the keys of `pwg_expected_shapes`: weight-norm pairs are folded once, in float64 (`fold_weight_norm`);
    a missing, surplus or wrongly shaped tensor raises a ValueError naming the key (`checked_load`)."""
    return checked_load(pwg_find_state_dict(obj), pwg_expected_shapes(geo), "vocoder", "generator", "Vocoder")


def pwg_init(geo, seed=0):
    """A fresh generator's state dict (the names and shapes of `pwg_expected_shapes`, plain weights): `conv_default_init`; the FIR of scale s starts as the
    moving average 1 / (2 s + 1)."""
    return conv_default_init(pwg_expected_shapes(geo), seed, lambda k, shape: torch.full(shape, 1.0 / shape[-1], dtype=torch.float32) if ".up_layers." in k else None)


def pwg_train_geometry(geo):
    """Raises ValueError naming the yaml keys when the backward's LDS tiles (larger than the forward's) do not fit; construction with trainable=True only."""
    R, S, A = geo["R"], geo["S"], geo["A"]
    K = 3 * R + A
    gate, data = 4 * PWG_TILE * (lds_row_stride(K) + R + S + 4), 4 * PWG_TILE * (6 * R + 4)
    if max(gate, data) > PWG_LDS:
        raise ValueError(f"Vocoder.Residual_Channels = {R} with Vocoder.Skip_Channels = {S} and Sound.Mel_Dim = {A}: training needs tiles of {gate} and {data} "
                         f"bytes, more than the {PWG_LDS} bytes of LDS (inference supports these sizes, trainable=True does not)")


def pwg_condition_stages(voc, mels, lengths, c):
    """Fills c [B, L * hop, A] and returns the input of every upsampling scale (`stages[k]` [B, L * prod(scales[:k]), A]): the conditioning's own entry point
    run on prefixes of the scale list (the identity FIR of a scale 1 for conv_in's output), so every stage is the forward's bit for bit."""
    g = voc.geo
    B, A, L = mels.shape
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=mels.device)
    work = f(2 * B * L * A * max(g["hop"] // g["scales"][-1], 1))
    stages = [f(B, L, A)]
    ops.pwg_condition(mels, lengths, voc.w_in, torch.tensor([0.0, 1.0, 0.0], device=mels.device), (ctypes.c_int * 1)(1), work, stages[0], g["ctx"])
    mult = 1
    for k in range(1, len(g["scales"])):
        mult *= g["scales"][k - 1]
        stages.append(f(B, L * mult, A))
        ops.pwg_condition(mels, lengths, voc.w_in, voc.firs, (ctypes.c_int * k)(*g["scales"][:k]), work, stages[k], g["ctx"])
    ops.pwg_condition(mels, lengths, voc.w_in, voc.firs, voc.scales, work, c, g["ctx"])
    return stages


def pwg_condition_backward(voc, mels, lengths, stages, dc, work, grads):
    """d c [B, L * hop, A] -> the FIRs' and conv_in's gradients into `grads` (torch's layouts): `pwg_upsample_bwd` per scale, last to first, then `pwg_cond_in_bwd`."""
    g, lib, P, st = voc.geo, _lib.api(), _lib.ptr, _lib.stream()
    B, A, L = mels.shape
    dcur, mult, off = dc, g["hop"], sum(2 * s + 1 for s in g["scales"])
    for k in reversed(range(len(g["scales"]))):
        s = g["scales"][k]
        mult //= s
        off -= 2 * s + 1
        din = torch.empty(B, L * mult, A, dtype=torch.float32, device=mels.device)
        lib.glowtts_pwg_train_upsample_bwd(P(dcur), P(stages[k]), P(voc.firs[off:]), P(lengths), P(work), P(din),
                                           P(grads[f"upsample_net.upsample.up_layers.{2 * k + 1}.weight"]), B, A, L, mult, s, st)
        dcur = din
    lib.glowtts_pwg_train_cond_in_bwd(P(mels), P(dcur), P(lengths), P(grads["upsample_net.conv_in.weight"]), B, A, L, g["ctx"], st)


def pwg_train_forward(voc, mels, lengths, seeds, noises):
    """The inference forward's launches with every layer's input kept -> dict(wav, keep [Layers + 1, B, T, R], skips, c, stages): `stages[k]` is the input of
    upsampling scale k, recomputed by running the conditioning's own entry point on prefixes of the scale list (the identity FIR of a scale 1 for
    conv_in's output), so every stage is the forward's bit for bit."""
    g = voc.geo
    B, A, L = mels.shape
    T, dev = L * g["hop"], mels.device
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    keep, skips, c, wav = f(g["layers"] + 1, B, T, g["R"]), f(B, T, g["S"]), f(B, T, g["A"]), f(B, T)
    stages = pwg_condition_stages(voc, mels, lengths, c)
    ops.pwg_first(noises, seeds, lengths, *voc.first, keep[0], L, g["hop"])
    for i, (lw, d) in enumerate(zip(voc.layer_weights, g["dilations"])):
        ops.pwg_layer(keep[i], c, *lw, keep[i + 1], skips, lengths, L, g["hop"], d, i > 0)
    ops.pwg_head(skips, lengths, *voc.head, wav, L, g["hop"], math.sqrt(1.0 / g["layers"]))
    return {"wav": wav, "keep": keep, "skips": skips, "c": c, "stages": stages}


def pwg_train_backward(voc, mels, lengths, seeds, noises, fwd, dwav):
    """-> {name: gradient in torch's layout} for every name of `pwg_expected_shapes`, from what `pwg_train_forward` kept and d wav [B, T]."""
    g, lib = voc.geo, _lib.api()
    B, A, L = mels.shape
    hop, R, G, S = g["hop"], g["R"], g["G"], g["S"]
    T, dev, P, st = L * hop, mels.device, _lib.ptr, _lib.stream()
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    grads = {k: f(*shape) for k, shape in pwg_expected_shapes(g).items()}
    work = f(lib.glowtts_pwg_train_work_floats(B, L, hop, R, S, A))
    keep, skips, c = fwd["keep"], fwd["skips"], fwd["c"]
    dwav = dwav.to(torch.float32).contiguous()
    y, h, dh, dskips = f(B, T, S), f(B, T, S), f(B, T, S), f(B, T, S)
    w1, b1, w2, b2 = voc.head
    lib.glowtts_pwg_train_head_bwd(P(skips), P(lengths), P(w1), P(voc.head_w1t), P(b1), P(w2), P(dwav), P(y), P(h), P(dh), P(dskips), B, L, hop, S,
                                   math.sqrt(1.0 / g["layers"]), st)
    lib.glowtts_pwg_train_head_wgrad(P(y), P(h), P(dh), P(dwav), P(lengths), P(work), P(grads["last_conv_layers.1.weight"]),
                                     P(grads["last_conv_layers.1.bias"]), P(grads["last_conv_layers.3.weight"]), P(grads["last_conv_layers.3.bias"]), B, L, hop, S, st)
    del y, h, dh
    gate, dpre, dc = f(B, T, R), f(B, T, G), f(B, T, A)
    dxp, dx = torch.zeros(B, T, R, dtype=torch.float32, device=dev), f(B, T, R)        # nothing reads the last layer's x': its gradient is zero
    for i in reversed(range(g["layers"])):
        (lw1, lb1, _, _), (w2t, w1t, wauxt), d, q = voc.layer_weights[i], voc.layer_weights_t[i], g["dilations"][i], f"conv_layers.{i}."
        lib.glowtts_pwg_train_layer_bwd(P(keep[i]), P(c), P(lw1), P(lb1), P(w2t), P(w1t), P(wauxt), P(dxp), P(dskips), P(gate), P(dpre), P(dx), P(dc),
                                        P(lengths), B, L, hop, R, S, A, d, int(i == g["layers"] - 1), st)
        lib.glowtts_pwg_train_layer_wgrad(P(keep[i]), P(c), P(gate), P(dpre), P(dxp), P(dskips), P(lengths), P(work), P(grads[q + "conv.weight"]),
                                          P(grads[q + "conv.bias"]), P(grads[q + "conv1x1_aux.weight"]), P(grads[q + "conv1x1_out.weight"]),
                                          P(grads[q + "conv1x1_out.bias"]), P(grads[q + "conv1x1_skip.weight"]), P(grads[q + "conv1x1_skip.bias"]),
                                          B, L, hop, R, S, A, d, st)
        dxp, dx = dx, dxp
    lib.glowtts_pwg_train_first_bwd(P(noises), P(seeds), P(dxp), P(lengths), P(work), P(grads["first_conv.weight"]), P(grads["first_conv.bias"]), B, L, hop, R, st)
    pwg_condition_backward(voc, mels, lengths, fwd["stages"], dc, work, grads)
    grads["dx0"] = dxp
    return grads


class _Generate(torch.autograd.Function):
    """wav = ParallelWaveGAN.generate(...): forward and backward are HIP launches (csrc/pwg_ops.hip, csrc/pwg_train_ops.hip); the mel gets no gradient."""

    @staticmethod
    def forward(ctx, voc, mels, lengths, seeds, noises, *params):
        voc._build_images({k: t.detach() for k, t in zip(voc.params, params)})
        fwd = pwg_train_forward(voc, mels, lengths, seeds, noises)
        ctx.voc, ctx.args, ctx.fwd = voc, (mels, lengths, seeds, noises), fwd
        return fwd["wav"]

    @staticmethod
    def backward(ctx, dwav):
        grads = pwg_train_backward(ctx.voc, *ctx.args, ctx.fwd, dwav)
        ctx.fwd = None
        return (None,) * 5 + tuple(grads[k] for k in ctx.voc.params)


class ParallelWaveGAN:
    """ParallelWaveGAN(hp, device, state_dict=None)(mels [B, Mel, T], mel_lengths, seeds=None, noises=None) -> (wav [B, T * hop] fp32 on the device,
    wav_lengths [B] int64).  state_dict None: `Vocoder.Checkpoint_Path` is loaded.  seeds [B, 2] (integer words, `pwg_seed_words`): z[t] is the counter hash
    gauss(s0, s1, 0, t, 1) of csrc/gauss_hash.h evaluated in the first kernel; noises [B, T * hop]: the caller's z; neither: torch.randn on the device.
    An utterance's waveform is bit-identical alone, in any batch, at any padding and from run to run (given its z).
    precision 'f32' / 'bf16' / None (the yaml's `Vocoder.Precision`, default 'f32'), readable as `.precision`: 'bf16' runs the layer launches with bf16 operands
    (csrc/pwg_bf16_ops.hip; DESIGN.md "bf16 inference mode" has the contract) - inference only: with trainable=True an explicit 'bf16' raises and the yaml's
    key is ignored (training is f32).
    trainable=True (DESIGN.md "Training the Parallel WaveGAN generator"): `params` holds float32 device leaves in `pwg_expected_shapes`' names - from
    `state_dict` or, without one, `pwg_init(geo, seed)` - and `generate` returns the same waveform with a backward (csrc/pwg_train_ops.hip)."""

    def __init__(self, hp, device="cuda:0", state_dict=None, trainable=False, seed=0, precision=None):
        self.geo = geo = pwg_geometry(hp)                           # before anything touches the device or the disk
        self.trainable = bool(trainable)
        if precision is not None and precision not in PWG_PRECISIONS:
            raise ValueError(f"precision = {precision!r} must be 'f32', 'bf16' or None (None: Vocoder.Precision of the yaml)")
        if self.trainable and precision == "bf16":
            raise ValueError("precision = 'bf16' with trainable=True: the bf16 mode is inference only, training stays f32")
        # the argument over the yaml's key; a trainable generator is f32 whatever the yaml says (the key is a serving setting)
        self.precision = "f32" if self.trainable else precision or geo["precision"]
        if self.precision == "bf16":
            pwg_bf16_geometry(geo)
        self.geo = geo = dict(geo, precision=self.precision)        # the precision that runs
        if self.trainable:
            pwg_train_geometry(geo)
        if state_dict is None and self.trainable:
            state_dict = pwg_init(geo, seed)
        if state_dict is None:
            path = pwg_settings(hp)["Checkpoint_Path"]
            if not path:
                raise ValueError("Vocoder.Checkpoint_Path is not set: the neural vocoder needs a Parallel WaveGAN generator checkpoint")
            state_dict = torch.load(path, map_location="cpu")
        w = pwg_load(state_dict, geo)
        supported = _lib.api().glowtts_pwg_supported_bf16 if self.precision == "bf16" else _lib.api().glowtts_pwg_supported
        if not supported(geo["R"], geo["G"], geo["S"], geo["A"], max(geo["dilations"])):
            raise ValueError(f"the Vocoder block's sizes {geo} are not supported by the kernels")
        self._layer_op = ops.pwg_layer_bf16 if self.precision == "bf16" else ops.pwg_layer
        self.device = torch.device(device)
        self.sample_rate, self.n_mel, self.hop = int(hp.Sound.Sample_Rate), geo["A"], geo["hop"]
        self.scales = (ctypes.c_int * len(geo["scales"]))(*geo["scales"])
        self._capacity, self._buffers = 0, None
        if self.trainable:                                          # float32 device leaves in pwg_expected_shapes' names; the images follow them (`_build_images`)
            self.params = {k: t.to(self.device).requires_grad_(True) for k, t in w.items()}
            w = {k: t.detach() for k, t in self.params.items()}
        self._build_images(w)

    def _build_images(self, w):
        """The weight images in the kernels' layouts (K-major: the MFMA B operand reads 16 consecutive output channels of one input row) from the tensors `w`
        (host or device): built once for a frozen generator; a trainable one rebuilds them on the device at every `generate`, with the transposed images of
        the backward.  precision 'bf16': the layers' two matrices are the packed bf16 images of `pwg_pack_bf16` instead (biases stay float32)."""
        geo = self.geo
        image = pwg_pack_bf16 if self.precision == "bf16" else lambda t: t
        dev = lambda t: t.contiguous().to(self.device)
        self.w_in = dev(w["upsample_net.conv_in.weight"].permute(2, 1, 0).reshape(-1, geo["A"]))
        self.firs = dev(torch.cat([w[f"upsample_net.upsample.up_layers.{2 * i + 1}.weight"].reshape(-1) for i in range(len(geo["scales"]))]))
        self.first = (dev(w["first_conv.weight"].reshape(-1)), dev(w["first_conv.bias"]))
        self.layer_weights = []
        for i in range(geo["layers"]):
            q = f"conv_layers.{i}."
            w1 = torch.cat([w[q + "conv.weight"].permute(2, 1, 0).reshape(3 * geo["R"], geo["G"]), w[q + "conv1x1_aux.weight"][:, :, 0].t()], dim=0)
            w2 = torch.cat([w[q + "conv1x1_out.weight"][:, :, 0].t(), w[q + "conv1x1_skip.weight"][:, :, 0].t()], dim=1)
            b2 = torch.cat([w[q + "conv1x1_out.bias"], w[q + "conv1x1_skip.bias"]])
            self.layer_weights.append((dev(image(w1)), dev(w[q + "conv.bias"]), dev(image(w2)), dev(b2)))
        self.head = (dev(w["last_conv_layers.1.weight"][:, :, 0].t()), dev(w["last_conv_layers.1.bias"]), dev(w["last_conv_layers.3.weight"].reshape(-1)),
                     dev(w["last_conv_layers.3.bias"]))
        if self.trainable:
            R, G = geo["R"], geo["G"]
            self.layer_weights_t = [(dev(w2.t()), dev(w1[:3 * R].view(3, R, G).permute(0, 2, 1).reshape(3 * G, R)), dev(w1[3 * R:].t()))
                                    for w1, _, w2, _ in self.layer_weights]
            self.head_w1t = dev(w["last_conv_layers.1.weight"][:, :, 0])

    def _refresh(self):
        """A trainable generator's images follow its parameters: rebuilt before every call that reads them (an optimizer step writes the leaves in place)."""
        if self.trainable:
            self._build_images({k: t.detach() for k, t in self.params.items()})

    def _work(self, B, L):
        """Work buffers of a call (the two x, skips, c, the conditioning's intermediates): views of ONE set sized for the largest B x L (rounded up to
        T_BUCKET frames) seen so far, like `GriffinLim._work`.  The kernels honour the lengths and write every row they later read."""
        g = self.geo
        frames = B * (-(-L // T_BUCKET) * T_BUCKET)
        if frames > self._capacity:
            self._buffers = None
            f = lambda n: torch.empty(n, dtype=torch.float32, device=self.device)
            rows = frames * g["hop"]
            self._buffers = {"x": [f(rows * g["R"]), f(rows * g["R"])], "skips": f(rows * g["S"]), "c": f(rows * g["A"]),
                             "cond": f(2 * frames * g["A"] * (g["hop"] // g["scales"][-1]))}
            self._capacity = frames
        T, bf = L * g["hop"], self._buffers
        return {"x": [v[:B * T * g["R"]].view(B, T, g["R"]) for v in bf["x"]], "skips": bf["skips"][:B * T * g["S"]].view(B, T, g["S"]),
                "c": bf["c"][:B * T * g["A"]].view(B, T, g["A"]), "cond": bf["cond"][:2 * B * L * g["A"] * (g["hop"] // g["scales"][-1])]}

    def _lengths(self, lengths, B, L):
        n = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int32).reshape(B).contiguous()
        return n.clamp(min=0, max=L)

    def condition(self, mels, mel_lengths, out=None, work=None):
        """mels [B, Mel, L] -> the conditioning rows c [B, L * hop, Mel] (rows beyond an utterance's own L * hop are not written)."""
        if not mels.is_cuda:
            raise _lib.GlowTTSHipError("expected a device tensor (the HIP path has no CPU fallback)")
        self._refresh()
        mels = mels.to(device=self.device, dtype=torch.float32).contiguous()
        B, Mel, L = mels.shape
        if Mel != self.n_mel:
            raise ValueError(f"mels have {Mel} channels, Sound.Mel_Dim = {self.n_mel}")
        g = self.geo
        c = out if out is not None else torch.zeros(B, L * g["hop"], Mel, dtype=torch.float32, device=self.device)
        work = work if work is not None else torch.empty(2 * B * L * Mel * (g["hop"] // g["scales"][-1]), dtype=torch.float32, device=self.device)
        ops.pwg_condition(mels, self._lengths(mel_lengths, B, L), self.w_in, self.firs, self.scales, work, c, g["ctx"])
        return c

    def layer(self, i, x, c, x_out, skips, frame_lengths, accumulate=True):
        """Layer i alone on rows x [B, T, R], c [B, T, A] -> x_out, skips (tests)."""
        self._refresh()
        B, T, _ = x.shape
        L = T // self.geo["hop"]
        self._layer_op(x, c, *self.layer_weights[i], x_out, skips, self._lengths(frame_lengths, B, L), L, self.geo["hop"], self.geo["dilations"][i], accumulate)

    @torch.no_grad()
    def __call__(self, mels, mel_lengths, seeds=None, noises=None):
        if seeds is not None and noises is not None:
            raise ValueError("`seeds` and `noises` both given: the noise is either drawn in the kernel from the seed words or the caller's")
        g = self.geo
        B, _, L = mels.shape
        T = L * g["hop"]
        wk = self._work(B, L)
        c = self.condition(mels, mel_lengths, out=wk["c"], work=wk["cond"])
        lengths = self._lengths(mel_lengths, B, L)
        if seeds is not None:
            from .alignment import seed_words
            seeds = seed_words(seeds, B, self.device)
        else:
            if noises is None:
                noises = torch.randn(B, T, dtype=torch.float32, device=self.device)
            noises = noises.to(device=self.device, dtype=torch.float32).reshape(B, -1).contiguous()
            if tuple(noises.shape) != (B, T):
                raise ValueError(f"noises have shape {tuple(noises.shape)}, expected {(B, T)} (or [B, 1, T])")
        x, xn = wk["x"]
        ops.pwg_first(noises, seeds, lengths, *self.first, x, L, g["hop"])
        for i, (lw, d) in enumerate(zip(self.layer_weights, g["dilations"])):
            self._layer_op(x, c, *lw, xn, wk["skips"], lengths, L, g["hop"], d, i > 0)
            x, xn = xn, x
        wav = torch.empty(B, T, dtype=torch.float32, device=self.device)
        ops.pwg_head(wk["skips"], lengths, *self.head, wav, L, g["hop"], math.sqrt(1.0 / g["layers"]))
        return wav, lengths.to(torch.int64) * g["hop"]

    def generate(self, mels, mel_lengths, seeds=None, noises=None):
        """The training forward: `__call__`'s arithmetic term for term (the same launches, so the waveform is bit-identical) -> (wav [B, T * hop], wav_lengths)
        with a backward that fills `.grad` of every tensor of `self.params`.  Only for `trainable=True`."""
        if not self.trainable:
            raise _lib.GlowTTSHipError("ParallelWaveGAN.generate needs a generator constructed with trainable=True (this one holds frozen weight images only)")
        if seeds is not None and noises is not None:
            raise ValueError("`seeds` and `noises` both given: the noise is either drawn in the kernel from the seed words or the caller's")
        if not mels.is_cuda:
            raise _lib.GlowTTSHipError("expected a device tensor (the HIP path has no CPU fallback)")
        mels = mels.to(device=self.device, dtype=torch.float32).contiguous()
        B, Mel, L = mels.shape
        if Mel != self.n_mel:
            raise ValueError(f"mels have {Mel} channels, Sound.Mel_Dim = {self.n_mel}")
        T = L * self.geo["hop"]
        lengths = self._lengths(mel_lengths, B, L)
        if seeds is not None:
            from .alignment import seed_words
            seeds = seed_words(seeds, B, self.device)
        else:
            if noises is None:
                noises = torch.randn(B, T, dtype=torch.float32, device=self.device)
            noises = noises.to(device=self.device, dtype=torch.float32).reshape(B, -1).contiguous()
            if tuple(noises.shape) != (B, T):
                raise ValueError(f"noises have shape {tuple(noises.shape)}, expected {(B, T)} (or [B, 1, T])")
        names = list(self.params)
        wav = _Generate.apply(self, mels, lengths, seeds, noises, *[self.params[k] for k in names])
        return wav, lengths.to(torch.int64) * self.geo["hop"]

    def to_host(self, wav, wav_lengths):
        """Device waveforms -> list of float32 numpy arrays clipped to [-1, 1] (what `audio.write_wav` takes).  No de-emphasis: the vocoder was trained on
        final audio."""
        wav, n = wav.cpu().numpy(), wav_lengths.cpu().tolist()
        return [np.clip(w[:m], -1.0, 1.0).astype(np.float32) for w, m in zip(wav, n)]


# ================================================================================================================================================
# Multi-resolution STFT loss (Yamamoto et al. 2020, eq. 4-6) on the kernels of csrc/stft_loss_ops.hip: stage one of the Parallel WaveGAN recipe trains the
# generator with it alone.  The contract is frozen in DESIGN.md ("STFT loss"); tests/pwg_train_ref.py restates it with the library STFT.
# ================================================================================================================================================
STFT_RESOLUTIONS = [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)]            # (n_fft, hop, win); the recipe's, restated from memory: this project's contract
STFT_KEY = "Vocoder.Train.STFT_Resolutions"


def stft_loss_geometry(resolutions=None, T=None):
    """[(n_fft, hop, win), ...] as ints; raises ValueError naming the yaml keys when the kernels do not support a resolution or, with `T` given, when the
    segment of T samples is too short for its reflect padding."""
    res = STFT_RESOLUTIONS if resolutions is None else resolutions
    try:
        res = [tuple(int(v) for v in r) for r in res]
    except (TypeError, ValueError):
        res = None
    if not res or any(len(r) != 3 for r in res):
        raise ValueError(f"{STFT_KEY} must be a non-empty list of [n_fft, hop, win] triples, got {resolutions!r}")
    for n_fft, hop, win in res:
        if n_fft < 256 or n_fft > 4096 or n_fft & (n_fft - 1):
            raise ValueError(f"{STFT_KEY}: n_fft = {n_fft} of {[n_fft, hop, win]} must be a power of two in [256, 4096]")
        if win < 1 or win > n_fft:
            raise ValueError(f"{STFT_KEY}: win = {win} of {[n_fft, hop, win]} must lie in [1, n_fft = {n_fft}]")
        if hop < 1 or hop > win:
            raise ValueError(f"{STFT_KEY}: hop = {hop} of {[n_fft, hop, win]} must lie in [1, win = {win}] (every sample is covered by a frame)")
        if T is not None and T <= n_fft // 2:
            raise ValueError(f"{STFT_KEY}: n_fft = {n_fft} of {[n_fft, hop, win]} needs segments longer than n_fft / 2 = {n_fft // 2} samples for its reflect "
                             f"padding, got {T} (Vocoder.Train.Segment_Frames * Sound.Frame_Shift)")
    return res


def stft_loss_forward(loss_fn, pred, target):
    """The forward launches of every resolution -> (loss [1], terms [n, 3] = (L_sc, L_mag, the backward's coefficient) per resolution, keeps): the entry
    points' own outputs, for `_STFTLoss` and the tests."""
    B, T = pred.shape
    L, dev, n = _lib.api(), pred.device, len(loss_fn.resolutions)
    loss, terms, keeps = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(n, 3, dtype=torch.float32, device=dev), []
    for i, ((n_fft, hop, win), (window, twiddle)) in enumerate(zip(loss_fn.resolutions, loss_fn.tables)):
        keep = torch.empty(L.glowtts_stft_loss_keep_floats(B, T, n_fft, hop), dtype=torch.float32, device=dev)
        work = loss_fn._work(L.glowtts_stft_loss_work_floats(B, T, win, hop))
        L.glowtts_stft_loss_forward(_lib.ptr(pred), _lib.ptr(target), _lib.ptr(window), _lib.ptr(twiddle), _lib.ptr(keep), _lib.ptr(work),
                                    _lib.ptr(terms[i]), _lib.ptr(loss), B, T, n_fft, win, hop, 1.0 / n, int(i > 0), _lib.stream())
        keeps.append(keep)
    return loss, terms, keeps


def stft_loss_backward(loss_fn, keeps, terms, grad_out, B, T):
    """The backward launches of every resolution -> d pred [B, T] = grad_out * dL/dpred (grad_out: one device float)."""
    L, dev, n = _lib.api(), terms.device, len(loss_fn.resolutions)
    dpred = torch.empty(B, T, dtype=torch.float32, device=dev)
    for i, ((n_fft, hop, win), (window, twiddle)) in enumerate(zip(loss_fn.resolutions, loss_fn.tables)):
        work = loss_fn._work(L.glowtts_stft_loss_work_floats(B, T, win, hop))
        L.glowtts_stft_loss_backward(_lib.ptr(keeps[i]), _lib.ptr(terms[i]), _lib.ptr(grad_out), _lib.ptr(window), _lib.ptr(twiddle), _lib.ptr(work),
                                     _lib.ptr(dpred), B, T, n_fft, win, hop, 1.0 / n, int(i > 0), _lib.stream())
    return dpred


class _STFTLoss(torch.autograd.Function):
    """loss = MultiResolutionSTFTLoss(pred, target): forward and backward are the HIP launches of csrc/stft_loss_ops.hip; the target gets no gradient."""

    @staticmethod
    def forward(ctx, loss_fn, pred, target):
        loss, terms, keeps = stft_loss_forward(loss_fn, pred, target)
        ctx.loss_fn, ctx.keeps, ctx.terms, ctx.shape = loss_fn, keeps, terms, tuple(pred.shape)
        loss_fn.terms = terms[:, :2]
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dpred = stft_loss_backward(ctx.loss_fn, ctx.keeps, ctx.terms, g.to(torch.float32).reshape(1).contiguous(), *ctx.shape)
        ctx.keeps = None
        return None, dpred, None


class MultiResolutionSTFTLoss:
    """MultiResolutionSTFTLoss(resolutions=None, device)(pred [B, T], target [B, T]) -> the scalar loss, the mean over the resolutions of
    L_sc + L_mag, with a backward that yields d pred (a second loss term of the caller's adds into the same tensor through autograd).  `.terms` [n, 2]
    holds (L_sc, L_mag) per resolution of the last call.  Every row is of the full length T: training segments are of one length, so `lengths` that
    differ from T raise.  Bit-identical from run to run."""

    def __init__(self, resolutions=None, device="cuda:0"):
        self.resolutions = stft_loss_geometry(resolutions)         # before anything touches the device
        self.device = torch.device(device)
        self.tables = []
        for n_fft, hop, win in self.resolutions:
            tw, w = fft_tables(n_fft, win)
            self.tables.append(tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device) for a in (w, tw)))
        self.terms, self._scratch = None, None

    def _work(self, floats):
        """One scratch buffer (the frames' sums, the backward's frame gradients) that grows to the largest request; a launch rewrites what it later reads."""
        if self._scratch is None or self._scratch.numel() < floats:
            self._scratch = None
            self._scratch = torch.empty(floats, dtype=torch.float32, device=self.device)
        return self._scratch

    def __call__(self, pred, target, lengths=None):
        if pred.dim() != 2 or tuple(pred.shape) != tuple(target.shape):
            raise ValueError(f"MultiResolutionSTFTLoss: expected pred and target [B, T] of one shape, got {list(pred.shape)} and {list(target.shape)}")
        if pred.dtype != torch.float32 or target.dtype != torch.float32 or not pred.is_cuda or not target.is_cuda:
            raise _lib.GlowTTSHipError("MultiResolutionSTFTLoss: expected fp32 device tensors (the HIP path has no CPU fallback)")
        B, T = pred.shape
        if lengths is not None and any(int(n) != T for n in torch.as_tensor(lengths).reshape(-1).tolist()):
            raise ValueError(f"MultiResolutionSTFTLoss: ragged input (lengths {torch.as_tensor(lengths).reshape(-1).tolist()} of T = {T}): every row must be of "
                             "the full length, training segments are of one length (Vocoder.Train.Segment_Frames)")
        stft_loss_geometry(self.resolutions, T)
        if B < 1 or B > 65535 or B * T >= 2 ** 31:
            raise ValueError(f"MultiResolutionSTFTLoss: batch of {B} x {T} samples is outside 1 <= B <= 65535, B T < 2^31 (Vocoder.Train.Batch_Size)")
        return _STFTLoss.apply(self, pred.contiguous(), target.detach().contiguous())


# ================================================================================================================================================
# Mel-spectrogram L1 loss (Kong et al. 2020, eq. 5; the 45 L_mel of the HiFi-GAN generator loss) on the kernels of csrc/mel_loss_ops.hip.  The contract
# is this project's own, in DESIGN.md ("Mel loss"); tests/mel_loss_ref.py restates it with the library STFT.  The class is Lambda-free: the trainer scales.
# ================================================================================================================================================
MEL_KEY = "Vocoder.Train.Mel_Loss"
MEL_LAMBDA, MEL_FLOOR = 45.0, 1.0e-5
MEL_MIN_FILTERS, MEL_MAX_FILTERS = 4, 256


def mel_loss_settings(hp):
    """The optional yaml block `Vocoder.Train.Mel_Loss` over its defaults {Lambda: 45.0, Floor: 1.0e-5, Mel_F_Min / Mel_F_Max: Sound's}, checked: a
    ValueError names every unknown or bad key as Vocoder.Train.Mel_Loss.<key>.  An absent block gives the defaults: whether the term is trained with is
    the caller's decision (`pwg_trainer.train_settings` keeps the key only when the yaml has it)."""
    block = getattr(getattr(getattr(hp, "Vocoder", None), "Train", None), "Mel_Loss", None)
    defaults = {"Lambda": MEL_LAMBDA, "Floor": MEL_FLOOR, "Mel_F_Min": hp.Sound.Mel_F_Min, "Mel_F_Max": hp.Sound.Mel_F_Max}

    def rules(s, need):
        for k in ("Lambda", "Floor"):
            need(k, lambda v: not isinstance(v, bool) and 0 < float(v) < float("inf"), "positive")
        need("Mel_F_Min", lambda v: not isinstance(v, bool) and 0 <= float(v) < float("inf"), "at least 0")
        need("Mel_F_Max", lambda v: not isinstance(v, bool) and float(v) > float(s["Mel_F_Min"]), "above Mel_F_Min")
    return overlay_settings(block, defaults, MEL_KEY, "vocoder", rules)


def mel_loss_geometry(hp, block=None, T=None):
    """The analysis geometry of the mel loss: {n_fft, hop, win, mel, sample_rate, f_min, f_max, floor} from hp.Sound and the settings `block`
    (`mel_loss_settings`' result; None: that of hp).  Raises ValueError naming the yaml key when the kernels do not support a size, when a filter of the
    filterbank is empty or, with `T` given, when the segment of T samples is too short for the reflect padding.  Touches no device."""
    s = hp.Sound
    block = mel_loss_settings(hp) if block is None else block
    n_fft, win, hop, mel = (int(s.Spectrogram_Dim) - 1) * 2, int(s.Frame_Length), int(s.Frame_Shift), int(s.Mel_Dim)
    if n_fft < 256 or n_fft > 4096 or n_fft & (n_fft - 1):
        raise ValueError(f"Sound.Spectrogram_Dim = {s.Spectrogram_Dim}: the mel loss needs n_fft = 2 * (Spectrogram_Dim - 1) to be a power of two in [256, 4096], "
                         f"got {n_fft}")
    if win < 1 or win > n_fft:
        raise ValueError(f"Sound.Frame_Length = {win} must lie in [1, n_fft = {n_fft}] (Sound.Spectrogram_Dim = {s.Spectrogram_Dim})")
    if hop < 1 or hop > win:
        raise ValueError(f"Sound.Frame_Shift = {hop} must lie in [1, Sound.Frame_Length = {win}] (every sample is covered by a frame)")
    if mel < MEL_MIN_FILTERS or mel > MEL_MAX_FILTERS:
        raise ValueError(f"Sound.Mel_Dim = {mel} must lie in [{MEL_MIN_FILTERS}, {MEL_MAX_FILTERS}] (one thread of the mel loss's workgroup per filter)")
    floor, f_min, f_max, rate = float(block["Floor"]), float(block["Mel_F_Min"]), float(block["Mel_F_Max"]), int(s.Sample_Rate)
    if not floor > 0:
        raise ValueError(f"{MEL_KEY}.Floor = {block['Floor']} must be positive")
    if not 0 <= f_min < f_max <= rate / 2:
        raise ValueError(f"{MEL_KEY}.Mel_F_Min = {f_min:g} and {MEL_KEY}.Mel_F_Max = {f_max:g} (absent: Sound's) must satisfy 0 <= Mel_F_Min < Mel_F_Max <= "
                         f"Sound.Sample_Rate / 2 = {rate / 2:g}")
    empty = np.flatnonzero(~audio.mel_filterbank(rate, n_fft, mel, f_min, f_max).any(axis=1))
    if empty.size:
        raise ValueError(f"Sound.Mel_Dim = {mel} filters between {MEL_KEY}.Mel_F_Min = {f_min:g} and {MEL_KEY}.Mel_F_Max = {f_max:g} (absent: Sound's) leave filter "
                         f"{int(empty[0])} without a bin at n_fft = {n_fft} (Sound.Spectrogram_Dim): fewer filters or a wider band")
    if T is not None and T <= n_fft // 2:
        raise ValueError(f"{MEL_KEY}: n_fft = {n_fft} (Sound.Spectrogram_Dim) needs segments longer than n_fft / 2 = {n_fft // 2} samples for its reflect "
                         f"padding, got {T} (Vocoder.Train.Segment_Frames * Sound.Frame_Shift)")
    return {"n_fft": n_fft, "hop": hop, "win": win, "mel": mel, "sample_rate": rate, "f_min": f_min, "f_max": f_max, "floor": floor}


def transposed_filterbank(index, weights, n_freq):
    """The sparse filterbank of `frontend.sparse_filterbank` read by bin (CSR): (start [n_freq + 1] int32, filter [n] int32, weights [n]) - bin k's
    entries are start[k] .. start[k + 1], its filters in ascending order.  Every entry of `weights` appears once (zeros inside a run included)."""
    count = index[:, 1].astype(np.int64)
    filt = np.repeat(np.arange(index.shape[0], dtype=np.int64), count)
    bins = np.concatenate([np.arange(f, f + c) for f, c in zip(index[:, 0].astype(np.int64), count)] or [np.zeros(0, np.int64)])
    order = np.lexsort((filt, bins))                                   # by bin, then by filter
    start = np.zeros(n_freq + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(bins, minlength=n_freq))
    return start, filt[order].astype(np.int32), np.ascontiguousarray(np.asarray(weights)[:filt.size][order])


def mel_loss_forward(loss_fn, pred, target):
    """The forward launches -> (loss [1] = L_mel, terms [1], keep [B frames Mel]): the entry point's own outputs, for `_MelLoss` and the tests."""
    B, T = pred.shape
    g, L, dev = loss_fn.geo, _lib.api(), pred.device
    loss, terms = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
    keep = torch.empty(L.glowtts_mel_loss_keep_floats(B, T, g["hop"], g["mel"]), dtype=torch.float32, device=dev)
    work = loss_fn._work(L.glowtts_mel_loss_work_floats(B, T, g["win"], g["hop"]))
    L.glowtts_mel_loss_forward(_lib.ptr(pred), _lib.ptr(target), _lib.ptr(loss_fn.window), _lib.ptr(loss_fn.twiddle), _lib.ptr(loss_fn.fb_index),
                               _lib.ptr(loss_fn.fb_weights), _lib.ptr(keep), _lib.ptr(work), _lib.ptr(terms), _lib.ptr(loss), B, T, g["n_fft"], g["win"], g["hop"],
                               g["mel"], loss_fn.fb_weights.numel(), g["floor"], 1.0, 0, _lib.stream())
    return loss, terms, keep


def mel_loss_backward(loss_fn, pred, keep, grad_out):
    """The backward launches -> d pred [B, T] = grad_out * dL_mel/dpred (grad_out: one device float; pred: the forward's)."""
    B, T = pred.shape
    g, L = loss_fn.geo, _lib.api()
    dpred = torch.empty(B, T, dtype=torch.float32, device=pred.device)
    work = loss_fn._work(L.glowtts_mel_loss_work_floats(B, T, g["win"], g["hop"]))
    L.glowtts_mel_loss_backward(_lib.ptr(pred), _lib.ptr(keep), _lib.ptr(grad_out), _lib.ptr(loss_fn.window), _lib.ptr(loss_fn.twiddle), _lib.ptr(loss_fn.fbt_start),
                                _lib.ptr(loss_fn.fbt_filter), _lib.ptr(loss_fn.fbt_weights), _lib.ptr(work), _lib.ptr(dpred), B, T, g["n_fft"], g["win"], g["hop"],
                                g["mel"], loss_fn.fbt_weights.numel(), 1.0, 0, _lib.stream())
    return dpred


class _MelLoss(torch.autograd.Function):
    """loss = MelSpectrogramLoss(pred, target): forward and backward are the HIP launches of csrc/mel_loss_ops.hip; the target gets no gradient."""

    @staticmethod
    def forward(ctx, loss_fn, pred, target):
        loss, terms, keep = mel_loss_forward(loss_fn, pred, target)
        ctx.loss_fn, ctx.keep, ctx.pred = loss_fn, keep, pred          # (the backward takes the prediction's spectrum again: nothing of it was kept)
        loss_fn.term = terms[0]
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dpred = mel_loss_backward(ctx.loss_fn, ctx.pred, ctx.keep, g.to(torch.float32).reshape(1).contiguous())
        ctx.keep = ctx.pred = None
        return None, dpred, None


class MelSpectrogramLoss:
    """MelSpectrogramLoss(hp, device, settings=None)(pred [B, T], target [B, T]) -> the scalar L_mel = mean |ln mel(target) - ln mel(pred)| at the analysis
    geometry of hp.Sound (`mel_loss_geometry`; settings: `mel_loss_settings`' result, None: that of hp), with a backward that yields d pred.  Lambda-free: the
    trainer scales the term.  `.term` holds the last value.  Every row is of the full length T.  Bit-identical from run to run."""

    def __init__(self, hp, device="cuda:0", settings=None):
        from .frontend import sparse_filterbank                    # (frontend imports this module)
        self.settings = mel_loss_settings(hp) if settings is None else settings
        g = self.geo = mel_loss_geometry(hp, self.settings)        # before anything touches the device
        self.device = torch.device(device)
        tw, w = fft_tables(g["n_fft"], g["win"])
        index, weights = sparse_filterbank(audio.mel_filterbank(g["sample_rate"], g["n_fft"], g["mel"], g["f_min"], g["f_max"]))
        start, filt, wt = transposed_filterbank(index, weights, g["n_fft"] // 2 + 1)
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        self.twiddle, self.window = to(tw, np.float32), to(w, np.float32)
        self.fb_index, self.fb_weights = to(index, np.int32), to(weights, np.float32)
        self.fbt_start, self.fbt_filter, self.fbt_weights = to(start, np.int32), to(filt, np.int32), to(wt, np.float32)
        self.term, self._scratch = None, None

    _work = MultiResolutionSTFTLoss._work

    def __call__(self, pred, target, lengths=None):
        if pred.dim() != 2 or tuple(pred.shape) != tuple(target.shape):
            raise ValueError(f"MelSpectrogramLoss: expected pred and target [B, T] of one shape, got {list(pred.shape)} and {list(target.shape)}")
        if pred.dtype != torch.float32 or target.dtype != torch.float32 or not pred.is_cuda or not target.is_cuda:
            raise _lib.GlowTTSHipError("MelSpectrogramLoss: expected fp32 device tensors (the HIP path has no CPU fallback)")
        B, T = pred.shape
        if lengths is not None and any(int(n) != T for n in torch.as_tensor(lengths).reshape(-1).tolist()):
            raise ValueError(f"MelSpectrogramLoss: ragged input (lengths {torch.as_tensor(lengths).reshape(-1).tolist()} of T = {T}): every row must be of "
                             "the full length, training segments are of one length (Vocoder.Train.Segment_Frames)")
        if T <= self.geo["n_fft"] // 2:
            raise ValueError(f"{MEL_KEY}: n_fft = {self.geo['n_fft']} (Sound.Spectrogram_Dim) needs segments longer than n_fft / 2 = {self.geo['n_fft'] // 2} samples "
                             f"for its reflect padding, got {T} (Vocoder.Train.Segment_Frames * Sound.Frame_Shift)")
        if B < 1 or B > 65535 or B * T >= 2 ** 31:
            raise ValueError(f"MelSpectrogramLoss: batch of {B} x {T} samples is outside 1 <= B <= 65535, B T < 2^31 (Vocoder.Train.Batch_Size)")
        return _MelLoss.apply(self, pred.contiguous(), target.detach().contiguous())


# ================================================================================================================================================
# The Parallel WaveGAN discriminator and the least-squares adversarial loss on the kernels of csrc/pwg_disc_ops.hip: stage two of the recipe.  The
# contract (DESIGN.md "Training the Parallel WaveGAN discriminator") restates the most widely used implementation from memory and is UNPINNED.
# ================================================================================================================================================
DISC_KEY = "Vocoder.Train.Discriminator"
DISC_DEFAULTS = {"Start_Step": 100000, "Lambda_Adversarial": 4.0, "Learning_Rate": 5.0e-5, "Epsilon": 1.0e-6, "Gradient_Norm": 1.0,
                 "Learning_Rate_Decay": {"Step": 200000, "Gamma": 0.5}, "Layers": 10, "Channels": 64, "Negative_Slope": 0.2}
DISC_MAX_LAYERS = 16


def pwg_disc_settings(hp):
    """The optional yaml block `Vocoder.Train.Discriminator` over DISC_DEFAULTS (absent block: None), checked: a ValueError names every unknown or bad key."""
    block = getattr(getattr(getattr(hp, "Vocoder", None), "Train", None), "Discriminator", None)
    if block is None:
        return None
    whole = lambda v: int(v) == v

    def rules(s, need):
        need("Start_Step", lambda v: whole(v) and int(v) >= 0, "an integer, at least 0")
        need("Lambda_Adversarial", lambda v: float(v) >= 0, "not negative")
        for k in ("Learning_Rate", "Epsilon", "Gradient_Norm"):
            need(k, lambda v: float(v) > 0, "positive")
        need("Learning_Rate_Decay", lambda v: int(v["Step"]) >= 1 and 0 < float(v["Gamma"]) <= 1, "Step >= 1, 0 < Gamma <= 1")
        need("Layers", lambda v: whole(v) and 3 <= int(v) <= DISC_MAX_LAYERS, "an integer in [3, {}]".format(DISC_MAX_LAYERS))
        need("Channels", lambda v: whole(v) and int(v) >= 16 and int(v) % 16 == 0 and pwg_disc_lds(int(v)) <= PWG_LDS and int(v) <= PWG_MAX_CHANNELS,
             "a multiple of 16 in [16, {}]: a tile of 64 rows x 3 Channels floats must fit the {} bytes of LDS".format(pwg_disc_max_channels(), PWG_LDS))
        need("Negative_Slope", lambda v: 0 <= float(v) < 1, "in [0, 1): the backward reads the LeakyReLU mask from the layer's output")
    return overlay_settings(block, DISC_DEFAULTS, DISC_KEY, "vocoder", rules)


def pwg_disc_lds(C):
    """Bytes of LDS of a middle layer's tile, forward and backward alike: 64 rows of 3 C floats at a stride whose quarter is odd."""
    return 4 * PWG_TILE * lds_row_stride(3 * C)


def pwg_disc_max_channels():
    return max(c for c in range(16, PWG_MAX_CHANNELS + 1, 16) if pwg_disc_lds(c) <= PWG_LDS)


def pwg_disc_geometry(hp):
    """The discriminator's sizes as a dict (layers, C, slope, dilations) from the block `Vocoder.Train.Discriminator` (absent: the defaults); raises ValueError
    naming the offending yaml keys when the kernels do not support them."""
    s = pwg_disc_settings(hp) or DISC_DEFAULTS
    layers, C = int(s["Layers"]), int(s["Channels"])
    return {"layers": layers, "C": C, "slope": float(s["Negative_Slope"]), "dilations": [1] + list(range(1, layers - 1)) + [1]}


def pwg_disc_expected_shapes(geo):
    """state-dict key -> shape of the discriminator with the sizes `geo`"""
    n, C, e = geo["layers"], geo["C"], {}
    for i in range(n):
        e[f"conv_layers.{i}.weight"] = (1 if i == n - 1 else C, 1 if i == 0 else C, 3)
        e[f"conv_layers.{i}.bias"] = (1 if i == n - 1 else C,)
    return e


def pwg_disc_init(geo, seed=0):
    """A fresh discriminator's state dict: torch.nn.Conv1d's default rule per tensor - uniform in +- 1 / sqrt(fan_in), weights and biases alike - drawn in
    the order of `pwg_disc_expected_shapes` on a host generator seeded with `seed` (the pattern of `pwg_init`)."""
    return conv_default_init(pwg_disc_expected_shapes(geo), seed)


def pwg_disc_find_state_dict(obj):
    """The discriminator's state dict inside what torch.load returned: under `discriminator` / `Discriminator`, possibly inside `model`, or at the top level."""
    return find_state_dict(obj, (("discriminator",), ("Discriminator",), ("model", "discriminator"), ("model", "Discriminator"), (), ("model",)),
                           lambda d: any(str(k).startswith("conv_layers.0.weight") for k in d) and not any(str(k).startswith("first_conv.") for k in d),
                           "no Parallel WaveGAN discriminator state dict found (looked for `conv_layers.0.weight*` under discriminator / Discriminator, inside model "
                           "and at the top level)")


def pwg_disc_load(obj, geo):
    """-> {key: float32 host tensor} with exactly the keys of `pwg_disc_expected_shapes`, as `pwg_load` gives the generator's (`checked_load`)."""
    return checked_load(pwg_disc_find_state_dict(obj), pwg_disc_expected_shapes(geo), "discriminator", "discriminator", DISC_KEY)


def pwg_disc_forward(disc, wav, alloc=None):
    """The forward launches on wav [B, T] (fp32, contiguous, on the device) -> dict(wav, scores [B, T], keep: the Layers - 1 hidden outputs [B, T, C] - C floats
    per row and layer, all the backward needs: the output of a LeakyReLU carries its mask).  alloc(*shape): the caller's buffers (tests)."""
    g, lib, P, st = disc.geo, _lib.api(), _lib.ptr, _lib.stream()
    B, T = wav.shape
    C, slope = g["C"], g["slope"]
    f = alloc or (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=wav.device))
    keep, scores = [f(B, T, C) for _ in range(g["layers"] - 1)], f(B, T)
    lib.glowtts_pwg_disc_first(P(wav), P(disc.first[0]), P(disc.first[1]), P(keep[0]), B, T, C, slope, st)
    for i in range(1, g["layers"] - 1):
        w, b, _ = disc.middle[i - 1]
        lib.glowtts_pwg_disc_layer(P(keep[i - 1]), P(w), P(b), P(keep[i]), B, T, C, g["dilations"][i], slope, st)
    lib.glowtts_pwg_disc_last(P(keep[-1]), P(disc.last[0]), P(disc.last[1]), P(scores), B, T, C, st)
    return {"wav": wav, "scores": scores, "keep": keep}


def pwg_disc_backward(disc, fwd, dscores, freeze=False, alloc=None):
    """d scores [B, T] -> (d wav [B, T], {name: gradient in torch's layout} or None when `freeze`) from what `pwg_disc_forward` kept (or the views of some of
    its batch rows).  freeze: the data chain alone - no dpre is written and no weight-gradient launch is made."""
    g, lib, P, st = disc.geo, _lib.api(), _lib.ptr, _lib.stream()
    wav, keep = fwd["wav"], fwd["keep"]
    B, T = wav.shape
    C, slope, n, dev = g["C"], g["slope"], g["layers"], wav.device
    f = alloc or (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev))
    dscores = dscores.to(torch.float32).contiguous()
    grads = work = lengths = dpre = None
    if not freeze:
        grads = {k: f(*shape) for k, shape in pwg_disc_expected_shapes(g).items()}
        work, lengths, dpre = f(lib.glowtts_pwg_disc_work_floats(B, T, C)), torch.full((B,), T, dtype=torch.int32, device=dev), f(B, T, C)

    def wgrad(i, a, d_out, cin, cout):
        lib.glowtts_pwg_disc_wgrad(P(a), P(d_out), P(lengths), P(work), P(grads[f"conv_layers.{i}.weight"]), P(grads[f"conv_layers.{i}.bias"]), B, T, cin,
                                   cout, g["dilations"][i], st)
    dout, dx = f(B, T, C), f(B, T, C)
    lib.glowtts_pwg_disc_last_bwd(P(dscores), P(disc.last[0]), P(dout), B, T, C, st)
    if not freeze:
        wgrad(n - 1, keep[-1], dscores, C, 1)
    for i in reversed(range(1, n - 1)):
        lib.glowtts_pwg_disc_layer_bwd(P(dout), P(keep[i]), P(disc.middle[i - 1][2]), P(dx), P(dpre), B, T, C, g["dilations"][i], slope, st)
        if not freeze:
            wgrad(i, keep[i - 1], dpre, C, C)
        dout, dx = dx, dout
    dwav = f(B, T)
    lib.glowtts_pwg_disc_first_bwd(P(dout), P(keep[0]), P(disc.first[0]), P(dwav), P(dpre), B, T, C, slope, st)
    if not freeze:
        wgrad(0, wav, dpre, 1, C)
    return dwav, grads


class _Score(torch.autograd.Function):
    """scores = PWGDiscriminator.score(wav): forward and backward are the HIP launches of csrc/pwg_disc_ops.hip.  `shared`: a forward that was already run on
    this waveform with these parameters (`PWGDiscriminator.score_pair`) - no forward launch is made then.  freeze: no parameter gradients."""

    @staticmethod
    def forward(ctx, disc, wav, freeze, shared, *params):
        if shared is None:
            disc._build_images({k: t.detach() for k, t in zip(disc.params, params)})
            shared = pwg_disc_forward(disc, wav.detach())
        ctx.disc, ctx.fwd, ctx.freeze, ctx.n = disc, shared, bool(freeze), len(params)
        return shared["scores"].clone()

    @staticmethod
    def backward(ctx, dscores):
        dwav, grads = pwg_disc_backward(ctx.disc, ctx.fwd, dscores, ctx.freeze)
        ctx.fwd = None
        return (None, dwav, None, None) + (tuple(grads[k] for k in ctx.disc.params) if not ctx.freeze else (None,) * ctx.n)


class PWGDiscriminator:
    """PWGDiscriminator(hp, device, state_dict=None, trainable=True, seed=0).score(wav [B, T], freeze=False) -> scores [B, T], one per sample, every row of
    the full length T.  The sizes come from the yaml block `Vocoder.Train.Discriminator` (absent: the defaults).  `params` holds float32 device leaves in
    `pwg_disc_expected_shapes`' names - from `state_dict` (`pwg_disc_load`) or, without one, `pwg_disc_init(geo, seed)`; the packed and transposed weight
    images are rebuilt from them at every call (an optimizer step writes the leaves in place).  The backward yields d wav and, unless `freeze`, the
    parameter gradients.  A row's scores and its d wav are bit-identical alone, in any batch and from run to run."""

    def __init__(self, hp, device="cuda:0", state_dict=None, trainable=True, seed=0):
        self.geo = geo = pwg_disc_geometry(hp)                      # before anything touches the device
        self.trainable = bool(trainable)
        w = pwg_disc_load(state_dict, geo) if state_dict is not None else pwg_disc_init(geo, seed)
        if not _lib.api().glowtts_pwg_disc_supported(geo["C"], geo["layers"], max(geo["dilations"])):
            raise ValueError(f"the {DISC_KEY} block's sizes {geo} are not supported by the kernels")
        self.device = torch.device(device)
        self.params = {k: t.to(self.device).requires_grad_(self.trainable) for k, t in w.items()}
        self._build_images({k: t.detach() for k, t in self.params.items()})

    def _build_images(self, w):
        """The weight images in the kernels' layouts: first and last [3][C] (row = tap); a middle layer's forward image [3 C][C] (row = tap * C + input
        channel) and its backward image [3 C][C] (row = tap * C + output channel)."""
        n, C = self.geo["layers"], self.geo["C"]
        dev = lambda t: t.contiguous().to(self.device)
        self.first = (dev(w["conv_layers.0.weight"][:, 0, :].t()), dev(w["conv_layers.0.bias"]))
        self.middle = [(dev(w[f"conv_layers.{i}.weight"].permute(2, 1, 0).reshape(3 * C, C)), dev(w[f"conv_layers.{i}.bias"]),
                        dev(w[f"conv_layers.{i}.weight"].permute(2, 0, 1).reshape(3 * C, C))) for i in range(1, n - 1)]
        self.last = (dev(w[f"conv_layers.{n - 1}.weight"][0].t()), dev(w[f"conv_layers.{n - 1}.bias"]))

    def _check(self, wav):
        if wav.dim() != 2 or wav.dtype != torch.float32 or not wav.is_cuda:
            raise _lib.GlowTTSHipError(f"PWGDiscriminator: expected an fp32 device tensor [B, T] (the HIP path has no CPU fallback), got {list(wav.shape)} {wav.dtype}")
        B, T = wav.shape
        if B < 1 or T < 1 or not _lib.api().glowtts_pwg_disc_work_floats(B, T, self.geo["C"]):
            raise ValueError(f"PWGDiscriminator: a batch of {B} x {T} samples is outside 1 <= B, 1 <= T, B T < 2^31, B ceil(T / 1024) <= 65535")

    def score(self, wav, freeze=False):
        self._check(wav)
        return _Score.apply(self, wav.contiguous(), freeze, None, *self.params.values())

    def score_pair(self, real, fake):
        """ONE forward over [real; fake] (2 B rows) -> (scores [2 B, T] whose backward yields the parameter gradients alone, p_fake [B, T] = scores[B:] whose
        backward yields d fake alone: the data chain over the fake rows, no weight-gradient launch).  The two backwards share what the forward kept."""
        self._check(fake)
        if tuple(real.shape) != tuple(fake.shape):
            raise ValueError(f"PWGDiscriminator.score_pair: real {list(real.shape)} and fake {list(fake.shape)} differ in shape")
        B = fake.shape[0]
        both = torch.cat([real.detach().to(device=self.device, dtype=torch.float32), fake.detach()]).contiguous()
        self._check(both)
        self._build_images({k: t.detach() for k, t in self.params.items()})
        fwd = pwg_disc_forward(self, both)
        half = {"wav": both[B:], "scores": fwd["scores"][B:], "keep": [k[B:] for k in fwd["keep"]]}
        return _Score.apply(self, both, False, fwd, *self.params.values()), _Score.apply(self, fake.contiguous(), True, half)


class _AdversarialMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, split, v0, v1, factor):
        lib, P, N = _lib.api(), _lib.ptr, scores.numel()
        dp, loss = torch.empty_like(scores), torch.empty(3, dtype=torch.float32, device=scores.device)
        work = torch.empty(4 * (-(-N // 4096)), dtype=torch.float32, device=scores.device)
        lib.glowtts_pwg_disc_mse(P(scores), P(dp), P(work), P(loss), N, split, v0, v1, factor, _lib.stream())
        ctx.dp = dp
        terms = loss[1:].clone()
        ctx.mark_non_differentiable(terms)
        return loss[0].reshape(()), terms

    @staticmethod
    def backward(ctx, g, _):
        return ctx.dp * g.to(torch.float32), None, None, None, None


def adversarial_mse(scores, value, factor=1.0):
    """The least-squares adversarial loss on `pwg_disc_mse`: factor * mean((scores - value)^2) over all scores, with a backward (d scores = factor 2 (scores -
    value) / count).  value = (v0, v1): the first half of the batch rows is held against v0, the second against v1, and the loss is the sum of the two halves'
    means (L_D on [real; fake] with (1, 0)).  -> (loss, terms [2]: the unscaled mean of each part, the second 0 for a single value)."""
    if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_cuda:
        raise _lib.GlowTTSHipError("adversarial_mse: expected fp32 device scores [B, T] (the HIP path has no CPU fallback)")
    N = scores.numel()
    if N < 1 or N >= 2 ** 31:
        raise ValueError(f"adversarial_mse: {N} scores are outside 1 <= B T < 2^31")
    if isinstance(value, (tuple, list)):
        if len(value) != 2 or scores.shape[0] % 2:
            raise ValueError("adversarial_mse: a pair of values needs a batch of an even number of rows ([real; fake])")
        split, v0, v1 = N // 2, float(value[0]), float(value[1])
    else:
        split, v0, v1 = N, float(value), 0.0
    return _AdversarialMSE.apply(scores.contiguous(), split, v0, v1, float(factor))


# ================================================================================================================================================
# Neural vocoder: the HiFi-GAN generator (Kong et al. 2020) on the kernels of csrc/hifigan_ops.hip: inference, f32 - or, with precision 'f16', on those of
# csrc/hifigan_f16_ops.hip (fp16 operands, fp32 sums; DESIGN.md "HiFi-GAN generator: fp16 inference mode").  The network, the launch plan and the
# boundary rule are written down in DESIGN.md ("HiFi-GAN generator"); the checkpoint layout restates the most widely used implementation's names from
# memory and is UNPINNED, like the Parallel WaveGAN's.  The state-dict finder, the weight-norm fold, the checked load and the initialiser are the shared ones.
# ================================================================================================================================================
HIFIGAN_DEFAULTS = {"Type": "HiFiGAN", "Checkpoint_Path": None, "Initial_Channels": 512, "Upsample_Rates": [8, 8, 2, 2], "Upsample_Kernel_Sizes": [16, 16, 4, 4],
                    "Resblock": "1", "Resblock_Kernel_Sizes": [3, 7, 11], "Resblock_Dilations": [[1, 3, 5], [1, 3, 5], [1, 3, 5]], "Precision": "f32"}
HIFIGAN_MAX_CHANNELS, HIFIGAN_MAX_TAPS, HIFIGAN_MAX_DILATION, HIFIGAN_MAX_RATE, HIFIGAN_MAX_UP_TAPS, HIFIGAN_MAX_PHASE_TAPS = 512, 11, 16, 16, 64, 8
HIFIGAN_PRE_TAPS = HIFIGAN_POST_TAPS = 7
HIFIGAN_SLOPE, HIFIGAN_LAST_SLOPE = 0.1, 0.01                       # LeakyReLU: 0.1 everywhere but before conv_post, which has torch's default
HIFIGAN_PRECISIONS = ("f32", "f16")
F16_MAX = 65504.0                                                   # the largest finite fp16: the f16 mode clamps to it before it rounds


def hifigan_settings(hp):
    """The `Vocoder` block of the yaml over HIFIGAN_DEFAULTS (an absent block: the defaults, the V1 sizes)."""
    v = getattr(hp, "Vocoder", None)
    return {k: getattr(v, k, d) if v is not None else d for k, d in HIFIGAN_DEFAULTS.items()}


def hifigan_geometry(hp):
    """The generator's sizes as a dict (A, hop, C0, rates, kernels, channels, resblock, rk, rd, nk, precision); raises ValueError naming the offending yaml
    keys when the kernels do not support them - the idiom of `pwg_geometry`."""
    v = hifigan_settings(hp)
    if v["Type"] != "HiFiGAN":
        raise ValueError(f"Vocoder.Type = {v['Type']!r}: the HiFi-GAN generator needs Vocoder.Type: 'HiFiGAN' (a 'PWG' block describes the Parallel WaveGAN generator)")
    if v["Precision"] not in HIFIGAN_PRECISIONS:
        raise ValueError(f"Vocoder.Precision = {v['Precision']!r}: the HiFi-GAN generator runs in 'f32' or 'f16' (f16: the convolutions' operands only, inference "
                         "only; bf16 is the Parallel WaveGAN layers' mode)")
    resblock = str(v["Resblock"])
    if resblock not in ("1", "2"):
        raise ValueError(f"Vocoder.Resblock = {v['Resblock']!r} must be '1' (two convolutions per dilation) or '2' (one)")
    try:
        C0 = int(v["Initial_Channels"])
        rates, kernels, rk = ([int(x) for x in v[k]] for k in ("Upsample_Rates", "Upsample_Kernel_Sizes", "Resblock_Kernel_Sizes"))
        rd = [[int(d) for d in ds] for ds in v["Resblock_Dilations"]]
    except (TypeError, ValueError):
        raise ValueError("Vocoder.Initial_Channels must be an integer, Vocoder.Upsample_Rates, Vocoder.Upsample_Kernel_Sizes and Vocoder.Resblock_Kernel_Sizes lists "
                         "of integers and Vocoder.Resblock_Dilations a list of such lists") from None
    A, hop = int(hp.Sound.Mel_Dim), int(hp.Sound.Frame_Shift)
    if A < 4 or A % 4 or A > HIFIGAN_MAX_CHANNELS:
        raise ValueError(f"Sound.Mel_Dim = {A} must be a multiple of 4 in [4, {HIFIGAN_MAX_CHANNELS}] for the neural vocoder (Vocoder block)")
    if not rates or len(rates) != len(kernels):
        raise ValueError(f"Vocoder.Upsample_Rates = {rates} and Vocoder.Upsample_Kernel_Sizes = {kernels} must be non-empty lists of one length")
    for u, k in zip(rates, kernels):
        if u < 1 or k < u or (k - u) % 2:
            raise ValueError(f"Vocoder.Upsample_Kernel_Sizes = {kernels} over Vocoder.Upsample_Rates = {rates}: a kernel k of rate u >= 1 needs k >= u and k - u even "
                             f"(padding (k - u) / 2 gives exactly u rows per input row), got k = {k}, u = {u}")
        if u > HIFIGAN_MAX_RATE or k > HIFIGAN_MAX_UP_TAPS or -(-k // u) > HIFIGAN_MAX_PHASE_TAPS:
            raise ValueError(f"Vocoder.Upsample_Rates = {rates} with Vocoder.Upsample_Kernel_Sizes = {kernels}: rates up to {HIFIGAN_MAX_RATE}, kernels up to "
                             f"{HIFIGAN_MAX_UP_TAPS} taps and at most {HIFIGAN_MAX_PHASE_TAPS} taps per phase (ceil(k / u)) are supported, got k = {k}, u = {u}")
    if math.prod(rates) != hop:
        raise ValueError(f"Vocoder.Upsample_Rates = {rates} multiply to {math.prod(rates)}, Sound.Frame_Shift is {hop}: the vocoder must produce one hop per frame")
    if C0 < 16 or C0 > HIFIGAN_MAX_CHANNELS or C0 % (16 << len(rates)):
        raise ValueError(f"Vocoder.Initial_Channels = {C0} halves once per stage of Vocoder.Upsample_Rates = {rates}: every width must stay a multiple of 16, so it "
                         f"must be a multiple of {16 << len(rates)} in [{16 << len(rates)}, {HIFIGAN_MAX_CHANNELS}]")
    if not rk or len(rk) != len(rd) or any(not ds for ds in rd):
        raise ValueError(f"Vocoder.Resblock_Kernel_Sizes = {rk} and Vocoder.Resblock_Dilations = {rd} must be non-empty lists of one length (one non-empty list "
                         "of dilations per kernel size)")
    if any(k < 1 or k % 2 == 0 or k > HIFIGAN_MAX_TAPS for k in rk):
        raise ValueError(f"Vocoder.Resblock_Kernel_Sizes = {rk} must be odd (the padding keeps the row count) and at most {HIFIGAN_MAX_TAPS}")
    if any(d < 1 or d > HIFIGAN_MAX_DILATION for ds in rd for d in ds):
        raise ValueError(f"Vocoder.Resblock_Dilations = {rd} must lie in [1, {HIFIGAN_MAX_DILATION}]")
    return {"A": A, "hop": hop, "C0": C0, "rates": rates, "kernels": kernels, "channels": [C0 >> (i + 1) for i in range(len(rates))], "resblock": resblock,
            "rk": rk, "rd": rd, "nk": len(rk), "precision": v["Precision"]}


def hifigan_expected_shapes(geo):
    """state-dict key -> shape of the generator with the sizes `geo`"""
    e = {"conv_pre.weight": (geo["C0"], geo["A"], HIFIGAN_PRE_TAPS), "conv_pre.bias": (geo["C0"],)}
    cin = geo["C0"]
    for i, (k, c) in enumerate(zip(geo["kernels"], geo["channels"])):
        e[f"ups.{i}.weight"], e[f"ups.{i}.bias"] = (cin, c, k), (c,)               # ConvTranspose1d: [in, out, k]
        for j, (rk, ds) in enumerate(zip(geo["rk"], geo["rd"])):
            for m in range(len(ds)):
                for convs in ("convs1", "convs2")[:2 if geo["resblock"] == "1" else 1]:
                    q = f"resblocks.{i * geo['nk'] + j}.{convs}.{m}."
                    e[q + "weight"], e[q + "bias"] = (c, c, rk), (c,)
        cin = c
    e["conv_post.weight"], e["conv_post.bias"] = (1, cin, HIFIGAN_POST_TAPS), (1,)
    return e


def hifigan_launches(geo):
    """Launches of one call: conv_pre, per stage the transposed convolution and every resblock convolution, conv_post (78 at the V1 sizes)."""
    per_dilation = 2 if geo["resblock"] == "1" else 1
    return 1 + len(geo["rates"]) * (1 + per_dilation * sum(len(ds) for ds in geo["rd"])) + 1


def hifigan_find_state_dict(obj):
    """The generator's state dict inside what torch.load returned: at the top level or under `generator` / `Generator`, possibly inside `model`."""
    return find_state_dict(obj, ((), ("generator",), ("Generator",), ("model",), ("model", "generator"), ("model", "Generator")),
                           lambda d: any(str(k).startswith("conv_pre.") for k in d),
                           "no HiFi-GAN generator state dict found (looked for `conv_pre.*` at the top level, under generator / Generator and inside model)")


def hifigan_load(obj, geo):
    """-> {key: float32 host tensor} with exactly the keys of `hifigan_expected_shapes`: weight-norm pairs are folded once, in float64 (`fold_weight_norm`: its
    norm over everything but dim 0 is also torch's for the transposed convolutions); a missing, surplus or wrongly shaped tensor raises a ValueError naming
    the key (`checked_load`)."""
    return checked_load(hifigan_find_state_dict(obj), hifigan_expected_shapes(geo), "vocoder", "HiFi-GAN generator", "Vocoder")


def hifigan_init(geo, seed=0):
    """A fresh generator's state dict (the names and shapes of `hifigan_expected_shapes`, plain weights): `conv_default_init`."""
    return conv_default_init(hifigan_expected_shapes(geo), seed)


def hifigan_conv_image(weight):
    """Conv1d weight [Cout, Cin, taps] -> the K-major image [taps * Cin, Cout] of csrc/hifigan_ops.hip (row = tap * Cin + input channel)"""
    return weight.permute(2, 1, 0).reshape(-1, weight.shape[0]).contiguous()


def hifigan_up_image(weight):
    """ConvTranspose1d weight [Cin, Cout, taps] -> the K-major image [taps * Cin, Cout] (row = tap * Cin + input channel)"""
    return weight.permute(2, 0, 1).reshape(-1, weight.shape[1]).contiguous()


def hifigan_pack_f16(image, taps):
    """The K-major f32 image [taps * Cin, Cout] of `hifigan_conv_image` / `hifigan_up_image` -> the fp16 image [taps, Cp / 8, Cout, 8] of
    csrc/hifigan_f16_ops.hip: clamped to +-65504 and rounded to nearest even, per tap zero rows from Cin to Cp = pad32(Cin); element (tap, k, n) lies at
    [tap, k // 8, n, k % 8], so a lane's eight k values of one column are 16 consecutive bytes."""
    K, N = image.shape
    Cin = K // taps
    p = torch.zeros(taps, pad32(Cin), N, dtype=torch.float16, device=image.device)
    p[:, :Cin] = image.to(torch.float32).clamp(-F16_MAX, F16_MAX).to(torch.float16).view(taps, Cin, N)
    return p.view(taps, -1, 8, N).permute(0, 1, 3, 2).contiguous()


def hifigan_unpack_f16(packed):
    """The inverse of `hifigan_pack_f16`: [taps, Cp / 8, Cout, 8] fp16 -> [taps, Cp, Cout] float32 (per tap the rounded weights, then the zero rows)"""
    taps, g, N, _ = packed.shape
    return packed.permute(0, 1, 3, 2).reshape(taps, g * 8, N).to(torch.float32)


# ---- training (csrc/hifigan_train_ops.hip; DESIGN.md "Training the HiFi-GAN generator") ----
HIFIGAN_TRAIN_MAX_OFFSETS, HIFIGAN_TRAIN_MAX_VIEW = 11, 4096
HIFIGAN_TRAIN_PRECISIONS = ("f32", "mixed")                         # mixed: f16 forward, bf16 backward (DESIGN.md "... mixed precision")
HIFIGAN_TRAIN_PRECISION_KEY = "Vocoder.Train.Precision"


def hifigan_conv_image_t(weight):
    """Conv1d weight [Cout, Cin, taps] -> the data gradient's image [taps * Cout, Cin]: tap-reversed and channel-transposed, row = (taps - 1 - tap) * Cout +
    output channel.  The convolution of dy (same padding, same dilation) with it is dx."""
    return weight.flip(2).permute(2, 0, 1).reshape(-1, weight.shape[1]).contiguous()


def hifigan_up_reach(u, k):
    """(lo, hi): the range of the row offsets e = m - o0(ph) that the transposed convolution (rate u, k taps, padding (k - u) / 2) reaches in dy read as
    [T, u * Cout]: output row u s + ph sums the taps j0 + m u of input row s + o0 - m (j0 = (ph + p) % u, o0 = (ph + p) // u), so dx[s] reads view row s + e."""
    p, lo, hi = (k - u) // 2, None, None
    for ph in range(u):
        j0, o0 = (ph + p) % u, (ph + p) // u
        nt = (k - j0 + u - 1) // u
        lo, hi = -o0 if lo is None else min(lo, -o0), nt - 1 - o0 if hi is None else max(hi, nt - 1 - o0)
    return lo, hi


def hifigan_up_taps(u, k):
    """[hi - lo + 1, u] int64: the tap j0 + (e + o0) u of (row offset e, phase ph), k where the pair has none"""
    p = (k - u) // 2
    lo, hi = hifigan_up_reach(u, k)
    idx = torch.full((hi - lo + 1, u), k, dtype=torch.int64)
    for ph in range(u):
        j0, o0 = (ph + p) % u, (ph + p) // u
        for m in range((k - j0 + u - 1) // u):
            idx[m - o0 - lo, ph] = j0 + m * u
    return idx


def hifigan_up_image_t(weight, u, taps=None):
    """ConvTranspose1d weight [Cin, Cout, k] of rate u -> the data gradient's image [(hi - lo + 1) * u * Cout, Cin] over dy read as [T, u * Cout]:
    row = (e - lo) * u * Cout + ph * Cout + output channel holds the tap of (e, ph), zero where there is none (`hifigan_up_taps`, given as `taps` when cached).
    A convolution over the view's rows with offsets lo .. hi against it is dx."""
    k = weight.shape[2]
    idx = (hifigan_up_taps(u, k) if taps is None else taps).to(weight.device)
    padded = torch.cat([weight, weight.new_zeros(weight.shape[0], weight.shape[1], 1)], dim=2)
    return padded[:, :, idx].permute(2, 3, 1, 0).reshape(-1, weight.shape[0]).contiguous()


def hifigan_convs(geo):
    """Every convolution of the generator in forward order: (state-dict prefix, Cin, Cout, taps, dilation, rate, rows per frame of its input)"""
    out = [("conv_pre", geo["A"], geo["C0"], HIFIGAN_PRE_TAPS, 1, 0, 1)]
    cin, mult = geo["C0"], 1
    for i, (u, k, c) in enumerate(zip(geo["rates"], geo["kernels"], geo["channels"])):
        out.append((f"ups.{i}", cin, c, k, 1, u, mult))
        mult *= u
        for j, (rk, ds) in enumerate(zip(geo["rk"], geo["rd"])):
            for m, d in enumerate(ds):
                out.append((f"resblocks.{i * geo['nk'] + j}.convs1.{m}", c, c, rk, d, 0, mult))
                if geo["resblock"] == "1":
                    out.append((f"resblocks.{i * geo['nk'] + j}.convs2.{m}", c, c, rk, 1, 0, mult))
        cin = c
    out.append(("conv_post", cin, 1, HIFIGAN_POST_TAPS, 1, 0, mult))
    return out


def hifigan_train_geometry(geo):
    """Raises ValueError naming the yaml keys for sizes that infer but cannot train (the backward's limits, `glowtts_hifigan_train_supported`): a transposed
    convolution's data gradient runs over dy read as [T, u * Cout] - at most HIFIGAN_TRAIN_MAX_VIEW columns and HIFIGAN_TRAIN_MAX_OFFSETS row offsets - and
    writes Cin columns in tiles of 16.  Construction with trainable=True only."""
    cin = geo["C0"]
    for u, k, c in zip(geo["rates"], geo["kernels"], geo["channels"]):
        lo, hi = hifigan_up_reach(u, k)
        if u * c > HIFIGAN_TRAIN_MAX_VIEW or hi - lo + 1 > HIFIGAN_TRAIN_MAX_OFFSETS or cin % 16:
            raise ValueError(f"Vocoder.Upsample_Rates = {geo['rates']} with Vocoder.Upsample_Kernel_Sizes = {geo['kernels']} and Vocoder.Initial_Channels = {geo['C0']}: "
                             f"training needs rate * channels <= {HIFIGAN_TRAIN_MAX_VIEW} and at most {HIFIGAN_TRAIN_MAX_OFFSETS} row offsets per stage, got u = {u}, "
                             f"k = {k} at {c} channels (inference supports these sizes, trainable=True does not)")
        cin = c
    supported = _lib.api().glowtts_hifigan_train_supported
    for name, ci, co, taps, d, rate, _ in hifigan_convs(geo):
        if not supported(ci, co, taps, d, rate):
            raise ValueError(f"the Vocoder block's sizes do not train: {name} ({ci} -> {co} channels, {taps} taps, dilation {d}, rate {rate}) is beyond the backward "
                             "kernels (Vocoder.Initial_Channels, Vocoder.Upsample_Rates, Vocoder.Upsample_Kernel_Sizes, Vocoder.Resblock_Kernel_Sizes, "
                             "Vocoder.Resblock_Dilations)")


def hifigan_train_precision(hp):
    """The yaml's `Vocoder.Train.Precision` (absent: 'f32'), unchecked"""
    train = plain_block(getattr(getattr(hp, "Vocoder", None), "Train", None))
    return train.get("Precision", "f32") if isinstance(train, dict) else "f32"


def hifigan_train_geometry_mixed(geo):
    """Raises ValueError naming the yaml keys for sizes that train in f32 but not in the mixed mode (`glowtts_hifigan_train_supported_mixed`: the 16-bit tiles'
    LDS terms).  Construction with train_precision='mixed' only, before the device is touched."""
    supported = _lib.api().glowtts_hifigan_train_supported_mixed
    for name, ci, co, taps, d, rate, _ in hifigan_convs(geo):
        if not supported(ci, co, taps, d, rate):
            raise ValueError(f"the Vocoder block's sizes do not train with {HIFIGAN_TRAIN_PRECISION_KEY} = 'mixed': {name} ({ci} -> {co} channels, {taps} taps, "
                             f"dilation {d}, rate {rate}) is beyond the 16-bit kernels (Vocoder.Initial_Channels, Vocoder.Upsample_Rates, "
                             "Vocoder.Upsample_Kernel_Sizes, Vocoder.Resblock_Kernel_Sizes, Vocoder.Resblock_Dilations, Sound.Mel_Dim)")


def hifigan_pack_bf16(image, taps):
    """The data gradient's f32 image [taps * K, N] of `hifigan_conv_image_t` / `hifigan_up_image_t` -> the bf16 image [taps, Kp / 8, N, 8] of
    csrc/hifigan_mixed_ops.hip: `hifigan_pack_f16`'s layout, rounded to bf16 (nearest even) without a clamp."""
    K, N = image.shape
    K //= taps
    p = torch.zeros(taps, pad32(K), N, dtype=torch.bfloat16, device=image.device)
    p[:, :K] = image.to(torch.float32).to(torch.bfloat16).view(taps, K, N)
    return p.view(taps, -1, 8, N).permute(0, 1, 3, 2).contiguous()


HIFIGAN_PACK_KINDS = {"conv_f16": 0, "up_f16": 1, "conv_t_bf16": 2, "up_t_bf16": 3, "post_f32": 4, "conv_bf16": 5, "conv_kt_bf16": 6}


def hifigan_pack_plan(geo):
    """The images of a mixed-precision step, one job of `hifigan_pack_images` each: [(state-dict key of the source, kind, Cin, Cout, taps, rate, shape, dtype)] -
    per convolution the fp16 forward image and (conv_pre has none) the bf16 data-gradient image; conv_post's f32 [taps * Cin] rows."""
    plan = []
    for name, ci, co, taps, _, rate, _ in hifigan_convs(geo):
        key = name + ".weight"
        if co == 1:
            plan.append((key, "post_f32", ci, co, taps, rate, (taps * ci,), torch.float32))
            continue
        plan.append((key, "up_f16" if rate else "conv_f16", ci, co, taps, rate, (taps, pad32(ci) // 8, co, 8), torch.float16))
        if name == "conv_pre":
            continue
        if rate:
            lo, hi = hifigan_up_reach(rate, taps)
            plan.append((key, "up_t_bf16", ci, co, taps, rate, (hi - lo + 1, pad32(rate * co) // 8, ci, 8), torch.bfloat16))
        else:
            plan.append((key, "conv_t_bf16", ci, co, taps, rate, (taps, pad32(co) // 8, ci, 8), torch.bfloat16))
    return plan


def hifigan_pack_jobs(plan, params, device):
    """-> (images, jobs, total_blocks): one flat device buffer cut into the plan's images (16-byte aligned views, in plan order) and the int64 job table
    [njobs, 8] of `ops.hifigan_pack_images` - source pointer (the parameter's LIVE storage), destination pointer, kind, Cin, Cout, taps, rate, first block.
    A job has one thread per 16-byte group of its image (conv_post: per float), 256 per block."""
    sizes = [math.prod(shape) * torch.empty(0, dtype=dtype).element_size() for *_, shape, dtype in plan]
    offsets = [0]
    for n in sizes:
        offsets.append(offsets[-1] + (n + 15) // 16 * 16)
    flat = torch.zeros(offsets[-1], dtype=torch.uint8, device=device)
    images, rows, block = [], [], 0
    for (key, kind, ci, co, taps, rate, shape, dtype), off, n in zip(plan, offsets, sizes):
        src = params[key]
        if src.dtype != torch.float32 or not src.is_contiguous() or src.device != flat.device:
            raise _lib.GlowTTSHipError(f"hifigan_pack_jobs needs contiguous float32 device parameters, got {key}: {src.dtype}, {src.device}")
        image = flat[off:off + n].view(dtype).view(shape)
        images.append(image)
        rows.append([src.data_ptr(), image.data_ptr(), HIFIGAN_PACK_KINDS[kind], ci, co, taps, rate, block])
        block += -(-(n // (4 if kind == "post_f32" else 16)) // 256)
    return images, torch.tensor(rows, dtype=torch.int64).to(device), block


def hifigan_train_launches(geo, train_precision="f32"):
    """Launches of one training forward + backward by their names in the launch log: the forward is the inference launches (`hifigan_launches`); the backward is
    conv_post's, then per convolution one data gradient (conv_pre has none: the mel gets no gradient) and the weight gradient's two launches.  'mixed': the
    f16 forward's names, the bf16 backward's, `hifigan_wgrad` once (conv_post) and the one `hifigan_pack_images` that builds the step's images."""
    convs = hifigan_launches(geo) - 2 - len(geo["rates"])           # the resblock convolutions
    n = hifigan_launches(geo)
    if train_precision == "mixed":
        return {"hifigan_pack_images": 1, "hifigan_conv_f16": 1 + convs, "hifigan_upsample_f16": len(geo["rates"]), "hifigan_conv,post": 1, "hifigan_post_bwd": 1,
                "hifigan_conv_bwd_bf16": convs, "hifigan_upsample_bwd_bf16": len(geo["rates"]), "hifigan_wgrad_bf16": n - 1, "hifigan_wgrad": 1,
                "hifigan_wgrad_sum": n}
    if train_precision != "f32":
        raise ValueError(f"train_precision = {train_precision!r}: 'f32' or 'mixed'")
    return {"hifigan_conv": 1 + convs, "hifigan_upsample": len(geo["rates"]), "hifigan_conv,post": 1, "hifigan_post_bwd": 1, "hifigan_conv_bwd": convs,
            "hifigan_upsample_bwd": len(geo["rates"]), "hifigan_wgrad": n, "hifigan_wgrad_sum": n}


def hifigan_train_keep_floats(geo):
    """Floats per mel frame that a training forward keeps for the backward: conv_pre's output, per stage the transposed convolution's output, every
    resblock convolution's input but the first of a block (which is that output) and the stage's mean, and the waveform."""
    per_block = [(2 if geo["resblock"] == "1" else 1) * len(ds) - 1 for ds in geo["rd"]]
    n, mult = geo["C0"], 1
    for u, c in zip(geo["rates"], geo["channels"]):
        mult *= u
        n += mult * c * (2 + sum(per_block))
    return n + geo["hop"]


def hifigan_train_forward(voc, mels, lengths):
    """The inference launches with every convolution writing a slab of its own -> dict(wav, x0, stages): stages[i] = dict(U, blocks, acc) with blocks[j][m] =
    (x_m, t_m): the input of step m of resblock j (x_0 is U) and, type '1', the input of its second convolution.  Only these pre-activation tensors are kept;
    LeakyReLU and its mask are recomputed from them.  The arithmetic is `HiFiGAN.__call__`'s launch for launch: the waveform is bit-identical."""
    g = voc.geo
    B, _, L = mels.shape
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=mels.device)
    x, mult, nk, stages = f(B, L, g["C0"]), 1, g["nk"], []
    conv, up = (ops.hifigan_conv_f16, ops.hifigan_upsample_f16) if voc.train_precision == "mixed" else (ops.hifigan_conv, ops.hifigan_upsample)
    conv(mels, *voc.pre, x, lengths, L, 1, HIFIGAN_PRE_TAPS, 1, channels_first=True)
    fwd = {"x0": x, "stages": stages}
    for i, (u, c) in enumerate(zip(g["rates"], g["channels"])):
        U, acc = f(B, L * mult * u, c), f(B, L * mult * u, c)
        up(x, *voc.ups[i], U, lengths, L, mult, g["kernels"][i], u, HIFIGAN_SLOPE)
        mult *= u
        blocks = []
        for j in range(nk):
            rk, steps, cur, kept = g["rk"][j], voc.blocks[i * nk + j], U, []
            mode = 0 if j == 0 else (2 if j == nk - 1 else 1)
            for m, (d, c1, c2) in enumerate(steps):
                last = m == len(steps) - 1
                dst = acc if last else torch.empty_like(U)
                if c2 is not None:
                    t = torch.empty_like(U)
                    conv(cur, *c1, t, lengths, L, mult, rk, d, HIFIGAN_SLOPE)
                    conv(t, *c2, dst, lengths, L, mult, rk, 1, HIFIGAN_SLOPE, residual=cur, accumulate=mode if last else 0, divisor=nk)
                else:
                    t = None
                    conv(cur, *c1, dst, lengths, L, mult, rk, d, HIFIGAN_SLOPE, residual=cur, accumulate=mode if last else 0, divisor=nk)
                kept.append((cur, t))
                cur = dst
            blocks.append(kept)
        stages.append({"U": U, "blocks": blocks, "acc": acc})
        x = acc
    fwd["wav"] = f(B, L * g["hop"])
    ops.hifigan_post(x, *voc.post, fwd["wav"], lengths, L, g["hop"], HIFIGAN_POST_TAPS, HIFIGAN_LAST_SLOPE)
    return fwd


def hifigan_train_backward(voc, mels, lengths, fwd, dwav):
    """-> {name: gradient in torch's layout} for every name of `hifigan_expected_shapes`, from what `hifigan_train_forward` kept and d wav [B, L * hop].
    Per convolution, last to first: the weight gradient from its kept input and its output's gradient, and the data gradient (`hifigan_conv_bwd`: mask of the
    kept input, + the skip branch's gradient; a block's first step adds into dU, so dU is the sum of the nk blocks' input gradients in block order).  The
    1 / nk of the MRF mean scales the launches that read d acc."""
    g = voc.geo
    B, _, L = mels.shape
    nk, type1 = g["nk"], g["resblock"] == "1"
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=mels.device)
    grads = {k: f(*shape) for k, shape in hifigan_expected_shapes(g).items()}
    work = f(max(ops.hifigan_wgrad_work_floats(B, L, mult, ci, co, taps, rate) for _, ci, co, taps, _, rate, mult in hifigan_convs(g)))
    mixed = voc.train_precision == "mixed"                         # the bf16 op set; conv_post's single output column stays on the f32 launches
    wgrad, conv_bwd, up_bwd = ((ops.hifigan_wgrad_bf16, ops.hifigan_conv_bwd_bf16, ops.hifigan_upsample_bwd_bf16) if mixed else
                               (ops.hifigan_wgrad, ops.hifigan_conv_bwd, ops.hifigan_upsample_bwd))
    wg = lambda key, x, dy, mult, taps, **kw: wgrad(x, dy, lengths, work, grads[key + ".weight"], grads[key + ".bias"], L, mult, taps, **kw)
    dwav = dwav.to(torch.float32).contiguous()
    mult, x = g["hop"], fwd["stages"][-1]["acc"]
    dpre, dA = f(B, L * mult), torch.empty_like(x)
    ops.hifigan_post_bwd(dwav, fwd["wav"], x, voc.post[0], dpre, dA, lengths, L, mult, HIFIGAN_POST_TAPS, HIFIGAN_LAST_SLOPE)
    wg("conv_post", x, dpre, mult, HIFIGAN_POST_TAPS, slope=HIFIGAN_LAST_SLOPE)
    for i in reversed(range(len(g["rates"]))):
        u, k, st = g["rates"][i], g["kernels"][i], fwd["stages"][i]
        x_in = fwd["x0"] if i == 0 else fwd["stages"][i - 1]["acc"]
        dU, G1, G2 = (torch.empty_like(dA) for _ in range(3))
        for j in range(nk):
            rk, n = g["rk"][j], i * nk + j
            dout, sc = dA, 1.0 / nk                                 # d acc / nk is every block's output gradient
            for m in reversed(range(len(voc.blocks[n]))):
                d, (x_m, t_m), (w1t, w2t), q = voc.blocks[n][m][0], st["blocks"][j][m], voc.blocks_t[n][m], f"resblocks.{n}."
                first = m == 0
                if type1:                                           # x' = conv2(lrelu(t)) + x, t = conv1(lrelu(x))
                    dst = dU if first else G2
                    conv_bwd(dout, w2t, t_m, G1, lengths, L, mult, rk, 1, HIFIGAN_SLOPE, scale=sc)
                    wg(q + f"convs2.{m}", t_m, dout, mult, rk, slope=HIFIGAN_SLOPE, scale=sc)
                    conv_bwd(G1, w1t, x_m, dst, lengths, L, mult, rk, d, HIFIGAN_SLOPE, residual=dout, res_scale=sc, accumulate=first and j > 0)
                    wg(q + f"convs1.{m}", x_m, G1, mult, rk, dilation=d, slope=HIFIGAN_SLOPE)
                else:                                               # x' = conv1(lrelu(x)) + x
                    dst = dU if first else (G1 if dout is G2 else G2)
                    conv_bwd(dout, w1t, x_m, dst, lengths, L, mult, rk, d, HIFIGAN_SLOPE, residual=dout, scale=sc, res_scale=sc, accumulate=first and j > 0)
                    wg(q + f"convs1.{m}", x_m, dout, mult, rk, dilation=d, slope=HIFIGAN_SLOPE, scale=sc)
                dout, sc = dst, 1.0
        mult //= u
        wg(f"ups.{i}", x_in, dU, mult, k, rate=u, slope=HIFIGAN_SLOPE)
        dA = torch.empty_like(x_in)
        up_bwd(dU, voc.ups_t[i], x_in, dA, lengths, L, mult, k, u, HIFIGAN_SLOPE)
    wg("conv_pre", mels, dA, 1, HIFIGAN_PRE_TAPS, channels_first=True)
    return grads


class _HiFiGenerate(torch.autograd.Function):
    """wav = HiFiGAN.generate(...): forward and backward are HIP launches (csrc/hifigan_ops.hip, csrc/hifigan_train_ops.hip); the mel gets no gradient."""

    @staticmethod
    def forward(ctx, voc, mels, lengths, *params):
        voc._build_images({k: t.detach() for k, t in zip(voc.params, params)})
        fwd = hifigan_train_forward(voc, mels, lengths)
        ctx.voc, ctx.args, ctx.fwd = voc, (mels, lengths), fwd
        return fwd["wav"]

    @staticmethod
    def backward(ctx, dwav):
        grads = hifigan_train_backward(ctx.voc, *ctx.args, ctx.fwd, dwav)
        ctx.fwd = None
        return (None,) * 3 + tuple(grads[k] for k in ctx.voc.params)


class HiFiGAN:
    """HiFiGAN(hp, device, state_dict=None)(mels [B, Mel, T], mel_lengths) -> (wav [B, T * hop] fp32 on the device, wav_lengths [B] int64).
    state_dict None: `Vocoder.Checkpoint_Path` is loaded.  The generator has no noise input: `seeds` / `noises` are accepted (the call signature of
    `ParallelWaveGAN`) and ignored, a waveform repeats bit for bit.  An utterance's waveform is bit-identical alone, in any batch, at any padding and from
    run to run.  precision 'f32' / 'f16' / None (the yaml's `Vocoder.Precision`, default 'f32'), readable as `.precision` and `geo["precision"]`: 'f16' runs
    the `hifigan_conv` and `hifigan_upsample` launches, conv_pre included, with fp16 operands and fp32 sums (csrc/hifigan_f16_ops.hip; DESIGN.md "fp16
    inference mode" of the HiFi-GAN generator has the contract) - its own reproducible waveform, not the f32 one; inference only: with trainable=True an
    explicit 'f16' raises and the yaml's key is ignored (training stays f32).  'bf16' raises (the Parallel WaveGAN layers' mode).
    `.last_rows` holds the rows entering conv_post of the last call ([B, T * hop,
    channels[-1]], a view of the work buffers: the next call overwrites it; `return_rows=True` returns a copy as a third result).
    `.conv`, `.upsample` and `.stage` run single operators (tests).
    trainable=True (DESIGN.md "Training the HiFi-GAN generator"): `params` holds float32 device leaves in `hifigan_expected_shapes`' names - plain weights,
    from `state_dict` or, without one, `hifigan_init(geo, seed)` - and `generate` returns the same waveform with a backward (csrc/hifigan_train_ops.hip).
    train_precision 'f32' / 'mixed' / None (the yaml's `Vocoder.Train.Precision`, default 'f32'), readable as `.train_precision` (None on a frozen generator, where
    the argument raises): 'mixed' (DESIGN.md "Training the HiFi-GAN generator: mixed precision") runs `generate`'s forward - and `__call__` - on the 'f16' mode's
    launches, bit-identical to a frozen `precision='f16'` generator of the same weights, and the backward's matrix products on bf16 operands
    (csrc/hifigan_mixed_ops.hip); the parameters, every tensor in memory, every sum and conv_post stay fp32, `.precision` still says 'f32', and ONE
    `hifigan_pack_images` launch per step builds the 16-bit images from the parameters."""

    def __init__(self, hp, device="cuda:0", state_dict=None, precision=None, trainable=False, seed=0, train_precision=None):
        if precision is not None and precision not in HIFIGAN_PRECISIONS:
            raise ValueError(f"precision = {precision!r}: the HiFi-GAN generator runs in 'f32' or 'f16' (None: Vocoder.Precision of the yaml; 'bf16' is the "
                             "Parallel WaveGAN layers' mode)")
        self.trainable = bool(trainable)
        if self.trainable and precision == "f16":
            raise ValueError("precision = 'f16' with trainable=True: the fp16 mode is inference only, training stays f32")
        if train_precision is not None and not self.trainable:
            raise ValueError(f"train_precision = {train_precision!r} on a frozen generator: the training precision needs trainable=True (a frozen generator's "
                             "arithmetic is `precision` / Vocoder.Precision)")
        geo = hifigan_geometry(hp)                                  # before anything touches the device or the disk
        self.train_precision = None
        if self.trainable:
            named = "train_precision" if train_precision is not None else HIFIGAN_TRAIN_PRECISION_KEY
            self.train_precision = train_precision if train_precision is not None else hifigan_train_precision(hp)
            if self.train_precision not in HIFIGAN_TRAIN_PRECISIONS:
                raise ValueError(f"{named} = {self.train_precision!r}: the HiFi-GAN generator trains in 'f32' or 'mixed' (f16 forward, bf16 backward, fp32 master "
                                 "weights)")
        self.precision = "f32" if self.trainable else precision or geo["precision"]
        self.geo = geo = dict(geo, precision=self.precision)        # the precision that runs
        f16 = self._f16 = self.precision == "f16" or self.train_precision == "mixed"      # the arithmetic of `__call__` and of the single operators
        self._conv_op, self._up_op = (ops.hifigan_conv_f16, ops.hifigan_upsample_f16) if f16 else (ops.hifigan_conv, ops.hifigan_upsample)
        if self.trainable:
            hifigan_train_geometry(geo)
            if self.train_precision == "mixed":
                hifigan_train_geometry_mixed(geo)
            if state_dict is None:
                state_dict = hifigan_init(geo, seed)
        if state_dict is None:
            path = hifigan_settings(hp)["Checkpoint_Path"]
            if not path:
                raise ValueError("Vocoder.Checkpoint_Path is not set: the neural vocoder needs a HiFi-GAN generator checkpoint")
            state_dict = torch.load(path, map_location="cpu")
        w = hifigan_load(state_dict, geo)
        supported = _lib.api().glowtts_hifigan_supported_f16 if f16 else _lib.api().glowtts_hifigan_supported
        cin, ok = geo["C0"], supported(geo["A"], geo["C0"], HIFIGAN_PRE_TAPS, 1, 0)
        for u, k, c in zip(geo["rates"], geo["kernels"], geo["channels"]):
            ok = ok and supported(cin, c, k, 1, u) and all(supported(c, c, rk, d, 0) for rk, ds in zip(geo["rk"], geo["rd"]) for d in ds + [1])
            cin = c
        if not (ok and supported(cin, 1, HIFIGAN_POST_TAPS, 1, 0)):
            keys = (" of Vocoder.Precision = 'f16' (Vocoder.Initial_Channels, Vocoder.Upsample_Rates, Vocoder.Upsample_Kernel_Sizes, "
                    "Vocoder.Resblock_Kernel_Sizes, Vocoder.Resblock_Dilations, Sound.Mel_Dim)") if f16 else ""
            raise ValueError(f"the Vocoder block's sizes {geo} are not supported by the kernels{keys}")
        self.device = torch.device(device)
        self.sample_rate, self.n_mel, self.hop = int(hp.Sound.Sample_Rate), geo["A"], geo["hop"]
        self._capacity, self._buffers, self.last_rows = 0, None, None
        if self.trainable:                                          # float32 device leaves in hifigan_expected_shapes' names; the images follow them
            self.params = {k: t.to(self.device).requires_grad_(True) for k, t in w.items()}
            w = {k: t.detach() for k, t in self.params.items()}
            self._up_taps = [hifigan_up_taps(u, k).to(self.device) for u, k in zip(geo["rates"], geo["kernels"])]
            self._pack = None                                       # 'mixed': (source pointers, images, job table, blocks) of hifigan_pack_images
        self._build_images(w)

    def _build_images(self, w):
        """The K-major weight images (the MFMA B operand reads 16 consecutive output channels of one input row) from the tensors `w` (host or device): built
        once for a frozen generator; a trainable one rebuilds them on the device at every `generate`, with the transposed images of the backward.
        precision 'f16': the convolutions' images are the packed fp16 images of `hifigan_pack_f16` instead (biases and conv_post stay float32)."""
        geo = self.geo
        if self.trainable and self.train_precision == "mixed":
            return self._pack_images(w)
        dev = lambda t: t.contiguous().to(self.device)
        packed = (lambda im, weight: hifigan_pack_f16(im, weight.shape[2])) if self.precision == "f16" else (lambda im, weight: im)
        pair = lambda q, image: (dev(packed(image(w[q + ".weight"]), w[q + ".weight"])), dev(w[q + ".bias"]))
        self.pre = pair("conv_pre", hifigan_conv_image)
        self.ups = [pair(f"ups.{i}", hifigan_up_image) for i in range(len(geo["rates"]))]
        self.blocks = []                                            # per resblock: per dilation (d, convs1 pair, convs2 pair or None)
        for n in range(len(geo["rates"]) * geo["nk"]):
            ds = geo["rd"][n % geo["nk"]]
            self.blocks.append([(d, pair(f"resblocks.{n}.convs1.{m}", hifigan_conv_image),
                                 pair(f"resblocks.{n}.convs2.{m}", hifigan_conv_image) if geo["resblock"] == "1" else None) for m, d in enumerate(ds)])
        self.post = (dev(w["conv_post.weight"].permute(2, 1, 0).reshape(-1)), dev(w["conv_post.bias"]))
        if self.trainable:
            image_t = lambda q: dev(hifigan_conv_image_t(w[q + ".weight"]))
            self.ups_t = [dev(hifigan_up_image_t(w[f"ups.{i}.weight"], u, self._up_taps[i])) for i, u in enumerate(geo["rates"])]
            self.blocks_t = [[(image_t(f"resblocks.{n}.convs1.{m}"), image_t(f"resblocks.{n}.convs2.{m}") if geo["resblock"] == "1" else None)
                              for m in range(len(geo["rd"][n % geo["nk"]]))] for n in range(len(self.blocks))]

    def _pack_images(self, w):
        """train_precision 'mixed': ONE `hifigan_pack_images` launch builds every image of the step - the fp16 forward images, the bf16 data-gradient images
        and conv_post's rows - from the parameters' live storage.  The destinations and the job table are built once; they are rebuilt only when a parameter's
        storage has moved.  The biases are the parameters themselves."""
        geo = self.geo
        plan = self._plan = getattr(self, "_plan", None) or hifigan_pack_plan(geo)
        ptrs = tuple(w[key].data_ptr() for key, *_ in plan)
        if self._pack is None or self._pack[0] != ptrs:
            src = {key: w[key] for key, *_ in plan}
            images, jobs, blocks = hifigan_pack_jobs(plan, src, self.device)
            self._pack = (ptrs, images, jobs, blocks)
            by = {}
            for (key, kind, *_), image in zip(plan, images):
                by[(key[:-len(".weight")], kind)] = image
            self._pack_by = by
        img = self._pack_by
        ops.hifigan_pack_images(self._pack[2], self._pack[3])
        pair = lambda q, kind: (img[(q, kind)], w[q + ".bias"])
        self.pre = pair("conv_pre", "conv_f16")
        self.ups = [pair(f"ups.{i}", "up_f16") for i in range(len(geo["rates"]))]
        self.ups_t = [img[(f"ups.{i}", "up_t_bf16")] for i in range(len(geo["rates"]))]
        type1 = geo["resblock"] == "1"
        self.blocks, self.blocks_t = [], []
        for n in range(len(geo["rates"]) * geo["nk"]):
            ds = geo["rd"][n % geo["nk"]]
            q1, q2 = f"resblocks.{n}.convs1.", f"resblocks.{n}.convs2."
            self.blocks.append([(d, pair(q1 + str(m), "conv_f16"), pair(q2 + str(m), "conv_f16") if type1 else None) for m, d in enumerate(ds)])
            self.blocks_t.append([(img[(q1 + str(m), "conv_t_bf16")], img[(q2 + str(m), "conv_t_bf16")] if type1 else None) for m in range(len(ds))])
        self.post = (img[("conv_post", "post_f32")], w["conv_post.bias"])

    def _work(self, B, L):
        """Work buffers of a call (two stage outputs that alternate, the transposed convolution's output and two resblock buffers): views of ONE set sized for
        the largest B x L (rounded up to T_BUCKET frames) seen so far, like `GriffinLim._work`.  The kernels honour the lengths and write every row they later
        read."""
        g = self.geo
        frames = B * (-(-L // T_BUCKET) * T_BUCKET)
        if frames > self._capacity:
            self._buffers = self.last_rows = None
            per_frame, mult = g["C0"], 1
            for u, c in zip(g["rates"], g["channels"]):
                mult *= u
                per_frame = max(per_frame, mult * c)
            self._buffers = [torch.empty(frames * per_frame, dtype=torch.float32, device=self.device) for _ in range(5)]
            self._capacity = frames
        return self._buffers

    def _lengths(self, lengths, B, L):
        n = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int32).reshape(B).contiguous()
        return n.clamp(min=0, max=L)

    def _rows(self, x):
        if not x.is_cuda:
            raise _lib.GlowTTSHipError("expected a device tensor (the HIP path has no CPU fallback)")
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def _image(self, image, weight):
        """A torch weight -> the image this generator's launches take, on the device (f32: K-major; f16: packed)"""
        weight = weight.to(device=self.device, dtype=torch.float32)
        return hifigan_pack_f16(image(weight), weight.shape[2]) if self._f16 else image(weight)

    def _image_sizes(self, image, cin):
        """(taps, Cout) of an image over `cin` input channels"""
        return (image.shape[0], image.shape[2]) if self._f16 else (image.shape[0] // cin, image.shape[1])

    def conv(self, x, frame_lengths, key=None, weight=None, bias=None, dilation=1, slope=1.0, residual=None, out=None, accumulate=0, divisor=1.0,
             channels_first=False):
        """One `hifigan_conv` launch on rows x [B, T, Cin] whose utterances own `frame_lengths` rows each -> out [B, T, Cout] (given, or a new tensor).  The
        weights are the generator's own under the state-dict prefix `key` ('conv_pre', 'resblocks.0.convs1.1', ...) or a Conv1d `weight` [Cout, Cin, taps] and
        `bias`.  accumulate: 0 out = y, 1 out = out + y, 2 out = (out + y) / divisor; residual: added first (may be `out`).  channels_first: x is
        [B, Cin, T], as conv_pre takes the mel."""
        x = self._rows(x)
        B, T, cin = (x.shape[0], x.shape[2], x.shape[1]) if channels_first else x.shape
        if key is not None:
            n, m = (int(s) for s in key.split(".")[1::2]) if key.startswith("resblocks.") else (0, 0)
            image, bias = self.pre if key == "conv_pre" else self.blocks[n][m][1 if ".convs1." in key else 2]
        else:
            image, bias = self._image(hifigan_conv_image, weight), bias.to(device=self.device, dtype=torch.float32).contiguous()
        taps, cout = self._image_sizes(image, cin)
        out = out if out is not None else torch.empty(B, T, cout, dtype=torch.float32, device=self.device)
        self._conv_op(x, image, bias, out, self._lengths(frame_lengths, B, T), T, 1, taps, dilation, slope, residual, accumulate, divisor, channels_first)
        return out

    def upsample(self, i, x, frame_lengths, out=None, weight=None, bias=None, rate=None):
        """One `hifigan_upsample` launch: rows x [B, T, Cin] -> out [B, T * rate, Cout] with stage i's own weights (LeakyReLU(0.1) prologue) or, i None, a
        ConvTranspose1d `weight` [Cin, Cout, taps], `bias` and `rate`."""
        x = self._rows(x)
        B, T, _ = x.shape
        if i is not None:
            (image, bias), rate = self.ups[i], self.geo["rates"][i]
        else:
            image, bias = self._image(hifigan_up_image, weight), bias.to(device=self.device, dtype=torch.float32).contiguous()
        taps, cout = self._image_sizes(image, x.shape[2])
        out = out if out is not None else torch.empty(B, T * rate, cout, dtype=torch.float32, device=self.device)
        self._up_op(x, image, bias, out, self._lengths(frame_lengths, B, T), T, 1, taps, rate, HIFIGAN_SLOPE)
        return out

    def _stage(self, i, x, lengths, Lmax, mult, U, X, T, acc):
        """Stage i on rows x (mult rows per frame) -> acc: the transposed convolution into U, then the nk resblocks on U through X and T; the last convolution
        of every block adds into `acc` in its epilogue - the first block writes, the last divides by nk - so the MRF mean costs no launch."""
        g = self.geo
        u, nk = g["rates"][i], g["nk"]
        conv = self._conv_op
        self._up_op(x, *self.ups[i], U, lengths, Lmax, mult, g["kernels"][i], u, HIFIGAN_SLOPE)
        mult *= u
        for j in range(nk):
            rk, steps, cur = g["rk"][j], self.blocks[i * nk + j], U
            mode = 0 if j == 0 else (2 if j == nk - 1 else 1)
            for m, (d, c1, c2) in enumerate(steps):
                last = m == len(steps) - 1
                if c2 is not None:                                  # type '1': t = conv1(lrelu(x)), x = conv2(lrelu(t)) + x
                    conv(cur, *c1, T, lengths, Lmax, mult, rk, d, HIFIGAN_SLOPE)
                    conv(T, *c2, acc if last else X, lengths, Lmax, mult, rk, 1, HIFIGAN_SLOPE, residual=cur, accumulate=mode if last else 0, divisor=nk)
                    cur = X
                else:                                               # type '2': x = conv1(lrelu(x)) + x
                    dst = acc if last else (T if cur is X else X)
                    conv(cur, *c1, dst, lengths, Lmax, mult, rk, d, HIFIGAN_SLOPE, residual=cur, accumulate=mode if last else 0, divisor=nk)
                    cur = dst

    def stage(self, i, x, frame_lengths):
        """Stage i alone (the transposed convolution and its MRF) on rows x [B, T, c_{i-1}] -> [B, T * rate_i, c_i] (tests)."""
        x = self._rows(x)
        B, T, _ = x.shape
        u, c = self.geo["rates"][i], self.geo["channels"][i]
        U, X, Tb, acc = (torch.empty(B, T * u, c, dtype=torch.float32, device=self.device) for _ in range(4))
        self._stage(i, x, self._lengths(frame_lengths, B, T), T, 1, U, X, Tb, acc)
        return acc

    @torch.no_grad()
    def __call__(self, mels, mel_lengths, seeds=None, noises=None, return_rows=False):
        if not mels.is_cuda:
            raise _lib.GlowTTSHipError("expected a device tensor (the HIP path has no CPU fallback)")
        mels = mels.to(device=self.device, dtype=torch.float32).contiguous()
        B, Mel, L = mels.shape
        if Mel != self.n_mel:
            raise ValueError(f"mels have {Mel} channels, Sound.Mel_Dim = {self.n_mel}")
        g = self.geo
        if self.trainable:                                          # the images follow the parameters (an optimizer step writes the leaves in place)
            self._build_images({k: t.detach() for k, t in self.params.items()})
        lengths = self._lengths(mel_lengths, B, L)
        p0, p1, U, X, T = self._work(B, L)
        view = lambda buf, rows, c: buf[:B * rows * c].view(B, rows, c)
        x, mult = view(p0, L, g["C0"]), 1
        self._conv_op(mels, *self.pre, x, lengths, L, 1, HIFIGAN_PRE_TAPS, 1, channels_first=True)       # the mel as the caller holds it: [B, Mel, L]
        for i, (u, c) in enumerate(zip(g["rates"], g["channels"])):
            rows = L * mult * u
            acc = view(p1 if i % 2 == 0 else p0, rows, c)
            self._stage(i, x, lengths, L, mult, view(U, rows, c), view(X, rows, c), view(T, rows, c), acc)
            x, mult = acc, mult * u
        wav = torch.empty(B, L * g["hop"], dtype=torch.float32, device=self.device)
        ops.hifigan_post(x, *self.post, wav, lengths, L, g["hop"], HIFIGAN_POST_TAPS, HIFIGAN_LAST_SLOPE)
        self.last_rows = x
        wav_lengths = lengths.to(torch.int64) * g["hop"]
        return (wav, wav_lengths, x.clone()) if return_rows else (wav, wav_lengths)

    def generate(self, mels, mel_lengths):
        """The training forward: `__call__`'s launches with every convolution's output in a slab of its own (so the waveform is bit-identical) ->
        (wav [B, T * hop], wav_lengths) with a backward that fills `.grad` of every tensor of `self.params`.  Only for `trainable=True`."""
        if not self.trainable:
            raise _lib.GlowTTSHipError("HiFiGAN.generate needs a generator constructed with trainable=True (this one holds frozen weight images only)")
        if not mels.is_cuda:
            raise _lib.GlowTTSHipError("expected a device tensor (the HIP path has no CPU fallback)")
        mels = mels.to(device=self.device, dtype=torch.float32).contiguous()
        B, Mel, L = mels.shape
        if Mel != self.n_mel:
            raise ValueError(f"mels have {Mel} channels, Sound.Mel_Dim = {self.n_mel}")
        lengths = self._lengths(mel_lengths, B, L)
        wav = _HiFiGenerate.apply(self, mels, lengths, *self.params.values())
        return wav, lengths.to(torch.int64) * self.geo["hop"]

    def to_host(self, wav, wav_lengths):
        """Device waveforms -> list of float32 numpy arrays clipped to [-1, 1] (what `audio.write_wav` takes).  No de-emphasis: the vocoder was trained on
        final audio."""
        wav, n = wav.cpu().numpy(), wav_lengths.cpu().tolist()
        return [np.clip(w[:m], -1.0, 1.0).astype(np.float32) for w, m in zip(wav, n)]


# ================================================================================================================================================
# The HiFi-GAN multi-period discriminator on the kernels of csrc/hifigan_disc_ops.hip: forward, backward, feature matching, f32.  The network is written
# down in DESIGN.md ("Training the HiFi-GAN discriminator"); it and the checkpoint layout restate the most widely used implementation from memory and are
# UNPINNED, like the other vocoder contracts.  Kernel sizes 5 / 3 and stride 3 are constants of the architecture, not yaml keys.  The multi-scale
# discriminator (the optional sub-block `Multi_Scale`) follows it below.
# ================================================================================================================================================
MPD_KEY = "Vocoder.Train.Adversarial"
MPD_DEFAULTS = {"Start_Step": 0, "Lambda_Adversarial": 1.0, "Lambda_Feature_Matching": 2.0, "Learning_Rate": 2.0e-4, "Epsilon": 1.0e-6, "Gradient_Norm": 10.0,
                "Learning_Rate_Decay": {"Step": 200000, "Gamma": 0.5}, "Periods": [2, 3, 5, 7, 11], "Channels": [32, 128, 512, 1024, 1024], "Negative_Slope": 0.1}
MPD_TAPS, MPD_POST_TAPS, MPD_STRIDE, MPD_MAX_PERIOD, MPD_MAX_PERIODS, MPD_MAX_CHANNELS, MPD_MAX_WIDTHS = 5, 3, 3, 16, 8, 1024, 6
MSD_BLOCK = "Multi_Scale"                                           # the optional sub-block of the multi-scale discriminator (below)
# The optional key `Vocoder.Train.Adversarial.Precision`: 'f32' (absent: f32) or 'bf16' - the middle convolutions of the multi-period discriminator on bf16
# MFMAs, forward and backward (DESIGN.md "The multi-period discriminator in bf16").  It governs the period discriminator ALONE: with `Multi_Scale` the
# multi-scale discriminator stays f32 entirely.  Not a key of MPD_DEFAULTS: it appears in the settings only when the yaml has it.
MPD_PRECISION, MPD_PRECISIONS = "Precision", ("f32", "bf16")


def hifigan_disc_precision(hp, precision=None):
    """The multi-period discriminator's precision: the argument, else the yaml's `Vocoder.Train.Adversarial.Precision`, else 'f32'; any other value raises a
    ValueError naming the key (or the argument)."""
    if precision is None:
        block = plain_block(getattr(getattr(getattr(hp, "Vocoder", None), "Train", None), "Adversarial", None))
        given = block.get(MPD_PRECISION, "f32") if isinstance(block, dict) else "f32"
        name = f"{MPD_KEY}.{MPD_PRECISION}"
    else:
        given, name = precision, "precision"
    if not isinstance(given, str) or given not in MPD_PRECISIONS:
        raise ValueError(f"{name} = {given!r}: the multi-period discriminator runs in 'f32' or 'bf16' (the key governs the period discriminator alone; the "
                         "multi-scale discriminator is f32)")
    return given


def hifigan_disc_settings(hp):
    """The optional yaml block `Vocoder.Train.Adversarial` over MPD_DEFAULTS (absent block: None), checked: a ValueError names every unknown or bad key.
    The optional sub-block `Multi_Scale` (`hifigan_msd_settings`) and the optional key `Precision` ('f32' / 'bf16') appear in the result only when the yaml
    has them."""
    block = getattr(getattr(getattr(hp, "Vocoder", None), "Train", None), "Adversarial", None)
    if block is None:
        return None
    whole = lambda v: int(v) == v

    def rules(s, need):
        need("Start_Step", lambda v: whole(v) and int(v) >= 0, "an integer, at least 0")
        for k in ("Lambda_Adversarial", "Lambda_Feature_Matching"):
            need(k, lambda v: float(v) >= 0, "not negative")
        for k in ("Learning_Rate", "Epsilon", "Gradient_Norm"):
            need(k, lambda v: float(v) > 0, "positive")
        need("Learning_Rate_Decay", lambda v: int(v["Step"]) >= 1 and 0 < float(v["Gamma"]) <= 1, "Step >= 1, 0 < Gamma <= 1")
        need("Periods", lambda v: 1 <= len(v) <= MPD_MAX_PERIODS and all(whole(p) and 2 <= int(p) <= MPD_MAX_PERIOD for p in v) and len(set(int(p) for p in v)) == len(v),
             "1 to {} distinct integers in [2, {}]".format(MPD_MAX_PERIODS, MPD_MAX_PERIOD))
        need("Channels", lambda v: 2 <= len(v) <= MPD_MAX_WIDTHS and all(whole(c) and 16 <= int(c) <= MPD_MAX_CHANNELS and int(c) % 16 == 0 for c in v),
             "2 to {} widths, each a multiple of 16 in [16, {}]".format(MPD_MAX_WIDTHS, MPD_MAX_CHANNELS))
        need("Negative_Slope", lambda v: 0 <= float(v) < 1, "in [0, 1)")
    s = overlay_settings(block, MPD_DEFAULTS, MPD_KEY, "vocoder", rules, also=(MSD_BLOCK, MPD_PRECISION))
    if MPD_PRECISION in s:
        s[MPD_PRECISION] = hifigan_disc_precision(hp)
    s["Periods"], s["Channels"] = [int(p) for p in s["Periods"]], [int(c) for c in s["Channels"]]
    if MSD_BLOCK in s:
        s[MSD_BLOCK] = hifigan_msd_settings(hp)
        if s[MSD_BLOCK] is None:
            del s[MSD_BLOCK]
    return s


def hifigan_disc_geometry(hp):
    """The discriminator's sizes as a dict (periods, channels, strides, slope) from the block `Vocoder.Train.Adversarial` (absent: the defaults); raises
    ValueError naming the offending yaml keys (`hifigan_disc_settings`)."""
    s = hifigan_disc_settings(hp) or MPD_DEFAULTS
    channels = list(s["Channels"])
    return {"periods": list(s["Periods"]), "channels": channels, "strides": [MPD_STRIDE] * (len(channels) - 1) + [1], "slope": float(s["Negative_Slope"])}


def hifigan_disc_rows(geo, T, p):
    """Rows h of the folded waveform and of every layer's output for period p: [H0 = ceil(T / p), H1, ..., H_last] (conv_post keeps H_last).  T below
    2 max(Periods) - the reflect pad would reach beyond the waveform - raises a ValueError naming the key."""
    if T < 2 * max(geo["periods"]):
        raise ValueError(f"{MPD_KEY}.Periods = {geo['periods']}: a waveform of {T} samples is shorter than 2 max(Periods) = {2 * max(geo['periods'])}, the reflect "
                         "pad would reach beyond it")
    H = [-(-T // p)]
    for s in geo["strides"]:
        H.append((H[-1] - 1) // s + 1)
    return H


def hifigan_disc_expected_shapes(geo):
    """state-dict key -> shape of the discriminator with the sizes `geo` (Conv2d weights with a kernel (k, 1))"""
    e = {}
    for i in range(len(geo["periods"])):
        cin = 1
        for j, c in enumerate(geo["channels"]):
            e[f"discriminators.{i}.convs.{j}.weight"], e[f"discriminators.{i}.convs.{j}.bias"] = (c, cin, MPD_TAPS, 1), (c,)
            cin = c
        e[f"discriminators.{i}.conv_post.weight"], e[f"discriminators.{i}.conv_post.bias"] = (1, cin, MPD_POST_TAPS, 1), (1,)
    return e


def hifigan_disc_init(geo, seed=0):
    """A fresh discriminator's state dict: torch's default rule per tensor (`conv_default_init`: uniform in +- 1 / sqrt(fan_in), fan_in = Cin * taps)."""
    return conv_default_init(hifigan_disc_expected_shapes(geo), seed)


def hifigan_disc_find_state_dict(obj):
    """The multi-period discriminator's state dict inside what torch.load returned: at the top level, under `discriminator` / `Discriminator` / `mpd`, or
    inside `model`.  Neither a Parallel WaveGAN discriminator (`conv_layers.*`) nor a generator (`conv_pre.*`) is taken for it."""
    names = ("discriminator", "Discriminator", "mpd")
    return find_state_dict(obj, ((),) + tuple((n,) for n in names) + (("model",),) + tuple(("model", n) for n in names),
                           lambda d: any(str(k).startswith("discriminators.0.convs.0.weight") for k in d),
                           "no HiFi-GAN multi-period discriminator state dict found (looked for `discriminators.0.convs.0.weight*` at the top level, under "
                           "discriminator / Discriminator / mpd and inside model)")


def hifigan_disc_load(obj, geo):
    """-> {key: float32 host tensor} with exactly the keys of `hifigan_disc_expected_shapes` (`checked_load`: weight-norm pairs are folded once)."""
    return checked_load(hifigan_disc_find_state_dict(obj), hifigan_disc_expected_shapes(geo), "discriminator", "multi-period discriminator", MPD_KEY)


def hifigan_disc_pack_bf16(weight):
    """The host restatement of the bf16 mode's images of one middle convolution (`hifigan_pack_images` kinds 5 and 6 write these bytes): Conv weight
    [Cout, Cin, taps(, 1)] -> (the forward image [taps, pad32(Cin) / 8, Cout, 8]: element (tap, k = input channel, n = output channel); the
    channel-transposed image [taps, pad32(Cout) / 8, Cin, 8]: element (tap, k = output channel, n = input channel), taps NOT reversed), both rounded to
    bf16 (nearest even) with zero rows from K to pad32(K): `hifigan_pack_bf16`'s layout."""
    w = weight[..., 0] if weight.dim() == 4 else weight
    co, ci, taps = w.shape
    return (hifigan_pack_bf16(w.permute(2, 1, 0).reshape(-1, co), taps), hifigan_pack_bf16(w.permute(2, 0, 1).reshape(-1, ci), taps))


def hifigan_disc_pack_plan(geo):
    """The bf16 images of every period's middle convolutions, one job of `hifigan_pack_images` each, in `hifigan_pack_plan`'s form: per convolution the
    forward image (kind 5), then the channel-transposed image (kind 6)."""
    plan, ch = [], geo["channels"]
    for i in range(len(geo["periods"])):
        for j in range(1, len(ch)):
            key, ci, co = f"discriminators.{i}.convs.{j}.weight", ch[j - 1], ch[j]
            plan.append((key, "conv_bf16", ci, co, MPD_TAPS, 0, (MPD_TAPS, pad32(ci) // 8, co, 8), torch.bfloat16))
            plan.append((key, "conv_kt_bf16", ci, co, MPD_TAPS, 0, (MPD_TAPS, pad32(co) // 8, ci, 8), torch.bfloat16))
    return plan


def hifigan_disc_forward(disc, wav, alloc=None):
    """The forward launches on wav [B, T] (fp32, contiguous, on the device) -> dict(wav, periods: per period dict(p, H, keep, scores)).  keep[j] [B, H[j + 1] p,
    C_j] is layer j's PRE-activation output with the flat row h p + c, scores [B, H[-1] p] conv_post's.  alloc(*shape): the caller's buffers (tests)."""
    g, lib, P, st = disc.geo, _lib.api(), _lib.ptr, _lib.stream()
    B, T = wav.shape
    ch, strides, slope = g["channels"], g["strides"], g["slope"]
    f = alloc or (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=wav.device))
    bf16 = getattr(disc, "precision", "f32") == "bf16"                 # the middle convolutions' op set; everything else is shared
    out = []
    for p, im in zip(g["periods"], disc.images):
        H = hifigan_disc_rows(g, T, p)
        keep = [f(B, H[j + 1] * p, c) for j, c in enumerate(ch)]
        scores = f(B, H[-1] * p)
        lib.glowtts_hifigan_disc_first(P(wav), P(im["first"][0]), P(im["first"][1]), P(keep[0]), B, T, p, strides[0], ch[0], st)
        for j in range(1, len(ch)):
            w, b, _ = im["convs"][j - 1]
            if bf16:
                ops.hifigan_disc_conv_bf16(keep[j - 1], w, b, keep[j], H[j], p, strides[j], slope)
            else:
                lib.glowtts_hifigan_disc_conv(P(keep[j - 1]), P(w), P(b), P(keep[j]), B, H[j], p, strides[j], ch[j - 1], ch[j], slope, st)
        lib.glowtts_hifigan_disc_post(P(keep[-1]), P(im["post"][0]), P(im["post"][1]), P(scores), B, H[-1], p, ch[-1], slope, st)
        out.append({"p": p, "H": H, "keep": keep, "scores": scores})
    # the images (and the precision) this forward ran with: its backward must not see a later rebuild
    return {"wav": wav, "periods": out, "images": disc.images, "bf16": bf16}


def hifigan_disc_feature_maps(disc, period_fwd):
    """The feature maps of one period of `hifigan_disc_forward` in torch's layout: the activated outputs [B, C_j, H, p], then conv_post's [B, 1, H, p]."""
    p, slope = period_fwd["p"], disc.geo["slope"]
    maps = [torch.nn.functional.leaky_relu(k, slope).reshape(k.shape[0], -1, p, k.shape[2]).permute(0, 3, 1, 2) for k in period_fwd["keep"]]
    return maps + [period_fwd["scores"].reshape(period_fwd["scores"].shape[0], 1, -1, p)]


def hifigan_disc_work(disc, B, T, device, alloc=None):
    """The work buffer of the backward and of the feature-matching loss on a batch of B x T: the largest layer's `glowtts_hifigan_disc_work_floats`."""
    g, lib = disc.geo, _lib.api()
    floats = 0
    for p in g["periods"]:
        H, cin = hifigan_disc_rows(g, T, p), 1
        for j, c in enumerate(g["channels"]):
            floats, cin = max(floats, lib.glowtts_hifigan_disc_work_floats(B, H[j + 1] * p, cin, c, MPD_TAPS)), c
        floats = max(floats, lib.glowtts_hifigan_disc_work_floats(B, H[-1] * p, cin, 1, MPD_POST_TAPS))
    f = alloc or (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=device))
    return f(floats)


def hifigan_disc_feature_matching(disc, fwd, alloc=None):
    """The feature-matching terms of a forward over [real; fake] (2 B rows) -> (terms, l_fm, inj).  terms [periods, widths + 1]: mean |lrelu(real) -
    lrelu(fake)| per map, raw for conv_post; l_fm [1]: their sum, added up by the kernels themselves in launch order (period, then map); inj: per period the
    gradients of the sum of its terms with respect to the fake rows' kept pre-activations (widths tensors) and scores (the last), each laid out as the fake
    half of what the forward kept."""
    g, lib, P, st = disc.geo, _lib.api(), _lib.ptr, _lib.stream()
    B2, T = fwd["wav"].shape
    B, dev = B2 // 2, fwd["wav"].device
    f = alloc or (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev))
    work, terms, total, inj = hifigan_disc_work(disc, B, T, dev, alloc), f(len(g["periods"]), len(g["channels"]) + 1), f(1), []
    for i, per in enumerate(fwd["periods"]):
        maps = [(k, g["slope"]) for k in per["keep"]] + [(per["scores"], 1.0)]
        inj.append([f(B, *k.shape[1:]) for k, _ in maps])
        for j, (k, slope) in enumerate(maps):
            lib.glowtts_hifigan_disc_fm(P(k), P(inj[i][j]), P(work), P(terms[i, j:]), P(total), k.numel() // 2, slope, 1 if i or j else 0, st)
    return terms, total, inj


def hifigan_disc_backward(disc, fwd, dscores, freeze=False, inj=None, inj_scale=None, need_dwav=True, alloc=None):
    """d scores (one [B, H_last p] per period) -> (d wav [B, T] summed over the periods in period order, or None unless `need_dwav`; {name: gradient in
    torch's layout} or None when `freeze`) from what `hifigan_disc_forward` kept (or the views of some of its batch rows).  inj (`hifigan_disc_feature_matching`)
    times the device scalar inj_scale is added to every d pre and to d scores on the way down.  freeze: the data chain alone, no weight-gradient launch."""
    g, lib, P, st = disc.geo, _lib.api(), _lib.ptr, _lib.stream()
    wav = fwd["wav"]
    B, T = wav.shape
    ch, strides, slope, dev, n = g["channels"], g["strides"], g["slope"], wav.device, len(g["channels"])
    f = alloc or (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev))
    grads = work = None
    if not freeze:
        grads, work = {k: f(*shape) for k, shape in hifigan_disc_expected_shapes(g).items()}, hifigan_disc_work(disc, B, T, dev, alloc)
    scale = P(inj_scale) if inj is not None else None
    dwav = f(B, T) if need_dwav else None
    bf16 = fwd.get("bf16", False)
    for i, (per, im, ds) in enumerate(zip(fwd["periods"], fwd["images"], dscores)):
        p, H, keep = per["p"], per["H"], per["keep"]
        ds, ij = ds.to(torch.float32).contiguous(), inj[i] if inj is not None else [None] * (n + 1)

        def wgrad(name, x, dy, h, stride, cin, cout, taps, samples, sl):
            lib.glowtts_hifigan_disc_wgrad(P(x), P(dy), P(work), P(grads[f"discriminators.{i}.{name}.weight"]), P(grads[f"discriminators.{i}.{name}.bias"]), B, h, p,
                                           stride, cin, cout, taps, samples, sl, st)
        d = f(B, H[-1] * p, ch[-1])
        lib.glowtts_hifigan_disc_post_bwd(P(ds), P(ij[n]) if ij[n] is not None else None, P(keep[-1]), P(im["post"][0]), P(ij[n - 1]) if ij[n - 1] is not None else None,
                                          scale, P(d), B, H[-1], p, ch[-1], slope, st)
        if not freeze:
            wgrad("conv_post", keep[-1], ds, H[-1], 1, ch[-1], 1, MPD_POST_TAPS, 0, slope)
        for j in reversed(range(1, n)):
            if not freeze and bf16:
                ops.hifigan_disc_wgrad_bf16(keep[j - 1], d, work, grads[f"discriminators.{i}.convs.{j}.weight"], grads[f"discriminators.{i}.convs.{j}.bias"], H[j], p,
                                            strides[j], slope)
            elif not freeze:
                wgrad(f"convs.{j}", keep[j - 1], d, H[j], strides[j], ch[j - 1], ch[j], MPD_TAPS, 0, slope)
            dx = f(B, H[j] * p, ch[j - 1])
            if bf16:
                ops.hifigan_disc_conv_bwd_bf16(d, im["convs"][j - 1][2], keep[j - 1], dx, H[j], p, strides[j], slope, inj=ij[j - 1],
                                               inj_scale=inj_scale if inj is not None else None)
            else:
                lib.glowtts_hifigan_disc_conv_bwd(P(d), P(im["convs"][j - 1][2]), P(keep[j - 1]), P(ij[j - 1]) if ij[j - 1] is not None else None, scale, P(dx), B, H[j],
                                                  p, strides[j], ch[j - 1], ch[j], slope, st)
            d = dx
        if not freeze:
            wgrad("convs.0", wav, d, H[0], strides[0], 1, ch[0], MPD_TAPS, T, 1.0)
        if need_dwav:
            lib.glowtts_hifigan_disc_first_bwd(P(d), P(im["first"][0]), P(dwav), B, T, p, strides[0], ch[0], 1 if i else 0, st)
    return dwav, grads


class _PeriodScore(torch.autograd.Function):
    """scores = HiFiGANPeriodDiscriminator.score(wav): forward and backward are the HIP launches of csrc/hifigan_disc_ops.hip.  `shared`: a forward that was
    already run on this waveform with these parameters (`score_pair`) - no forward launch is made then.  freeze: no parameter gradients.  The discriminator
    names its forward and backward (`OPS`) and the key of its sub-networks in what the forward returns (`NETS`): the multi-scale discriminator shares this node."""

    @staticmethod
    def forward(ctx, disc, wav, freeze, shared, *params):
        if shared is None:
            disc._build_images({k: t.detach() for k, t in zip(disc.params, params)})
            shared = disc.OPS[0](disc, wav.detach())
        ctx.disc, ctx.fwd, ctx.freeze, ctx.n = disc, shared, bool(freeze), len(params)
        return tuple(per["scores"].clone() for per in shared[disc.NETS])

    @staticmethod
    def backward(ctx, *dscores):
        dwav, grads = ctx.disc.OPS[1](ctx.disc, ctx.fwd, dscores, ctx.freeze, need_dwav=ctx.needs_input_grad[1])
        ctx.fwd = None
        return (None, dwav, None, None) + (tuple(grads[k] for k in ctx.disc.params) if not ctx.freeze else (None,) * ctx.n)


class _FakeTerms(torch.autograd.Function):
    """(p_fake per period ..., l_fm) of `score_pair` as ONE node: its backward runs the frozen data chain once per period with the feature-matching gradient
    (times d l_fm, read on the device) injected into every d pre, however many of the outputs the loss used."""

    @staticmethod
    def forward(ctx, disc, fake, half, l_fm, inj):
        ctx.disc, ctx.fwd, ctx.inj = disc, half, inj
        return tuple(per["scores"].clone() for per in half[disc.NETS]) + (l_fm.reshape(()).clone(),)

    @staticmethod
    def backward(ctx, *g):
        scale = g[-1].to(torch.float32).reshape(1).contiguous()
        dwav, _ = ctx.disc.OPS[1](ctx.disc, ctx.fwd, g[:-1], True, inj=ctx.inj, inj_scale=scale)
        ctx.fwd = ctx.inj = None
        return None, dwav, None, None, None


class HiFiGANPeriodDiscriminator:
    """HiFiGANPeriodDiscriminator(hp, device, state_dict=None, trainable=True, seed=0, precision=None): the multi-period discriminator.  precision: 'f32',
    'bf16' (the middle convolutions on bf16 MFMAs, forward and backward; DESIGN.md "The multi-period discriminator in bf16") or None: the yaml's
    `Vocoder.Train.Adversarial.Precision`, absent 'f32'; readable as `.precision`.  Parameters, checkpoints and every tensor are fp32 in both.  The sizes come from the yaml block
    `Vocoder.Train.Adversarial` (absent: the defaults).  `params` holds float32 device leaves in `hifigan_disc_expected_shapes`' names - from `state_dict`
    (`hifigan_disc_load`) or, without one, `hifigan_disc_init(geo, seed)`; the weight images are rebuilt from them at every call (an optimizer step writes
    the leaves in place).  A row's scores, feature maps and d wav are bit-identical alone, in any batch and from run to run."""
    OPS, NETS = (hifigan_disc_forward, hifigan_disc_backward), "periods"

    def __init__(self, hp, device="cuda:0", state_dict=None, trainable=True, seed=0, precision=None):
        self.geo = geo = hifigan_disc_geometry(hp)                  # before anything touches the device
        self.precision = hifigan_disc_precision(hp, precision)
        self.trainable = bool(trainable)
        w = hifigan_disc_load(state_dict, geo) if state_dict is not None else hifigan_disc_init(geo, seed)
        lib, widths = _lib.api(), [1] + geo["channels"] + [1]
        supported = lib.glowtts_hifigan_disc_supported_bf16 if self.precision == "bf16" else lib.glowtts_hifigan_disc_supported
        if not all(supported(p, a, b) for p in geo["periods"] for a, b in zip(widths, widths[1:])):
            raise ValueError(f"the {MPD_KEY} block's sizes {geo} are not supported by the {self.precision} kernels")
        self.device = torch.device(device)
        self._plan = hifigan_disc_pack_plan(geo) if self.precision == "bf16" else None
        self._pack = None                                           # 'bf16': (source pointers, job table, image offsets on the device and here, blocks) of hifigan_pack_images
        self.params = {k: t.to(self.device).requires_grad_(self.trainable) for k, t in w.items()}
        self._build_images({k: t.detach() for k, t in self.params.items()})

    def _build_images(self, w):
        """Per period the weight images in the kernels' layouts: first [5][C0] and post [3][C] (row = tap); a middle layer's forward image [5 Cin][Cout]
        (row = tap Cin + input channel) and its backward image [5 Cout][Cin] (row = tap Cout + output channel)."""
        dev, n = (lambda t: t.contiguous().to(self.device)), len(self.geo["channels"])
        packed = self._pack_images(w) if self.precision == "bf16" else None
        self.images = []
        for i in range(len(self.geo["periods"])):
            q = f"discriminators.{i}."
            conv = lambda j: w[f"{q}convs.{j}.weight"][..., 0]
            if packed is not None:                                  # precision 'bf16': (forward image, bias, channel-transposed image) in bf16
                convs = [(packed[2 * (i * (n - 1) + j - 1)], dev(w[f"{q}convs.{j}.bias"]), packed[2 * (i * (n - 1) + j - 1) + 1]) for j in range(1, n)]
            else:
                convs = [(dev(conv(j).permute(2, 1, 0).reshape(-1, conv(j).shape[0])), dev(w[f"{q}convs.{j}.bias"]),
                          dev(conv(j).permute(2, 0, 1).reshape(-1, conv(j).shape[1]))) for j in range(1, n)]
            self.images.append({"first": (dev(conv(0)[:, 0, :].t()), dev(w[f"{q}convs.0.bias"])), "convs": convs,
                                "post": (dev(w[f"{q}conv_post.weight"][0, :, :, 0].t()), dev(w[f"{q}conv_post.bias"]))})

    def _pack_images(self, w):
        """precision 'bf16': ONE `hifigan_pack_images` launch over a job table covering every period builds the bf16 images of the middle convolutions
        (`hifigan_disc_pack_plan`: per convolution the forward and the channel-transposed image) from the parameters' live storage -> the images in plan
        order.  The job table is built once (again only when a parameter's storage has moved); every rebuild writes a FRESH buffer, whose address goes into
        the table's destination column on the device, so that an earlier forward's backward keeps the images it ran with."""
        plan = self._plan
        src = [w[key].to(self.device) for key, *_ in plan]
        ptrs = tuple(t.data_ptr() for t in src)
        if self._pack is None or self._pack[0] != ptrs:                 # the table: sources, kinds, sizes and first blocks; the destinations follow per rebuild
            offsets, rows, block = [0], [], 0
            for (key, kind, ci, co, taps, rate, shape, _), t in zip(plan, src):
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise _lib.GlowTTSHipError(f"HiFiGANPeriodDiscriminator needs contiguous float32 parameters, got {key}: {t.dtype}")
                n = math.prod(shape) * 2                                # bytes of the bf16 image: a multiple of 16, one thread per 16-byte group
                rows.append([t.data_ptr(), 0, HIFIGAN_PACK_KINDS[kind], ci, co, taps, rate, block])
                block += -(-(n // 16) // 256)
                offsets.append(offsets[-1] + n)
            self._pack = (ptrs, torch.tensor(rows, dtype=torch.int64).to(self.device), torch.tensor(offsets[:-1], dtype=torch.int64).to(self.device), offsets, block)
        _, jobs, offsets_dev, offsets, blocks = self._pack
        flat = torch.empty(offsets[-1], dtype=torch.uint8, device=self.device)  # the launch writes every group of every image, the zero rows included
        # Both launches go to the CURRENT stream, like every launch of the discriminator: the table's column is rewritten after the previous pack launch has
        # read it and before this one does.  Rebuilding on two streams at once is not supported.
        torch.add(offsets_dev, flat.data_ptr(), out=jobs[:, 1])
        ops.hifigan_pack_images(jobs, blocks)
        return [flat[off:end].view(dtype).view(shape) for (*_, shape, dtype), off, end in zip(plan, offsets, offsets[1:])]

    def _check(self, wav):
        if wav.dim() != 2 or wav.dtype != torch.float32 or not wav.is_cuda:
            raise _lib.GlowTTSHipError("HiFiGANPeriodDiscriminator: expected an fp32 device tensor [B, T] (the HIP path has no CPU fallback), got "
                                       f"{list(wav.shape)} {wav.dtype}")
        B, T = wav.shape
        for p in self.geo["periods"]:
            hifigan_disc_rows(self.geo, T, p)
        if B < 1 or B > 65535 or B * (T + MPD_MAX_PERIOD) > 2 ** 30:
            raise ValueError(f"HiFiGANPeriodDiscriminator: a batch of {B} x {T} samples is outside 1 <= B <= 65535, B (T + {MPD_MAX_PERIOD}) <= 2^30")

    def score(self, wav, freeze=False):
        """wav [B, T] -> a list of scores [B, H_last p], one per period, with a backward: d wav summed over the periods in period order and, unless `freeze`,
        the parameter gradients."""
        self._check(wav)
        return list(_PeriodScore.apply(self, wav.contiguous(), freeze, None, *self.params.values()))

    def score_pair(self, real, fake):
        """ONE forward over [real; fake] (2 B rows) per period -> (both: scores [2 B, N_p] per period whose backward yields the parameter gradients alone;
        p_fake: scores [B, N_p] of the fake rows per period, and l_fm: the 0-d sum over periods and maps of mean |lrelu(real map) - lrelu(fake map)| - the
        backward of these two is ONE frozen data chain per period over the fake rows, reaching the fake waveform alone, with no weight-gradient launch;
        fm_terms [periods, widths + 1]: the terms).  The real rows' feature maps are constants."""
        self._check(fake)
        if tuple(real.shape) != tuple(fake.shape):
            raise ValueError(f"HiFiGANPeriodDiscriminator.score_pair: real {list(real.shape)} and fake {list(fake.shape)} differ in shape")
        B = fake.shape[0]
        both = torch.cat([real.detach().to(device=self.device, dtype=torch.float32), fake.detach()]).contiguous()
        self._check(both)
        self._build_images({k: t.detach() for k, t in self.params.items()})
        fwd = hifigan_disc_forward(self, both)
        terms, l_fm, inj = hifigan_disc_feature_matching(self, fwd)
        half = {"wav": both[B:], "images": fwd["images"], "bf16": fwd["bf16"], "periods": [{"p": per["p"], "H": per["H"], "keep": [k[B:] for k in per["keep"]], "scores": per["scores"][B:]}
                                             for per in fwd["periods"]]}
        out = _FakeTerms.apply(self, fake.contiguous(), half, l_fm, inj)
        return list(_PeriodScore.apply(self, both, False, fwd, *self.params.values())), list(out[:-1]), out[-1], terms.detach()

# ================================================================================================================================================
# The HiFi-GAN multi-scale discriminator on the kernels of csrc/hifigan_msd_ops.hip (the dense last layer and conv_post: the multi-period discriminator's
# kernels at period 1): forward, backward, feature matching, f32.  The network is written down in DESIGN.md ("The multi-scale discriminator"); it and the
# checkpoint layout restate the most widely used implementation from memory and are UNPINNED, like the other vocoder contracts.  The block is the optional
# `Vocoder.Train.Adversarial.Multi_Scale`; conv_post's 3 taps and the pool (4 taps, stride 2, padding 2) are constants of the architecture, not yaml keys.
# ================================================================================================================================================
MSD_KEY = MPD_KEY + "." + MSD_BLOCK
MSD_DEFAULTS = {"Scales": 3, "Channels": [128, 128, 256, 512, 1024, 1024, 1024], "Groups": [1, 4, 16, 16, 16, 16, 1], "Strides": [1, 2, 2, 4, 4, 1, 1],
                "Kernel_Sizes": [15, 41, 41, 41, 41, 41, 5]}
MSD_PREFIX = "scale_discriminators."                                # of the multi-scale discriminator's names among the parameters of `HiFiGANDiscriminators`
MSD_POST_TAPS, MSD_LAST_TAPS, MSD_FIRST_MAX_TAPS, MSD_MAX_TAPS, MSD_MAX_SCALES, MSD_MAX_CHANNELS, MSD_MAX_GROUP_IN = 3, 5, 15, 41, 4, 1024, 64
MSD_MIN_LAYERS, MSD_MAX_LAYERS, MSD_STRIDES = 3, 8, (1, 2, 4)
MSD_MIN_SAMPLES = 16            # the shortest waveform: one more than the first layer's 15 taps; at 4 scales its coarsest copy still has 3 samples


def hifigan_msd_settings(hp):
    """The optional yaml block `Vocoder.Train.Adversarial.Multi_Scale` over MSD_DEFAULTS (absent block: None; `{}`: the defaults), checked: a ValueError
    names every unknown or bad key."""
    adv = getattr(getattr(getattr(hp, "Vocoder", None), "Train", None), "Adversarial", None)
    block = getattr(adv, MSD_BLOCK, None)
    if block is None:
        return None
    whole = lambda v: int(v) == v
    ints = lambda v: all(whole(x) for x in v)

    def rules(s, need):
        need("Scales", lambda v: whole(v) and 1 <= int(v) <= MSD_MAX_SCALES, f"an integer in [1, {MSD_MAX_SCALES}]")
        need("Channels", lambda v: MSD_MIN_LAYERS <= len(v) <= MSD_MAX_LAYERS and all(whole(c) and 16 <= int(c) <= MSD_MAX_CHANNELS and int(c) % 16 == 0 for c in v),
             f"{MSD_MIN_LAYERS} to {MSD_MAX_LAYERS} widths, each a multiple of 16 in [16, {MSD_MAX_CHANNELS}]")
        n = len(s["Channels"]) if isinstance(s["Channels"], (list, tuple)) else -1
        mid = lambda v: list(v)[1:-1]
        need("Kernel_Sizes", lambda v: ints(v) and len(v) == n >= 1 and v[0] % 2 == 1 and 1 <= v[0] <= MSD_FIRST_MAX_TAPS and v[-1] == MSD_LAST_TAPS and
             all(k % 2 == 1 and 1 <= k <= MSD_MAX_TAPS for k in mid(v)),
             f"as many as Channels: the first odd and at most {MSD_FIRST_MAX_TAPS}, the last {MSD_LAST_TAPS}, the others odd and at most {MSD_MAX_TAPS}")
        need("Strides", lambda v: ints(v) and len(v) == n >= 1 and v[0] == 1 and v[-1] == 1 and all(x in MSD_STRIDES for x in mid(v)),
             "as many as Channels: the first and the last 1, the others 1, 2 or 4")

        def groups(v):
            ch = [int(c) for c in s["Channels"]]
            if not (ints(v) and len(v) == n >= 1 and v[0] == 1 and v[-1] == 1):
                return False
            return all(g >= 1 and ch[j] % g == 0 and ch[j - 1] % g == 0 and (ch[j] // g) % 16 == 0 and (ch[j - 1] // g) % 4 == 0 and
                       ch[j - 1] // g <= MSD_MAX_GROUP_IN for j, g in list(enumerate(v))[1:-1])
        need("Groups", groups, "as many as Channels: the first and the last 1; for the others Channels[j] / Groups[j] a multiple of 16 and "
             f"Channels[j - 1] / Groups[j] a multiple of 4, at most {MSD_MAX_GROUP_IN}")
    s = overlay_settings(block, MSD_DEFAULTS, MSD_KEY, "vocoder", rules)
    s["Scales"] = int(s["Scales"])
    for k in ("Channels", "Groups", "Strides", "Kernel_Sizes"):
        s[k] = [int(v) for v in s[k]]
    return s


def hifigan_msd_geometry(hp):
    """The multi-scale discriminator's sizes as a dict (scales, channels, groups, strides, kernels, slope) from the block
    `Vocoder.Train.Adversarial.Multi_Scale` (absent: the defaults) and `Negative_Slope` of the block around it; raises ValueError naming the offending yaml
    keys (`hifigan_disc_settings`)."""
    adv = hifigan_disc_settings(hp) or MPD_DEFAULTS
    s = adv.get(MSD_BLOCK) or MSD_DEFAULTS
    return {"scales": int(s["Scales"]), "channels": list(s["Channels"]), "groups": list(s["Groups"]), "strides": list(s["Strides"]),
            "kernels": list(s["Kernel_Sizes"]), "slope": float(adv["Negative_Slope"])}


def hifigan_msd_rows(geo, T):
    """Per scale the rows of its waveform and of every layer's output: [[T_i, L_1, ..., L_n]] with T_0 = T, T_{i+1} = T_i // 2 + 1 (the pool) and
    L' = (L - 1) // stride + 1 (conv_post keeps L_n).  T below MSD_MIN_SAMPLES raises a ValueError naming the key."""
    if T < MSD_MIN_SAMPLES:
        raise ValueError(f"{MSD_KEY}: a waveform of {T} samples is shorter than the {MSD_MIN_SAMPLES} samples the multi-scale discriminator supports")
    rows = []
    for _ in range(geo["scales"]):
        L = [T]
        for s in geo["strides"]:
            L.append((L[-1] - 1) // s + 1)
        rows.append(L)
        T = T // 2 + 1
    return rows


def hifigan_msd_expected_shapes(geo):
    """state-dict key -> shape of the multi-scale discriminator with the sizes `geo` (Conv1d weights [Cout, Cin / groups, k])"""
    e = {}
    for i in range(geo["scales"]):
        cin = 1
        for j, (c, g, k) in enumerate(zip(geo["channels"], geo["groups"], geo["kernels"])):
            e[f"discriminators.{i}.convs.{j}.weight"], e[f"discriminators.{i}.convs.{j}.bias"] = (c, cin // g, k), (c,)
            cin = c
        e[f"discriminators.{i}.conv_post.weight"], e[f"discriminators.{i}.conv_post.bias"] = (1, cin, MSD_POST_TAPS), (1,)
    return e


def hifigan_msd_init(geo, seed=0):
    """A fresh multi-scale discriminator's state dict: torch's default rule per tensor (`conv_default_init`, fan_in = (Cin / groups) k)."""
    return conv_default_init(hifigan_msd_expected_shapes(geo), seed)


def hifigan_msd_find_state_dict(obj):
    """The multi-scale discriminator's state dict inside what torch.load returned: at the top level, under `scale_discriminator` / `msd`, or inside `model`.
    It is told by its 3-d Conv1d weights: the multi-period discriminator's state dict has the same names with 4-d Conv2d weights and is not taken for it."""
    names = ("scale_discriminator", "msd")

    def mine(d):
        first = [v for k, v in d.items() if str(k).startswith("discriminators.0.convs.0.weight") and torch.is_tensor(v)]
        return bool(first) and any(v.dim() == 3 for v in first) and not any(v.dim() == 4 for v in first)
    return find_state_dict(obj, ((),) + tuple((n,) for n in names) + (("model",),) + tuple(("model", n) for n in names), mine,
                           "no HiFi-GAN multi-scale discriminator state dict found (looked for a 3-d `discriminators.0.convs.0.weight*` at the top level, under "
                           "scale_discriminator / msd and inside model)")


def hifigan_msd_load(obj, geo):
    """-> {key: float32 host tensor} with exactly the keys of `hifigan_msd_expected_shapes` (`checked_load`: weight-norm pairs are folded once).  A
    spectral-norm triple (`weight_orig`, `weight_u`, `weight_v`) is refused by name: that parametrisation is out of scope."""
    found = hifigan_msd_find_state_dict(obj)
    spectral = sorted(k for k in found if str(k).endswith(".weight_orig"))
    if spectral:
        raise ValueError(f"multi-scale discriminator checkpoint: {spectral[0]} is a spectral-norm parametrisation, which this project does not load "
                         "(fold it into a plain `weight` first)")
    return checked_load(found, hifigan_msd_expected_shapes(geo), "multi-scale discriminator", "multi-scale discriminator", MSD_KEY)


def hifigan_msd_forward(disc, wav, alloc=None):
    """The forward launches on wav [B, T] (fp32, contiguous, on the device) -> dict(wav, scales: per scale dict(i, L, x, keep, scores)).  x [B, L[0]] is the
    scale's waveform (scale i: i pools), keep[j] [B, L[j + 1], C_j] layer j's PRE-activation output, scores [B, L[-1]] conv_post's.  alloc(*shape): the
    caller's buffers (tests)."""
    g, lib, P, st = disc.geo, _lib.api(), _lib.ptr, _lib.stream()
    B, T = wav.shape
    ch, groups, strides, ks, slope, n = g["channels"], g["groups"], g["strides"], g["kernels"], g["slope"], len(g["channels"])
    f = alloc or (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=wav.device))
    out, x = [], wav
    for i, (L, im) in enumerate(zip(hifigan_msd_rows(g, T), disc.images)):
        if i:
            y = f(B, L[0])
            lib.glowtts_hifigan_msd_pool(P(x), P(y), B, x.shape[1], st)
            x = y
        keep = [f(B, L[j + 1], c) for j, c in enumerate(ch)]
        scores = f(B, L[-1])
        lib.glowtts_hifigan_msd_first(P(x), P(im["first"][0]), P(im["first"][1]), P(keep[0]), B, L[0], ks[0], ch[0], st)
        for j in range(1, n - 1):
            w, b, _ = im["convs"][j - 1]
            lib.glowtts_hifigan_msd_conv(P(keep[j - 1]), P(w), P(b), P(keep[j]), B, L[j], ks[j], strides[j], groups[j], ch[j - 1], ch[j], slope, st)
        w, b, _ = im["last"]
        lib.glowtts_hifigan_msd_dense(P(keep[n - 2]), P(w), P(b), P(keep[n - 1]), B, L[n - 1], ch[n - 2], ch[n - 1], slope, st)
        lib.glowtts_hifigan_msd_post(P(keep[-1]), P(im["post"][0]), P(im["post"][1]), P(scores), B, L[-1], ch[-1], slope, st)
        out.append({"i": i, "L": L, "x": x, "keep": keep, "scores": scores})
    return {"wav": wav, "scales": out, "images": disc.images}       # the images this forward ran with: its backward must not see a later rebuild


def hifigan_msd_feature_maps(disc, scale_fwd):
    """The feature maps of one scale of `hifigan_msd_forward` in torch's layout: the activated outputs [B, C_j, L], then conv_post's [B, 1, L]."""
    return [torch.nn.functional.leaky_relu(k, disc.geo["slope"]).permute(0, 2, 1) for k in scale_fwd["keep"]] + [scale_fwd["scores"][:, None, :]]


def hifigan_msd_work(disc, B, T, device, alloc=None):
    """The work buffer of the backward and of the feature-matching loss on a batch of B x T: the largest layer's `glowtts_hifigan_msd_work_floats` (the
    dense layers: `glowtts_hifigan_disc_work_floats`)."""
    g, lib = disc.geo, _lib.api()
    ch, n, floats = g["channels"], len(g["channels"]), 0
    for L in hifigan_msd_rows(g, T):
        cin = 1
        for j in range(n - 1):
            floats, cin = max(floats, lib.glowtts_hifigan_msd_work_floats(B, L[j + 1], cin, ch[j], g["kernels"][j], g["groups"][j])), ch[j]
        floats = max(floats, lib.glowtts_hifigan_disc_work_floats(B, L[n], cin, ch[-1], MSD_LAST_TAPS), lib.glowtts_hifigan_disc_work_floats(B, L[n], ch[-1], 1, MSD_POST_TAPS))
    f = alloc or (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=device))
    return f(floats)


def hifigan_msd_feature_matching(disc, fwd, alloc=None):
    """The feature-matching terms of a forward over [real; fake] (2 B rows) -> (terms [scales, layers + 1], l_fm [1], inj), as `hifigan_disc_feature_matching`
    gives them for the periods: `glowtts_hifigan_disc_fm` per map, added up by the kernels in launch order (scale, then map)."""
    g, lib, P, st = disc.geo, _lib.api(), _lib.ptr, _lib.stream()
    B2, T = fwd["wav"].shape
    B, dev = B2 // 2, fwd["wav"].device
    f = alloc or (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev))
    work, terms, total, inj = hifigan_msd_work(disc, B, T, dev, alloc), f(g["scales"], len(g["channels"]) + 1), f(1), []
    for i, sc in enumerate(fwd["scales"]):
        maps = [(k, g["slope"]) for k in sc["keep"]] + [(sc["scores"], 1.0)]
        inj.append([f(B, *k.shape[1:]) for k, _ in maps])
        for j, (k, slope) in enumerate(maps):
            lib.glowtts_hifigan_disc_fm(P(k), P(inj[i][j]), P(work), P(terms[i, j:]), P(total), k.numel() // 2, slope, 1 if i or j else 0, st)
    return terms, total, inj


def hifigan_msd_backward(disc, fwd, dscores, freeze=False, inj=None, inj_scale=None, need_dwav=True, alloc=None):
    """d scores (one [B, L_last] per scale) -> (d wav [B, T], or None unless `need_dwav`; {name: gradient in torch's layout} or None when `freeze`) from what
    `hifigan_msd_forward` kept (or the views of some of its batch rows).  d wav: every scale's d of its own waveform, then from the coarsest scale down each is
    sent through the pool's gradient and added to the next finer one.  inj (`hifigan_msd_feature_matching`) times the device scalar inj_scale is added to
    every d pre and to d scores on the way down.  freeze: the data chain alone, no weight-gradient launch."""
    g, lib, P, st = disc.geo, _lib.api(), _lib.ptr, _lib.stream()
    wav = fwd["wav"]
    B, T = wav.shape
    ch, groups, strides, ks, slope, dev, n = g["channels"], g["groups"], g["strides"], g["kernels"], g["slope"], wav.device, len(g["channels"])
    f = alloc or (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev))
    grads = work = None
    if not freeze:
        grads, work = {k: f(*shape) for k, shape in hifigan_msd_expected_shapes(g).items()}, hifigan_msd_work(disc, B, T, dev, alloc)
    scale = P(inj_scale) if inj is not None else None
    opt = lambda t: P(t) if t is not None else None
    dxs = []
    for i, (sc, im, ds) in enumerate(zip(fwd["scales"], fwd["images"], dscores)):
        L, keep, q = sc["L"], sc["keep"], f"discriminators.{i}."
        ds, ij = ds.to(torch.float32).contiguous(), inj[i] if inj is not None else [None] * (n + 1)
        gw = lambda name: (P(grads[q + name + ".weight"]), P(grads[q + name + ".bias"]))
        d = f(B, L[n], ch[-1])
        lib.glowtts_hifigan_msd_post_bwd(P(ds), opt(ij[n]), P(keep[-1]), P(im["post"][0]), opt(ij[n - 1]), scale, P(d), B, L[n], ch[-1], slope, st)
        if not freeze:
            lib.glowtts_hifigan_msd_dense_wgrad(P(keep[-1]), P(ds), P(work), *gw("conv_post"), B, L[n], ch[-1], 1, MSD_POST_TAPS, slope, st)
            lib.glowtts_hifigan_msd_dense_wgrad(P(keep[n - 2]), P(d), P(work), *gw(f"convs.{n - 1}"), B, L[n - 1], ch[n - 2], ch[n - 1], MSD_LAST_TAPS, slope, st)
        dx = f(B, L[n - 1], ch[n - 2])
        lib.glowtts_hifigan_msd_dense_bwd(P(d), P(im["last"][2]), P(keep[n - 2]), opt(ij[n - 2]), scale, P(dx), B, L[n - 1], ch[n - 2], ch[n - 1], slope, st)
        d = dx
        for j in reversed(range(1, n - 1)):
            if not freeze:
                lib.glowtts_hifigan_msd_wgrad(P(keep[j - 1]), P(d), P(work), *gw(f"convs.{j}"), B, L[j], ks[j], strides[j], groups[j], ch[j - 1], ch[j], slope, st)
            dx = f(B, L[j], ch[j - 1])
            lib.glowtts_hifigan_msd_conv_bwd(P(d), P(im["convs"][j - 1][2]), P(keep[j - 1]), opt(ij[j - 1]), scale, P(dx), B, L[j], ks[j], strides[j], groups[j],
                                             ch[j - 1], ch[j], slope, st)
            d = dx
        if not freeze:
            lib.glowtts_hifigan_msd_first_wgrad(P(sc["x"]), P(d), P(work), *gw("convs.0"), B, L[0], ks[0], ch[0], st)
        if need_dwav:
            dxs.append(f(B, L[0]))
            lib.glowtts_hifigan_msd_first_bwd(P(d), P(im["first"][0]), P(dxs[-1]), B, L[0], ks[0], ch[0], 0, st)
    if not need_dwav:
        return None, grads
    for i in reversed(range(1, len(dxs))):                          # the scales add up through the pools, from the coarsest to the finest
        lib.glowtts_hifigan_msd_pool_bwd(P(dxs[i]), P(dxs[i - 1]), B, dxs[i - 1].shape[1], 1, st)
    return dxs[0], grads


class HiFiGANScaleDiscriminator:
    """HiFiGANScaleDiscriminator(hp, device, state_dict=None, trainable=True, seed=0): the multi-scale discriminator.  The sizes come from the yaml block
    `Vocoder.Train.Adversarial.Multi_Scale` (absent: the defaults).  `params` holds float32 device leaves in `hifigan_msd_expected_shapes`' names - from
    `state_dict` (`hifigan_msd_load`) or, without one, `hifigan_msd_init(geo, seed)`; the weight images are rebuilt from them at every call.  A row's scores,
    feature maps and d wav are bit-identical alone, in any batch and from run to run."""
    OPS, NETS = (hifigan_msd_forward, hifigan_msd_backward), "scales"

    def __init__(self, hp, device="cuda:0", state_dict=None, trainable=True, seed=0):
        self.geo = geo = hifigan_msd_geometry(hp)                   # before anything touches the device
        self.trainable = bool(trainable)
        w = hifigan_msd_load(state_dict, geo) if state_dict is not None else hifigan_msd_init(geo, seed)
        lib, widths = _lib.api(), [1] + geo["channels"] + [1]
        layers = zip(widths, widths[1:], geo["kernels"] + [MSD_POST_TAPS], geo["strides"] + [1], geo["groups"] + [1])
        if not all(lib.glowtts_hifigan_msd_supported(*layer) for layer in layers):
            raise ValueError(f"the {MSD_KEY} block's sizes {geo} are not supported by the kernels")
        self.device = torch.device(device)
        self.params = {k: t.to(self.device).requires_grad_(self.trainable) for k, t in w.items()}
        self._build_images({k: t.detach() for k, t in self.params.items()})

    def _build_images(self, w):
        """Per scale the weight images in the kernels' layouts: first [k][C0] and post [3][C] (row = tap); a grouped layer's forward image
        [groups][k Cin_g][Cout_g] (row = tap Cin_g + input channel of the group) and its backward image [groups][k][Cout_g][Cin_g rounded up to 16, the
        new columns zero]; the dense last layer's [5 Cin][Cout] and [5 Cout][Cin]."""
        dev, g = (lambda t: t.contiguous().to(self.device)), self.geo
        n = len(g["channels"])
        self.images = []
        for i in range(g["scales"]):
            q = f"discriminators.{i}."
            convs = []
            for j in range(1, n - 1):
                wj, G = w[f"{q}convs.{j}.weight"], g["groups"][j]
                v = wj.reshape(G, wj.shape[0] // G, wj.shape[1], wj.shape[2])                      # [G, Cout_g, Cin_g, k]
                back = torch.nn.functional.pad(v.permute(0, 3, 1, 2), (0, -wj.shape[1] % 16))
                convs.append((dev(v.permute(0, 3, 2, 1).reshape(G, -1, v.shape[1])), dev(w[f"{q}convs.{j}.bias"]), dev(back)))
            last = w[f"{q}convs.{n - 1}.weight"]
            self.images.append({"first": (dev(w[f"{q}convs.0.weight"][:, 0, :].t()), dev(w[f"{q}convs.0.bias"])), "convs": convs,
                                "last": (dev(last.permute(2, 1, 0).reshape(-1, last.shape[0])), dev(w[f"{q}convs.{n - 1}.bias"]),
                                         dev(last.permute(2, 0, 1).reshape(-1, last.shape[1]))),
                                "post": (dev(w[f"{q}conv_post.weight"][0].t()), dev(w[f"{q}conv_post.bias"]))})

    def _check(self, wav):
        if wav.dim() != 2 or wav.dtype != torch.float32 or not wav.is_cuda:
            raise _lib.GlowTTSHipError("HiFiGANScaleDiscriminator: expected an fp32 device tensor [B, T] (the HIP path has no CPU fallback), got "
                                       f"{list(wav.shape)} {wav.dtype}")
        B, T = wav.shape
        hifigan_msd_rows(self.geo, T)
        if B < 1 or B > 65535 or B * T > 2 ** 30:
            raise ValueError(f"HiFiGANScaleDiscriminator: a batch of {B} x {T} samples is outside 1 <= B <= 65535, B T <= 2^30")

    def score(self, wav, freeze=False):
        """wav [B, T] -> a list of scores [B, L_last], one per scale, with a backward: d wav summed over the scales and, unless `freeze`, the parameter
        gradients."""
        self._check(wav)
        return list(_PeriodScore.apply(self, wav.contiguous(), freeze, None, *self.params.values()))

    def score_pair(self, real, fake):
        """`HiFiGANPeriodDiscriminator.score_pair` for the scales: ONE forward over [real; fake] (2 B rows) -> (both: scores [2 B, L_last] per scale whose
        backward yields the parameter gradients alone; p_fake: the fake rows' scores per scale, and l_fm: the 0-d sum over scales and maps of
        mean |lrelu(real map) - lrelu(fake map)| - their backward is ONE frozen data chain per scale over the fake rows, with no weight-gradient launch;
        fm_terms [scales, layers + 1])."""
        self._check(fake)
        if tuple(real.shape) != tuple(fake.shape):
            raise ValueError(f"HiFiGANScaleDiscriminator.score_pair: real {list(real.shape)} and fake {list(fake.shape)} differ in shape")
        B = fake.shape[0]
        both = torch.cat([real.detach().to(device=self.device, dtype=torch.float32), fake.detach()]).contiguous()
        self._check(both)
        self._build_images({k: t.detach() for k, t in self.params.items()})
        fwd = hifigan_msd_forward(self, both)
        terms, l_fm, inj = hifigan_msd_feature_matching(self, fwd)
        half = {"wav": both[B:], "images": fwd["images"], "scales": [{"i": sc["i"], "L": sc["L"], "x": sc["x"][B:], "keep": [k[B:] for k in sc["keep"]],
                                                                     "scores": sc["scores"][B:]} for sc in fwd["scales"]]}
        out = _FakeTerms.apply(self, fake.contiguous(), half, l_fm, inj)
        return list(_PeriodScore.apply(self, both, False, fwd, *self.params.values())), list(out[:-1]), out[-1], terms.detach()


def hifigan_discs_split(sd):
    """The parameters of `HiFiGANDiscriminators` -> (the multi-period discriminator's, the multi-scale discriminator's under its own names)"""
    return ({k: v for k, v in sd.items() if not str(k).startswith(MSD_PREFIX)}, {str(k)[len(MSD_PREFIX):]: v for k, v in sd.items() if str(k).startswith(MSD_PREFIX)})


def hifigan_discs_load(obj, geo):
    """-> {key: float32 host tensor} of both discriminators (geo: dict(periods, scales) of their sizes) from the union `HiFiGANDiscriminators.params` names:
    found at the top level, under `discriminator` or inside `model`; each half goes through its own loader's checks.  A union without the scales' names
    raises a ValueError naming the first of them."""
    found = find_state_dict(obj, ((), ("discriminator",), ("model",), ("model", "discriminator")),
                            lambda d: any(str(k).startswith("discriminators.0.convs.0.weight") for k in d),
                            "no HiFi-GAN discriminator state dict found (looked for `discriminators.0.convs.0.weight*` at the top level, under discriminator and "
                            "inside model)")
    mpd, msd = hifigan_discs_split(found)
    if not msd:
        raise ValueError(f"discriminator checkpoint: missing key {MSD_PREFIX}discriminators.0.convs.0.weight (it was written without the block {MSD_KEY})")
    out = hifigan_disc_load(mpd, geo["periods"])
    out.update({MSD_PREFIX + k: v for k, v in hifigan_msd_load(msd, geo["scales"]).items()})
    return out


class HiFiGANDiscriminators:
    """HiFiGANDiscriminators(hp, device, state_dict=None, trainable=True, seed=0, precision=None): the multi-period and the multi-scale discriminator as the
    ONE discriminator of the adversarial stage.  precision ('f32' / 'bf16' / None: the yaml's `Vocoder.Train.Adversarial.Precision`) is handed to the period
    discriminator and governs it alone: the multi-scale discriminator stays f32 entirely.  `params`: the multi-period discriminator's names unchanged, then the multi-scale discriminator's under `scale_discriminators.`.
    state_dict: what `hifigan_discs_load` reads."""

    def __init__(self, hp, device="cuda:0", state_dict=None, trainable=True, seed=0, precision=None):
        self.geo = {"periods": hifigan_disc_geometry(hp), "scales": hifigan_msd_geometry(hp)}                  # before anything touches the device
        self.precision = hifigan_disc_precision(hp, precision)                                                 # the period discriminator's; the scales are f32
        mpd = msd = None
        if state_dict is not None:
            mpd, msd = hifigan_discs_split(hifigan_discs_load(state_dict, self.geo))
        self.periods = HiFiGANPeriodDiscriminator(hp, device, mpd, trainable, seed, precision=self.precision)
        self.scales = HiFiGANScaleDiscriminator(hp, device, msd, trainable, seed)
        self.device, self.trainable = self.periods.device, bool(trainable)
        self.params = dict(self.periods.params)
        self.params.update({MSD_PREFIX + k: t for k, t in self.scales.params.items()})

    def score(self, wav, freeze=False):
        """-> the periods' scores, then the scales'"""
        return self.periods.score(wav, freeze) + self.scales.score(wav, freeze)

    def score_pair(self, real, fake):
        """-> (both, p_fake: the periods' lists with the scales' appended; l_fm: the periods' sum + the scales' sum; the periods' terms; the scales' terms)"""
        both, p_fake, l_fm, terms = self.periods.score_pair(real, fake)
        both_s, p_fake_s, l_fm_s, terms_s = self.scales.score_pair(real, fake)
        return both + both_s, p_fake + p_fake_s, l_fm + l_fm_s, terms, terms_s


VOCODER_KINDS = ("griffin_lim", "pwg", "hifigan")


def vocoder_kind(hp, kind=None, checkpoint=None):
    """Which vocoder a run uses: `kind` when given; else 'hifigan' for a `Vocoder` block whose Type is 'HiFiGAN', 'pwg' for any other `Vocoder` block or a
    checkpoint argument alone, 'griffin_lim' without either."""
    if kind not in (None,) + VOCODER_KINDS:
        raise ValueError("vocoder must be 'pwg', 'hifigan', 'griffin_lim' or None, got {!r}".format(kind))
    block = getattr(hp, "Vocoder", None)
    if kind is None and getattr(block, "Type", None) == "HiFiGAN":
        return "hifigan"
    return kind or ("pwg" if checkpoint or block is not None else "griffin_lim")


def make_vocoder(hp, device, kind=None, checkpoint=None, precision=None):
    """The one place that chooses a vocoder: `kind` as `vocoder_kind` resolves it; `checkpoint` overrides `Vocoder.Checkpoint_Path` of the yaml; `precision`
    is the neural vocoders' (Griffin-Lim ignores it; Parallel WaveGAN takes 'f32' / 'bf16', HiFi-GAN 'f32' / 'f16')."""
    import argparse
    import copy
    kind = vocoder_kind(hp, kind, checkpoint)
    if kind == "griffin_lim":
        return GriffinLim(hp, device)
    settings = pwg_settings if kind == "pwg" else hifigan_settings
    if checkpoint:                                                  # the argument overrides the yaml's path
        hp = copy.copy(hp)
        hp.Vocoder = argparse.Namespace(**dict(settings(hp), Checkpoint_Path=checkpoint))
    return (ParallelWaveGAN if kind == "pwg" else HiFiGAN)(hp, device, precision=precision)
