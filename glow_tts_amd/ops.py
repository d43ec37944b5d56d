"""Thin Python wrappers over the C ABI (include/glowtts_hip.h): argument marshalling only.
Every function launches asynchronously on torch's current HIP stream, through the checked handle `_lib.api()`: a status other than GLOWTTS_OK raises there."""
import ctypes

import torch

from . import _lib
from ._lib import c_int
from .abi import (APRO_NONE, APRO_PAIRMUL, APRO_SQNEG, BF16, EPI_COUPLE, EPI_DGATE, EPI_GATE, EPI_LINEAR, EPI_RESSKIP, F32, F_ACCUM, F_ADD_IN0, F_BIAS,  # noqa: F401
                  F_COLMASK, F_DROPOUT, F_FIRST, F_GATE_IN0, F_LAST, F_MASK, F_RELU, F_REVERSE, IO_A_BF16, IO_IN0_BF16, IO_OUT0_BF16, PERM_NONE, PERM_PAIR,
                  WIO_DMA, WIO_DY_BF16, WIO_WIDE, WIO_X_BF16, ConvArgs, PackJob)


class PackedWeight:
    """A conv weight in MFMA tile order (glowtts_pack_weight)."""
    __slots__ = ("data", "npad", "kchunks", "taps", "precision", "n")

    def __init__(self, data, npad, kchunks, taps, precision, n):
        self.data, self.npad, self.kchunks, self.taps, self.precision, self.n = data, npad, kchunks, taps, precision, n


def pack_weight(w, transpose=False, perm=PERM_NONE, perm_h=0, precision=BF16):
    """w: fp32 device tensor [O, I, taps] (torch Conv1d layout) -> PackedWeight."""
    L = _lib.api()
    w = w.contiguous()
    O, I, taps = w.shape
    npad, kch = c_int(0), c_int(0)
    L.glowtts_pack_weight(None, O, I, taps, int(transpose), perm, perm_h, precision, None, ctypes.byref(npad), ctypes.byref(kch), None)
    buf = torch.empty(taps * kch.value * npad.value * 64, dtype=torch.uint8, device=w.device)
    L.glowtts_pack_weight(_lib.ptr(w), O, I, taps, int(transpose), perm, perm_h, precision, _lib.ptr(buf), None, None, _lib.stream())
    n = I if transpose else O
    return PackedWeight(buf, npad.value, kch.value, taps, precision, n)


class PackSet:
    """Conv weights of different shapes packed by ONE launch (glowtts_pack_weight_multi) into one buffer.
    items: [(key, fp32 weight [O, I, taps], transpose)].  The device job table is built once; `run()` re-packs the current values
    (call it once per forward: the optimizer changes them in place).  `matches(items)` tells whether the pointers still hold."""

    def __init__(self, items, precision=BF16):
        L = _lib.api()
        assert items
        dev = items[0][1].device
        n = len(items)
        jobs = (PackJob * n)()
        blocks, nbytes = c_int(0), ctypes.c_int64(0)
        offs, total = [], 0
        for i, (_, w, tr) in enumerate(items):
            assert w.dim() == 3 and w.is_contiguous() and w.dtype == torch.float32
            O, I, k = w.shape
            L.glowtts_pack_job_init(ctypes.byref(jobs[i]), None, O, I, k, int(tr), PERM_NONE, 0, precision, None, 0, ctypes.byref(blocks), ctypes.byref(nbytes))
            offs.append(total)
            total += (nbytes.value + 255) // 256 * 256
        self.data = torch.empty(total, dtype=torch.uint8, device=dev)
        self.packed, b0 = {}, 0
        for i, (key, w, tr) in enumerate(items):
            O, I, k = w.shape
            L.glowtts_pack_job_init(ctypes.byref(jobs[i]), w.data_ptr(), O, I, k, int(tr), PERM_NONE, 0, precision,
                                    self.data.data_ptr() + offs[i], b0, ctypes.byref(blocks), ctypes.byref(nbytes))
            b0 += blocks.value
            self.packed[(key, bool(tr))] = PackedWeight(self.data[offs[i]:offs[i] + nbytes.value], jobs[i].npad, jobs[i].kchunks, k, precision,
                                                        I if tr else O)
        self.table = torch.frombuffer(bytearray(jobs), dtype=torch.uint8).to(dev)
        self.njobs, self.blocks, self.precision = n, b0, precision
        self.sig = self.signature(items)

    @staticmethod
    def signature(items):
        return tuple((k, w.data_ptr(), tuple(w.shape), bool(tr)) for k, w, tr in items)

    def run(self):
        _lib.api().glowtts_pack_weight_multi(self.table.data_ptr(), self.njobs, self.blocks, self.precision, _lib.stream())

    def get(self, key):
        """(forward pack, transposed pack or None)"""
        return self.packed[(key, False)], self.packed.get((key, True))


def conv_cl(a, pw, ca, rows, *, lda=None, a2=None, lda2=0, ca1=0, apro=APRO_NONE, pad=0, epi=EPI_LINEAR, flags=0,
            n=None, h=0, rows_per_utt=1, bias=None, rowmask=None, cond=None, ldcond=0,
            out0=None, ld0=0, out1=None, ld1=0, in0=None, ldi0=0, out0_off=0, a_off=0, drop_p=0.0, seed=0, seed_t=None, io_flags=0):
    """Launches glowtts_conv_cl.  Tensors are fp32 device tensors; *_off are element offsets into them
    (to address a channel sub-range of a wider row).  io_flags (IO_*): a / in0 / out0 are bf16 tensors instead."""
    args = ConvArgs()
    args.a = a.data_ptr() + 4 * a_off
    args.lda = lda if lda is not None else a.shape[-1]
    args.a2 = a2.data_ptr() if a2 is not None else None
    args.lda2 = lda2
    args.ca1, args.ca, args.apro, args.rows = ca1, ca, apro, rows
    args.w = pw.data.data_ptr()
    args.n = n if n is not None else pw.n
    args.npad, args.kchunks, args.taps, args.pad, args.precision = pw.npad, pw.kchunks, pw.taps, pad, pw.precision
    args.epi, args.flags, args.h, args.rows_per_utt = epi, flags, h, rows_per_utt
    args.bias = bias.data_ptr() if bias is not None else None
    args.rowmask = rowmask.data_ptr() if rowmask is not None else None
    args.cond = cond.data_ptr() if cond is not None else None
    args.ldcond = ldcond
    args.out0 = out0.data_ptr() + 4 * out0_off
    args.ld0 = ld0
    args.out1 = out1.data_ptr() if out1 is not None else None
    args.ld1 = ld1
    args.in0 = in0.data_ptr() if in0 is not None else None
    args.ldi0 = ldi0
    args.drop_p, args.seed = float(drop_p), int(seed) & 0xFFFFFFFF
    args.seed_ptr = seed_t.data_ptr() if seed_t is not None else None
    args.io_flags = io_flags
    assert not (io_flags and (a_off or out0_off))
    _lib.api().glowtts_conv_cl(ctypes.byref(args), _lib.stream())


# ---- Griffin-Lim vocoder (csrc/vocoder_ops.hip).  geo = (n_fft, win_length, hop); lengths: int32 device tensors [B] ----
def mel_to_linear(mels, frame_lengths, basis, mag, max_abs):
    """mels [B, Mel, T] -> mag [B, T, F] (glowtts_mel_to_linear_f32)."""
    B, Mel, T = mels.shape
    _lib.api().glowtts_mel_to_linear_f32(_lib.ptr(mels), _lib.ptr(frame_lengths), _lib.ptr(basis), _lib.ptr(mag), B, Mel, T, mag.shape[2], float(max_abs), _lib.stream())


def stft(wav, wav_lengths, window, twiddle, spec, geo):
    """wav [B, L] -> spec [B, T, F, 2] (glowtts_stft_f32)."""
    _lib.api().glowtts_stft_f32(_lib.ptr(wav), _lib.ptr(wav_lengths), _lib.ptr(window), _lib.ptr(twiddle), _lib.ptr(spec), wav.shape[0],
                                wav.shape[1], spec.shape[1], *geo, _lib.stream())


def istft(spec, frame_lengths, window, twiddle, frames, wav, geo):
    """spec [B, T, F, 2] -> wav [B, L >= hop (T - 1)] through frames [B, T, win] (glowtts_istft_f32)."""
    _lib.api().glowtts_istft_f32(_lib.ptr(spec), _lib.ptr(frame_lengths), _lib.ptr(window), _lib.ptr(twiddle), _lib.ptr(frames), _lib.ptr(wav),
                                 spec.shape[0], spec.shape[1], wav.shape[1], *geo, _lib.stream())


def overlap_add(frames, frame_lengths, window, wav, geo):
    """frames [B, T, win] -> wav [B, L] (glowtts_overlap_add_f32)."""
    _lib.api().glowtts_overlap_add_f32(_lib.ptr(frames), _lib.ptr(frame_lengths), _lib.ptr(window), _lib.ptr(wav), frames.shape[0], frames.shape[1],
                                       wav.shape[1], *geo, _lib.stream())


def griffin_lim_step(x, x_prev, mag, frame_lengths, window, twiddle, alpha, frames, geo):
    """One fused Griffin-Lim iteration: (x, x_prev) [B, L], mag [B, T, F] -> frames [B, T, win] (glowtts_griffin_lim_step_f32)."""
    _lib.api().glowtts_griffin_lim_step_f32(_lib.ptr(x), _lib.ptr(x_prev), _lib.ptr(mag), _lib.ptr(frame_lengths), _lib.ptr(window), _lib.ptr(twiddle),
                                            float(alpha), _lib.ptr(frames), mag.shape[0], mag.shape[1], x.shape[1], *geo, _lib.stream())


# ---- analysis front end (csrc/frontend_ops.hip).  wav [B, L] fp32, wav_lengths int32 [B], both on the device ----
def mel_analysis(wav, wav_lengths, window, twiddle, fb_index, fb_weight, mel, geo, pre_emphasis, min_db, max_abs):
    """wav [B, L] -> normalised mel [B, T, Mel] (glowtts_mel_analysis_f32); fb_index [Mel, 3] int32 / fb_weight: the sparse filterbank."""
    B, T, Mel = mel.shape
    _lib.api().glowtts_mel_analysis_f32(_lib.ptr(wav), _lib.ptr(wav_lengths), _lib.ptr(window), _lib.ptr(twiddle), _lib.ptr(fb_index),
                                        _lib.ptr(fb_weight), _lib.ptr(mel), B, wav.shape[1], T, Mel, fb_weight.numel(), *geo, float(pre_emphasis),
                                        float(min_db), float(max_abs), _lib.stream())


def yin(wav, wav_lengths, pitch, w_len, w_step, tau_min, tau_max, thresh, sample_rate, cmnd=None):
    """wav [B, L] -> pitch [B, T] in Hz, 0 where unvoiced (glowtts_yin_f32); cmnd [B, T, tau_max]: optionally the normalised difference function."""
    B, T = pitch.shape
    _lib.api().glowtts_yin_f32(_lib.ptr(wav), _lib.ptr(wav_lengths), _lib.ptr(pitch), _lib.ptr(cmnd), B, wav.shape[1], T, int(w_len), int(w_step),
                               int(tau_min), int(tau_max), float(thresh), float(sample_rate), _lib.stream())


# ---- neural vocoder (csrc/pwg_ops.hip).  Rows are samples, channels-last; frame_lengths: int32 device tensor [B] ----
def pwg_condition(mels, frame_lengths, w_in, firs, scales, work, c, ctx):
    """mels [B, A, Lmax] -> c [B, Lmax * hop, A] (glowtts_pwg_condition); scales: a ctypes int array on the host."""
    B, A, Lmax = mels.shape
    _lib.api().glowtts_pwg_condition(_lib.ptr(mels), _lib.ptr(frame_lengths), _lib.ptr(w_in), _lib.ptr(firs), scales, len(scales), _lib.ptr(work),
                                     _lib.ptr(c), B, A, Lmax, int(ctx), _lib.stream())


def pwg_first(noises, seeds, frame_lengths, w, bias, x, Lmax, hop):
    """x [B, Lmax * hop, R] = first_conv(z); z: noises [B, Lmax * hop] or the in-kernel draw from seeds [B, 2] (glowtts_pwg_first)."""
    _lib.api().glowtts_pwg_first(_lib.ptr(noises), _lib.ptr(seeds), _lib.ptr(frame_lengths), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(x), x.shape[0],
                                 int(Lmax), int(hop), x.shape[2], _lib.stream())


def pwg_layer(x, c, w1, b1, w2, b2, x_out, skips, frame_lengths, Lmax, hop, dilation, accumulate):
    """One WaveNet layer (glowtts_pwg_layer): x, x_out [B, Lmax * hop, R], c [.., A], skips [.., S]."""
    _lib.api().glowtts_pwg_layer(_lib.ptr(x), _lib.ptr(c), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(x_out), _lib.ptr(skips),
                                 _lib.ptr(frame_lengths), x.shape[0], int(Lmax), int(hop), x.shape[2], skips.shape[2], c.shape[2], int(dilation),
                                 int(bool(accumulate)), _lib.stream())


def pwg_layer_bf16(x, c, w1p, b1, w2p, b2, x_out, skips, frame_lengths, Lmax, hop, dilation, accumulate):
    """One WaveNet layer with bf16 operands (glowtts_pwg_layer_bf16): as `pwg_layer`; w1p, w2p: the packed bf16 images of `vocoder.pwg_pack_bf16`."""
    R, S, A = x.shape[2], skips.shape[2], c.shape[2]
    if w1p.dtype != torch.bfloat16 or w2p.dtype != torch.bfloat16 or tuple(w1p.shape) != ((3 * R + A + 31) // 32 * 4, 2 * R, 8) or \
            tuple(w2p.shape) != ((R + 31) // 32 * 4, R + S, 8):
        raise _lib.GlowTTSHipError("glowtts_pwg_layer_bf16 needs the packed bf16 weight images of vocoder.pwg_pack_bf16 for these sizes")
    _lib.api().glowtts_pwg_layer_bf16(_lib.ptr(x), _lib.ptr(c), _lib.ptr(w1p), _lib.ptr(b1), _lib.ptr(w2p), _lib.ptr(b2), _lib.ptr(x_out), _lib.ptr(skips),
                                      _lib.ptr(frame_lengths), x.shape[0], int(Lmax), int(hop), R, S, A, int(dilation), int(bool(accumulate)), _lib.stream())


def pwg_head(skips, frame_lengths, w1, b1, w2, b2, wav, Lmax, hop, scale):
    """skips [B, Lmax * hop, S] -> wav [B, Lmax * hop], zero beyond each utterance (glowtts_pwg_head)."""
    _lib.api().glowtts_pwg_head(_lib.ptr(skips), _lib.ptr(frame_lengths), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(wav),
                                skips.shape[0], int(Lmax), int(hop), skips.shape[2], float(scale), _lib.stream())


# ---- neural vocoder (csrc/hifigan_ops.hip).  Rows are samples, channels-last; frame_lengths: int32 device tensor [B]; w: K-major images [taps * Cin, Cout] ----
def hifigan_conv(x, w, bias, out, frame_lengths, Lmax, mult, taps, dilation, slope=1.0, residual=None, accumulate=0, divisor=1.0, channels_first=False):
    """out [B, Lmax * mult, Cout] from x [B, Lmax * mult, Cin] (channels_first: [B, Cin, Lmax * mult]): one dilated convolution (glowtts_hifigan_conv)."""
    Cin = x.shape[1] if channels_first else x.shape[2]
    _lib.api().glowtts_hifigan_conv(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(residual), _lib.ptr(out), _lib.ptr(frame_lengths), x.shape[0], int(Lmax),
                                    int(mult), Cin, out.shape[2], int(taps), int(dilation), float(slope), int(accumulate), float(divisor), int(bool(channels_first)),
                                    _lib.stream())


def hifigan_upsample(x, w, bias, out, frame_lengths, Lmax, mult, taps, rate, slope):
    """x [B, Lmax * mult, Cin] -> out [B, Lmax * mult * rate, Cout]: the transposed convolution in polyphase form (glowtts_hifigan_upsample)."""
    _lib.api().glowtts_hifigan_upsample(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(frame_lengths), x.shape[0], int(Lmax), int(mult),
                                        x.shape[2], out.shape[2], int(taps), int(rate), float(slope), _lib.stream())


def hifigan_post(x, w, bias, wav, frame_lengths, Lmax, mult, taps, slope):
    """x [B, Lmax * mult, Cin] -> wav [B, Lmax * mult] = tanh(conv_post(lrelu(x))), zero beyond each utterance (glowtts_hifigan_post)."""
    _lib.api().glowtts_hifigan_post(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(wav), _lib.ptr(frame_lengths), x.shape[0], int(Lmax), int(mult), x.shape[2],
                                    int(taps), float(slope), _lib.stream())


# ---- fp16 inference mode (csrc/hifigan_f16_ops.hip): the same arguments; w: the packed fp16 images of vocoder.hifigan_pack_f16 ([taps, Cp / 8, Cout, 8]) ----
def _hifigan_f16_image(name, w, Cin, Cout, taps):
    if w.dtype != torch.float16 or tuple(w.shape) != (int(taps), (Cin + 31) // 32 * 4, Cout, 8) or not w.is_contiguous():
        raise _lib.GlowTTSHipError(f"{name} needs the packed fp16 weight image of vocoder.hifigan_pack_f16 for these sizes")


def hifigan_conv_f16(x, w, bias, out, frame_lengths, Lmax, mult, taps, dilation, slope=1.0, residual=None, accumulate=0, divisor=1.0, channels_first=False):
    """`hifigan_conv` with fp16 operands and fp32 sums (glowtts_hifigan_conv_f16)."""
    Cin = x.shape[1] if channels_first else x.shape[2]
    _hifigan_f16_image("glowtts_hifigan_conv_f16", w, Cin, out.shape[2], taps)
    _lib.api().glowtts_hifigan_conv_f16(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(residual), _lib.ptr(out), _lib.ptr(frame_lengths), x.shape[0], int(Lmax),
                                        int(mult), Cin, out.shape[2], int(taps), int(dilation), float(slope), int(accumulate), float(divisor),
                                        int(bool(channels_first)), _lib.stream())


def hifigan_upsample_f16(x, w, bias, out, frame_lengths, Lmax, mult, taps, rate, slope):
    """`hifigan_upsample` with fp16 operands and fp32 sums (glowtts_hifigan_upsample_f16)."""
    _hifigan_f16_image("glowtts_hifigan_upsample_f16", w, x.shape[2], out.shape[2], taps)
    _lib.api().glowtts_hifigan_upsample_f16(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(frame_lengths), x.shape[0], int(Lmax), int(mult),
                                            x.shape[2], out.shape[2], int(taps), int(rate), float(slope), _lib.stream())


# ---- training the HiFi-GAN generator (csrc/hifigan_train_ops.hip).  x: the forward's input before its LeakyReLU; wt: the transposed images of vocoder.py ----
def hifigan_conv_bwd(dy, wt, x, out, frame_lengths, Lmax, mult, taps, dilation, mask_slope, residual=None, scale=1.0, res_scale=1.0, accumulate=False):
    """dy [B, Lmax * mult, Cout] -> out [B, Lmax * mult, Cin]: the data gradient of `hifigan_conv` with the mask / residual / accumulate epilogue
    (glowtts_hifigan_conv_bwd)."""
    _lib.api().glowtts_hifigan_conv_bwd(_lib.ptr(dy), _lib.ptr(wt), _lib.ptr(x), _lib.ptr(residual), _lib.ptr(out), _lib.ptr(frame_lengths), dy.shape[0], int(Lmax),
                                        int(mult), out.shape[2], dy.shape[2], int(taps), int(dilation), float(mask_slope), float(scale), float(res_scale),
                                        int(bool(accumulate)), _lib.stream())


def hifigan_upsample_bwd(dy, wt, x, out, frame_lengths, Lmax, mult, taps, rate, mask_slope):
    """dy [B, Lmax * mult * rate, Cout] -> out [B, Lmax * mult, Cin]: the data gradient of `hifigan_upsample` (glowtts_hifigan_upsample_bwd)."""
    _lib.api().glowtts_hifigan_upsample_bwd(_lib.ptr(dy), _lib.ptr(wt), _lib.ptr(x), _lib.ptr(out), _lib.ptr(frame_lengths), dy.shape[0], int(Lmax), int(mult),
                                            out.shape[2], dy.shape[2], int(taps), int(rate), float(mask_slope), _lib.stream())


def hifigan_post_bwd(dwav, wav, x, w, dpre, dx, frame_lengths, Lmax, mult, taps, slope):
    """d wav [B, Lmax * mult] -> dpre [B, Lmax * mult] and dx [B, Lmax * mult, Cin], the gradient of the rows entering conv_post (glowtts_hifigan_post_bwd)."""
    _lib.api().glowtts_hifigan_post_bwd(_lib.ptr(dwav), _lib.ptr(wav), _lib.ptr(x), _lib.ptr(w), _lib.ptr(dpre), _lib.ptr(dx), _lib.ptr(frame_lengths), x.shape[0],
                                        int(Lmax), int(mult), x.shape[2], int(taps), float(slope), _lib.stream())


def hifigan_wgrad_work_floats(B, Lmax, mult, Cin, Cout, taps, rate=0):
    return int(_lib.api().glowtts_hifigan_wgrad_work_floats(int(B), int(Lmax), int(mult), int(Cin), int(Cout), int(taps), int(rate)))


def hifigan_wgrad(x, dy, frame_lengths, work, dw, dbias, Lmax, mult, taps, dilation=1, rate=0, slope=1.0, scale=1.0, channels_first=False):
    """dw (torch's layout: Conv1d [Cout, Cin, taps]; rate >= 1: ConvTranspose1d [Cin, Cout, taps]) and dbias [Cout] of one convolution from its input x before
    the LeakyReLU and dy; dy [B, Lmax * mult (* rate)] for conv_post (glowtts_hifigan_wgrad)."""
    Cin = x.shape[1] if channels_first else x.shape[2]
    _lib.api().glowtts_hifigan_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(frame_lengths), _lib.ptr(work), _lib.ptr(dw), _lib.ptr(dbias), x.shape[0], int(Lmax), int(mult),
                                     Cin, dbias.shape[0], int(taps), int(dilation), int(rate), float(slope), float(scale), int(bool(channels_first)), _lib.stream())


# ---- mixed-precision training of the HiFi-GAN generator (csrc/hifigan_mixed_ops.hip): the same arguments; wt: the packed bf16 images [T', Kp / 8, Cin, 8] ----
def _hifigan_bf16_image(name, wt, offsets, K, N):
    if wt.dtype != torch.bfloat16 or tuple(wt.shape) != (int(offsets), (K + 31) // 32 * 4, N, 8) or not wt.is_contiguous():
        raise _lib.GlowTTSHipError(f"{name} needs the packed bf16 data-gradient image of vocoder.hifigan_pack_bf16 for these sizes")


def hifigan_conv_bwd_bf16(dy, wt, x, out, frame_lengths, Lmax, mult, taps, dilation, mask_slope, residual=None, scale=1.0, res_scale=1.0, accumulate=False):
    """`hifigan_conv_bwd` with bf16 operands and fp32 sums (glowtts_hifigan_conv_bwd_bf16)."""
    _hifigan_bf16_image("glowtts_hifigan_conv_bwd_bf16", wt, taps, dy.shape[2], out.shape[2])
    _lib.api().glowtts_hifigan_conv_bwd_bf16(_lib.ptr(dy), _lib.ptr(wt), _lib.ptr(x), _lib.ptr(residual), _lib.ptr(out), _lib.ptr(frame_lengths), dy.shape[0],
                                             int(Lmax), int(mult), out.shape[2], dy.shape[2], int(taps), int(dilation), float(mask_slope), float(scale),
                                             float(res_scale), int(bool(accumulate)), _lib.stream())


def hifigan_upsample_bwd_bf16(dy, wt, x, out, frame_lengths, Lmax, mult, taps, rate, mask_slope):
    """`hifigan_upsample_bwd` with bf16 operands and fp32 sums (glowtts_hifigan_upsample_bwd_bf16)."""
    if wt.dim() != 4:
        raise _lib.GlowTTSHipError("glowtts_hifigan_upsample_bwd_bf16 needs the packed bf16 data-gradient image of vocoder.hifigan_pack_bf16")
    _hifigan_bf16_image("glowtts_hifigan_upsample_bwd_bf16", wt, wt.shape[0], int(rate) * dy.shape[2], out.shape[2])
    _lib.api().glowtts_hifigan_upsample_bwd_bf16(_lib.ptr(dy), _lib.ptr(wt), _lib.ptr(x), _lib.ptr(out), _lib.ptr(frame_lengths), dy.shape[0], int(Lmax), int(mult),
                                                 out.shape[2], dy.shape[2], int(taps), int(rate), float(mask_slope), _lib.stream())


def hifigan_wgrad_bf16(x, dy, frame_lengths, work, dw, dbias, Lmax, mult, taps, dilation=1, rate=0, slope=1.0, scale=1.0, channels_first=False):
    """`hifigan_wgrad` with lrelu(x) and dy rounded to bf16, fp32 sums; the bias gradient from the unrounded dy (glowtts_hifigan_wgrad_bf16).  A single output
    channel (conv_post) runs the f32 launches."""
    Cin = x.shape[1] if channels_first else x.shape[2]
    _lib.api().glowtts_hifigan_wgrad_bf16(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(frame_lengths), _lib.ptr(work), _lib.ptr(dw), _lib.ptr(dbias), x.shape[0], int(Lmax),
                                          int(mult), Cin, dbias.shape[0], int(taps), int(dilation), int(rate), float(slope), float(scale),
                                          int(bool(channels_first)), _lib.stream())


def hifigan_pack_images(jobs, total_blocks):
    """Every weight image of a mixed-precision step from the fp32 master weights in ONE launch; jobs: the int64 device table [njobs, 8] of
    vocoder.hifigan_pack_jobs (glowtts_hifigan_pack_images)."""
    if jobs.dtype != torch.int64 or jobs.dim() != 2 or jobs.shape[1] != 8 or not jobs.is_contiguous() or not jobs.is_cuda:
        raise _lib.GlowTTSHipError("glowtts_hifigan_pack_images needs the int64 device job table [njobs, 8] of vocoder.hifigan_pack_jobs")
    _lib.api().glowtts_hifigan_pack_images(_lib.ptr(jobs), jobs.shape[0], int(total_blocks), _lib.stream())


# ---- the bf16 mode of the HiFi-GAN multi-period discriminator (csrc/hifigan_disc_bf16_ops.hip): the middle convolutions (5 taps); activations are
# [B, H * period, C] float32, the images the packed bf16 images of vocoder.hifigan_disc_pack_bf16 ([5, pad32(K) / 8, N, 8]) ----
def _hifigan_disc_bf16_image(name, w, K, N):
    if w.dtype != torch.bfloat16 or tuple(w.shape) != (5, (K + 31) // 32 * 4, N, 8) or not w.is_contiguous() or not w.is_cuda:
        raise _lib.GlowTTSHipError(f"{name} needs the packed bf16 device image [5, {(K + 31) // 32 * 4}, {N}, 8] of vocoder.hifigan_disc_pack_bf16 for these sizes, "
                                   f"got {w.dtype} {list(w.shape)} on {w.device}")


def _hifigan_disc_f32(name, what, t, *shapes):
    """t: a contiguous float32 device tensor of one of `shapes` - the kernels take every size from the arguments, so a wrong buffer would be read or written
    out of bounds"""
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) not in shapes:
        raise _lib.GlowTTSHipError(f"{name}: {what} must be a contiguous float32 device tensor {' or '.join(str(list(s)) for s in shapes)}, got {t.dtype} "
                                   f"{list(t.shape)} on {t.device}")


def _hifigan_disc_rows(name, x, H, period, stride):
    """-> (B, Cin, rows of the layer's output per batch row) of an input x [B, H * period, Cin]"""
    H, period, stride = int(H), int(period), int(stride)
    if x.dim() != 3 or H < 1 or period < 1 or stride < 1:
        raise _lib.GlowTTSHipError(f"{name}: x must be [B, H * period, Cin] with H, period, stride >= 1, got {list(x.shape)}, H = {H}, period = {period}, stride = {stride}")
    _hifigan_disc_f32(name, "x", x, (x.shape[0], H * period, x.shape[2]))
    return x.shape[0], x.shape[2], ((H - 1) // stride + 1) * period


def hifigan_disc_conv_bf16(x, w, bias, out, H, period, stride, slope):
    """x [B, H * period, Cin] (pre-activations) -> out [B, H' * period, Cout] = bias + conv(bf16(lrelu(x, slope)), bf16 w), fp32 sums
    (glowtts_hifigan_disc_conv_bf16); w: the forward image.  H' = (H - 1) // stride + 1."""
    name = "glowtts_hifigan_disc_conv_bf16"
    B, Cin, rows = _hifigan_disc_rows(name, x, H, period, stride)
    if out.dim() != 3:
        raise _lib.GlowTTSHipError(f"{name}: out must be [B, H' * period, Cout], got {list(out.shape)}")
    Cout = out.shape[2]
    _hifigan_disc_f32(name, "out", out, (B, rows, Cout))
    _hifigan_disc_f32(name, "bias", bias, (Cout,))
    _hifigan_disc_bf16_image(name, w, Cin, Cout)
    _lib.api().glowtts_hifigan_disc_conv_bf16(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), B, int(H), int(period), int(stride), Cin, Cout, float(slope),
                                              _lib.stream())


def hifigan_disc_conv_bwd_bf16(dy, wt, x, dx, H, period, stride, slope, inj=None, inj_scale=None):
    """dy [B, H' * period, Cout] -> dx [B, H * period, Cin] = lrelu'(x) * (the transposed convolution of bf16(dy) with bf16 wt) + inj * inj_scale[0]
    (glowtts_hifigan_disc_conv_bwd_bf16); wt: the channel-transposed image, taps not reversed; inj: laid out as dx, inj_scale: a device scalar."""
    name = "glowtts_hifigan_disc_conv_bwd_bf16"
    B, Cin, rows = _hifigan_disc_rows(name, x, H, period, stride)
    if dy.dim() != 3:
        raise _lib.GlowTTSHipError(f"{name}: dy must be [B, H' * period, Cout], got {list(dy.shape)}")
    Cout = dy.shape[2]
    _hifigan_disc_f32(name, "dy", dy, (B, rows, Cout))
    _hifigan_disc_f32(name, "dx", dx, tuple(x.shape))
    if inj is not None:
        if inj_scale is None:
            raise _lib.GlowTTSHipError(f"{name}: inj needs the device scalar inj_scale")
        _hifigan_disc_f32(name, "inj", inj, tuple(x.shape))
        _hifigan_disc_f32(name, "inj_scale", inj_scale, (1,), ())
    _hifigan_disc_bf16_image(name, wt, Cout, Cin)
    _lib.api().glowtts_hifigan_disc_conv_bwd_bf16(_lib.ptr(dy), _lib.ptr(wt), _lib.ptr(x), _lib.ptr(inj), _lib.ptr(inj_scale) if inj is not None else None, _lib.ptr(dx),
                                                  B, int(H), int(period), int(stride), Cin, Cout, float(slope), _lib.stream())


def hifigan_disc_wgrad_bf16(x, dy, work, dw, dbias, H, period, stride, slope):
    """dw [Cout, Cin, 5(, 1)] and dbias [Cout] of one middle convolution from its input x [B, H * period, Cin] before the LeakyReLU and dy
    [B, H' * period, Cout], both rounded to bf16; the bias gradient from the unrounded dy (glowtts_hifigan_disc_wgrad_bf16).  work: at least
    glowtts_hifigan_disc_work_floats(B, H' * period, Cin, Cout, 5) floats."""
    name = "glowtts_hifigan_disc_wgrad_bf16"
    B, Cin, rows = _hifigan_disc_rows(name, x, H, period, stride)
    if dy.dim() != 3:
        raise _lib.GlowTTSHipError(f"{name}: dy must be [B, H' * period, Cout], got {list(dy.shape)}")
    Cout = dy.shape[2]
    _hifigan_disc_f32(name, "dy", dy, (B, rows, Cout))
    _hifigan_disc_f32(name, "dw", dw, (Cout, Cin, 5), (Cout, Cin, 5, 1))
    _hifigan_disc_f32(name, "dbias", dbias, (Cout,))
    need = int(_lib.api().glowtts_hifigan_disc_work_floats(B, rows, Cin, Cout, 5))
    if need < 1 or work.dim() != 1 or work.numel() < need:
        raise _lib.GlowTTSHipError(f"{name}: work must hold glowtts_hifigan_disc_work_floats(B, rows, Cin, Cout, 5) = {need} floats (0: sizes out of range), got "
                                   f"{list(work.shape)}")
    _hifigan_disc_f32(name, "work", work, tuple(work.shape))
    _lib.api().glowtts_hifigan_disc_wgrad_bf16(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(work), _lib.ptr(dw), _lib.ptr(dbias), B, int(H), int(period), int(stride), Cin, Cout,
                                               5, 0, float(slope), _lib.stream())
