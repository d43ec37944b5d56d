"""The cases and the bars of the HiFi-GAN generator's fp16 inference mode, shared by tests/test_hifigan_f16_cpu.py and tests/test_gpu_hifigan_f16.py.
The contract and its three realisations (emu64, emu32, emu32b): tests/hifigan_f16_ref.py.

OPERATORS.  The kernel rounds exactly given float32 inputs, so there are no rounding flips between it and emu64: the bar is the project's f32 bar,
max |got - emu64| / max |emu64| <= 4 e32' + 1e-6, with e32' the error of emu32 against emu64 on the same case; guard 0 < e32' < 1e-3.

WHOLE GENERATOR.  No closed bound exists for a chain of this depth, and a rounding that flips early moves everything after it, so the bars are multiples of
e_f16 = max |emu64 - ref64| (ref64: hifigan_ref in float64, the unrounded generator), measured on reference arithmetic and never on the kernel:
  (a) max |got - ref64| <= BAR_A e_f16, BAR_A = 1.5 x the largest of |emu32 - ref64| / e_f16 and |emu32b - ref64| / e_f16 over the cases, waveform and rows;
  (b) on NARROW and ODD, max |got - emu64| <= BAR_B e_f16, BAR_B = 2 x the largest of |emu32 - emu64| / e_f16 and |emu32b - emu64| / e_f16 over those cases.
The margins 1.5 and 2: a third realisation of the same rounding noise may land that far from two others (the margins of the Parallel WaveGAN bf16 bars).
(b) is not asserted on DEFAULT: a flip early in 78 layers of 512 channels moves the result as far as the rounding noise itself (0.61 .. 1.00 below).
Guard in every case: e_f16 > 100 e32 > 0 (e32 = max |ref32 - ref64|) and max |ref64| > 1e-3.
Figure (b) is decided by whether any early rounding flips at all, so one weight seed samples it poorly: NARROW and ODD run under two weight seeds.

MEASURED on the CPU (float64 / float32 torch; per case the larger of waveform and rows; lengths 3, 5, 2, 7):
  quantity                               seed 1234                     seed 4321
  e_f16 / max |ref64|                    2.0e-4 .. 8.4e-4              2.3e-4 .. 6.1e-4       (DEFAULT, seed 1234: 2.4e-4 .. 3.8e-4)
  e_f16 / e32                            768 .. 3841                   385 .. 4497            (DEFAULT: 554 .. 1168)
  |emu32 - ref64| / e_f16                0.982 .. 1.018                0.943 .. 1.044         (DEFAULT: 0.956 .. 1.105)
  |emu32b - ref64| / e_f16               0.955 .. 1.015                0.943 .. 1.033         (DEFAULT: 0.865 .. 1.007)
  |emu32 - emu64| / e_f16, NARROW, ODD   <= 0.147                      <= 0.453               (DEFAULT: 0.613 .. 0.951, not asserted)
  |emu32b - emu64| / e_f16, NARROW, ODD  <= 0.100                      <= 0.453               (DEFAULT: 0.685 .. 0.996, not asserted)
so A_MAX = 1.105 and B_MAX = 0.453."""
import torch

import hifigan_f16_ref as R
import hifigan_ref as H

CFGS = {"default": H.DEFAULT, "narrow": H.NARROW, "odd": H.ODD}
RAGGED = [5, 2, 7]
# (config, weight seed, the batches' lengths)
GENERATOR_CASES = [("narrow", 1234, [3]), ("narrow", 1234, RAGGED), ("narrow", 4321, [3]), ("narrow", 4321, RAGGED),
                   ("odd", 1234, [3]), ("odd", 1234, RAGGED), ("odd", 4321, [3]), ("odd", 4321, RAGGED),
                   ("default", 1234, [3]), ("default", 1234, [2])]
A_MAX, B_MAX = 1.105, 0.453                                                  # the measured figures above
BAR_A, BAR_B = 1.5 * A_MAX, 2.0 * B_MAX

# Whether v_mfma_f32_16x16x32_f16 treats fp16 subnormal operands as zero.  Decided on an MI355X by the operator case `subnormal_rows` below (rows scaled into
# [1e-7, 6e-5], all below the smallest normal fp16 6.1e-5): it meets the bar against the contract that KEEPS them (ratio printed by the test) and misses it by
# orders of magnitude against the one that flushes.
FLUSH_SUBNORMALS = False

# ---- operator cases: the smallest shapes that reach every path ----
CONV_CHANNELS = [(16, 16, False), (32, 16, False), (8, 64, False), (80, 512, True), (256, 256, False)]       # (Cin, Cout, channels-first)
CONV_TAPS = [(3, 1), (3, 5), (7, 3), (11, 5)]                                # (taps, dilation)
CONV_ROWS = [1, 5, 63, 64, 65, 200]                                          # 1, 5: shorter than the reach; 63 / 64 / 65: around the 64-row tile
EPILOGUES = [("plain", False, 0), ("residual", True, 0), ("accumulate 1", True, 1), ("accumulate 2 / 3", True, 2)]    # (tag, residual, accumulate); divisor 3
UP_KERNELS = [(8, 16), (2, 4), (3, 7), (5, 11)]                              # (rate, taps): (3, 7), (5, 11) have phases of unequal tap counts
UP_CHANNELS = [(64, 32), (16, 16)]
UP_ROWS = [1, 2, 9, 33, 65]

_SD, _REF = {}, {}


def sd_of(name, seed):
    if (name, seed) not in _SD:
        _SD[(name, seed)] = H.random_state_dict(CFGS[name], seed)
    return _SD[(name, seed)]


def mel_of(name, L):
    return H.uniform_mel(CFGS[name]["A"], L, 10 + L)


def reference(name, seed, L):
    """dict(mel, ref64, ref32, emu64, emu32, emu32b), each a (waveform, rows entering conv_post) pair, of the utterance of L frames: computed once, shared,
    never changed"""
    key = (name, seed, L)
    if key not in _REF:
        cfg, sd, mel = CFGS[name], sd_of(name, seed), mel_of(name, L)
        e64, e32, e32b = R.emus(FLUSH_SUBNORMALS)
        _REF[key] = {"mel": mel, "ref64": H.generator(sd, cfg, mel), "ref32": H.generator(sd, cfg, mel, torch.float32), "emu64": e64.generator(sd, cfg, mel),
                     "emu32": e32.generator(sd, cfg, mel), "emu32b": e32b.generator(sd, cfg, mel)}
    return _REF[key]


def dist(a, b):
    return float((a.double() - b.double()).abs().max())


def figures(ref, i):
    """(scale, e_f16, e32) of tensor i (0 waveform, 1 rows) of a `reference` entry, with the guard"""
    scale, e_f16, e32 = float(ref["ref64"][i].abs().max()), dist(ref["emu64"][i], ref["ref64"][i]), dist(ref["ref32"][i], ref["ref64"][i])
    assert e_f16 > 100 * e32 > 0 and scale > 1e-3, ("degenerate case", scale, e_f16, e32)
    return scale, e_f16, e32


def check_generator(tag, got, ref, i, narrow_or_odd):
    """Bars (a) and (b) for tensor i of the realisation `got`; prints the observed ratios first"""
    _, e_f16, _ = figures(ref, i)
    a, b = dist(got, ref["ref64"][i]) / e_f16, dist(got, ref["emu64"][i]) / e_f16
    print(f"{tag}: |got - ref64| / e_f16 {a:.3f} (bar {BAR_A:.3f})  |got - emu64| / e_f16 {b:.3f} (bar {BAR_B:.3f}{'' if narrow_or_odd else ', not asserted'})")
    assert a <= BAR_A, tag
    assert not narrow_or_odd or b <= BAR_B, tag
    return a, b


def check_operator(tag, got, emu64, emu32):
    """The operator bar; prints the observed ratio first"""
    scale = float(emu64.abs().max())
    err, e32 = dist(got, emu64) / scale, dist(emu32, emu64) / scale
    print(f"{tag}: err {err:.3e}  e32' {e32:.3e}  ratio {err / e32:.2f}  max|emu64| {scale:.3e}")
    assert 0 < e32 < 1e-3, "degenerate case"
    assert err <= 4 * e32 + 1e-6, tag
    return err / e32
