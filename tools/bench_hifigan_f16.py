"""The HiFi-GAN vocoder's fp16 inference mode against its f32 mode on one MI355X (glow_tts_amd/vocoder.py: HiFiGAN with precision 'f32' / 'f16';
csrc/hifigan_ops.hip and csrc/hifigan_f16_ops.hip): ONE generator at the V1 sizes (512 initial channels, rates 8 8 2 2, kernels 16 16 4 4, resblock '1'
with kernel sizes 3 7 11 and dilations 1 3 5, 80 mel bins, hop 256), `hifigan_init` weights, B = 1 x 800 and B = 32 x 800 frames, the same mels for both.
The f32 path is the code of before this mode, untouched, which is why it serves as the baseline of the same run.  Per size:
  * ms per call of each precision: the median of `--iters` (>= 20) timed calls taken ALTERNATELY (f32, f16, a second f32 generator, ...), so that a drifting
    clock meets all; each a host clock around a call that ends in a device synchronise, after `--warmup` calls of each;
  * the A/A spread: the two f32 generators' medians against each other - a speedup counts only where it is clearly more than this;
  * the f16 launches alone (conv_pre and the stages, issued back to back on the call's own buffers; counted in the launch log) and their share of the call;
    what remains is conv_post + tanh (f32) and the waveform's allocation;
  * the f16 launches' distance from their HBM floor: every launch reads its input rows once (and the residual and, where it accumulates, the sum so far) and
    writes its output rows, all fp32 - `hbm_floats_per_frame`, from the shapes - over the 8 TB/s of the MI355X's HBM; the weights and the halo rows are not
    counted;
  * the largest difference of the two waveforms relative to the f32 one's largest value (what the rounding costs on these weights).
Usage: python tools/bench_hifigan_f16.py [--iters 20] [--out profiles/bench_hifigan_f16.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_hifigan import macs_per_frame  # noqa: E402

SR, FRAMES, PEAK_F16_TFLOPS, PEAK_F32_TFLOPS, HBM_TBS = 24000, 800, 2500.0, 155.0, 8.0
F16_CLASSES = ("hifigan_conv_f16", "hifigan_upsample_f16")


def hbm_floats_per_frame(geo):
    """fp32 values that the launches before conv_post read and write per mel frame, from the plan of `HiFiGAN._stage`"""
    n, cin, rows = geo["A"] + geo["C0"], geo["C0"], 1
    for u, c in zip(geo["rates"], geo["channels"]):
        n += rows * cin + rows * u * c                                       # the transposed convolution
        rows *= u
        for j, ds in enumerate(geo["rd"]):
            for m in range(len(ds)):
                last = m == len(ds) - 1
                if geo["resblock"] == "1":
                    n += rows * c * 2                                        # convs1: in, out
                n += rows * c * (3 + (1 if last and j > 0 else 0))           # the step's last convolution: in, residual, out (+ the MRF sum so far)
        cin = c
    return n


def alternating_ms(fns, warmup, iters):
    """{name: (median, min, max) ms} of `iters` timed calls of every function of `fns`, taken in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def launches_before_post(v, mels, lengths):
    """`HiFiGAN.__call__` without conv_post: conv_pre and the stages on the call's own buffers"""
    from glow_tts_amd.vocoder import HIFIGAN_PRE_TAPS
    g = v.geo
    B, _, L = mels.shape
    p0, p1, U, X, T = v._work(B, L)
    view = lambda buf, rows, c: buf[:B * rows * c].view(B, rows, c)
    x, mult = view(p0, L, g["C0"]), 1
    v._conv_op(mels, *v.pre, x, lengths, L, 1, HIFIGAN_PRE_TAPS, 1, channels_first=True)
    for i, (u, c) in enumerate(zip(g["rates"], g["channels"])):
        rows = L * mult * u
        acc = view(p1 if i % 2 == 0 else p0, rows, c)
        v._stage(i, x, lengths, L, mult, view(U, rows, c), view(X, rows, c), view(T, rows, c), acc)
        x, mult = acc, mult * u


def run(B, vocoders, warmup, iters):
    from glow_tts_amd import _lib
    geo, dev = vocoders["f32"].geo, vocoders["f32"].device
    L, T = FRAMES, FRAMES * geo["hop"]
    g = torch.Generator().manual_seed(5)
    mels = (torch.rand(B, geo["A"], L, generator=g) * 8.0 - 4.0).to(dev)
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    wav = {p: v(mels, lengths)[0] for p, v in vocoders.items()}
    assert torch.equal(wav["f32"], wav["f32_again"])
    diff = float((wav["f16"] - wav["f32"]).abs().max() / wav["f32"].abs().max())
    del wav
    _lib.lib().glowtts_launch_log_reset()
    vocoders["f16"](mels, lengths)
    n_f16 = sum(int(_lib.lib().glowtts_launch_count(c.encode())) for c in F16_CLASSES)
    n_all = int(_lib.lib().glowtts_launch_count(b"hifigan_"))
    call = alternating_ms({p: (lambda v=v: v(mels, lengths)) for p, v in vocoders.items()}, warmup, iters)
    part = alternating_ms({p: (lambda v=v: launches_before_post(v, mels, lengths)) for p, v in vocoders.items()}, warmup, iters)
    flop = 2.0 * macs_per_frame(geo) * B * L
    hbm_bytes = 4.0 * hbm_floats_per_frame(geo) * B * L
    floor_hbm_ms = hbm_bytes / (HBM_TBS * 1e12) * 1e3
    audio = B * T / SR
    out = {"B": B, "frames": L, "audio_seconds": round(audio, 3), "waveform_max_diff_f16_vs_f32_rel": diff, "call_tflop": round(flop / 1e12, 3),
           "launches_per_call": n_all, "f16_launches_per_call": n_f16, "hbm_gbytes_before_conv_post": round(hbm_bytes / 1e9, 3),
           "hbm_floor_ms": round(floor_hbm_ms, 3), "f16_mfma_floor_ms": round(flop / (PEAK_F16_TFLOPS * 1e12) * 1e3, 3),
           "f32_mfma_floor_ms": round(flop / (PEAK_F32_TFLOPS * 1e12) * 1e3, 3)}
    for p in vocoders:
        out[p] = {"ms_per_call": round(call[p][0], 3), "ms_min_max": [round(call[p][1], 3), round(call[p][2], 3)],
                  "times_real_time": round(audio / (call[p][0] * 1e-3), 1), "launches_before_conv_post_ms": round(part[p][0], 3),
                  "launches_before_conv_post_ms_min_max": [round(part[p][1], 3), round(part[p][2], 3)],
                  "share_of_call_before_conv_post": round(part[p][0] / call[p][0], 3), "call_tflops": round(flop / (call[p][0] * 1e-3) / 1e12, 2),
                  "hbm_tbytes_per_s_before_conv_post": round(hbm_bytes / (part[p][0] * 1e-3) / 1e12, 3),
                  "hbm_floor_over_ms_before_conv_post": round(floor_hbm_ms / part[p][0], 3)}
    aa = abs(call["f32"][0] - call["f32_again"][0]) / min(call["f32"][0], call["f32_again"][0])
    out["f32_aa_spread"] = round(aa, 4)
    out["speedup_f16_over_f32_call"] = round(call["f32"][0] / call["f16"][0], 2)
    out["speedup_f16_over_f32_before_conv_post"] = round(part["f32"][0] / part["f16"][0], 2)
    out["f16_faster_by_more_than_the_aa_spread"] = bool(call["f32"][0] / call["f16"][0] > 1.0 + 3.0 * aa)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_hifigan_f16.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_hifigan_f16.py measures on the GPU"
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.vocoder import HIFIGAN_DEFAULTS, HiFiGAN, hifigan_geometry, hifigan_init
    d = load_yaml(DEFAULT_YAML)
    d["Vocoder"] = dict(HIFIGAN_DEFAULTS)
    hp = Recursive_Parse(d)
    sd = hifigan_init(hifigan_geometry(hp), 1234)
    vocoders = {"f32": HiFiGAN(hp, "cuda:0", state_dict=sd, precision="f32"), "f16": HiFiGAN(hp, "cuda:0", state_dict=sd, precision="f16"),
                "f32_again": HiFiGAN(hp, "cuda:0", state_dict=sd)}
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup,
           "geometry": {k: vocoders["f32"].geo[k] for k in ("A", "hop", "C0", "rates", "kernels", "channels", "resblock", "rk", "rd")}, "sample_rate": SR,
           "mmac_per_frame": round(macs_per_frame(vocoders["f32"].geo) / 1e6, 1), "hbm_kbytes_per_frame": round(4 * hbm_floats_per_frame(vocoders["f32"].geo) / 1e3, 1),
           "f16_mfma_peak_tflops": PEAK_F16_TFLOPS, "f32_mfma_peak_tflops": PEAK_F32_TFLOPS, "hbm_peak_tbytes_per_s": HBM_TBS,
           "results": [run(B, vocoders, args.warmup, args.iters) for B in (1, 32)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
