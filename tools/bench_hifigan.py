"""HiFi-GAN vocoder (glow_tts_amd/vocoder.py: HiFiGAN, csrc/hifigan_ops.hip) on one MI355X: B = 1 x 800 and B = 32 x 800 frames at the V1 sizes
(512 initial channels, rates 8 8 2 2, kernels 16 16 4 4, resblock '1' with kernel sizes 3 7 11 and dilations 1 3 5, 80 mel bins, hop 256).  Per size:
  * ms per call of the HIP path (conv_pre, per stage the transposed convolution and 18 resblock convolutions, conv_post: 78 launches, counted from the
    launch log) and multiples of real time at 24 kHz;
  * the BASELINE: the same generator written HERE with torch.nn.functional.conv1d / conv_transpose1d (vendor-library convolutions, f32) on the same
    device and weights; the two are called ALTERNATELY, so that a drifting clock meets both; HIP-over-baseline ratio (printed as it is, whichever side
    wins) and the two waveforms' largest difference;
  * the arithmetic of a call computed from the shapes (`macs_per_frame`: 307 M MAC per mel frame at V1), the achieved TFLOP/s of the whole call, its
    share of the 155 TF/s this project uses for the exact-f32 MFMA, and the floor that figure sets.  The share is a whole-call rate over the peak (launch
    gaps and epilogues included), not a kernel's.
Weights: `hifigan_init` under a fixed seed; mels uniform in [-4, 4].  Medians of `--iters` (>= 20) timed calls per side after `--warmup`, each a host clock
around a call that ends in a device synchronise; the sustained clock is noted as tools/bench_vc.py does.
Usage: python tools/bench_hifigan.py [--iters 20] [--out profiles/bench_hifigan.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402

SR, FRAMES, PEAK_TFLOPS = 24000, 800, 155.0


def macs_per_frame(geo):
    """Multiply-accumulates per mel frame, from the shapes: conv_pre, per stage the transposed convolution (every input row meets every tap once) and the
    resblock convolutions at the stage's row rate, conv_post."""
    from glow_tts_amd.vocoder import HIFIGAN_POST_TAPS, HIFIGAN_PRE_TAPS
    macs, cin, rows = geo["A"] * geo["C0"] * HIFIGAN_PRE_TAPS, geo["C0"], 1
    per_dilation = 2 if geo["resblock"] == "1" else 1
    for u, k, c in zip(geo["rates"], geo["kernels"], geo["channels"]):
        macs += rows * cin * c * k
        rows *= u
        macs += rows * c * c * sum(rk * per_dilation * len(ds) for rk, ds in zip(geo["rk"], geo["rd"]))
        cin = c
    return macs + rows * cin * HIFIGAN_POST_TAPS


def torch_generator(w, geo, mels):
    """The baseline: mels [B, A, L] -> wav [B, L * hop] on torch's convolutions (all utterances of full length)."""
    x = F.conv1d(mels, w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
    nk = geo["nk"]
    for i, (u, k) in enumerate(zip(geo["rates"], geo["kernels"])):
        x = F.conv_transpose1d(F.leaky_relu(x, 0.1), w[f"ups.{i}.weight"], w[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        xs = None
        for j, (rk, ds) in enumerate(zip(geo["rk"], geo["rd"])):
            q, r = f"resblocks.{i * nk + j}.", x
            for m, d in enumerate(ds):
                t = F.conv1d(F.leaky_relu(r, 0.1), w[q + f"convs1.{m}.weight"], w[q + f"convs1.{m}.bias"], padding=(rk - 1) // 2 * d, dilation=d)
                if geo["resblock"] == "1":
                    t = F.conv1d(F.leaky_relu(t, 0.1), w[q + f"convs2.{m}.weight"], w[q + f"convs2.{m}.bias"], padding=(rk - 1) // 2)
                r = t + r
            xs = r if xs is None else xs.add_(r)
        x = xs / nk
    return torch.tanh(F.conv1d(F.leaky_relu(x, 0.01), w["conv_post.weight"], w["conv_post.bias"], padding=3))[:, 0]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run(B, vocoder, w_dev, warmup, iters):
    from glow_tts_amd import _lib
    geo, dev = vocoder.geo, vocoder.device
    L, T = FRAMES, FRAMES * geo["hop"]
    g = torch.Generator().manual_seed(5)
    mels = (torch.rand(B, geo["A"], L, generator=g) * 8.0 - 4.0).to(dev)
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    hip = lambda: vocoder(mels, lengths)[0]
    with torch.no_grad():
        base = lambda: torch_generator(w_dev, geo, mels)
        _lib.lib().glowtts_launch_log_reset()
        y_hip = hip()
        launches = int(_lib.lib().glowtts_launch_count(b"hifigan_"))        # (the count of every class with this prefix)
        y_base = base()
        diff = float((y_hip - y_base).abs().max() / y_base.abs().max())
        del y_hip, y_base
        for _ in range(warmup):
            hip(), base()
        torch.cuda.synchronize()
        th, tb = [], []
        for _ in range(iters):                                           # alternating: a drifting clock meets both sides
            th.append(timed(hip))
            tb.append(timed(base))
    hip_ms, base_ms = statistics.median(th), statistics.median(tb)
    flop = 2.0 * macs_per_frame(geo) * B * L
    audio = B * T / SR
    side = lambda ms, ts: {"ms_per_call": round(ms, 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "times_real_time": round(audio / (ms * 1e-3), 1),
                           "call_tflops": round(flop / (ms * 1e-3) / 1e12, 2), "call_fraction_of_f32_mfma_peak": round(flop / (ms * 1e-3) / 1e12 / PEAK_TFLOPS, 3)}
    return {"B": B, "frames": L, "audio_seconds": round(audio, 3), "call_tflop": round(flop / 1e12, 3), "floor_ms_at_f32_mfma_peak": round(flop / (PEAK_TFLOPS * 1e12) * 1e3, 2),
            "waveform_max_diff_hip_vs_baseline_rel": diff, "hip": dict(side(hip_ms, th), launches_per_call=launches), "baseline_torch_conv": side(base_ms, tb),
            "speedup_hip_over_baseline": round(base_ms / hip_ms, 2), "hip_faster": bool(hip_ms < base_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_hifigan.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_hifigan.py measures on the GPU"
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.vocoder import HIFIGAN_DEFAULTS, HiFiGAN, hifigan_geometry, hifigan_init
    d = load_yaml(DEFAULT_YAML)
    d["Vocoder"] = dict(HIFIGAN_DEFAULTS)
    hp = Recursive_Parse(d)
    sd = hifigan_init(hifigan_geometry(hp), 1234)
    vocoder = HiFiGAN(hp, "cuda:0", state_dict=sd)
    w_dev = {k: v.to(vocoder.device) for k, v in sd.items()}
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup,
           "geometry": {k: vocoder.geo[k] for k in ("A", "hop", "C0", "rates", "kernels", "channels", "resblock", "rk", "rd")}, "sample_rate": SR,
           "mmac_per_frame": round(macs_per_frame(vocoder.geo) / 1e6, 1), "f32_mfma_peak_tflops": PEAK_TFLOPS,
           "results": [run(B, vocoder, w_dev, args.warmup, args.iters) for B in (1, 32)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
