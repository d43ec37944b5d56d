"""Neural vocoder (glow_tts_amd/vocoder.py: ParallelWaveGAN, csrc/pwg_ops.hip) on one MI355X: B = 32 x 800 and B = 1 x 800 frames at the default sizes
(30 layers, 3 stacks, 64 / 128 / 64 channels, 80 mel bins, hop 256).  Per size:
  * ms per call of the HIP path (conditioning, seeded noise + first_conv, 30 layer launches, head) and multiples of real time at 24 kHz;
  * the BASELINE: the same generator written HERE with torch.nn.functional convs (vendor-library convolutions, f32) on the same device, weights and
    noise, A/B interleaved so that a drifting clock meets both; HIP-over-baseline speed-up and the two waveforms' largest difference;
  * the 30 layer launches alone (issued back to back on the call's own buffers): achieved TFLOP/s against the 155 TF/s the exact-f32 MFMA sustains and
    the floor that figure sets (2 (K G + R (R + S)) FLOP per sample and layer, K = 3 R + A).
Weights: uniform in +- 1 / sqrt(fan_in) under a fixed seed; mels uniform in [-4, 4].  Median of `--iters` (>= 20) timed calls after `--warmup`, each a host
clock around a call that ends in a device synchronise; the sustained clock is noted as tools/bench_vc.py does.
Usage: python tools/bench_pwg.py [--iters 20] [--out profiles/bench_pwg.json]"""
import argparse
import json
import math
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


def random_weights(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in shapes.items():
        fan_in = math.prod(shapes[k[:-len("bias")] + "weight"][1:]) if k.endswith("bias") else math.prod(shape[1:])
        sd[k] = (torch.rand(shape, generator=g) * 2.0 - 1.0) / math.sqrt(fan_in)
    return sd


def torch_generator(w, geo, mels, z):
    """The baseline: mels [B, A, L], z [B, L * hop] -> wav [B, L * hop] on torch's convolutions (all utterances of full length)."""
    c = F.conv1d(F.pad(mels, (geo["ctx"], geo["ctx"]), mode="replicate"), w["upsample_net.conv_in.weight"])
    for i, s in enumerate(geo["scales"]):
        c = F.conv2d(c.repeat_interleave(s, dim=2)[:, None], w[f"upsample_net.upsample.up_layers.{2 * i + 1}.weight"], padding=(0, s))[:, 0]
    x = F.conv1d(z[:, None], w["first_conv.weight"], w["first_conv.bias"])
    skips = None
    for i, d in enumerate(geo["dilations"]):
        q = f"conv_layers.{i}."
        h = F.conv1d(x, w[q + "conv.weight"], w[q + "conv.bias"], padding=d, dilation=d) + F.conv1d(c, w[q + "conv1x1_aux.weight"])
        g = torch.tanh(h[:, :geo["R"]]) * torch.sigmoid(h[:, geo["R"]:])
        del h
        s = F.conv1d(g, w[q + "conv1x1_skip.weight"], w[q + "conv1x1_skip.bias"])
        skips = s if skips is None else skips.add_(s)
        x = (F.conv1d(g, w[q + "conv1x1_out.weight"], w[q + "conv1x1_out.bias"]) + x) * math.sqrt(0.5)
    y = torch.relu(skips * math.sqrt(1.0 / geo["layers"]))
    y = torch.relu(F.conv1d(y, w["last_conv_layers.1.weight"], w["last_conv_layers.1.bias"]))
    return F.conv1d(y, w["last_conv_layers.3.weight"], w["last_conv_layers.3.bias"])[:, 0]


def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def run(B, vocoder, w_dev, warmup, iters):
    from glow_tts_amd import ops
    geo, dev = vocoder.geo, vocoder.device
    L, T = FRAMES, FRAMES * vocoder.geo["hop"]
    g = torch.Generator().manual_seed(5)
    mels = (torch.rand(B, geo["A"], L, generator=g) * 8.0 - 4.0).to(dev)
    z = torch.randn(B, T, generator=g).to(dev)
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    hip = lambda: vocoder(mels, lengths, noises=z)[0]
    with torch.no_grad():
        base = lambda: torch_generator(w_dev, geo, mels, z)
        y_hip, y_base = hip(), base()
        diff = float((y_hip - y_base).abs().max() / y_base.abs().max())
        del y_hip, y_base
        h1 = median_ms(hip, warmup, iters // 2)
        b1 = median_ms(base, warmup, iters // 2)
        h2 = median_ms(hip, 1, iters - iters // 2)
        b2 = median_ms(base, 1, iters - iters // 2)
    hip_ms, base_ms = (h1[0] + h2[0]) / 2, (b1[0] + b2[0]) / 2
    wk = vocoder._work(B, L)

    def layers():
        x, xn = wk["x"]
        for i, (lw, d) in enumerate(zip(vocoder.layer_weights, geo["dilations"])):
            ops.pwg_layer(x, wk["c"], *lw, xn, wk["skips"], lengths, L, geo["hop"], d, i > 0)
            x, xn = xn, x
    lay_ms = median_ms(layers, 2, iters)[0]
    flop = 2.0 * ((3 * geo["R"] + geo["A"]) * geo["G"] + geo["R"] * (geo["R"] + geo["S"])) * geo["layers"] * B * T
    audio = B * T / SR
    return {"B": B, "frames": L, "audio_seconds": round(audio, 3), "waveform_max_diff_hip_vs_baseline_rel": diff,
            "hip": {"ms_per_call": round(hip_ms, 3), "ms_min_max": [round(min(h1[1], h2[1]), 3), round(max(h1[2], h2[2]), 3)],
                    "ms_per_call_halves": [round(h1[0], 3), round(h2[0], 3)], "times_real_time": round(audio / (hip_ms * 1e-3), 1),
                    "layers_ms": round(lay_ms, 3), "layers_tflop": round(flop / 1e12, 3), "layers_tflops": round(flop / (lay_ms * 1e-3) / 1e12, 2),
                    "layers_fraction_of_f32_mfma_peak": round(flop / (lay_ms * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
                    "layers_floor_ms_at_peak": round(flop / (PEAK_TFLOPS * 1e12) * 1e3, 2)},
            "baseline_torch_conv": {"ms_per_call": round(base_ms, 3), "ms_min_max": [round(min(b1[1], b2[1]), 3), round(max(b1[2], b2[2]), 3)],
                                    "ms_per_call_halves": [round(b1[0], 3), round(b2[0], 3)], "times_real_time": round(audio / (base_ms * 1e-3), 1)},
            "speedup_hip_over_baseline": round(base_ms / hip_ms, 2), "hip_faster": bool(hip_ms < base_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_pwg.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_pwg.py measures on the GPU"
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.vocoder import PWG_DEFAULTS, ParallelWaveGAN, pwg_expected_shapes, pwg_geometry
    d = load_yaml(DEFAULT_YAML)
    d["Vocoder"] = dict(PWG_DEFAULTS)
    hp = Recursive_Parse(d)
    sd = random_weights(pwg_expected_shapes(pwg_geometry(hp)), 1234)
    vocoder = ParallelWaveGAN(hp, "cuda:0", state_dict=sd)
    w_dev = {k: v.to(vocoder.device) for k, v in sd.items()}
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup,
           "geometry": {k: vocoder.geo[k] for k in ("layers", "stacks", "R", "G", "S", "A", "ctx", "scales", "hop")}, "sample_rate": SR,
           "f32_mfma_peak_tflops": PEAK_TFLOPS, "results": [run(B, vocoder, w_dev, args.warmup, args.iters) for B in (32, 1)]}
    out["hip_faster_at_both_sizes"] = all(r["hip_faster"] for r in out["results"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
