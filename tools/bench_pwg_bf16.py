"""The neural vocoder's bf16 inference mode against its f32 mode on one MI355X (glow_tts_amd/vocoder.py: ParallelWaveGAN with precision 'f32' / 'bf16';
csrc/pwg_ops.hip and csrc/pwg_bf16_ops.hip): ONE generator at the default sizes (30 layers, 3 stacks, 64 / 128 / 64 channels, 80 mel bins, hop 256), random
weights, B = 1 x 800 and B = 32 x 800 frames, the same mels and noise for both.  The f32 path is the code of before this mode, untouched, which is why it
serves as the baseline of the same run.  Per size:
  * ms per call of each precision: the median of `--iters` (>= 20) timed calls taken ALTERNATELY (f32, bf16, f32, ...), so that a drifting clock meets
    both; each a host clock around a call that ends in a device synchronise, after `--warmup` calls of each, as tools/bench_pwg.py does;
  * the 30 layer launches alone (issued back to back on the call's own buffers), alternating likewise, and their share of the call;
  * the bf16 layers' distance from their HBM floor: a layer reads x and c once and the skips, and writes x' and the skips - 4 (2 R + A + 2 S) bytes per
    sample, 1344 at the default sizes - over the 8 TB/s of the MI355X's HBM; and the f32 layers' compute floor at the 155 TF/s exact-f32 MFMA peak;
  * the largest difference of the two waveforms relative to the f32 one's largest value (what the rounding costs on random weights).
Usage: python tools/bench_pwg_bf16.py [--iters 20] [--out profiles/bench_pwg_bf16.json]"""
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
from bench_pwg import random_weights  # noqa: E402

SR, FRAMES, PEAK_F32_TFLOPS, HBM_TBS = 24000, 800, 155.0, 8.0


def alternating_ms(fns, warmup, iters):
    """{name: median ms} of `iters` timed calls of every function of `fns`, taken in turn"""
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


def run(B, vocoders, warmup, iters):
    geo, dev = vocoders["f32"].geo, vocoders["f32"].device
    L, T = FRAMES, FRAMES * geo["hop"]
    g = torch.Generator().manual_seed(5)
    mels = (torch.rand(B, geo["A"], L, generator=g) * 8.0 - 4.0).to(dev)
    z = torch.randn(B, T, generator=g).to(dev)
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    wav = {p: v(mels, lengths, noises=z)[0] for p, v in vocoders.items()}
    diff = float((wav["bf16"] - wav["f32"]).abs().max() / wav["f32"].abs().max())
    del wav
    call = alternating_ms({p: (lambda v=v: v(mels, lengths, noises=z)) for p, v in vocoders.items()}, warmup, iters)

    def layers(v):
        wk = v._work(B, L)
        x, xn = wk["x"]
        for i, (lw, d) in enumerate(zip(v.layer_weights, geo["dilations"])):
            v._layer_op(x, wk["c"], *lw, xn, wk["skips"], lengths, L, geo["hop"], d, i > 0)
            x, xn = xn, x
    lay = alternating_ms({p: (lambda v=v: layers(v)) for p, v in vocoders.items()}, warmup, iters)
    R, S, A, G, n = geo["R"], geo["S"], geo["A"], geo["G"], geo["layers"]
    flop = 2.0 * ((3 * R + A) * G + R * (R + S)) * n * B * T
    hbm_bytes = 4.0 * (2 * R + A + 2 * S) * n * B * T
    floor_hbm_ms, floor_f32_ms = hbm_bytes / (HBM_TBS * 1e12) * 1e3, flop / (PEAK_F32_TFLOPS * 1e12) * 1e3
    audio = B * T / SR
    out = {"B": B, "frames": L, "audio_seconds": round(audio, 3), "waveform_max_diff_bf16_vs_f32_rel": diff, "layers_tflop": round(flop / 1e12, 3),
           "layers_hbm_gbytes": round(hbm_bytes / 1e9, 3), "layers_hbm_floor_ms": round(floor_hbm_ms, 3), "layers_f32_mfma_floor_ms": round(floor_f32_ms, 3)}
    for p in vocoders:
        out[p] = {"ms_per_call": round(call[p][0], 3), "ms_min_max": [round(call[p][1], 3), round(call[p][2], 3)],
                  "times_real_time": round(audio / (call[p][0] * 1e-3), 1), "layers_ms": round(lay[p][0], 3),
                  "layers_ms_min_max": [round(lay[p][1], 3), round(lay[p][2], 3)], "layers_share_of_call": round(lay[p][0] / call[p][0], 3),
                  "layers_tflops": round(flop / (lay[p][0] * 1e-3) / 1e12, 2), "layers_hbm_tbytes_per_s": round(hbm_bytes / (lay[p][0] * 1e-3) / 1e12, 3),
                  "layers_ms_over_hbm_floor": round(lay[p][0] / floor_hbm_ms, 2)}
    out["speedup_bf16_over_f32_call"] = round(call["f32"][0] / call["bf16"][0], 2)
    out["speedup_bf16_over_f32_layers"] = round(lay["f32"][0] / lay["bf16"][0], 2)
    out["bf16_faster"] = bool(call["bf16"][0] < call["f32"][0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_pwg_bf16.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_pwg_bf16.py measures on the GPU"
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.vocoder import PWG_DEFAULTS, ParallelWaveGAN, pwg_expected_shapes, pwg_geometry
    d = load_yaml(DEFAULT_YAML)
    d["Vocoder"] = dict(PWG_DEFAULTS)
    hp = Recursive_Parse(d)
    sd = random_weights(pwg_expected_shapes(pwg_geometry(hp)), 1234)
    vocoders = {p: ParallelWaveGAN(hp, "cuda:0", state_dict=sd, precision=p) for p in ("f32", "bf16")}
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup,
           "geometry": {k: vocoders["f32"].geo[k] for k in ("layers", "stacks", "R", "G", "S", "A", "ctx", "scales", "hop")}, "sample_rate": SR,
           "f32_mfma_peak_tflops": PEAK_F32_TFLOPS, "hbm_peak_tbytes_per_s": HBM_TBS, "results": [run(B, vocoders, args.warmup, args.iters) for B in (1, 32)]}
    out["bf16_faster_at_both_sizes"] = all(r["bf16_faster"] for r in out["results"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
