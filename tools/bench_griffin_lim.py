"""Griffin-Lim vocoder (glow_tts_amd/vocoder.py, csrc/vocoder_ops.hip) on one MI355X: B = 1 x 800 and B = 32 x 800 frames, 60 iterations, n_fft 2048,
window 1024, hop 256 (the default Hyper_Parameters.yaml).  Per size:
  * ms per call of `GriffinLim.griffin_lim` (start spectrum + inverse STFT + 60 x (fused step + overlap-add)), ms per iteration, and the real-time
    factor at 24 kHz (seconds of audio per second of compute);
  * the bytes an iteration moves by the kernels' own argument sizes (step: two signals gathered under the window + the magnitudes in, the frames'
    contributions out; overlap-add: win / hop contributions per sample in, the signal out) against the achieved bandwidth;
  * the BASELINE: the same loop - same update rule, floors and start - written HERE with torch.stft / torch.istft (rocFFT, complex spectrogram in HBM) on
    the same device and inputs, and HIP-over-baseline speed-up;
  * the final spectral convergence || |STFT(x)| - S || / || S || of both (computed with the baseline's STFT), so the two are seen to do the same work.
Targets are |STFT| of seeded harmonic-plus-noise signals; the start phase is shared.  Median of `--iters` (>= 20) timed calls after `--warmup`, each a host
clock around a call that ends in a device synchronise; the sustained clock is noted as tools/bench_vc.py does.
Usage: python tools/bench_griffin_lim.py [--iters 20] [--out profiles/bench_griffin_lim.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402

N_FFT, WIN, HOP, SR, FRAMES, ITERATIONS, MOMENTUM = 2048, 1024, 256, 24000, 800, 60, 0.99


def signals(B, L, dev):
    """[B, L]: 30 harmonics of a per-utterance f0 with a slow on/off envelope, 2 % noise (seeded)."""
    g = torch.Generator().manual_seed(11)
    t = torch.arange(L, dtype=torch.float64)[None, :] / SR
    f0 = 90.0 + 120.0 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    x = sum(torch.sin(2 * torch.pi * k * f0 * t + 6.28 * torch.rand(B, 1, generator=g, dtype=torch.float64)) / k for k in range(1, 31))
    x = x * torch.clamp(1.5 * torch.sin(2 * torch.pi * 2.5 * t) + 0.5, 0.0, 1.0)
    x = 0.5 * x / x.abs().amax(dim=1, keepdim=True) + 0.01 * torch.randn(B, L, generator=g, dtype=torch.float64)
    return x.float().to(dev)


def torch_window(dev):
    w = torch.zeros(N_FFT, device=dev)
    lpad = (N_FFT - WIN) // 2
    w[lpad:lpad + WIN] = torch.hann_window(WIN, periodic=True, device=dev)
    return w


def torch_stft(x, w):
    return torch.stft(x, N_FFT, HOP, N_FFT, window=w, center=True, pad_mode="reflect", return_complex=True).transpose(1, 2)     # [B, T, F]


def torch_griffin_lim(mag, phase, w, iterations, alpha):
    """The baseline: the loop of vocoder.GriffinLim.griffin_lim on torch.stft / torch.istft."""
    L = HOP * (mag.shape[1] - 1)
    inv = lambda s: torch.istft(s.transpose(1, 2), N_FFT, HOP, N_FFT, window=w, center=True, length=L)
    x = inv(torch.polar(mag, phase))
    xp = x
    for _ in range(iterations):
        y = x + alpha * (x - xp)
        Y = torch_stft(y, w)
        xp, x = x, inv(mag * (Y / Y.abs().clamp_min(1e-8)))
    return x


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


def iteration_bytes(B, T):
    """HBM bytes of one iteration by the kernels' argument sizes (the window and twiddle tables, 12 KiB, stay in cache)."""
    F, L = N_FFT // 2 + 1, HOP * (T - 1)
    step = B * T * (2 * WIN + F + WIN) * 4              # gathers of x_n and x_n-1 under the window, magnitudes; contributions out
    ola = B * L * (WIN // HOP + 1) * 4                  # win / hop contributions per sample, one sample out
    return step, ola


def run(B, vocoder, warmup, iters):
    dev = vocoder.device
    T = FRAMES
    L = HOP * (T - 1)
    w = torch_window(dev)
    x = signals(B, L, dev)
    mag = torch_stft(x, w).abs().contiguous()
    assert mag.shape == (B, T, N_FFT // 2 + 1)
    phase = (torch.rand(mag.shape, device=dev, generator=torch.Generator(dev).manual_seed(3)) * 2 - 1) * torch.pi
    lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
    sc = lambda y: float((torch_stft(y, w).abs() - mag).norm() / mag.norm())
    hip = lambda: vocoder.griffin_lim(mag, lengths, ITERATIONS, MOMENTUM, phase)[0]
    base = lambda: torch_griffin_lim(mag, phase, w, ITERATIONS, MOMENTUM)
    y_hip, y_base = hip(), base()
    res = {"B": B, "frames": T, "iterations": ITERATIONS, "momentum": MOMENTUM, "audio_seconds": round(B * L / SR, 3),
           "spectral_convergence": {"hip": round(sc(y_hip), 5), "baseline": round(sc(y_base), 5)},
           "waveform_rel_l2_hip_vs_baseline": float((y_hip - y_base).norm() / y_base.norm())}
    # alternate the two so that a drifting clock or a noisy neighbour meets both
    h1 = median_ms(hip, warmup, iters // 2)
    b1 = median_ms(base, warmup, iters // 2)
    h2 = median_ms(hip, 1, iters - iters // 2)
    b2 = median_ms(base, 1, iters - iters // 2)
    hip_ms, base_ms = (h1[0] + h2[0]) / 2, (b1[0] + b2[0]) / 2
    # the iterations alone: calls of 60 and of 0 iterations differ by the loop
    h0 = median_ms(lambda: vocoder.griffin_lim(mag, lengths, 0, MOMENTUM, phase), 2, iters)[0]
    step_b, ola_b = iteration_bytes(B, T)
    per_it = (hip_ms - h0) / ITERATIONS
    res["hip"] = {"ms_per_call": round(hip_ms, 3), "ms_min_max": [round(min(h1[1], h2[1]), 3), round(max(h1[2], h2[2]), 3)],
                  "ms_per_call_halves": [round(h1[0], 3), round(h2[0], 3)], "ms_start_only": round(h0, 3), "ms_per_iteration": round(per_it, 4),
                  "real_time_factor": round(B * L / SR / (hip_ms * 1e-3), 1),
                  "bytes_per_iteration": {"step": step_b, "overlap_add": ola_b}, "achieved_GBps": round((step_b + ola_b) / (per_it * 1e-3) / 1e9, 1)}
    res["baseline_torch_stft"] = {"ms_per_call": round(base_ms, 3), "ms_min_max": [round(min(b1[1], b2[1]), 3), round(max(b1[2], b2[2]), 3)],
                                  "ms_per_call_halves": [round(b1[0], 3), round(b2[0], 3)], "ms_per_iteration": round(base_ms / ITERATIONS, 4),
                                  "real_time_factor": round(B * L / SR / (base_ms * 1e-3), 1)}
    res["speedup_hip_over_baseline"] = round(base_ms / hip_ms, 2)
    res["hip_faster"] = bool(hip_ms < base_ms)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_griffin_lim.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_griffin_lim.py measures on the GPU"
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.vocoder import GriffinLim
    vocoder = GriffinLim(Recursive_Parse(load_yaml(DEFAULT_YAML)), "cuda:0")
    assert vocoder.geo == (N_FFT, WIN, HOP)
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup,
           "geometry": {"n_fft": N_FFT, "win_length": WIN, "hop": HOP, "sample_rate": SR},
           "results": [run(B, vocoder, args.warmup, args.iters) for B in (1, 32)]}
    out["hip_faster_at_both_sizes"] = all(r["hip_faster"] for r in out["results"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
