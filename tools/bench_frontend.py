"""Analysis front end (glow_tts_amd/frontend.py, csrc/frontend_ops.hip) on one MI355X at the default Hyper_Parameters.yaml (n_fft 2048, window 1024, hop 256,
80 mels, 24 kHz): B = 32 x 800 and B = 1 x 800 frames.  Per size:
  * ms per call of the device mel alone (`Analyzer.mel`), the device YIN alone (`Analyzer.yin`) and both with the normalised track (`mel` + `pitch`), on
    signals already on the device: median of `--iters` (>= 20) timed calls after `--warmup`, each a host clock around a call that ends in a synchronise;
  * the bytes the mel kernel moves by its own argument sizes against the achieved bandwidth, and the YIN's difference terms per second;
  * the HOST path of the parent commit on the same box and the same audio: `audio.mel_generate` + `audio.yin_pitch` per utterance on 16 threads (median of
    `--host-iters` calls), and device-over-host speed-up;
  * the worst |device mel - host mel| and the YIN frames that differ, so the two are seen to do the same work.
Then `Pattern_Generator.py` end to end, in-process, on a synthetic corpus of 200 files (LJ layout, 2 .. 8 s each) with and without `--host`, 16 host
threads: files per second including decode, trim, pickling and the metadata pass - the figure a user sees; the host stages bound it.
The sustained clock is noted as tools/bench_vc.py does.
Usage: python tools/bench_frontend.py [--iters 20] [--out profiles/bench_frontend.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tools.bench_griffin_lim import median_ms, signals  # noqa: E402

N_FFT, WIN, HOP, SR, FRAMES, MEL, THREADS, FILES = 2048, 1024, 256, 24000, 800, 80, 16, 200


def host_pass(wavs, hp, pool):
    s = hp.Sound
    from glow_tts_amd import audio

    def one(x):
        mel = audio.mel_generate(x, s.Sample_Rate, s.Mel_Dim, s.Spectrogram_Dim, s.Frame_Length, s.Frame_Shift, mel_fmin=s.Mel_F_Min, mel_fmax=s.Mel_F_Max,
                                 max_abs_value=s.Max_Abs_Mel)
        return mel, audio.yin_pitch(x, s.Sample_Rate, 1.0 - float(s.Confidence_Threshold))
    return list(pool.map(one, wavs))


def run(B, an, hp, warmup, iters, host_iters, pool):
    L = HOP * (FRAMES - 1)
    x = signals(B, L, an.device)
    host_x = list(x.cpu().numpy())
    mel, _ = an.mel(x)
    hz, frames, _ = an.yin(x)
    want = host_pass(host_x, hp, pool)
    res = {"B": B, "frames": FRAMES, "audio_seconds": round(B * L / SR, 3),
           "worst_abs_mel_difference_to_host": float(max(np.abs(m - w[0]).max() for m, w in zip(mel.cpu().numpy(), want))),
           "yin_frames_differing_from_host": int(sum((h[:len(w[1])] != w[1].astype(np.float32)).sum() for h, w in zip(hz.cpu().numpy(), want))),
           "yin_frames": int(frames.sum())}
    t_mel = median_ms(lambda: an.mel(x), warmup, iters)
    t_yin = median_ms(lambda: an.yin(x), warmup, iters)
    t_both = median_ms(lambda: (an.mel(x), an.pitch(x)), warmup, iters)
    ts = []
    for _ in range(host_iters):
        t0 = time.perf_counter()
        host_pass(host_x, hp, pool)
        ts.append((time.perf_counter() - t0) * 1e3)
    host_ms = statistics.median(ts)
    mel_bytes = B * FRAMES * (WIN + MEL) * 4                        # the samples under every window in (L2 absorbs the 4 x overlap or not: counted), a mel row out
    yin_terms = B * FRAMES * sum(1024 - tau for tau in range(1, an.tau_max))
    f = lambda t: {"ms_per_call": round(t[0], 4), "ms_min_max": [round(t[1], 4), round(t[2], 4)]}
    res["device"] = {"mel": dict(f(t_mel), achieved_GBps=round(mel_bytes / (t_mel[0] * 1e-3) / 1e9, 1)),
                     "yin": dict(f(t_yin), difference_terms_per_second=float("%.3g" % (yin_terms / (t_yin[0] * 1e-3)))),
                     "mel_and_normalised_pitch": dict(f(t_both), real_time_factor=round(B * L / SR / (t_both[0] * 1e-3), 1))}
    res["host_16_threads"] = {"ms_per_call": round(host_ms, 2), "ms_min_max": [round(min(ts), 2), round(max(ts), 2)], "calls": host_iters,
                              "real_time_factor": round(B * L / SR / (host_ms * 1e-3), 1)}
    res["speedup_device_over_host"] = round(host_ms / t_both[0], 1)
    return res


def corpus(root, n):
    """n wavs of 2 .. 8 s in the LJ layout: harmonic tones with an envelope and quiet ends, 16-bit at 24 kHz."""
    from scipy.io import wavfile
    rng = np.random.default_rng(5)
    os.makedirs(os.path.join(root, "wavs"))
    total = 0
    with open(os.path.join(root, "metadata.csv"), "w") as f:
        for i in range(n):
            m = int(SR * rng.uniform(2.0, 8.0))
            t = np.arange(m) / SR
            f0 = rng.uniform(90, 210)
            x = sum(np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 6.28)) / k for k in range(1, 21))
            x = x * np.clip(1.5 * np.sin(2 * np.pi * 2.5 * t) + 0.5, 0.0, 1.0)
            x = 0.5 * x / np.abs(x).max() + 0.005 * rng.standard_normal(m)
            x = np.concatenate([1e-4 * rng.standard_normal(SR // 5), x, 1e-4 * rng.standard_normal(SR // 5)])
            wavfile.write(os.path.join(root, "wavs", "F{:04d}.wav".format(i)), SR, np.round(x * 32767 * 0.9).astype(np.int16))
            f.write("F{:04d}|the same few words for every file|the same few words for every file\n".format(i))
            total += len(x)
    return total / SR


def generator_runs(tmp):
    import yaml
    from glow_tts_amd import pattern_generator
    from glow_tts_amd.hparams import DEFAULT_YAML, load_yaml
    seconds = corpus(os.path.join(tmp, "corpus"), FILES)
    out = {"files": FILES, "audio_seconds": round(seconds, 1), "host_threads": THREADS}
    for mode in ("device", "host", "device_second_run"):           # the second device run has the file cache and the allocator warm, like the host run after it
        d = load_yaml(DEFAULT_YAML)
        root = os.path.join(tmp, mode)
        os.makedirs(root)
        d["Token_Path"] = os.path.join(root, "Token.yaml")
        d["Train"]["Train_Pattern"]["Path"], d["Train"]["Eval_Pattern"]["Path"] = os.path.join(root, "train"), os.path.join(root, "eval")
        with open(os.path.join(root, "hp.yaml"), "w") as f:
            yaml.dump(d, f)
        t0 = time.perf_counter()
        res = pattern_generator.main(["-hp", os.path.join(root, "hp.yaml"), "-lj", os.path.join(tmp, "corpus"), "-text", "-mw", str(THREADS), "-evalm", "2"]
                                     + (["--host"] if mode == "host" else []))
        dt = time.perf_counter() - t0
        assert res["written"] == FILES and res["failed"] == 0
        out[mode] = {"seconds_patterns_only": round(res["seconds"], 3), "seconds_with_metadata": round(dt, 3),
                     "files_per_second": round(FILES / res["seconds"], 1), "files_per_second_with_metadata": round(FILES / dt, 1)}
    out["speedup_device_over_host"] = round(out["host"]["seconds_patterns_only"] / out["device_second_run"]["seconds_patterns_only"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_frontend.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_frontend.py measures on the GPU"
    from glow_tts_amd.frontend import Analyzer
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    hp = Recursive_Parse(load_yaml(DEFAULT_YAML))
    an = Analyzer(hp, "cuda:0")
    assert an.geo == (N_FFT, WIN, HOP) and an.n_mel == MEL
    ghz, _ = bench.sustained_mfma_clock()
    with ThreadPoolExecutor(THREADS) as pool:
        results = [run(B, an, hp, args.warmup, args.iters, args.host_iters, pool) for B in (32, 1)]
    with tempfile.TemporaryDirectory() as tmp:
        gen = generator_runs(tmp)
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup,
           "geometry": {"n_fft": N_FFT, "win_length": WIN, "hop": HOP, "mel": MEL, "sample_rate": SR, "yin": [1024, 256, an.tau_min, an.tau_max]},
           "results": results, "pattern_generator": gen}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
