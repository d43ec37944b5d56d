"""What the teacher-forced pass (`GlowTTS.teacher_forced(reconstruct=True)`) costs against the composition that was possible without it, on one MI355X.
Full-width Vanilla model (default Hyper_Parameters.yaml), 120 tokens x 800 frames per utterance, B = 32 and B = 1, f32 and bf16.
  * teacher_forced  encode-only flows, text encoder, log-prior + alignment search, one launch from the index to durations / score / seeded sample, inverse flows
  * composition     the eval-mode `forward` under no_grad (every activation kept, the dense [B, Tx, Ty] attentions written), `attn.sum` for the durations,
                    the expanded prior it returns sampled with torch (`exp`, `randn_like`, the frame mask), `_inverse_flow`
Both alternate in ONE process, and the composition is measured as two interleaved series (A/A): per round  composition (a1), teacher_forced, composition
(a2).  Host wall clock around call + synchronize (the calls are eager), median of `--calls` timed calls after `--warmup`; the A/A spread
|median(a1) - median(a2)| is the noise of this very run.  Peak allocation: `torch.cuda.max_memory_allocated` over one call, above what was allocated when
it began.  The two do not draw the same noise (counter hash against torch's generator), so their mels differ; the alignments are compared.
Usage: python tools/bench_align.py [--calls 20] [--warmup 5] [--out profiles/bench_align.json]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402
from bench_sampling import interleaved, launch_log, wall_ms  # noqa: E402

TOKENS, FRAMES, NOISE_SCALE = 120, 800, 0.667


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2 ** 20, 2)


def rows_for(precision, B, args):
    from glow_tts_amd import _lib
    dev = torch.device("cuda:0")
    model, _, hp = bench.build_model(precision, dev, mode="Vanilla")
    g = torch.Generator().manual_seed(17)
    tokens = torch.randint(2, 35, (B, TOKENS), generator=g).to(dev)
    tl = torch.full((B,), TOKENS, device=dev)
    mels = (torch.randn(B, 80, FRAMES, generator=g) * 1.5).clamp(-4, 4).to(dev)
    ml = torch.full((B,), FRAMES, device=dev)
    seeds = torch.stack([torch.arange(B), torch.arange(B) + 1000], 1)
    with torch.no_grad():
        model(tokens, tl, mels, ml, None, None, None)        # ActNorm data init (the first forward, train mode)
    model.eval()
    scales = torch.full((B,), NOISE_SCALE, device=dev)

    @torch.no_grad()
    def teacher_forced():
        return model.teacher_forced(tokens, tl, mels, ml, noise_scale=scales, seeds=seeds, reconstruct=True)

    @torch.no_grad()
    def composition():
        z, mel_mean, mel_log_std, _, _, _, attn, _ = model(tokens, tl, mels, ml, None, None, None)
        durations = attn.sum(2)
        mask = model.Mask_Generate(ml, mel_mean.shape[2])
        sample = (mel_mean + torch.exp(mel_log_std) * torch.randn_like(mel_mean) * NOISE_SCALE) * mask
        out, _, _ = model._inverse_flow((sample, attn), ml, None, None, None, None, None)
        return durations, out

    r = {"precision": precision, "B": B, "tokens": TOKENS, "mel_frames": FRAMES}
    logs = {}
    for name, fn in (("composition", composition), ("teacher_forced", teacher_forced)):
        fn()                                                  # (caches warm)
        _lib.api().glowtts_launch_log_reset()
        out = fn()
        torch.cuda.synchronize()
        logs[name] = sum(launch_log().values())
        if name == "composition":
            want = out[0]
        else:
            r["durations_equal"] = bool(torch.equal(out.durations, want.to(torch.int32)))
        del out
    r["logged_launches"] = logs
    t = interleaved({"composition_a1": composition, "teacher_forced": teacher_forced, "composition_a2": composition}, args.calls, args.warmup, wall_ms)
    a1, tf, a2 = (statistics.median(t[k]) for k in ("composition_a1", "teacher_forced", "composition_a2"))
    both = statistics.median(t["composition_a1"] + t["composition_a2"])
    r["call_ms"] = {"composition_a1": round(a1, 4), "composition_a2": round(a2, 4), "composition": round(both, 4), "teacher_forced": round(tf, 4),
                    "aa_spread": round(abs(a1 - a2), 4), "composition_over_teacher_forced": round(both / tf, 3)}
    r["peak_mib"] = {"composition": peak_mib(composition), "teacher_forced": peak_mib(teacher_forced)}
    print(json.dumps(r), flush=True)
    del model
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_align.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_align.py measures on the GPU"
    rows = [rows_for(precision, B, args) for precision in ("f32", "bf16") for B in (32, 1)]
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup, "rows": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
