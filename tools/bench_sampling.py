"""What seeded sampling (the fused glowtts_prior_sample launch) costs or saves against the unseeded path, on one MI355X.
Full-width Vanilla model (default Hyper_Parameters.yaml), 160 tokens x 5 frames = 800 frames per utterance, B = 1 and B = 32, f32 and bf16.  Two timings:
  * prelude   the back half of inference up to the first decoder launch - durations -> hard alignment -> dense attentions -> expanded prior -> sample
              (`GlowTTS._unseeded_sample` / `GlowTTS._seeded_sample`), each captured as a hipGraph at the mel bucket serving picks (896) and replayed:
              device time per replay from hip events; and the launches each one issues into the launch log (torch's own kernels are not in that log).
  * call      the whole of `GraphedInference.__call__` (front graph, the length read, back graph), host wall clock around call + synchronize.
Both paths alternate in ONE process and the unseeded path is measured as two interleaved series (A/A): per round  unseeded (a1), seeded, unseeded (a2).
Median of `--calls` timed calls after `--warmup`.  The A/A spread |median(a1) - median(a2)| is the noise of this very run: `seeded_within_aa_spread`
says whether median(seeded) - median(a1 + a2) stays within it.
Usage: python tools/bench_sampling.py [--calls 20] [--warmup 5] [--out profiles/bench_sampling.json]"""
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

import bench  # noqa: E402

TOKENS, FRAMES_PER_TOKEN, BUCKET = 160, 5, 896


def launch_log():
    import ctypes
    from glow_tts_amd import _lib
    buf = ctypes.create_string_buffer(1 << 17)
    _lib.api().glowtts_launch_log_dump(buf, len(buf))
    rows = [ln.rsplit(" ", 1) for ln in buf.value.decode().splitlines()]
    return {name: int(n) for name, n in rows if int(n) > 0}


def interleaved(fns, calls, warmup, timer):
    """fns: name -> callable, run round-robin in the given order; -> name -> [seconds or ms per call]"""
    for _ in range(warmup):
        for fn in fns.values():
            timer(fn)
    t = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            t[k].append(timer(fn))
    return t


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summarise(t, unit_scale=1.0, digits=4):
    a1, s, a2 = (statistics.median(t[k]) * unit_scale for k in ("unseeded_a1", "seeded", "unseeded_a2"))
    both = statistics.median(t["unseeded_a1"] + t["unseeded_a2"]) * unit_scale
    spread = abs(a1 - a2)
    return {"unseeded_a1": round(a1, digits), "unseeded_a2": round(a2, digits), "unseeded": round(both, digits), "seeded": round(s, digits),
            "aa_spread": round(spread, digits), "seeded_minus_unseeded": round(s - both, digits), "seeded_within_aa_spread": bool(s - both <= spread)}


def capture(fn, stream, warmup=2):
    cur = torch.cuda.current_stream()
    stream.wait_stream(cur)
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
    cur.wait_stream(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def rows_for(precision, B, args):
    from glow_tts_amd import _lib
    from glow_tts_amd.alignment import seed_words
    from glow_tts_amd.graph_infer import GraphedInference
    dev = torch.device("cuda:0")
    model, _, hp = bench.build_model(precision, dev, mode="Vanilla")
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():                                    # a fixed 5 frames per token; ActNorm data init (the first forward)
        wq = "layer_Dict.Encoder.layer_Dict.Duration_Predictor.layer_Dict.Projection"
        sd = model.state_dict()
        sd[wq + ".weight"].zero_()
        sd[wq + ".bias"].fill_(math.log(FRAMES_PER_TOKEN - 0.5))
        model(torch.randint(2, 35, (1, 120), generator=g).to(dev), torch.tensor([120], device=dev),
              (torch.randn(1, 80, 400, generator=g) * 1.5).clamp(-4, 4).to(dev), torch.tensor([400], device=dev), None, None, None)
    model.eval()
    tokens = torch.randint(2, 35, (B, TOKENS), generator=g).to(dev)
    tl = torch.full((B,), TOKENS, device=dev)
    seeds = torch.stack([torch.arange(B), torch.arange(B) + 1000], 1)
    gi = GraphedInference(model)
    _, lengths, _ = gi(tokens, tl, noise_scale=0.667)
    frames = int(lengths.max())
    assert frames == TOKENS * FRAMES_PER_TOKEN, frames
    r = {"precision": precision, "B": B, "tokens": TOKENS, "mel_frames": frames, "bucket": BUCKET}

    # ---- the prelude alone, as replayed graphs
    with torch.no_grad():
        mean, log_std, dur, mel_lengths = (t.clone() for t in model.inference_front(tokens, tl, length_scale=1.0)[:4])
        sd_t, sc_t, ns_t = seed_words(seeds, B, dev), torch.full((B,), 0.667, device=dev), torch.tensor(0.667, device=dev)
        un = lambda: model._unseeded_sample(mean, log_std, dur, mel_lengths, BUCKET, ns_t, None)
        se = lambda: model._seeded_sample(mean, log_std, dur, mel_lengths, BUCKET, sc_t, sd_t)
        logs = {}
        for name, fn in (("unseeded", un), ("seeded", se)):
            _lib.api().glowtts_launch_log_reset()
            fn()
            torch.cuda.synchronize()
            logs[name] = launch_log()
        stream = torch.cuda.Stream()
        gu, _ = capture(un, stream)
        gs, _ = capture(se, stream)
    t = interleaved({"unseeded_a1": gu.replay, "seeded": gs.replay, "unseeded_a2": gu.replay}, args.calls, args.warmup, event_ms)
    r["prelude_us"] = summarise(t, 1e3, 2)
    r["prelude_launch_log"] = logs

    # ---- the whole serving call
    call_u = lambda: gi(tokens, tl, noise_scale=0.667)
    call_s = lambda: gi(tokens, tl, noise_scale=0.667, seeds=seeds)
    t = interleaved({"unseeded_a1": call_u, "seeded": call_s, "unseeded_a2": call_u}, args.calls, args.warmup, wall_ms)
    r["call_ms"] = summarise(t)
    print(json.dumps(r), flush=True)
    del gi, model, gu, gs
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_sampling.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sampling.py measures on the GPU"
    rows = [rows_for(precision, B, args) for precision in ("f32", "bf16") for B in (1, 32)]
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup, "rows": rows,
           "seeded_within_aa_spread": all(r["call_ms"]["seeded_within_aa_spread"] and r["prelude_us"]["seeded_within_aa_spread"] for r in rows)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
