"""Voice conversion through the invertible decoder (GlowTTS.voice_conversion / encode_mels) at full width: SE-LUT model of the default
Hyper_Parameters.yaml (12 flows x 4 WaveNet layers x 192 channels), B = 32 x 800 frames, f32 and bf16.  Per precision:
  * voice_conversion: ms per call, mel frames per second (valid frames of the batch over the call time);
  * encode_mels alone, beside the eval GlowTTS.forward on the same mels (no_grad: text encoder, decoder forward with its kept activations, MAS);
  * the inverse alone: decoder.decoder_inverse on the same z under the target conditioning (what inference_back runs after its prior sample,
    weights packed per call as there);
  * the peak allocated bytes above the resident model + inputs of each.
Host clock around `iters` calls that end in a device synchronise, after `warmup` calls.  Usage: python tools/bench_vc.py [--iters 10] [--out FILE]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402

B, TT, TM = 32, 120, 800


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
        del out
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    return dt * 1e3, torch.cuda.max_memory_allocated() - base


def run(precision, warmup, iters):
    from glow_tts_amd import decoder
    dev = torch.device("cuda:0")
    model, _, hp = bench.build_model(precision, dev, mode="SE", spk_type="LUT")
    tokens, tl, mels, ml = bench.synthetic_batch(B, TT, TM, 80, 1, dev)
    g = torch.Generator().manual_seed(9)
    spk = torch.randint(0, int(hp.Speaker_Embedding.Num_Speakers), (B,), generator=g).to(dev)
    tspk = torch.randint(0, int(hp.Speaker_Embedding.Num_Speakers), (B,), generator=g).to(dev)
    with torch.no_grad():
        model(tokens, tl, mels, ml, spk, None, None)                # ActNorm data init (the first forward)
    model.eval()
    frames = int(((ml // 2) * 2).sum())
    rows = B * (TM // 2 + 4)
    res = {"precision": precision, "B": B, "frames_per_utt": TM, "valid_frames": frames, "squeezed_rows": rows}
    ms, peak = timed(lambda: model.voice_conversion(mels, ml, spk, target_speakers=tspk), warmup, iters)
    res["voice_conversion"] = {"ms": round(ms, 3), "mel_frames_per_s": round(frames / ms * 1e3), "peak_bytes": peak, "peak_bytes_per_row": round(peak / rows)}
    ms, peak = timed(lambda: model.encode_mels(mels, ml, spk), warmup, iters)
    res["encode_mels"] = {"ms": round(ms, 3), "peak_bytes": peak, "peak_bytes_per_row": round(peak / rows)}

    def fwd():
        with torch.no_grad():
            return model(tokens, tl, mels, ml, spk, None, None)
    ms, peak = timed(fwd, warmup, iters)
    res["eval_forward"] = {"ms": round(ms, 3), "peak_bytes": peak, "peak_bytes_per_row": round(peak / rows)}
    z, zl = model.encode_mels(mels, ml, spk)
    P = model._params()
    stacks = model._stacks(P)

    def inv():
        with torch.no_grad():
            W = dict(zip(decoder.WEIGHT_KEYS, [w.contiguous() for w in stacks.weights()]))
            cond = stacks.conditioning(torch.nn.functional.embedding(tspk, P["layer_Dict.LUT.weight"]), None)
            return decoder.decoder_inverse(model.dec_cfg, W, z, zl, cond=cond, fill=-4.0)
    ms, peak = timed(inv, warmup, iters)
    res["inverse"] = {"ms": round(ms, 3), "peak_bytes": peak, "peak_bytes_per_row": round(peak / rows)}
    res["conversion_over_inverse"] = round(res["voice_conversion"]["ms"] / res["inverse"]["ms"], 3)
    res["encode_over_eval_forward"] = round(res["encode_mels"]["ms"] / res["eval_forward"]["ms"], 3)
    del model
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vc.py measures on the GPU"
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup,
           "results": [run(p, args.warmup, args.iters) for p in ("f32", "bf16")]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
