"""Long texts on one MI355X: the eval-mode attention core (glowtts_rpr_attention_fwd_eval) and end-to-end inference of a ~1000-character prompt.
  * attention core, H = 2, D = 96, win = 4, ragged-free rows: us per call for Tp in {128, 256, 512, 1024, 2048}, B in {1, 32}, f32 and bf16;
    at Tp <= 256 the training kernel (glowtts_rpr_attention_fwd_prec, which also writes P) side by side, the two interleaved in one process.
    GFLOP counts 4 B H Tp^2 D (the two contractions); TF/s against that.
  * `Inferencer`-style inference (GlowTTS of the default Hyper_Parameters.yaml, Vanilla, B = 1, 1000 tokens, injected noise, length scale 1):
    the encoder half (`inference_front`) and the inverse half (`inference_back` with the packed decoder weights), ms each, f32 and bf16.
Device time from hip events around `iters` back-to-back calls after `warmup`, median of `rounds`.  The waves-per-workgroup choice of the eval kernel
can be forced with the experiment build (`make -C glow_tts_amd/csrc tools`, GLOWTTS_LIB_PATH=tools/_build/libglowtts_hip_tools.so,
GLOWTTS_ATTN_EVAL_WAVES=1|2|4): each row records the variant the launch log saw.
Usage: python tools/bench_long_text.py [--iters 20] [--rounds 5] [--out profiles/bench_long_text.json]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def launched(prefix):
    """Names of the kernel classes with `prefix` that the launch log counted since its last reset."""
    import ctypes
    from glow_tts_amd import _lib
    buf = ctypes.create_string_buffer(1 << 17)
    _lib.api().glowtts_launch_log_dump(buf, len(buf))
    rows = [ln.rsplit(" ", 1) for ln in buf.value.decode().splitlines()]
    return [name for name, n in rows if name.startswith(prefix) and int(n) > 0]


def attention_rows(args):
    from glow_tts_amd import _lib
    from glow_tts_amd.conv_fn import _A
    L = _A()
    H, D, win = 2, 96, 4
    rows = []
    for B in (1, 32):
        for Tp in (128, 256, 512, 1024, 2048):
            g = torch.Generator().manual_seed(Tp + B)
            qkv = (torch.randn(B * Tp, 3 * H * D, generator=g) * 0.6).cuda()
            relk = (torch.randn(2 * win + 1, D, generator=g) * D ** -0.5).cuda()
            relv = (torch.randn(2 * win + 1, D, generator=g) * D ** -0.5).cuda()
            rowmask = torch.ones(B * Tp, device="cuda")
            out, oute = torch.empty(B * Tp, H * D, device="cuda"), torch.empty(B * Tp, H * D, device="cuda")
            P = torch.empty(B, H, Tp, Tp, device="cuda") if Tp <= 256 else None
            for prec in (0, 1):
                # both entries called directly on preallocated outputs: the same host cost per call, so a host-bound small shape skews neither
                fns = {"eval": lambda: L.glowtts_rpr_attention_fwd_eval(qkv.data_ptr(), relk.data_ptr(), relv.data_ptr(), rowmask.data_ptr(),
                                                                          oute.data_ptr(), B, Tp, H, D, win, prec, _lib.stream())}
                if P is not None:
                    fns["train"] = lambda: L.glowtts_rpr_attention_fwd_prec(qkv.data_ptr(), relk.data_ptr(), relv.data_ptr(), rowmask.data_ptr(),
                                                                              out.data_ptr(), P.data_ptr(), B, Tp, H, D, win, 0.0, 0, None, prec, _lib.stream())
                for fn in fns.values():
                    for _ in range(args.warmup):
                        fn()
                t = {k: [] for k in fns}
                for _ in range(args.rounds):                     # interleaved rounds: both kernels see the same clock history
                    for k, fn in fns.items():
                        t[k].append(event_ms(fn, args.iters))
                gflop = 4.0 * B * H * Tp * Tp * D / 1e9
                r = {"B": B, "Tp": Tp, "H": H, "D": D, "win": win, "precision": "bf16" if prec else "f32", "gflop": round(gflop, 4)}
                for k, v in t.items():
                    us = statistics.median(v) * 1e3
                    r[f"{k}_us"] = round(us, 2)
                    r[f"{k}_tflops"] = round(gflop / us * 1e3, 2)
                if "train_us" in r:
                    r["eval_over_train"] = round(r["eval_us"] / r["train_us"], 3)
                L.glowtts_launch_log_reset()
                fns["eval"]()
                torch.cuda.synchronize()
                r["eval_kernel"] = launched("attn_fwd_eval")
                rows.append(r)
                print(json.dumps(r), flush=True)
            del qkv, out, oute, P
            torch.cuda.empty_cache()
    return rows


def e2e_rows(args):
    rows = []
    Tt = 1000
    for precision in ("f32", "bf16"):
        dev = torch.device("cuda:0")
        model, _, hp = bench.build_model(precision, dev, mode="Vanilla")
        g = torch.Generator().manual_seed(17)
        tokens = torch.randint(2, 35, (1, Tt), generator=g).to(dev)
        tl = torch.tensor([Tt], device=dev)
        with torch.no_grad():                                    # ActNorm data init (the first forward), then eval
            model(tokens[:, :120], torch.tensor([120], device=dev), (torch.randn(1, 80, 400, generator=g) * 1.5).clamp(-4, 4).to(dev),
                  torch.tensor([400], device=dev), None, None, None)
        model.eval()
        prep = model.prepared_decoder_weights()
        ls = torch.tensor([1.0], device=dev)
        with torch.no_grad():
            front = model.inference_front(tokens, tl, length_scale=ls)
        frames = int(front[3].max())
        noise = torch.randn(1, 80, frames, generator=g).to(dev)

        def fr():
            with torch.no_grad():
                return model.inference_front(tokens, tl, length_scale=ls)

        def bk():
            with torch.no_grad():
                return model.inference_back(front, None, 0.667, noise, prep=prep)
        for fn in (fr, bk):
            for _ in range(args.warmup):
                fn()
        tf, tb = [], []
        for _ in range(args.rounds):
            tf.append(event_ms(fr, max(1, args.iters // 4)))
            tb.append(event_ms(bk, max(1, args.iters // 4)))
        r = {"precision": precision, "B": 1, "tokens": Tt, "mel_frames": frames, "encoder_half_ms": round(statistics.median(tf), 3),
             "inverse_half_ms": round(statistics.median(tb), 3)}
        r["total_ms"] = round(r["encoder_half_ms"] + r["inverse_half_ms"], 3)
        rows.append(r)
        print(json.dumps(r), flush=True)
        del model, prep, front
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_long_text.json"))
    ap.add_argument("--attention-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_long_text.py measures on the GPU"
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
           "attention": attention_rows(args), "end_to_end": [] if args.attention_only else e2e_rows(args)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
