"""Mixed-precision training of the HiFi-GAN generator (`Vocoder.Train.Precision: 'mixed'`: csrc/hifigan_f16_ops.hip forward, csrc/hifigan_mixed_ops.hip
backward) on one MI355X at the V1 sizes and the trainer's default batch (16 segments of 32 frames), `hifigan_init` weights.  Three sides are called
ALTERNATELY, so that a drifting clock meets all of them: the mixed step, the unchanged f32 HIP step, and the torch f32 autograd step of
tools/bench_hifigan_train.py.  Reported, as medians of `--iters` (>= 20) timed calls per side after `--warmup`:
  * forward + backward of the generator under a fixed d wav, and the whole `Train_Step`, for the three sides;
  * the f32-against-f32 A/A spread: a second, identical f32 HIP trainer alternated with the first (what two equal sides differ by);
  * the 78 weight-gradient launch pairs replayed alone at the step's shapes, in both modes;
  * the one `hifigan_pack_images` launch against the torch image build that the f32 mode runs at every `generate`;
  * the mixed forward + backward against its HBM floor: the fp32 slabs that every launch reads and writes once (`hbm_floats_per_frame`, derived in DESIGN.md
    "Training the HiFi-GAN generator: mixed precision") over the 8 TB/s of the MI355X's HBM; weights, halo rows and the partial sums are not counted.
There is no target ratio: the figures are printed as they fall, and `mixed_faster_than_f32` / `mixed_faster_than_torch` say plainly which side won.
Usage: python tools/bench_hifigan_train_mixed.py [--iters 20] [--out profiles/bench_hifigan_train_mixed.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_hifigan import macs_per_frame, timed, torch_generator  # noqa: E402
from bench_hifigan_train import write_corpus  # noqa: E402

HBM_TBS = 8.0


def hbm_floats_per_frame(geo):
    """fp32 floats per mel frame that the launches of one mixed forward + backward read and write, every slab once per launch: a convolution reads its input
    (and its residual) and writes its output; a data gradient reads dy, the kept x (the mask) and its residual and writes dx; a weight gradient reads x and
    dy; conv_post's forward, `hifigan_post_bwd` (d wav, wav, x -> d pre, dx) and its weight gradient."""
    type1 = geo["resblock"] == "1"
    n = 2 * (geo["A"] + geo["C0"])                                  # conv_pre: forward and weight gradient (no data gradient)
    cin, mult = geo["C0"], 1
    for u, c in zip(geo["rates"], geo["channels"]):
        up_in, rows = mult * cin, mult * u * c
        n += (up_in + rows) + (rows + 2 * up_in) + (up_in + rows)   # the transposed convolution: forward, data gradient, weight gradient
        for ds in geo["rd"]:
            for _ in ds:
                if type1:                                           # conv1: in, out | dy, x, residual, dx | x, dy;  conv2: in, residual, out | dy, x, dx | x, dy
                    n += (2 + 4 + 2) * rows + (3 + 3 + 2) * rows
                else:
                    n += (3 + 4 + 2) * rows
        cin, mult = c, mult * u
    rows, wav = mult * cin, mult
    return n + (rows + wav) + (3 * wav + 2 * rows) + (rows + wav)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_hifigan_train_mixed.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_hifigan_train_mixed.py measures on the GPU"
    from glow_tts_amd import _lib, ops, optim
    from glow_tts_amd.hifigan_trainer import HiFiGAN_Trainer
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.vocoder import HIFIGAN_DEFAULTS, HIFIGAN_LAST_SLOPE, HIFIGAN_SLOPE, HiFiGAN, hifigan_convs, hifigan_train_launches
    with tempfile.TemporaryDirectory() as root:
        d = load_yaml(DEFAULT_YAML)
        d["Vocoder"] = dict(HIFIGAN_DEFAULTS, Train={"Checkpoint_Path": os.path.join(root, "ckpt")})
        d["Train"]["Train_Pattern"].update(Path=root, Metadata_File="METADATA.PICKLE")
        d["Train"]["Eval_Pattern"].update(Path="", Metadata_File="METADATA.PICKLE")
        write_corpus(root, d["Sound"]["Mel_Dim"], d["Sound"]["Frame_Shift"], 32)
        dm = copy.deepcopy(d)
        dm["Vocoder"]["Train"]["Precision"] = "mixed"
        f32, f32_twin, mixed = (HiFiGAN_Trainer(hp=Recursive_Parse(copy.deepcopy(x)), seed=0) for x in (d, d, dm))
        mel, target = (t.to(f32.device).contiguous() for t in f32.sampler["Train"].batch(0))
    assert (f32.model.train_precision, mixed.model.train_precision) == ("f32", "mixed")
    geo, s, dev = f32.model.geo, f32.set, f32.device
    B, _, L = mel.shape
    lengths = [L] * B
    base_w = {k: p.detach().clone().requires_grad_(True) for k, p in f32.model.params.items()}
    base_opt = optim.RAdam(list(base_w.values()), lr=float(s["Learning_Rate"]), eps=float(s["Epsilon"]))
    dwav = torch.randn(B, L * geo["hop"], generator=torch.Generator().manual_seed(1)).to(dev)

    def zero(params):
        for p in params:
            p.grad = None

    def hip_fb(tr):
        def run():
            zero(tr.params)
            tr.model.generate(mel, lengths)[0].backward(dwav)
        return run

    def base_fb():
        zero(base_w.values())
        torch_generator(base_w, geo, mel).backward(dwav)

    def base_step():
        zero(base_w.values())
        f32.criterion(torch_generator(base_w, geo, mel), target).backward()
        optim.clip_grad_norm_(list(base_w.values()), float(s["Gradient_Norm"]), _table_key=("bench_base", 0))
        base_opt.step()

    def rounds(sides, warmup, iters):
        """the sides called alternately -> one list of times per side"""
        for _ in range(warmup):
            for f in sides:
                f()
        torch.cuda.synchronize()
        times = [[] for _ in sides]
        for _ in range(iters):
            for ts, f in zip(times, sides):
                ts.append(timed(f))
        return times

    hip_fb(mixed)(), hip_fb(f32)()
    diff = max(float((p.grad - f32.model.params[k].grad).abs().max() / f32.model.params[k].grad.abs().max()) for k, p in mixed.model.params.items())
    _lib.lib().glowtts_launch_log_reset()
    hip_fb(mixed)()
    launches = int(_lib.lib().glowtts_launch_count(b"hifigan_"))
    fb_m, fb_f, fb_b = rounds([hip_fb(mixed), hip_fb(f32), base_fb], args.warmup, args.iters)
    st_m, st_f, st_b = rounds([lambda: mixed.Train_Step(mel, target), lambda: f32.Train_Step(mel, target), base_step], args.warmup, args.iters)
    aa_1, aa_2 = rounds([hip_fb(f32), hip_fb(f32_twin)], args.warmup, args.iters)

    # the weight-gradient launches alone, at the step's shapes (the values do not matter to the time), in both modes
    ln = f32.model._lengths(lengths, B, L)
    rnd = lambda *shape: torch.randn(*shape, device=dev)
    jobs, work_floats = [], 0
    for name, ci, co, taps, dil, rate, mult in hifigan_convs(geo):
        x = mel if name == "conv_pre" else rnd(B, L * mult, ci)
        dy = rnd(B, L * mult * max(rate, 1)) if co == 1 else rnd(B, L * mult * max(rate, 1), co)
        dw, db = torch.empty_like(f32.model.params[name + ".weight"]), torch.empty_like(f32.model.params[name + ".bias"])
        slope = 1.0 if name == "conv_pre" else (HIFIGAN_LAST_SLOPE if name == "conv_post" else HIFIGAN_SLOPE)
        jobs.append((x, dy, dw, db, mult, taps, dict(dilation=dil, rate=rate, slope=slope, channels_first=name == "conv_pre")))
        work_floats = max(work_floats, ops.hifigan_wgrad_work_floats(B, L, mult, ci, co, taps, rate))
    work = torch.empty(work_floats, device=dev)

    def wgrads(op):
        def run():
            for x, dy, dw, db, mult, taps, kw in jobs:
                op(x, dy, ln, work, dw, db, L, mult, taps, **kw)
        return run

    wg_m, wg_f = rounds([wgrads(ops.hifigan_wgrad_bf16), wgrads(ops.hifigan_wgrad)], args.warmup, args.iters)

    # the image build: the one pack launch against the torch ops of the f32 mode
    w_m, w_f = ({k: p.detach() for k, p in tr.model.params.items()} for tr in (mixed, f32))
    pk_m, pk_f = rounds([lambda: mixed.model._build_images(w_m), lambda: f32.model._build_images(w_f)], args.warmup, args.iters)

    macs = macs_per_frame(geo)
    flop = 2.0 * (3 * macs - geo["A"] * geo["C0"] * 7) * B * L
    floats = hbm_floats_per_frame(geo)
    floor_ms = floats * 4.0 * B * L / (HBM_TBS * 1e12) * 1e3
    med = statistics.median
    side = lambda ts: {"ms": round(med(ts), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)]}
    three = lambda m, f, b: {"mixed": side(m), "f32_hip": side(f), "baseline_torch_autograd": side(b), "speedup_mixed_over_f32_hip": round(med(f) / med(m), 2),
                             "speedup_mixed_over_baseline": round(med(b) / med(m), 2), "mixed_faster_than_f32": bool(med(m) < med(f)),
                             "mixed_faster_than_torch": bool(med(m) < med(b))}
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup, "B": B, "frames": L,
           "geometry": {k: geo[k] for k in ("A", "hop", "C0", "rates", "kernels", "channels", "resblock", "rk", "rd")},
           "launches_forward_backward_mixed": launches, "launch_plan_mixed": hifigan_train_launches(geo, "mixed"), "step_tflop": round(flop / 1e12, 3),
           "gradient_max_diff_mixed_vs_f32_hip_rel": diff,
           "forward_backward": three(fb_m, fb_f, fb_b), "train_step": three(st_m, st_f, st_b),
           "f32_against_f32": {"first": side(aa_1), "twin": side(aa_2), "ratio_of_medians": round(med(aa_2) / med(aa_1), 3)},
           "weight_gradient_launches": {"mixed": side(wg_m), "f32_hip": side(wg_f), "speedup_mixed_over_f32_hip": round(med(wg_f) / med(wg_m), 2),
                                        "share_of_mixed_train_step": round(med(wg_m) / med(st_m), 3)},
           "image_build": {"pack_images_launch": side(pk_m), "torch_image_build_f32_mode": side(pk_f)},
           "hbm": {"floats_per_frame": floats, "peak_tbytes_per_s": HBM_TBS, "floor_ms": round(floor_ms, 3),
                   "floor_over_mixed_forward_backward": round(floor_ms / med(fb_m), 3)}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
