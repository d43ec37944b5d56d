"""Training the HiFi-GAN generator (glow_tts_amd/vocoder.py: HiFiGAN(trainable=True), csrc/hifigan_train_ops.hip, glow_tts_amd/hifigan_trainer.py) on one
MI355X at the V1 sizes and the trainer's default batch (16 segments of 32 frames).  Two measurements, each against the BASELINE - the same generator written
with torch.nn.functional.conv1d / conv_transpose1d / leaky_relu (tools/bench_hifigan.py: `torch_generator`) under autograd in f32 on the same device and
weights - called ALTERNATELY, so that a drifting clock meets both:
  * forward + backward of the generator under a fixed d wav;
  * the whole `Train_Step` (generator, multi-resolution STFT loss, clipping, RAdam); the baseline's step is the torch generator under the same loss, clipping
    and optimizer objects' kind.
Also: the arithmetic of a step from the shapes (forward, data gradients - conv_pre has none - and weight gradients; the zero taps of the transposed
convolutions' data gradients are not counted), its share of the 155 TF/s this project uses for the exact-f32 MFMA, and the share of the step that the
weight-gradient launches take (all 78 `hifigan_wgrad` + `hifigan_wgrad_sum` pairs replayed alone at the step's shapes, over the step's time).
There is no target ratio: the figures are printed as they fall.  Medians of `--iters` (>= 20) timed calls per side after `--warmup`, each a host clock around a
call that ends in a device synchronise.
Usage: python tools/bench_hifigan_train.py [--iters 20] [--out profiles/bench_hifigan_train.json]"""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from bench_hifigan import PEAK_TFLOPS, macs_per_frame, timed, torch_generator  # noqa: E402


def write_corpus(root, mel_dim, hop, frames, files=8):
    rng = np.random.default_rng(0)
    meta = {"File_List": [], "Mel_Length_Dict": {}, "Audio_Length_Dict": {}}
    for i in range(files):
        n, name = frames + 8 + i, "F{}.PICKLE".format(i)
        with open(os.path.join(root, name), "wb") as f:
            pickle.dump({"Audio": (rng.standard_normal(n * hop) * 0.3).astype(np.float32), "Mel": rng.uniform(-4, 4, (n, mel_dim)).astype(np.float32)}, f)
        meta["File_List"].append(name)
        meta["Mel_Length_Dict"][name], meta["Audio_Length_Dict"][name] = n, n * hop
    with open(os.path.join(root, "METADATA.PICKLE"), "wb") as f:
        pickle.dump(meta, f)


def alternate(a, b, warmup, iters):
    for _ in range(warmup):
        a(), b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(iters):
        ta.append(timed(a))
        tb.append(timed(b))
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_hifigan_train.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_hifigan_train.py measures on the GPU"
    from glow_tts_amd import _lib, ops, optim
    from glow_tts_amd.hifigan_trainer import HiFiGAN_Trainer
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.vocoder import HIFIGAN_DEFAULTS, HIFIGAN_LAST_SLOPE, HIFIGAN_SLOPE, hifigan_convs, hifigan_train_keep_floats
    with tempfile.TemporaryDirectory() as root:
        d = load_yaml(DEFAULT_YAML)
        d["Vocoder"] = dict(HIFIGAN_DEFAULTS, Train={"Checkpoint_Path": os.path.join(root, "ckpt")})
        d["Train"]["Train_Pattern"].update(Path=root, Metadata_File="METADATA.PICKLE")
        d["Train"]["Eval_Pattern"].update(Path="", Metadata_File="METADATA.PICKLE")
        write_corpus(root, d["Sound"]["Mel_Dim"], d["Sound"]["Frame_Shift"], 32)
        tr = HiFiGAN_Trainer(hp=Recursive_Parse(d), seed=0)
        mel, target = (t.to(tr.device).contiguous() for t in tr.sampler["Train"].batch(0))
    voc, geo, s = tr.model, tr.model.geo, tr.set
    B, _, L = mel.shape
    lengths = [L] * B
    base_w = {k: p.detach().clone().requires_grad_(True) for k, p in voc.params.items()}
    base_opt = optim.RAdam(list(base_w.values()), lr=float(s["Learning_Rate"]), eps=float(s["Epsilon"]))
    dwav = torch.randn(B, L * geo["hop"], generator=torch.Generator().manual_seed(1)).to(tr.device)

    def zero(params):
        for p in params:
            p.grad = None

    def hip_fb():
        zero(tr.params)
        voc.generate(mel, lengths)[0].backward(dwav)

    def base_fb():
        zero(base_w.values())
        torch_generator(base_w, geo, mel).backward(dwav)

    def base_step():
        zero(base_w.values())
        tr.criterion(torch_generator(base_w, geo, mel), target).backward()
        optim.clip_grad_norm_(list(base_w.values()), float(s["Gradient_Norm"]), _table_key=("bench_base", 0))
        base_opt.step()

    hip_fb(), base_fb()
    diff = max(float((p.grad - base_w[k].grad).abs().max() / base_w[k].grad.abs().max()) for k, p in voc.params.items())
    _lib.lib().glowtts_launch_log_reset()
    hip_fb()
    launches = int(_lib.lib().glowtts_launch_count(b"hifigan_"))
    fb_h, fb_b = alternate(hip_fb, base_fb, args.warmup, args.iters)
    st_h, st_b = alternate(lambda: tr.Train_Step(mel, target), base_step, args.warmup, args.iters)

    # the weight-gradient launches alone, at the step's shapes (the values do not matter to the time)
    ln = voc._lengths(lengths, B, L)
    rnd = lambda *shape: torch.randn(*shape, device=tr.device)
    jobs, work_floats = [], 0
    for name, ci, co, taps, dil, rate, mult in hifigan_convs(geo):
        x = mel if name == "conv_pre" else rnd(B, L * mult, ci)
        dy = rnd(B, L * mult * max(rate, 1)) if co == 1 else rnd(B, L * mult * max(rate, 1), co)
        dw, db = torch.empty_like(voc.params[name + ".weight"]), torch.empty_like(voc.params[name + ".bias"])
        slope = 1.0 if name == "conv_pre" else (HIFIGAN_LAST_SLOPE if name == "conv_post" else HIFIGAN_SLOPE)
        jobs.append((x, dy, dw, db, mult, taps, dict(dilation=dil, rate=rate, slope=slope, channels_first=name == "conv_pre")))
        work_floats = max(work_floats, ops.hifigan_wgrad_work_floats(B, L, mult, ci, co, taps, rate))
    work = torch.empty(work_floats, device=tr.device)

    def wgrads():
        for x, dy, dw, db, mult, taps, kw in jobs:
            ops.hifigan_wgrad(x, dy, ln, work, dw, db, L, mult, taps, **kw)

    for _ in range(args.warmup):
        wgrads()
    torch.cuda.synchronize()
    wg = [timed(wgrads) for _ in range(args.iters)]

    macs = macs_per_frame(geo)
    pre = geo["A"] * geo["C0"] * 7
    flop = 2.0 * (3 * macs - pre) * B * L
    med = statistics.median
    side = lambda ts: {"ms": round(med(ts), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)]}
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup, "B": B, "frames": L,
           "geometry": {k: geo[k] for k in ("A", "hop", "C0", "rates", "kernels", "channels", "resblock", "rk", "rd")},
           "kept_floats_per_frame": hifigan_train_keep_floats(geo), "launches_forward_backward": launches, "step_tflop": round(flop / 1e12, 3),
           "f32_mfma_peak_tflops": PEAK_TFLOPS, "gradient_max_diff_hip_vs_baseline_rel": diff,
           "forward_backward": {"hip": side(fb_h), "baseline_torch_autograd": side(fb_b), "speedup_hip_over_baseline": round(med(fb_b) / med(fb_h), 2),
                                "hip_faster": bool(med(fb_h) < med(fb_b)), "hip_tflops": round(flop / (med(fb_h) * 1e-3) / 1e12, 2),
                                "hip_fraction_of_f32_mfma_peak": round(flop / (med(fb_h) * 1e-3) / 1e12 / PEAK_TFLOPS, 3)},
           "train_step": {"hip": side(st_h), "baseline_torch_autograd": side(st_b), "speedup_hip_over_baseline": round(med(st_b) / med(st_h), 2),
                          "hip_faster": bool(med(st_h) < med(st_b)), "hip_fraction_of_f32_mfma_peak": round(flop / (med(st_h) * 1e-3) / 1e12 / PEAK_TFLOPS, 3)},
           "weight_gradient_launches": dict(side(wg), share_of_train_step=round(med(wg) / med(st_h), 3))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
