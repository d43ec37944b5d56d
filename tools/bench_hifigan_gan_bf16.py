"""The bf16 mode of the multi-period discriminator (`Vocoder.Train.Adversarial.Precision: 'bf16'`; csrc/hifigan_disc_bf16_ops.hip) against the unchanged f32
HIP discriminator and torch f32 autograd, in ONE run, at tools/bench_hifigan_gan.py's defaults: the V1 generator, 16 segments of 32 frames (8192 samples), the
default five periods and widths.  Every series is timed ALTERNATELY, call by call over all its sides, so that a drifting clock meets every side; medians of
`--iters` (>= 20) calls after `--warmup`, each a host clock around a call that ends in a device synchronise.
  * the discriminator's launches alone (`score_pair` on a fixed fake waveform, the generator term, L_D, both backwards): bf16, f32 (two instances, A and B:
    their ratio is the A/A spread), torch;
  * the whole adversarial `Train_Step` with the generator in f32 and in 'mixed', the discriminator in f32 and in bf16 (four trainers), and torch's f32 step;
  * the weight-gradient launch pairs of L_D's backward replayed alone at the step's shapes (2 B rows): the bf16 step's (bf16 for the middle layers, f32 for
    layer 0 and conv_post) against the f32 step's;
  * the image rebuild: the one pack launch of the bf16 mode against the f32 mode's permutes.
The yardstick is the f32 HIP path and torch IN THIS FILE; ratios, not milliseconds, compare across files.  No figure is a target.
Usage: python tools/bench_hifigan_gan_bf16.py [--iters 20] [--out profiles/bench_hifigan_gan_bf16.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from bench_hifigan import timed, torch_generator  # noqa: E402
from bench_hifigan_gan import torch_losses  # noqa: E402
from bench_hifigan_train import write_corpus  # noqa: E402


def rotate(fns, warmup, iters):
    """-> one series per callable, timed alternating call by call"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(iters):
        for ts, fn in zip(out, fns):
            ts.append(timed(fn))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_hifigan_gan_bf16.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_hifigan_gan_bf16.py measures on the GPU"
    from glow_tts_amd import _lib, ops, optim
    from glow_tts_amd.hifigan_trainer import HiFiGAN_Trainer
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.vocoder import (HIFIGAN_DEFAULTS, MPD_POST_TAPS, MPD_TAPS, HiFiGANPeriodDiscriminator, adversarial_mse, hifigan_disc_rows,
                                      hifigan_disc_work)
    trainers = {}
    with tempfile.TemporaryDirectory() as root:
        for gen in ("f32", "mixed"):
            for dp in ("f32", "bf16"):
                d = load_yaml(DEFAULT_YAML)
                train = {"Checkpoint_Path": os.path.join(root, "ckpt"), "Adversarial": {"Precision": dp} if dp == "bf16" else {}}
                if gen == "mixed":
                    train["Precision"] = "mixed"
                d["Vocoder"] = dict(HIFIGAN_DEFAULTS, Train=train)
                d["Train"]["Train_Pattern"].update(Path=root, Metadata_File="METADATA.PICKLE")
                d["Train"]["Eval_Pattern"].update(Path="", Metadata_File="METADATA.PICKLE")
                if not trainers:
                    write_corpus(root, d["Sound"]["Mel_Dim"], d["Sound"]["Frame_Shift"], 32)
                trainers[(gen, dp)] = HiFiGAN_Trainer(hp=Recursive_Parse(d), seed=0)
        tr = trainers[("f32", "f32")]
        mel, target = (t.to(tr.device).contiguous() for t in tr.sampler["Train"].batch(0))
        hp = tr.hp
    assert all(t.discriminator.precision == dp for (_, dp), t in trainers.items())
    geo, dgeo, s, a, dev = tr.model.geo, tr.discriminator.geo, tr.set, tr.disc_set, tr.device
    lam_adv, lam_fm = float(a["Lambda_Adversarial"]), float(a["Lambda_Feature_Matching"])
    B, _, L = mel.shape
    T = L * geo["hop"]
    sd = {k: p.detach().cpu().clone() for k, p in tr.discriminator.params.items()}                 # the same weights on every side: before any step
    discs = {name: HiFiGANPeriodDiscriminator(hp, dev, state_dict={"discriminator": sd}, precision=p)
             for name, p in (("bf16", "bf16"), ("f32_a", "f32"), ("f32_b", "f32"))}
    base_g = {k: p.detach().clone().requires_grad_(True) for k, p in tr.model.params.items()}
    base_d = {k: v.to(dev).clone().requires_grad_(True) for k, v in sd.items()}
    base_opt = optim.RAdam(list(base_g.values()), lr=float(s["Learning_Rate"]), eps=float(s["Epsilon"]))
    base_dopt = optim.RAdam(list(base_d.values()), lr=float(a["Learning_Rate"]), eps=float(a["Epsilon"]))
    fake = (torch.randn(B, T, generator=torch.Generator().manual_seed(1)) * 0.3).to(dev)

    def zero(params):
        for p in params:
            p.grad = None

    def base_step():
        zero(list(base_g.values()) + list(base_d.values()))
        wav = torch_generator(base_g, geo, mel)
        term, d_loss = torch_losses(base_d, dgeo, target, wav, lam_adv, lam_fm)
        (tr.criterion(wav, target) + term).backward()
        d_loss.backward()
        optim.clip_grad_norm_(list(base_g.values()), float(s["Gradient_Norm"]), _table_key=("bench_gan_bf16_base", 0))
        optim.clip_grad_norm_(list(base_d.values()), float(a["Gradient_Norm"]), _table_key=("bench_gan_bf16_base", 1))
        base_opt.step()
        base_dopt.step()

    def hip_disc(disc):
        def run():
            zero(disc.params.values())
            x = fake.clone().requires_grad_(True)
            both, p_fake, l_fm, _ = disc.score_pair(target, x)
            term = lam_adv * sum(adversarial_mse(p, 1.0)[0] for p in p_fake) + lam_fm * l_fm
            d_loss = sum(adversarial_mse(b, (1.0, 0.0))[0] for b in both)
            term.backward()
            d_loss.backward()
            return term.detach(), d_loss.detach(), x.grad
        return run

    def base_disc():
        zero(base_d.values())
        x = fake.clone().requires_grad_(True)
        term, d_loss = torch_losses(base_d, dgeo, target, x, lam_adv, lam_fm)
        term.backward()
        d_loss.backward()
        return term.detach(), d_loss.detach(), x.grad

    runs = {k: hip_disc(d) for k, d in discs.items()}
    t = base_disc()

    def agreement(name):
        h = runs[name]()
        return {"generator_term": abs(float(h[0]) - float(t[0])) / abs(float(t[0])), "L_D": abs(float(h[1]) - float(t[1])) / abs(float(t[1])),
                "d_fake": float((h[2] - t[2]).abs().max() / t[2].abs().max()),
                "discriminator_gradients": max(float((p.grad - base_d[k].grad).abs().max() / base_d[k].grad.abs().max()) for k, p in discs[name].params.items())}
    agree = {name: agreement(name) for name in ("bf16", "f32_a")}
    launches = {}
    for name in ("bf16", "f32_a"):
        _lib.lib().glowtts_launch_log_reset()
        runs[name]()
        launches[name] = {k: int(_lib.lib().glowtts_launch_count(k.encode())) for k in ("hifigan_disc_", "hifigan_disc_conv_bf16", "hifigan_disc_conv_bwd_bf16",
                                                                                        "hifigan_disc_wgrad_bf16", "hifigan_pack_images")}
    di = dict(zip(("bf16", "f32_a", "f32_b", "torch"), rotate([runs["bf16"], runs["f32_a"], runs["f32_b"], base_disc], args.warmup, args.iters)))
    keys = [("f32", "bf16"), ("f32", "f32"), ("mixed", "bf16"), ("mixed", "f32")]
    st = rotate([(lambda t_=trainers[k]: t_.Train_Step(mel, target)) for k in keys] + [base_step], args.warmup, args.iters)
    st = dict(zip([f"generator_{g}_discriminator_{p}" for g, p in keys] + ["torch"], st))

    # the weight-gradient launch pairs of L_D's backward alone, at the step's shapes: 2 B rows (the values do not matter to the time)
    lib, P, stream, B2 = _lib.api(), _lib.ptr, _lib.stream(), 2 * B
    rnd = lambda *shape: torch.randn(*shape, device=dev)
    work, jobs = hifigan_disc_work(discs["f32_a"], B2, T, dev), []
    for i, p in enumerate(dgeo["periods"]):
        H, cin, x = hifigan_disc_rows(dgeo, T, p), 1, rnd(B2, T)
        for j, (c, stride) in enumerate(zip(dgeo["channels"], dgeo["strides"])):
            dy = rnd(B2, H[j + 1] * p, c)
            jobs.append((x, dy, torch.empty(c, cin, MPD_TAPS, 1, device=dev), torch.empty(c, device=dev), H[j], p, stride, cin, c, MPD_TAPS, T if j == 0 else 0,
                         1.0 if j == 0 else dgeo["slope"]))
            x, cin = dy, c
        jobs.append((x, rnd(B2, H[-1] * p), torch.empty(1, cin, MPD_POST_TAPS, 1, device=dev), torch.empty(1, device=dev), H[-1], p, 1, cin, 1, MPD_POST_TAPS, 0,
                     dgeo["slope"]))

    def wgrads(bf16):
        def run():
            for x, dy, dw, db, h_in, p, stride, cin, cout, taps, samples, slope in jobs:
                if bf16 and cin > 1 and cout > 1:
                    ops.hifigan_disc_wgrad_bf16(x, dy, work, dw, db, h_in, p, stride, slope)
                else:
                    lib.glowtts_hifigan_disc_wgrad(P(x), P(dy), P(work), P(dw), P(db), B2, h_in, p, stride, cin, cout, taps, samples, slope, stream)
        return run
    wg = dict(zip(("bf16", "f32"), rotate([wgrads(True), wgrads(False)], args.warmup, args.iters)))
    rebuild = lambda d: (lambda: d._build_images({k: t_.detach() for k, t_ in d.params.items()}))
    pk = dict(zip(("bf16_pack_launch", "f32_permutes"), rotate([rebuild(discs["bf16"]), rebuild(discs["f32_a"])], args.warmup, args.iters)))

    med = statistics.median
    side = lambda ts: {"ms": round(med(ts), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)]}
    ratio = lambda x, y: round(med(x) / med(y), 3)
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "B": B, "frames": L, "samples": T, "periods": dgeo["periods"],
           "channels": dgeo["channels"], "lambda_adversarial": lam_adv, "lambda_feature_matching": lam_fm, "launches_of_the_discriminator_alone": launches,
           "max_rel_diff_vs_torch_f32": agree,
           "discriminator_alone": dict({k: side(v) for k, v in di.items()}, bf16_over_f32_time=ratio(di["bf16"], di["f32_a"]),
                                       f32_a_over_f32_b_time=ratio(di["f32_a"], di["f32_b"]), bf16_over_torch_time=ratio(di["bf16"], di["torch"]),
                                       f32_over_torch_time=ratio(di["f32_a"], di["torch"])),
           "adversarial_train_step": dict({k: side(v) for k, v in st.items()},
                                          bf16_over_f32_time_generator_f32=ratio(st["generator_f32_discriminator_bf16"], st["generator_f32_discriminator_f32"]),
                                          bf16_over_f32_time_generator_mixed=ratio(st["generator_mixed_discriminator_bf16"], st["generator_mixed_discriminator_f32"]),
                                          mixed_bf16_over_torch_time=ratio(st["generator_mixed_discriminator_bf16"], st["torch"]),
                                          f32_f32_over_torch_time=ratio(st["generator_f32_discriminator_f32"], st["torch"])),
           "weight_gradient_launches": dict({k: side(v) for k, v in wg.items()}, pairs=len(jobs), bf16_over_f32_time=ratio(wg["bf16"], wg["f32"])),
           "image_rebuild": dict({k: side(v) for k, v in pk.items()}, bf16_over_f32_time=ratio(pk["bf16_pack_launch"], pk["f32_permutes"]))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
