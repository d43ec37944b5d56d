"""The HiFi-GAN multi-scale discriminator (csrc/hifigan_msd_ops.hip; `Vocoder.Train.Adversarial.Multi_Scale`) on one MI355X at the defaults: 16 segments of
32 frames (8192 samples), the V1 generator, the default multi-period discriminator, three scales of the default widths.  By the method of
tools/bench_hifigan_gan.py - medians of `--iters` (>= 20) timed calls per side after `--warmup`, the two sides called ALTERNATELY, each call a host clock
around a call that ends in a device synchronise:
  * the multi-scale discriminator's launches alone: `score_pair` on a fixed fake waveform, L_G's adversarial and feature-matching terms, L_D and both
    backwards - against the BASELINE, the same networks on F.avg_pool1d / F.conv1d(groups=) / leaky_relu under autograd in f32 on the same device and weights;
    the baseline is also timed against ITSELF the same way (A/A), so that the spread of the method is on the page beside the ratio;
  * the whole adversarial `Train_Step` with and without the sub-block `Multi_Scale` (two trainers of the same seed, alternately);
  * the weight-gradient launches alone: every `hifigan_msd_wgrad`, `hifigan_msd_first_wgrad` and `hifigan_msd_dense_wgrad` pair of L_D's backward replayed at
    the step's shapes (2 B rows);
  * the launches of a step, by prefix.
The arithmetic is counted here from the layer table: multiply-accumulates of one forward per sample of a scale's own waveform (each layer's output rows x
taps x Cin / groups x Cout), then over the scales' lengths; forward, data and weight gradients over the 2 B rows and the frozen data chain over the B fake
rows (the first layer has no data gradient worth counting, the polyphase data gradient multiplies no zero row).  The fraction of the 155 TF/s this project
uses for the exact-f32 MFMA is a whole-call rate, not a kernel's share of peak.  There is no target ratio: the figures are printed as they fall.
Usage: python tools/bench_hifigan_msd.py [--iters 20] [--out profiles/bench_hifigan_msd.json]"""
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
import torch.nn.functional as F  # noqa: E402

from bench_hifigan import PEAK_TFLOPS, timed  # noqa: E402
from bench_hifigan_train import alternate, write_corpus  # noqa: E402

POST_TAPS = 3


def forward_macs(geo, T):
    """-> (multiply-accumulates of one forward per waveform row summed over the scales, the same of scale 0 alone per sample of the waveform)"""
    from glow_tts_amd.vocoder import hifigan_msd_rows
    per_scale = []
    for L in hifigan_msd_rows(geo, T):
        cin, total = 1, 0
        for j, (c, g, k) in enumerate(zip(geo["channels"], geo["groups"], geo["kernels"])):
            total, cin = total + L[j + 1] * k * (cin // g) * c, c
        per_scale.append(total + L[-1] * POST_TAPS * cin)
    return sum(per_scale), per_scale[0] / T


def torch_scores(params, geo, x):
    """the same networks on F.conv1d(groups=) -> [(scores, maps)] per scale"""
    out, h0 = [], x[:, None, :]
    for i in range(geo["scales"]):
        if i:
            h0 = F.avg_pool1d(h0, 4, 2, padding=2)
        h, maps = h0, []
        for j, (g, s, k) in enumerate(zip(geo["groups"], geo["strides"], geo["kernels"])):
            h = F.leaky_relu(F.conv1d(h, params[f"discriminators.{i}.convs.{j}.weight"], params[f"discriminators.{i}.convs.{j}.bias"], stride=s, padding=k // 2,
                                      groups=g), geo["slope"])
            maps.append(h)
        h = F.conv1d(h, params[f"discriminators.{i}.conv_post.weight"], params[f"discriminators.{i}.conv_post.bias"], padding=1)
        maps.append(h)
        out.append((h.flatten(1), maps))
    return out


def torch_losses(dparams, geo, real, fake, lam_adv, lam_fm):
    """-> (the generator's adversarial + feature-matching term, L_D) of the baseline, as tools/bench_hifigan_gan.py forms them"""
    B = real.shape[0]
    frozen = {k: v.detach() for k, v in dparams.items()}
    out_g = torch_scores(frozen, geo, torch.cat([real, fake]))
    fm = sum((m[:B].detach() - m[B:]).abs().mean() for _, maps in out_g for m in maps)
    term = lam_adv * sum(((s[B:] - 1) ** 2).mean() for s, _ in out_g) + lam_fm * fm
    out_d = torch_scores(dparams, geo, torch.cat([real, fake.detach()]))
    return term, sum(((s[:B] - 1) ** 2).mean() + (s[B:] ** 2).mean() for s, _ in out_d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_hifigan_msd.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_hifigan_msd.py measures on the GPU"
    from glow_tts_amd import _lib
    from glow_tts_amd.hifigan_trainer import HiFiGAN_Trainer
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.vocoder import HIFIGAN_DEFAULTS, MSD_LAST_TAPS, MSD_POST_TAPS, adversarial_mse, hifigan_msd_rows, hifigan_msd_work
    trainers = {}
    with tempfile.TemporaryDirectory() as root:
        write_corpus(root, load_yaml(DEFAULT_YAML)["Sound"]["Mel_Dim"], load_yaml(DEFAULT_YAML)["Sound"]["Frame_Shift"], 32)
        for name, adv in (("with", {"Multi_Scale": {}}), ("without", {})):
            d = load_yaml(DEFAULT_YAML)
            d["Vocoder"] = dict(HIFIGAN_DEFAULTS, Train={"Checkpoint_Path": os.path.join(root, "ckpt_" + name), "Adversarial": adv})
            d["Train"]["Train_Pattern"].update(Path=root, Metadata_File="METADATA.PICKLE")
            d["Train"]["Eval_Pattern"].update(Path="", Metadata_File="METADATA.PICKLE")
            trainers[name] = HiFiGAN_Trainer(hp=Recursive_Parse(d), seed=0)
        tr, plain = trainers["with"], trainers["without"]
        mel, target = (t.to(tr.device).contiguous() for t in tr.sampler["Train"].batch(0))
    assert tr.adversarial(0) and plain.adversarial(0), "the default Start_Step is 0: every step is adversarial"
    disc, geo, a = tr.discriminator.scales, tr.discriminator.scales.geo, tr.disc_set
    lam_adv, lam_fm = float(a["Lambda_Adversarial"]), float(a["Lambda_Feature_Matching"])
    B, _, L = mel.shape
    T = L * tr.model.geo["hop"]
    base_d = {k: p.detach().clone().requires_grad_(True) for k, p in disc.params.items()}
    fake = (torch.randn(B, T, generator=torch.Generator().manual_seed(1)) * 0.3).to(tr.device)

    def zero(params):
        for p in params:
            p.grad = None

    def hip_disc():
        zero(disc.params.values())
        x = fake.clone().requires_grad_(True)
        both, p_fake, l_fm, _ = disc.score_pair(target, x)
        term = lam_adv * sum(adversarial_mse(p, 1.0)[0] for p in p_fake) + lam_fm * l_fm
        d_loss = sum(adversarial_mse(b, (1.0, 0.0))[0] for b in both)
        term.backward()
        d_loss.backward()
        return term.detach(), d_loss.detach(), x.grad

    def base_disc():
        zero(base_d.values())
        x = fake.clone().requires_grad_(True)
        term, d_loss = torch_losses(base_d, geo, target, x, lam_adv, lam_fm)
        term.backward()
        d_loss.backward()
        return term.detach(), d_loss.detach(), x.grad

    h, t = hip_disc(), base_disc()                                          # the same weights on both sides: before any step
    agree = {"generator_term": abs(float(h[0]) - float(t[0])) / abs(float(t[0])), "L_D": abs(float(h[1]) - float(t[1])) / abs(float(t[1])),
             "d_fake": float((h[2] - t[2]).abs().max() / t[2].abs().max()),
             "discriminator_gradients": max(float((p.grad - base_d[k].grad).abs().max() / base_d[k].grad.abs().max()) for k, p in disc.params.items())}
    count = lambda prefix: int(_lib.lib().glowtts_launch_count(prefix))
    _lib.lib().glowtts_launch_log_reset()
    hip_disc()
    alone_launches = count(b"hifigan_msd_") + count(b"hifigan_disc_fm")
    di_h, di_b = alternate(hip_disc, base_disc, args.warmup, args.iters)
    aa_1, aa_2 = alternate(base_disc, base_disc, args.warmup, args.iters)
    launches = {}
    for name, trainer in trainers.items():
        trainer.Train_Step(mel, target)                                      # (the first step of a trainer builds its tables)
        _lib.lib().glowtts_launch_log_reset()
        trainer.Train_Step(mel, target)
        launches[name] = {"hifigan_msd_": count(b"hifigan_msd_"), "hifigan_disc_": count(b"hifigan_disc_")}
    st_w, st_p = alternate(lambda: tr.Train_Step(mel, target), lambda: plain.Train_Step(mel, target), args.warmup, args.iters)

    # the weight-gradient launches of L_D's backward alone, at the step's shapes: 2 B rows (the values do not matter to the time)
    lib, P, st, B2, dev = _lib.api(), _lib.ptr, _lib.stream(), 2 * B, tr.device
    rnd = lambda *shape: torch.randn(*shape, device=dev)
    ch, n = geo["channels"], len(geo["channels"])
    work, jobs = hifigan_msd_work(disc, B2, T, dev), []
    for Ls in hifigan_msd_rows(geo, T):
        x = rnd(B2, Ls[0])
        dy = rnd(B2, Ls[1], ch[0])
        jobs.append(("first", x, dy, torch.empty(ch[0], 1, geo["kernels"][0], device=dev), torch.empty(ch[0], device=dev), Ls[0], 0))
        for j in range(1, n - 1):
            x, dy = dy, rnd(B2, Ls[j + 1], ch[j])
            jobs.append(("grouped", x, dy, torch.empty(ch[j], ch[j - 1] // geo["groups"][j], geo["kernels"][j], device=dev), torch.empty(ch[j], device=dev), Ls[j], j))
        x, dy = dy, rnd(B2, Ls[n], ch[-1])
        jobs.append(("dense", x, dy, torch.empty(ch[-1], ch[-2], MSD_LAST_TAPS, device=dev), torch.empty(ch[-1], device=dev), Ls[n - 1], n - 1))
        jobs.append(("post", dy, rnd(B2, Ls[n]), torch.empty(1, ch[-1], MSD_POST_TAPS, device=dev), torch.empty(1, device=dev), Ls[n], n))

    def wgrads():
        for kind, x, dy, dw, db, rows, j in jobs:
            if kind == "first":
                lib.glowtts_hifigan_msd_first_wgrad(P(x), P(dy), P(work), P(dw), P(db), B2, rows, geo["kernels"][0], ch[0], st)
            elif kind == "grouped":
                lib.glowtts_hifigan_msd_wgrad(P(x), P(dy), P(work), P(dw), P(db), B2, rows, geo["kernels"][j], geo["strides"][j], geo["groups"][j], ch[j - 1], ch[j],
                                              geo["slope"], st)
            elif kind == "dense":
                lib.glowtts_hifigan_msd_dense_wgrad(P(x), P(dy), P(work), P(dw), P(db), B2, rows, ch[-2], ch[-1], MSD_LAST_TAPS, geo["slope"], st)
            else:
                lib.glowtts_hifigan_msd_dense_wgrad(P(x), P(dy), P(work), P(dw), P(db), B2, rows, ch[-1], 1, MSD_POST_TAPS, geo["slope"], st)

    for _ in range(args.warmup):
        wgrads()
    torch.cuda.synchronize()
    wg = [timed(wgrads) for _ in range(args.iters)]

    macs, macs_per_sample = forward_macs(geo, T)
    disc_flop = 2.0 * macs * (3 * B2 + B)                                   # forward, data and weight gradients over 2 B rows; the frozen chain over B
    med = statistics.median
    side = lambda ts: {"ms": round(med(ts), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)]}
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "B": B, "frames": L, "samples": T, "scales": geo["scales"],
           "channels": ch, "groups": geo["groups"], "strides": geo["strides"], "kernel_sizes": geo["kernels"], "periods": tr.discriminator.periods.geo["periods"],
           "lambda_adversarial": lam_adv, "lambda_feature_matching": lam_fm, "f32_mfma_peak_tflops": PEAK_TFLOPS,
           "forward_kmacs_per_sample_scale_0": round(macs_per_sample * 1e-3, 1), "forward_macs_all_scales_over_scale_0": round(macs / (macs_per_sample * T), 3),
           "forward_gmacs_per_row": round(macs * 1e-9, 3), "multi_scale_tflop": round(disc_flop / 1e12, 3), "max_rel_diff_hip_vs_baseline": agree,
           "multi_scale_alone": {"hip": side(di_h), "baseline_torch_autograd": side(di_b), "hip_over_baseline_time": round(med(di_h) / med(di_b), 2),
                                 "hip_faster": bool(med(di_h) < med(di_b)), "launches": alone_launches,
                                 "hip_fraction_of_f32_mfma_peak": round(disc_flop / (med(di_h) * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
                                 "baseline_against_itself": {"first": side(aa_1), "second": side(aa_2), "ratio_of_medians": round(med(aa_1) / med(aa_2), 3)}},
           "adversarial_train_step": {"with_multi_scale": side(st_w), "without_multi_scale": side(st_p), "with_over_without_time": round(med(st_w) / med(st_p), 2),
                                      "launches": launches},
           "weight_gradient_launches": dict(side(wg), pairs=len(jobs), share_of_multi_scale_alone=round(med(wg) / med(di_h), 3),
                                            share_of_train_step_with_multi_scale=round(med(wg) / med(st_w), 3))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
