"""The adversarial step of the HiFi-GAN trainer (glow_tts_amd/hifigan_trainer.py with `Vocoder.Train.Adversarial`; csrc/hifigan_disc_ops.hip) on one MI355X
at the defaults: the V1 generator, 16 segments of 32 frames, the default multi-period discriminator.  Three measurements; the first two against the BASELINE -
the same networks on torch.nn.functional.conv1d / conv_transpose1d / conv2d / leaky_relu under autograd in f32 on the same device and weights - called
ALTERNATELY, so that a drifting clock meets both:
  * the whole adversarial `Train_Step` (generator, multi-resolution STFT loss, one discriminator forward over [target; wav], L_G and L_D, both backwards, both
    clippings and RAdams); the baseline's step is the torch generator and the torch discriminator under the same loss, clipping and optimizer objects' kind;
  * the discriminator's launches alone: `score_pair` on a fixed fake waveform, L_G's adversarial and feature-matching terms, L_D and both backwards;
  * the weight-gradient launches alone: all `hifigan_disc_wgrad` + `hifigan_disc_wgrad_sum` pairs of L_D's backward replayed at the step's shapes (2 B rows),
    over the step's time.
The arithmetic is counted from the layer sizes: the generator's as tools/bench_hifigan_train.py counts it; the discriminator's forward, data gradients and
weight gradients over the 2 B rows and the frozen data chain over the B fake rows (the first layer has no data gradient worth counting; the zero taps of the
strided data gradients are not counted).  The fraction of the 155 TF/s this project uses for the exact-f32 MFMA is a whole-call rate, not a kernel's share of
peak.  There is no target ratio: the figures are printed as they fall.  Medians of `--iters` (>= 20) timed calls per side after `--warmup`, each a host clock
around a call that ends in a device synchronise.
Usage: python tools/bench_hifigan_gan.py [--iters 20] [--out profiles/bench_hifigan_gan.json]"""
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

from bench_hifigan import PEAK_TFLOPS, macs_per_frame, timed, torch_generator  # noqa: E402
from bench_hifigan_train import alternate, write_corpus  # noqa: E402


def forward_macs(geo, T):
    """multiply-accumulates of one discriminator forward per waveform row, summed over the periods"""
    from glow_tts_amd.vocoder import MPD_POST_TAPS, MPD_TAPS, hifigan_disc_rows
    total = 0
    for p in geo["periods"]:
        H, cin = hifigan_disc_rows(geo, T, p), 1
        for j, c in enumerate(geo["channels"]):
            total, cin = total + H[j + 1] * p * MPD_TAPS * cin * c, c
        total += H[-1] * p * MPD_POST_TAPS * cin
    return total


def torch_scores(params, geo, x):
    """the same networks on F.conv2d -> [(scores, maps)] per period"""
    out, n = [], len(geo["channels"])
    for i, p in enumerate(geo["periods"]):
        B, T = x.shape
        h = F.pad(x[:, None], (0, p - T % p), mode="reflect")[:, 0] if T % p else x
        h, maps = h.view(B, 1, -1, p), []
        for j in range(n):
            h = F.leaky_relu(F.conv2d(h, params[f"discriminators.{i}.convs.{j}.weight"], params[f"discriminators.{i}.convs.{j}.bias"],
                                      stride=(3 if j < n - 1 else 1, 1), padding=(2, 0)), geo["slope"])
            maps.append(h)
        h = F.conv2d(h, params[f"discriminators.{i}.conv_post.weight"], params[f"discriminators.{i}.conv_post.bias"], padding=(1, 0))
        maps.append(h)
        out.append((h.flatten(1), maps))
    return out


def torch_losses(dparams, geo, real, fake, lam_adv, lam_fm):
    """-> (the generator's adversarial + feature-matching term, L_D) of the baseline: one forward over [real; fake] with the fake rows attached for the
    generator term (parameters constant) and detached for L_D"""
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_hifigan_gan.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_hifigan_gan.py measures on the GPU"
    from glow_tts_amd import _lib, optim
    from glow_tts_amd.hifigan_trainer import HiFiGAN_Trainer
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.vocoder import HIFIGAN_DEFAULTS, MPD_POST_TAPS, MPD_TAPS, adversarial_mse, hifigan_disc_rows, hifigan_disc_work
    with tempfile.TemporaryDirectory() as root:
        d = load_yaml(DEFAULT_YAML)
        d["Vocoder"] = dict(HIFIGAN_DEFAULTS, Train={"Checkpoint_Path": os.path.join(root, "ckpt"), "Adversarial": {}})
        d["Train"]["Train_Pattern"].update(Path=root, Metadata_File="METADATA.PICKLE")
        d["Train"]["Eval_Pattern"].update(Path="", Metadata_File="METADATA.PICKLE")
        write_corpus(root, d["Sound"]["Mel_Dim"], d["Sound"]["Frame_Shift"], 32)
        tr = HiFiGAN_Trainer(hp=Recursive_Parse(d), seed=0)
        mel, target = (t.to(tr.device).contiguous() for t in tr.sampler["Train"].batch(0))
    assert tr.adversarial(0), "the default Start_Step is 0: every step is adversarial"
    voc, disc, geo, dgeo, s, a = tr.model, tr.discriminator, tr.model.geo, tr.discriminator.geo, tr.set, tr.disc_set
    lam_adv, lam_fm = float(a["Lambda_Adversarial"]), float(a["Lambda_Feature_Matching"])
    B, _, L = mel.shape
    T = L * geo["hop"]
    base_g = {k: p.detach().clone().requires_grad_(True) for k, p in voc.params.items()}
    base_d = {k: p.detach().clone().requires_grad_(True) for k, p in disc.params.items()}
    base_opt = optim.RAdam(list(base_g.values()), lr=float(s["Learning_Rate"]), eps=float(s["Epsilon"]))
    base_dopt = optim.RAdam(list(base_d.values()), lr=float(a["Learning_Rate"]), eps=float(a["Epsilon"]))
    fake = (torch.randn(B, T, generator=torch.Generator().manual_seed(1)) * 0.3).to(tr.device)

    def zero(params):
        for p in params:
            p.grad = None

    def base_step():
        zero(list(base_g.values()) + list(base_d.values()))
        wav = torch_generator(base_g, geo, mel)
        term, d_loss = torch_losses(base_d, dgeo, target, wav, lam_adv, lam_fm)
        (tr.criterion(wav, target) + term).backward()
        d_loss.backward()
        optim.clip_grad_norm_(list(base_g.values()), float(s["Gradient_Norm"]), _table_key=("bench_gan_base", 0))
        optim.clip_grad_norm_(list(base_d.values()), float(a["Gradient_Norm"]), _table_key=("bench_gan_base", 1))
        base_opt.step()
        base_dopt.step()

    def hip_disc():
        zero(tr.disc_params)
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
        term, d_loss = torch_losses(base_d, dgeo, target, x, lam_adv, lam_fm)
        term.backward()
        d_loss.backward()
        return term.detach(), d_loss.detach(), x.grad

    h, t = hip_disc(), base_disc()                                          # the same weights on both sides: before any step
    agree = {"generator_term": abs(float(h[0]) - float(t[0])) / abs(float(t[0])), "L_D": abs(float(h[1]) - float(t[1])) / abs(float(t[1])),
             "d_fake": float((h[2] - t[2]).abs().max() / t[2].abs().max()),
             "discriminator_gradients": max(float((p.grad - base_d[k].grad).abs().max() / base_d[k].grad.abs().max()) for k, p in disc.params.items())}
    _lib.lib().glowtts_launch_log_reset()
    hip_disc()
    launches = int(_lib.lib().glowtts_launch_count(b"hifigan_disc_"))
    di_h, di_b = alternate(hip_disc, base_disc, args.warmup, args.iters)
    st_h, st_b = alternate(lambda: tr.Train_Step(mel, target), base_step, args.warmup, args.iters)

    # the weight-gradient launches of L_D's backward alone, at the step's shapes: 2 B rows (the values do not matter to the time)
    lib, P, st, B2 = _lib.api(), _lib.ptr, _lib.stream(), 2 * B
    rnd = lambda *shape: torch.randn(*shape, device=tr.device)
    work, jobs = hifigan_disc_work(disc, B2, T, tr.device), []
    for i, p in enumerate(dgeo["periods"]):
        H, cin, x = hifigan_disc_rows(dgeo, T, p), 1, rnd(B2, T)
        for j, (c, stride) in enumerate(zip(dgeo["channels"], dgeo["strides"])):
            dy = rnd(B2, H[j + 1] * p, c)
            jobs.append((x, dy, torch.empty(c, cin, MPD_TAPS, 1, device=tr.device), torch.empty(c, device=tr.device), H[j], p, stride, cin, c, MPD_TAPS,
                         T if j == 0 else 0, 1.0 if j == 0 else dgeo["slope"]))
            x, cin = dy, c
        jobs.append((x, rnd(B2, H[-1] * p), torch.empty(1, cin, MPD_POST_TAPS, 1, device=tr.device), torch.empty(1, device=tr.device), H[-1], p, 1, cin, 1,
                     MPD_POST_TAPS, 0, dgeo["slope"]))

    def wgrads():
        for x, dy, dw, db, h_in, p, stride, cin, cout, taps, samples, slope in jobs:
            lib.glowtts_hifigan_disc_wgrad(P(x), P(dy), P(work), P(dw), P(db), B2, h_in, p, stride, cin, cout, taps, samples, slope, st)

    for _ in range(args.warmup):
        wgrads()
    torch.cuda.synchronize()
    wg = [timed(wgrads) for _ in range(args.iters)]

    dmacs = forward_macs(dgeo, T)
    gmacs, pre = macs_per_frame(geo), geo["A"] * geo["C0"] * 7
    disc_flop = 2.0 * dmacs * (3 * B2 + B)                                  # forward, data and weight gradients over 2 B rows; the frozen chain over B
    step_flop = disc_flop + 2.0 * (3 * gmacs - pre) * B * L
    med = statistics.median
    side = lambda ts: {"ms": round(med(ts), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)]}
    rate = lambda flop, ts: round(flop / (med(ts) * 1e-3) / 1e12 / PEAK_TFLOPS, 3)
    pair = lambda hs, bs, flop: {"hip": side(hs), "baseline_torch_autograd": side(bs), "hip_over_baseline_time": round(med(hs) / med(bs), 2),
                                 "hip_faster": bool(med(hs) < med(bs)), "hip_fraction_of_f32_mfma_peak": rate(flop, hs)}
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "B": B, "frames": L, "samples": T,
           "generator": {k: geo[k] for k in ("C0", "rates", "kernels", "resblock", "rk", "rd")}, "periods": dgeo["periods"], "channels": dgeo["channels"],
           "lambda_adversarial": lam_adv, "lambda_feature_matching": lam_fm, "f32_mfma_peak_tflops": PEAK_TFLOPS,
           "discriminator_forward_gmacs_per_row": round(dmacs * 1e-9, 3), "discriminator_tflop": round(disc_flop / 1e12, 3), "step_tflop": round(step_flop / 1e12, 3),
           "discriminator_launches": launches, "max_rel_diff_hip_vs_baseline": agree,
           "adversarial_train_step": pair(st_h, st_b, step_flop), "discriminator_alone": pair(di_h, di_b, disc_flop),
           "weight_gradient_launches": dict(side(wg), pairs=len(jobs), share_of_train_step=round(med(wg) / med(st_h), 3),
                                            share_of_discriminator_alone=round(med(wg) / med(di_h), 3))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
