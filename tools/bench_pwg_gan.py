"""One adversarial training step of the Parallel WaveGAN vocoder (csrc/pwg_ops.hip, csrc/pwg_train_ops.hip, csrc/stft_loss_ops.hip, csrc/pwg_disc_ops.hip) on
one MI355X at the defaults: B = 8 x 100 frames, hop 256, the 30-layer generator, the 10-layer 64-channel discriminator.  A step here is: generator forward,
multi-resolution STFT loss, ONE discriminator forward on the 2 B rows [target; wav], the generator's backward under L_stft + 4 L_adv (the discriminator's data
chain over the fake rows, frozen) and the discriminator's backward under L_D; no optimizer.
  * ms per step of the HIP path (`ParallelWaveGAN.generate`, `MultiResolutionSTFTLoss`, `PWGDiscriminator.score_pair`, `adversarial_mse`);
  * the BASELINE: the same step on torch.nn.functional.conv1d under autograd plus `torch.stft`, on the same device, weights and noise (the discriminator
    scores wav with detached weights for the generator term and [target; wav.detach()] for L_D, the way autograd code writes it); the two paths ALTERNATE
    call by call, so that a drifting clock meets both; median of `--iters` (>= 20) each;
  * the losses of both paths and the largest relative difference of the discriminator's parameter gradients (both paths are float32);
  * the discriminator's launches of a step alone - forward on 2 B rows, the frozen data chain on B rows, the full backward on 2 B rows - against the
    155 TF/s the exact-f32 MFMA sustains: 8 middle layers x 2 x 192 x 64 = 197 kFLOP per sample forward, as much again for the data gradient and for the
    weight gradient (the first and the last layer are not counted).
Usage: python tools/bench_pwg_gan.py [--iters 20] [--out profiles/bench_pwg_gan.json]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
from bench_pwg import PEAK_TFLOPS, random_weights, torch_generator  # noqa: E402
from bench_pwg_train import B, FRAMES, timed, torch_stft_loss  # noqa: E402

LAMBDA = 4.0


def torch_discriminator(w, geo, wav):
    x = wav.unsqueeze(1)
    for i, d in enumerate(geo["dilations"]):
        x = F.conv1d(x, w[f"conv_layers.{i}.weight"], w[f"conv_layers.{i}.bias"], padding=d, dilation=d)
        if i < geo["layers"] - 1:
            x = F.leaky_relu(x, geo["slope"])
    return x.squeeze(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_pwg_gan.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_pwg_gan.py measures on the GPU"
    from glow_tts_amd import vocoder as V
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    d = load_yaml(DEFAULT_YAML)
    d["Vocoder"] = dict(V.PWG_DEFAULTS)
    hp = Recursive_Parse(d)
    geo, dgeo = V.pwg_geometry(hp), V.pwg_disc_geometry(hp)
    sd = random_weights(V.pwg_expected_shapes(geo), 1234)
    dsd = {k: v * 3.0 for k, v in V.pwg_disc_init(dgeo, 1234).items()}
    voc = V.ParallelWaveGAN(hp, "cuda:0", state_dict=sd, trainable=True)
    disc = V.PWGDiscriminator(hp, "cuda:0", state_dict=dsd)
    crit = V.MultiResolutionSTFTLoss(None, "cuda:0")
    dev, T = voc.device, FRAMES * geo["hop"]
    g = torch.Generator().manual_seed(5)
    mels = (torch.rand(B, geo["A"], FRAMES, generator=g) * 8.0 - 4.0).to(dev)
    z, target = torch.randn(B, T, generator=g).to(dev), (torch.randn(B, T, generator=g) * 0.3).to(dev)
    lengths = torch.full((B,), FRAMES, dtype=torch.int32, device=dev)
    w_base = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}
    dw_base = {k: v.to(dev).requires_grad_(True) for k, v in dsd.items()}

    def hip():
        for p in list(voc.params.values()) + list(disc.params.values()):
            p.grad = None
        wav = voc.generate(mels, lengths, noises=z)[0]
        stft = crit(wav, target)
        both, p_fake = disc.score_pair(target, wav)
        adv, _ = V.adversarial_mse(p_fake, 1.0, LAMBDA)
        d_loss, _ = V.adversarial_mse(both, (1.0, 0.0))
        (stft + adv).backward()
        d_loss.backward()
        return (stft + adv).detach(), d_loss.detach()

    def base():
        for p in list(w_base.values()) + list(dw_base.values()):
            p.grad = None
        wav = torch_generator(w_base, geo, mels, z)
        stft = torch_stft_loss(wav, target, crit.resolutions)
        p_fake = torch_discriminator({k: v.detach() for k, v in dw_base.items()}, dgeo, wav)
        loss = stft + LAMBDA * ((p_fake - 1.0) ** 2).mean()
        p = torch_discriminator(dw_base, dgeo, torch.cat([target, wav.detach()]))
        d_loss = ((p[:B] - 1.0) ** 2).mean() + (p[B:] ** 2).mean()
        loss.backward()
        d_loss.backward()
        return loss.detach(), d_loss.detach()

    for _ in range(args.warmup):
        l_hip, l_base = hip(), base()
    torch.cuda.synchronize()
    diff = max(float((disc.params[k].grad - dw_base[k].grad).abs().max() / dw_base[k].grad.abs().max().clamp_min(1e-30)) for k in dsd)
    th, tb = [], []
    for _ in range(args.iters):                                     # alternating call by call
        th.append(timed(hip)[0])
        tb.append(timed(base)[0])
    hip_ms, base_ms = statistics.median(th), statistics.median(tb)

    # the discriminator's launches of a step alone
    with torch.no_grad():
        wav = voc(mels, lengths, noises=z)[0]
    both = torch.cat([target, wav]).contiguous()
    ds2, ds1 = torch.randn(2 * B, T, device=dev), torch.randn(B, T, device=dev)

    def launches():
        fwd = V.pwg_disc_forward(disc, both)
        half = {"wav": both[B:], "scores": fwd["scores"][B:], "keep": [k[B:] for k in fwd["keep"]]}
        V.pwg_disc_backward(disc, half, ds1, freeze=True)
        V.pwg_disc_backward(disc, fwd, ds2)

    for _ in range(2):
        launches()
    torch.cuda.synchronize()
    d_ms = statistics.median([timed(launches)[0] for _ in range(args.iters)])
    per_sample = (dgeo["layers"] - 2) * 2.0 * 3 * dgeo["C"] * dgeo["C"]
    flop = per_sample * T * (2 * B + B + 2 * 2 * B)                 # forward on 2 B rows, data chain on B, data chain + weight gradients on 2 B
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup, "B": B, "frames": FRAMES,
           "samples_per_row": T, "lambda_adversarial": LAMBDA, "generator": {k: geo[k] for k in ("layers", "stacks", "R", "G", "S", "A", "hop")},
           "discriminator": {"layers": dgeo["layers"], "channels": dgeo["C"], "negative_slope": dgeo["slope"]}, "stft_resolutions": crit.resolutions,
           "f32_mfma_peak_tflops": PEAK_TFLOPS, "loss_g_hip": float(l_hip[0]), "loss_g_baseline": float(l_base[0]), "loss_d_hip": float(l_hip[1]),
           "loss_d_baseline": float(l_base[1]), "discriminator_gradient_max_diff_rel": diff,
           "hip": {"ms_per_step": round(hip_ms, 3), "ms_min_max": [round(min(th), 3), round(max(th), 3)]},
           "baseline_torch": {"ms_per_step": round(base_ms, 3), "ms_min_max": [round(min(tb), 3), round(max(tb), 3)]},
           "speedup_hip_over_baseline": round(base_ms / hip_ms, 2), "hip_faster": bool(hip_ms < base_ms),
           "discriminator_launches": {"ms": round(d_ms, 3), "kflop_per_sample_forward": round(per_sample / 1e3, 1), "tflop": round(flop / 1e12, 3),
                                      "tflops": round(flop / (d_ms * 1e-3) / 1e12, 2),
                                      "fraction_of_f32_mfma_peak": round(flop / (d_ms * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
                                      "floor_ms_at_peak": round(flop / (PEAK_TFLOPS * 1e12) * 1e3, 2)}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
