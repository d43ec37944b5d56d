"""sha256 digests of what the HiFi-GAN kernels compute (csrc/hifigan_ops.hip, hifigan_train_ops.hip, hifigan_disc_ops.hip), for comparing two builds bit for
bit: a refactor of the kernels must leave every digest as it was.  Prints one JSON object, name -> sha256 of the tensor's raw bytes after a device synchronise.
  * generator: the configs NARROW, ODD and DEFAULT of tests/hifigan_ref.py with the tests' seeded weights, mels of the ragged lengths [5, 2, 7]: the waveform
    of `HiFiGAN.__call__`, and with `trainable=True` the waveform of `generate` and every parameter gradient under a seeded d wav;
  * discriminator: five cases of tests/test_gpu_hifigan_disc.py (c64_80 is defined here as well, so that a checkout without it runs it too) with that file's
    seeded weights and waveforms: from `score` and its backward the scores, every kept pre-activation, d wav and every parameter gradient; from `score_pair`
    the fake waveform's gradient under sum_p adversarial_mse(p_fake, 1) + 2 L_fm, and the parameter gradients of L_D.
Not a test: there is no reference in it.  Usage: python tools/hifigan_digest.py [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))
import torch  # noqa: E402

import hifigan_ref as H  # noqa: E402
import test_gpu_hifigan as G  # noqa: E402
import test_gpu_hifigan_disc as D  # noqa: E402

DISC_CASES = ["narrow_b3", "rows65", "splits", "default_p11", "c64_80"]
D.CASES.setdefault("c64_80", ([3], [64, 64, 80], 2, 200))


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def generator(out):
    from glow_tts_amd.vocoder import HiFiGAN
    for name in ("narrow", "odd", "default"):
        cfg = G.CFGS[name]
        mel, lengths = G.pad_mels([H.uniform_mel(cfg["A"], L, 10 + L) for L in G.RAGGED])
        out[f"generator {name} wav"] = sha(G.voc(name)(mel, lengths)[0])
        v = HiFiGAN(G._hp(cfg), "cuda:0", state_dict={"generator": G.sd_of(name)}, trainable=True)
        wav, _ = v.generate(mel, lengths)
        wav.backward(torch.randn(wav.shape, generator=torch.Generator().manual_seed(7)).cuda())
        out[f"generator {name} train wav"] = sha(wav)
        for k, p in v.params.items():
            out[f"generator {name} d {k}"] = sha(p.grad)


def discriminator(out):
    from glow_tts_amd.vocoder import adversarial_mse, hifigan_disc_forward
    for case in DISC_CASES:
        _, _, B, T = D.CASES[case]
        disc, wav = D.build(case)
        got = D.step(disc, wav)
        for i, per in enumerate(hifigan_disc_forward(disc, wav)["periods"]):
            out[f"disc {case} scores[{i}]"] = sha(got["scores"][i])
            assert torch.equal(per["scores"], got["scores"][i])
            for j, k in enumerate(per["keep"]):
                out[f"disc {case} keep[{i}][{j}]"] = sha(k)
        out[f"disc {case} dwav"] = sha(got["dwav"])
        for k, g in got["grads"].items():
            out[f"disc {case} d {k}"] = sha(g)
        for p in disc.params.values():
            p.grad = None
        fake = (torch.randn(B, T, generator=torch.Generator().manual_seed(21)) * D.AMPLITUDE).float().cuda().requires_grad_(True)
        both, p_fake, l_fm, _ = disc.score_pair(wav, fake)
        (sum(adversarial_mse(p, 1.0)[0] for p in p_fake) + 2.0 * l_fm).backward()
        out[f"disc {case} pair dfake"] = sha(fake.grad)
        sum(adversarial_mse(b, (1.0, 0.0))[0] for b in both).backward()
        for k, p in disc.params.items():
            out[f"disc {case} L_D d {k}"] = sha(p.grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hifigan_digest.py runs the kernels: it needs the GPU"
    out = {}
    generator(out)
    discriminator(out)
    text = json.dumps(out, indent=0, sort_keys=True)
    print(text)
    print(f"{len(out)} digests", file=sys.stderr)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
