"""GPU: `HiFiGAN_Trainer` with the yaml key `Vocoder.Train.Adversarial.Precision: 'bf16'` on the tiny configuration and with the helpers of
tests/test_gpu_hifigan_gan_trainer.py: two `Train_Step`s across Start_Step = 1.  The first is stage one and must be bit-identical to the f32 trainer's; the
second is adversarial and its discriminator links are replayed FROM THE DEVICE'S OWN STATE before it - the discriminator's parameters, the device's waveform
and the target - in the bf16 restatement (tests/hifigan_disc_bf16_ref.py), link by link under bar (b) of tests/hifigan_disc_bf16_cases.py: every period's
p_fake, the adversarial sum, L_fm and its terms, the discriminator's part of d wav, L_D with its two sums and every discriminator gradient; then the
discriminator's update (clipping, RAdam, step decay: f32 code the mode does not touch) fed with the device's gradients under the project's bar.  With
`Multi_Scale` also present the scale discriminator's launch classes are the f32 ones."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import hifigan_disc_bf16_cases as C  # noqa: E402
import hifigan_disc_bf16_ref as BR  # noqa: E402
import hifigan_disc_ref as HR  # noqa: E402
import test_gpu_hifigan_gan_trainer as GT  # noqa: E402
import test_gpu_hifigan_msd_trainer as MT  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402

pytestmark = pytest.mark.gpu
NEW = ("hifigan_disc_conv_bf16", "hifigan_disc_conv_bwd_bf16", "hifigan_disc_wgrad_bf16")
PERIODS, N, SLOPE = GT.PERIODS, len(GT.CHANNELS), GT.SLOPE


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("hifigan_disc_bf16_train"))
    for i, split in enumerate(("Train", "Eval")):
        GT.write_corpus(os.path.join(root, split), seed=i)
    return root


def hp_dict(root, precision="bf16", multi_scale=False, name="hifigan_bf16"):
    d = GT.hp_dict(root, name=name)
    if precision is not None:
        d["Vocoder"]["Train"]["Adversarial"]["Precision"] = precision
    if multi_scale:
        d["Vocoder"]["Train"]["Adversarial"]["Multi_Scale"] = copy.deepcopy(MT.MSD)
    return d


def test_two_steps_across_start_step_match_the_restatement(corpus):
    from glow_tts_amd.vocoder import HiFiGANPeriodDiscriminator, adversarial_mse
    tr = GT.trainer(hp_dict(corpus))
    plain = GT.trainer(hp_dict(corpus, precision=None, name="hifigan_bf16_plain"))
    assert isinstance(tr.discriminator, HiFiGANPeriodDiscriminator) and tr.discriminator.precision == "bf16" and plain.discriminator.precision == "f32"
    assert tr.disc_set["Precision"] == "bf16" and "Precision" not in plain.disc_set
    # step 1: stage one, the f32 trainer's bits; the discriminator is untouched
    mel, target = tr.sampler["Train"].batch(0)
    launch_reset()
    a, b = tr.Train_Step(mel, target), plain.Train_Step(mel, target)
    assert torch.equal(a, b) and all(torch.equal(v, GT.state_of(plain)[k]) for k, v in GT.state_of(tr).items())
    assert all(torch.equal(v, GT.dstate_of(plain)[k]) for k, v in GT.dstate_of(tr).items()) and not any("hifigan_disc" in k and c for k, c in launch_counts().items())
    # step 2: adversarial.  The links from the device's own state, through the trainer's own discriminator
    mel, target = tr.sampler["Train"].batch(1)
    dbefore, adv_set, dev = GT.dstate_of(tr), tr.disc_set, tr.device
    wav = tr.generate(mel.to(dev), [GT.FRAMES] * GT.BATCH, tr.steps).detach()
    lam_adv, lam_fm = float(adv_set["Lambda_Adversarial"]), float(adv_set["Lambda_Feature_Matching"])
    for p in tr.disc_params:
        p.grad = None
    x = wav.clone().requires_grad_(True)
    launch_reset()
    both, p_fake, l_fm, fm_terms = tr.discriminator.score_pair(target.to(dev), x)
    adv = [adversarial_mse(p, 1.0)[0] for p in p_fake]
    (lam_adv * sum(adv) + lam_fm * l_fm).backward()
    assert all(p.grad is None for p in tr.disc_params)
    d_terms = [adversarial_mse(s, (1.0, 0.0)) for s in both]
    d_loss = sum(t[0] for t in d_terms)
    d_loss.backward()
    torch.cuda.synchronize()
    counts = launch_counts()
    assert counts.get(NEW[0]) == len(PERIODS) * (N - 1) and counts.get(NEW[1]) == 2 * len(PERIODS) * (N - 1) and counts.get(NEW[2]) == len(PERIODS) * (N - 1), counts
    assert not counts.get("hifigan_disc_conv") and not counts.get("hifigan_disc_conv_bwd") and counts.get("hifigan_disc_wgrad") == 2 * len(PERIODS), counts
    got = {"adv": sum(adv).detach().reshape(1), "L_fm": l_fm.detach().reshape(1), "fm_terms": fm_terms, "d fake": x.grad, "L_D": d_loss.detach().reshape(1),
           "D_terms": torch.stack([sum(t[1][0] for t in d_terms), sum(t[1][1] for t in d_terms)]).detach()}
    got.update({f"p_fake[{i}]": p.detach() for i, p in enumerate(p_fake)})
    dgrads = {k: p.grad.detach().cpu().clone() for k, p in tr.discriminator.params.items()}
    got.update({"L_D " + k: g for k, g in dgrads.items()})
    # the very Train_Step: the same bits (everything is deterministic), so the links above ARE the step's
    launch_reset()
    tr.Train_Step(mel, target)
    counts = launch_counts()
    assert counts.get("hifigan_pack_images") == 1 and not counts.get("hifigan_disc_conv") and not counts.get("hifigan_disc_conv_bwd"), counts
    assert torch.equal(tr.last["L_adv"].reshape(1), got["adv"]) and torch.equal(tr.last["L_fm"].reshape(1), got["L_fm"])
    assert torch.equal(tr.last["Discriminator_Loss"].reshape(1), got["L_D"]) and torch.equal(tr.last["FM_Terms"], fm_terms)
    assert torch.equal(tr.last["Real_Term"], got["D_terms"][0]) and torch.equal(tr.last["Fake_Term"], got["D_terms"][1])
    dafter = GT.dstate_of(tr)
    # the replay: the contract in float64 (emu), the unrounded network in float64 and float32 (e_mix and the guard)
    tc, wc = target.cpu(), wav.cpu()

    def links(mod, dtype):
        g = mod.generator_term_grads(dbefore, tc, wc, PERIODS, N, SLOPE, lam_adv, lam_fm, dtype)
        p = mod.pair_grads(dbefore, tc, wc, PERIODS, N, SLOPE, dtype)
        scores = [s.detach() for s, _ in mod.forward({k: v.to(dtype) for k, v in dbefore.items()}, wc.to(dtype), PERIODS, N, SLOPE)]
        out = {"adv": g["adv_terms"].sum().reshape(1), "L_fm": g["l_fm"], "fm_terms": g["fm_terms"], "d fake": g["dfake"], "L_D": p["loss"],
               "D_terms": torch.stack([p["real_terms"].sum(), p["fake_terms"].sum()])}
        out.update({f"p_fake[{i}]": s for i, s in enumerate(scores)})
        out.update({"L_D " + k: v for k, v in p["grads"].items()})
        return out
    emu, r64, r32 = links(BR, torch.float64), links(HR, torch.float64), links(HR, torch.float32)
    assert set(got) == set(emu)
    failed, dropped = [], []
    for k in emu:
        assert tuple(got[k].shape) == tuple(emu[k].shape), k
        e_mix, e32 = C.dist(emu[k], r64[k]), C.dist(r32[k], r64[k])
        if not e_mix > C.GUARD * e32:
            dropped.append(k)
            continue
        b = C.dist(got[k].cpu(), emu[k]) / e_mix
        print(f"step 2 {k}: e_mix {e_mix:.3e}  e32 {e32:.3e}  |got - emu64| / e_mix {b:.5f} (bar {C.BAR_B:.5f})")
        if not b <= C.BAR_B:
            failed.append((k, b))
    print("dropped (e_mix <= 100 e32):", dropped)
    assert len(dropped) <= C.MAX_DROPPED * len(emu), dropped
    # the discriminator's update from the device's gradients: its first update
    dnames = list(tr.discriminator.params)
    du = {dt: GT.OptimizerReplay(dnames, tr.disc_set, dt).update(dbefore, dgrads) for dt in (torch.float64, torch.float32)}
    GT.check_updates(failed, "step 2 discriminator", dnames, dbefore, dafter, du[torch.float64][0], du[torch.float32][0])
    assert not failed, failed
    assert tr.steps == 2 and tr.disc_steps == 1
    # the checkpoint's keys and the discriminator's names are the f32 run's; the state resumes in either precision
    saved = torch.load(tr.Save_Checkpoint(), map_location="cpu")
    assert set(saved) == GT.SIX and list(saved["discriminator"]) == list(GT.dstate_of(plain))
    for precision in ("f32", "bf16"):
        resumed = GT.trainer(hp_dict(corpus, precision=precision), steps=2)
        assert resumed.discriminator.precision == precision and resumed.disc_steps == 1
        assert all(torch.equal(v, dafter[k]) for k, v in GT.dstate_of(resumed).items())
        assert torch.isfinite(resumed.Train_Step(*resumed.sampler["Train"].batch(2)))


def test_with_multi_scale_the_scales_stay_f32(corpus):
    from glow_tts_amd.vocoder import HiFiGANDiscriminators
    tr = GT.trainer(hp_dict(corpus, multi_scale=True, name="hifigan_bf16_msd"))
    ref = GT.trainer(hp_dict(corpus, precision=None, multi_scale=True, name="hifigan_f32_msd"))
    assert isinstance(tr.discriminator, HiFiGANDiscriminators) and tr.discriminator.precision == "bf16" and tr.discriminator.periods.precision == "bf16"
    assert list(tr.discriminator.params) == list(ref.discriminator.params)
    counts = []
    for t in (tr, ref):
        t.Train_Step(*t.sampler["Train"].batch(0))
        launch_reset()
        t.Train_Step(*t.sampler["Train"].batch(1))
        counts.append({k: c for k, c in launch_counts().items() if c})
    bf, f32 = counts
    scale = lambda c: {k: v for k, v in c.items() if "hifigan_msd" in k}
    assert scale(bf) == scale(f32) and scale(bf) and not any("bf16" in k for k in scale(bf)), (scale(bf), scale(f32))
    assert all(bf.get(k) for k in NEW) and not bf.get("hifigan_disc_conv") and not bf.get("hifigan_disc_conv_bwd"), bf
    assert not any(f32.get(k) for k in NEW + ("hifigan_pack_images",)) and f32.get("hifigan_disc_conv"), f32
    same = lambda k: k not in NEW + ("hifigan_disc_conv", "hifigan_disc_conv_bwd", "hifigan_disc_wgrad", "hifigan_pack_images")
    assert {k: v for k, v in bf.items() if same(k)} == {k: v for k, v in f32.items() if same(k)}
    assert all(torch.isfinite(p).all() for p in tr.discriminator.params.values())
