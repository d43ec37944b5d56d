"""GPU: the adversarial stage of the HiFi-GAN trainer with the yaml sub-block `Vocoder.Train.Adversarial.Multi_Scale`, by the method and with the helpers of
tests/test_gpu_hifigan_gan_trainer.py (corpus, optimizer replay, link checks): the tiny generator, its narrow multi-period discriminator plus a narrow
multi-scale discriminator (two scales, tests/hifigan_msd_ref.py's NARROW) on 2 x 8 frames, three `Train_Step`s with Start_Step = 1.  Every step is replayed
in float64 on the CPU FROM THE DEVICE'S OWN STATE before it and checked link by link under the project's bar (`pwg_train_ref.check`): the waveform; L_stft,
every period's and every scale's p_fake, the adversarial sum, L_fm with the periods' and the scales' terms, L_G, L_D with its two sums, the total d wav;
the generator's gradients under the device's d wav; the gradients of L_D for the union of the discriminators' parameters; both updates.  Then the
checkpoint's keys and a bit-for-bit resume, that a run without the sub-block equals the same run built the way it was before the sub-block existed
(launch log and parameters), and the rule for a checkpoint without the scales' names."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import hifigan_msd_ref as MR  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
import test_gpu_hifigan_gan_trainer as GT  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, SCALES, NET, PREFIX = GT.STEPS, 2, MR.NARROW, "scale_discriminators."
MSD = {"Scales": SCALES, "Channels": NET["channels"], "Groups": NET["groups"], "Strides": NET["strides"], "Kernel_Sizes": NET["kernels"]}
START = GT.ADV["Start_Step"]


def hp_dict(root, multi_scale=True, name=None):
    d = GT.hp_dict(root, name=name or ("hifigan_msd" if multi_scale else "hifigan_mpd_alone"))
    if multi_scale:
        d["Vocoder"]["Train"]["Adversarial"]["Multi_Scale"] = copy.deepcopy(MSD)
    return d


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("hifigan_msd_train"))
    for i, split in enumerate(("Train", "Eval")):
        GT.write_corpus(os.path.join(root, split), seed=i)
    return root, hp_dict(root)


def split(dstate):
    return ({k: v for k, v in dstate.items() if not k.startswith(PREFIX)}, {k[len(PREFIX):]: v for k, v in dstate.items() if k.startswith(PREFIX)})


def reference_links(gstate, dstate, mel, target, settings, dtype, adversarial, wav_in, dwav_in):
    """tests/test_gpu_hifigan_gan_trainer.py's links for the generator and the periods, with the scales' added to every sum"""
    mpd, msd = split(dstate)
    out = GT.reference_links(gstate, mpd, mel, target, settings, dtype, adversarial, wav_in, dwav_in)
    if adversarial:
        a, pred = settings["Adversarial"], wav_in.to(dtype)
        g = MR.generator_term_grads(msd, target, pred, SCALES, NET, GT.SLOPE, float(a["Lambda_Adversarial"]), float(a["Lambda_Feature_Matching"]), dtype)
        p = MR.pair_grads(msd, target, pred, SCALES, NET, GT.SLOPE, dtype)
        out.update({"p_fake[{}]".format(len(GT.PERIODS) + i): s for i, s in enumerate(g["p_fake"])})
        out.update(adv=out["adv"] + g["adv_terms"].sum().reshape(1), L_fm=out["L_fm"] + g["l_fm"], fm_terms_scale=g["fm_terms"], L_G=out["L_G"] + g["loss"],
                   dwav=out["dwav"] + g["dfake"], L_D=out["L_D"] + p["loss"],
                   D_terms=out["D_terms"] + torch.stack([p["real_terms"].sum(), p["fake_terms"].sum()]),
                   dgrads=dict(out["dgrads"], **{PREFIX + k: v for k, v in p["grads"].items()}))
    return out


def device_step(tr, mel, target):
    """`GT.device_step` (which also asserts ONE forward and one frozen chain per period) with the scales' launches counted around the same calls"""
    adversarial = tr.adversarial(tr.steps)
    links = GT.device_step(tr, mel, target)
    if adversarial:
        links["fm_terms_scale"] = tr.last["FM_Terms_Scale"].cpu()
        assert tr.last["FM_Terms"].shape == (len(GT.PERIODS), len(GT.CHANNELS) + 1) and links["fm_terms_scale"].shape == (SCALES, len(NET["channels"]) + 1)
    else:
        assert "FM_Terms_Scale" not in tr.last
    return links


def test_three_steps_match_the_float64_replay(corpus):
    root, d = corpus
    tr = GT.trainer(d)
    from glow_tts_amd.vocoder import HiFiGANDiscriminators
    assert isinstance(tr.discriminator, HiFiGANDiscriminators) and len(tr.disc_params) == len(tr.discriminator.params)
    names, dnames = list(tr.model.params), list(tr.discriminator.params)
    assert sum(k.startswith(PREFIX) for k in dnames) == SCALES * 2 * (len(NET["channels"]) + 1) and not dnames[0].startswith(PREFIX)
    opt = {dt: GT.OptimizerReplay(names, tr.set, dt) for dt in (torch.float64, torch.float32)}
    dopt = {dt: GT.OptimizerReplay(dnames, tr.disc_set, dt) for dt in (torch.float64, torch.float32)}
    failed = []
    for step in range(STEPS):
        mel, target = tr.sampler["Train"].batch(step)
        before, dbefore, adversarial = GT.state_of(tr), GT.dstate_of(tr), step >= START
        launch_reset()
        dev = device_step(tr, mel, target)
        counts = launch_counts()
        assert bool(counts.get("hifigan_msd_conv")) == adversarial and bool(counts.get("hifigan_msd_wgrad")) == adversarial, counts
        after, dafter = GT.state_of(tr), GT.dstate_of(tr)
        r64, r32 = (reference_links(before, dbefore, mel, target, tr.set, dt, adversarial, dev["wav"], dev["dwav"]) for dt in (torch.float64, torch.float32))
        tag = "step {}".format(step + 1)
        GT.check_all(failed, tag + " (a)", dev, {"wav": r64["wav"]}, {"wav": r32["wav"]})
        keys = ("L", "terms", "L_G")
        if adversarial:
            keys += tuple("p_fake[{}]".format(i) for i in range(len(GT.PERIODS) + SCALES)) + ("adv", "L_fm", "fm_terms", "fm_terms_scale", "L_D", "D_terms")
        GT.check_all(failed, tag + " (b)", dev, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
        dwav_inside = TR.errors(r32["dwav"], r64["dwav"], r32["dwav"])[1] < 1e-3
        assert dwav_inside or step > 0, "the reference's d wav leaves the guard at the first step"
        if dwav_inside:
            GT.check_all(failed, tag + " (b)", dev, {"dwav": r64["dwav"]}, {"dwav": r32["dwav"]})
        GT.check_all(failed, tag + " (c)", dev["grads"], r64["grads"], r32["grads"])
        u = {dt: opt[dt].update(before, dev["grads"]) for dt in opt}
        assert u[torch.float64][2] < 1.0, ("the generator's clipping is not active", u[torch.float64][1:])
        GT.check_updates(failed, tag, names, before, after, u[torch.float64][0], u[torch.float32][0])
        if adversarial:
            assert set(dev["dgrads"]) == set(r64["dgrads"]) == set(dnames)
            GT.check_all(failed, tag + " (c')", dev["dgrads"], r64["dgrads"], r32["dgrads"])
            du = {dt: dopt[dt].update(dbefore, dev["dgrads"]) for dt in dopt}
            assert du[torch.float64][2] < 1.0, ("the discriminator's clipping is not active", du[torch.float64][1:])
            GT.check_updates(failed, tag + " discriminator", dnames, dbefore, dafter, du[torch.float64][0], du[torch.float32][0])
            assert tr.disc_steps == dopt[torch.float64].step == step + 1 - START
        else:
            assert all(torch.equal(dafter[k], dbefore[k]) for k in dbefore) and tr.disc_steps == 0
    assert not failed, failed
    assert tr.steps == STEPS


def test_checkpoint_holds_the_union_and_resumes_bit_for_bit(corpus):
    from glow_tts_amd.vocoder import hifigan_disc_geometry, hifigan_disc_load, hifigan_msd_geometry, hifigan_msd_load
    from glow_tts_amd.hparams import Recursive_Parse
    root, d = corpus
    tr = GT.trainer(d)
    states = []
    for s in range(STEPS):
        tr.Train_Step(*tr.sampler["Train"].batch(s))
        states.append((GT.state_of(tr), GT.dstate_of(tr)))
        if s == 1:
            tr.Save_Checkpoint()
    saved = torch.load(tr.Save_Checkpoint(), map_location="cpu")
    assert set(saved) == GT.SIX and saved["Steps"] == STEPS and saved["Discriminator_Steps"] == STEPS - START
    assert list(saved["discriminator"]) == list(tr.discriminator.params) and any(k.startswith(PREFIX) for k in saved["discriminator"])
    # each loader finds its half in the file as it is written
    hp = Recursive_Parse(copy.deepcopy(d))
    mpd, msd = split(saved["discriminator"])
    assert all(torch.equal(v, mpd[k]) for k, v in hifigan_disc_load(mpd, hifigan_disc_geometry(hp)).items())
    assert all(torch.equal(v, msd[k]) for k, v in hifigan_msd_load({"msd": msd}, hifigan_msd_geometry(hp)).items())
    # resumed in the middle of the adversarial stage, the run continues bit for bit
    resumed = GT.trainer(d, steps=2)
    assert resumed.steps == 2 and resumed.disc_steps == 2 - START
    assert all(torch.equal(v, states[1][1][k]) for k, v in GT.dstate_of(resumed).items())
    resumed.Train_Step(*resumed.sampler["Train"].batch(2))
    assert all(torch.equal(v, states[2][0][k]) for k, v in GT.state_of(resumed).items())
    assert all(torch.equal(v, states[2][1][k]) for k, v in GT.dstate_of(resumed).items())
    again = GT.trainer(d)                                                                          # and the whole run repeats
    for s in range(STEPS):
        again.Train_Step(*again.sampler["Train"].batch(s))
    assert all(torch.equal(v, states[-1][1][k]) for k, v in GT.dstate_of(again).items())


def test_without_the_sub_block_the_run_is_the_one_built_the_old_way(corpus):
    """The trainer as it was before the sub-block existed - the multi-period discriminator built directly, `score_pair`'s four values unpacked as they were -
    against today's trainer without `Multi_Scale`: the same launches, the same parameters after two steps, the same `last` and checkpoint keys."""
    from glow_tts_amd import hifigan_trainer as T
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.vocoder import HiFiGANPeriodDiscriminator, adversarial_mse
    root, _ = corpus

    class Old(T.HiFiGAN_Trainer):
        def make_discriminator(self):
            return HiFiGANPeriodDiscriminator(self.hp, self.device, trainable=True, seed=self.seed)

        def adversarial_losses(self, target, wav, stft):
            both, p_fake, l_fm, fm_terms = self.discriminator.score_pair(target, wav)
            adv, d_loss, d_terms = 0.0, 0.0, 0.0
            for b, p in zip(both, p_fake):
                a, _ = adversarial_mse(p, 1.0)
                dl, t = adversarial_mse(b, (1.0, 0.0))
                adv, d_loss, d_terms = adv + a, d_loss + dl, d_terms + t
            self.fm, self.fm_scale = (l_fm.detach(), fm_terms), None
            loss = stft + float(self.disc_set["Lambda_Adversarial"]) * adv + float(self.disc_set["Lambda_Feature_Matching"]) * l_fm
            return loss, d_loss, torch.cat([adv.detach().reshape(1), d_terms]), stft

    runs = []
    for cls, name in ((Old, "old_way"), (T.HiFiGAN_Trainer, "new_way")):
        tr = cls(steps=0, hp=Recursive_Parse(copy.deepcopy(hp_dict(root, multi_scale=False, name=name))), seed=GT.SEED)
        GT.scale_discriminator(tr)
        assert isinstance(tr.discriminator, HiFiGANPeriodDiscriminator) and tr.bundles() == T.BUNDLES
        logs = []
        for s in range(2):
            launch_reset()
            loss = tr.Train_Step(*tr.sampler["Train"].batch(s))
            logs.append(({k: n for k, n in launch_counts().items() if n}, loss.cpu(), set(tr.last)))
        saved = torch.load(tr.Save_Checkpoint(), map_location="cpu")
        runs.append((logs, GT.state_of(tr), GT.dstate_of(tr), set(saved), list(saved["discriminator"])))
    (la, ga, da, ka, na), (lb, gb, db, kb, nb) = runs
    assert [x[0] for x in la] == [x[0] for x in lb] and all(torch.equal(x[1], y[1]) for x, y in zip(la, lb)) and [x[2] for x in la] == [x[2] for x in lb]
    assert not any(k.startswith("hifigan_msd") for x in lb for k in x[0]) and "FM_Terms_Scale" not in lb[1][2]
    assert all(torch.equal(ga[k], gb[k]) for k in ga) and list(da) == list(db) and all(torch.equal(da[k], db[k]) for k in da)
    assert ka == kb == GT.SIX and na == nb and not any(k.startswith(PREFIX) for k in nb)


def test_a_checkpoint_without_the_scales_resumes_up_to_start_step_only(corpus):
    root, _ = corpus
    alone_d, both_d = hp_dict(root, multi_scale=False, name="hifigan_msd_rule"), hp_dict(root, name="hifigan_msd_rule")
    alone = GT.trainer(alone_d, scale=False)
    for s in range(2):
        alone.Train_Step(*alone.sampler["Train"].batch(s))
        saved = torch.load(alone.Save_Checkpoint(), map_location="cpu")
        assert set(saved) == GT.SIX and not any(k.startswith(PREFIX) for k in saved["discriminator"])
    whole = GT.trainer(both_d, scale=False)
    for s in range(2):
        whole.Train_Step(*whole.sampler["Train"].batch(s))
    resumed = GT.trainer(both_d, steps=1)                                                          # Steps = 1 <= Start_Step = 1: the stage-one rule
    assert resumed.steps == 1 and resumed.disc_steps == 0
    fresh = GT.trainer(both_d, scale=False)
    assert all(torch.equal(v, GT.dstate_of(fresh)[k]) for k, v in GT.dstate_of(resumed).items())   # both seeded inits
    resumed.Train_Step(*resumed.sampler["Train"].batch(1))
    assert resumed.disc_steps == 1
    assert all(torch.equal(v, GT.state_of(whole)[k]) for k, v in GT.state_of(resumed).items())
    assert all(torch.equal(v, GT.dstate_of(whole)[k]) for k, v in GT.dstate_of(resumed).items())
    with pytest.raises(ValueError, match=r"scale_discriminators\.discriminators\.0\.convs\.0\.weight.*Vocoder\.Train\.Adversarial\.Multi_Scale"):
        GT.trainer(both_d, steps=2)
