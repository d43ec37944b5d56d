"""GPU: the adversarial stage of the HiFi-GAN trainer (glow_tts_amd/hifigan_trainer.py with the yaml block `Vocoder.Train.Adversarial`) on a synthetic
pattern directory, by the method of tests/test_gpu_pwg_gan_trainer.py (its helpers are copied here, not imported): the tiny generator `TINY` of
tests/test_gpu_hifigan.py, a tiny multi-period discriminator (two periods, three widths) and three `Train_Step`s with Start_Step = 1 - the first is stage one
and must be bit-identical to a block-less trainer's, the second and third are adversarial - against a float64 replay on the CPU
(tests/hifigan_train_ref.py's generator, tests/hifigan_disc_ref.py's discriminator and losses, the library-STFT loss of tests/pwg_train_ref.py,
oracle/radam_ref.py), the six-key checkpoint through `Vocoder.Checkpoint_Path`, resuming across the Start_Step boundary and from a stage-one checkpoint.

Every step is replayed FROM THE DEVICE'S OWN STATE before it and checked link by link, each link under the project's bar (`pwg_train_ref.check`):
(a) the waveform; (b) L_stft and its terms, every period's p_fake, the adversarial sum, L_fm and its terms, L_G, L_D with its two sums and the total d wav
(STFT term + Lambda_Adversarial * adversarial term + Lambda_Feature_Matching * feature-matching term) at the device's waveform; (c) every generator gradient
under the device's d wav as the functional; (c') every discriminator gradient of L_D at the device's waveform and target; (d) both updates - clipping, RAdam
and the step decay, each with its own settings and its OWN update count - fed with the device's gradients.  The discriminator starts from its seeded init
times 3, as in tests/test_gpu_hifigan_disc.py.  d wav is held to the bar wherever the reference's own float32 run stays inside the guard e32 < 1e-3 (the
1 / |X| of L_mag; it must at the first step); the updates hold the inequality and the e32 guard for every tensor.  The number of tensors whose update exceeds
1e-3 is printed, not asserted."""
import copy
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import hifigan_disc_ref as HR  # noqa: E402
import hifigan_train_ref as R  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
import test_gpu_hifigan as G  # noqa: E402
from helpers import launch_counts, launch_reset, tiny_hp_dict  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, BATCH, FRAMES, SEED, HOP = 3, 2, 8, 5, 256
RESOLUTIONS = [(256, 50, 240), (512, 120, 400)]
# The generator's: unrectified RAdam with the clipping active (asserted), so an update has the norm rate * bound.  A float32 parameter is stored to 1 ulp,
# 1.2e-7 of its size, whatever computes it; that stays below the bar's 1e-6 of an update only while the update is above a tenth of the parameter, and the bar
# of a one-element tensor (conv_post.bias) has no e32 to speak of.  The stage-one test keeps rate * bound = 1; here the rate is halved at the third step
# (the decay is part of what is checked), so the rate starts at 20 and rate * bound is 2, 2, 1.
LEARNING_RATE, GRADIENT_NORM = 20.0, 0.1
PERIODS, CHANNELS, SLOPE = [2, 3], [16, 32, 16], 0.1
ADV = {"Start_Step": 1, "Lambda_Adversarial": 1.5, "Lambda_Feature_Matching": 2.5, "Learning_Rate": 0.5, "Gradient_Norm": 0.5,
       "Learning_Rate_Decay": {"Step": 1, "Gamma": 0.5}, "Periods": PERIODS, "Channels": CHANNELS, "Negative_Slope": SLOPE}
DISC_SCALE = 3.0
SIX = {"generator", "Optimizer", "Steps", "discriminator", "Discriminator_Optimizer", "Discriminator_Steps"}


def write_corpus(root, seed):
    rng = np.random.default_rng(seed)
    meta = {"File_List": [], "Mel_Length_Dict": {}, "Audio_Length_Dict": {}}
    os.makedirs(root, exist_ok=True)
    for i, n in enumerate((9, 12, 6, 10)):                                   # 6 frames: too short for a segment of 8
        name = "F{}.PICKLE".format(i)
        pat = {"Audio": (rng.standard_normal(n * HOP) * 0.3).astype(np.float32), "Mel": rng.uniform(-4, 4, (n, G.TINY["A"])).astype(np.float32)}
        with open(os.path.join(root, name), "wb") as f:
            pickle.dump(pat, f)
        meta["File_List"].append(name)
        meta["Mel_Length_Dict"][name], meta["Audio_Length_Dict"][name] = n, n * HOP
    with open(os.path.join(root, "METADATA.PICKLE"), "wb") as f:
        pickle.dump(meta, f)


def hp_dict(root, adversarial=True, name=None):
    d = tiny_hp_dict("Vanilla")
    assert d["Sound"]["Frame_Shift"] == HOP
    d["Vocoder"] = G.block_of(G.TINY, Train={"Batch_Size": BATCH, "Segment_Frames": FRAMES, "Learning_Rate": LEARNING_RATE, "Gradient_Norm": GRADIENT_NORM,
                                             "STFT_Resolutions": [list(r) for r in RESOLUTIONS], "Learning_Rate_Decay": {"Step": 2, "Gamma": 0.5},
                                             "Max_Step": 4, "Checkpoint_Save_Interval": 2, "Evaluation_Interval": 2,
                                             "Checkpoint_Path": os.path.join(root, name or ("hifigan_gan" if adversarial else "hifigan_plain"))})
    if adversarial:
        d["Vocoder"]["Train"]["Adversarial"] = copy.deepcopy(ADV)
    for split, key in (("Train", "Train_Pattern"), ("Eval", "Eval_Pattern")):
        d["Train"][key].update(Path=os.path.join(root, split), Metadata_File="METADATA.PICKLE")
    return d


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("hifigan_gan_train"))
    for i, split in enumerate(("Train", "Eval")):
        write_corpus(os.path.join(root, split), seed=i)
    return root, hp_dict(root)


def scale_discriminator(tr):
    with torch.no_grad():
        for p in tr.discriminator.params.values():
            p.mul_(DISC_SCALE)


def trainer(d, steps=0, scale=True):
    """A trainer whose fresh discriminator starts from its seeded init times DISC_SCALE (a resumed one: from its checkpoint)"""
    from glow_tts_amd.hifigan_trainer import HiFiGAN_Trainer
    from glow_tts_amd.hparams import Recursive_Parse
    tr = HiFiGAN_Trainer(steps=steps, hp=Recursive_Parse(copy.deepcopy(d)), seed=SEED)
    if steps == 0 and scale and tr.discriminator is not None:
        scale_discriminator(tr)
    return tr


def state_of(tr):
    return {k: v.detach().cpu().clone() for k, v in tr.model.params.items()}


def dstate_of(tr):
    return {k: v.detach().cpu().clone() for k, v in tr.discriminator.params.items()}


@pytest.fixture(scope="module")
def run(corpus):
    """-> (hp dict, the trainer after STEPS steps, the generator's and the discriminator's states after each step, the batches, each step's launch counts)"""
    root, d = corpus
    tr = trainer(d)
    batches = [tr.sampler["Train"].batch(s) for s in range(STEPS)]
    states, counts = [], []
    for mel, target in batches:
        launch_reset()
        tr.Train_Step(mel, target)
        counts.append(launch_counts())
        states.append((state_of(tr), dstate_of(tr)))
    torch.cuda.synchronize()
    return d, tr, states, batches, counts


def reference_links(gstate, dstate, mel, target, settings, dtype, adversarial, wav_in, dwav_in):
    """One step's links in `dtype` on the CPU from the parameters `gstate`, `dstate`: the waveform; L_stft, its terms and, at the prediction `wav_in`, every
    adversarial and feature-matching link, L_G, L_D and the total d wav; the generator's gradients under the functional `dwav_in`; the discriminator's
    gradients of L_D at `wav_in` and the target."""
    wavs, grads = R.generator_grads(gstate, G.TINY, list(mel), list(dwav_in), dtype)
    pred = wav_in.to(dtype)
    r = TR.loss_and_grad(pred, target, settings["STFT_Resolutions"], dtype)
    out = {"wav": torch.stack(wavs), "L": r["L"], "terms": r["terms"], "dwav": r["dpred"], "grads": grads, "L_G": r["L"]}
    if adversarial:
        a, n = settings["Adversarial"], len(CHANNELS)
        g = HR.generator_term_grads(dstate, target, pred, PERIODS, n, SLOPE, float(a["Lambda_Adversarial"]), float(a["Lambda_Feature_Matching"]), dtype)
        p = HR.pair_grads(dstate, target, pred, PERIODS, n, SLOPE, dtype)
        scores = [s.detach() for s, _ in HR.forward({k: v.to(dtype) for k, v in dstate.items()}, pred, PERIODS, n, SLOPE)]
        out.update({"p_fake[{}]".format(i): s for i, s in enumerate(scores)})
        out.update(adv=g["adv_terms"].sum().reshape(1), L_fm=g["l_fm"], fm_terms=g["fm_terms"], L_G=r["L"] + g["loss"], dwav=r["dpred"] + g["dfake"],
                   L_D=p["loss"], D_terms=torch.stack([p["real_terms"].sum(), p["fake_terms"].sum()]), dgrads=p["grads"])
    return out


class OptimizerReplay:
    """Clipping, RAdam (oracle/radam_ref.py's scalars) and the step decay in `dtype`, fed with given gradients; `step` counts this optimizer's own updates"""

    def __init__(self, names, settings, dtype):
        self.s, self.dtype, self.m, self.v, self.step = settings, dtype, {k: 0.0 for k in names}, {k: 0.0 for k in names}, 0

    def update(self, params, grads):
        """-> ({name: update}, gradient norm, clip coefficient) of the next step for `params` (the state before it)"""
        from oracle import radam_ref
        s, dt = self.s, self.dtype
        norm, coef = radam_ref.clip_coef([g.double().numpy() for g in grads.values()], float(s["Gradient_Norm"]))
        lr = float(s["Learning_Rate"]) * float(s["Learning_Rate_Decay"]["Gamma"]) ** (self.step // int(s["Learning_Rate_Decay"]["Step"]))
        self.step += 1
        n_sma, size = radam_ref.radam_scalars(self.step, 0.9, 0.999)
        out = {}
        for k, g in grads.items():
            gk = (g.to(dt) * torch.tensor(coef, dtype=dt))
            self.v[k] = self.v[k] * 0.999 + (1 - 0.999) * gk * gk
            self.m[k] = self.m[k] * 0.9 + (1 - 0.9) * gk
            p = params[k].to(dt)
            out[k] = (p - size * lr * (self.m[k] / (self.v[k].sqrt() + float(s["Epsilon"])) if n_sma >= 5 else self.m[k])) - p
        return out, float(norm), float(coef)


def check_all(failed, tag, got, r64, r32):
    for k in r64:
        try:
            TR.check("{} {}".format(tag, k), got[k], r64[k], r32[k])
        except AssertionError as err:
            failed.append(str(err))


def check_updates(failed, tag, names, before, after, u64, u32):
    """(d): the bar's inequality and its e32 guard for every tensor -> the number of tensors whose float64 update exceeds 1e-3"""
    large = 0
    for k in names:
        err, e32, scale = TR.errors(after[k].double() - before[k].double(), u64[k], u32[k])
        print("{} (d) update of {}: err {:.3e}  e32 {:.3e}  ratio {:.3f}  max|ref| {:.3e}".format(tag, k, err, e32, err / (4 * e32 + 1e-6), scale))
        assert 0 < e32 < 1e-3 and scale > 0, (tag, k, e32, scale)
        if err > 4 * e32 + 1e-6:
            failed.append(str((tag + " (d) update of " + k, err, e32)))
        large += scale > 1e-3
    return large


def device_step(tr, mel, target):
    """The step's links through the trainer's own parts, then the very `Train_Step` (bit-identical arithmetic: everything is deterministic)"""
    adversarial, dev, n = tr.adversarial(tr.steps), tr.device, len(CHANNELS)
    for p in tr.params + tr.disc_params:
        p.grad = None
    wav = tr.generate(mel.to(dev), [FRAMES] * BATCH, tr.steps)
    wav.retain_grad()
    stft = tr.criterion(wav, target.to(dev))
    links = {"wav": wav.detach().cpu(), "L": stft.detach().cpu().reshape(1), "terms": tr.criterion.terms.cpu().clone()}
    loss = stft
    if adversarial:
        launch_reset()
        loss, d_loss, adv_terms, _ = tr.adversarial_losses(target.to(dev), wav, stft)
        counts = launch_counts()
        assert counts.get("hifigan_disc_first") == len(PERIODS) and counts.get("hifigan_disc_post") == len(PERIODS), counts   # ONE forward per period
        l_fm, fm_terms = tr.fm
        launch_reset()
        loss.backward()
        counts = launch_counts()
        assert not any("hifigan_disc_wgrad" in k and c for k, c in counts.items()), counts             # the generator term: the data chain alone,
        assert counts.get("hifigan_disc_conv_bwd") == len(PERIODS) * (n - 1) and counts.get("hifigan_disc_first_bwd") == len(PERIODS), counts   # once per period
        assert all(p.grad is None for p in tr.disc_params)
        d_loss.backward()
        links.update(adv=adv_terms[:1].cpu(), L_fm=l_fm.cpu().reshape(1), fm_terms=fm_terms.cpu(), L_D=d_loss.detach().cpu().reshape(1),
                     D_terms=adv_terms[1:].cpu(), dgrads={k: p.grad.detach().cpu().clone() for k, p in tr.discriminator.params.items()})
        both = tr.discriminator.score(wav.detach(), freeze=True)
        links.update({"p_fake[{}]".format(i): s.detach().cpu() for i, s in enumerate(both)})
    else:
        loss.backward()
        assert all(p.grad is None for p in tr.disc_params)
    links.update(L_G=loss.detach().cpu().reshape(1), dwav=wav.grad.cpu().clone(), grads={k: p.grad.detach().cpu().clone() for k, p in tr.model.params.items()})
    got = tr.Train_Step(mel, target)
    assert torch.equal(got.cpu().reshape(1), links["L_G"])
    if adversarial:
        assert torch.equal(tr.last["L_adv"].cpu().reshape(1), links["adv"]) and torch.equal(tr.last["Discriminator_Loss"].cpu().reshape(1), links["L_D"])
        assert torch.equal(tr.last["Real_Term"].cpu(), links["D_terms"][0]) and torch.equal(tr.last["Fake_Term"].cpu(), links["D_terms"][1])
        assert torch.equal(tr.last["L_fm"].cpu().reshape(1), links["L_fm"]) and torch.equal(tr.last["STFT_Loss"].cpu().reshape(1), links["L"])
    return links


def test_three_steps_match_the_float64_replay(corpus):
    root, d = corpus
    tr = trainer(d)
    names, dnames = list(tr.model.params), list(tr.discriminator.params)
    opt = {dt: OptimizerReplay(names, tr.set, dt) for dt in (torch.float64, torch.float32)}
    dopt = {dt: OptimizerReplay(dnames, tr.disc_set, dt) for dt in (torch.float64, torch.float32)}
    failed = []
    for step in range(STEPS):
        mel, target = tr.sampler["Train"].batch(step)
        before, dbefore, adversarial = state_of(tr), dstate_of(tr), step >= ADV["Start_Step"]
        dev = device_step(tr, mel, target)
        after, dafter = state_of(tr), dstate_of(tr)
        r64, r32 = (reference_links(before, dbefore, mel, target, tr.set, dt, adversarial, dev["wav"], dev["dwav"]) for dt in (torch.float64, torch.float32))
        tag = "step {}".format(step + 1)
        check_all(failed, tag + " (a)", dev, {"wav": r64["wav"]}, {"wav": r32["wav"]})
        keys = ("L", "terms", "L_G") + (tuple("p_fake[{}]".format(i) for i in range(len(PERIODS))) + ("adv", "L_fm", "fm_terms", "L_D", "D_terms") if adversarial else ())
        check_all(failed, tag + " (b)", dev, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
        dwav_inside = TR.errors(r32["dwav"], r64["dwav"], r32["dwav"])[1] < 1e-3
        assert dwav_inside or step > 0, "the reference's d wav leaves the guard at the first step"
        if dwav_inside:
            check_all(failed, tag + " (b)", dev, {"dwav": r64["dwav"]}, {"dwav": r32["dwav"]})
        check_all(failed, tag + " (c)", dev["grads"], r64["grads"], r32["grads"])
        u = {dt: opt[dt].update(before, dev["grads"]) for dt in opt}
        assert u[torch.float64][2] < 1.0, ("the generator's clipping is not active", u[torch.float64][1:])
        large, dlarge = check_updates(failed, tag, names, before, after, u[torch.float64][0], u[torch.float32][0]), None
        if adversarial:
            check_all(failed, tag + " (c')", dev["dgrads"], r64["dgrads"], r32["dgrads"])
            du = {dt: dopt[dt].update(dbefore, dev["dgrads"]) for dt in dopt}
            assert du[torch.float64][2] < 1.0, ("the discriminator's clipping is not active", du[torch.float64][1:])
            dlarge = check_updates(failed, tag + " discriminator", dnames, dbefore, dafter, du[torch.float64][0], du[torch.float32][0])
            assert tr.disc_steps == dopt[torch.float64].step == step + 1 - ADV["Start_Step"]
        else:
            assert all(torch.equal(dafter[k], dbefore[k]) for k in dbefore) and tr.disc_steps == 0
        print("{}: d wav {} the guard; {} of {} generator updates and {} of {} discriminator updates above 1e-3".format(
            tag, "inside" if dwav_inside else "OUTSIDE", large, len(names), dlarge, len(dnames)))
    assert not failed, failed
    assert tr.steps == STEPS
    # each rate follows its own update count
    assert tr.learning_rate(1) == LEARNING_RATE and tr.learning_rate(2) == LEARNING_RATE * 0.5
    assert tr.disc_learning_rate(0) == ADV["Learning_Rate"] and tr.disc_learning_rate(1) == ADV["Learning_Rate"] * 0.5


def test_the_first_step_is_stage_one_bit_for_bit(run, corpus):
    """Before Start_Step the generator's step is a block-less trainer's in every tensor and in its launches, and the discriminator is not touched."""
    root, d = corpus
    _, tr, states, batches, counts = run
    plain = trainer(hp_dict(root, adversarial=False))
    assert plain.discriminator is None
    launch_reset()
    loss = plain.Train_Step(*batches[0])
    ran = lambda c: {k: n for k, n in c.items() if n}
    assert ran(launch_counts()) == ran(counts[0]) and not any("hifigan_disc" in k and c for k, c in counts[0].items())
    assert any("hifigan_disc" in k and c for k, c in counts[1].items())
    assert all(torch.equal(v, states[0][0][k]) for k, v in state_of(plain).items())
    fresh = trainer(d)
    assert all(torch.equal(v, states[0][1][k]) for k, v in dstate_of(fresh).items())          # D after step 1 = D at construction (times DISC_SCALE)
    first = fresh.Train_Step(*batches[0])
    assert torch.equal(first, loss) and set(fresh.last) == set(plain.last) and fresh.disc_steps == 0
    assert any(not torch.equal(states[1][1][k], states[0][1][k]) for k in states[0][1])          # and it moves from Start_Step on


def test_without_the_block_nothing_changes(corpus):
    """A block-less trainer: no discriminator, today's settings key for key, today's three checkpoint keys, no discriminator launch, and two runs of its
    steps agree bit for bit."""
    from glow_tts_amd import hifigan_trainer as T
    root, _ = corpus
    d = hp_dict(root, adversarial=False, name="hifigan_blockless")
    a, b = trainer(d), trainer(d)
    assert a.discriminator is None and a.disc_set is None and set(a.set) == set(T.DEFAULTS) and a.bundles() == T.BUNDLES[:1]
    launch_reset()
    for s in range(2):
        la, lb = a.Train_Step(*a.sampler["Train"].batch(s)), b.Train_Step(*b.sampler["Train"].batch(s))
        assert torch.equal(la, lb) and set(a.last) == {"Loss", "Terms", "Gradient_Norm"}
    assert not any("disc" in k and c for k, c in launch_counts().items())
    assert all(torch.equal(v, state_of(b)[k]) for k, v in state_of(a).items())
    saved = torch.load(a.Save_Checkpoint(), map_location="cpu")
    assert set(saved) == {"generator", "Optimizer", "Steps"} and saved["Steps"] == 2


def test_three_steps_repeat_bit_for_bit(run, corpus):
    d, tr, states, batches, _ = run
    assert tr.steps == STEPS and tr.disc_steps == STEPS - ADV["Start_Step"]
    assert all(torch.isfinite(tr.last[k]).all() for k in ("Loss", "STFT_Loss", "L_adv", "L_fm", "Real_Term", "Fake_Term", "Discriminator_Loss"))
    again = trainer(d)
    for mel, target in batches:
        again.Train_Step(mel, target)
    assert all(torch.equal(v, states[-1][0][k]) for k, v in state_of(again).items())
    assert all(torch.equal(v, states[-1][1][k]) for k, v in dstate_of(again).items())


def test_checkpoint_has_six_keys_loads_frozen_and_resumes(run, corpus):
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.vocoder import HiFiGAN, hifigan_disc_geometry, hifigan_disc_load
    d, tr, states, batches, _ = run
    # a checkpoint before Start_Step already carries the discriminator (initialised at construction); resuming from it crosses the boundary
    early = trainer(d)
    saved = torch.load(early.Save_Checkpoint(), map_location="cpu")
    assert set(saved) == SIX and saved["Steps"] == 0 and saved["Discriminator_Steps"] == 0
    early.Train_Step(*batches[0])
    early.Save_Checkpoint()
    resumed = trainer(d, steps=1)
    assert resumed.steps == 1 and resumed.disc_steps == 0
    for s in (1, 2):
        resumed.Train_Step(*resumed.sampler["Train"].batch(resumed.steps))
        assert all(torch.equal(v, states[s][0][k]) for k, v in state_of(resumed).items()), s
        assert all(torch.equal(v, states[s][1][k]) for k, v in dstate_of(resumed).items()), s
    # after the adversarial steps: six keys; the frozen vocoder reads it through Vocoder.Checkpoint_Path and reproduces the live generator
    path = tr.Save_Checkpoint()
    assert os.path.basename(path) == "HIFIGAN_{}.pt".format(STEPS)
    saved = torch.load(path, map_location="cpu")
    assert set(saved) == SIX and saved["Steps"] == STEPS and saved["Discriminator_Steps"] == STEPS - ADV["Start_Step"]
    assert set(saved["discriminator"]) == set(states[-1][1])
    dd = copy.deepcopy(d)
    dd["Vocoder"]["Checkpoint_Path"] = path
    hp = Recursive_Parse(copy.deepcopy(dd))
    frozen = HiFiGAN(hp, "cuda:0")
    mel, _ = tr.sampler["Eval"].batch(0)
    live = tr.model.generate(mel.cuda(), [FRAMES] * BATCH)[0].detach()
    assert torch.equal(frozen(mel.cuda(), [FRAMES] * BATCH)[0], live)
    loaded = hifigan_disc_load(saved, hifigan_disc_geometry(hp))
    assert all(torch.equal(loaded[k], v) for k, v in states[-1][1].items())
    # a resumed run continues bit-identically to the uninterrupted one over two more adversarial steps
    resumed = trainer(d, steps=STEPS)
    assert resumed.steps == STEPS and resumed.disc_steps == tr.disc_steps
    assert all(torch.equal(v, states[-1][1][k]) for k, v in dstate_of(resumed).items())
    for _ in range(2):
        nxt = tr.sampler["Train"].batch(tr.steps)
        resumed.Train_Step(*resumed.sampler["Train"].batch(resumed.steps))
        tr.Train_Step(*nxt)
        assert all(torch.equal(v, state_of(resumed)[k]) for k, v in state_of(tr).items())
        assert all(torch.equal(v, dstate_of(resumed)[k]) for k, v in dstate_of(tr).items())
    ev = tr.Evaluation(batches=2)
    assert ev is not None and len(ev) == 3 and np.isfinite(ev[0]) and ev[1].shape == (len(RESOLUTIONS), 2)
    assert ev[2].shape == (3,) and torch.isfinite(ev[2]).all() and (ev[2] >= 0).all()


def test_a_stage_one_checkpoint_resumes_up_to_start_step(corpus):
    """`HIFIGAN_1.pt` of a block-less run (three keys) resumes under the block at Steps = 1 <= Start_Step = 1 with the seeded-init discriminator and continues
    exactly as a run that had the block from the start (the discriminator is untouched before Start_Step); beyond Start_Step it is the ValueError of the
    Parallel WaveGAN trainer."""
    root, _ = corpus
    plain_d, gan_d = hp_dict(root, adversarial=False, name="hifigan_stage_one"), hp_dict(root, name="hifigan_stage_one")
    plain = trainer(plain_d)
    for s in range(2):
        plain.Train_Step(*plain.sampler["Train"].batch(s))
        assert set(torch.load(plain.Save_Checkpoint(), map_location="cpu")) == {"generator", "Optimizer", "Steps"}
    whole = trainer(gan_d, scale=False)
    for s in range(2):
        whole.Train_Step(*whole.sampler["Train"].batch(s))
    resumed = trainer(gan_d, steps=1)
    assert resumed.steps == 1 and resumed.disc_steps == 0
    fresh = trainer(gan_d, scale=False)
    assert all(torch.equal(v, dstate_of(fresh)[k]) for k, v in dstate_of(resumed).items())       # the seeded init
    resumed.Train_Step(*resumed.sampler["Train"].batch(1))                                        # an adversarial step
    assert resumed.disc_steps == 1
    assert all(torch.equal(v, state_of(whole)[k]) for k, v in state_of(resumed).items())
    assert all(torch.equal(v, dstate_of(whole)[k]) for k, v in dstate_of(resumed).items())
    with pytest.raises(ValueError, match=r"holds no discriminator.*Vocoder\.Train\.Adversarial"):
        trainer(gan_d, steps=2)
