"""GPU: the adversarial stage of the Parallel WaveGAN trainer (glow_tts_amd/pwg_trainer.py with the yaml block `Vocoder.Train.Discriminator`) on a synthetic
pattern directory, by the method of tests/test_gpu_pwg_trainer.py (its helpers are copied here, not imported): three `Train_Step`s with Start_Step = 1 - the
first is stage one and must be bit-identical to a block-less trainer's, the second and third are adversarial - against a float64 replay on the CPU
(tests/pwg_ref.py's generator, tests/pwg_disc_ref.py's discriminator and losses, the library-STFT loss of tests/pwg_train_ref.py, oracle/radam_ref.py),
the six-key checkpoint through `Vocoder.Checkpoint_Path`, and resuming across the Start_Step boundary.

Every step is replayed FROM THE DEVICE'S OWN STATE before it and checked link by link, each link under the project's bar (`pwg_train_ref.check`):
(a) the waveform; (b) L_stft and its terms, p_fake, L_adv, L_D with its two terms and the total d wav (STFT term + Lambda_Adversarial * adversarial term) at the
device's waveform; (c) every generator gradient under the device's d wav as the functional; (c') every discriminator gradient of L_D at the device's
waveform and target; (d) both updates - clipping, RAdam and the step decay, each with its own settings and its OWN update count (the discriminator's first
update is its step 1 and its decay counts its own updates) - fed with the device's gradients.  The discriminator starts from its seeded init times 3 (at
scale 1 its early layers' gradients fall below the guard max |ref64| > 1e-3).  Guards: (a), (b) without d wav, (c) and (c') hold the bar's guards at every
step; d wav holds them at the first step (asserted) and is held to the bar later when the reference's own float32 run stays inside e32 < 1e-3 there (the
old test's rule: the 1 / |X| of L_mag); the updates hold the inequality and the e32 guard for every tensor, and at least UPDATES_ABOVE of the tensors that
have a gradient exceed 1e-3 at every step they are updated (the count the float64 reference alone reaches; printed).
"""
import copy
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import pwg_disc_ref as DR  # noqa: E402
import pwg_ref as P  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
from helpers import launch_counts, launch_reset, tiny_hp_dict  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, BATCH, FRAMES, HOP, SEED = 3, 3, 40, 15, 5
RESOLUTIONS = [(256, 50, 240), (512, 120, 400)]
LEARNING_RATE, GRADIENT_NORM = 1.0, 1.0                                      # the generator's, as in the stage-one test: unrectified RAdam, clipping active
DISC = {"Start_Step": 1, "Lambda_Adversarial": 4.0, "Learning_Rate": 0.5, "Gradient_Norm": 0.5, "Learning_Rate_Decay": {"Step": 1, "Gamma": 0.5},
        "Layers": 4, "Channels": 16}
DISC_SCALE = 3.0
UPDATES_ABOVE = {"generator": 30, "discriminator": 8}                        # of 35 and of 8 tensors


def config():
    hp = tiny_hp_dict("Vanilla")
    return dict(P.NARROW, A=hp["Sound"]["Mel_Dim"])


def write_corpus(root, mel_dim, seed):
    """A handful of short files: white noise of amplitude 0.3 (no STFT bin near the clamp) under uniform mels"""
    rng = np.random.default_rng(seed)
    meta = {"File_List": [], "Mel_Length_Dict": {}, "Audio_Length_Dict": {}}
    os.makedirs(root, exist_ok=True)
    for i, n in enumerate((45, 60, 30, 52, 41)):                              # 30 frames: too short for a segment of 40
        name = "F{}.PICKLE".format(i)
        pat = {"Audio": (rng.standard_normal(n * HOP) * 0.3).astype(np.float32), "Mel": rng.uniform(-4, 4, (n, mel_dim)).astype(np.float32)}
        with open(os.path.join(root, name), "wb") as f:
            pickle.dump(pat, f)
        meta["File_List"].append(name)
        meta["Mel_Length_Dict"][name], meta["Audio_Length_Dict"][name] = n, n * HOP
    with open(os.path.join(root, "METADATA.PICKLE"), "wb") as f:
        pickle.dump(meta, f)


def hp_dict(root, disc=True):
    cfg = config()
    d = tiny_hp_dict("Vanilla")
    d["Sound"]["Frame_Shift"] = HOP
    d["Vocoder"] = {"Type": "PWG", "Layers": cfg["layers"], "Stacks": cfg["stacks"], "Residual_Channels": cfg["R"], "Gate_Channels": cfg["G"],
                    "Skip_Channels": cfg["S"], "Upsample_Scales": list(cfg["scales"]),
                    "Train": {"Batch_Size": BATCH, "Segment_Frames": FRAMES, "Learning_Rate": LEARNING_RATE, "Gradient_Norm": GRADIENT_NORM,
                              "STFT_Resolutions": [list(r) for r in RESOLUTIONS], "Learning_Rate_Decay": {"Step": 2, "Gamma": 0.5},
                              "Max_Step": 4, "Checkpoint_Save_Interval": 2, "Evaluation_Interval": 2,
                              "Checkpoint_Path": os.path.join(root, "pwg_gan" if disc else "pwg_plain")}}
    if disc:
        d["Vocoder"]["Train"]["Discriminator"] = copy.deepcopy(DISC)
    for split, key in (("Train", "Train_Pattern"), ("Eval", "Eval_Pattern")):
        d["Train"][key].update(Path=os.path.join(root, split), Metadata_File="METADATA.PICKLE")
    return d


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pwg_gan_train"))
    for i, split in enumerate(("Train", "Eval")):
        write_corpus(os.path.join(root, split), config()["A"], seed=i)
    return root, hp_dict(root)


def trainer(d, steps=0):
    """A trainer whose fresh discriminator starts from its seeded init times DISC_SCALE (a resumed one: from its checkpoint)"""
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.pwg_trainer import PWG_Trainer
    tr = PWG_Trainer(steps=steps, hp=Recursive_Parse(copy.deepcopy(d)), seed=SEED)
    if steps == 0 and tr.discriminator is not None:
        with torch.no_grad():
            for p in tr.discriminator.params.values():
                p.mul_(DISC_SCALE)
    return tr


def state_of(tr):
    return {k: v.detach().cpu().clone() for k, v in tr.model.params.items()}


def dstate_of(tr):
    return {k: v.detach().cpu().clone() for k, v in tr.discriminator.params.items()}


@pytest.fixture(scope="module")
def run(corpus):
    """-> (hp dict, the trainer after STEPS steps, the generator's and the discriminator's states after each step, the batches)"""
    root, d = corpus
    tr = trainer(d)
    batches = [tr.sampler["Train"].batch(s) for s in range(STEPS)]
    states = []
    for mel, target in batches:
        tr.Train_Step(mel, target)
        states.append((state_of(tr), dstate_of(tr)))
    torch.cuda.synchronize()
    return d, tr, states, batches


def reference_links(gstate, dstate, mel, target, seed, step, settings, dtype, adversarial, wav_in=None, dwav_in=None):
    """One step's links in `dtype` on the CPU from the parameters `gstate`, `dstate`: the waveform; L_stft, its terms, p_fake, L_adv, L_D, its terms and the
    total d wav at the prediction `wav_in` (default: the reference's own waveform); the generator's gradients under the functional `dwav_in` (default: that
    total d wav); the discriminator's gradients of L_D at `wav_in` and the target."""
    from glow_tts_amd.pwg_trainer import noise_seed_words
    cfg, ds = config(), settings.get("Discriminator")
    leaves = {k: t.to(dtype).clone().requires_grad_(True) for k, t in gstate.items()}
    T = mel.shape[2] * HOP
    wav = torch.stack([P.generator(leaves, cfg, mel[i], P.seeded_noise(*noise_seed_words(seed, step, i), T), dtype) for i in range(mel.shape[0])])
    out = {"wav": wav.detach()}
    pred = (wav.detach() if wav_in is None else wav_in).to(dtype)
    r = TR.loss_and_grad(pred, target, settings["STFT_Resolutions"], dtype)
    out.update(L=r["L"], terms=r["terms"], dwav=r["dpred"])
    if adversarial:
        g = DR.score_grads(dstate, pred, 1.0, float(ds["Negative_Slope"]), dtype, factor=float(ds["Lambda_Adversarial"]))
        p = DR.pair_grads(dstate, target, pred, float(ds["Negative_Slope"]), dtype)
        out.update(p_fake=g["scores"], L_adv=g["loss"], dwav=r["dpred"] + g["dwav"], L_D=p["loss"], D_terms=p["terms"], dgrads=p["grads"])
    (wav * (out["dwav"] if dwav_in is None else dwav_in).to(dtype)).sum().backward()
    out["grads"] = {k: torch.zeros_like(t) if t.grad is None else t.grad.detach() for k, t in leaves.items()}
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
    from glow_tts_amd.vocoder import adversarial_mse
    adversarial = tr.adversarial(tr.steps)
    for p in tr.params + tr.disc_params:
        p.grad = None
    B, _, L = mel.shape
    wav, _ = tr.model.generate(mel.to(tr.device), [L] * B, seeds=tr.seeds(tr.steps, B))
    wav.retain_grad()
    stft = tr.criterion(wav, target.to(tr.device))
    links = {"wav": wav.detach().cpu(), "L": stft.detach().cpu().reshape(1), "terms": tr.criterion.terms.cpu().clone()}
    loss = stft
    if adversarial:
        both, p_fake = tr.discriminator.score_pair(target.to(tr.device), wav)
        adv, adv_terms = adversarial_mse(p_fake, 1.0, float(tr.disc_set["Lambda_Adversarial"]))
        d_loss, d_terms = adversarial_mse(both, (1.0, 0.0))
        loss = stft + adv
        launch_reset()
        loss.backward()
        counts = launch_counts()
        assert not any("disc_wgrad" in k and n for k, n in counts.items()), counts      # the generator term: the data chain alone
        assert all(p.grad is None for p in tr.disc_params)
        d_loss.backward()
        links.update(p_fake=p_fake.detach().cpu(), L_adv=adv_terms[:1].cpu(), L_D=d_loss.detach().cpu().reshape(1), D_terms=d_terms.cpu(),
                     dgrads={k: p.grad.detach().cpu().clone() for k, p in tr.discriminator.params.items()})
    else:
        loss.backward()
        assert all(p.grad is None for p in tr.disc_params)
    links.update(dwav=wav.grad.cpu().clone(), grads={k: p.grad.detach().cpu().clone() for k, p in tr.model.params.items()})
    got = tr.Train_Step(mel, target)
    assert torch.equal(got.cpu().reshape(1), loss.detach().cpu().reshape(1))
    if adversarial:
        assert torch.equal(tr.last["L_adv"].cpu().reshape(1), links["L_adv"]) and torch.equal(tr.last["Discriminator_Loss"].cpu().reshape(1), links["L_D"])
        assert torch.equal(tr.last["Real_Term"].cpu(), links["D_terms"][0]) and torch.equal(tr.last["Fake_Term"].cpu(), links["D_terms"][1])
    return links


def test_three_steps_match_the_float64_replay(corpus):
    root, d = corpus
    tr = trainer(d)
    last = "conv_layers.{}.conv1x1_out".format(config()["layers"] - 1)          # nothing reads the last layer's x': no gradient, no update
    names = [k for k in tr.model.params if not k.startswith(last)]
    dnames = list(tr.discriminator.params)
    opt = {dt: OptimizerReplay(names, tr.set, dt) for dt in (torch.float64, torch.float32)}
    dopt = {dt: OptimizerReplay(dnames, tr.disc_set, dt) for dt in (torch.float64, torch.float32)}
    failed, direct = [], []
    for step in range(STEPS):
        mel, target = tr.sampler["Train"].batch(step)
        before, dbefore, adversarial = state_of(tr), dstate_of(tr), step >= DISC["Start_Step"]
        dev = device_step(tr, mel, target)
        after, dafter = state_of(tr), dstate_of(tr)
        fed = {dt: reference_links(before, dbefore, mel, target, tr.seed, step, tr.set, dt, adversarial, wav_in=dev["wav"], dwav_in=dev["dwav"])
               for dt in (torch.float64, torch.float32)}
        r64, r32, tag = fed[torch.float64], fed[torch.float32], "step {}".format(step + 1)
        check_all(failed, tag + " (a)", dev, {"wav": r64["wav"]}, {"wav": r32["wav"]})
        keys = ("L", "terms") + (("p_fake", "L_adv", "L_D", "D_terms") if adversarial else ())
        check_all(failed, tag + " (b)", dev, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
        dwav_inside = TR.errors(r32["dwav"], r64["dwav"], r32["dwav"])[1] < 1e-3
        assert dwav_inside or step > 0, "the reference's d wav leaves the guard at the first step"
        if dwav_inside:
            check_all(failed, tag + " (b)", dev, {"dwav": r64["dwav"]}, {"dwav": r32["dwav"]})
        check_all(failed, tag + " (c)", dev["grads"], {k: r64["grads"][k] for k in names}, {k: r32["grads"][k] for k in names})
        u = {dt: opt[dt].update(before, {k: dev["grads"][k] for k in names}) for dt in opt}
        assert u[torch.float64][2] < 1.0, ("the generator's clipping is not active", u[torch.float64][1:])
        large = check_updates(failed, tag, names, before, after, u[torch.float64][0], u[torch.float32][0])
        assert all(torch.equal(after[k], before[k]) for k in before if k.startswith(last))
        dlarge = None
        if adversarial:
            check_all(failed, tag + " (c')", dev["dgrads"], r64["dgrads"], r32["dgrads"])
            du = {dt: dopt[dt].update(dbefore, dev["dgrads"]) for dt in dopt}
            assert du[torch.float64][2] < 1.0, ("the discriminator's clipping is not active", du[torch.float64][1:])
            dlarge = check_updates(failed, tag + " discriminator", dnames, dbefore, dafter, du[torch.float64][0], du[torch.float32][0])
            assert tr.disc_steps == dopt[torch.float64].step == step + 1 - DISC["Start_Step"]
        else:
            assert all(torch.equal(dafter[k], dbefore[k]) for k in dbefore) and tr.disc_steps == 0
        print("{}: d wav {} the guard; {} of {} generator updates and {} of {} discriminator updates above 1e-3".format(
            tag, "inside" if dwav_inside else "OUTSIDE", large, len(names), dlarge, len(dnames)))
        direct.append((dwav_inside, large, dlarge))
    assert not failed, failed
    assert tr.steps == STEPS and direct[0][0] and all(n >= UPDATES_ABOVE["generator"] for _, n, _ in direct)
    assert all(n >= UPDATES_ABOVE["discriminator"] for _, _, n in direct[DISC["Start_Step"]:])
    # the discriminator's rate follows its own update count
    assert tr.disc_learning_rate(0) == DISC["Learning_Rate"] and tr.disc_learning_rate(1) == DISC["Learning_Rate"] * 0.5


def test_the_first_step_is_stage_one_bit_for_bit(run, corpus):
    """Before Start_Step the generator's step is a block-less trainer's in every tensor, and the discriminator is not touched."""
    root, d = corpus
    _, tr, states, batches = run
    plain = trainer(hp_dict(root, disc=False))
    assert plain.discriminator is None
    loss = plain.Train_Step(*batches[0])
    assert all(torch.equal(v, states[0][0][k]) for k, v in state_of(plain).items())
    fresh = trainer(d)
    assert all(torch.equal(v, states[0][1][k]) for k, v in dstate_of(fresh).items())          # D after step 1 = D at construction (times DISC_SCALE)
    first = fresh.Train_Step(*batches[0])
    assert torch.equal(first, loss) and set(fresh.last) == set(plain.last) and fresh.disc_steps == 0
    assert any(not torch.equal(states[1][1][k], states[0][1][k]) for k in states[0][1])          # and it moves from Start_Step on


def test_three_steps_repeat_bit_for_bit(run, corpus):
    d, tr, states, batches = run
    assert tr.steps == STEPS and tr.disc_steps == STEPS - DISC["Start_Step"]
    assert all(torch.isfinite(tr.last[k]).all() for k in ("Loss", "STFT_Loss", "L_adv", "Real_Term", "Fake_Term", "Discriminator_Loss"))
    again = trainer(d)
    for mel, target in batches:
        again.Train_Step(mel, target)
    assert all(torch.equal(v, states[-1][0][k]) for k, v in state_of(again).items())
    assert all(torch.equal(v, states[-1][1][k]) for k, v in dstate_of(again).items())


def test_checkpoint_has_six_keys_loads_frozen_and_resumes(run, corpus):
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.vocoder import ParallelWaveGAN
    d, tr, states, batches = run
    # a checkpoint before Start_Step already carries the discriminator (initialised at construction); resuming from it crosses the boundary
    early = trainer(d)
    path0 = early.Save_Checkpoint()
    saved = torch.load(path0, map_location="cpu")
    assert set(saved) == {"generator", "Optimizer", "Steps", "discriminator", "Discriminator_Optimizer", "Discriminator_Steps"}
    assert saved["Steps"] == 0 and saved["Discriminator_Steps"] == 0
    early.Train_Step(*batches[0])
    path1 = early.Save_Checkpoint()
    resumed = trainer(d, steps=1)
    assert resumed.steps == 1 and resumed.disc_steps == 0
    for s in (1, 2):
        resumed.Train_Step(*resumed.sampler["Train"].batch(resumed.steps))
        assert all(torch.equal(v, states[s][0][k]) for k, v in state_of(resumed).items()), s
        assert all(torch.equal(v, states[s][1][k]) for k, v in dstate_of(resumed).items()), s
    # after the adversarial steps: six keys, the frozen vocoder reads it through Vocoder.Checkpoint_Path and reproduces the live generator
    path = tr.Save_Checkpoint()
    assert os.path.basename(path) == "PWG_{}.pt".format(STEPS)
    saved = torch.load(path, map_location="cpu")
    assert set(saved) == {"generator", "Optimizer", "Steps", "discriminator", "Discriminator_Optimizer", "Discriminator_Steps"}
    assert saved["Steps"] == STEPS and saved["Discriminator_Steps"] == STEPS - DISC["Start_Step"] and set(saved["discriminator"]) == set(states[-1][1])
    dd = copy.deepcopy(d)
    dd["Vocoder"]["Checkpoint_Path"] = path
    frozen = ParallelWaveGAN(Recursive_Parse(copy.deepcopy(dd)), "cuda:0")
    mel, _ = tr.sampler["Eval"].batch(0)
    z = torch.randn(mel.shape[0], FRAMES * HOP, generator=torch.Generator().manual_seed(1)).cuda()
    live = tr.model(mel.cuda(), [FRAMES] * BATCH, noises=z)[0].clone()
    assert torch.equal(frozen(mel.cuda(), [FRAMES] * BATCH, noises=z)[0], live)
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
