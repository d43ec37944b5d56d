"""GPU: both vocoder trainers with the yaml block `Vocoder.Train.Mel_Loss`, on the synthetic pattern directories and the narrow generators of
tests/test_gpu_pwg_trainer.py and tests/test_gpu_hifigan_gan_trainer.py (imported, with their float64 replays).  The method is theirs: a step is replayed on
the CPU FROM THE DEVICE'S OWN STATE before it and checked link by link, each link under the project's bar (`pwg_train_ref.check`): (a) the waveform; (b)
L_stft with its terms, L_mel (tests/mel_loss_ref.py), the loss L_stft + Lambda L_mel and the total d wav at the device's waveform - for HiFi-GAN's adversarial
step also every adversarial link of the helper module, where L_G carries Lambda L_mel and L_D, its two sums and the discriminator's gradients do not; (c)
every generator gradient under the device's d wav as the functional; (d) the update.  Without the block a trainer is today's: no mel launch, today's keys, and
two of them agree bit for bit.

The mel term at the generators' own waveforms: the replay asserts in float64 that every mel of the device's waveform and of the target stays above
10 x Floor, so no fp32 run decides the floor differently."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import mel_loss_ref as MR  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
import test_gpu_hifigan_gan_trainer as GT  # noqa: E402
import test_gpu_pwg_trainer as PT  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCK = {"Lambda": 4.5, "Floor": 1.0e-5}
MEL_LAUNCHES = ("mel_loss_fwd", "mel_loss_reduce", "mel_loss_bwd_frames", "mel_loss_bwd_fold")
HIFIGAN_GEO = dict(MR.DEFAULT, mel=12)                                          # the tiny Sound block: (2048, 256, 1024) x 12 at T = 8 * 256
PWG_GEO = dict(MR.SMALL, hop=PT.HOP, mel=12)                                    # T = 40 * 15 = 600 needs a short n_fft: (256, 15, 240) x 12


def with_block(d, block=BLOCK):
    d = copy.deepcopy(d)
    if block is not None:
        d["Vocoder"]["Train"]["Mel_Loss"] = dict(block)
    return d


@pytest.fixture(scope="module")
def hifigan(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("hifigan_mel"))
    for i, split in enumerate(("Train", "Eval")):
        GT.write_corpus(os.path.join(root, split), seed=i)
    return root


@pytest.fixture(scope="module")
def pwg(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pwg_mel"))
    for i, split in enumerate(("Train", "Eval")):
        PT.write_corpus(os.path.join(root, split), PT.config()["A"], seed=i)
    d = PT.hp_dict(root)
    d["Sound"].update(Spectrogram_Dim=PWG_GEO["n_fft"] // 2 + 1, Frame_Length=PWG_GEO["win"])
    return root, d


def mel_links(wav, target, geo, lam, r):
    """The helper module's links `r` of one dtype with the mel term added where the contract puts it"""
    dtype = r["L"].dtype
    m = MR.loss_and_grad(wav, target, geo, dtype)
    out = dict(r, L_mel=m["L"], L_base=r["L"] + lam * m["L"], L_G=r["L_G"] + lam * m["L"], dwav=r["dwav"] + lam * m["dpred"])
    return out, min(m["low_pred"], m["low_target"])


def device_head(tr, mel, target):
    """The loss of `PWG_Trainer.forward` through the trainer's own parts -> (wav with its gradient retained, L_stft + Lambda L_mel, the links so far)"""
    dev = tr.device
    B, _, L = mel.shape
    wav = tr.generate(mel.to(dev), [L] * B, tr.steps)
    wav.retain_grad()
    stft = tr.criterion(wav, target.to(dev))
    terms = tr.criterion.terms.cpu().clone()
    base = stft + float(tr.mel_set["Lambda"]) * tr.mel_criterion(wav, target.to(dev))
    links = {"wav": wav.detach().cpu(), "L": stft.detach().cpu().reshape(1), "terms": terms, "L_mel": tr.mel_criterion.term.cpu().reshape(1),
             "L_base": base.detach().cpu().reshape(1)}
    return wav, base, links


def test_hifigan_steps_match_the_float64_replay(hifigan):
    """Step 1 is stage one, step 2 adversarial (Start_Step = 1)"""
    tr = GT.trainer(with_block(GT.hp_dict(hifigan, name="mel")))
    assert tr.mel_criterion.geo == HIFIGAN_GEO and tr.mel_set == dict(BLOCK, Mel_F_Min=125, Mel_F_Max=7600)
    lam, n = BLOCK["Lambda"], len(GT.CHANNELS)
    names, dnames = list(tr.model.params), list(tr.discriminator.params)
    opt = {dt: GT.OptimizerReplay(names, tr.set, dt) for dt in (torch.float64, torch.float32)}
    dopt = {dt: GT.OptimizerReplay(dnames, tr.disc_set, dt) for dt in (torch.float64, torch.float32)}
    failed = []
    for step in range(2):
        mel, target = tr.sampler["Train"].batch(step)
        before, dbefore, adversarial = GT.state_of(tr), GT.dstate_of(tr), step >= GT.ADV["Start_Step"]
        for p in tr.params + tr.disc_params:
            p.grad = None
        wav, loss, dev = device_head(tr, mel, target)
        if adversarial:
            loss, d_loss, adv_terms, _ = tr.adversarial_losses(target.to(tr.device), wav, loss)
            l_fm, fm_terms = tr.fm
            loss.backward()
            assert all(p.grad is None for p in tr.disc_params)                 # L_G, the mel term in it, reaches the generator alone
            d_loss.backward()
            dev.update(adv=adv_terms[:1].cpu(), L_fm=l_fm.cpu().reshape(1), fm_terms=fm_terms.cpu(), L_D=d_loss.detach().cpu().reshape(1),
                       D_terms=adv_terms[1:].cpu(), dgrads={k: p.grad.detach().cpu().clone() for k, p in tr.discriminator.params.items()})
            dev.update({"p_fake[{}]".format(i): s.detach().cpu() for i, s in enumerate(tr.discriminator.score(wav.detach(), freeze=True))})
        else:
            loss.backward()
        dev.update(L_G=loss.detach().cpu().reshape(1), dwav=wav.grad.cpu().clone(), grads={k: p.grad.detach().cpu().clone() for k, p in tr.model.params.items()})
        launch_reset()
        got = tr.Train_Step(mel, target)                                       # the very step: everything is deterministic
        counts = launch_counts()
        assert all(counts.get(k) == 1 for k in MEL_LAUNCHES), counts
        assert torch.equal(got.cpu().reshape(1), dev["L_G"]) and torch.equal(tr.last["Mel_Loss"].cpu().reshape(1), dev["L_mel"])
        if adversarial:
            assert torch.equal(tr.last["Discriminator_Loss"].cpu().reshape(1), dev["L_D"]) and torch.equal(tr.last["STFT_Loss"].cpu().reshape(1), dev["L_base"])
        after, dafter = GT.state_of(tr), GT.dstate_of(tr)
        ref = {}
        for dt in (torch.float64, torch.float32):
            ref[dt], low = mel_links(dev["wav"], target, HIFIGAN_GEO, lam,
                                     GT.reference_links(before, dbefore, mel, target, tr.set, dt, adversarial, dev["wav"], dev["dwav"]))
            assert low > 10 * HIFIGAN_GEO["floor"], low
        r64, r32, tag = ref[torch.float64], ref[torch.float32], "hifigan step {}".format(step + 1)
        GT.check_all(failed, tag + " (a)", dev, {"wav": r64["wav"]}, {"wav": r32["wav"]})
        keys = ("L", "terms", "L_mel", "L_base", "L_G") + \
            (tuple("p_fake[{}]".format(i) for i in range(len(GT.PERIODS))) + ("adv", "L_fm", "fm_terms", "L_D", "D_terms") if adversarial else ())
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
            GT.check_all(failed, tag + " (c')", dev["dgrads"], r64["dgrads"], r32["dgrads"])      # the reference's L_D knows no mel term
            du = {dt: dopt[dt].update(dbefore, dev["dgrads"]) for dt in dopt}
            GT.check_updates(failed, tag + " discriminator", dnames, dbefore, dafter, du[torch.float64][0], du[torch.float32][0])
        else:
            assert all(torch.equal(dafter[k], dbefore[k]) for k in dbefore) and tr.disc_steps == 0
    assert not failed, failed
    assert tr.steps == 2 and tr.disc_steps == 1


def test_pwg_step_matches_the_float64_replay(pwg):
    root, d = pwg
    tr = PT.trainer(with_block(d))
    assert tr.mel_criterion.geo == PWG_GEO
    lam = BLOCK["Lambda"]
    last = "conv_layers.{}.conv1x1_out".format(PT.config()["layers"] - 1)        # nothing reads the last layer's x': no gradient, no update
    names = [k for k in tr.model.params if not k.startswith(last)]
    opt = {dt: PT.OptimizerReplay(names, tr.set, dt) for dt in (torch.float64, torch.float32)}
    mel, target = tr.sampler["Train"].batch(0)
    before = PT.state_of(tr)
    for p in tr.params:
        p.grad = None
    wav, loss, dev = device_head(tr, mel, target)
    loss.backward()
    dev.update(L_G=loss.detach().cpu().reshape(1), dwav=wav.grad.cpu().clone(), grads={k: p.grad.detach().cpu().clone() for k, p in tr.model.params.items() if k in names})
    launch_reset()
    got = tr.Train_Step(mel, target)
    counts = launch_counts()
    assert all(counts.get(k) == 1 for k in MEL_LAUNCHES), counts
    assert torch.equal(got.cpu().reshape(1), dev["L_G"]) and torch.equal(tr.last["Mel_Loss"].cpu().reshape(1), dev["L_mel"])
    assert set(tr.last) == {"Loss", "Terms", "Gradient_Norm", "Mel_Loss"}
    after = PT.state_of(tr)
    ref = {}
    for dt in (torch.float64, torch.float32):
        r = PT.reference_links(before, mel, target, tr.seed, 0, tr.set, dt, wav_in=dev["wav"], dwav_in=dev["dwav"])
        ref[dt], low = mel_links(dev["wav"], target, PWG_GEO, lam, dict(r, L_G=r["L"]))
        assert low > 10 * PWG_GEO["floor"], low
    r64, r32, failed = ref[torch.float64], ref[torch.float32], []
    for tag, keys in ((" (a)", ("wav",)), (" (b)", ("L", "terms", "L_mel", "L_base", "L_G", "dwav"))):
        PT.check_all(failed, "pwg step 1" + tag, dev, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
    PT.check_all(failed, "pwg step 1 (c)", dev["grads"], {k: r64["grads"][k] for k in names}, {k: r32["grads"][k] for k in names})
    u = {dt: opt[dt].update(before, dev["grads"]) for dt in opt}
    assert u[torch.float64][2] < 1.0, ("the clipping is not active", u[torch.float64][1:])
    GT.check_updates(failed, "pwg step 1", names, before, after, u[torch.float64][0], u[torch.float32][0])
    assert not failed, failed
    # the evaluation: the return value keeps its shape, the mean mel term is on the trainer
    ev = tr.Evaluation(batches=2)
    assert len(ev) == 2 and ev[1].shape == (len(PT.RESOLUTIONS), 2) and tr.last_evaluation_mel > 0
    saved = torch.load(tr.Save_Checkpoint(), map_location="cpu")
    assert set(saved) == {"generator", "Optimizer", "Steps"}                     # the loss has no state


@pytest.mark.parametrize("kind", ["hifigan", "pwg"])
def test_without_the_block_nothing_changes(kind, hifigan, pwg):
    if kind == "hifigan":
        make, d, state = GT.trainer, GT.hp_dict(hifigan, adversarial=False, name="mel_blockless"), GT.state_of
    else:
        make, d, state = PT.trainer, copy.deepcopy(pwg[1]), PT.state_of
        d["Vocoder"]["Train"]["Checkpoint_Path"] = os.path.join(pwg[0], "pwg_blockless")
    a, b, c = make(d), make(d), make(with_block(d))
    assert a.mel_criterion is None and a.mel_set is None and "Mel_Loss" not in a.set and set(c.set) == set(a.set) | {"Mel_Loss"}
    launch_reset()
    for s in range(2):
        la, lb = a.Train_Step(*a.sampler["Train"].batch(s)), b.Train_Step(*b.sampler["Train"].batch(s))
        assert torch.equal(la, lb) and set(a.last) == {"Loss", "Terms", "Gradient_Norm"}
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.params, b.params) if p.grad is not None)
    plain = {k: n for k, n in launch_counts().items() if n}
    assert not any("mel_loss" in k for k in plain), plain
    assert all(torch.equal(v, state(b)[k]) for k, v in state(a).items())
    launch_reset()
    lc = c.Train_Step(*c.sampler["Train"].batch(0))
    assert {k: n for k, n in launch_counts().items() if "mel_loss" in k} == dict.fromkeys(MEL_LAUNCHES, 1)
    assert set(c.last) == set(a.last) | {"Mel_Loss"} and float(lc) > 0 and float(c.last["Mel_Loss"]) > 0
    saved, with_mel = torch.load(a.Save_Checkpoint(), map_location="cpu"), torch.load(c.Save_Checkpoint(), map_location="cpu")
    assert set(saved) == set(with_mel) == {"generator", "Optimizer", "Steps"} and saved["Steps"] == 2
    assert a.Evaluation(batches=1) is not None and a.last_evaluation_mel is None
