"""GPU: the HiFi-GAN trainer (glow_tts_amd/hifigan_trainer.py, Train_HiFiGAN.py) on a synthetic pattern directory with the small generator `TINY` of
tests/test_gpu_hifigan.py.  The method is tests/test_gpu_pwg_trainer.py's, with the same bar, link by link: every step is replayed in float64 on the CPU FROM
THE DEVICE'S OWN STATE before it - (a) the waveform; (b) the loss, its terms and d wav at the device's waveform; (c) every parameter gradient of the restatement
under the device's d wav as the functional; (d) every update through the replay of clipping, RAdam and the decayed rate fed with the device's gradients.
d wav is held to the bar wherever the reference's own float32 run stays inside the guard e32 < 1e-3 (the 1 / |X| of L_mag), which it must at the first step."""
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

import hifigan_train_ref as R  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
import test_gpu_hifigan as G  # noqa: E402
import test_gpu_pwg_trainer as PT  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, BATCH, FRAMES, SEED = 3, 2, 8, 5
HOP = 256                                                                   # the tiny model's Frame_Shift = prod(TINY rates)
# The first steps of RAdam are unrectified: an update is -rate times the bias-corrected mean of the clipped gradients, so its norm is rate * bound = 1 while
# the clipping is active (asserted): large enough that float32's rounding of a parameter stays far below its update.
LEARNING_RATE, GRADIENT_NORM = 10.0, 0.1


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


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("hifigan_train"))
    for i, split in enumerate(("Train", "Eval")):
        write_corpus(os.path.join(root, split), seed=i)
    d = tiny_hp_dict("Vanilla")
    assert d["Sound"]["Frame_Shift"] == HOP
    d["Vocoder"] = G.block_of(G.TINY, Train={"Batch_Size": BATCH, "Segment_Frames": FRAMES, "Learning_Rate": LEARNING_RATE, "Gradient_Norm": GRADIENT_NORM,
                                             "STFT_Resolutions": [list(r) for r in PT.RESOLUTIONS], "Learning_Rate_Decay": {"Step": 2, "Gamma": 0.5},
                                             "Max_Step": 4, "Checkpoint_Save_Interval": 2, "Evaluation_Interval": 2,
                                             "Checkpoint_Path": os.path.join(root, "hifigan")})
    for split, key in (("Train", "Train_Pattern"), ("Eval", "Eval_Pattern")):
        d["Train"][key].update(Path=os.path.join(root, split), Metadata_File="METADATA.PICKLE")
    return root, d


def trainer(d, steps=0):
    from glow_tts_amd.hifigan_trainer import HiFiGAN_Trainer
    from glow_tts_amd.hparams import Recursive_Parse
    return HiFiGAN_Trainer(steps=steps, hp=Recursive_Parse(copy.deepcopy(d)), seed=SEED)


def reference_links(state, mel, target, settings, dtype, wav_in, dwav_in):
    wavs, grads = R.generator_grads(state, G.TINY, list(mel), list(dwav_in), dtype)
    r = TR.loss_and_grad(wav_in.to(dtype), target, settings["STFT_Resolutions"], dtype)
    return {"wav": torch.stack(wavs), "L": r["L"], "terms": r["terms"], "dwav": r["dpred"], "grads": grads}


def test_three_steps_match_the_float64_replay(corpus):
    root, d = corpus
    tr = trainer(d)
    names = list(tr.model.params)
    opt = {dt: PT.OptimizerReplay(names, tr.set, dt) for dt in (torch.float64, torch.float32)}
    failed = []
    for step in range(STEPS):
        mel, target = tr.sampler["Train"].batch(step)
        before = PT.state_of(tr)
        for p in tr.params:
            p.grad = None
        wav, _ = tr.model.generate(mel.to(tr.device), [FRAMES] * BATCH)
        wav.retain_grad()
        loss = tr.criterion(wav, target.to(tr.device))
        loss.backward()
        grads = {k: p.grad.detach().cpu().clone() for k, p in tr.model.params.items()}
        wav_d, L, terms, dwav = wav.detach().cpu(), loss.detach().cpu().reshape(1), tr.criterion.terms.cpu().clone(), wav.grad.cpu().clone()
        assert torch.equal(tr.Train_Step(mel, target).cpu().reshape(1), L)   # the very step: everything is deterministic
        after = PT.state_of(tr)
        r64, r32 = (reference_links(before, mel, target, tr.set, dt, wav_d, dwav) for dt in (torch.float64, torch.float32))
        tag = "step {}".format(step + 1)
        PT.check_all(failed, tag + " (a)", {"wav": wav_d}, {"wav": r64["wav"]}, {"wav": r32["wav"]})
        PT.check_all(failed, tag + " (b)", {"L": L, "terms": terms}, {k: r64[k] for k in ("L", "terms")}, {k: r32[k] for k in ("L", "terms")})
        dwav_inside = TR.errors(r32["dwav"], r64["dwav"], r32["dwav"])[1] < 1e-3
        assert dwav_inside or step > 0, "the reference's d wav leaves the guard at the first step"
        if dwav_inside:
            PT.check_all(failed, tag + " (b)", {"dwav": dwav}, {"dwav": r64["dwav"]}, {"dwav": r32["dwav"]})
        PT.check_all(failed, tag + " (c)", grads, r64["grads"], r32["grads"])
        u = {dt: opt[dt].update(before, grads) for dt in opt}
        assert u[torch.float64][2] < 1.0, ("the clipping is not active", u[torch.float64][1:])
        for k in names:                                                      # (d): the bar's inequality and its e32 guard for every tensor
            err, e32, scale = TR.errors(after[k].double() - before[k].double(), u[torch.float64][0][k], u[torch.float32][0][k])
            print("{} (d) update of {}: err {:.3e}  e32 {:.3e}  max|ref| {:.3e}".format(tag, k, err, e32, scale))
            assert 0 < e32 < 1e-3 and scale > 0, (tag, k, e32, scale)
            if err > 4 * e32 + 1e-6:
                failed.append(str((tag + " (d) update of " + k, err, e32)))
    assert not failed, failed
    assert tr.steps == STEPS and tr.learning_rate(1) == LEARNING_RATE and tr.learning_rate(2) == LEARNING_RATE * 0.5


def test_resume_checkpoint_and_command_line(corpus, tmp_path):
    import yaml
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.vocoder import HiFiGAN
    import Train_HiFiGAN
    root, d = corpus
    whole = trainer(d)
    for s in range(3):
        whole.Train_Step(*whole.sampler["Train"].batch(s))
    first = trainer(d)
    for s in range(2):
        first.Train_Step(*first.sampler["Train"].batch(s))
    assert os.path.basename(first.Save_Checkpoint()) == "HIFIGAN_2.pt"
    resumed = trainer(d, steps=2)
    assert resumed.steps == 2
    resumed.Train_Step(*resumed.sampler["Train"].batch(2))
    assert all(torch.equal(v, PT.state_of(whole)[k]) for k, v in PT.state_of(resumed).items())
    path = resumed.Save_Checkpoint()
    saved = torch.load(path, map_location="cpu")
    assert os.path.basename(path) == "HIFIGAN_3.pt" and set(saved) == {"generator", "Optimizer", "Steps"} and saved["Steps"] == 3
    dd = copy.deepcopy(d)
    dd["Vocoder"]["Checkpoint_Path"] = path
    frozen = HiFiGAN(Recursive_Parse(dd), "cuda:0")
    mel, _ = whole.sampler["Eval"].batch(0)
    live = whole.model.generate(mel.cuda(), [FRAMES] * BATCH)[0].detach()
    assert torch.equal(frozen(mel.cuda(), [FRAMES] * BATCH)[0], live) and torch.equal(whole.model(mel.cuda(), [FRAMES] * BATCH)[0], live)
    # the command line: two steps from scratch into a directory of its own
    cl = copy.deepcopy(d)
    cl["Vocoder"]["Train"].update(Max_Step=2, Checkpoint_Path=str(tmp_path / "cl"))
    with open(tmp_path / "hp.yaml", "w") as f:
        yaml.dump(cl, f)
    Train_HiFiGAN.main(["-hp", str(tmp_path / "hp.yaml"), "--seed", str(SEED)])
    made = torch.load(str(tmp_path / "cl" / "HIFIGAN_2.pt"), map_location="cpu")
    assert made["Steps"] == 2 and all(torch.equal(made["generator"][k], v) for k, v in PT.state_of(first).items())
