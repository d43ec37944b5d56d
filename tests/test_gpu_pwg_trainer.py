"""GPU: the Parallel WaveGAN trainer (glow_tts_amd/pwg_trainer.py, Train_PWG.py) on a synthetic pattern directory: three `Train_Step`s against a float64
replay on the CPU (tests/pwg_ref.py's generator under autograd, the library-STFT loss of tests/pwg_train_ref.py, oracle/radam_ref.py, the same clipping and
decay) under the project's bar, the checkpoint through `Vocoder.Checkpoint_Path` and `Inferencer.Vocode`, and resuming.

How the replay is conditioned.  The composed gradient d loss / d parameter inherits the 1 / |X| of L_mag at the small high-frequency bins of a generator's
coloured output: the float32 run of the reference alone is 1e-3 .. 5e-3 off its float64 run on many tensors, outside the bar's guard e32 < 1e-3, and a
chained float32 replay drifts further with every step.  So every step is replayed FROM THE DEVICE'S OWN STATE before it and checked link by link, each link
under the bar: (a) the waveform (noise seeds, step index, weights in use); (b) the loss, its terms and d wav at the device's waveform (target pairing, the
loss); (c) every parameter gradient of the reference generator under the device's d wav as the functional (the backward, and its composition with the loss:
the device's gradients must be the generator's transposed Jacobian applied to the device's own d wav, so (b) and (c) leave no gap and no sign free); (d) every
parameter's update against the replay of clipping, RAdam and the decayed rate fed with the device's gradients (rate, epsilon, clipping and decay as the
kernel received them).  Guards: (a), (b)'s loss and terms and (c) hold the bar's guards at every step.  d wav holds them at the first step (asserted) and is
held to the bar at later steps when the reference's own float32 run stays inside e32 < 1e-3 there.  The updates hold the inequality and the e32 guard for
every tensor; max |ref64| > 1e-3 holds for at least 30 of the 35 tensors at every step (asserted) - a rate at which the smallest gradients would clear it too
moves the generator so far in two steps that no link stays conditioned - and every update is nonzero.
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

import pwg_ref as P  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
from helpers import load_case, tiny_hp_dict  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, BATCH, FRAMES, HOP, SEED = 3, 3, 40, 15, 5
RESOLUTIONS = [(256, 50, 240), (512, 120, 400)]
# The first steps of RAdam are unrectified: an update is -rate times the bias-corrected mean of the clipped gradients.  The norm bound is below the gradient
# norm of every step, so the clipping is active (asserted).
LEARNING_RATE, GRADIENT_NORM = 1.0, 1.0


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


def hp_dict(root):
    cfg = config()
    d = tiny_hp_dict("Vanilla")
    d["Sound"]["Frame_Shift"] = HOP
    d["Vocoder"] = {"Type": "PWG", "Layers": cfg["layers"], "Stacks": cfg["stacks"], "Residual_Channels": cfg["R"], "Gate_Channels": cfg["G"],
                    "Skip_Channels": cfg["S"], "Upsample_Scales": list(cfg["scales"]),
                    "Train": {"Batch_Size": BATCH, "Segment_Frames": FRAMES, "Learning_Rate": LEARNING_RATE, "Gradient_Norm": GRADIENT_NORM,
                              "STFT_Resolutions": [list(r) for r in RESOLUTIONS], "Learning_Rate_Decay": {"Step": 2, "Gamma": 0.5},
                              "Max_Step": 4, "Checkpoint_Save_Interval": 2, "Evaluation_Interval": 2, "Checkpoint_Path": os.path.join(root, "pwg")}}
    for split, key in (("Train", "Train_Pattern"), ("Eval", "Eval_Pattern")):
        d["Train"][key].update(Path=os.path.join(root, split), Metadata_File="METADATA.PICKLE")
    return d


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pwg_train"))
    for i, split in enumerate(("Train", "Eval")):
        write_corpus(os.path.join(root, split), config()["A"], seed=i)
    return root, hp_dict(root)


def trainer(d, steps=0):
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.pwg_trainer import PWG_Trainer
    return PWG_Trainer(steps=steps, hp=Recursive_Parse(copy.deepcopy(d)), seed=SEED)


def state_of(tr):
    return {k: v.detach().cpu().clone() for k, v in tr.model.params.items()}


@pytest.fixture(scope="module")
def run(corpus):
    """-> (hp dict, the trainer after STEPS steps, its start state, its states after each step, the batches)"""
    root, d = corpus
    tr = trainer(d)
    start = state_of(tr)
    batches = [tr.sampler["Train"].batch(s) for s in range(STEPS)]
    states = []
    for mel, target in batches:
        tr.Train_Step(mel, target)
        states.append(state_of(tr))
    torch.cuda.synchronize()
    return d, tr, start, states, batches


def reference_links(state, mel, target, seed, step, settings, dtype, wav_in=None, dwav_in=None):
    """One step's links in `dtype` on the CPU from the parameters `state`: the waveform; the loss, its terms and d wav at the prediction `wav_in` (default:
    the reference's own waveform); the parameter gradients under the functional `dwav_in` (default: composed with the loss by autograd)."""
    from glow_tts_amd.pwg_trainer import noise_seed_words
    cfg = config()
    leaves = {k: t.to(dtype).clone().requires_grad_(True) for k, t in state.items()}
    T = mel.shape[2] * HOP
    wav = torch.stack([P.generator(leaves, cfg, mel[i], P.seeded_noise(*noise_seed_words(seed, step, i), T), dtype) for i in range(mel.shape[0])])
    out = {"wav": wav.detach()}
    pred = (wav.detach() if wav_in is None else wav_in).to(dtype)
    r = TR.loss_and_grad(pred, target, settings["STFT_Resolutions"], dtype)
    out.update(L=r["L"], terms=r["terms"], dwav=r["dpred"])
    if dwav_in is None:
        TR.stft_loss(wav, target, settings["STFT_Resolutions"], dtype)[0].backward()
    else:
        (wav * dwav_in.to(dtype)).sum().backward()
    out["grads"] = {k: torch.zeros_like(t) if t.grad is None else t.grad.detach() for k, t in leaves.items()}
    return out


class OptimizerReplay:
    """Clipping, RAdam (oracle/radam_ref.py's scalars) and the step decay in `dtype`, fed with given gradients"""

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


def replay_steps(tr, batches, device_step):
    """The link-by-link replay of `len(batches)` steps of the trainer `tr`; `device_step(mel, target)` -> (wav, L, terms, d wav, unclipped gradients, the
    state after the step) runs the step under test.  Returns the failures of the bar and, per step, (d wav inside its guard, updates above 1e-3)."""
    last = "conv_layers.{}.conv1x1_out".format(config()["layers"] - 1)          # nothing reads the last layer's x': no gradient, no update
    names = [k for k in tr.model.params if not k.startswith(last)]
    opt = {dt: OptimizerReplay(names, tr.set, dt) for dt in (torch.float64, torch.float32)}
    failed, direct = [], []
    for step, (mel, target) in enumerate(batches):
        before = state_of(tr)
        wav, L, terms, dwav, grads, after = device_step(mel, target)
        fed = {dt: reference_links(before, mel, target, tr.seed, step, tr.set, dt, wav_in=wav, dwav_in=dwav) for dt in (torch.float64, torch.float32)}
        r64, r32, tag = fed[torch.float64], fed[torch.float32], "step {}".format(step + 1)
        check_all(failed, tag + " (a)", {"wav": wav}, {"wav": r64["wav"]}, {"wav": r32["wav"]})
        check_all(failed, tag + " (b)", {"L": L, "terms": terms}, {k: r64[k] for k in ("L", "terms")}, {k: r32[k] for k in ("L", "terms")})
        # d wav: the 1 / |X| of L_mag makes the reference's own float32 run erratic once the stepped generator's waveform has tiny bins; the bar applies
        # wherever its guard holds, and it must hold at the first step (the initialised generator: a wide margin)
        dwav_inside = TR.errors(r32["dwav"], r64["dwav"], r32["dwav"])[1] < 1e-3
        assert dwav_inside or step > 0, "the reference's d wav leaves the guard at the first step"
        if dwav_inside:
            check_all(failed, tag + " (b)", {"dwav": dwav}, {"dwav": r64["dwav"]}, {"dwav": r32["dwav"]})
        check_all(failed, tag + " (c)", grads, {k: r64["grads"][k] for k in names}, {k: r32["grads"][k] for k in names})
        u = {dt: opt[dt].update(before, {k: grads[k].cpu() for k in names}) for dt in opt}
        assert u[torch.float64][2] < 1.0, ("the clipping is not active", u[torch.float64][1:])
        large = 0
        for k in names:                                                      # (d): the bar's inequality and its e32 guard for every tensor
            err, e32, scale = TR.errors(after[k].double() - before[k].double(), u[torch.float64][0][k], u[torch.float32][0][k])
            print("{} (d) update of {}: err {:.3e}  e32 {:.3e}  ratio {:.3f}  max|ref| {:.3e}".format(tag, k, err, e32, err / (4 * e32 + 1e-6), scale))
            assert 0 < e32 < 1e-3 and scale > 0, (tag, k, e32, scale)
            if err > 4 * e32 + 1e-6:
                failed.append(str((tag + " (d) update of " + k, err, e32)))
            large += scale > 1e-3
        assert all(torch.equal(after[k], before[k]) for k in before if k.startswith(last))
        print("{}: d wav {} the guard; {} of {} updates above 1e-3; norm {:.3f}, clip {:.3f}".format(tag, "inside" if dwav_inside else "OUTSIDE", large, len(names),
                                                                                                  *u[torch.float64][1:]))
        direct.append((dwav_inside, large))
    return failed, direct


def test_three_steps_match_the_float64_replay(corpus):
    root, d = corpus
    tr = trainer(d)

    def device_step(mel, target):
        """The step's links through the trainer's own parts, then the very `Train_Step` (bit-identical arithmetic: everything is deterministic)"""
        for p in tr.params:
            p.grad = None
        B, _, L = mel.shape
        wav, _ = tr.model.generate(mel.to(tr.device), [L] * B, seeds=tr.seeds(tr.steps, B))
        wav.retain_grad()
        loss = tr.criterion(wav, target.to(tr.device))
        loss.backward()
        grads = {k: p.grad.detach().cpu().clone() for k, p in tr.model.params.items()}
        links = wav.detach().cpu(), loss.detach().cpu().reshape(1), tr.criterion.terms.cpu().clone(), wav.grad.cpu().clone()
        got = tr.Train_Step(mel, target)
        assert torch.equal(got.cpu().reshape(1), links[1])
        return links + (grads, state_of(tr))

    batches = [tr.sampler["Train"].batch(s) for s in range(STEPS)]
    failed, direct = replay_steps(tr, batches, device_step)
    assert not failed, failed
    assert tr.steps == STEPS and direct[0][0] and all(n >= 30 for _, n in direct)      # of 35 tensors that have a gradient


def test_three_steps_repeat_bit_for_bit(run, corpus):
    """A second trainer repeats the run bit for bit (the batches and the noise are functions of (seed, step)), and the rate follows the step decay."""
    d, tr, start, states, batches = run
    assert tr.steps == STEPS and tr.learning_rate(1) == LEARNING_RATE and tr.learning_rate(2) == LEARNING_RATE * 0.5
    assert torch.isfinite(tr.last["Loss"]) and tr.last["Terms"].shape == (len(RESOLUTIONS), 2)
    again = trainer(d)
    for mel, target in batches:
        again.Train_Step(mel, target)
    assert all(torch.equal(v, states[-1][k]) for k, v in state_of(again).items())


def test_checkpoint_loads_through_the_vocoder_block_and_resumes(run, corpus, tmp_path):
    import yaml
    from scipy.io import wavfile
    from glow_tts_amd import data
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.inferencer import Inferencer
    from glow_tts_amd.vocoder import ParallelWaveGAN
    d, tr, _, states, _ = run
    path = tr.Save_Checkpoint()
    assert os.path.basename(path) == "PWG_{}.pt".format(STEPS)
    saved = torch.load(path, map_location="cpu")
    assert set(saved) == {"generator", "Optimizer", "Steps"} and saved["Steps"] == STEPS and set(saved["generator"]) == set(states[-1])
    # the frozen vocoder reads it through Vocoder.Checkpoint_Path and reproduces the live generator
    dd = copy.deepcopy(d)
    dd["Vocoder"]["Checkpoint_Path"] = path
    frozen = ParallelWaveGAN(Recursive_Parse(copy.deepcopy(dd)), "cuda:0")
    mel, _ = tr.sampler["Eval"].batch(0)
    z = torch.randn(mel.shape[0], FRAMES * HOP, generator=torch.Generator().manual_seed(1)).cuda()
    live = tr.model(mel.cuda(), [FRAMES] * BATCH, noises=z)[0].clone()       # the inference call of the trainable generator follows the stepped parameters
    assert torch.equal(frozen(mel.cuda(), [FRAMES] * BATCH, noises=z)[0], live)
    assert torch.equal(live, tr.model.generate(mel.cuda(), [FRAMES] * BATCH, noises=z)[0].detach())
    # Inferencer.Vocode writes a wav with it
    sd, _, _ = load_case("tiny_vanilla.npz")
    torch.save({"Model": sd, "Steps": 0}, str(tmp_path / "S_0.pt"))
    dd["Token_Path"] = str(tmp_path / "Token.yaml")
    with open(dd["Token_Path"], "w") as f:
        yaml.dump(data.make_token_dict(["HELLO WORLD."]), f)
    inf = Inferencer(str(tmp_path / "S_0.pt"), hp=Recursive_Parse(copy.deepcopy(dd)))
    assert inf.vocoder_kind == "pwg"
    files = inf.Vocode(["A"], [mel[0].T.numpy()], str(tmp_path / "voc"))
    sr, y = wavfile.read(files[0])
    assert y.shape == (FRAMES * HOP,) and np.abs(y.astype(np.int32)).max() > 0
    # a resumed run continues bit-identically to the uninterrupted one over two more steps
    resumed = trainer(d, steps=STEPS)
    assert resumed.steps == STEPS and all(torch.equal(v, states[-1][k]) for k, v in state_of(resumed).items())
    for _ in range(2):
        nxt = tr.sampler["Train"].batch(tr.steps)
        resumed.Train_Step(*resumed.sampler["Train"].batch(resumed.steps))
        tr.Train_Step(*nxt)
        a, b = state_of(tr), state_of(resumed)
        assert all(torch.equal(a[k], b[k]) for k in a)
    ev = tr.Evaluation(batches=2)
    assert ev is not None and np.isfinite(ev[0]) and ev[1].shape == (len(RESOLUTIONS), 2)
