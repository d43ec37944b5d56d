"""GPU suite of the neural vocoder (glow_tts_amd/vocoder.py: ParallelWaveGAN on csrc/pwg_ops.hip) against the float64 restatement tests/pwg_ref.py.

Weights: torch's default Conv initialisation under a fixed seed; mels uniform in [-4, 4].  THE BAR (no closed bound exists for 30 chained layers, so it is
measured on the reference arithmetic, never on the code under test): every case also runs the restatement in float32 on the CPU; with
e32 = max |ref32 - ref64| / max |ref64| the HIP result must satisfy  max |hip - ref64| / max |ref64| <= 4 * e32 + 1e-6  (4: the exact-f32 MFMA sums the
same products in another order than torch's CPU conv; 1e-6: a floor for cases whose e32 happens to be tiny).  Guard against degenerate inputs:
0 < e32 < 1e-3 and max |ref64| > 1e-3.  The observed ratio err / e32 of every case is printed before it is asserted (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import pwg_ref as P  # noqa: E402
from helpers import launch_counts, launch_reset, load_case, tiny_hp_dict  # noqa: E402

gpu = pytest.mark.gpu

ODD = dict(P.DEFAULT, layers=10, stacks=1, scales=[3, 5])                    # default widths, hop 15, dilations 1 .. 512
CFGS = {"default": P.DEFAULT, "narrow": P.NARROW, "odd": ODD}
WEIGHT_SEED = 1234
RAGGED = [5, 2, 7]
_VOC, _SD = {}, {}


def _hp(cfg):
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    d = load_yaml(DEFAULT_YAML)
    d["Sound"].update(Mel_Dim=cfg["A"], Frame_Shift=P.hop(cfg))
    d["Vocoder"] = {"Type": "PWG", "Layers": cfg["layers"], "Stacks": cfg["stacks"], "Residual_Channels": cfg["R"], "Gate_Channels": cfg["G"],
                    "Skip_Channels": cfg["S"], "Aux_Context_Window": cfg["ctx"], "Upsample_Scales": list(cfg["scales"])}
    return Recursive_Parse(d)


def sd_of(name):
    if name not in _SD:
        _SD[name] = P.random_state_dict(CFGS[name], WEIGHT_SEED)
    return _SD[name]


def voc(name):
    from glow_tts_amd.vocoder import ParallelWaveGAN
    if name not in _VOC:
        _VOC[name] = ParallelWaveGAN(_hp(CFGS[name]), "cuda:0", state_dict={"generator": sd_of(name)})
    return _VOC[name]


def check(tag, got, ref64, ref32):
    err, e32 = P.errors(got.cpu(), ref64, ref32)
    print(f"{tag}: err {err:.3e}  e32 {e32:.3e}  ratio {err / e32:.2f}  max|ref| {float(ref64.abs().max()):.3e}")
    assert 0 < e32 < 1e-3 and float(ref64.abs().max()) > 1e-3, "degenerate case"
    assert err <= 4 * e32 + 1e-6, tag
    return err / e32


def pad_mels(mels, Lmax=None):
    """[A, L_b] -> ([B, A, Lmax] filled with -4 beyond each utterance, lengths)"""
    Lmax = Lmax or max(m.shape[1] for m in mels)
    out = torch.full((len(mels), mels[0].shape[0], Lmax), -4.0)
    for b, m in enumerate(mels):
        out[b, :, :m.shape[1]] = m
    return out.cuda(), torch.tensor([m.shape[1] for m in mels])


def noise_of(T, seed):
    return torch.randn(T, generator=torch.Generator().manual_seed(seed))


def pad_rows(rows, Tmax=None, fill=0.0):
    """[T_b, ...] -> [B, Tmax, ...]"""
    Tmax = Tmax or max(r.shape[0] for r in rows)
    out = torch.full((len(rows), Tmax) + tuple(rows[0].shape[1:]), fill)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out.cuda()


# ---------------------------------------------------------------------------------------------------------------- 1. conditioning
@gpu
@pytest.mark.parametrize("name", ["default", "narrow"])
def test_conditioning_against_float64_and_ragged_bit_identity(name):
    cfg, sd, v = CFGS[name], sd_of(name), voc(name)
    hop = P.hop(cfg)
    single = {}
    for L in (1, 2, 5, 7):                                                    # 1, 2: fewer frames than the context window reaches
        mel = P.uniform_mel(cfg["A"], L, 20 + L)
        c = v.condition(*pad_mels([mel]))
        assert c.shape == (1, L * hop, cfg["A"])
        check(f"cond {name} L={L}", c[0].T, P.condition(sd, cfg, mel), P.condition(sd, cfg, mel, torch.float32))
        single[L] = c[0].clone()
    for Lmax in (7, 11):
        c = v.condition(*pad_mels([P.uniform_mel(cfg["A"], L, 20 + L) for L in RAGGED], Lmax))
        for b, L in enumerate(RAGGED):
            assert torch.equal(c[b, :L * hop], single[L]), (Lmax, b)


# ---------------------------------------------------------------------------------------------------------------- 2. one layer
@gpu
@pytest.mark.parametrize("name, lengths", [("default", [3, 1, 2]), ("odd", [7, 2, 5])])      # T = 768 / 256 / 512 and T = 105 / 30 / 75
@pytest.mark.parametrize("layer", [0, 1, 6, 9])                                              # dilations 1, 2, 64, 512
def test_one_layer_against_float64_and_ragged_bit_identity(name, lengths, layer):
    cfg, sd, v = CFGS[name], sd_of(name), voc(name)
    hop, R, S, A = P.hop(cfg), cfg["R"], cfg["S"], cfg["A"]
    assert P.dilation(cfg, layer) == v.geo["dilations"][layer] == 2 ** layer
    g = torch.Generator().manual_seed(300 + layer)
    xs = [torch.randn(L * hop, R, generator=g) for L in lengths]
    cs = [torch.randn(L * hop, A, generator=g) for L in lengths]
    s0 = [torch.randn(L * hop, S, generator=g) for L in lengths]

    def run(idx, Tmax=None):
        x, c, sk = pad_rows([xs[i] for i in idx], Tmax, 7.0), pad_rows([cs[i] for i in idx], Tmax, 7.0), pad_rows([s0[i] for i in idx], Tmax, 7.0)
        xo = torch.full_like(x, 9.0)
        v.layer(layer, x, c, xo, sk, [lengths[i] for i in idx])
        return xo, sk

    T = lengths[0] * hop
    xo, sk = run([0])
    ref = [P.layer(sd, cfg, layer, xs[0].T, cs[0].T, dt) for dt in (torch.float64, torch.float32)]
    check(f"layer {name} d={2 ** layer} T={T} x", xo[0].T, ref[0][0], ref[1][0])
    check(f"layer {name} d={2 ** layer} T={T} skips", sk[0].T, s0[0].T.double() + ref[0][1], s0[0].T + ref[1][1])
    bx, bs = run([1, 0, 2], (max(lengths) + 1) * hop)                        # another place in a batch, a larger padding
    assert torch.equal(bx[1, :T], xo[0]) and torch.equal(bs[1, :T], sk[0])
    assert bool((bx[1, T:] == 9.0).all()) and bool((bs[1, T:] == 7.0).all())  # nothing is written beyond the utterance
    for b, i in ((0, 1), (2, 2)):
        ox, os_ = run([i])
        n = lengths[i] * hop
        assert torch.equal(bx[b, :n], ox[0]) and torch.equal(bs[b, :n], os_[0])
    fresh = torch.full_like(sk, 5.0)                                         # the first layer of a call overwrites the skips
    v.layer(layer, pad_rows([xs[0]]), pad_rows([cs[0]]), torch.empty_like(xo), fresh, [lengths[0]], accumulate=False)
    assert torch.equal(fresh[0] + s0[0].cuda(), sk[0])


# ---------------------------------------------------------------------------------------------------------------- 3. whole generator
@gpu
@pytest.mark.parametrize("name, lengths", [("default", [3]), ("default", RAGGED), ("narrow", RAGGED)])
def test_generator_against_float64_and_batch_independence(name, lengths):
    cfg, sd, v = CFGS[name], sd_of(name), voc(name)
    hop = P.hop(cfg)
    mels = [P.uniform_mel(cfg["A"], L, 10 + L) for L in lengths]
    zs = [noise_of(L * hop, 110 + L) for L in lengths]
    wav, n = v(*pad_mels(mels), noises=pad_rows(zs))
    assert wav.shape == (len(lengths), max(lengths) * hop) and n.tolist() == [L * hop for L in lengths] and n.dtype == torch.int64
    for b, L in enumerate(lengths):
        check(f"generator {name} {lengths} utterance {b}", wav[b, :L * hop], P.generator(sd, cfg, mels[b], zs[b]), P.generator(sd, cfg, mels[b], zs[b], torch.float32))
        assert bool((wav[b, L * hop:] == 0).all())
    if len(lengths) > 1:
        wide, _ = v(*pad_mels(mels, max(lengths) + 3), noises=pad_rows(zs, (max(lengths) + 3) * hop))
        for b, L in enumerate(lengths):
            alone, _ = v(*pad_mels([mels[b]]), noises=pad_rows([zs[b]]))
            assert torch.equal(alone[0], wav[b, :L * hop]) and torch.equal(wide[b, :L * hop], alone[0]), b
            assert bool((wide[b, L * hop:] == 0).all())
    with pytest.raises(ValueError):
        v(*pad_mels(mels), noises=pad_rows(zs)[:, :-1])


# ---------------------------------------------------------------------------------------------------------------- 4. seeded noise
@gpu
@pytest.mark.parametrize("name", ["default", "narrow"])
def test_seeded_noise_is_drawn_in_the_kernel(name):
    cfg, sd, v = CFGS[name], sd_of(name), voc(name)
    hop = P.hop(cfg)
    lengths = [3, 2]
    mels = [P.uniform_mel(cfg["A"], L, 40 + L) for L in lengths]
    words = [P.pwg_seed_words(7, label, 0) for label in ("A", "B")]
    seeds = torch.tensor(words, dtype=torch.int64)
    wav, _ = v(*pad_mels(mels), seeds=seeds)
    for b, L in enumerate(lengths):
        z = P.seeded_noise(*words[b], L * hop)
        check(f"seeded {name} utterance {b}", wav[b, :L * hop], P.generator(sd, cfg, mels[b], z), P.generator(sd, cfg, mels[b], z, torch.float32))
    again, _ = v(*pad_mels(mels), seeds=seeds)
    assert torch.equal(again, wav)
    other, _ = v(*pad_mels([mels[1], mels[0], mels[1]], 6), seeds=seeds[[1, 0, 1]])
    assert torch.equal(other[1, :3 * hop], wav[0]) and torch.equal(other[0, :2 * hop], wav[1, :2 * hop]) and torch.equal(other[2], other[0])
    with pytest.raises(ValueError, match="seeds"):
        v(*pad_mels(mels), seeds=seeds, noises=torch.zeros(2, 3 * hop, device="cuda"))
    unseeded = [v(*pad_mels(mels))[0] for _ in range(2)]                      # torch.randn on the device: two draws differ
    assert not torch.equal(unseeded[0], unseeded[1])


# ---------------------------------------------------------------------------------------------------------------- 5. launches
@gpu
@pytest.mark.parametrize("name", ["default", "narrow"])
def test_launch_plan_and_no_vendor_library_kernel(name):
    """One conditioning group (conv_in + one launch per scale), one first, `Layers` layer launches, one head; and no ATen matrix product or convolution is
    dispatched during the call (those are the operators behind which the vendor BLAS / DNN libraries sit)."""
    from torch.utils._python_dispatch import TorchDispatchMode
    cfg, v = CFGS[name], voc(name)
    mels, lengths = pad_mels([P.uniform_mel(cfg["A"], L, 10 + L) for L in RAGGED])
    v(mels, lengths)                                                         # buffers exist
    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    launch_reset()
    with Record():
        v(mels, lengths, seeds=torch.tensor([[1, 2], [3, 4], [5, 6]]))
    counts = {k: n for k, n in launch_counts().items() if n}
    assert counts == {"pwg_cond_in": 1, "pwg_upsample": len(cfg["scales"]), "pwg_first": 1, "pwg_layer": cfg["layers"], "pwg_head": 1}, counts
    assert seen and not [s for s in seen if any(w in s for w in ("conv", "mm", "matmul", "linear", "einsum", "dot", "bmm"))], seen


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def _tiny_setup(root):
    import yaml
    from glow_tts_amd import data
    from glow_tts_amd.hparams import Recursive_Parse
    sd, _, _ = load_case("tiny_vanilla.npz")
    torch.save({"Model": sd, "Steps": 0}, os.path.join(root, "S_0.pt"))
    with open(os.path.join(root, "Token.yaml"), "w") as f:
        yaml.dump(data.make_token_dict(["HELLO WORLD."]), f)
    hp = tiny_hp_dict("Vanilla")
    cfg = dict(P.NARROW, A=hp["Sound"]["Mel_Dim"], scales=[4, 4, 4, 4])
    assert P.hop(cfg) == hp["Sound"]["Frame_Shift"]
    torch.save({"model": {"generator": P.random_state_dict(cfg, 77)}}, os.path.join(root, "vocoder.pt"))
    hp["Token_Path"] = os.path.join(root, "Token.yaml")
    hp["Inference_Batch_Size"] = 2
    hp["Griffin_Lim"] = {"Iterations": 4}
    hp["Vocoder"] = {"Type": "PWG", "Checkpoint_Path": os.path.join(root, "vocoder.pt"), "Layers": cfg["layers"], "Stacks": cfg["stacks"],
                     "Residual_Channels": cfg["R"], "Gate_Channels": cfg["G"], "Skip_Channels": cfg["S"]}
    return Recursive_Parse(hp)


@pytest.mark.late(1)
@gpu
def test_inference_writes_seeded_neural_wavs_and_griffin_lim_stays_selectable(tmp_path):
    from scipy.io import wavfile
    from glow_tts_amd.inferencer import Inferencer
    from glow_tts_amd.vocoder import GriffinLim, ParallelWaveGAN
    root = str(tmp_path)
    hp = _tiny_setup(root)
    inf = Inferencer(os.path.join(root, "S_0.pt"), hp=hp)
    assert inf.vocoder_kind == "pwg" and inf._vocoder is None
    labels, texts, scales = ["A", "B", "C"], ["HELLO WORLD.", "HELLO.", "WORLD WORLD HELLO."], [1.0, 1.2, 0.9]
    runs = []
    for tag in ("one", "two"):
        launch_reset()
        files = inf.Inference(labels, texts, scales, inference_path=os.path.join(root, tag), wav=True, seed=7)
        assert isinstance(inf._vocoder, ParallelWaveGAN) and launch_counts().get("pwg_layer", 0) == 2 * 4      # two batches of four layers
        assert [os.path.relpath(f, root) for f in inf.last_wav_files] == [os.path.join(tag, "WAV", x + ".wav") for x in labels]
        data_ = []
        for q, w in zip(files, inf.last_wav_files):
            sr, y = wavfile.read(w)
            assert sr == hp.Sound.Sample_Rate and y.dtype == np.int16 and y.shape == (np.load(q).shape[0] * hp.Sound.Frame_Shift,)
            assert np.abs(y.astype(np.int32)).max() > 0
            data_.append(open(w, "rb").read())
        runs.append(data_)
    assert runs[0] == runs[1]                                                 # byte-identical from run to run
    voc_files = inf.Vocode(labels, files, os.path.join(root, "voc"))          # existing mels go through the active vocoder too
    assert [wavfile.read(w)[1].shape for w in voc_files] == [wavfile.read(w)[1].shape for w in inf.last_wav_files]
    gl = Inferencer(os.path.join(root, "S_0.pt"), hp=hp, vocoder="griffin_lim")
    launch_reset()
    gl.Inference(labels, texts, scales, inference_path=os.path.join(root, "gl"), wav=True, seed=7)
    counts = {k: n for k, n in launch_counts().items() if n}
    assert isinstance(gl._vocoder, GriffinLim) and not [k for k in counts if k.startswith("pwg")] and counts.get("vocoder_griffin_lim_step") == 2 * 4
    by_arg = Inferencer(os.path.join(root, "S_0.pt"), hp=hp, vocoder_checkpoint=os.path.join(root, "vocoder.pt"))
    assert by_arg.vocoder_kind == "pwg"
    with pytest.raises(ValueError):
        Inferencer(os.path.join(root, "S_0.pt"), hp=hp, vocoder="wavernn")
