"""GPU suite of the neural vocoder's bf16 inference mode (`ParallelWaveGAN(..., precision='bf16')` on csrc/pwg_bf16_ops.hip) against the restatement of
its contract, tests/pwg_bf16_ref.py.  The cases, the bars and where they come from: tests/pwg_bf16_cases.py; tests/test_pwg_bf16_cpu.py holds the float32
restatements themselves to the same bars.  Every observed ratio is printed before it is asserted (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import pwg_bf16_cases as C  # noqa: E402
import pwg_ref as P  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402
from test_gpu_pwg import _hp, _tiny_setup, pad_mels, pad_rows  # noqa: E402

gpu = pytest.mark.gpu
_VOC = {}


def voc(name, precision="bf16", **kw):
    from glow_tts_amd.vocoder import ParallelWaveGAN
    key = (name, precision) + tuple(sorted(kw.items()))
    if key not in _VOC:
        _VOC[key] = ParallelWaveGAN(_hp(C.CFGS[name]), "cuda:0", state_dict={"generator": C.sd_of(name)}, precision=precision, **kw)
    return _VOC[key]


# ---------------------------------------------------------------------------------------------------------------- 1. one layer
@gpu
@pytest.mark.parametrize("name, lengths, layer", C.LAYER_CASES)
def test_one_layer_against_the_contract_and_ragged_bit_identity(name, lengths, layer):
    cfg, v = C.CFGS[name], voc(name)
    hop = P.hop(cfg)
    assert v.precision == "bf16" and P.dilation(cfg, layer) == v.geo["dilations"][layer] == 2 ** layer
    case = C.layer_case(name, lengths, layer)
    xs, cs, s0 = case["xs"], case["cs"], case["s0"]

    def run(idx, Tmax=None):
        x, c, sk = pad_rows([xs[i] for i in idx], Tmax, 7.0), pad_rows([cs[i] for i in idx], Tmax, 7.0), pad_rows([s0[i] for i in idx], Tmax, 7.0)
        xo = torch.full_like(x, 9.0)
        v.layer(layer, x, c, xo, sk, [lengths[i] for i in idx])
        return xo, sk

    T = lengths[0] * hop
    launch_reset()
    xo, sk = run([0])
    assert {k: n for k, n in launch_counts().items() if n} == {"pwg_layer_bf16": 1}
    C.check_layer(f"layer {name} d={2 ** layer} T={T} x", xo[0].T, case["x"])
    C.check_layer(f"layer {name} d={2 ** layer} T={T} skips", sk[0].T, case["skips"])
    bx, bs = run([1, 0, 2], (max(lengths) + 1) * hop)                        # another place in a batch, a larger padding
    assert torch.equal(bx[1, :T], xo[0]) and torch.equal(bs[1, :T], sk[0])
    assert bool((bx[1, T:] == 9.0).all()) and bool((bs[1, T:] == 7.0).all())  # nothing is written beyond the utterance
    for b, i in ((0, 1), (2, 2)):
        ox, os_ = run([i])
        n = lengths[i] * hop
        assert torch.equal(bx[b, :n], ox[0]) and torch.equal(bs[b, :n], os_[0])
    again = run([0])                                                          # from run to run
    assert torch.equal(again[0], xo) and torch.equal(again[1], sk)
    fresh = torch.full_like(sk, 5.0)                                         # the first layer of a call overwrites the skips
    v.layer(layer, pad_rows([xs[0]]), pad_rows([cs[0]]), torch.empty_like(xo), fresh, [lengths[0]], accumulate=False)
    assert torch.equal(fresh[0] + s0[0].cuda(), sk[0])


# ---------------------------------------------------------------------------------------------------------------- 2. whole generator
@gpu
@pytest.mark.parametrize("name, lengths", C.GENERATOR_CASES)
def test_generator_against_the_contract_and_batch_independence(name, lengths):
    cfg, v = C.CFGS[name], voc(name)
    hop = P.hop(cfg)
    mels, zs = C.generator_inputs(name, lengths)
    wav, n = v(*pad_mels(mels), noises=pad_rows(zs))
    assert wav.shape == (len(lengths), max(lengths) * hop) and n.tolist() == [L * hop for L in lengths] and n.dtype == torch.int64
    for b, L in enumerate(lengths):
        C.check_generator(f"generator {name} {lengths} utterance {b}", wav[b, :L * hop], C.generator_refs(name, mels[b], zs[b]))
        assert bool((wav[b, L * hop:] == 0).all())
    if len(lengths) > 1:
        wide, _ = v(*pad_mels(mels, max(lengths) + 3), noises=pad_rows(zs, (max(lengths) + 3) * hop))
        for b, L in enumerate(lengths):
            alone, _ = v(*pad_mels([mels[b]]), noises=pad_rows([zs[b]]))
            assert torch.equal(alone[0], wav[b, :L * hop]) and torch.equal(wide[b, :L * hop], alone[0]), b
            assert bool((wide[b, L * hop:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 3. the bf16 path was taken
@gpu
@pytest.mark.parametrize("name", ["default", "narrow"])
def test_launch_plan_is_bf16_layers_only_and_f32_stays_f32(name):
    from torch.utils._python_dispatch import TorchDispatchMode
    cfg, v, f = C.CFGS[name], voc(name), voc(name, "f32")
    mels, lengths = pad_mels([P.uniform_mel(cfg["A"], L, 10 + L) for L in C.RAGGED])
    seeds = torch.tensor([[1, 2], [3, 4], [5, 6]])
    v(mels, lengths)                                                         # buffers exist
    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    launch_reset()
    with Record():
        wav, _ = v(mels, lengths, seeds=seeds)
    counts = {k: n for k, n in launch_counts().items() if n}
    assert counts == {"pwg_cond_in": 1, "pwg_upsample": len(cfg["scales"]), "pwg_first": 1, "pwg_layer_bf16": cfg["layers"], "pwg_head": 1}, counts
    assert seen and not [s for s in seen if any(w in s for w in ("conv", "mm", "matmul", "linear", "einsum", "dot", "bmm"))], seen
    launch_reset()
    wav32, _ = f(mels, lengths, seeds=seeds)
    counts = {k: n for k, n in launch_counts().items() if n}
    assert counts == {"pwg_cond_in": 1, "pwg_upsample": len(cfg["scales"]), "pwg_first": 1, "pwg_layer": cfg["layers"], "pwg_head": 1}, counts
    assert f.precision == "f32" and not torch.equal(wav, wav32)
    from test_gpu_pwg import voc as voc_as_before                             # constructed without the argument: the same f32 wav, bit for bit
    assert voc_as_before(name).precision == "f32" and torch.equal(voc_as_before(name)(mels, lengths, seeds=seeds)[0], wav32)


@gpu
def test_yaml_key_selects_bf16_and_a_trainable_generator_stays_f32():
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.vocoder import ParallelWaveGAN
    cfg, sd = C.CFGS["narrow"], {"generator": C.sd_of("narrow")}
    hp = _hp(cfg)
    hp.Vocoder.Precision = "bf16"
    by_key, by_arg, back = ParallelWaveGAN(hp, "cuda:0", state_dict=sd), voc("narrow"), ParallelWaveGAN(hp, "cuda:0", state_dict=sd, precision="f32")
    assert (by_key.precision, by_key.geo["precision"], back.precision) == ("bf16", "bf16", "f32")
    mels, lengths = pad_mels([P.uniform_mel(cfg["A"], L, 10 + L) for L in C.RAGGED])
    seeds = torch.tensor([[1, 2], [3, 4], [5, 6]])
    assert torch.equal(by_key(mels, lengths, seeds=seeds)[0], by_arg(mels, lengths, seeds=seeds)[0])
    assert torch.equal(back(mels, lengths, seeds=seeds)[0], voc("narrow", "f32")(mels, lengths, seeds=seeds)[0])
    train = ParallelWaveGAN(hp, "cuda:0", state_dict=sd, trainable=True)      # the key is a serving setting
    assert train.precision == "f32"
    launch_reset()
    wav, _ = train.generate(mels, lengths, seeds=seeds)
    counts = launch_counts()
    assert counts.get("pwg_layer") == cfg["layers"] and not counts.get("pwg_layer_bf16") and torch.equal(wav.detach(), back(mels, lengths, seeds=seeds)[0])
    with pytest.raises(ValueError, match="trainable"):
        ParallelWaveGAN(hp, "cuda:0", state_dict=sd, trainable=True, precision="bf16")


# ---------------------------------------------------------------------------------------------------------------- 4. seeded noise
@gpu
@pytest.mark.parametrize("name", C.SEEDED_CASES)
def test_seeded_bf16_wav_repeats_and_matches_the_contract(name):
    cfg, v = C.CFGS[name], voc(name)
    hop = P.hop(cfg)
    mels, words, zs = C.seeded_inputs(name)
    seeds = torch.tensor(words, dtype=torch.int64)
    wav, _ = v(*pad_mels(mels), seeds=seeds)
    for b, L in enumerate(C.SEEDED_LENGTHS):
        C.check_generator(f"seeded {name} utterance {b}", wav[b, :L * hop], C.generator_refs(name, mels[b], zs[b]))
    again, _ = v(*pad_mels(mels), seeds=seeds)
    assert torch.equal(again, wav)
    other, _ = v(*pad_mels([mels[1], mels[0], mels[1]], 6), seeds=seeds[[1, 0, 1]])
    assert torch.equal(other[1, :3 * hop], wav[0]) and torch.equal(other[0, :2 * hop], wav[1, :2 * hop]) and torch.equal(other[2], other[0])


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
@pytest.mark.late(1)
@gpu
def test_inference_writes_seeded_bf16_wavs_and_the_default_is_unchanged(tmp_path):
    from scipy.io import wavfile
    from glow_tts_amd.inferencer import Inferencer
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import compare_pwg_precision
    root = str(tmp_path)
    hp = _tiny_setup(root)
    labels, texts, scales = ["A", "B", "C"], ["HELLO WORLD.", "HELLO.", "WORLD WORLD HELLO."], [1.0, 1.2, 0.9]

    def run(tag, layer_class, **kw):
        inf = Inferencer(os.path.join(root, "S_0.pt"), hp=hp, **kw)
        launch_reset()
        files = inf.Inference(labels, texts, scales, inference_path=os.path.join(root, tag), wav=True, seed=7)
        counts = {k: n for k, n in launch_counts().items() if n and k.startswith("pwg_layer")}
        assert counts == {layer_class: 2 * 4}, counts                          # two batches of four layers
        return files, [open(w, "rb").read() for w in inf.last_wav_files], list(inf.last_wav_files)

    mel_files, as_before, _ = run("f32", "pwg_layer")                                           # constructed as today
    _, explicit, _ = run("f32b", "pwg_layer", vocoder="pwg", vocoder_precision="f32")
    _, one, wavs = run("bf16", "pwg_layer_bf16", vocoder="pwg", vocoder_precision="bf16")
    _, two, _ = run("bf16b", "pwg_layer_bf16", vocoder="pwg", vocoder_precision="bf16")
    assert as_before == explicit                                              # without the flag: today's bytes
    assert one == two                                                         # byte-identical from run to run
    assert all(a != b and len(a) == len(b) for a, b in zip(one, as_before))   # another wav of the same length
    for w in wavs:
        sr, y = wavfile.read(w)
        assert sr == hp.Sound.Sample_Rate and y.dtype == np.int16 and np.abs(y.astype(np.int32)).max() > 0
    with pytest.raises(ValueError, match="vocoder_precision"):
        Inferencer(os.path.join(root, "S_0.pt"), hp=hp, vocoder_precision="fp16")
    rows = compare_pwg_precision.compare(hp, os.path.join(root, "vocoder.pt"), list(zip(labels, mel_files)), seed=7)
    assert [r["label"] for r in rows] == labels
    for r in rows:
        print(r)
        assert np.isfinite(r["snr_db"]) and r["snr_db"] > 0 and np.isfinite(r["stft_loss"]) and r["stft_loss"] > 0
