"""GPU suite of the HiFi-GAN vocoder (glow_tts_amd/vocoder.py: HiFiGAN on csrc/hifigan_ops.hip) against the float64 restatement tests/hifigan_ref.py.

Weights: torch's default Conv initialisation under a fixed seed; mels uniform in [-4, 4]; the operator tests use unit-scale random rows.  THE BAR (no closed
bound exists for a chain of this depth, so it is measured on the reference arithmetic, never on the code under test): every case also runs the restatement
in float32 on the CPU; with e32 = max |ref32 - ref64| / max |ref64| the HIP result must satisfy  max |hip - ref64| / max |ref64| <= 4 * e32 + 1e-6
(4: the exact-f32 MFMA sums the same products in another order than torch's CPU convolution; 1e-6: a floor for cases whose e32 happens to be tiny).
Guard against degenerate inputs: 0 < e32 < 1e-3 and max |ref64| > 1e-3.  The waveform at random weights is small and partly conv_post's bias, so the
whole-generator tests hold the rows entering conv_post to the same bar too.  The observed ratio err / e32 of every case is printed before it is asserted
(pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import hifigan_ref as H  # noqa: E402
from helpers import launch_counts, launch_reset, load_case, tiny_hp_dict  # noqa: E402

gpu = pytest.mark.gpu

CFGS = {"default": H.DEFAULT, "narrow": H.NARROW, "odd": H.ODD}
WEIGHT_SEED = 1234
RAGGED = [5, 2, 7]
TILE = 64                                                                    # rows per workgroup of both kernels (TM of csrc/pwg_common.h)
_VOC, _SD, _REF = {}, {}, {}


def block_of(cfg, **more):
    return dict({"Type": "HiFiGAN", "Initial_Channels": cfg["C0"], "Upsample_Rates": list(cfg["rates"]), "Upsample_Kernel_Sizes": list(cfg["kernels"]),
                 "Resblock": cfg["resblock"], "Resblock_Kernel_Sizes": list(cfg["rk"]), "Resblock_Dilations": [list(d) for d in cfg["rd"]]}, **more)


def _hp(cfg):
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    d = load_yaml(DEFAULT_YAML)
    d["Sound"].update(Mel_Dim=cfg["A"], Frame_Shift=H.hop(cfg))
    d["Vocoder"] = block_of(cfg)
    return Recursive_Parse(d)


def sd_of(name):
    if name not in _SD:
        _SD[name] = H.random_state_dict(CFGS[name], WEIGHT_SEED)
    return _SD[name]


def voc(name):
    from glow_tts_amd.vocoder import HiFiGAN
    if name not in _VOC:
        _VOC[name] = HiFiGAN(_hp(CFGS[name]), "cuda:0", state_dict={"generator": sd_of(name)})
    return _VOC[name]


def reference(name, L):
    """(mel, (wav64, rows64), (wav32, rows32)) of the utterance of L frames: computed once, shared, never changed"""
    if (name, L) not in _REF:
        cfg = CFGS[name]
        mel = H.uniform_mel(cfg["A"], L, 10 + L)
        _REF[(name, L)] = (mel, H.generator(sd_of(name), cfg, mel), H.generator(sd_of(name), cfg, mel, torch.float32))
    return _REF[(name, L)]


def check(tag, got, ref64, ref32):
    err, e32 = H.errors(got.cpu(), ref64, ref32)
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


def pad_rows(rows, Tmax=None, fill=7.0):
    """[T_b, C] -> [B, Tmax, C] holding `fill` beyond each utterance"""
    Tmax = Tmax or max(r.shape[0] for r in rows)
    out = torch.full((len(rows), Tmax) + tuple(rows[0].shape[1:]), fill)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out.cuda()


# ---------------------------------------------------------------------------------------------------------------- 1. hifigan_conv alone
CONV_LENGTHS = [1, 5, TILE - 1, TILE, TILE + 1, 200]                         # 1, 5: shorter than the 25-row reach of (11, 5); 63 / 64 / 65: around the tile edge


@gpu
@pytest.mark.parametrize("taps, d", [(3, 1), (3, 5), (7, 3), (11, 5), (7, 1)])
@pytest.mark.parametrize("cin, cout", [(16, 16), (32, 16), (256, 256), (8, 64), (80, 512)])       # (8, 64): conv_pre at A = 8; (80, 512): conv_pre at V1
def test_conv_against_float64_every_epilogue_and_ragged_bit_identity(cin, cout, taps, d):
    v = voc("narrow")
    g = torch.Generator().manual_seed(1000 * cin + 10 * taps + d)
    w = (torch.rand(cout, cin, taps, generator=g) * 2 - 1) / (cin * taps) ** 0.5
    b = torch.rand(cout, generator=g) * 2 - 1
    lengths = CONV_LENGTHS + [37]                                            # 37: the ragged batch's third utterance
    xs = [torch.randn(T, cin, generator=g) for T in lengths]
    rs = [torch.randn(T, cout, generator=g) for T in lengths]                # the residual
    os_ = [torch.randn(T, cout, generator=g) for T in lengths]               # what the MRF sum holds so far

    def ref(i, dt, slope, res, acc):
        y = H.conv(xs[i].T.to(dt), w.to(dt), b.to(dt), d, slope)
        if res:
            y = y + rs[i].T.to(dt)
        return y if acc == 0 else (os_[i].T.to(dt) + y if acc == 1 else (os_[i].T.to(dt) + y) / 3)

    def run(idx, slope, res, acc, Tmax=None):
        out = pad_rows([os_[i] for i in idx], Tmax)
        x = pad_rows([xs[i] for i in idx], Tmax)
        r = pad_rows([rs[i] for i in idx], Tmax) if res else None
        return v.conv(x, [lengths[i] for i in idx], weight=w, bias=b, dilation=d, slope=1.0 if slope is None else slope, residual=r, out=out,
                      accumulate=acc, divisor=3.0)

    everything = list(range(len(CONV_LENGTHS)))
    for tag, slope, res, acc in (("plain", None, False, 0), ("lrelu", H.SLOPE, False, 0), ("lrelu+res", H.SLOPE, True, 0), ("lrelu+res+acc", H.SLOPE, True, 1),
                                 ("res+last", None, True, 2), ("lrelu+res+last", H.SLOPE, True, 2)):
        out = run(everything, slope, res, acc)
        for i, T in enumerate(CONV_LENGTHS):
            check(f"conv {cin}->{cout} k={taps} d={d} {tag} T={T}", out[i, :T].T, ref(i, torch.float64, slope, res, acc), ref(i, torch.float32, slope, res, acc))
            assert bool((out[i, T:] == 7.0).all())                            # nothing is written beyond the utterance
    # a ragged batch [T, 1, 37] at two paddings: every utterance is its single run, bit for bit
    idx = [5, 0, 6]
    single = [run([i], H.SLOPE, True, 2) for i in idx]
    for Tmax in (200, 200 + TILE + 1):
        batch = run(idx, H.SLOPE, True, 2, Tmax)
        for bi, i in enumerate(idx):
            assert torch.equal(batch[bi, :lengths[i]], single[bi][0]), (Tmax, bi)
            assert bool((batch[bi, lengths[i]:] == 7.0).all())


@gpu
def test_conv_with_the_generators_own_weights_and_in_place_residual():
    """`key` addresses a convolution of the generator; the residual may be the output tensor (the second convolution of a type-'1' step adds x in place)."""
    cfg, sd, v = H.ODD, sd_of("odd"), voc("odd")
    g = torch.Generator().manual_seed(5)
    x, t = torch.randn(70, 32, generator=g), torch.randn(70, 32, generator=g)
    key = "resblocks.2.convs2.1"
    xo = pad_rows([x])
    v.conv(pad_rows([t]), [70], key=key, slope=H.SLOPE, residual=xo, out=xo)
    ref = [H.conv(t.T.to(dt), sd[key + ".weight"].to(dt), sd[key + ".bias"].to(dt), 1, H.SLOPE) + x.T.to(dt) for dt in (torch.float64, torch.float32)]
    check("conv own weights, in place", xo[0].T, *ref)
    pre = v.conv(pad_rows([H.uniform_mel(cfg["A"], 9, 1).T]), [9], key="conv_pre")
    mel = H.uniform_mel(cfg["A"], 9, 1)
    check("conv_pre by key", pre[0].T, *[H.conv(mel.to(dt), sd["conv_pre.weight"].to(dt), sd["conv_pre.bias"].to(dt)) for dt in (torch.float64, torch.float32)])


# ---------------------------------------------------------------------------------------------------------------- 2. hifigan_upsample
UP_LENGTHS = [1, 2, 9, 33, TILE + 1]                                         # 65: a second workgroup along the rows


@gpu
@pytest.mark.parametrize("u, k", [(2, 4), (8, 16), (3, 7), (5, 11)])         # (3, 7), (5, 11): the phases have unequal tap counts
@pytest.mark.parametrize("cin", [32, 64, 512])
def test_upsample_against_float64_length_and_ragged_bit_identity(u, k, cin):
    v = voc("narrow")
    cout = cin // 2
    g = torch.Generator().manual_seed(100 * u + k + cin)
    w = (torch.rand(cin, cout, k, generator=g) * 2 - 1) / (cout * k) ** 0.5
    b = torch.rand(cout, generator=g) * 2 - 1
    xs = [torch.randn(T, cin, generator=g) for T in UP_LENGTHS]

    def run(idx, Tmax=None):
        Tmax = Tmax or max(UP_LENGTHS[i] for i in idx)
        out = torch.full((len(idx), u * Tmax, cout), 7.0, device="cuda")
        return v.upsample(None, pad_rows([xs[i] for i in idx], Tmax), [UP_LENGTHS[i] for i in idx], out=out, weight=w, bias=b, rate=u)

    out = run(list(range(len(UP_LENGTHS))))
    assert out.shape == (len(UP_LENGTHS), u * max(UP_LENGTHS), cout)
    for i, T in enumerate(UP_LENGTHS):
        ref = [H.upsample(xs[i].T.to(dt), w.to(dt), b.to(dt), u) for dt in (torch.float64, torch.float32)]
        assert ref[0].shape == (cout, u * T)                                  # exactly u rows per input row
        check(f"upsample {cin}->{cout} u={u} k={k} T={T}", out[i, :u * T].T, *ref)
        assert bool((out[i, u * T:] == 7.0).all())
    idx = [3, 0, 2]
    single = [run([i]) for i in idx]
    for Tmax in (33, 33 + TILE):
        batch = run(idx, Tmax)
        for bi, i in enumerate(idx):
            n = u * UP_LENGTHS[i]
            assert torch.equal(batch[bi, :n], single[bi][0]) and bool((batch[bi, n:] == 7.0).all()), (Tmax, bi)


# ---------------------------------------------------------------------------------------------------------------- 3. one stage
@gpu
@pytest.mark.parametrize("name", ["narrow", "odd"])
@pytest.mark.parametrize("i", [0, 1])
def test_one_stage_against_float64_and_ragged_bit_identity(name, i):
    cfg, sd, v = CFGS[name], sd_of(name), voc(name)
    u, cin = cfg["rates"][i], H.channels(cfg, i - 1)
    lengths = [40, 3, TILE + 6]
    g = torch.Generator().manual_seed(40 + i)
    xs = [torch.randn(T, cin, generator=g) for T in lengths]
    out = v.stage(i, pad_rows(xs), lengths)
    assert out.shape == (3, u * max(lengths), H.channels(cfg, i))
    for b, T in enumerate(lengths):
        check(f"stage {name} {i} T={T}", out[b, :u * T].T, H.stage(sd, cfg, i, xs[b].T.double()), H.stage(sd, cfg, i, xs[b].T))
        assert torch.equal(v.stage(i, pad_rows([xs[b]]), [T])[0], out[b, :u * T]), b
    wide = v.stage(i, pad_rows(xs, max(lengths) + TILE + 3), lengths)
    assert all(torch.equal(wide[b, :u * T], out[b, :u * T]) for b, T in enumerate(lengths))


# ---------------------------------------------------------------------------------------------------------------- 4. whole generator
@gpu
@pytest.mark.parametrize("name, lengths", [("default", [3]), ("default", RAGGED), ("narrow", RAGGED), ("narrow", [1]), ("odd", RAGGED), ("odd", [1])])
def test_generator_against_float64_batch_independence_and_launch_plan(name, lengths):
    from torch.utils._python_dispatch import TorchDispatchMode
    from glow_tts_amd.vocoder import hifigan_launches
    cfg, v = CFGS[name], voc(name)
    hop = H.hop(cfg)
    refs = [reference(name, L) for L in lengths]
    mels = [r[0] for r in refs]
    v(*pad_mels(mels))                                                       # buffers exist
    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    launch_reset()
    with Record():
        wav, n, rows = v(*pad_mels(mels), return_rows=True)
    counts = {k: c for k, c in launch_counts().items() if c}
    convs = hifigan_launches(v.geo) - 2 - len(cfg["rates"])
    assert counts == {"hifigan_conv": 1 + convs, "hifigan_upsample": len(cfg["rates"]), "hifigan_conv,post": 1}, counts
    assert sum(counts.values()) == hifigan_launches(v.geo) and (name != "default" or sum(counts.values()) == 78)
    assert seen and not [s for s in seen if any(w in s for w in ("conv", "mm", "matmul", "linear", "einsum", "dot", "bmm"))], seen
    assert wav.shape == (len(lengths), max(lengths) * hop) and n.tolist() == [L * hop for L in lengths] and n.dtype == torch.int64
    assert rows.shape == (len(lengths), max(lengths) * hop, H.channels(cfg, len(cfg["rates"]) - 1)) and torch.equal(rows, v.last_rows)
    for b, (L, (_, (w64, r64), (w32, r32))) in enumerate(zip(lengths, refs)):
        check(f"generator {name} {lengths} utterance {b} rows", rows[b, :L * hop].T, r64, r32)
        check(f"generator {name} {lengths} utterance {b} wav", wav[b, :L * hop], w64, w32)
        assert bool((wav[b, L * hop:] == 0).all())
    again, _ = v(*pad_mels(mels), seeds=torch.tensor([[1, 2]] * len(lengths)))   # no noise input: the seed words change nothing; run to run bit-identical
    assert torch.equal(again, wav)
    if len(lengths) > 1:
        wide, _ = v(*pad_mels(mels, max(lengths) + 3))
        for b, L in enumerate(lengths):
            alone, _ = v(*pad_mels([mels[b]]))
            assert torch.equal(alone[0], wav[b, :L * hop]) and torch.equal(wide[b, :L * hop], alone[0]), b
            assert bool((wide[b, L * hop:] == 0).all())
    with pytest.raises(ValueError, match="Sound.Mel_Dim"):
        v(torch.zeros(1, cfg["A"] + 4, 3, device="cuda"), [3])


# ---------------------------------------------------------------------------------------------------------------- 5. entry points
TINY = {"A": 12, "C0": 128, "rates": [8, 8, 4], "kernels": [16, 16, 8], "resblock": "2", "rk": [3, 5], "rd": [[1, 3], [1, 3]]}      # the tiny model's mel size and hop


def _tiny_setup(root, vocoder_block):
    import yaml
    from glow_tts_amd import data
    from glow_tts_amd.hparams import Recursive_Parse
    sd, _, _ = load_case("tiny_vanilla.npz")
    torch.save({"Model": sd, "Steps": 0}, os.path.join(root, "S_0.pt"))
    with open(os.path.join(root, "Token.yaml"), "w") as f:
        yaml.dump(data.make_token_dict(["HELLO WORLD."]), f)
    hp = tiny_hp_dict("Vanilla")
    assert H.hop(TINY) == hp["Sound"]["Frame_Shift"] and TINY["A"] == hp["Sound"]["Mel_Dim"]
    torch.save({"generator": H.random_state_dict(TINY, 77)}, os.path.join(root, "hifigan.pt"))
    hp["Token_Path"] = os.path.join(root, "Token.yaml")
    hp["Inference_Batch_Size"] = 2
    if vocoder_block is not None:
        hp["Vocoder"] = vocoder_block
    return Recursive_Parse(hp)


@pytest.mark.late(1)
@gpu
def test_inferencer_vocodes_and_synthesises_through_hifigan(tmp_path):
    from scipy.io import wavfile
    from glow_tts_amd.inferencer import Inferencer
    from glow_tts_amd.vocoder import HiFiGAN, ParallelWaveGAN
    root = str(tmp_path)
    ckpt = os.path.join(root, "hifigan.pt")
    hp = _tiny_setup(root, block_of(TINY))                                   # no Checkpoint_Path in the yaml: the argument gives it
    inf = Inferencer(os.path.join(root, "S_0.pt"), hp=hp, vocoder="hifigan", vocoder_checkpoint=ckpt)
    assert inf.vocoder_kind == "hifigan" and inf._vocoder is None
    g = torch.Generator().manual_seed(3)
    labels, mels = ["A", "B", "C"], [(torch.rand(T, 12, generator=g) * 8 - 4).numpy() for T in (9, 4, 13)]
    runs = []
    for tag in ("one", "two"):
        launch_reset()
        files = inf.Vocode(labels, mels, os.path.join(root, tag))
        counts = {k: c for k, c in launch_counts().items() if c}
        assert isinstance(inf._vocoder, HiFiGAN) and counts.get("hifigan_upsample") == 2 * 3 and not [k for k in counts if k.startswith("pwg")]      # two batches
        assert files == inf.last_wav_files and [os.path.relpath(f, root) for f in files] == [os.path.join(tag, "WAV", x + ".wav") for x in labels]
        data_ = []
        for m, w in zip(mels, files):
            sr, y = wavfile.read(w)
            assert sr == hp.Sound.Sample_Rate and y.dtype == np.int16 and y.shape == (m.shape[0] * hp.Sound.Frame_Shift,)
            assert np.abs(y.astype(np.int32)).max() > 0
            data_.append(open(w, "rb").read())
        runs.append(data_)
    assert runs[0] == runs[1]                                                 # byte-identical from run to run
    texts, scales = ["HELLO WORLD.", "HELLO.", "WORLD WORLD HELLO."], [1.0, 1.2, 0.9]
    seeded = []
    for tag, seed in (("s7", 7), ("s7b", 7)):                                # --wav: the mel is seeded, the vocoder needs no seed
        files = inf.Inference(labels, texts, scales, inference_path=os.path.join(root, tag), wav=True, seed=seed)
        assert [wavfile.read(w)[1].shape[0] for w in inf.last_wav_files] == [np.load(q).shape[0] * hp.Sound.Frame_Shift for q in files]
        seeded.append([open(w, "rb").read() for w in inf.last_wav_files])
    assert seeded[0] == seeded[1]
    by_block = Inferencer(os.path.join(root, "S_0.pt"), hp=_tiny_setup(root, block_of(TINY, Checkpoint_Path=ckpt)))       # Type: 'HiFiGAN' selects it without the flag
    assert by_block.vocoder_kind == "hifigan"
    again = by_block.Vocode(labels, mels, os.path.join(root, "block"))
    assert isinstance(by_block._vocoder, HiFiGAN) and [open(w, "rb").read() for w in again] == runs[0]
    with pytest.raises(ValueError, match="Vocoder.Precision"):
        Inferencer(os.path.join(root, "S_0.pt"), hp=hp, vocoder="hifigan", vocoder_checkpoint=ckpt, vocoder_precision="bf16").Vocode(labels[:1], mels[:1], root)
    # a Type: 'PWG' block still builds the Parallel WaveGAN generator
    import pwg_ref as P
    pcfg = dict(P.NARROW, A=12, scales=[4, 4, 4, 4])
    torch.save({"generator": P.random_state_dict(pcfg, 77)}, os.path.join(root, "pwg.pt"))
    pwg = Inferencer(os.path.join(root, "S_0.pt"), hp=_tiny_setup(root, {"Type": "PWG", "Checkpoint_Path": os.path.join(root, "pwg.pt"), "Layers": 4, "Stacks": 2,
                                                                        "Residual_Channels": 32, "Gate_Channels": 64, "Skip_Channels": 32}))
    assert pwg.vocoder_kind == "pwg"
    pwg.Vocode(labels[:1], mels[:1], os.path.join(root, "pwg"))
    assert isinstance(pwg._vocoder, ParallelWaveGAN)
