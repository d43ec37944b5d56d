"""GPU suite of the HiFi-GAN vocoder's fp16 inference mode (`HiFiGAN(..., precision='f16')` on csrc/hifigan_f16_ops.hip) against the restatement of its
contract, tests/hifigan_f16_ref.py.  The cases, the bars and where they come from: tests/hifigan_f16_cases.py; tests/test_hifigan_f16_cpu.py holds the float32
realisations of the restatement to the same bars.  Every observed ratio is printed before it is asserted (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hifigan_f16_cases as C  # noqa: E402
import hifigan_f16_ref as R  # noqa: E402
import hifigan_ref as H  # noqa: E402
import test_gpu_hifigan as G  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402

gpu = pytest.mark.gpu
TILE = G.TILE
_VOC = {}


def voc(name, seed=G.WEIGHT_SEED, precision="f16", **kw):
    from glow_tts_amd.vocoder import HiFiGAN
    key = (name, seed, precision)
    if kw:
        return HiFiGAN(G._hp(C.CFGS[name]), "cuda:0", state_dict={"generator": C.sd_of(name, seed)}, precision=precision, **kw)
    if key not in _VOC:
        _VOC[key] = HiFiGAN(G._hp(C.CFGS[name]), "cuda:0", state_dict={"generator": C.sd_of(name, seed)}, precision=precision)
    return _VOC[key]


def emu_pair(fn):
    """fn(emu) for emu64 and emu32 of the contract as the hardware was found to treat subnormals"""
    e64, e32, _ = R.emus(C.FLUSH_SUBNORMALS)
    return fn(e64), fn(e32)


# ---------------------------------------------------------------------------------------------------------------- 1. operators against the contract
@gpu
@pytest.mark.parametrize("taps, d", C.CONV_TAPS)
@pytest.mark.parametrize("cin, cout, cf", C.CONV_CHANNELS)
def test_conv_against_the_contract_every_epilogue_and_ragged_bit_identity(cin, cout, cf, taps, d):
    v = voc("narrow")
    assert v.precision == "f16"
    g = torch.Generator().manual_seed(1000 * cin + 10 * taps + d)
    w = (torch.rand(cout, cin, taps, generator=g) * 2 - 1) / (cin * taps) ** 0.5
    b = torch.rand(cout, generator=g) * 2 - 1
    lengths = C.CONV_ROWS + [37]                                              # 37: the ragged batch's third utterance
    xs = [torch.randn(T, cin, generator=g) for T in lengths]
    rs = [torch.randn(T, cout, generator=g) for T in lengths]                 # the residual
    os_ = [torch.randn(T, cout, generator=g) for T in lengths]                # what the MRF sum holds so far
    convs = [emu_pair(lambda e: e.conv(xs[i].T, w, b, d, H.SLOPE)) for i in range(len(C.CONV_ROWS))]        # once per length, shared by the epilogues

    def ref(i, k, res, acc):
        y, dt = convs[i][k], convs[i][k].dtype
        if res:
            y = y + rs[i].T.to(dt)
        return y if acc == 0 else (os_[i].T.to(dt) + y if acc == 1 else (os_[i].T.to(dt) + y) / 3)

    def run(idx, res, acc, Tmax=None):
        Tmax = Tmax or max(lengths[i] for i in idx)
        out = G.pad_rows([os_[i] for i in idx], Tmax)
        x = G.pad_rows([xs[i] for i in idx], Tmax)
        if cf:
            x = x.transpose(1, 2).contiguous()                                # [B, Cin, T], as conv_pre takes the mel
        r = G.pad_rows([rs[i] for i in idx], Tmax) if res else None
        return v.conv(x, [lengths[i] for i in idx], weight=w, bias=b, dilation=d, slope=H.SLOPE, residual=r, out=out, accumulate=acc, divisor=3.0,
                      channels_first=cf)

    everything = list(range(len(C.CONV_ROWS)))
    for tag, res, acc in C.EPILOGUES:
        launch_reset()
        out = run(everything, res, acc)
        assert {k: n for k, n in launch_counts().items() if n} == {"hifigan_conv_f16": 1}
        for i, T in enumerate(C.CONV_ROWS):
            C.check_operator(f"conv {cin}->{cout}{' cf' if cf else ''} k={taps} d={d} {tag} T={T}", out[i, :T].T.cpu(), ref(i, 0, res, acc), ref(i, 1, res, acc))
            assert bool((out[i, T:] == 7.0).all())                            # nothing is written beyond the utterance
        assert torch.equal(run(everything, res, acc), out)                    # run to run
    # a ragged batch [T, 1, 37] at two paddings: every utterance is its single run, bit for bit
    idx = [5, 0, 6]
    single = [run([i], True, 2) for i in idx]
    for Tmax in (200, 200 + TILE + 1):
        batch = run(idx, True, 2, Tmax)
        for bi, i in enumerate(idx):
            assert torch.equal(batch[bi, :lengths[i]], single[bi][0]), (Tmax, bi)
            assert bool((batch[bi, lengths[i]:] == 7.0).all())


@gpu
@pytest.mark.parametrize("u, k", C.UP_KERNELS)
@pytest.mark.parametrize("cin, cout", C.UP_CHANNELS)
def test_upsample_against_the_contract_and_ragged_bit_identity(cin, cout, u, k):
    v = voc("narrow")
    g = torch.Generator().manual_seed(100 * u + k + cin)
    w = (torch.rand(cin, cout, k, generator=g) * 2 - 1) / (cout * k) ** 0.5
    b = torch.rand(cout, generator=g) * 2 - 1
    xs = [torch.randn(T, cin, generator=g) for T in C.UP_ROWS]

    def run(idx, Tmax=None):
        Tmax = Tmax or max(C.UP_ROWS[i] for i in idx)
        out = torch.full((len(idx), u * Tmax, cout), 7.0, device="cuda")
        return v.upsample(None, G.pad_rows([xs[i] for i in idx], Tmax), [C.UP_ROWS[i] for i in idx], out=out, weight=w, bias=b, rate=u)

    launch_reset()
    out = run(list(range(len(C.UP_ROWS))))
    assert {k_: n for k_, n in launch_counts().items() if n} == {"hifigan_upsample_f16": 1}
    for i, T in enumerate(C.UP_ROWS):
        r64, r32 = emu_pair(lambda e: e.upsample(xs[i].T, w, b, u))
        assert r64.shape == (cout, u * T)                                     # exactly u rows per input row
        C.check_operator(f"upsample {cin}->{cout} u={u} k={k} T={T}", out[i, :u * T].T.cpu(), r64, r32)
        assert bool((out[i, u * T:] == 7.0).all())
    assert torch.equal(run(list(range(len(C.UP_ROWS)))), out)                 # run to run
    idx = [3, 0, 2]
    single = [run([i]) for i in idx]
    for Tmax in (33, 33 + TILE):
        batch = run(idx, Tmax)
        for bi, i in enumerate(idx):
            n = u * C.UP_ROWS[i]
            assert torch.equal(batch[bi, :n], single[bi][0]) and bool((batch[bi, n:] == 7.0).all()), (Tmax, bi)


@gpu
def test_operators_on_the_ragged_batch_5_2_7_are_the_single_runs():
    v = voc("odd")
    g = torch.Generator().manual_seed(527)
    xs = [torch.randn(T, 32, generator=g) for T in C.RAGGED]
    key = "resblocks.2.convs1.1"
    batch = v.conv(G.pad_rows(xs), C.RAGGED, key=key, dilation=3, slope=H.SLOPE, out=torch.full((3, 7, 32), 7.0, device="cuda"))
    sd = C.sd_of("odd", G.WEIGHT_SEED)
    for b, T in enumerate(C.RAGGED):
        alone = v.conv(G.pad_rows([xs[b]]), [T], key=key, dilation=3, slope=H.SLOPE)
        assert torch.equal(alone[0], batch[b, :T]) and bool((batch[b, T:] == 7.0).all())
        r64, r32 = emu_pair(lambda e: e.conv(xs[b].T, sd[key + ".weight"], sd[key + ".bias"], 3, H.SLOPE))
        C.check_operator(f"conv own weights {key} T={T}", alone[0].T.cpu(), r64, r32)
    up = v.upsample(1, G.pad_rows(xs), C.RAGGED, out=torch.full((3, 35, 16), 7.0, device="cuda"))
    for b, T in enumerate(C.RAGGED):
        alone = v.upsample(1, G.pad_rows([xs[b]]), [T])
        assert torch.equal(alone[0], up[b, :5 * T]) and bool((up[b, 5 * T:] == 7.0).all())


@gpu
def test_subnormal_rows_decide_whether_the_mfma_keeps_fp16_subnormals():
    """Rows scaled into [1e-7, 6e-5] are fp16 subnormals once rounded (the smallest normal is 6.1e-5); zero bias, so that the output is their products
    alone.  The contract as hifigan_f16_cases.FLUSH_SUBNORMALS states it must hold at the operator bar; the other reading is far outside it."""
    v = voc("narrow")
    g = torch.Generator().manual_seed(77)
    cin, cout, taps, T = 32, 16, 3, 70
    mag = 10.0 ** (torch.rand(T, cin, generator=g) * (np.log10(6e-5) - np.log10(1e-7)) + np.log10(1e-7))
    x = mag * torch.where(torch.rand(T, cin, generator=g) < 0.5, -1.0, 1.0)
    assert float(x.abs().min()) >= 1e-7 and float(x.abs().max()) <= 6e-5
    w, b = (torch.rand(cout, cin, taps, generator=g) * 2 - 1), torch.zeros(cout)
    out = v.conv(G.pad_rows([x]), [T], weight=w, bias=b)[0].T.cpu()
    keep, flush = R.emus(False), R.emus(True)
    k64, k32, f64 = keep[0].conv(x.T, w, b), keep[1].conv(x.T, w, b), flush[0].conv(x.T, w, b)
    scale = float(k64.abs().max())
    print(f"subnormal rows: max|kept| {scale:.3e}  |got - kept| / scale {C.dist(out, k64) / scale:.3e}  |got - flushed| / scale {C.dist(out, f64) / scale:.3e}  "
          f"max|flushed| {float(f64.abs().max()):.3e}  max|got| {float(out.abs().max()):.3e}")
    assert float(f64.abs().max()) == 0.0 and scale > 1e-6                     # the two readings are far apart
    if C.FLUSH_SUBNORMALS:
        assert float(out.abs().max()) == 0.0
    else:
        C.check_operator("subnormal rows, kept", out, k64, k32)


@gpu
def test_a_row_value_of_1e6_is_clamped_to_65504():
    v = voc("narrow")
    g = torch.Generator().manual_seed(78)
    cin, cout, taps, T = 16, 16, 3, 20
    x = torch.randn(T, cin, generator=g)
    x[7, 3], x[11, 5] = 1.0e6, -1.0e6
    w, b = (torch.rand(cout, cin, taps, generator=g) * 2 - 1) / (cin * taps) ** 0.5, torch.rand(cout, generator=g)
    for slope in (None, H.SLOPE):                                             # -1e6 * 0.1 = -1e5 is clamped too
        out = v.conv(G.pad_rows([x]), [T], weight=w, bias=b, slope=1.0 if slope is None else slope)[0].T.cpu()
        r64, r32 = emu_pair(lambda e: e.conv(x.T, w, b, 1, slope))
        assert bool(torch.isfinite(out).all()) and float(r64.abs().max()) > 1e3    # 65504 times a weight of up to 0.14
        C.check_operator(f"1e6 row, slope {slope}", out, r64, r32)
    unclamped = H.conv(x.T.double(), w.double(), b.double())
    assert C.dist(unclamped, r64) > 1e4                                       # the clamp is what the case is about


# ---------------------------------------------------------------------------------------------------------------- 2. whole generator
@gpu
@pytest.mark.parametrize("name, seed, lengths", C.GENERATOR_CASES)
def test_generator_against_ref64_and_the_contract_and_batch_independence(name, seed, lengths):
    cfg, v = C.CFGS[name], voc(name, seed)
    hop = H.hop(cfg)
    refs = [C.reference(name, seed, L) for L in lengths]
    mels = [r["mel"] for r in refs]
    wav, n, rows = v(*G.pad_mels(mels), return_rows=True)
    assert wav.shape == (len(lengths), max(lengths) * hop) and n.tolist() == [L * hop for L in lengths]
    for b, (L, ref) in enumerate(zip(lengths, refs)):
        for i, (what, got) in enumerate((("wav", wav[b, :L * hop]), ("rows", rows[b, :L * hop].T))):
            scale, e_f16, e32 = C.figures(ref, i)
            print(f"{name} seed {seed} {lengths} utterance {b} {what}: max|ref64| {scale:.3e}  e_f16 / scale {e_f16 / scale:.3e}  e_f16 / e32 {e_f16 / e32:.0f}")
            C.check_generator(f"f16 {name} seed {seed} {lengths} utterance {b} {what}", got.cpu(), ref, i, name != "default")
        assert bool((wav[b, L * hop:] == 0).all())
    again, _ = v(*G.pad_mels(mels))                                           # run to run
    assert torch.equal(again, wav)
    if len(lengths) > 1:
        wide, _ = v(*G.pad_mels(mels, max(lengths) + 3))
        for b, L in enumerate(lengths):
            alone, _ = v(*G.pad_mels([mels[b]]))
            assert torch.equal(alone[0], wav[b, :L * hop]) and torch.equal(wide[b, :L * hop], alone[0]), b
            assert bool((wide[b, L * hop:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 3. the path was taken
@gpu
@pytest.mark.parametrize("name", ["narrow", "odd", "default"])
def test_launch_plan_is_f16_launches_and_f32_stays_f32(name):
    from torch.utils._python_dispatch import TorchDispatchMode
    from glow_tts_amd.vocoder import hifigan_launches
    cfg, v, f32 = C.CFGS[name], voc(name), G.voc(name)
    assert (v.precision, v.geo["precision"], f32.precision, f32.geo["precision"]) == ("f16", "f16", "f32", "f32")
    lengths = C.RAGGED if name != "default" else [3]
    mels = [C.mel_of(name, L) for L in lengths]
    v(*G.pad_mels(mels))                                                      # buffers exist
    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    launch_reset()
    with Record():
        wav, _ = v(*G.pad_mels(mels))
    counts = {k: c for k, c in launch_counts().items() if c}
    convs = hifigan_launches(v.geo) - 2 - len(cfg["rates"])
    assert counts == {"hifigan_conv_f16": 1 + convs, "hifigan_upsample_f16": len(cfg["rates"]), "hifigan_conv,post": 1}, counts
    assert sum(counts.values()) == hifigan_launches(v.geo) and (name != "default" or sum(counts.values()) == 78)
    assert seen and not [s for s in seen if any(w in s for w in ("conv", "mm", "matmul", "linear", "einsum", "dot", "bmm"))], seen
    launch_reset()
    wav32, _ = f32(*G.pad_mels(mels))
    counts = {k: c for k, c in launch_counts().items() if c}
    assert counts == {"hifigan_conv": 1 + convs, "hifigan_upsample": len(cfg["rates"]), "hifigan_conv,post": 1}, counts
    explicit, _ = voc(name, precision="f32")(*G.pad_mels(mels))
    assert torch.equal(explicit, wav32) and not torch.equal(wav, wav32)       # the default is the f32 path bit for bit; f16 is not the f32 waveform
    for b, L in enumerate(lengths):                                           # and that f32 waveform is still right, at the f32 suite's own bar
        _, (w64, _), (w32, _) = G.reference(name, L)
        G.check(f"f32 generator {name} utterance {b} wav", wav32[b, :L * H.hop(cfg)], w64, w32)


# ---------------------------------------------------------------------------------------------------------------- 4. plumbing
@gpu
def test_yaml_key_selects_f16_the_argument_overrides_and_a_trainable_generator_stays_f32():
    from glow_tts_amd.vocoder import HiFiGAN, make_vocoder
    name = "narrow"
    cfg, sd = C.CFGS[name], {"generator": C.sd_of(name, G.WEIGHT_SEED)}
    hp = G._hp(cfg)
    hp.Vocoder.Precision = "f16"
    by_key, back, trainable = HiFiGAN(hp, "cuda:0", state_dict=sd), HiFiGAN(hp, "cuda:0", state_dict=sd, precision="f32"), HiFiGAN(hp, "cuda:0", state_dict=sd, trainable=True)
    assert (by_key.precision, by_key.geo["precision"], back.precision, back.geo["precision"], trainable.precision, trainable.geo["precision"]) == \
        ("f16", "f16", "f32", "f32", "f32", "f32")
    mels, lengths = G.pad_mels([C.mel_of(name, L) for L in C.RAGGED])
    wav16, wav32 = voc(name)(mels, lengths)[0], G.voc(name)(mels, lengths)[0]
    assert torch.equal(by_key(mels, lengths)[0], wav16) and torch.equal(back(mels, lengths)[0], wav32)
    launch_reset()
    wav, _ = trainable.generate(mels, lengths)
    counts = {k: c for k, c in launch_counts().items() if c}
    assert counts.get("hifigan_conv") and not [k for k in counts if k.endswith("_f16")] and torch.equal(wav.detach(), wav32)
    assert torch.equal(trainable(mels, lengths)[0], wav32)
    with pytest.raises(ValueError, match="trainable"):
        HiFiGAN(hp, "cuda:0", state_dict=sd, trainable=True, precision="f16")
    import tempfile
    with tempfile.TemporaryDirectory() as root:
        torch.save(sd, os.path.join(root, "g.pt"))
        made = make_vocoder(G._hp(cfg), "cuda:0", "hifigan", checkpoint=os.path.join(root, "g.pt"), precision="f16")
    assert made.precision == "f16" and torch.equal(made(mels, lengths)[0], wav16)


@pytest.mark.late(1)
@gpu
def test_inferencer_vocodes_in_f16_like_the_direct_call(tmp_path):
    from scipy.io import wavfile
    from glow_tts_amd.inferencer import Inferencer
    from glow_tts_amd.vocoder import HiFiGAN
    root = str(tmp_path)
    ckpt = os.path.join(root, "hifigan.pt")
    hp = G._tiny_setup(root, G.block_of(G.TINY))
    inf = Inferencer(os.path.join(root, "S_0.pt"), hp=hp, vocoder="hifigan", vocoder_checkpoint=ckpt, vocoder_precision="f16")
    g = torch.Generator().manual_seed(3)
    labels, mels = ["A", "B", "C"], [(torch.rand(T, 12, generator=g) * 8 - 4).numpy() for T in (9, 4, 13)]
    launch_reset()
    files = inf.Vocode(labels, mels, os.path.join(root, "f16"))
    counts = {k: c for k, c in launch_counts().items() if c}
    assert isinstance(inf._vocoder, HiFiGAN) and inf._vocoder.precision == "f16"
    assert counts.get("hifigan_upsample_f16") == 2 * 3 and not counts.get("hifigan_upsample") and not counts.get("hifigan_conv")      # two batches
    direct = HiFiGAN(hp, "cuda:0", state_dict=torch.load(ckpt), precision="f16")
    f32 = HiFiGAN(hp, "cuda:0", state_dict=torch.load(ckpt))
    differs = False
    for m, path in zip(mels, files):
        mel = torch.from_numpy(m).T[None].cuda()
        want = direct.to_host(*direct(mel, [m.shape[0]]))[0]
        other = f32.to_host(*f32(mel, [m.shape[0]]))[0]
        sr, y = wavfile.read(path)
        assert sr == hp.Sound.Sample_Rate and y.dtype == np.int16 and y.shape == (m.shape[0] * hp.Sound.Frame_Shift,)
        ref_path = os.path.join(root, "direct.wav")
        from glow_tts_amd import audio
        audio.write_wav(ref_path, want, hp.Sound.Sample_Rate)
        assert np.array_equal(wavfile.read(ref_path)[1], y)                   # the same PCM as the direct call
        differs = differs or not np.array_equal(want, other)
    assert differs                                                            # and f16 was not silently f32
    by_key = Inferencer(os.path.join(root, "S_0.pt"), hp=G._tiny_setup(root, G.block_of(G.TINY, Checkpoint_Path=ckpt, Precision="f16")))
    again = by_key.Vocode(labels, mels, os.path.join(root, "key"))
    assert by_key._vocoder.precision == "f16" and [open(w, "rb").read() for w in again] == [open(w, "rb").read() for w in files]
    sys.path.insert(0, os.path.join(G.REPO, "tools"))                         # the comparison tool on the two utterances long enough for its analyses
    import compare_hifigan_precision
    rows = compare_hifigan_precision.compare(hp, ckpt, [(labels[i], mels[i]) for i in (0, 2)])
    assert [r["label"] for r in rows] == ["A", "C"]
    for r, i in zip(rows, (0, 2)):
        print(r)
        assert r["samples"] == mels[i].shape[0] * hp.Sound.Frame_Shift
        assert np.isfinite(r["snr_db"]) and r["snr_db"] > 20 and all(np.isfinite(r[k]) and r[k] > 0 for k in ("stft_loss", "mel_l1"))
