"""GPU suite of the analysis front end (glow_tts_amd/frontend.py on csrc/frontend_ops.hip) against `audio.mel_generate` / `audio.yin_pitch` in float64, the
vectors the reference's own yin.py wrote (tests/golden/yin_case.npz) and the host path of the pattern generator.

Inputs: `griffin_lim_ref.make_signal` (24 kHz, 72 000 samples) and cuts of it, the five signals of yin_case.npz; geometries full = (2048, 1024, 256) with 80
mels and tiny = (256, 256, 64) with 20.  The mel bar is derived in frontend_cases.mel_want_and_tol; the YIN bars are 8 x the error of a float32 numpy
restatement with sequential summation that the test computes itself on the same signal.  Every figure is printed before it is asserted (pytest -s)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import frontend_cases as C  # noqa: E402
from helpers import load_case, tiny_hp_dict  # noqa: E402

gpu = pytest.mark.gpu

CUTS = [72000, 38400, 16391]
YIN_SHAPES = {"full": (1024, 256, 48, 240, CUTS + [2148]), "tiny": (256, 64, 48, 240, [16391, 2148, 700])}
_AN = {}


def analyzer(geo="full"):
    from glow_tts_amd.frontend import Analyzer
    if geo not in _AN:
        _AN[geo] = Analyzer(C.hp(geo), "cuda:0", with_pitch=geo == "full")
    return _AN[geo]


def batch_of(cuts, x=None):
    x = C.signal32() if x is None else x
    out = np.zeros((len(cuts), max(max(cuts), 1)), np.float32)
    for b, n in enumerate(cuts):
        out[b, :n] = x[:n]
    return torch.from_numpy(out).cuda()


def check_mel(got, x, hp_, label):
    """got [T, Mel] against audio.mel_generate on the float64 signal, under the per-element bar; returns the worst |err| / bar."""
    want, tol = C.mel_want_and_tol(x, hp_)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / tol).max())
    print(f"mel[{label}]: worst |err| / bar {worst:.3f}, worst |err| {err.max():.3e}, clipped elements {int((np.abs(want) >= hp_.Sound.Max_Abs_Mel).sum())}")
    assert (err <= tol).all(), (label, worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. mel
@pytest.mark.parametrize("geo", ["full", "tiny"])
@gpu
def test_mel_against_float64(geo):
    (n_fft, win, hop), n_mel = C.GEOS[geo]
    a, hp_ = analyzer(geo), C.hp(geo)
    x = C.signal32()
    lens = CUTS + [n_fft + 100]
    got, frames = a.mel(batch_of(lens), lens)
    got = got.cpu().numpy()
    assert got.shape == (4, 1 + 72000 // hop, n_mel) and frames.dtype == torch.int64 and frames.tolist() == [1 + n // hop for n in lens]
    for b, n in enumerate(lens):
        T = 1 + n // hop
        check_mel(got[b, :T], x[:n], hp_, f"{geo}, {n} samples")
        assert (got[b, T:] == -np.float32(hp_.Sound.Max_Abs_Mel)).all()     # frames beyond the utterance: the collater's pad value, exactly


@gpu
def test_mel_edges():
    a, hp_ = analyzer(), C.hp()
    hop, top = 256, np.float32(hp_.Sound.Max_Abs_Mel)
    silence, _ = a.mel(torch.zeros(2, 4096, device="cuda"), [4096, 1000])
    assert silence.shape == (2, 17, 80) and (silence.cpu().numpy() == -top).all()
    tone = np.sin(2 * np.pi * 1000.0 * np.arange(12000) / C.SR).astype(np.float32)
    mel, _ = a.mel(torch.from_numpy(tone[None]).cuda())
    mel = mel.cpu().numpy()
    print(f"full-scale 1 kHz sine: max {mel.max()}, min {mel.min()}")
    assert np.isfinite(mel).all() and mel.max() == top and mel.min() >= -top
    for frames in (2, 3, 4):                                       # hop (T - 1) = 256 .. 768 samples under 1024 of padding: the reflection folds more than once
        n = hop * (frames - 1)
        x = C.signal32()[12000:12000 + n]
        got, fl = a.mel(torch.from_numpy(x[None].copy()).cuda())
        assert fl.tolist() == [frames]
        check_mel(got.cpu().numpy()[0], x, hp_, f"{frames} frames")
    lens = [38400, 0, 16391]                                       # an empty utterance yields no frames and disturbs no neighbour
    got, fl = a.mel(batch_of(lens), lens)
    fl = fl.tolist()
    assert fl == [151, 0, 65] and bool((got[1] == -top).all())
    for b in (0, 2):
        one, _ = a.mel(batch_of([lens[b]]))
        assert torch.equal(got[b, :fl[b]], one[0]) and bool((got[b, fl[b]:] == -top).all())


# ---------------------------------------------------------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("geo", ["full", "tiny"])
@gpu
def test_ragged_batch_equals_single_runs_bit_for_bit(geo):
    (n_fft, win, hop), _ = C.GEOS[geo]
    w_len, w_step, tau_min, tau_max, _ = YIN_SHAPES[geo]
    a = analyzer(geo)
    lens = CUTS + [n_fft + 100]
    wav = batch_of(lens)
    yin = lambda w, n: a.yin(w, n, thresh=0.4, w_len=w_len, w_step=w_step, tau_min=tau_min, tau_max=tau_max, with_cmnd=True)
    mel, fl = a.mel(wav, lens)
    hz, pf, cm = yin(wav, lens)
    fl, pf = fl.tolist(), pf.tolist()
    assert np.count_nonzero(hz.cpu().numpy()) > 20                 # the input does have voiced frames
    for b, n in enumerate(lens):
        one = batch_of([n])
        m1, f1 = a.mel(one)
        h1, p1, c1 = yin(one, [n])
        assert f1.tolist() == [fl[b]] and p1.tolist() == [pf[b]] and p1[0] == len(C.yin_frames(np.zeros(n), w_len, w_step))
        assert torch.equal(mel[b, :fl[b]], m1[0]), b
        assert torch.equal(hz[b, :pf[b]], h1[0]) and not hz[b, pf[b]:].any(), b
        assert torch.equal(cm[b, :pf[b]], c1[0]) and not cm[b, pf[b]:].any(), b
    mel2, _ = a.mel(wav, lens)
    hz2, _, cm2 = yin(wav, lens)
    assert torch.equal(mel, mel2) and torch.equal(hz, hz2) and torch.equal(cm, cm2)


# ---------------------------------------------------------------------------------------------------------------- 3. YIN
def _golden():
    return np.load(os.path.join(HERE, "golden", "yin_case.npz"))


NAMES = ("glide", "vowel", "noise", "mix", "odd")
_GOLD = {}


def golden_run(thr):
    """Device Hz per signal of yin_case.npz at a threshold (one ragged batch), computed once."""
    if thr not in _GOLD:
        d = _golden()
        sigs = [d[f"{n}/sig"].astype(np.float32) for n in NAMES]
        wav = np.zeros((len(sigs), max(len(s) for s in sigs)), np.float32)
        for b, s in enumerate(sigs):
            wav[b, :len(s)] = s
        hz, frames, _ = analyzer().yin(torch.from_numpy(wav).cuda(), [len(s) for s in sigs], thresh=thr)
        hz, frames = hz.cpu().numpy(), frames.tolist()
        _GOLD[thr] = {n: hz[b, :frames[b]] for b, n in enumerate(NAMES)}
    return _GOLD[thr]


@gpu
def test_yin_against_the_reference_vectors():
    """Frame by frame against `compute_yin` of the reference's yin.py.  A differing frame is tolerated only when its float64 decision margin is positive and below
    8 e (e: the float32 restatement's largest |cm32 - cm64| on that signal), and at most 1 % of all frames may differ.  Frames of margin 0 (the silent stretch
    of `vowel`) must match exactly."""
    d = _golden()
    assert int(d["sr"]) == C.SR and (analyzer().tau_min, analyzer().tau_max) == (48, 240)
    total = differing = 0
    for name in NAMES:
        cm64, e = C.yin_case(name, d[f"{name}/sig"], 1024, 256, 240)
        for thr in (0.15, 0.4):
            want, got = d[f"{name}/yin_{thr}"], golden_run(thr)[name]
            assert got.shape == want.shape, (name, got.shape, want.shape)
            taus, margins = C.yin_decide(cm64, 48, 240, thr)
            assert np.array_equal(np.where(taus > 0, C.SR / np.maximum(taus, 1), 0.0), want), name      # the float64 yardstick reproduces the vectors
            bad = np.flatnonzero(got != want.astype(np.float32))
            total, differing = total + len(want), differing + len(bad)
            print(f"yin[{name}, {thr}]: {len(want)} frames, {int((want > 0).sum())} voiced, {len(bad)} differ, e {e:.2e}, "
                  f"smallest margin {margins.min():.2e}" + (f", margins of the differing frames {margins[bad]}" if len(bad) else ""))
            exact = margins == 0                                   # silence: both sides compute exact zeros, so these frames must match whatever e is
            assert np.array_equal(got[exact], want.astype(np.float32)[exact]), (name, thr, np.flatnonzero(exact & (got != want.astype(np.float32))))
            assert ((margins[bad] > 0) & (margins[bad] < 8 * e)).all(), (name, thr, bad, margins[bad])
            if name == "vowel":
                assert exact.sum() >= 10                           # the silent stretch is there
    print(f"yin: {differing} of {total} frames differ")
    assert total == 1044 and differing <= 0.01 * total


@pytest.mark.parametrize("shape", ["full", "tiny"])
@gpu
def test_yin_cmnd_and_pitch_against_float64(shape):
    from glow_tts_amd import audio
    w_len, w_step, tau_min, tau_max, cuts = YIN_SHAPES[shape]
    a = analyzer(shape)
    x = C.signal32()
    hz, frames, cm = a.yin(batch_of(cuts), cuts, thresh=0.4, w_len=w_len, w_step=w_step, tau_min=tau_min, tau_max=tau_max, with_cmnd=True)
    hz, cm, frames = hz.cpu().numpy(), cm.cpu().numpy(), frames.tolist()
    total = left_out = 0
    for b, n in enumerate(cuts):
        cm64, e = C.yin_case(("signal", n), x[:n], w_len, w_step, tau_max)
        want = audio.yin_pitch(x[:n], C.SR, 0.4, w_len=w_len, w_step=w_step)
        assert frames[b] == len(want) == len(cm64), (n, frames[b], len(want))
        err = float(np.abs(cm[b, :frames[b]].astype(np.float64) - cm64).max())
        _, margins = C.yin_decide(cm64, tau_min, tau_max, 0.4)
        safe = margins > 8 * e
        got = hz[b, :frames[b]]
        print(f"yin[{shape}, {n} samples]: {frames[b]} frames, max |cmnd - cm64| {err:.3e} (bar {8 * e:.3e}), {int((~safe).sum())} frames left out, "
              f"smallest margin {margins.min():.2e}, {int((got[safe] != want.astype(np.float32)[safe]).sum())} mismatches among the rest")
        assert err <= 8 * e
        assert np.array_equal(got[safe], want.astype(np.float32)[safe])
        total, left_out = total + len(want), left_out + int((~safe).sum())
    print(f"yin[{shape}]: {left_out} of {total} frames left out by the margin rule")
    assert left_out <= 0.02 * total


@gpu
def test_normalised_track_equals_pitch_generate():
    """Analyzer.pitch against audio.pitch_generate within 1e-6 at (confidence 0.6, sigma 0) and (0.85, sigma 1: host smoothing), on the signals of
    yin_case.npz whose YIN frames agree with the vectors."""
    from glow_tts_amd import audio
    from glow_tts_amd.frontend import Analyzer
    d = _golden()
    compared = 0
    for conf, sigma, thr in ((0.6, 0.0, 0.4), (0.85, 1.0, 0.15)):
        hp_ = C.hp(Confidence_Threshold=conf, Gaussian_Smoothing_Sigma=sigma)
        a = Analyzer(hp_, "cuda:0")
        for name in NAMES:
            if not np.array_equal(golden_run(thr)[name], d[f"{name}/yin_{thr}"].astype(np.float32)):
                print(f"pitch[{name}, {conf}, {sigma}]: YIN frames differ, not compared")
                continue
            sig = d[f"{name}/sig"].astype(np.float32)
            got, frames = a.pitch(torch.from_numpy(sig[None]).cuda())
            want = audio.pitch_generate(sig, hp_)
            assert frames.tolist() == [len(want)]
            err = float(np.abs(got.cpu().numpy()[0, :len(want)].astype(np.float64) - want).max())
            print(f"pitch[{name}, confidence {conf}, sigma {sigma}]: max |err| {err:.2e}")
            assert err <= 1e-6 and got.dtype == torch.float32
            compared += 1
    assert compared >= 6


# ---------------------------------------------------------------------------------------------------------------- 4. lists of utterances
@gpu
def test_call_on_a_shuffled_list_equals_single_calls():
    a = analyzer()
    x = C.signal32()
    lens = [16391, 700, 38400, 5000, 2148, 20000]                  # six lengths, not sorted
    arrays = [x[1000 + 37 * i:1000 + 37 * i + n].copy() for i, n in enumerate(lens)]
    singles = [a([arr])[0] for arr in arrays]
    for budget in (8 << 20, 60000):                                # one batch; several batches (a padded batch holds at most 60 000 samples)
        got = a(arrays, sample_budget=budget)
        assert len(got) == 6
        for (mel, pit), (m1, p1), n in zip(got, singles, lens):
            assert mel.shape == (1 + n // 256, 80) and pit.shape == (1 + n // 256,) and mel.dtype == pit.dtype == np.float32
            assert np.array_equal(mel, m1) and np.array_equal(pit, p1)
    mel_only = a(arrays, with_pitch=False)
    assert all(p is None and np.array_equal(m, s[0]) for (m, p), s in zip(mel_only, singles))


@pytest.mark.late(1)
@gpu
def test_generator_on_the_device_matches_the_host_path(tmp_path):
    from glow_tts_amd import pattern_generator
    corpus = str(tmp_path / "LJSpeech-1.1")
    C.make_lj_tree(corpus)
    runs = {}
    for mode in ("host", "device"):
        out = str(tmp_path / mode)
        os.makedirs(out)
        yml, hp_ = C.write_hp(out)
        res = pattern_generator.main(["-hp", yml, "-lj", corpus, "-text", "-evalm", "1", "-mw", "2"] + (["--host"] if mode == "host" else []))
        assert res["written"] == 3 and res["failed"] == 0
        runs[mode] = (C.load_patterns(hp_.Train.Train_Pattern.Path), C.load_patterns(hp_.Train.Eval_Pattern.Path))
    for host, dev in zip(runs["host"], runs["device"]):            # the same files in the same split
        assert sorted(host) == sorted(dev) and len(host) > 0
        for rel in host:
            h, g = host[rel], dev[rel]
            assert set(h) == set(g) and all(h[k] == g[k] for k in ("Speaker_ID", "Speaker", "Dataset", "Text"))
            assert g["Audio"].dtype == g["Mel"].dtype == g["Pitch"].dtype == np.float32
            assert np.array_equal(h["Audio"], g["Audio"]) and g["Mel"].shape == h["Mel"].shape
            check_mel(g["Mel"], g["Audio"], hp_, rel)
            assert np.array_equal(h["Pitch"], g["Pitch"]), rel


def _tiny_setup(root, mode, fname):
    import yaml
    from glow_tts_amd import data
    from glow_tts_amd.hparams import Recursive_Parse
    sd, _, _ = load_case(fname)
    torch.save({"Model": sd, "Steps": 0}, os.path.join(root, "S_0.pt"))
    with open(os.path.join(root, "Token.yaml"), "w") as f:
        yaml.dump(data.make_token_dict(["HELLO WORLD."]), f)
    hp_ = tiny_hp_dict(mode)
    hp_["Token_Path"] = os.path.join(root, "Token.yaml")
    hp_["Inference_Batch_Size"] = 2
    return Recursive_Parse(hp_)


@pytest.mark.late(1)
@gpu
def test_inferencer_reference_through_the_device_front_end(tmp_path):
    from scipy.io import wavfile
    from glow_tts_amd import audio
    from glow_tts_amd.inferencer import Inferencer
    root = str(tmp_path)
    hp_ = _tiny_setup(root, "GR", "tiny_gr.npz")
    wav = os.path.join(root, "ref.wav")
    wavfile.write(wav, C.SR, C.utterance(3, 0.9))
    host = Inferencer(os.path.join(root, "S_0.pt"), hp=hp_)
    dev = Inferencer(os.path.join(root, "S_0.pt"), hp=hp_, device_frontend=True)
    assert host.device_frontend is False and host._analyzer is None
    (m0, p0), (m1, p1) = host._reference(wav), dev._reference(wav)
    assert host._analyzer is None and dev._analyzer is not None
    assert m1.dtype == p1.dtype == np.float32 and m1.shape == m0.shape == (p0.shape[0], 12) and p1.shape == p0.shape
    check_mel(m1, audio.audio_prep(wav, C.SR, 30), hp_, "reference wav")
    assert np.array_equal(p0, p1)                                  # GR: the pitch track
    assert np.array_equal(dev._reference(m0)[0], m0)               # arrays and .npy references are untouched by the option


# ---------------------------------------------------------------------------------------------------------------- 5. registers
def test_frontend_kernels_use_no_scratch_memory(tmp_path):
    """As test_gpu_griffin_lim.test_vocoder_kernels_use_no_scratch_memory, for the kernels of csrc/frontend_ops.hip (code-object metadata; nothing is executed)."""
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    assert os.path.exists(f"{llvm}/llvm-objdump") and os.path.exists(f"{llvm}/llvm-readelf"), "ROCm LLVM tools not found"
    shutil.copy(os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    kernels = {}
    for f in [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        for name, scratch, vgpr in re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S):
            kernels[name] = (int(scratch), int(vgpr))
    want = {r"mel_analysis_kernel": 0, r"yin_kernel": 0}
    for name, (scratch, vgpr) in kernels.items():
        for h in want:
            if re.search(h, name):
                want[h] += 1
                print(f"{name}: {vgpr} VGPRs, {scratch} bytes of scratch")
                assert scratch == 0, f"{name} spills: {scratch} bytes of scratch per lane at {vgpr} VGPRs"
    assert all(n > 0 for n in want.values()), want
