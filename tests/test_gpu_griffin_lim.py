"""GPU suite of the waveform output (glow_tts_amd/vocoder.py on csrc/vocoder_ops.hip) against the float64 numpy restatement tests/griffin_lim_ref.py.

Input: the synthetic signal of `griffin_lim_ref.make_signal` (24 kHz, 3 s, a 39-harmonic tone with a wandering f0, a syllable-like envelope, 2 % noise, fixed
seed: T = 282 frames at hop 256), a ragged batch of it (T = 282 / 150 / 64 / 9), cuts of 2 to 4 frames and the tiny geometry n_fft 256, win 256, hop 64.

Where a bar is "20 x the float32 restatement's error", the test computes that error itself on the same input: the float32 numpy copy shows what single
precision costs on this input with numpy's FFT; the factor 20 covers a different FFT factorisation and summation order.  Every figure is printed before
it is asserted (pytest -s)."""
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

import griffin_lim_ref as R  # noqa: E402
from helpers import load_case, tiny_hp_dict  # noqa: E402

gpu = pytest.mark.gpu

GEOS = {"full": (2048, 1024, 256), "tiny": (256, 256, 64)}
RAGGED_T = [282, 150, 64, 9]
U = 2.0 ** -24


def _hp(geo="full"):
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    d = load_yaml(DEFAULT_YAML)
    n_fft, win, hop = GEOS[geo]
    d["Sound"].update(Spectrogram_Dim=n_fft // 2 + 1, Frame_Length=win, Frame_Shift=hop)
    return Recursive_Parse(d)


_VOC = {}


def voc(geo="full"):
    from glow_tts_amd.vocoder import GriffinLim
    if geo not in _VOC:
        _VOC[geo] = GriffinLim(_hp(geo), "cuda:0")
    return _VOC[geo]


def signal32():
    return R.make_signal().astype(np.float32)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def case(geo):
    """(target magnitudes [T, F] fp32 = |STFT64(signal)|, start phase [T, F] fp32)"""
    n_fft, win, hop = GEOS[geo]
    S = np.abs(R.stft(signal32().astype(np.float64), n_fft, hop, win)).astype(np.float32)
    ph = np.random.default_rng(1).uniform(-np.pi, np.pi, S.shape).astype(np.float32)
    return S, ph


def gpu_gl(geo, S, ph, lengths, iterations, momentum=0.99):
    v = voc(geo)
    w, n = v.griffin_lim(torch.from_numpy(S).cuda(), lengths, iterations, momentum, None if ph is None else torch.from_numpy(ph).cuda())
    torch.cuda.synchronize()
    return w.cpu().numpy(), n.cpu().tolist()


# ---------------------------------------------------------------------------------------------------------------- 1. the transforms
@pytest.mark.parametrize("geo", ["full", "tiny"])
@gpu
def test_stft_against_float64(geo):
    """Per-frame relative L2 error of the complex spectrum <= 4 log2(n_fft) 2^-24 (the fp32 FFT error bound with exact twiddles), single and ragged."""
    n_fft, win, hop = GEOS[geo]
    bar = 4 * np.log2(n_fft) * U
    x = signal32()
    lens = [len(x), 38400, 16384 + 7, n_fft + 100]
    batch = np.zeros((4, len(x)), np.float32)
    for b, n in enumerate(lens):
        batch[b, :n] = x[:n]
    got = voc(geo).stft(torch.from_numpy(batch).cuda(), lens).cpu().numpy()
    single = voc(geo).stft(torch.from_numpy(x[None]).cuda()).cpu().numpy()
    assert got.shape == (4, 1 + len(x) // hop, n_fft // 2 + 1) and np.array_equal(got[0], single[0])
    worst = 0.0
    for b, n in enumerate(lens):
        want = R.stft(x[:n].astype(np.float64), n_fft, hop, win)
        T = want.shape[0]
        assert T == 1 + n // hop
        err = np.linalg.norm(got[b, :T] - want, axis=1) / np.linalg.norm(want, axis=1)
        worst = max(worst, float(err.max()))
        assert not got[b, T:].any()                                # frames beyond the utterance: zeros
    print(f"stft[{geo}]: worst per-frame relative L2 {worst:.3e} (bar {bar:.3e})")
    assert worst <= bar


@pytest.mark.parametrize("geo", ["full", "tiny"])
@gpu
def test_istft_against_float64(geo):
    n_fft, win, hop = GEOS[geo]
    bar = 4 * np.log2(n_fft) * U
    x = signal32().astype(np.float64)
    S = R.stft(x, n_fft, hop, win).astype(np.complex64)
    T = S.shape[0]
    specs = np.zeros((len(RAGGED_T), T, S.shape[1]), np.complex64)
    for b, t in enumerate(RAGGED_T):
        specs[b, :t] = S[:t]
    got = voc(geo).istft(torch.from_numpy(specs).cuda(), RAGGED_T).cpu().numpy()
    assert got.shape == (len(RAGGED_T), hop * (T - 1))
    worst = 0.0
    for b, t in enumerate(RAGGED_T):
        want = R.istft(S[:t].astype(np.complex128), n_fft, hop, win)
        worst = max(worst, rel(got[b, :hop * (t - 1)], want))
        assert not got[b, hop * (t - 1):].any()
    print(f"istft[{geo}]: worst relative L2 over an utterance {worst:.3e} (bar {bar:.3e})")
    assert worst <= bar
    again = voc(geo).istft(torch.from_numpy(specs).cuda(), RAGGED_T).cpu().numpy()
    assert np.array_equal(got, again)                              # a gather, no atomics: bit-identical


# ---------------------------------------------------------------------------------------------------------------- 2. mel -> linear
@gpu
def test_mel_to_linear_against_float64():
    """Per element |err| <= (Mel + 8) 2^-24 sum_k |P_fk| |amp_k| (the dot-product bound plus a few ulp for the exponential); padded frames exactly zero."""
    v = voc()
    rng = np.random.default_rng(2)
    B, Mel, T = 4, v.n_mel, 282
    mels = rng.uniform(-4.5, 4.5, (B, Mel, T)).astype(np.float32)
    mels[0, :, :40] = -4.0
    mels[1, :, :40] = 4.0
    got = v.mel_to_linear(torch.from_numpy(mels).cuda(), RAGGED_T).cpu().numpy()
    basis = v.basis.cpu().numpy().astype(np.float64)              # the table the kernel reads: float64 pseudo-inverse rounded once
    assert np.abs(basis - R.mel_basis_pinv(24000, 2048, Mel, 125, 7600)).max() <= U * np.abs(basis).max()
    worst = 0.0
    for b, t in enumerate(RAGGED_T):
        m = mels[b].astype(np.float64)[:, :t]
        want = R.mel_to_linear(m, basis, 4.0)
        bound = (Mel + 8) * U * (np.abs(basis) @ R.mel_amplitude(m, 4.0)).T
        err = np.abs(got[b, :t] - want)
        err[(got[b, :t] == np.float32(1e-10)) & (want == 1e-10)] = 0.0      # both on the clamp: equal up to the fp32 rounding of the constant
        assert not err[bound == 0].any()                                   # bins above Mel_F_Max: all-zero basis rows
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert not got[b, t:].any() and got[b, :t].min() >= 1e-10
    print(f"mel_to_linear: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 3. a few iterations
@pytest.mark.parametrize("geo", ["full", "tiny"])
@pytest.mark.parametrize("iterations", [1, 3])
@gpu
def test_iterations_against_float64(geo, iterations):
    n_fft, win, hop = GEOS[geo]
    S, ph = case(geo)
    want = R.griffin_lim(S, ph, n_fft, hop, win, iterations, 0.99)
    e32 = rel(R.griffin_lim(S, ph, n_fft, hop, win, iterations, 0.99, np.float32), want)
    got, n = gpu_gl(geo, S[None], ph[None], [S.shape[0]], iterations)
    assert n == [hop * (S.shape[0] - 1)] and got.shape == (1, n[0])
    e = rel(got[0], want)
    print(f"griffin_lim[{geo}, {iterations} it]: relative L2 {e:.3e}, float32 restatement {e32:.3e} (bar {20 * e32:.3e})")
    assert e <= 20 * e32


@pytest.mark.parametrize("frames", [2, 3, 4])
@gpu
def test_short_utterance_reflects_more_than_once(frames):
    """hop (T - 1) = 256 .. 768 samples under n_fft / 2 = 1024 samples of padding: the reflection folds back several times (numpy's `reflect`, period
    2 (L - 1)).  The STFT under the operator bar of item 1, three iterations under the 20 x float32 bar of item 3, both against the float64 restatement."""
    n_fft, win, hop = GEOS["full"]
    L = hop * (frames - 1)
    x = signal32()[12000:12000 + L]
    want = R.stft(x.astype(np.float64), n_fft, hop, win)
    assert want.shape[0] == frames
    got = voc().stft(torch.from_numpy(x[None].copy()).cuda()).cpu().numpy()[0]
    err = float((np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)).max())
    bar = 4 * np.log2(n_fft) * U
    print(f"stft[T = {frames}]: worst per-frame relative L2 {err:.3e} (bar {bar:.3e})")
    assert err <= bar
    S = np.abs(want).astype(np.float32)
    ph = np.random.default_rng(1).uniform(-np.pi, np.pi, S.shape).astype(np.float32)
    want = R.griffin_lim(S, ph, n_fft, hop, win, 3, 0.99)
    e32 = rel(R.griffin_lim(S, ph, n_fft, hop, win, 3, 0.99, np.float32), want)
    y, n = gpu_gl("full", S[None], ph[None], [frames], 3)
    e = rel(y[0], want)
    print(f"griffin_lim[T = {frames}, 3 it]: relative L2 {e:.3e}, float32 restatement {e32:.3e} (bar {20 * e32:.3e})")
    assert n == [L] and e <= 20 * e32


# ---------------------------------------------------------------------------------------------------------------- 4. sixty iterations
@gpu
def test_sixty_iterations_converge_like_float64():
    n_fft, win, hop = GEOS["full"]
    S, ph = case("full")
    sc = {}
    for it in (3, 32, 60):
        got, _ = gpu_gl("full", S[None], ph[None], [S.shape[0]], it)
        sc[it] = R.spectral_convergence(got[0], S, n_fft, hop, win)
    want = R.griffin_lim(S, ph, n_fft, hop, win, 60, 0.99)
    sc64 = R.spectral_convergence(want, S, n_fft, hop, win)
    e32 = rel(R.griffin_lim(S, ph, n_fft, hop, win, 60, 0.99, np.float32), want)
    e = rel(got[0], want)
    print(f"spectral convergence: {sc[3]:.4f} (3) {sc[32]:.4f} (32) {sc[60]:.4f} (60); float64 at 60: {sc64:.4f}; waveform relative L2 {e:.3e}, "
          f"float32 restatement {e32:.3e} (bar {20 * e32:.3e})")
    assert abs(sc[60] - sc64) <= 0.02 * sc64
    assert sc[60] < sc[32] < sc[3]
    assert e <= 20 * e32


# ---------------------------------------------------------------------------------------------------------------- 5. from a mel
@gpu
def test_from_a_mel_lines_up_with_the_front_end():
    """audio.mel_generate(signal) -> GriffinLim -> deemphasis -> audio.mel_generate: the RMS difference to the input mel is no worse than the float64
    restatement's on the same start, plus 0.01 (denormalisation, basis, lengths and de-emphasis line up with the front end)."""
    from glow_tts_amd import audio
    v = voc()
    n_fft, win, hop = GEOS["full"]
    gen = lambda a: audio.mel_generate(a, 24000, v.n_mel, n_fft // 2 + 1, win, hop, mel_fmin=125, mel_fmax=7600, max_abs_value=4.0)
    mel = gen(signal32().astype(np.float64))                      # [T, Mel]
    T = mel.shape[0]
    ph = np.random.default_rng(1).uniform(-np.pi, np.pi, (T, n_fft // 2 + 1)).astype(np.float32)
    w, n = v(torch.from_numpy(mel.T[None].copy()).cuda(), [T], iterations=60, initial_phase=torch.from_numpy(ph[None]).cuda())
    host = v.to_host(w, n)
    assert len(host) == 1 and host[0].shape == (hop * (T - 1),) and host[0].dtype == np.float32
    rms = float(np.sqrt(np.mean((gen(host[0].astype(np.float64)) - mel) ** 2)))
    mag64 = R.mel_to_linear(mel.T.astype(np.float64), R.mel_basis_pinv(24000, n_fft, v.n_mel, 125, 7600), 4.0)
    w64 = audio.deemphasis(R.griffin_lim(mag64, ph, n_fft, hop, win, 60, 0.99))
    rms64 = float(np.sqrt(np.mean((gen(w64) - mel) ** 2)))
    print(f"mel -> wav -> mel: RMS difference {rms:.4f}, float64 restatement {rms64:.4f} (bar {rms64 + 0.01:.4f})")
    assert rms <= rms64 + 0.01


# ---------------------------------------------------------------------------------------------------------------- 6. ragged batch
@pytest.mark.parametrize("geo", ["full", "tiny"])
@gpu
def test_ragged_batch_equals_single_runs_bit_for_bit(geo):
    n_fft, win, hop = GEOS[geo]
    S, ph = case(geo)
    T = S.shape[0]
    lens = RAGGED_T if T >= 282 else [T, T // 2, 64, 9]
    lens = [min(t, T) for t in lens]
    lens[0] = T
    mags, phs = np.zeros((4,) + S.shape, np.float32), np.zeros((4,) + S.shape, np.float32)
    for b, t in enumerate(lens):
        mags[b, :t], phs[b, :t] = S[:t], ph[:t]
    got, n = gpu_gl(geo, mags, phs, lens, 8)
    assert n == [hop * (t - 1) for t in lens]
    for b, t in enumerate(lens):
        one, _ = gpu_gl(geo, S[None, :t], ph[None, :t], [t], 8)
        assert np.array_equal(got[b, :n[b]], one[0]), b
        assert not got[b, n[b]:].any() and np.isfinite(got[b]).all() and np.abs(got[b, :n[b]]).max() > 0
    again, _ = gpu_gl(geo, mags, phs, lens, 8)
    assert np.array_equal(got, again)
    torch.manual_seed(5)
    a, _ = gpu_gl(geo, mags, None, lens, 4)
    torch.manual_seed(5)
    b_, _ = gpu_gl(geo, mags, None, lens, 4)
    torch.manual_seed(6)
    c, _ = gpu_gl(geo, mags, None, lens, 4)
    assert np.array_equal(a, b_) and not np.array_equal(a, c)


@gpu
def test_unsupported_arguments_are_refused():
    from glow_tts_amd import _lib
    v = voc()
    with pytest.raises(ValueError):
        v.mel_to_linear(torch.zeros(1, v.n_mel + 1, 8, device="cuda"), [8])
    with pytest.raises(ValueError):
        v.griffin_lim(torch.ones(1, 8, v.n_freq, device="cuda"), [8], 1, 0.99, torch.zeros(1, 7, v.n_freq, device="cuda"))
    with pytest.raises(_lib.GlowTTSHipError):                      # a host tensor: the HIP path has no CPU fallback
        v.griffin_lim(torch.ones(1, 8, v.n_freq), [8], 1)


# ---------------------------------------------------------------------------------------------------------------- 7. entry points
_CHILD = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, {repo!r})
from glow_tts_amd import inferencer
root = {root!r}
os.chdir(root)
inferencer.main(["-c", os.path.join(root, "S_0.pt"), "--convert", os.path.join(root, "convert.tsv"), "-o", os.path.join(root, "cli"), "--wav"])
inferencer.main(["-c", os.path.join(root, "S_0.pt"), "--vocode", os.path.join(root, "vocode.tsv"), "-o", os.path.join(root, "voc")])
"""


def _tiny_setup(root, mode, fname):
    import yaml
    from glow_tts_amd import data
    from glow_tts_amd.hparams import Recursive_Parse
    sd, _, _ = load_case(fname)
    torch.save({"Model": sd, "Steps": 0}, os.path.join(root, "S_0.pt"))
    with open(os.path.join(root, "Token.yaml"), "w") as f:
        yaml.dump(data.make_token_dict(["HELLO WORLD."]), f)
    hp = tiny_hp_dict(mode)
    hp["Token_Path"] = os.path.join(root, "Token.yaml")
    hp["Inference_Batch_Size"] = 2
    hp["Griffin_Lim"] = {"Iterations": 8}
    with open(os.path.join(root, "Hyper_Parameters.yaml"), "w") as f:
        yaml.dump(hp, f)
    return Recursive_Parse(hp)


@pytest.mark.late(1)
@gpu
def test_inference_writes_wavs_and_vocode_reproduces_them(tmp_path):
    from scipy.io import wavfile
    from glow_tts_amd.inferencer import Inferencer
    root = str(tmp_path)
    hp = _tiny_setup(root, "Vanilla", "tiny_vanilla.npz")
    inf = Inferencer(os.path.join(root, "S_0.pt"), hp=hp)
    assert inf._vocoder is None
    inner, calls = inf._write_wavs, [0]

    def seeded(*a, **k):                                           # the default start comes from torch's device generator: seed every vocoder call
        torch.manual_seed(100 + calls[0])
        calls[0] += 1
        return inner(*a, **k)
    inf._write_wavs = seeded
    labels, texts, scales = ["A", "B", "C"], ["HELLO WORLD.", "HELLO.", "WORLD WORLD HELLO."], [1.0, 1.2, 0.9]
    plain = inf.Inference(labels, texts, scales, inference_path=os.path.join(root, "plain"), noise_scale=0.0)
    assert inf.last_wav_files == [] and not os.path.exists(os.path.join(root, "plain", "WAV")) and inf._vocoder is None
    files = inf.Inference(labels, texts, scales, inference_path=os.path.join(root, "wav"), noise_scale=0.0, wav=True)
    assert [os.path.basename(f) for f in files] == [x + ".npy" for x in labels] and all(f.endswith(".npy") for f in files)
    assert [os.path.relpath(f, root) for f in inf.last_wav_files] == [os.path.join("wav", "WAV", x + ".wav") for x in labels]
    wavs = []
    for p, q, w in zip(plain, files, inf.last_wav_files):
        assert open(p, "rb").read() == open(q, "rb").read()       # the mel output is what it is without the option
        T = np.load(q).shape[0]
        sr, y = wavfile.read(w)
        assert sr == hp.Sound.Sample_Rate and y.dtype == np.int16 and y.shape == (hp.Sound.Frame_Shift * (T - 1),) and np.abs(y.astype(np.int32)).max() > 0
        wavs.append(open(w, "rb").read())
    calls[0] = 0
    again = inf.Vocode(labels, files, os.path.join(root, "voc"))
    assert again == inf.last_wav_files and [os.path.basename(f) for f in again] == [x + ".wav" for x in labels]
    for w, data_ in zip(again, wavs):
        assert open(w, "rb").read() == data_
    calls[0] = 0
    arrays = inf.Vocode(labels, [np.load(f) for f in files], os.path.join(root, "voc2"))
    assert [open(w, "rb").read() for w in arrays] == wavs


@pytest.mark.late(1)
@gpu
def test_cli_convert_with_wav_and_vocode(tmp_path):
    from scipy.io import wavfile
    root = str(tmp_path)
    hp = _tiny_setup(root, "SE", "tiny_se.npz")
    rng = np.random.default_rng(3)
    lens = [57, 40, 23]
    for i, n in enumerate(lens):
        np.save(os.path.join(root, f"src{i}.npy"), rng.normal(0, 1.5, (n, 12)).clip(-4, 4).astype(np.float32))
    with open(os.path.join(root, "convert.tsv"), "w") as f:
        for i in range(3):
            f.write(f"V{i}\t{root}/src{i}.npy\t{i}\t{4 - i}\t\n")
    with open(os.path.join(root, "vocode.tsv"), "w") as f:
        for i in range(3):
            f.write(f"M{i}\t{root}/src{i}.npy\n")
    p = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO, root=root)], env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    for i, n in enumerate(lens):
        T = np.load(os.path.join(root, "cli", "NPY", f"V{i}.npy")).shape[0]
        assert T == (n // 2) * 2
        for path, frames in ((os.path.join(root, "cli", "WAV", f"V{i}.wav"), T), (os.path.join(root, "voc", "WAV", f"M{i}.wav"), n)):
            sr, y = wavfile.read(path)
            assert sr == hp.Sound.Sample_Rate and y.dtype == np.int16 and y.shape == (hp.Sound.Frame_Shift * (frames - 1),), path
        assert f"cli/WAV/V{i}.wav" in p.stdout and f"voc/WAV/M{i}.wav" in p.stdout
    assert not os.path.exists(os.path.join(root, "voc", "NPY"))


# ---------------------------------------------------------------------------------------------------------------- 8. registers
def test_vocoder_kernels_use_no_scratch_memory(tmp_path):
    """As test_abi.test_hot_kernels_use_no_scratch_memory, for the kernels of csrc/vocoder_ops.hip (code-object metadata; nothing is executed)."""
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
    want = {r"vocoder_frame_kernelILi0E": 0, r"vocoder_frame_kernelILi1E": 0, r"vocoder_frame_kernelILi2E": 0, r"vocoder_ola_kernel": 0,
            r"vocoder_mel_to_linear_kernel": 0}
    for name, (scratch, vgpr) in kernels.items():
        for h in want:
            if re.search(h, name):
                want[h] += 1
                print(f"{name}: {vgpr} VGPRs, {scratch} bytes of scratch")
                assert scratch == 0, f"{name} spills: {scratch} bytes of scratch per lane at {vgpr} VGPRs"
    assert all(n > 0 for n in want.values()), want
