"""CPU suite of the waveform output: pins the float64 yardstick (tests/griffin_lim_ref.py) against the front end it inverts, and the host pieces of the
vocoder path - de-emphasis, the wav writer, the --vocode list parser, the geometry errors, the exported symbols."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import griffin_lim_ref as R  # noqa: E402

N_FFT, WIN, HOP = 2048, 1024, 256


def test_istft_inverts_stft_on_interior_samples():
    x = R.make_signal()
    for n_fft, win, hop in [(N_FFT, WIN, HOP), (256, 256, 64)]:
        S = R.stft(x, n_fft, hop, win)
        assert S.shape == (1 + len(x) // hop, n_fft // 2 + 1)
        y = R.istft(S, n_fft, hop, win)
        assert y.shape == (hop * (S.shape[0] - 1),)
        err = np.abs(y[n_fft:-n_fft] - x[n_fft:len(y) - n_fft]).max()
        assert err <= 1e-12, err


def test_stft_magnitude_equals_the_front_ends():
    from glow_tts_amd import audio
    x = R.make_signal()
    for n_fft, win, hop in [(N_FFT, WIN, HOP), (256, 256, 64)]:
        err = np.abs(np.abs(R.stft(x, n_fft, hop, win)).T - audio.stft_magnitude(x, n_fft, hop, win)).max()
        assert err <= 1e-12, err


def test_float32_copy_of_the_restatement_is_single_precision():
    """The error bars of the GPU tests are sized by the float32 copy: it must really run in float32 and sit near, not on, the float64 values."""
    x = R.make_signal()[:20000]
    S64, S32 = R.stft(x, N_FFT, HOP, WIN), R.stft(x, N_FFT, HOP, WIN, np.float32)
    assert S32.dtype == np.complex64 and R.istft(S32, N_FFT, HOP, WIN, np.float32).dtype == np.float32
    rel = np.linalg.norm(S32 - S64) / np.linalg.norm(S64)
    assert 1e-9 < rel < 4 * 11 * 2.0 ** -24, rel


def test_deemphasis_inverts_preemphasis():
    from glow_tts_amd import audio
    x = R.make_signal()
    assert np.abs(audio.deemphasis(audio.preemphasis(x)) - x).max() <= 1e-10
    assert np.abs(audio.deemphasis(audio.preemphasis(x, 0.9), 0.9) - x).max() <= 1e-10


def test_write_wav_round_trip(tmp_path):
    from scipy.io import wavfile
    from glow_tts_amd import audio
    x = 0.7 * R.make_signal()[:5000] / np.abs(R.make_signal()[:5000]).max()
    p = str(tmp_path / "a.wav")
    audio.write_wav(p, x.astype(np.float32), 24000)
    sr, y = wavfile.read(p)
    assert sr == 24000 and y.dtype == np.int16 and y.shape == x.shape
    assert np.abs(y.astype(np.float64) - x.astype(np.float32).astype(np.float64) * 32767.0).max() <= 1.0
    # only a signal beyond full scale is normalised, to a peak of 0.99
    audio.write_wav(p, 3.0 * x, 16000)
    sr, y = wavfile.read(p)
    assert sr == 16000 and abs(int(np.abs(y.astype(np.int32)).max()) - round(0.99 * 32767)) <= 1
    assert np.abs(y.astype(np.float64) - x / np.abs(x).max() * 0.99 * 32767.0).max() <= 1.0


def test_vocode_list_parser(tmp_path):
    from glow_tts_amd.inferencer import read_vocode_list
    p = tmp_path / "list.tsv"
    p.write_text("a\tx/a.npy\n\nb b\t y/b.npy \n", encoding="utf-8")
    assert read_vocode_list(str(p)) == [("a", "x/a.npy"), ("b b", "y/b.npy")]
    for bad in ("only_label\n", "a\tb\tc\n", "\tb.npy\n"):
        p.write_text(bad, encoding="utf-8")
        with pytest.raises(ValueError):
            read_vocode_list(str(p))


def _hp(**sound):
    from helpers import tiny_hp_dict
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Sound"].update(sound)
    return Recursive_Parse(d)


def test_geometry_errors_name_the_sound_keys():
    from glow_tts_amd import vocoder
    assert vocoder.geometry(_hp()) == (2048, 1024, 256)
    assert vocoder.geometry(_hp(Spectrogram_Dim=129, Frame_Length=256, Frame_Shift=64)) == (256, 256, 64)
    cases = [(dict(Spectrogram_Dim=1001), ["Sound.Spectrogram_Dim"]),                       # n_fft = 2000: not a power of two
             (dict(Spectrogram_Dim=65, Frame_Length=64, Frame_Shift=16), ["Sound.Spectrogram_Dim"]),     # 128 < 256
             (dict(Spectrogram_Dim=4097, Frame_Length=1024), ["Sound.Spectrogram_Dim"]),                 # 8192 > 4096
             (dict(Spectrogram_Dim=257, Frame_Length=1024), ["Sound.Frame_Length"]),                     # window longer than n_fft
             (dict(Frame_Length=1000, Frame_Shift=256), ["Sound.Frame_Length", "Sound.Frame_Shift"])]    # win % hop
    for sound, keys in cases:
        with pytest.raises(ValueError) as e:
            vocoder.GriffinLim(_hp(**sound), "cuda:0")             # raised at construction, before anything touches a device
        for k in keys:
            assert k in str(e.value), (sound, str(e.value))
    assert vocoder.settings(_hp()) == (60, 0.99)
    hp = _hp()
    from glow_tts_amd.hparams import Recursive_Parse
    hp.Griffin_Lim = Recursive_Parse({"Iterations": 32})
    assert vocoder.settings(hp) == (32, 0.99)


def test_default_yaml_documents_the_optional_block():
    text = open(os.path.join(REPO, "glow_tts_amd", "Hyper_Parameters.default.yaml")).read()
    assert re.search(r"^# Griffin_Lim: \{Iterations: 60, Momentum: 0.99\}", text, re.M)
    import yaml
    assert "Griffin_Lim" not in yaml.safe_load(text)              # commented: a reference yaml and the default stay the same schema


NEW_SYMBOLS = ["glowtts_vocoder_supported", "glowtts_mel_to_linear_f32", "glowtts_stft_f32", "glowtts_istft_f32", "glowtts_overlap_add_f32",
               "glowtts_griffin_lim_step_f32"]


def test_new_symbols_are_declared_and_exported_with_abi_7():
    header = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    assert re.search(r"#define GLOWTTS_ABI_VERSION\s+7\b", header)
    so = os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so")
    if not os.path.exists(so):
        sys.path.insert(0, REPO)
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(so)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", header), f"{n} not declared"
        assert hasattr(L, n), f"{n} not exported"
    assert L.glowtts_abi_version() == 7
    # the host-side geometry predicate agrees with the Python check
    for geo, ok in [((2048, 1024, 256), 1), ((256, 256, 64), 1), ((4096, 4096, 1024), 1), ((2000, 1000, 250), 0), ((128, 128, 32), 0), ((8192, 1024, 256), 0),
                    ((512, 1024, 256), 0), ((2048, 1000, 256), 0)]:
        assert L.glowtts_vocoder_supported(*geo) == ok, geo


def test_package_stays_free_of_library_ffts():
    """No rocFFT on the product path: the package never names torch's FFT entry points."""
    pkg = os.path.join(REPO, "glow_tts_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"torch\.fft|torch\.stft|torch\.istft|\.stft\(\s*n_fft|hipfft|rocfft", src), f
