"""Shared inputs and float64 yardsticks of the analysis front end's tests (test_pattern_generator_cpu.py, test_gpu_frontend.py): hyper-parameters at the two
geometries, synthetic corpora in the LJ / VCTK / list layouts, the per-element mel error bar and a float64 YIN (difference function summed directly) with the
decision margins; the float32 copy of the YIN with sequential summation sizes the error bars, never serves as a reference.  The product never imports it."""
import os

import numpy as np

import griffin_lim_ref as R

GEOS = {"full": ((2048, 1024, 256), 80), "tiny": ((256, 256, 64), 20)}
SR = 24000
U = 2.0 ** -24


def hp_dict(geo="full", root=None, **sound):
    from glow_tts_amd.hparams import DEFAULT_YAML, load_yaml
    d = load_yaml(DEFAULT_YAML)
    (n_fft, win, hop), mel = GEOS[geo]
    d["Sound"].update(Spectrogram_Dim=n_fft // 2 + 1, Frame_Length=win, Frame_Shift=hop, Mel_Dim=mel)
    d["Sound"].update(sound)
    if root is not None:
        d["Token_Path"] = os.path.join(root, "Token.yaml")
        d["Train"]["Train_Pattern"]["Path"] = os.path.join(root, "train")
        d["Train"]["Eval_Pattern"]["Path"] = os.path.join(root, "eval")
    return d


def hp(geo="full", root=None, **sound):
    from glow_tts_amd.hparams import Recursive_Parse
    return Recursive_Parse(hp_dict(geo, root, **sound))


def write_hp(root, geo="full", **sound):
    """Writes <root>/Hyper_Parameters.yaml with the pattern and token paths under root; returns (path, parsed hp)."""
    import yaml
    path = os.path.join(root, "Hyper_Parameters.yaml")
    with open(path, "w") as f:
        yaml.dump(hp_dict(geo, root, **sound), f)
    return path, hp(geo, root, **sound)


_SIGNAL = {}


def signal32():
    if "x" not in _SIGNAL:
        _SIGNAL["x"] = R.make_signal().astype(np.float32)
    return _SIGNAL["x"]


def utterance(i, seconds, sr=SR):
    """A cut of the synthetic signal between 0.12 s of near-silence on either side (so that the trim has something to decide), as int16."""
    x = R.make_signal(seed=10 + i, sample_rate=sr, seconds=seconds)
    quiet = 1e-4 * np.random.default_rng(i).standard_normal(int(0.12 * sr))
    y = np.concatenate([quiet, x, quiet])
    return np.clip(np.round(y * 32767.0 * 0.8), -32768, 32767).astype(np.int16)


LJ_TEXTS = [("LJ001-0001", "Printing, in the only sense with which we are at present concerned."),
            ("LJ001-0002", "differs from most if not from all the arts"),
            ("LJ001-0003", "Chapter 3 of 1850 costs $5"),                       # digits and a dollar sign: text_filtering rejects it
            ("LJ001-0004", "And it is worth mention in passing that, (as an example) of fine typography;")]


def make_lj_tree(root):
    """metadata.csv (id|transcription|normalised transcription) and wavs/<id>.wav; the third line's text does not pass the filter."""
    from scipy.io import wavfile
    os.makedirs(os.path.join(root, "wavs"))
    with open(os.path.join(root, "metadata.csv"), "w", encoding="utf-8") as f:
        for i, (name, text) in enumerate(LJ_TEXTS):
            f.write("{}|{}|{}\n".format(name, text, text))
            wavfile.write(os.path.join(root, "wavs", name + ".wav"), SR, utterance(i, 0.5 + 0.13 * i))
    return [n for n, _ in LJ_TEXTS]


VCTK_FILES = [("p225", "p225_001", "Please call Stella."), ("p225", "p225_002", "Ask her to bring these things with her from the store."),
              ("p226", "p226_001", "Six spoons of fresh snow peas."), ("p315", "p315_001", None)]


def make_vctk_tree(root, sr=48000):
    """wav48/<speaker>/<id>.wav at 48 kHz, txt/<speaker>/<id>.txt; p315 has no transcripts."""
    from scipy.io import wavfile
    for i, (spk, name, text) in enumerate(VCTK_FILES):
        os.makedirs(os.path.join(root, "wav48", spk), exist_ok=True)
        wavfile.write(os.path.join(root, "wav48", spk, name + ".wav"), sr, utterance(20 + i, 0.45 + 0.1 * i, sr))
        if text is not None:
            os.makedirs(os.path.join(root, "txt", spk), exist_ok=True)
            with open(os.path.join(root, "txt", spk, name + ".txt"), "w") as f:
                f.write(text + "\n")


def load_patterns(root):
    """{relative path: pattern dict} of every pattern pickle under root."""
    import pickle
    out = {}
    for base, _, files in os.walk(root):
        for name in files:
            if name.endswith(".PICKLE") and name != "METADATA.PICKLE":
                with open(os.path.join(base, name), "rb") as f:
                    out[os.path.relpath(os.path.join(base, name), root).replace("\\", "/")] = pickle.load(f)
    return out


# ---------------------------------------------------------------------------------------------------------------- mel
def mel_want_and_tol(x, hp_):
    """(audio.mel_generate on float64 input [T, Mel], per-element bar [T, Mel]).
    tol = (2 max_abs / 100) (20 / ln 10) ||fb_j|| eps ||S_t|| / (m64 + 1e-7) + 2^-18: the transform bound eps = 4 log2(n_fft) 2^-24 on the magnitude frame
    carried through the filter row (Cauchy-Schwarz), the derivative of 20 log10 and the normalisation's slope; 2^-18 for the fp32 dB / normalise arithmetic
    at magnitudes up to 100.  Clipping is 1-Lipschitz."""
    from glow_tts_amd import audio
    s = hp_.Sound
    n_fft = (s.Spectrogram_Dim - 1) * 2
    x = np.asarray(x, np.float64)
    want = audio.mel_generate(x, s.Sample_Rate, s.Mel_Dim, s.Spectrogram_Dim, s.Frame_Length, s.Frame_Shift, mel_fmin=s.Mel_F_Min, mel_fmax=s.Mel_F_Max,
                              max_abs_value=s.Max_Abs_Mel)
    S = audio.stft_magnitude(audio.preemphasis(x), n_fft, s.Frame_Shift, s.Frame_Length).T                      # [T, F]
    fb = audio.mel_filterbank(s.Sample_Rate, n_fft, s.Mel_Dim, s.Mel_F_Min, s.Mel_F_Max).astype(np.float64)      # [Mel, F]
    m64 = S @ fb.T
    eps = 4 * np.log2(n_fft) * U
    slope = 2.0 * float(s.Max_Abs_Mel) / 100.0
    tol = slope * (20.0 / np.log(10.0)) * np.linalg.norm(fb, axis=1)[None, :] * eps * np.linalg.norm(S, axis=1)[:, None] / (m64 + 1e-7) + 2.0 ** -18
    return want, tol


# ---------------------------------------------------------------------------------------------------------------- YIN
def yin_frames(sig, w_len, w_step, dtype=np.float64):
    """The frames `audio.yin_pitch` analyses: [frames, w_len]."""
    sig = np.asarray(sig, np.float64)
    sig = np.pad(sig, (w_step + w_len - sig.shape[0] % w_step) // 2, mode="reflect")
    starts = np.arange(0, len(sig) - w_len, w_step)
    return sig[starts[:, None] + np.arange(w_len)[None, :]].astype(dtype)


def yin_cm(frames, tau_max, dtype=np.float64):
    """Cumulative-mean-normalised difference [frames, tau_max] with d(tau) summed directly.  float32: every sum runs sequentially in float32 (cumsum)."""
    fr = np.asarray(frames, dtype)
    n, w_len = fr.shape
    d = np.zeros((n, tau_max), dtype)
    for tau in range(1, tau_max):
        sq = (fr[:, :w_len - tau] - fr[:, tau:]) ** 2
        d[:, tau] = np.cumsum(sq, axis=1, dtype=dtype)[:, -1] if np.dtype(dtype) == np.float32 else sq.sum(axis=1)
    cm = np.ones((n, tau_max), dtype)
    cm[:, 1:] = d[:, 1:] * np.arange(1, tau_max, dtype=dtype)[None, :] / (np.cumsum(d[:, 1:], axis=1, dtype=dtype) + dtype(1e-8))
    return cm


def yin_decide(cm, tau_min, tau_max, thresh):
    """Per frame (tau, 0 where unvoiced; decision margin): the smallest |cm - thresh| over the taus examined and |cm[tau + 1] - cm[tau]| along the walk,
    the comparison that ends it included."""
    taus, margins = np.zeros(len(cm), np.int64), np.zeros(len(cm))
    for i, c in enumerate(cm):
        below = np.flatnonzero(c[tau_min:tau_max] < thresh)
        if not below.size:
            margins[i] = np.abs(c[tau_min:tau_max] - thresh).min()
            continue
        tau = tau_min + int(below[0])
        m = np.abs(c[tau_min:tau + 1] - thresh).min()
        while tau + 1 < tau_max:
            m = min(m, abs(c[tau + 1] - c[tau]))
            if not c[tau + 1] < c[tau]:
                break
            tau += 1
        taus[i], margins[i] = tau, m
    return taus, margins


_YIN = {}


def yin_case(key, sig, w_len, w_step, tau_max):
    """(cm64, e = max |cm32 - cm64|) of a signal, computed once per key."""
    k = (key, w_len, w_step, tau_max)
    if k not in _YIN:
        cm64 = yin_cm(yin_frames(sig, w_len, w_step), tau_max)
        cm32 = yin_cm(yin_frames(sig, w_len, w_step, np.float32), tau_max, np.float32)
        _YIN[k] = (cm64, float(np.abs(cm32.astype(np.float64) - cm64).max()) if cm64.size else 0.0)
    return _YIN[k]
