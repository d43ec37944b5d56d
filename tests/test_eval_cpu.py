"""CPU suite of the objective evaluation (glow_tts_amd/evaluation.py, Evaluate.py): the float64 restatement tests/eval_ref.py against brute force and scipy, the
cepstrum's contract against `audio.mel_generate`, the F0 metrics on hand-made tracks, the list reader, the yaml block, the command line and the new C symbols.
Nothing here touches a device."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import eval_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("glowtts_mel_cepstrum_supported", "glowtts_mel_cepstrum", "glowtts_dtw_supported", "glowtts_dtw_work_bytes", "glowtts_dtw")


def test_restated_dtw_equals_brute_force_up_to_5x5():
    """Every shape up to 5 x 5, integer features in a small range (exact arithmetic, many ties): the cost is the minimum over ALL monotone paths and the
    path is the one the tie-break picks among the minimal ones; all-equal sequences make every path of max(Tx, Ty) .. steps tie."""
    rng = np.random.default_rng(0)
    for tx, ty in itertools.product(range(1, 6), repeat=2):
        cases = [(np.zeros((tx, 1)), np.zeros((ty, 1)))] + [(rng.integers(-2, 3, (tx, 1)).astype(np.float64), rng.integers(-2, 3, (ty, 1)).astype(np.float64))
                                                             for _ in range(8)]
        for x, y in cases:                                                            # (one feature: the local cost is |difference|, an integer)
            cost, ix, iy, moves = R.dtw(x, y)
            best, paths = R.brute_force_dtw(x, y)
            assert cost == best, (tx, ty)
            assert tuple(zip(ix.tolist(), iy.tolist())) == R.tie_break_path(paths), (tx, ty)
            assert sum(moves) == len(ix) - 1 and moves[0] + moves[1] == tx - 1 and moves[0] + moves[2] == ty - 1
            c32, ix32, iy32, _ = R.dtw(x, y, np.float32)
            assert c32 == cost and np.array_equal(ix32, ix) and np.array_equal(iy32, iy)          # exact inputs: float32 is exact too


def test_restated_cepstrum_equals_scipy_dct():
    from scipy.fft import dct
    rng = np.random.default_rng(1)
    for mel_dim, K in ((80, 13), (80, 32), (20, 19), (12, 1)):
        mel = rng.uniform(-4, 4, (37, mel_dim))
        want = dct(R.log_amplitude(mel), type=2, norm="ortho", axis=1)[:, 1:K + 1]
        got = R.cepstrum(mel, K)
        assert got.shape == (37, K) and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        from glow_tts_amd import evaluation
        assert np.array_equal(evaluation.dct_basis(mel_dim, K), R.dct_basis(mel_dim, K))
        f32 = R.cepstrum(mel.astype(np.float32), K, dtype=np.float32)
        assert f32.dtype == np.float32 and np.abs(f32 - got).max() <= 1e-4 * np.abs(want).max()
    shifted = R.cepstrum(mel + 0.25, 1)                                                      # a constant offset drops out of every k >= 1
    assert np.abs(shifted - R.cepstrum(mel, 1)).max() <= 1e-12


def test_cepstrum_of_mel_generate_is_the_dct_of_log_amplitudes():
    """`audio.mel_generate`'s normalisation undone: on frames with no clipped bin the cepstrum is the DCT of ln(mag + 1e-7)."""
    from scipy.fft import dct
    from glow_tts_amd import audio
    sr, n_mel, n_freq, win, hop = 22050, 80, 513, 1024, 256
    rng = np.random.default_rng(2)
    t = np.arange(sr // 2) / sr
    x = (0.4 * np.sin(2 * np.pi * (200 + 600 * t) * t) + 0.05 * rng.standard_normal(t.size)).astype(np.float32)
    mel = audio.mel_generate(x, sr, n_mel, n_freq, win, hop)
    mag = audio.mel_filterbank(sr, (n_freq - 1) * 2, n_mel, 125, 7600) @ audio.stft_magnitude(audio.preemphasis(x), (n_freq - 1) * 2, hop, win)
    want = dct(np.log(mag.T + 1e-7), type=2, norm="ortho", axis=1)[:, 1:14]
    clean = (np.abs(mel) < 4.0).all(1)
    assert clean.sum() >= 10
    got = R.cepstrum(mel, 13)
    assert np.abs(got[clean] - want[clean]).max() <= 2e-5                                     # (the mel is stored in float32: 2.4e-7 * 1.44 per bin)


class _Path:
    def __init__(self, ix, iy):
        n = max(len(a) for a in ix)
        self.ix = torch.tensor([list(a) + [-1] * (n - len(a)) for a in ix], dtype=torch.int32)
        self.iy = torch.tensor([list(a) + [-1] * (n - len(a)) for a in iy], dtype=torch.int32)


def test_f0_metrics_on_hand_made_tracks():
    from glow_tts_amd.evaluation import f0_metrics
    # pair 0: steps (0,0) (1,1) (2,1) (3,2): both voiced at steps 0 and 3 - one octave up, then equal; voicing differs at step 2
    # pair 1: no step where both are voiced
    path = _Path([[0, 1, 2, 3], [0, 1]], [[0, 1, 1, 2], [0, 0]])
    ref = torch.tensor([[100.0, 0.0, 150.0, 220.0], [0.0, 120.0, 0.0, 0.0]])
    cand = torch.tensor([[200.0, 0.0, 220.0], [0.0, 130.0, 0.0]])
    got = f0_metrics(path, ref, cand)
    assert got[0]["voiced_steps"] == 2 and got[0]["f0_rmse_cents"] == pytest.approx(np.sqrt((1200.0 ** 2 + 0.0) / 2), rel=1e-12)
    assert got[0]["vuv_error"] == pytest.approx(1 / 4)
    assert got[1] == {"f0_rmse_cents": None, "vuv_error": pytest.approx(1 / 2), "voiced_steps": 0}
    for b, (ix, iy) in enumerate(zip(([0, 1, 2, 3], [0, 1]), ([0, 1, 1, 2], [0, 0]))):
        rmse, vuv, n = R.f0_metrics(np.array(ix), np.array(iy), ref[b].numpy(), cand[b].numpy())
        assert n == got[b]["voiced_steps"] and vuv == pytest.approx(got[b]["vuv_error"]) and (rmse is None) == (got[b]["f0_rmse_cents"] is None)
        if rmse is not None:
            assert rmse == pytest.approx(got[b]["f0_rmse_cents"], rel=1e-12)


def test_pairs_list_reader_and_its_errors(tmp_path):
    from glow_tts_amd.evaluation import read_pairs_list
    p = tmp_path / "pairs.tsv"
    p.write_text("a\tr.npy\tc.npy\n\n b \t r.wav \t c.wav \n")
    assert read_pairs_list(str(p)) == [("a", "r.npy", "c.npy"), ("b", "r.wav", "c.wav")]
    p.write_text("a\tr.npy\tc.npy\n\nb\tr.npy\n")
    with pytest.raises(ValueError, match=r"pairs\.tsv:3: expected label<TAB>reference<TAB>candidate"):
        read_pairs_list(str(p))
    p.write_text("a\t\tc.npy\n")
    with pytest.raises(ValueError, match=r"pairs\.tsv:1:"):
        read_pairs_list(str(p))


def test_evaluation_block_defaults_and_unknown_key():
    from glow_tts_amd.evaluation import evaluation_settings
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    d = load_yaml(DEFAULT_YAML)
    assert "Evaluation" not in d and "# Evaluation: {Cepstral_Coefficients: 13}" in open(DEFAULT_YAML).read()
    assert evaluation_settings(Recursive_Parse(d)) == {"Cepstral_Coefficients": 13}          # absent block: a reference yaml drops in unchanged
    assert evaluation_settings(Recursive_Parse(dict(d, Evaluation={"Cepstral_Coefficients": 24}))) == {"Cepstral_Coefficients": 24}
    assert evaluation_settings(Recursive_Parse(dict(d, Evaluation={}))) == {"Cepstral_Coefficients": 13}
    with pytest.raises(ValueError, match=r"Evaluation\.Band"):
        evaluation_settings(Recursive_Parse(dict(d, Evaluation={"Band": 10})))
    for bad in (0, 65, "13", 2.5):
        with pytest.raises(ValueError, match=r"Evaluation\.Cepstral_Coefficients"):
            evaluation_settings(Recursive_Parse(dict(d, Evaluation={"Cepstral_Coefficients": bad})))


def test_parser_modes_are_mutually_exclusive():
    from glow_tts_amd.evaluation import build_parser
    ap = build_parser()
    a = ap.parse_args(["--pairs", "l.tsv", "-o", "d"])
    assert a.pairs == "l.tsv" and a.patterns is None and a.out == "d" and a.seed == 0 and not a.device_frontend and a.speaker_encoder is None
    assert ap.parse_args(["-c", "x.pt", "--patterns"]).patterns == -1                         # all of them
    a = ap.parse_args(["-c", "x.pt", "--patterns", "3", "--seed", "7", "--speaker-encoder", "g.pt", "--device-frontend"])
    assert (a.patterns, a.seed, a.checkpoint, a.speaker_encoder, a.device_frontend) == (3, 7, "x.pt", "g.pt", True)
    for argv in (["--pairs", "l.tsv", "--patterns", "3"], []):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
    src = open(os.path.join(REPO, "Evaluate.py")).read()
    assert "from glow_tts_amd.evaluation import" in src and "main()" in src


def test_new_prototypes_are_declared_tabulated_and_exported():
    from glow_tts_amd import _lib, abi
    header = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in abi.SIGNATURES, n
        assert hasattr(_lib.lib(), n), n
    assert {"glowtts_dtw_supported", "glowtts_mel_cepstrum_supported"} <= abi.VALUE_RETURNING
    assert abi.SIGNATURES["glowtts_dtw_work_bytes"][0] is ctypes.c_int64
    assert abi.ABI_VERSION == 7 and _lib.lib().glowtts_abi_version() == 7
    assert (abi.DTW_MAX_FRAMES, abi.DTW_MAX_K) == (4096, 64)
    A = _lib.api()
    assert A.glowtts_dtw_supported(4096, 4096, 13) == 1 and A.glowtts_dtw_supported(800, 800, 32) == 1
    assert A.glowtts_dtw_supported(4097, 10, 13) == 0 and A.glowtts_dtw_supported(10, 4097, 13) == 0 and A.glowtts_dtw_supported(10, 10, 65) == 0
    assert A.glowtts_dtw_supported(0, 10, 13) == 0 and A.glowtts_dtw_supported(10, 10, 0) == 0
    assert A.glowtts_dtw_work_bytes(800, 800) == 800 * 200 and A.glowtts_dtw_work_bytes(3, 5) == 3 * 2
    assert A.glowtts_mel_cepstrum_supported(80, 13) == 1 and A.glowtts_mel_cepstrum_supported(80, 32) == 1 and A.glowtts_mel_cepstrum_supported(20, 19) == 1
    assert A.glowtts_mel_cepstrum_supported(20, 20) == 0 and A.glowtts_mel_cepstrum_supported(80, 0) == 0


def test_null_pointers_are_refused_before_any_launch():
    from glow_tts_amd import _lib, abi
    row = (None,) * 10 + (1, 8, 8, 13, None)                                                  # every pointer NULL: no device is touched
    with pytest.raises(_lib.GlowTTSHipError, match=r"glowtts_dtw failed with code -1"):
        _lib.api().glowtts_dtw(*row)
    assert _lib.lib().glowtts_dtw(*row) == abi.E_ARG
    with pytest.raises(_lib.GlowTTSHipError, match=r"glowtts_mel_cepstrum failed with code -1"):
        _lib.api().glowtts_mel_cepstrum(None, None, None, None, 1, 8, 80, 13, 640, 80, 1, 4.0, None)


def test_host_tensors_and_oversized_arguments_are_refused():
    from glow_tts_amd import _lib, evaluation
    with pytest.raises(_lib.GlowTTSHipError):
        evaluation.mel_cepstrum(torch.zeros(1, 80, 5), [5])
    with pytest.raises(_lib.GlowTTSHipError):
        evaluation.dtw(torch.zeros(1, 5, 13), [5], torch.zeros(1, 4, 13), [4])
