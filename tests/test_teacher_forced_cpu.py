"""CPU suite of the teacher-forced pass: tests/teacher_forced_ref.py (the float64 restatement of glowtts_prior_sample_aligned) against brute force on
hand-sized cases; the argument errors of Align.py; `GlowTTS.teacher_forced` refusing a noise scale without seeds; the new entry point's place in the
header, the signature table and the built library."""
import math
import os
import re

import numpy as np
import pytest
import torch

import prior_sample_ref as PS
import teacher_forced_ref as R
from helpers import tiny_hp_dict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_case():
    """B = 2, C = 3, Tx = 4, Tmax = 7.  Row 0: token 1 has no frame, one index is >= Tx (treated as -1), the tail is -1; row 1: no valid frame."""
    rng = np.random.default_rng(0)
    mean = rng.normal(0, 1, (2, 3, 4)).astype(np.float32)
    log_std = rng.uniform(-1, 0.5, (2, 3, 4)).astype(np.float32)
    z_rec = rng.normal(0, 1, (2, 3, 7)).astype(np.float32)
    idx = np.array([[0, 0, 2, 9, 3, -1, -1], [-1, -1, -1, -1, 4, -7, -1]], np.int32)
    seeds = np.array([[1, 2], [0xFFFFFFFF, 7]], np.int64)
    scales = np.array([0.75, 1.0], np.float32)
    return mean, log_std, idx, z_rec, seeds, scales


def test_restatement_matches_brute_force():
    mean, log_std, idx, z_rec, seeds, scales = hand_case()
    z, dur, score = R.aligned(mean, log_std, idx, z_rec, seeds, scales)
    assert dur.dtype == np.int32 and dur.tolist() == [[2, 0, 1, 1], [0, 0, 0, 0]]
    want_z = np.zeros((2, 3, 7))
    total, count = 0.0, 0
    for y, x in ((0, 0), (1, 0), (2, 2), (4, 3)):                                  # the valid frames of row 0
        for c in range(3):
            g = float(PS.gauss(1, 2, c, y, 3))
            m, ls = float(mean[0, c, x]), float(log_std[0, c, x])
            want_z[0, c, y] = m + math.exp(ls) * g * 0.75
            total += -0.5 * math.log(2 * math.pi) - ls - 0.5 * (float(z_rec[0, c, y]) - m) ** 2 * math.exp(-2 * ls)
            count += 1
    assert np.abs(z - want_z).max() <= 1e-14 and (z[1] == 0).all() and (z[0][:, [3, 5, 6]] == 0).all()
    assert abs(score[0] - total / count) <= 1e-14 and score[1] == 0.0
    # the float32 evaluation is the same arithmetic: close, and not the float64 result
    z32, dur32, score32 = R.aligned(mean, log_std, idx, z_rec, seeds, scales, np.float32)
    assert z32.dtype == np.float32 and np.array_equal(dur32, dur) and np.abs(z32 - z).max() <= 1e-5 and abs(score32[0] - score[0]) <= 1e-5


def test_restatement_is_the_seeded_sample_along_the_same_index():
    """The index `prior_sample` builds from durations, fed back: the same z; the durations come back as the bincount."""
    rng = np.random.default_rng(1)
    B, C, Tx, Tmax = 2, 5, 6, 19
    mean, log_std = rng.normal(0, 1, (B, C, Tx)).astype(np.float32), rng.uniform(-1, 0.5, (B, C, Tx)).astype(np.float32)
    dur = np.array([[2, 0, 3, 1, 4, 0], [1, 1, 1, 0, 0, 0]], np.float32)
    lengths = dur.sum(1).astype(np.int64)
    seeds, scales = np.array([[3, 4], [5, 6]], np.int64), np.array([1.0, 0.3], np.float32)
    z, idx, _ = PS.prior_sample(mean, log_std, dur, lengths, seeds, scales, Tmax)
    assert np.array_equal(R.sample(mean, log_std, idx, seeds, scales), z)
    assert np.array_equal(R.durations(idx, Tx), dur.astype(np.int32))
    # the score of the prior's own mean is the mean of -0.5 log(2 pi) - ls over the aligned elements
    z0 = R.sample(mean, log_std, idx, seeds, np.zeros(B, np.float32))
    want = [np.mean(-0.5 * R.LOG_2PI - log_std[b].astype(np.float64)[:, idx[b][idx[b] >= 0]]) for b in range(B)]
    assert np.abs(R.score(mean, log_std, idx, z0) - want).max() <= 1e-14


def test_aligner_argument_errors(capsys):
    from glow_tts_amd import aligner
    with pytest.raises(SystemExit):
        aligner.parse_args(["-c", "x.pt", "--patterns", "train", "-o", "out", "--gta"])
    err = capsys.readouterr().err
    assert "--seed" in err and "--noise-scale" in err
    with pytest.raises(SystemExit):
        aligner.parse_args(["-c", "x.pt", "--patterns", "dev", "-o", "out"])
    assert "--patterns" in capsys.readouterr().err
    a = aligner.parse_args(["-c", "x.pt", "--patterns", "eval", "-o", "out", "--gta", "--noise-scale", "0"])      # the prior's mean needs no seed
    assert a.gta and a.seed is None and a.noise_scale == 0.0 and a.limit is None
    a = aligner.parse_args(["-c", "x.pt", "--patterns", "train", "-o", "out", "--gta", "--seed", "0", "--limit", "3"])
    assert a.seed == 0 and a.noise_scale == 1.0 and a.limit == 3
    from glow_tts_amd import inferencer
    assert a.noise_scale == inferencer.build_parser().get_default("noise_scale")                                 # Inference.py's default


def test_aligner_refuses_two_patterns_of_one_label():
    from glow_tts_amd import aligner
    aligner.check_labels(["LJ/LJ/A.PICKLE", "VCTK/P1/B.PICKLE", "VCTK/P2/C.PICKLE"])
    assert aligner.label_of("VCTK/P1/B.001.PICKLE") == "B.001"
    with pytest.raises(ValueError, match=r"VCTK/P1/A\.PICKLE.*share the label 'A'"):
        aligner.check_labels(["LJ/LJ/A.PICKLE", "VCTK/P1/B.PICKLE", "VCTK/P1/A.PICKLE"])


def test_aligned_sample_argument_errors_are_value_errors():
    """Refused on the host, before the library is touched: a sample without seeds or scales, a wrong index"""
    from glow_tts_amd import alignment
    mean, idx = torch.zeros(2, 3, 4), torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match="noise_scales"):
        alignment.aligned_sample(mean, mean, idx, None, torch.zeros(2, 2, dtype=torch.int64), None)
    with pytest.raises(ValueError, match="seeds"):
        alignment.aligned_sample(mean, mean, idx, None, None, torch.ones(2))
    for bad in (idx[0], idx[:1], idx.long()):
        with pytest.raises(ValueError, match="idx"):
            alignment.aligned_sample(mean, mean, bad, None, None, None, want_z=False)
    with pytest.raises(ValueError, match="z_rec"):
        alignment.aligned_sample(mean, mean, idx, torch.zeros(2, 3, 4), None, None, want_z=False)


def test_teacher_forced_refuses_a_noise_scale_without_seeds():
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS, TeacherForced
    model = GlowTTS(Recursive_Parse(tiny_hp_dict("Vanilla")))
    tokens, tl = torch.zeros(1, 4, dtype=torch.int64), torch.tensor([4])
    mels, ml = torch.zeros(1, 12, 8), torch.tensor([8])
    for scale in (1.0, torch.tensor([0.5])):
        with pytest.raises(ValueError, match=r"seeds.*noise_scale.*0"):
            model.teacher_forced(tokens, tl, mels, ml, noise_scale=scale)
    assert TeacherForced._fields == ("durations", "idx", "score", "z", "mels", "mel_lengths")


def test_entry_point_is_declared_tabulated_and_exported():
    import ctypes
    from glow_tts_amd import _lib, abi
    text = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    m = re.search(r"int\s+glowtts_prior_sample_aligned\s*\(([^)]*)\)\s*;", text)
    assert m, "include/glowtts_hip.h does not declare glowtts_prior_sample_aligned"
    params = [p.strip() for p in m.group(1).split(",")]
    names = [re.split(r"[\s*]+", p)[-1] for p in params]
    assert names == ["mean", "log_std", "idx", "z_rec", "seeds", "noise_scales", "z", "dur", "score", "score_partials", "B", "C", "Tx", "Tmax", "stream"]
    restype, argtypes = abi.SIGNATURES["glowtts_prior_sample_aligned"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p] * 10 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    assert "glowtts_prior_sample_aligned" not in abi.VALUE_RETURNING and abi.ABI_VERSION == 7
    # every pointer NULL: refused before anything is launched (no device is touched)
    row = (None,) * 10 + (1, 4, 3, 8, None)
    assert _lib.lib().glowtts_prior_sample_aligned(*row) == abi.E_ARG
    with pytest.raises(_lib.GlowTTSHipError, match=r"glowtts_prior_sample_aligned failed with code -1"):
        _lib.api().glowtts_prior_sample_aligned(*row)
