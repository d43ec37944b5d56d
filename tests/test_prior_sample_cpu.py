"""CPU suite of seeded sampling: the noise contract (csrc/gauss_hash.h, restated in tests/prior_sample_ref.py) - its statistics at N = 2^20 draws, the
independence of the streams of related seeds, golden values - and the structure around it (C ABI entry, seed words of the entry point, command line).
Every bar is 5 sigma for N independent standard normals: mean 5 / sqrt(N), variance 5 sqrt(2 / N), excess kurtosis 5 sqrt(24 / N), correlations
5 / sqrt(N), tail share 5 sqrt(p (1 - p) / N) with p = P(|x| > 3) = 2.700e-3."""
import os
import re

import numpy as np
import pytest

import prior_sample_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 20
C = 80                                                   # Sound.Mel_Dim of the default model
T = N // C + 2


def stream(s0, s1):
    """N draws in the layout of z: channel-major, frames contiguous"""
    return R.noise(s0, s1, C, T).reshape(-1)[:N]


def corr(a, b, lag):
    a = (a - a.mean()) / a.std()
    b = (b - b.mean()) / b.std()
    if lag >= 0:
        return float((a[:N - lag] * b[lag:]).mean())
    return float((a[-lag:] * b[:N + lag]).mean())


@pytest.fixture(scope="module")
def base():
    return stream(*R.seed_words(0, "statistics", 0))


def test_restatement_statistics(base):
    x = base
    mean, var = x.mean(), x.var()
    kurt = ((x - mean) ** 4).mean() / var ** 2 - 3.0
    tail = (np.abs(x) > 3.0).mean()
    auto = [corr(x, x, lag) for lag in (1, 2, 3, 4)]
    print(f"mean {mean:.3e} var-1 {var - 1:.3e} kurt {kurt:.3e} tail {tail:.4e} auto {auto} max {np.abs(x).max():.3f}")
    assert abs(mean) <= 4.9e-3
    assert abs(var - 1.0) <= 6.9e-3
    assert abs(kurt) <= 2.4e-2
    assert max(abs(a) for a in auto) <= 4.9e-3
    assert abs(tail - 2.700e-3) <= 2.5e-4
    assert np.abs(x).max() <= 5.77                       # sqrt(-2 ln 2^-24): the largest radius a 24-bit u1 gives
    # the frame-major order (the counter's own order) is as uncorrelated as the channel-major one
    xt = R.noise(*R.seed_words(0, "statistics", 0), C, T).T.reshape(-1)[:N]
    assert max(abs(corr(xt, xt, lag)) for lag in (1, 2, 3, 4)) <= 4.9e-3


def test_streams_of_related_seeds_are_independent():
    s, a, b = 0x00C0FFEE, 0xDEADBEEF, 0x01234567
    pairs = [((s, 0), (s + 1, 0)), ((s, 0), ((s + 0x9E3779B1) & 0xFFFFFFFF, 0)),                      # (s, s + 1), (s, s + K) in the first word ...
             ((0, s), (0, s + 1)), ((0, s), (0, (s + 0x9E3779B1) & 0xFFFFFFFF)),                      # ... and in the second
             ((a, b), (b, a)), ((a, b), (a, b + 1))]
    for p, q in pairs:
        u, v = stream(*p), stream(*q)
        worst = max(abs(corr(u, v, lag)) for lag in range(-4, 5))
        print(p, q, worst)
        assert worst <= 4.9e-3, (p, q, worst)
        assert (u == v).mean() < 1e-3                    # neither equal ...
        for lag in (1, 2, 3, 4):                         # ... nor shifted
            assert (u[lag:] == v[:N - lag]).mean() < 1e-3 and (v[lag:] == u[:N - lag]).mean() < 1e-3


GOLDEN_1_2_C12 = [0.6804174128778339, -0.8961580153433145, 0.2276204608545471, -1.3771353724623425,
                  0.15448593361231655, -0.4201199298192559, -0.11809634256899468, -0.9390946424156337]


GOLDEN_KEYS = [913717668, 1655065684, 3006241722]                                    # (k0, k1, k2) of seeds (1, 2)
GOLDEN_H1 = [2280535614, 1060987163, 3370114475]                                     # the draws of pair counters 0, 1, 2
GOLDEN_H2 = [3665133986, 2516242820, 344900755]


def test_golden_values_pin_the_contract():
    """The first 8 values (channel 0, frames 0..7) for seeds (1, 2), C = 12; the keys and the first draws as integers."""
    got = R.noise(1, 2, 12, 8)[0]
    assert np.allclose(got, GOLDEN_1_2_C12, rtol=0, atol=1e-12), got.tolist()
    assert [int(k) for k in R.keys(1, 2)] == GOLDEN_KEYS
    h1, h2 = R.draws(1, 2, np.arange(3, dtype=np.uint32))
    assert h1.tolist() == GOLDEN_H1 and h2.tolist() == GOLDEN_H2
    # frames 2j and 2j + 1 share one Box-Muller pair (cosine, sine): their squares add up to the pair's squared radius -2 ln u1
    g = R.noise(1, 2, 12, 8)
    h1, _ = R.draws(1, 2, (np.arange(4)[None, :] * 12 + np.arange(12)[:, None]).astype(np.uint32))
    u1 = ((h1 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    assert np.allclose(g[:, 0::2] ** 2 + g[:, 1::2] ** 2, -2.0 * np.log(u1), rtol=0, atol=1e-12)
    # a pure function of (seed, channel, frame, C): the values do not depend on how many frames are drawn
    assert np.array_equal(R.noise(1, 2, 12, 8), R.noise(1, 2, 12, 31)[:, :8])




def test_seed_words_of_the_entry_point():
    from glow_tts_amd.inferencer import utterance_seed_words
    assert utterance_seed_words(7, "Alpha", 0) == (2499690753, 1716153205)
    assert R.seed_words(7, "Alpha", 0) == (2499690753, 1716153205)
    assert utterance_seed_words(7, "Alpha", 1) != utterance_seed_words(7, "Alpha", 0) != utterance_seed_words(7, "Bravo", 0)
    assert utterance_seed_words(71, "", 0) != utterance_seed_words(7, "1", 0)          # the separators keep the fields apart


def test_seed_word_buffer_keeps_the_bit_patterns():
    import torch
    from glow_tts_amd.alignment import seed_words
    want = np.array([[1, 2], [0xFFFFFFFF, 2499690753]], np.uint32)
    for t in (torch.tensor(want.astype(np.int64)), torch.tensor(want.astype(np.int64)) + (1 << 32), torch.from_numpy(want.view(np.int32).copy())):
        got = seed_words(t, 2, "cpu")
        assert got.dtype == torch.int32 and np.array_equal(got.numpy().view(np.uint32), want)
    with pytest.raises(ValueError):
        seed_words(torch.zeros(2, 3, dtype=torch.int64), 2, "cpu")
    with pytest.raises(ValueError):
        seed_words(torch.zeros(2, 2), 2, "cpu")


def test_header_and_signature_table_declare_the_entry():
    from glow_tts_amd import abi
    text = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"int\s+glowtts_prior_sample\s*\(([^)]*)\)\s*;", text)
    assert m, "include/glowtts_hip.h does not declare glowtts_prior_sample"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert len(params) == 14 and params[4] == "const uint32_t *seeds" and params[5] == "const float *noise_scales" and params[-1] == "void *stream"
    restype, argtypes = abi.SIGNATURES["glowtts_prior_sample"]
    assert restype is abi.I and argtypes == [abi.P] * 9 + [abi.I] * 4 + [abi.P]
    assert abi.SAMPLE_SCAN_CHUNK >= 256 and abi.SAMPLE_TILE % 4 == 0
    assert abi.ABI_VERSION == 7


def test_inference_command_line_parses_the_sampling_flags():
    from glow_tts_amd import inferencer
    args = inferencer.build_parser().parse_args(["-c", "x.pt", "--seed", "7", "--noise-scale", "0.667", "--samples", "3", "--wav"])
    assert args.seed == 7 and args.noise_scale == 0.667 and args.samples == 3 and args.wav
    args = inferencer.build_parser().parse_args(["-c", "x.pt"])
    assert args.seed is None and args.noise_scale == 1.0 and args.samples == 1


def test_sampling_argument_checks_name_both_arguments():
    import torch
    from glow_tts_amd.modules import GlowTTS
    with pytest.raises(ValueError, match=r"seeds.*noises"):
        GlowTTS._check_sampling_args(1.0, torch.zeros(1, 2, 3), torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"noise_scale.*seeds"):
        GlowTTS._check_sampling_args(torch.ones(3), None, None)
    GlowTTS._check_sampling_args(torch.ones(3), None, torch.zeros(3, 2, dtype=torch.int64))
    GlowTTS._check_sampling_args(torch.tensor(0.5), None, None)
