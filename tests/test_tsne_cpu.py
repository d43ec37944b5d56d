"""CPU suite of the embedding maps: the float64 / float32 restatement of the contract (tests/tsne_ref.py) checked on its own - entropies, symmetry, the gradient
against finite differences of the cost, sklearn's affinities where it imports - the separation and link-by-link cases the GPU tests reuse, the settings and the
command line.  No device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_ref as R  # noqa: E402


@pytest.mark.parametrize("N,perplexity", [(8, 2.0), (65, 5.0), (130, 30.0)])
def test_row_entropies_and_joint_affinities(N, perplexity):
    x = R.affinity_case(N)
    p, _ = R.conditional(R.sqdist(x), perplexity)
    assert np.abs(R.row_entropy(p) - np.log(perplexity)).max() < 1e-9
    assert np.abs(p.sum(1) - 1).max() < 1e-12 and (np.diag(p) == 0).all()
    P = R.joint(p)
    assert np.array_equal(P, P.T) and (np.diag(P) == 0).all() and abs(P.sum() - 1) < 1e-9
    assert P[~np.eye(N, dtype=bool)].min() >= 1e-12


def test_gradient_is_the_derivative_of_the_cost():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(12, 5))
    P = R.affinities(x, 3.0)
    y = rng.normal(size=(12, 2))
    g = R.gradient(P, y, 1.0)
    h = 1e-5
    fd = np.zeros_like(y)
    for i in range(12):
        for d in range(2):
            e = np.zeros_like(y)
            e[i, d] = h
            fd[i, d] = (R.kl_divergence(P, y + e) - R.kl_divergence(P, y - e)) / (2 * h)
    assert np.abs(g - fd).max() <= 1e-6 * np.abs(fd).max()
    # the cost is sum P ln(P Z / w), term by term
    w = 1 / (1 + R.sqdist(y))
    np.fill_diagonal(w, 0)
    off = ~np.eye(12, dtype=bool)
    assert abs(R.kl_divergence(P, y) - (P[off] * np.log(P[off] * w.sum() / w[off])).sum()) < 1e-12


def test_joint_affinities_agree_with_sklearn():
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    if not hasattr(sk, "_joint_probabilities"):
        pytest.skip("sklearn.manifold._t_sne._joint_probabilities not found")
    from scipy.spatial.distance import squareform
    x = np.random.default_rng(1).normal(size=(130, 8))
    P = R.affinities(x, 30.0)
    theirs = squareform(sk._joint_probabilities(R.sqdist(x).astype(np.float32), 30.0, 0))
    assert np.abs(P - theirs).max() <= 1e-4 * P.max()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_separation_case_in_both_precisions(seed):
    _, labels, _ = R.separation_case(seed)
    y64, kl64, at = R.separation_fit(seed, np.float64)
    y32, kl32, _ = R.separation_fit(seed, np.float32)
    assert at == list(range(0, 500, 50)) + [500]
    assert R.nearest_neighbour_agreement(y64, labels) == 1.0 and R.nearest_neighbour_agreement(y32, labels) == 1.0
    print(f"seed {seed}: final KL float64 {kl64[-1]:.4f}, float32 / float64 {kl32[-1] / kl64[-1]:.4f}")
    assert abs(kl32[0] - kl64[0]) <= 1e-4 * kl64[0] and kl64[-1] < kl64[1]


def step_links(dtype, state_of):
    """The link-by-link replay of tests/tsne_ref.step_case: 12 iterations with 6 exaggerated ones.  `state_of(t, y, u, gain)` -> the state AFTER iteration t as the
    code under test computes it from (y, u, gain); each link is replayed in float64 and float32 from that code's own state, each precision over its own
    affinities of the same x (as the code under test has its own).
    -> per iteration (got, want64, want32): three (y, u, gain, g) tuples (g of `got` is None)."""
    x, y0, perplexity = R.step_case()
    P64, P32 = R.affinities(x, perplexity), R.affinities(x, perplexity, np.float32)
    y, u, gain = y0.astype(dtype), np.zeros_like(y0, dtype), np.ones_like(y0, dtype)
    out = []
    for t in range(12):
        want64 = R.step(P64, y, u, gain, t, 6, 200.0, np.float64)
        want32 = R.step(P32, y, u, gain, t, 6, 200.0, np.float32)
        # the gains in float32 arithmetic, as the kernel's, with the float64 gradient's decisions
        f = np.float32
        gain32 = np.maximum(np.where(np.sign(want64[3]) != np.sign(u), gain.astype(f) + f(0.2), gain.astype(f) * f(0.8)), f(0.01)).astype(f)
        y, u, gain = state_of(t, y, u, gain)
        out.append(((y, u, gain, None), want64[:2] + (gain32, want64[3]), want32))
    return out


def link_errors(got, want64, want32):
    """-> (error of y, bar, error of u, bar, share of gain elements left out, gains equal elsewhere): the bars are 4 x the float32 restatement's own error; a gain
    element is left out where the float64 |g| is below the gradient's bar."""
    bar = lambda k: 4.0 * np.abs(want32[k].astype(np.float64) - want64[k]).max()
    out_of = np.abs(want64[3]) < bar(3)
    same = np.array_equal(np.asarray(got[2], np.float32)[~out_of], want64[2][~out_of])
    return (np.abs(got[0] - want64[0]).max(), bar(0), np.abs(got[1] - want64[1]).max(), bar(1), float(out_of.mean()), same)


def test_step_case_leaves_no_gain_out_in_float32():
    x, _, perplexity = R.step_case()
    P32 = R.affinities(x, perplexity, np.float32)
    links = step_links(np.float32, lambda t, y, u, gain: R.step(P32, y, u, gain, t, 6, 200.0, np.float32)[:3])
    for t, (got, want64, want32) in enumerate(links):
        ey, by, eu, bu, left_out, same = link_errors(got, want64, want32)
        assert left_out == 0.0 and same, (t, left_out, same)


# ---------------------------------------------------------------------------------------------------------------- settings and the command line
def _hp(block):
    from glow_tts_amd.hparams import Recursive_Parse
    return Recursive_Parse({"Mode": "PE"} if block is None else {"Mode": "PE", "Projection": block})


def test_projection_settings_defaults_and_validation():
    from glow_tts_amd.projection import projection_settings
    assert projection_settings(_hp(None)) == {"Perplexity": 30.0, "Iterations": 1000, "Exaggeration_Iterations": 250, "Learning_Rate": 200.0}
    s = projection_settings(_hp({"Perplexity": 12, "Iterations": 300}))
    assert s["Perplexity"] == 12 and s["Iterations"] == 300 and s["Exaggeration_Iterations"] == 250
    for block, key in [({"Perplexity": 0.5}, "Perplexity"), ({"Perplexity": "x"}, "Perplexity"), ({"Iterations": 0}, "Iterations"), ({"Iterations": 2.5}, "Iterations"),
                       ({"Exaggeration_Iterations": -1}, "Exaggeration_Iterations"), ({"Learning_Rate": 0}, "Learning_Rate"), ({"Perplexty": 3}, "Perplexty")]:
        with pytest.raises(ValueError, match=key):
            projection_settings(_hp(block))


def test_prosody_check_settings():
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.visualizer import prosody_check_settings
    assert prosody_check_settings(Recursive_Parse({"Train": {"Prosody_Check_Interval": 5000}})) is None
    hp = Recursive_Parse({"Train": {"Prosody_Check": {"Speakers": 3}}})
    assert prosody_check_settings(hp) == {"Speakers": 3, "Samples_per_Speaker": 100}
    for block, key in [({"Speakers": 0}, "Speakers"), ({"Samples_per_Speaker": "many"}, "Samples_per_Speaker"), ({"Speaker": 3}, "Speaker")]:
        with pytest.raises(ValueError, match=key):
            prosody_check_settings(Recursive_Parse({"Train": {"Prosody_Check": block}}))


def test_argument_parser():
    from glow_tts_amd.visualizer import build_parser
    ap = build_parser()
    a = ap.parse_args(["-c", "ck.pt", "--patterns", "eval", "-o", "out"])
    assert (a.checkpoint, a.patterns, a.what, a.speakers, a.per_speaker, a.seed, a.out, a.no_plot) == ("ck.pt", "eval", None, 50, 100, 0, "out", False)
    a = ap.parse_args(["--vectors", "v.npy", "--labels", "l.tsv", "-o", "out", "--no-plot", "--seed", "3"])
    assert (a.vectors, a.labels, a.no_plot, a.seed, a.patterns) == ("v.npy", "l.tsv", True, 3, None)
    a = ap.parse_args(["-c", "ck.pt", "--patterns", "train", "--what", "speaker", "--speakers", "4", "--per-speaker", "7", "-o", "o"])
    assert (a.what, a.speakers, a.per_speaker, a.patterns) == ("speaker", 4, 7, "train")
    for bad in (["-c", "ck.pt", "--patterns", "dev", "-o", "o"], ["-c", "ck.pt", "--patterns", "eval", "--what", "pitch", "-o", "o"], ["--patterns", "eval"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_select_patterns_repeats_and_respects_the_bounds():
    from glow_tts_amd.visualizer import select_patterns
    by_speaker = {s: ["{}/{:02d}.pickle".format(s, i) for i in range(9, -1, -1)] for s in ("c", "a", "b", "d")}
    one, two = select_patterns(by_speaker, 3, 4, 5), select_patterns(dict(reversed(list(by_speaker.items()))), 3, 4, 5)
    assert one == two and len(one) == 12 and len({f.split("/")[0] for f in one}) == 3 and len(set(one)) == 12
    assert select_patterns(by_speaker, 3, 4, 6) != one
    assert sorted(select_patterns(by_speaker, 50, 100, 0)) == sorted(f for v in by_speaker.values() for f in v)
