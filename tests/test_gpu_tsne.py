"""GPU: the embedding-map kernels (csrc/tsne_ops.hip) and `projection.tsne` against the float64 restatement of the contract (tests/tsne_ref.py).  Bars are
4 x the float32 restatement's own error against float64 on the same inputs unless a test says otherwise; every test prints observed / bar.
Figures of the MI355X run that accompanied the change are recorded in DESIGN.md "Embedding maps"."""
import numpy as np
import pytest
import torch

import tsne_ref as R
from helpers import launch_counts, launch_reset
from test_tsne_cpu import link_errors, step_links

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def report(what, err, bar):
    print(f"{what}: error {err:.3e}, bar {bar:.3e}, ratio {err / bar if bar > 0 else float(err > 0):.3f}")
    assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("N,D", [(8, 1), (65, 3), (130, 257), (200, 1024)])
def test_sqdist(N, D):
    from glow_tts_amd import projection
    x = np.random.default_rng(N).normal(size=(N, D)).astype(np.float32)
    x[5] = x[2]
    got = projection.sqdist(dev(x)).cpu().numpy().astype(np.float64)
    want = R.sqdist(x)
    report(f"sqdist ({N}, {D})", np.abs(got - want).max(), 4.0 * np.abs(R.sqdist(x, np.float32) - want).max())
    assert got[5, 2] == 0.0 and got[2, 5] == 0.0 and (np.diag(got) == 0).all()
    assert np.array_equal(got, got.T)


@pytest.mark.parametrize("N,perplexity", [(8, 2.0), (65, 5.0), (65, 21.0), (130, 5.0), (130, 30.0)])
def test_affinities(N, perplexity):
    """Two identical points and a far outlier in every set (tests/tsne_ref.affinity_case): both branches of the search.  (At N = 65 perplexity 30 is beyond
    (N - 1) / 3: 21 is the largest whole one supported.)"""
    from glow_tts_amd import projection
    x = R.affinity_case(N)
    d2 = R.sqdist(x)
    p64, _ = R.conditional(d2, perplexity)
    p32, _ = R.conditional(R.sqdist(x, np.float32), perplexity, np.float32)
    rows = projection.Fit(dev(x), perplexity, joint=False).matrix().cpu().numpy()
    assert (np.diag(rows) == 0).all()
    report(f"row entropy ({N}, {perplexity:.3g})", np.abs(R.row_entropy(rows) - np.log(perplexity)).max(),
           4.0 * np.abs(R.row_entropy(p32) - np.log(perplexity)).max())
    report(f"conditional ({N}, {perplexity:.3g})", np.abs(rows - p64).max(), 4.0 * np.abs(p32 - p64).max())
    P = projection.Fit(dev(x), perplexity).matrix().cpu().numpy()
    want = R.joint(p64)
    report(f"P ({N}, {perplexity:.3g})", np.abs(P - want).max(), 4.0 * np.abs(R.joint(p32, np.float32) - want).max())
    assert np.array_equal(P, P.T) and (np.diag(P) == 0).all()
    assert P[~np.eye(N, dtype=bool)].min() >= np.float32(1e-12)


def _forces_case(N, scale):
    rng = np.random.default_rng(N)
    x = rng.normal(size=(N, 6)).astype(np.float32)
    P = R.affinities(x, min(30.0, (N - 1) / 3.0)).astype(np.float32)
    y = (rng.normal(size=(N, 2)) * scale).astype(np.float32)
    return P, y


@pytest.mark.parametrize("scale", [1e-4, 30.0])
@pytest.mark.parametrize("N", [8, 65, 130, 1000])
def test_forces(N, scale):
    """One evaluation: P (the float32 matrix, the same bits on both sides) and y -> attractive and repulsive sums, Z and KL; and the gradient
    4 (a attractive - repulsive / Z) put together from the device's sums in float32 for a = 12 and a = 1."""
    from glow_tts_amd import _lib, projection
    P, y = _forces_case(N, scale)
    ld = projection.pitch(N)
    Pd = torch.zeros(N, ld, device=DEV)
    Pd[:, :N] = dev(P)
    sums, shares = torch.empty(N, 4, device=DEV), torch.empty(N, 4, dtype=torch.float64, device=DEV)
    yd = dev(y)
    want, f32 = R.forces(P, y), R.forces(P, y, np.float32)
    for kl in (1, 0):
        sums.fill_(float("nan")); shares.fill_(float("nan"))
        _lib.api().glowtts_tsne_forces(_lib.ptr(Pd), _lib.ptr(yd), _lib.ptr(sums), _lib.ptr(shares), N, kl, _lib.stream())
        s, sh = sums.cpu().numpy(), shares.cpu().numpy()
        tag = f"({N}, {scale:g}, kl {kl})"
        report("attractive " + tag, np.abs(s[:, :2] - want[0]).max(), 4.0 * np.abs(f32[0] - want[0]).max())
        report("repulsive " + tag, np.abs(s[:, 2:] - want[1]).max(), 4.0 * np.abs(f32[1] - want[1]).max())
        Z = sh[:, 0].sum()
        if kl:                                                                     # the launch whose figures are reported: Z and KL at the bar
            report("Z " + tag, abs(Z - want[2]), 4.0 * abs(float(f32[2]) - want[2]))
            got_kl = sh[:, 1].sum() + np.log(Z) * sh[:, 2].sum()
            report("KL " + tag, abs(got_kl - want[3]), 4.0 * abs(float(f32[3]) - want[3]))
        else:
            # the hot launch adds the f32 w exactly: d = dx^2 + dy^2 is within 2 ulp (the differences, the squares, the sum), 1 + d and the division add half an ulp
            # each, and d / (1 + d) <= 1 - every w, hence Z, lies within 3 * 2^-24 of its float64 value, relatively.  (At N = 8, scale 30 it is 0.43 * 2^-24 Z out and
            # the float32 restatement, by cancellation in its own sum, 0.04: a bar of 4 x that one number would not be a bar.)
            report("Z of the hot launch " + tag, abs(Z - want[2]), 3.0 * 2.0 ** -24 * want[2])
            assert (sh[:, 1:] == 0).all()
        for a in (12.0, 1.0):
            g = np.float32(4) * (np.float32(a) * s[:, :2] - s[:, 2:] / np.float32(Z))
            g64 = R.gradient(P, y, a)
            report(f"gradient a = {a:g} " + tag, np.abs(g - g64).max(), 4.0 * np.abs(R.gradient(P, y, a, np.float32) - g64).max())


def test_step_link_by_link():
    """12 single iterations, 6 of them exaggerated, each from the device's own state and replayed in float64 (tests/test_tsne_cpu.step_links)."""
    from glow_tts_amd import projection
    x, _, perplexity = R.step_case()
    fit = projection.Fit(dev(x), perplexity)

    def state_of(t, y, u, gain):
        fit.y, fit.u, fit.gain = dev(y), dev(u), dev(gain)
        fit.iterate(t, t + 1, 6, 200.0)
        return fit.y.cpu().numpy(), fit.u.cpu().numpy(), fit.gain.cpu().numpy()

    # the affinities under the steps are the device's own; the replay uses float64 ones: their difference is part of the error held to the bar
    for t, (got, want64, want32) in enumerate(step_links(np.float32, state_of)):
        ey, by, eu, bu, left_out, same = link_errors(got, want64, want32)
        print(f"iteration {t}: gain elements left out {left_out:.3f}")
        report(f"y after iteration {t}", ey, by)
        report(f"u after iteration {t}", eu, bu)
        assert left_out <= 0.01 and same, (t, left_out, same)
        assert abs(got[0].mean(0)).max() <= 1e-6 * abs(got[0]).max()


@pytest.fixture(scope="module")
def separation_bar():
    """3 x the largest |ratio - 1| of the float32 restatement's final KL against float64's over the three seeds"""
    return 3.0 * max(abs(R.separation_fit(s, np.float32)[1][-1] / R.separation_fit(s, np.float64)[1][-1] - 1) for s in (0, 1, 2))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_whole_run_separates_the_clusters(seed, separation_bar):
    from glow_tts_amd import projection
    x, labels, y0 = R.separation_case(seed)
    _, kl64, at = R.separation_fit(seed, np.float64)
    _, kl32, _ = R.separation_fit(seed, np.float32)
    s = R.SEPARATION
    res = projection.tsne(dev(x), s["perplexity"], s["iterations"], s["exaggeration_iterations"], s["learning_rate"], y0=y0.astype(np.float32))
    assert res.kl_iterations == at and len(res.kl) == len(at) and np.isfinite(res.kl).all()
    assert projection.nearest_neighbour_agreement(res.y, labels.tolist()) == 1.0
    assert R.nearest_neighbour_agreement(res.y.cpu().numpy(), labels) == 1.0
    report(f"KL at iteration 0, seed {seed}", abs(res.kl[0] - kl64[0]), 4.0 * abs(kl32[0] - kl64[0]))
    report(f"final KL / float64 - 1, seed {seed}", abs(res.kl[-1] / kl64[-1] - 1), separation_bar)
    y = res.y.cpu().numpy()
    assert np.isfinite(y).all() and abs(y.mean(0)).max() <= 1e-5 * abs(y).max()


def test_two_runs_are_bit_identical():
    from glow_tts_amd import projection
    x = dev(np.random.default_rng(3).normal(size=(333, 7)))
    a = projection.tsne(x, 20.0, 60, 30, 200.0, seed=4)
    b = projection.tsne(x, 20.0, 60, 30, 200.0, seed=4)
    assert torch.equal(a.y, b.y) and a.kl == b.kl and a.kl_iterations == [0, 50, 60]
    c = projection.tsne(x, 20.0, 60, 30, 200.0, seed=5)
    assert not torch.equal(a.y, c.y)


def test_launch_anatomy():
    """3 + 2 T + 2 launches: the affinities' three, `tsne_forces` (`tsne_forces,kl` on iteration 0 and for the final y) and `tsne_step` per iteration, and
    the `tsne_step,finish` of the final KL."""
    from glow_tts_amd import projection
    x = dev(np.random.default_rng(5).normal(size=(100, 4)))
    torch.cuda.synchronize()
    launch_reset()
    projection.tsne(x, 10.0, 20, 10, 200.0)
    counts = {k: v for k, v in launch_counts().items() if v}
    assert counts == {"tsne_sqdist": 1, "tsne_affinity": 1, "tsne_symmetrize": 1, "tsne_forces": 19, "tsne_forces,kl": 2, "tsne_step": 20, "tsne_step,finish": 1}, counts
    assert sum(counts.values()) == 3 + 2 * 20 + 2


def test_largest_size_runs():
    """N = 8192 (y fills the 64 KiB of LDS, the affinity row 32 KiB): P sums to 1 and two iterations leave a finite, centred map."""
    from glow_tts_amd import abi, projection
    N = abi.TSNE_MAX_N
    x = dev(np.random.default_rng(6).normal(size=(N, 2)))
    fit = projection.Fit(x, 30.0)
    P = fit.matrix()
    assert abs(float(P.double().sum()) - 1.0) < 1e-4 and torch.equal(P, P.t()) and float(P.diagonal().abs().max()) == 0.0
    fit.start(projection.initial_map(N, 0))
    kl = fit.iterate(0, 2, 1, 200.0, 50, True).cpu().numpy()
    assert np.isfinite(kl).all() and kl[0] > 0
    assert torch.isfinite(fit.y).all() and float(fit.y.mean(0).abs().max()) < 1e-6


def test_refusals():
    from glow_tts_amd import _lib, abi, projection
    L = _lib.lib()
    x = torch.zeros(8193, 2, device=DEV)
    work = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    for n, d, perplexity, key in [(7, 2, 2.0, "N"), (8193, 2, 30.0, "N"), (30, 1025, 5.0, "D"), (30, 4, 10.0, "perplexity")]:
        with pytest.raises(ValueError, match=key):
            projection.tsne(torch.zeros(n, d, device=DEV), perplexity, 10, 5)
        assert L.glowtts_tsne_affinities(_lib.ptr(x), _lib.ptr(work), n, d, perplexity, 1, _lib.stream()) == abi.E_ARG
    assert L.glowtts_tsne_supported(8, 1) == 1 and L.glowtts_tsne_supported(8192, 1024) == 1
    assert L.glowtts_tsne_supported(7, 1) == 0 and L.glowtts_tsne_supported(8193, 1) == 0 and L.glowtts_tsne_supported(8, 1025) == 0
    assert L.glowtts_tsne_work_bytes(7) == 0 and L.glowtts_tsne_work_bytes(8193) == 0 and L.glowtts_tsne_work_bytes(10) == 10 * 12 * 4 + 10 * 48
    with pytest.raises(ValueError, match="y0"):
        projection.tsne(torch.zeros(30, 4, device=DEV), 5.0, 10, 5, y0=np.zeros((29, 2), np.float32))
    with pytest.raises(_lib.GlowTTSHipError):
        projection.tsne(torch.zeros(30, 4), 5.0, 10, 5)
