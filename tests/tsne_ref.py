"""The contract of the embedding maps (DESIGN.md "Embedding maps"; csrc/tsne_ops.hip, glow_tts_amd/projection.py) restated in numpy: exact t-SNE into two
dimensions.  `dtype` is a parameter of every function: float64 is the reference, float32 - the same statements at the kernels' precision - gives the error bars."""
import numpy as np

EXAGGERATION, MOMENTUM_EARLY, MOMENTUM_LATE, P_FLOOR, BISECTION_STEPS = 12.0, 0.5, 0.8, 1e-12, 64


def sqdist(x, dtype=np.float64):
    """d2[i][j] = sum_k (x_ik - x_jk)^2 by direct differences, k ascending"""
    x = np.asarray(x, dtype)
    d2 = np.zeros((x.shape[0], x.shape[0]), dtype)
    for k in range(x.shape[1]):
        df = x[:, None, k] - x[None, :, k]
        d2 += df * df
    return d2


def conditional(d2, perplexity, dtype=np.float64):
    """p_{j|i} [N][N] (0 on the diagonal) of the 64-step bisection of beta, all rows at once; also the betas last evaluated."""
    d2 = np.asarray(d2, dtype)
    N = d2.shape[0]
    off = ~np.eye(N, dtype=bool)
    d = d2 - np.where(off, d2, np.inf).min(1, keepdims=True).astype(dtype)
    d = np.where(off, d, dtype(0))
    target = dtype(np.log(dtype(perplexity)))
    beta, lo, hi = np.ones((N, 1), dtype), np.zeros((N, 1), dtype), np.full((N, 1), np.inf, dtype)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for _ in range(BISECTION_STEPS):
            e = np.where(off, np.exp(-beta * d), dtype(0)).astype(dtype)
            s = e.sum(1, keepdims=True, dtype=dtype)
            H = np.log(s) + beta * (d * e).sum(1, keepdims=True, dtype=dtype) / s
            beta_e, p = beta, e / s
            up = H > target
            new_up = np.where(np.isinf(hi), beta * dtype(2), (beta + np.where(np.isinf(hi), dtype(0), hi)) / dtype(2))
            lo, hi = np.where(up, beta, lo), np.where(up, hi, beta)
            beta = np.where(up, new_up, (beta + lo) / dtype(2)).astype(dtype)
    return p.astype(dtype), beta_e


def joint(p, dtype=np.float64):
    """P_ij = max((p_{j|i} + p_{i|j}) / (2N), 1e-12) off the diagonal, 0 on it"""
    p = np.asarray(p, dtype)
    N = p.shape[0]
    P = np.maximum((p + p.T) / dtype(2 * N), dtype(P_FLOOR)).astype(dtype)
    np.fill_diagonal(P, 0)
    return P


def affinities(x, perplexity, dtype=np.float64):
    return joint(conditional(sqdist(x, dtype), perplexity, dtype)[0], dtype)


def row_entropy(p):
    """Shannon entropy (nats) of each row of conditional affinities, in float64 whatever the rows' dtype"""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(p > 0, p * np.log(p), 0.0).sum(1)


def forces(P, y, dtype=np.float64):
    """-> attractive [N][2] = sum_j P_ij w_ij (y_i - y_j), repulsive [N][2] = sum_j w_ij^2 (y_i - y_j), Z = sum_{i != j} w_ij,
    KL = sum_ij P_ij (ln P_ij - ln w_ij) + ln Z sum_ij P_ij  (= sum P ln(P Z / w))"""
    P, y = np.asarray(P, dtype), np.asarray(y, dtype)
    N = y.shape[0]
    diff = y[:, None, :] - y[None, :, :]
    w = dtype(1) / (dtype(1) + (diff * diff).sum(2, dtype=dtype))
    np.fill_diagonal(w, 0)
    attractive = ((P * w)[:, :, None] * diff).sum(1, dtype=dtype)
    repulsive = ((w * w)[:, :, None] * diff).sum(1, dtype=dtype)
    Z = w.sum(dtype=dtype)
    off = ~np.eye(N, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(off & (P > 0), P * (np.log(P) - np.log(w)), dtype(0)).astype(dtype)
    kl = term.sum(dtype=dtype) + np.log(Z) * P.sum(dtype=dtype)
    return attractive.astype(dtype), repulsive.astype(dtype), dtype(Z), dtype(kl)


def gradient(P, y, exaggeration, dtype=np.float64):
    a, r, Z, _ = forces(P, y, dtype)
    return (dtype(4) * (dtype(exaggeration) * a - r / Z)).astype(dtype)


def kl_divergence(P, y, dtype=np.float64):
    return forces(P, y, dtype)[3]


def step(P, y, u, gain, t, exaggeration_iterations=250, learning_rate=200.0, dtype=np.float64):
    """iteration t on copies of the state -> y, u, gain, g"""
    y, u, gain = np.array(y, dtype), np.array(u, dtype), np.array(gain, dtype)
    early = t < exaggeration_iterations
    g = gradient(P, y, EXAGGERATION if early else 1.0, dtype)
    mu = dtype(MOMENTUM_EARLY if early else MOMENTUM_LATE)
    gain = np.maximum(np.where(np.sign(g) != np.sign(u), gain + dtype(0.2), gain * dtype(0.8)), dtype(0.01)).astype(dtype)
    u = (mu * u - dtype(learning_rate) * gain * g).astype(dtype)
    y = (y + u).astype(dtype)
    y = (y - y.mean(0, dtype=dtype)).astype(dtype)
    return y, u, gain, g


def fit(x, y0, perplexity=30.0, iterations=1000, exaggeration_iterations=250, learning_rate=200.0, kl_every=50, dtype=np.float64):
    """-> y, the KL series, its iterations (0, every `kl_every`-th, and `iterations` for the final y)"""
    P = affinities(x, perplexity, dtype)
    y, u, gain = np.array(y0, dtype), np.zeros_like(y0, dtype), np.ones_like(y0, dtype)
    kl, at = [], []
    for t in range(iterations):
        if t % kl_every == 0:
            kl.append(float(kl_divergence(P, y, dtype))); at.append(t)
        y, u, gain, _ = step(P, y, u, gain, t, exaggeration_iterations, learning_rate, dtype)
    kl.append(float(kl_divergence(P, y, dtype))); at.append(iterations)
    return y, kl, at


def nearest_neighbour_agreement(points, labels):
    """share of points whose nearest other point (squared Euclidean, ties to the lowest index) carries the same label"""
    d2 = sqdist(points)
    np.fill_diagonal(d2, np.inf)
    labels = np.asarray(labels)
    return float((labels[d2.argmin(1)] == labels).mean())


def separation_case(seed):
    """The issue's case: 6 centres, 40 points each in 16 dimensions, and the start; drawn in this order."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(6, 16)) * 4
    x = (centres[:, None, :] + rng.normal(size=(6, 40, 16))).reshape(240, 16)
    y0 = rng.normal(size=(240, 2)) * 1e-4
    return x, np.repeat(np.arange(6), 40), y0


SEPARATION = dict(perplexity=15.0, learning_rate=200.0, iterations=500, exaggeration_iterations=250)
_FITS = {}


def separation_fit(seed, dtype):
    """the restated fit of the separation case, computed once per (seed, dtype) and shared"""
    key = (seed, np.dtype(dtype).name)
    if key not in _FITS:
        x, labels, y0 = separation_case(seed)
        _FITS[key] = fit(x, y0, dtype=dtype, **SEPARATION)
    return _FITS[key]


def affinity_case(N, seed=0, D=5):
    """N points with two identical ones and one far outlier"""
    rng = np.random.default_rng(seed + N)
    x = rng.normal(size=(N, D))
    x[3] = x[1]
    x[N - 2] = 50.0 + rng.normal(size=D)
    return x.astype(np.float32)


def step_case():
    """The link-by-link case: 3 clusters of 10 points in 4 dimensions, perplexity 5, a start at scale 1e-2."""
    rng = np.random.default_rng(7)
    x = (rng.normal(size=(3, 1, 4)) * 3 + rng.normal(size=(3, 10, 4))).reshape(30, 4).astype(np.float32)
    y0 = (rng.normal(size=(30, 2)) * 1e-2).astype(np.float32)
    return x, y0, 5.0
