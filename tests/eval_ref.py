"""Numpy restatement of glow_tts_amd/evaluation.py's arithmetic, for the evaluation suites: the cepstrum, DTW with the same tie-break, MCD and the F0
metrics in float64 (`dtype=np.float64`, the reference) and in float32 (`dtype=np.float32`: every operation rounded to float32 - its distance from the
float64 result is the error bar the device is held to, times four).  Nothing here imports the package."""
import itertools
import math

import numpy as np

MCD_FACTOR = 10.0 * math.sqrt(2.0) / math.log(10.0)


def dct_basis(mel_dim, K):
    k = np.arange(1, K + 1, dtype=np.float64)[:, None]
    m = np.arange(mel_dim, dtype=np.float64)[None, :]
    return math.sqrt(2.0 / mel_dim) * np.cos(np.pi * k * (m + 0.5) / mel_dim)


def log_amplitude(mel, max_abs=4.0, dtype=np.float64):
    """The contract: L = ln(amplitude) = (ln 10 / 20) ((m + A) 100 / (2A) - 100).  float32: the folded form s (m - A), s = ln 10 * 2.5 / A rounded once."""
    mel = np.asarray(mel)
    if dtype == np.float64:
        m = mel.astype(np.float64)
        return (math.log(10.0) / 20.0) * ((m + max_abs) * 100.0 / (2.0 * max_abs) - 100.0)
    return np.float32(math.log(10.0) * 2.5 / max_abs) * (mel.astype(np.float32) - np.float32(max_abs))


def cepstrum(mel, K=13, max_abs=4.0, dtype=np.float64):
    """mel [T, Mel] -> [T, K].  float32: basis rounded once, the sum over m ascending in float32 (products rounded, then added)."""
    L = log_amplitude(mel, max_abs, dtype)
    basis = dct_basis(L.shape[1], K).astype(dtype)
    if dtype == np.float64:
        return L @ basis.T
    acc = np.zeros((L.shape[0], K), np.float32)
    for m in range(L.shape[1]):
        acc = (acc + (L[:, m:m + 1] * basis[None, :, m]).astype(np.float32)).astype(np.float32)
    return acc


def local_cost(x, y, dtype=np.float64):
    """[Tx, K], [Ty, K] -> [Tx, Ty]: sqrt(sum_k (x_ik - y_jk)^2), k ascending."""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    acc = np.zeros((x.shape[0], y.shape[0]), dtype)
    for k in range(x.shape[1]):
        df = (x[:, None, k] - y[None, :, k]).astype(dtype)
        acc = (acc + (df * df).astype(dtype)).astype(dtype)
    return np.sqrt(acc).astype(dtype)


def dtw(x, y, dtype=np.float64):
    """-> (cost, ix, iy, moves): the recurrence over anti-diagonals, the predecessor being the diagonal if <= both others, else (i-1, j) if <= (i, j-1),
    else (i, j-1); moves = the numbers of diagonal, (i-1, j) and (i, j-1) steps."""
    d = local_cost(x, y, dtype)
    Tx, Ty = d.shape
    D = np.full((Tx + 1, Ty + 1), np.inf, dtype)
    bp = np.zeros((Tx, Ty), np.int8)
    for s in range(Tx + Ty - 1):
        i = np.arange(max(0, s - (Ty - 1)), min(Tx - 1, s) + 1)
        j = s - i
        dg, up, lf = D[i, j], D[i, j + 1], D[i + 1, j]                          # D is shifted by one: D[i + 1, j + 1] = D(i, j)
        if s == 0:
            D[1, 1] = d[0, 0]
            continue
        code = np.where((dg <= up) & (dg <= lf), 0, np.where(up <= lf, 1, 2))
        best = np.where(code == 0, dg, np.where(code == 1, up, lf))
        D[i + 1, j + 1] = (d[i, j] + best).astype(dtype)
        bp[i, j] = code
    i, j, ix, iy, moves = Tx - 1, Ty - 1, [], [], [0, 0, 0]
    while True:
        ix.append(i); iy.append(j)
        if i == 0 and j == 0:
            break
        c = int(bp[i, j])
        moves[c] += 1
        i, j = i - (c != 2), j - (c != 1)
    return D[Tx, Ty], np.array(ix[::-1], np.int32), np.array(iy[::-1], np.int32), moves


def path_cost(x, y, ix, iy):
    """The cost of a given path, in float64."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.sqrt(((x[ix] - y[iy]) ** 2).sum(1)).sum())


def brute_force_dtw(x, y):
    """Every monotone path from (0, 0) to (Tx-1, Ty-1) enumerated (float64) -> (minimal cost, the set of minimal paths as tuples of (i, j))."""
    d = local_cost(x, y)
    Tx, Ty = d.shape
    best, paths = np.inf, []

    def walk(i, j, cost, path):
        nonlocal best, paths
        cost += d[i, j]
        path = path + ((i, j),)
        if i == Tx - 1 and j == Ty - 1:
            if cost < best:
                best, paths = cost, [path]
            elif cost == best:
                paths.append(path)
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < Tx and j + dj < Ty:
                walk(i + di, j + dj, cost, path)
    walk(0, 0, 0.0, ())
    return best, paths


def tie_break_path(paths):
    """Of several minimal paths the one the backtrack's tie-break takes: walking back from the end, prefer the diagonal, then (i-1, j), then (i, j-1) - among
    the predecessors that still lie on SOME minimal path (with exact arithmetic every such predecessor has the same cumulative cost)."""
    alive = [p[::-1] for p in paths]
    for s in itertools.count(1):
        if all(len(p) <= s for p in alive):
            return alive[0][::-1]
        i, j = alive[0][s - 1]
        for cand in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
            keep = [p for p in alive if len(p) > s and p[s] == cand]
            if keep:
                alive = keep
                break


def mcd_dtw(ref_mel, cand_mel, K=13, max_abs=4.0, dtype=np.float64):
    """mels [T, Mel] -> (mcd in dB, steps, ix, iy)"""
    cost, ix, iy, _ = dtw(cepstrum(ref_mel, K, max_abs, dtype), cepstrum(cand_mel, K, max_abs, dtype), dtype)
    return MCD_FACTOR * float(cost) / len(ix), len(ix), ix, iy


def f0_metrics(ix, iy, f0_ref, f0_cand):
    """-> (rmse in cents or None, share of steps whose voicing differs, both-voiced steps)"""
    fr, fc = np.asarray(f0_ref, np.float64)[ix], np.asarray(f0_cand, np.float64)[iy]
    both = (fr > 0) & (fc > 0)
    n = int(both.sum())
    rmse = float(np.sqrt(np.mean((1200.0 * np.log2(fc[both] / fr[both])) ** 2))) if n else None
    return rmse, float(((fr > 0) != (fc > 0)).mean()), n
