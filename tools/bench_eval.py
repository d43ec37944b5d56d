"""Objective evaluation (glow_tts_amd/evaluation.py, csrc/eval_ops.hip) on one MI355X: `mcd_dtw` at B = 32 x (800, 800) and B = 1 x (800, 800) frames, 80 mels,
13 coefficients, against two baselines of the same recurrence and tie-break on the same mels:
  * torch: cepstra by a matmul, the local costs by `torch.cdist`, then one batched step of torch operations per anti-diagonal, on the device - cost and
    back-pointers only: the backtrack is left out of its time, which favours it;
  * numpy: the vectorised anti-diagonal DTW of tests/eval_ref.py's kind on the host, batched over the pairs, likewise without the backtrack.
Medians of `--iters` (>= 20) alternating calls after `--warmup`, each a host clock around a call that ends in a synchronise; the host baseline is called
`--host-iters` times.  The three costs are compared so that the paths are seen to do the same work.  The sustained clock is noted as tools/bench_vc.py does.
Usage: python tools/bench_eval.py [--iters 20] [--out profiles/bench_eval.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

FRAMES, MEL, K, MAX_ABS = 800, 80, 13, 4.0


def mels(B, device):
    """[B, MEL, FRAMES] reference mels and candidates: the reference warped in time (a slow sine) plus noise"""
    rng = np.random.default_rng(3)
    ref = np.cumsum(rng.standard_normal((B, FRAMES, MEL)) * 0.2, axis=1).clip(-3.5, 3.5).astype(np.float32)
    t = np.arange(FRAMES)
    warp = np.clip(np.round(t + 25.0 * np.sin(2 * np.pi * t / FRAMES)), 0, FRAMES - 1).astype(np.int64)
    cand = (ref[:, warp] + 0.2 * rng.standard_normal((B, FRAMES, MEL))).clip(-4, 4).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1))).to(device)
    return to(ref), to(cand)


def torch_dtw_cost(ref, cand, basis, scale):
    """The recurrence as batched torch operations, one step per anti-diagonal -> (cost [B], back-pointers [B, Tx + Ty - 1, Tx] uint8)"""
    cx = (scale * (ref.transpose(1, 2) - MAX_ABS)) @ basis.T
    cy = (scale * (cand.transpose(1, 2) - MAX_ABS)) @ basis.T
    d = torch.cdist(cx, cy)                                                                   # [B, Tx, Ty]
    B, Tx, Ty = d.shape
    inf = torch.full((B, Tx + 1), float("inf"), device=d.device)
    p1, p2 = inf.clone(), inf.clone()                                                         # diagonals d - 1, d - 2 at row i + 1 (row 0: the border)
    rows = torch.arange(Tx, device=d.device)
    bp = torch.empty(B, Tx + Ty - 1, Tx, dtype=torch.uint8, device=d.device)
    for s in range(Tx + Ty - 1):
        j = s - rows
        on = (j >= 0) & (j < Ty)
        local = d[:, rows, j.clamp(0, Ty - 1)]
        dg, up, lf = p2[:, :-1], p1[:, :-1], p1[:, 1:]
        code = torch.where((dg <= up) & (dg <= lf), 0, torch.where(up <= lf, 1, 2))
        best = torch.where(code == 0, dg, torch.where(code == 1, up, lf))
        if s == 0:
            best = torch.zeros_like(best)
        cur = torch.where(on, local + best, inf[:, 1:])
        bp[:, s] = code.to(torch.uint8)
        p2, p1 = p1, torch.cat([inf[:, :1], cur], 1)
    return p1[:, Tx], bp


def numpy_dtw_cost(cx, cy):
    """The same on the host, vectorised over the pairs and the anti-diagonal -> cost [B]"""
    d = np.zeros((cx.shape[0], cx.shape[1], cy.shape[1]), np.float32)
    for k in range(cx.shape[2]):
        d += (cx[:, :, None, k] - cy[:, None, :, k]) ** 2
    d = np.sqrt(d)
    B, Tx, Ty = d.shape
    D = np.full((B, Tx + 1, Ty + 1), np.inf, np.float32)
    bp = np.zeros((B, Tx, Ty), np.uint8)
    D[:, 1, 1] = d[:, 0, 0]
    for s in range(1, Tx + Ty - 1):
        i = np.arange(max(0, s - (Ty - 1)), min(Tx - 1, s) + 1)
        j = s - i
        dg, up, lf = D[:, i, j], D[:, i, j + 1], D[:, i + 1, j]
        code = np.where((dg <= up) & (dg <= lf), 0, np.where(up <= lf, 1, 2))
        D[:, i + 1, j + 1] = d[:, i, j] + np.where(code == 0, dg, np.where(code == 1, up, lf))
        bp[:, i, j] = code
    return D[:, Tx, Ty]


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run(B, warmup, iters, host_iters):
    from glow_tts_amd import evaluation
    dev = torch.device("cuda:0")
    ref, cand = mels(B, dev)
    lengths = torch.full((B,), FRAMES, dtype=torch.int64, device=dev)
    basis = torch.from_numpy(evaluation.dct_basis(MEL, K).astype(np.float32)).to(dev)
    scale = float(np.log(10.0) * 2.5 / MAX_ABS)
    hip = lambda: evaluation.mcd_dtw(ref, lengths, cand, lengths, K, MAX_ABS)
    tch = lambda: torch_dtw_cost(ref, cand, basis, scale)
    for _ in range(warmup):
        hip(), tch()
    torch.cuda.synchronize()
    t_hip, t_torch = [], []
    for _ in range(iters):                                                                    # alternating: drift of the clock hits both alike
        t_hip.append(clock(hip)[0])
        t_torch.append(clock(tch)[0])
    res = hip()
    cost_torch = tch()[0]
    cx = evaluation.mel_cepstrum(ref, lengths, K, MAX_ABS).cpu().numpy()
    cy = evaluation.mel_cepstrum(cand, lengths, K, MAX_ABS).cpu().numpy()
    t_host = []
    for _ in range(host_iters):
        t0 = time.perf_counter()
        cost_host = numpy_dtw_cost(cx, cy)
        t_host.append((time.perf_counter() - t0) * 1e3)
    f = lambda ts: {"ms_per_call": round(statistics.median(ts), 4), "ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "calls": len(ts)}
    cost = res.path.cost.cpu().numpy()
    out = {"B": B, "frames": [FRAMES, FRAMES], "mel": MEL, "coefficients": K, "cells": B * FRAMES * FRAMES,
           "hip_mcd_dtw": dict(f(t_hip), launches="2 eval_mel_cepstrum + 1 eval_dtw", includes="cepstra, recurrence, backtrack, path"),
           "torch_anti_diagonals": dict(f(t_torch), includes="cepstra, local costs, recurrence, back-pointers; no backtrack"),
           "numpy_anti_diagonals_host": dict(f(t_host), includes="local costs, recurrence, back-pointers; no cepstra, no backtrack"),
           "mean_mcd_db": float(res.mcd.mean()), "mean_steps": float(res.steps.double().mean()),
           "worst_relative_cost_difference": {"torch": float(np.abs(cost_torch.cpu().numpy() / cost - 1).max()), "numpy": float(np.abs(cost_host / cost - 1).max())}}
    out["speedup_hip_over_torch"] = round(out["torch_anti_diagonals"]["ms_per_call"] / out["hip_mcd_dtw"]["ms_per_call"], 2)
    out["speedup_hip_over_numpy"] = round(out["numpy_anti_diagonals_host"]["ms_per_call"] / out["hip_mcd_dtw"]["ms_per_call"], 2)
    out["cells_per_second_hip"] = float("%.3g" % (out["cells"] / (out["hip_mcd_dtw"]["ms_per_call"] * 1e-3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_eval.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_eval.py measures on the GPU"
    ghz, _ = bench.sustained_mfma_clock()
    results = [run(B, args.warmup, args.iters, args.host_iters) for B in (32, 1)]
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup, "results": results}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
