"""numpy restatement of glowtts_prior_sample_aligned (glow_tts_amd/csrc/sample_ops.hip; the contract is in include/glowtts_hip.h and DESIGN.md
"Teacher-forced alignment"): the sample of the prior along a GIVEN per-frame token index, the index's run lengths and the alignment score.  The noise is
tests/prior_sample_ref.py's restatement of the counter hash, the durations are a bincount, the score is the formula.  `dtype` float64 is the reference,
float32 the same arithmetic at the kernel's input precision (the accuracy bar of tests/test_gpu_teacher_forced.py is 4 x its error).  Shared by
tests/test_teacher_forced_cpu.py and tests/test_gpu_teacher_forced.py."""
import numpy as np

import prior_sample_ref as PS

LOG_2PI = np.log(2.0 * np.pi)


def clean_index(idx, Tx):
    """anything outside [0, Tx) is -1"""
    idx = np.asarray(idx).astype(np.int64)
    return np.where((idx >= 0) & (idx < Tx), idx, -1)


def durations(idx, Tx):
    """[B, Tmax] -> int32 [B, Tx]: the number of frames of every token"""
    idx = clean_index(idx, Tx)
    return np.stack([np.bincount(row[row >= 0], minlength=Tx) for row in idx]).astype(np.int32)


def sample(mean, log_std, idx, seeds, scales, dtype=np.float64):
    """-> z [B, C, Tmax]: mean[idx] + exp(log_std[idx]) * gauss * scale where idx >= 0, 0 elsewhere"""
    B, C, Tx = mean.shape
    idx = clean_index(idx, Tx)
    Tmax = idx.shape[1]
    z = np.zeros((B, C, Tmax), dtype)
    for b in range(B):
        ok = idx[b] >= 0
        src = idx[b][ok]
        g = PS.noise(int(seeds[b][0]), int(seeds[b][1]), C, Tmax)[:, ok].astype(dtype)
        z[b][:, ok] = mean[b].astype(dtype)[:, src] + np.exp(log_std[b].astype(dtype)[:, src]) * g * dtype(scales[b])
    return z


def score(mean, log_std, idx, z_rec, dtype=np.float64):
    """-> [B]: the mean over the valid (c, y) of -0.5 log(2 pi) - ls - 0.5 (z_rec - m)^2 exp(-2 ls), m / ls gathered by idx; 0 without a valid frame"""
    B, C, Tx = mean.shape
    idx = clean_index(idx, Tx)
    out = np.zeros(B, dtype)
    for b in range(B):
        ok = idx[b] >= 0
        if not ok.any():
            continue
        src = idx[b][ok]
        m, ls, z = mean[b].astype(dtype)[:, src], log_std[b].astype(dtype)[:, src], z_rec[b].astype(dtype)[:, ok]
        d = z - m
        terms = dtype(-0.5 * LOG_2PI) - ls - dtype(0.5) * d * d * np.exp(dtype(-2.0) * ls)
        out[b] = terms.sum(dtype=dtype) / dtype(terms.size)
    return out


def aligned(mean, log_std, idx, z_rec, seeds, scales, dtype=np.float64):
    """-> (z, dur, score) as the kernel writes them"""
    Tx = mean.shape[2]
    return sample(mean, log_std, idx, seeds, scales, dtype), durations(idx, Tx), score(mean, log_std, idx, z_rec, dtype)
