"""numpy restatement of the seeded-sampling noise contract (glow_tts_amd/csrc/gauss_hash.h, DESIGN.md "Seeded sampling"): the integer part bit for
bit (uint32 arithmetic), the Gaussian in float64; and of glowtts_prior_sample's semantics (durations -> per-frame token index -> dense attentions,
expanded prior, sample) in float64.  Shared by tests/test_prior_sample_cpu.py and tests/test_gpu_prior_sample.py."""
import hashlib

import numpy as np

U = np.uint32


def fmix(h):
    """murmur3 finalizer on uint32 arrays"""
    h = np.asarray(h, dtype=U).copy()
    h ^= h >> U(16)
    h *= U(0x85EBCA6B)
    h ^= h >> U(13)
    h *= U(0xC2B2AE35)
    h ^= h >> U(16)
    return h


def keys(s0, s1):
    with np.errstate(over="ignore"):
        k0 = fmix(U(s0 & 0xFFFFFFFF) ^ U(0x243F6A88))
        k1 = fmix(U(s1 & 0xFFFFFFFF) + k0)
        k0 = fmix(k0 ^ k1)
        k2 = fmix(k1 + U(0x9E3779B9))
    return k0, k1, k2


def draws(s0, s1, p):
    """pair counters p (uint32 array) -> (h1, h2)"""
    k0, k1, k2 = keys(s0, s1)
    with np.errstate(over="ignore"):
        m = (np.asarray(p, dtype=U) ^ k0) * U(0x9E3779B1)
        h1 = fmix(m + k1)
        h2 = fmix(h1 + (m ^ k2))
    return h1, h2


def gauss(s0, s1, c, t, C):
    """The contract's pure function on broadcastable integer arrays c (channel), t (frame): float64 normals.  Frames 2j and 2j + 1 share one
    Box-Muller pair (cosine for the even frame, sine for the odd one)."""
    c, t = np.broadcast_arrays(np.asarray(c, dtype=np.int64), np.asarray(t, dtype=np.int64))
    p = (((t >> 1) * int(C) + c) & 0xFFFFFFFF).astype(U)
    h1, h2 = draws(s0, s1, p)
    u1 = ((h1 >> U(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (h2 >> U(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.where(t & 1, r * np.sin(ang), r * np.cos(ang))


def noise(s0, s1, C, T):
    """[C, T] float64: the noise of one utterance"""
    return gauss(s0, s1, np.arange(C)[:, None], np.arange(T)[None, :], C)


def seed_words(seed, label, k=0):
    """The two uint32 seed words of (run seed, utterance label, sample number): the first 8 bytes of blake2b, little endian."""
    d = hashlib.blake2b(f"{seed}\0{label}\0{k}".encode()).digest()
    return int.from_bytes(d[:4], "little"), int.from_bytes(d[4:8], "little")


def prior_sample(mean, log_std, dur, mel_lengths, seeds, scales, Tmax):
    """float64 restatement of glowtts_prior_sample on numpy arrays: mean / log_std [B, C, Tx], dur [B, Tx], mel_lengths [B], seeds [B, 2],
    scales [B] -> (z [B, C, Tmax], idx [B, Tmax] int32, attn [B, Tx, Tmax] float32)."""
    B, C, Tx = mean.shape
    z = np.zeros((B, C, Tmax), np.float64)
    idx = np.full((B, Tmax), -1, np.int32)
    attn = np.zeros((B, Tx, Tmax), np.float32)
    for b in range(B):
        cum = np.cumsum(dur[b].astype(np.int64))
        for y in range(Tmax):
            n = int(np.searchsorted(cum, y, side="right"))
            if y < int(mel_lengths[b]) and n < Tx:
                idx[b, y] = n
                attn[b, n, y] = 1.0
        g = noise(int(seeds[b][0]), int(seeds[b][1]), C, Tmax)
        ok = idx[b] >= 0
        src = idx[b][ok]
        z[b][:, ok] = mean[b].astype(np.float64)[:, src] + np.exp(log_std[b].astype(np.float64)[:, src]) * g[:, ok] * float(scales[b])
    return z, idx, attn
