// The Gaussian noise of seeded sampling (glowtts_prior_sample, sample_ops.hip): a pure counter hash of (utterance seed words, mel channel, frame).
// FROZEN: a seeded mel changes if anything below changes.  tests/prior_sample_ref.py restates it (integers bit for bit, the Gaussian in float64),
// tests/test_prior_sample_cpu.py pins golden values, DESIGN.md ("Seeded sampling") states it in words.
//
//   keys      k0 = fmix(s0 ^ 0x243F6A88), k1 = fmix(s1 + k0), k0 = fmix(k0 ^ k1), k2 = fmix(k1 + 0x9E3779B9)      (fmix: the murmur3 finalizer, device_common.h)
//             - both seed words reach every key through full avalanche rounds, asymmetrically: (a, b) / (b, a), s / s + 1 and s / s + K
//             (K the counter's multiplier) give unrelated keys, so no pair of seeds yields equal or shifted streams (the pitfall of `id * K + seed`)
//   counter   two consecutive frames share one Box-Muller pair:  p = (t >> 1) * C + c   (uint32 arithmetic);  m = (p ^ k0) * 0x9E3779B1
//   draws     h1 = fmix(m + k1),  h2 = fmix(h1 + (m ^ k2))
//   uniforms  u1 = ((h1 >> 8) + 1) * 2^-24 in (0, 1],  u2 = (h2 >> 8) * 2^-24 in [0, 1)      (24 bits: exact in fp32)
//   normals   r = sqrtf(-2 logf(u1));  frame t even: r * cospif(2 u2),  t odd: r * sinpif(2 u2)     (|value| <= sqrt(48 ln 2) = 5.77)
// Nothing else is read: not the batch size, the padded lengths, the utterance's place in the batch or the launch geometry.
// Accurate logf / sqrtf / sincospif only (the build has no fast-math flag); 2 u2 is exactly representable, so the angle needs no reduction of a rounded product.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"

namespace gauss_hash {

struct Keys { uint32_t k0, k1, k2; };

__host__ __device__ __forceinline__ Keys keys(uint32_t s0, uint32_t s1)
{
    Keys k;
    k.k0 = fmix(s0 ^ 0x243F6A88u);
    k.k1 = fmix(s1 + k.k0);
    k.k0 = fmix(k.k0 ^ k.k1);
    k.k2 = fmix(k.k1 + 0x9E3779B9u);
    return k;
}

// the two 32-bit draws of pair p = (t >> 1) * C + c
__host__ __device__ __forceinline__ void draws(const Keys& k, uint32_t p, uint32_t& h1, uint32_t& h2)
{
    const uint32_t m = (p ^ k.k0) * 0x9E3779B1u;
    h1 = fmix(m + k.k1);
    h2 = fmix(h1 + (m ^ k.k2));
}

// both normals of pair p: g_even for frame 2 (t >> 1), g_odd for frame 2 (t >> 1) + 1
__device__ __forceinline__ void gauss_pair(const Keys& k, uint32_t p, float& g_even, float& g_odd)
{
    uint32_t h1, h2;
    draws(k, p, h1, h2);
    const float u1 = (float)((h1 >> 8) + 1u) * (1.0f / 16777216.0f);
    const float a = (float)(h2 >> 8) * (2.0f / 16777216.0f);            // 2 u2 in [0, 2): the angle in units of pi
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(a, &sn, &cs);
    g_even = r * cs;
    g_odd = r * sn;
}

// gauss(s0, s1, c, t, C) of the contract, for callers that want one element
__device__ __forceinline__ float gauss(uint32_t s0, uint32_t s1, uint32_t c, uint32_t t, uint32_t C)
{
    float ge, go;
    gauss_pair(keys(s0, s1), (t >> 1) * C + c, ge, go);
    return (t & 1u) ? go : ge;
}

}  // namespace gauss_hash
