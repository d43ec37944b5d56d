// Seeded prior sample of GlowTTS.inference (Modules.py:175-191) for gfx950, ONE launch: durations -> per-frame token index (hard alignment) -> dense 0/1
// attentions, expanded prior and the sample  z = mean[idx] + exp(log_std[idx]) * gauss * noise_scale.  The noise is the counter hash of gauss_hash.h: a
// function of (utterance seed words, channel, frame) only, so an utterance's z does not depend on the batch around it, its padding or the mel bucket.
//
// Grid (frame tile of GLOWTTS_SAMPLE_TILE frames, utterance), 256 threads.  A workgroup
//   1. streams its utterance's durations through LDS in chunks of GLOWTTS_SAMPLE_SCAN_CHUNK tokens: block scan (int32) on top of a running carry; wave 0
//      holds one frame per lane and adds, per chunk, the number of tokens whose span ended at or before its frame (all / none of the chunk from its first and
//      last sums, else a binary search in LDS).  The walk stops at the first chunk whose carry lies beyond the tile.  LDS is fixed whatever Tx is; the re-scan
//      per tile reads a few KB that stay in L2.
//   2. writes idx, then z row by row and the attention rows, coalesced along the frames: 16-byte stores when every row is 16-byte aligned (Tmax % 4 == 0),
//      one frame per lane otherwise.  Both forms evaluate `sample_value` on the same operands: the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/glowtts_hip.h"
#include "gauss_hash.h"
#include "launch_log.h"

namespace {

constexpr int TILE = 64;                                  // frames per workgroup
constexpr int CHUNK = GLOWTTS_SAMPLE_SCAN_CHUNK;          // tokens per scan step
constexpr int THREADS = 256;
constexpr int PER_THREAD = CHUNK / THREADS;
static_assert(CHUNK % THREADS == 0 && PER_THREAD >= 1, "the scan gives every thread the same number of consecutive tokens");

// (explicit fma: the vector and the scalar store paths must round alike; noise_scale = 0 returns mean itself)
__device__ __forceinline__ float sample_value(float mean, float log_std, float g, float scale) { return fmaf(expf(log_std), g * scale, mean); }

template <bool VEC>
__global__ __launch_bounds__(THREADS) void prior_sample_kernel(const float* __restrict__ mean, const float* __restrict__ log_std, const float* __restrict__ dur,
                                                               const int64_t* __restrict__ mel_lengths, const uint32_t* __restrict__ seeds,
                                                               const float* __restrict__ noise_scales, float* __restrict__ z, int32_t* __restrict__ idx,
                                                               float* __restrict__ attn, int C, int Tx, int Tmax)
{
    __shared__ int32_t cum_s[CHUNK];
    __shared__ int32_t wave_s[THREADS / 64];
    __shared__ int32_t idx_s[TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, y0 = blockIdx.x * TILE;
    const float* d = dur + (size_t)b * Tx;

    // ---- 1. idx[y] = #{x : cum[x] <= y} for the tile's frames
    const int y = y0 + tid;                                // (meaningful for tid < TILE)
    int count = 0, carry = 0;
    for (int x0 = 0; x0 < Tx; x0 += CHUNK) {
        const int n = min(CHUNK, Tx - x0);
        int v[PER_THREAD], tsum = 0;
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) {
            const int x = tid * PER_THREAD + j;
            tsum += x < n ? (int)d[x0 + x] : 0;
            v[j] = tsum;
        }
        int incl = tsum;                                   // inclusive scan of the threads' sums over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wave_s[wave] = incl;
        __syncthreads();
        int base = carry, total = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) {
            const int s = wave_s[w];
            if (w < wave) base += s;
            total += s;
        }
        base += incl - tsum;
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) cum_s[tid * PER_THREAD + j] = base + v[j];
        __syncthreads();
        if (tid < TILE && y < Tmax) {
            if (cum_s[n - 1] <= y) count += n;
            else if (cum_s[0] <= y) {
                int lo = 0, hi = n - 1;                    // cum_s[lo] <= y < cum_s[hi]: the first element above y
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (cum_s[mid] <= y) lo = mid; else hi = mid;
                }
                count += hi;
            }
        }
        carry += total;
        __syncthreads();                                   // (the next chunk overwrites cum_s / wave_s)
        if (carry > y0 + TILE - 1) break;                  // every later sum lies beyond the tile (uniform over the workgroup)
    }
    if (tid < TILE) {
        const bool ok = y < Tmax && (int64_t)y < mel_lengths[b] && count < Tx;
        const int id = ok ? count : -1;
        idx_s[tid] = id;
        if (y < Tmax) idx[(size_t)b * Tmax + y] = id;
    }
    __syncthreads();

    // ---- 2. z and the attentions
    const gauss_hash::Keys keys = gauss_hash::keys(seeds[2 * b], seeds[2 * b + 1]);
    const float scale = noise_scales[b];
    const float* mb = mean + (size_t)b * C * Tx;
    const float* lb = log_std + (size_t)b * C * Tx;
    if (VEC) {
        const int g = tid & (TILE / 4 - 1), r0 = tid / (TILE / 4);
        constexpr int ROWS = THREADS / (TILE / 4);
        const int yy = y0 + 4 * g;
        if (yy >= Tmax) return;                            // (Tmax % 4 == 0: a group lies wholly inside or outside; no barrier below)
        const int i0 = idx_s[4 * g], i1 = idx_s[4 * g + 1], i2 = idx_s[4 * g + 2], i3 = idx_s[4 * g + 3];
        const bool any01 = (i0 >= 0) | (i1 >= 0), any23 = (i2 >= 0) | (i3 >= 0);
        for (int c = r0; c < C; c += ROWS) {
            const float* m = mb + (size_t)c * Tx;
            const float* l = lb + (size_t)c * Tx;
            float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
            const uint32_t p = (uint32_t)(yy >> 1) * (uint32_t)C + (uint32_t)c;
            if (any01) gauss_hash::gauss_pair(keys, p, g0, g1);
            if (any23) gauss_hash::gauss_pair(keys, p + (uint32_t)C, g2, g3);
            float4 o;
            o.x = i0 >= 0 ? sample_value(m[i0], l[i0], g0, scale) : 0.f;
            o.y = i1 >= 0 ? sample_value(m[i1], l[i1], g1, scale) : 0.f;
            o.z = i2 >= 0 ? sample_value(m[i2], l[i2], g2, scale) : 0.f;
            o.w = i3 >= 0 ? sample_value(m[i3], l[i3], g3, scale) : 0.f;
            *reinterpret_cast<float4*>(z + ((size_t)b * C + c) * Tmax + yy) = o;
        }
        if (attn) {
            for (int x = r0; x < Tx; x += ROWS) {
                float4 o;
                o.x = i0 == x ? 1.f : 0.f; o.y = i1 == x ? 1.f : 0.f; o.z = i2 == x ? 1.f : 0.f; o.w = i3 == x ? 1.f : 0.f;
                *reinterpret_cast<float4*>(attn + ((size_t)b * Tx + x) * Tmax + yy) = o;
            }
        }
    } else {
        const int f = tid & (TILE - 1), r0 = tid / TILE;
        constexpr int ROWS = THREADS / TILE;
        const int yy = y0 + f;
        if (yy >= Tmax) return;
        const int id = idx_s[f];
        for (int c = r0; c < C; c += ROWS) {
            float v = 0.f;
            if (id >= 0) {
                float ge, go;
                gauss_hash::gauss_pair(keys, (uint32_t)(yy >> 1) * (uint32_t)C + (uint32_t)c, ge, go);
                v = sample_value(mb[(size_t)c * Tx + id], lb[(size_t)c * Tx + id], (yy & 1) ? go : ge, scale);
            }
            z[((size_t)b * C + c) * Tmax + yy] = v;
        }
        if (attn)
            for (int x = r0; x < Tx; x += ROWS) attn[((size_t)b * Tx + x) * Tmax + yy] = id == x ? 1.f : 0.f;
    }
}

}  // namespace

extern "C" int glowtts_prior_sample(const float* mean, const float* log_std, const float* dur, const int64_t* mel_lengths, const uint32_t* seeds,
                                    const float* noise_scales, float* z, int32_t* idx, float* attn, int B, int C, int Tx, int Tmax, void* stream)
{
    if (!mean || !log_std || !dur || !mel_lengths || !seeds || !noise_scales || !z || !idx || B < 1 || B > 65535 || C < 1 || Tx < 1 || Tmax < 1)
        return GLOWTTS_E_ARG;
    if ((int64_t)Tmax + TILE >= ((int64_t)1 << 31) || (int64_t)Tmax / 2 * C + C >= ((int64_t)1 << 32)) return GLOWTTS_E_ARG;      // frame and pair counters stay in range
    const dim3 grid((Tmax + TILE - 1) / TILE, B);
    const bool vec = (Tmax & 3) == 0 && ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(attn)) & 15) == 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(prior_sample_kernel<true>, grid, dim3(THREADS), 0, s, mean, log_std, dur, mel_lengths, seeds, noise_scales, z, idx, attn, C, Tx, Tmax);
    else     hipLaunchKernelGGL(prior_sample_kernel<false>, grid, dim3(THREADS), 0, s, mean, log_std, dur, mel_lengths, seeds, noise_scales, z, idx, attn, C, Tx, Tmax);
    GLOWTTS_NOTE_STATIC("prior_sample");
    RET_LAUNCH();
}
