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
// The z rows of step 2 are `sample_rows`, shared with the teacher-forced kernel at the end of this file (glowtts_prior_sample_aligned: the index is given, not
// built), so that both write the same bits for the same index.
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

// Step 2 of both kernels below: the z rows of one frame tile of one utterance.  idx_s holds the tile's token indices (-1: no token); m / l / z are the
// utterance's own [C][Tx] / [C][Tmax] slabs.  All 256 threads call it behind the barrier that publishes idx_s; there is no barrier inside.
template <bool VEC>
__device__ __forceinline__ void sample_rows(const gauss_hash::Keys& keys, float scale, const float* __restrict__ mb, const float* __restrict__ lb,
                                            float* __restrict__ zb, const int32_t* idx_s, int y0, int C, int Tx, int Tmax)
{
    const int tid = threadIdx.x;
    if (VEC) {
        const int g = tid & (TILE / 4 - 1), r0 = tid / (TILE / 4);
        constexpr int ROWS = THREADS / (TILE / 4);
        const int yy = y0 + 4 * g;
        if (yy >= Tmax) return;                            // (Tmax % 4 == 0: a group lies wholly inside or outside)
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
            *reinterpret_cast<float4*>(zb + (size_t)c * Tmax + yy) = o;
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
            zb[(size_t)c * Tmax + yy] = v;
        }
    }
}

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
    sample_rows<VEC>(keys, noise_scales[b], mean + (size_t)b * C * Tx, log_std + (size_t)b * C * Tx, z + (size_t)b * C * Tmax, idx_s, y0, C, Tx, Tmax);
    if (!attn) return;
    if (VEC) {
        const int g = tid & (TILE / 4 - 1), r0 = tid / (TILE / 4);
        constexpr int ROWS = THREADS / (TILE / 4);
        const int yy = y0 + 4 * g;
        if (yy >= Tmax) return;
        const int i0 = idx_s[4 * g], i1 = idx_s[4 * g + 1], i2 = idx_s[4 * g + 2], i3 = idx_s[4 * g + 3];
        for (int x = r0; x < Tx; x += ROWS) {
            float4 o;
            o.x = i0 == x ? 1.f : 0.f; o.y = i1 == x ? 1.f : 0.f; o.z = i2 == x ? 1.f : 0.f; o.w = i3 == x ? 1.f : 0.f;
            *reinterpret_cast<float4*>(attn + ((size_t)b * Tx + x) * Tmax + yy) = o;
        }
    } else {
        const int f = tid & (TILE - 1), r0 = tid / TILE;
        constexpr int ROWS = THREADS / TILE;
        const int yy = y0 + f;
        if (yy >= Tmax) return;
        const int id = idx_s[f];
        for (int x = r0; x < Tx; x += ROWS) attn[((size_t)b * Tx + x) * Tmax + yy] = id == x ? 1.f : 0.f;
    }
}

// ---- teacher-forced pass: the sample of the prior ALONG a given per-frame token index (MAS's), the index's run lengths and the alignment score ----
// Grid (frame tiles [+ 1 when durations are asked for], utterance), 256 threads.
//   tile blocks   read their 64 indices (anything outside [0, Tx) becomes -1), write the z rows through `sample_rows` - the code glowtts_prior_sample runs - and
//                 sum  -0.5 log(2 pi) - ls - 0.5 (z_rec - m)^2 exp(-2 ls)  over (channel, frame in tile): thread (row r = tid / 64, frame f = tid % 64) adds
//                 channels r, r + 4, ... in ascending order, the four rows of a frame are added in ascending order, the 64 frames by one shuffle tree.  The
//                 layout does not depend on the store form; terms and sums are float64 (one rounding, to the float partial), invalid frames add +0.0.
//   the last block (blockIdx.x == ntiles) counts the frames of every token: an int32 histogram in LDS, CHUNK tokens per pass over the utterance's indices -
//                 it asks nothing of the index's order.
// prior_score_final_kernel, one wave per utterance: valid frames counted, the tile partials added in ascending order (float64), divided, rounded once.
constexpr double HALF_LOG_2PI = 0.91893853320467274178;

template <bool VEC>
__global__ __launch_bounds__(THREADS) void prior_sample_aligned_kernel(const float* __restrict__ mean, const float* __restrict__ log_std, const int32_t* __restrict__ idx,
                                                                       const float* __restrict__ z_rec, const uint32_t* __restrict__ seeds,
                                                                       const float* __restrict__ noise_scales, float* __restrict__ z, int32_t* __restrict__ dur,
                                                                       float* __restrict__ partials, int C, int Tx, int Tmax, int ntiles)
{
    // (static LDS of both block roles, 6.3 KB in all: a tile block never touches hist_s, the duration block only hist_s - far below what would cost a wave of
    //  occupancy, so the roles are not split into two kernels)
    __shared__ int32_t hist_s[CHUNK];
    __shared__ int32_t idx_s[TILE];
    __shared__ double part_s[THREADS];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int32_t* ib = idx + (size_t)b * Tmax;
    if ((int)blockIdx.x == ntiles) {                       // (launched only when dur is given; uniform over the workgroup)
        for (int x0 = 0; x0 < Tx; x0 += CHUNK) {
            const int n = min(CHUNK, Tx - x0);
            for (int j = tid; j < n; j += THREADS) hist_s[j] = 0;
            __syncthreads();
            for (int y = tid; y < Tmax; y += THREADS) {
                const uint32_t rel = (uint32_t)ib[y] - (uint32_t)x0;      // (a negative index wraps beyond n)
                if (rel < (uint32_t)n) atomicAdd(&hist_s[rel], 1);
            }
            __syncthreads();
            for (int j = tid; j < n; j += THREADS) dur[(size_t)b * Tx + x0 + j] = hist_s[j];
            __syncthreads();                               // (the next pass clears hist_s)
        }
        return;
    }
    const int y0 = blockIdx.x * TILE;
    if (tid < TILE) {
        const int y = y0 + tid;
        const int id = y < Tmax ? ib[y] : -1;
        idx_s[tid] = (uint32_t)id < (uint32_t)Tx ? id : -1;
    }
    __syncthreads();
    const float* mb = mean + (size_t)b * C * Tx;
    const float* lb = log_std + (size_t)b * C * Tx;
    if (z) sample_rows<VEC>(gauss_hash::keys(seeds[2 * b], seeds[2 * b + 1]), noise_scales[b], mb, lb, z + (size_t)b * C * Tmax, idx_s, y0, C, Tx, Tmax);
    if (!partials) return;                                 // (uniform)
    const int f = tid & (TILE - 1), r0 = tid / TILE;
    constexpr int ROWS = THREADS / TILE;
    const int id = idx_s[f];                               // (>= 0 only for frames below Tmax)
    double acc = 0.0;
    if (id >= 0) {
        const float* zr = z_rec + (size_t)b * C * Tmax + y0 + f;
        for (int c = r0; c < C; c += ROWS) {
            const double ls = (double)lb[(size_t)c * Tx + id];
            const double d = (double)zr[(size_t)c * Tmax] - (double)mb[(size_t)c * Tx + id];
            acc += (-HALF_LOG_2PI - ls) - 0.5 * d * d * exp(-2.0 * ls);
        }
    }
    part_s[tid] = acc;
    __syncthreads();
    if (tid < TILE) {
        double s = part_s[tid];
#pragma unroll
        for (int r = 1; r < ROWS; ++r) s += part_s[r * TILE + tid];
        static_assert(TILE == 64, "one wave holds the tile's frames");
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (tid == 0) partials[(size_t)b * ntiles + blockIdx.x] = (float)s;
    }
}

__global__ __launch_bounds__(64) void prior_score_final_kernel(const int32_t* __restrict__ idx, const float* __restrict__ partials, float* __restrict__ score,
                                                               int C, int Tx, int Tmax, int ntiles)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int32_t* ib = idx + (size_t)b * Tmax;
    int frames = 0;
    for (int y = lane; y < Tmax; y += 64) frames += (uint32_t)ib[y] < (uint32_t)Tx ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) frames += __shfl_down(frames, o, 64);
    if (lane != 0) return;
    double s = 0.0;
    for (int t = 0; t < ntiles; ++t) s += (double)partials[(size_t)b * ntiles + t];
    score[b] = frames > 0 ? (float)(s / ((double)frames * (double)C)) : 0.f;
}

}  // namespace

extern "C" int glowtts_prior_sample_aligned(const float* mean, const float* log_std, const int32_t* idx, const float* z_rec, const uint32_t* seeds,
                                            const float* noise_scales, float* z, int32_t* dur, float* score, float* score_partials, int B, int C, int Tx,
                                            int Tmax, void* stream)
{
    if (!mean || !log_std || !idx || (z && (!seeds || !noise_scales)) || (score && (!score_partials || !z_rec)) || (!z && !dur && !score) || B < 1 ||
        B > 65535 || C < 1 || Tx < 1 || Tmax < 1)
        return GLOWTTS_E_ARG;
    if ((int64_t)Tmax + TILE >= ((int64_t)1 << 31) || (int64_t)Tmax / 2 * C + C >= ((int64_t)1 << 32)) return GLOWTTS_E_ARG;      // frame and pair counters stay in range
    const int ntiles = (Tmax + TILE - 1) / TILE;
    const dim3 grid(ntiles + (dur ? 1 : 0), B);
    float* partials = score ? score_partials : nullptr;
    const bool vec = (Tmax & 3) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(prior_sample_aligned_kernel<true>, grid, dim3(THREADS), 0, s, mean, log_std, idx, z_rec, seeds, noise_scales, z, dur, partials, C, Tx, Tmax, ntiles);
    else     hipLaunchKernelGGL(prior_sample_aligned_kernel<false>, grid, dim3(THREADS), 0, s, mean, log_std, idx, z_rec, seeds, noise_scales, z, dur, partials, C, Tx, Tmax, ntiles);
    GLOWTTS_NOTE_STATIC("prior_sample_aligned");
    if (!score) RET_LAUNCH();
    if (hipGetLastError() != hipSuccess) return GLOWTTS_E_LAUNCH;
    hipLaunchKernelGGL(prior_score_final_kernel, dim3(B), dim3(64), 0, s, idx, score_partials, score, C, Tx, Tmax, ntiles);
    GLOWTTS_NOTE_STATIC("prior_score_final");
    RET_LAUNCH();
}

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
