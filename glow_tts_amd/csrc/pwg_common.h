// What the Parallel WaveGAN generator's forward (pwg_ops.hip) and backward (pwg_train_ops.hip) share: the tile constants, the host-side
// batch and LDS checks, the layer's row gather and the head's first stage.  The backward recomputes the gate and the head's hidden layer from rows and
// sums that are this text, not a copy of it; what it must additionally keep in step with the forward is said at the two GEMM 1 loops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glowtts_hip.h"
#include "device_common.h"

namespace {

constexpr int TM = 64;                                    // samples (rows) per workgroup: four 16-row MFMA tiles
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_LDS = 160 * 1024;
constexpr int MAX_SCALE = 16, MAX_CHANNELS = 256;
constexpr float RSQRT2 = 0.70710678118654752440f;

bool bad_batch(int B, int Lmax, int hop)
{
    return B < 1 || B > 65535 || Lmax < 1 || hop < 1 || hop > (1 << 16) || (int64_t)Lmax * hop > ((int64_t)1 << 30);
}

// Allows `Kernel` this much dynamic LDS.  The largest size allowed so far is remembered per kernel in a process-wide static: one device per process is assumed,
// it grows monotonically, and a racing second caller sets the same or a larger value.
template <auto Kernel> int allow_lds(int bytes)
{
    static int allowed = 0;
    if (bytes > allowed) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return GLOWTTS_E_LAUNCH;
        allowed = bytes;
    }
    return GLOWTTS_OK;
}

// The sum of `v` over the workgroup's 256 threads in a fixed tree order (red: 256 doubles of LDS); every thread gets it.
__device__ __forceinline__ double block_sum(double v, double* red, int tid)
{
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = THREADS >> 1; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// The layer's rows: [x(t - d) | x(t) | x(t + d) | c(t)] of samples t0 .. t0 + 63 of the utterance whose slab starts at row0 and holds T samples, zero outside
// it, into Xs [64][xs]; K = 3 R + A floats per row, 16 bytes per access, coalesced along the channels.  No barrier.
__device__ __forceinline__ void pwg_gather_rows(const float* __restrict__ x, const float* __restrict__ c, float* Xs, size_t row0, int t0, int T, int R, int A, int d,
                                                int xs)
{
    const int kq = (3 * R + A) >> 2;
    for (int e = threadIdx.x; e < TM * kq; e += THREADS) {
        const int row = e / kq, k4 = (e - row * kq) * 4, t = t0 + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < T) {
            if (k4 < 3 * R) {
                const int j = k4 / R, ci = k4 - j * R, ts = t + (j - 1) * d;
                if (ts >= 0 && ts < T) v = *reinterpret_cast<const float4*>(x + (row0 + ts) * R + ci);
            } else {
                v = *reinterpret_cast<const float4*>(c + (row0 + t) * A + (k4 - 3 * R));
            }
        }
        *reinterpret_cast<float4*>(Xs + row * xs + k4) = v;
    }
}

// The head's first stage for the 64 rows from t0, in two steps so that each kernel keeps its own loop over the column tiles and its own epilogue (one function
// with an epilogue functor made the compiler hoist the epilogue's 16 store addresses out of that loop: +36 VGPRs in the backward).
// a. y = relu(scale skips) into Ys [64][S + 4], zero beyond T; `keep_y(offset, y)` sees every float4 inside the utterance at its offset in the [rows][S]
//    tensor.  Ends with the barrier.
template <typename KeepY>
__device__ __forceinline__ void pwg_head_stage(const float* __restrict__ skips, float* Ys, size_t row0, int t0, int T, int S, float scale, KeepY keep_y)
{
    const int st = S + 4, kq = S >> 2;
    for (int e = threadIdx.x; e < TM * kq; e += THREADS) {
        const int row = e / kq, k4 = (e - row * kq) * 4, t = t0 + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < T) {
            v = *reinterpret_cast<const float4*>(skips + (row0 + t) * S + k4);
            v.x = fmaxf(v.x * scale, 0.f); v.y = fmaxf(v.y * scale, 0.f); v.z = fmaxf(v.z * scale, 0.f); v.w = fmaxf(v.w * scale, 0.f);
            keep_y((row0 + t) * S + k4, v);
        }
        *reinterpret_cast<float4*>(Ys + row * st + k4) = v;
    }
    __syncthreads();
}
// b. h' = W1 y + b1 for the wave's 16 columns (this lane's: col) and all four row tiles: bias-initialised, k ascending.  w1 [S][S], row = input channel.
__device__ __forceinline__ void pwg_head_w1(const float* Ys, const float* __restrict__ w1, const float* __restrict__ b1, int S, int col, f32x4 (&acc)[4])
{
    const int lane = threadIdx.x & 63, st = S + 4;
    const float bv = b1[col];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{bv, bv, bv, bv};
    const float* ya = Ys + (lane & 15) * st + (lane >> 4);
    for (int k0 = 0; k0 < S; k0 += 4) {
        const float wk = w1[(size_t)(k0 + (lane >> 4)) * S + col];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = mfma4(ya[rt * 16 * st + k0], wk, acc[rt]);
    }
}

}  // namespace
