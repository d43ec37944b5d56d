// What the per-frame loss kernels on the LDS FFT share beyond vocoder_fft.h - the STFT loss (stft_loss_ops.hip) and the mel loss (mel_loss_ops.hip): the fixed
// float64 reduction tree of a workgroup, the overlap-add of windowed frame gradients as a gather (the one fold body of both backwards), and the grid of a
// frame kernel.  Each written once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vocoder_fft.h"

namespace {

// fixed tree over the workgroup's 256 values of each of NS sums; the result is in red[i][0]
template <int NS>
__device__ __forceinline__ void voc_tree(double (*red)[VOC_NT], int tid)
{
    __syncthreads();
    for (int h = VOC_NT >> 1; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int i = 0; i < NS; ++i) red[i][tid] += red[i][tid + h];
        }
        __syncthreads();
    }
}

// d pred[b][s] = dpad(M + s) + [1 <= s <= M] dpad(M - s) + [T - 1 - M <= s <= T - 2] dpad(M + 2 (T - 1) - s), dpad(p) = the frames' contributions at padded
// position p summed in ascending frame order (window position j = p - lpad - t hop in [0, win)).  dframes [B][NF][win]; grid ((T + 255) / 256, B) x 256.
__global__ __launch_bounds__(256) void voc_frames_fold_kernel(const float* __restrict__ dframes, float* __restrict__ dpred, int T, int NF, int n_fft, int win, int hop,
                                                              int accumulate)
{
    const int b = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s >= T) return;
    const int M = n_fft >> 1, lpad = (n_fft - win) >> 1;
    const float* fb = dframes + (int64_t)b * NF * win;
    auto dpad = [&](int p) {
        const int pp = p - lpad;
        float acc = 0.f;
        if (pp < 0) return acc;
        int t_hi = pp / hop;
        const int t_lo = pp >= win ? (pp - win) / hop + 1 : 0;
        if (t_hi > NF - 1) t_hi = NF - 1;
        for (int t = t_lo; t <= t_hi; ++t) acc += fb[(int64_t)t * win + (pp - t * hop)];
        return acc;
    };
    float r = dpad(M + s);
    if (s >= 1 && s <= M) r += dpad(M - s);
    if (s >= T - 1 - M && s <= T - 2) r += dpad(M + 2 * (T - 1) - s);
    float* out = dpred + (int64_t)b * T + s;
    *out = accumulate ? *out + r : r;
}

int voc_frames_grid(int frames) { return frames < 1280 ? frames : 1280; }     // 5 resident workgroups (by LDS at n_fft = 2048) on each of 256 CUs; more frames: strided
// the sizes every frame loss shares: 1 <= B <= 65535, B T < 2^31, B NF <= 2^24 (the caller has checked hop >= 1)
bool voc_frames_bad_batch(int B, int T, int hop) { return B < 1 || B > 65535 || (int64_t)B * T >= (int64_t)1 << 31 || (int64_t)B * (1 + T / hop) > (int64_t)1 << 24; }

}  // namespace
