// The Parallel WaveGAN discriminator for gfx950, f32: forward, data backward, weight gradients and the least-squares loss (DESIGN.md "Training the Parallel
// WaveGAN discriminator").  `Layers` 1-D convolutions of kernel size 3 over the waveform [B][T]: 1 -> C (dilation 1), C -> C with dilation i for the middle
// layers i = 1 .. Layers - 2, C -> 1 (dilation 1); "same" zero padding, bias, LeakyReLU after every layer but the last.  Rows are samples, channels-last
// [B][T][C], every batch row of the full length T; tiles are counted from a batch row's own sample 0 and every tap is masked by the row's own [0, T), so a
// row's score does not depend on the batch around it.  Every matrix product runs on v_mfma_f32_16x16x4_f32 (`mfma4`; operand layout: see pwg_ops.hip).
// No float atomics, no kernel waits on another workgroup, every sum has a fixed partition and order: every output is bit-identical from run to run.
//
//   pwg_disc_first      1 -> C: three taps on the VALU (bias, then taps ascending), LeakyReLU; one thread per (sample, 4 channels).
//   pwg_disc_layer      per 64-row tile of one middle layer: the generator's row gather (pwg_common.h, no conditioning columns) of [h(t - d) | h(t) | h(t + d)]
//                       into LDS, K = 3 C against the packed image w [3 C][C] (row = tap * C + input channel), bias-initialised accumulators, k ascending,
//                       LeakyReLU; writes the layer's output to its own slab (the backward reads the mask from it: LeakyReLU is monotone).
//   pwg_disc_last       C -> 1: one thread per sample, bias, then taps and channels ascending.
//   pwg_disc_mse        sum (p - v)^2 of 4096 scores per block as a float64 sum in a fixed tree order, and d p = factor 2 (p - v) / count; the scores before
//                       `split` are held against v0, the others against v1, each part is a mean of its own.  `pwg_disc_mse_sum`: the blocks' sums in
//                       ascending order -> (factor (m0 + m1), m0, m1).
//   pwg_disc_last_bwd   d h of the last hidden layer from d p: per (sample, 4 channels), taps ascending.
//   pwg_disc_layer_bwd  per 64-row tile: gathers dpre(t + d) | dpre(t) | dpre(t - d) with dpre = dout (out > 0 ? 1 : slope) formed during the gather, zero
//                       outside the row, K = 3 C against wt [3 C][C] (row = tap * C + output channel), writes dx; its own rows of dpre go to a separate
//                       buffer for the weight gradient (never in place over dout: neighbouring tiles still read it) unless that buffer is NULL.
//   pwg_disc_first_bwd  d wav(t): per sample, the three taps' dot products over C (channels ascending), added as (s0 + s1) + s2; writes dpre of layer 0 for
//                       the weight gradient unless that buffer is NULL.
//   pwg_disc_wgrad      the generator's weight-gradient kernels (pwg_wgrad.h) under the discriminator's names: three tap jobs per layer, the centre one with
//                       the constant-one column that yields the bias; + `pwg_disc_wgrad_sum`.
#include <algorithm>

#include "launch_log.h"
#include "pwg_common.h"
#include "pwg_wgrad.h"

namespace {

constexpr int MSE_ELEMS = 4096;                           // scores of one block of the loss

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }
__device__ __forceinline__ float lmask(float dout, float out, float slope) { return out > 0.f ? dout : dout * slope; }

// ---- first layer: grid (ceil(T C / 4 / 256), B).  w [3][C]: row = tap ----
__global__ __launch_bounds__(THREADS) void pwg_disc_first_kernel(const float* __restrict__ wav, const float* __restrict__ w, const float* __restrict__ bias,
                                                                 float* __restrict__ out, int T, int C, float slope)
{
    const int b = blockIdx.y, c4n = C >> 2;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t t = e / c4n;
    if (t >= T) return;
    const int c = (int)(e - t * c4n) * 4;
    const float* x = wav + (size_t)b * T;
    float4 acc = *reinterpret_cast<const float4*>(bias + c);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int64_t ts = t + j - 1;
        const float xv = ts >= 0 && ts < T ? x[ts] : 0.f;
        const float4 wv = *reinterpret_cast<const float4*>(w + j * C + c);
        acc.x = fmaf(wv.x, xv, acc.x); acc.y = fmaf(wv.y, xv, acc.y); acc.z = fmaf(wv.z, xv, acc.z); acc.w = fmaf(wv.w, xv, acc.w);
    }
    acc.x = lrelu(acc.x, slope); acc.y = lrelu(acc.y, slope); acc.z = lrelu(acc.z, slope); acc.w = lrelu(acc.w, slope);
    *reinterpret_cast<float4*>(out + ((size_t)b * T + t) * C + c) = acc;
}

// ---- middle layer: grid (ceil(T / 64), B), LDS Xs [64][xs] ----
__global__ __launch_bounds__(THREADS) void pwg_disc_layer_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                 float* __restrict__ out, int T, int C, int d, int xs, float slope)
{
    extern __shared__ __attribute__((aligned(16))) float pwd_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, t0 = blockIdx.x * TM;
    const size_t row0 = (size_t)b * T;
    float* Xs = pwd_smem;
    pwg_gather_rows(x, nullptr, Xs, row0, t0, T, C, 0, d, xs);
    __syncthreads();
    const int K = 3 * C;
    for (int n = wave; n < C / 16; n += WAVES) {
        const int col = n * 16 + r;
        const float bv = bias[col];
        f32x4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{bv, bv, bv, bv};
        const float* xa = Xs + r * xs + q;
        for (int k0 = 0; k0 < K; k0 += 4) {
            const float wk = w[(size_t)(k0 + q) * C + col];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[rt] = mfma4(xa[rt * 16 * xs + k0], wk, acc[rt]);
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + rt * 16 + q * 4 + i;
                if (t < T) out[(row0 + t) * C + col] = lrelu(acc[rt][i], slope);
            }
    }
}

// ---- last layer: grid (ceil(T / 256), B).  w [3][C]: row = tap ----
__global__ __launch_bounds__(THREADS) void pwg_disc_last_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                float* __restrict__ scores, int T, int C)
{
    const int b = blockIdx.y, t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const size_t row0 = (size_t)b * T;
    float acc = bias[0];
    for (int j = 0; j < 3; ++j) {
        const int ts = t + j - 1;
        if (ts < 0 || ts >= T) continue;
        const float* h = x + (row0 + ts) * C;
        for (int c = 0; c < C; c += 4) {
            const float4 hv = *reinterpret_cast<const float4*>(h + c), wv = *reinterpret_cast<const float4*>(w + j * C + c);
            acc = fmaf(hv.x, wv.x, acc); acc = fmaf(hv.y, wv.y, acc); acc = fmaf(hv.z, wv.z, acc); acc = fmaf(hv.w, wv.w, acc);
        }
    }
    scores[row0 + t] = acc;
}

// ---- loss: grid (ceil(N / 4096)) -> partial [blocks][2] float64 ----
__global__ __launch_bounds__(THREADS) void pwg_disc_mse_kernel(const float* __restrict__ p, float* __restrict__ dp, double* __restrict__ partial, int64_t N,
                                                               int64_t split, float v0, float v1, float factor)
{
    __shared__ double red[THREADS];
    const int tid = threadIdx.x;
    const float g0 = factor * 2.f / (float)split, g1 = split < N ? factor * 2.f / (float)(N - split) : 0.f;
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < MSE_ELEMS / THREADS; ++k) {
        const int64_t e = (int64_t)blockIdx.x * MSE_ELEMS + k * THREADS + tid;
        if (e >= N) break;
        const bool first = e < split;
        const float diff = p[e] - (first ? v0 : v1);
        dp[e] = diff * (first ? g0 : g1);
        const double sq = (double)diff * (double)diff;
        if (first) s0 += sq; else s1 += sq;
    }
    const double t0 = block_sum(s0, red, tid), t1 = block_sum(s1, red, tid);
    if (tid == 0) { partial[2 * (size_t)blockIdx.x] = t0; partial[2 * (size_t)blockIdx.x + 1] = t1; }
}

__global__ __launch_bounds__(64) void pwg_disc_mse_sum_kernel(const double* __restrict__ partial, float* __restrict__ loss, int blocks, int64_t N, int64_t split,
                                                              float factor)
{
    if (threadIdx.x != 0) return;
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < blocks; ++k) { s0 += partial[2 * (size_t)k]; s1 += partial[2 * (size_t)k + 1]; }
    const double m0 = s0 / (double)split, m1 = split < N ? s1 / (double)(N - split) : 0.0;
    loss[0] = (float)((double)factor * (m0 + m1));
    loss[1] = (float)m0;
    loss[2] = (float)m1;
}

// ---- d h of the last hidden layer: grid (ceil(T C / 4 / 256), B): dh(u)[c] = sum_j dp(u - (j - 1)) w[j][c] ----
__global__ __launch_bounds__(THREADS) void pwg_disc_last_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ w, float* __restrict__ dh, int T, int C)
{
    const int b = blockIdx.y, c4n = C >> 2;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t t = e / c4n;
    if (t >= T) return;
    const int c = (int)(e - t * c4n) * 4;
    const float* g = dp + (size_t)b * T;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int64_t ts = t - (j - 1);
        const float gv = ts >= 0 && ts < T ? g[ts] : 0.f;
        const float4 wv = *reinterpret_cast<const float4*>(w + j * C + c);
        acc.x = fmaf(wv.x, gv, acc.x); acc.y = fmaf(wv.y, gv, acc.y); acc.z = fmaf(wv.z, gv, acc.z); acc.w = fmaf(wv.w, gv, acc.w);
    }
    *reinterpret_cast<float4*>(dh + ((size_t)b * T + t) * C + c) = acc;
}

// ---- middle layer, backward: grid (ceil(T / 64), B), LDS Ds [64][xs].  dout, out [B][T][C]: the gradient of the layer's output and that output ----
__global__ __launch_bounds__(THREADS) void pwg_disc_layer_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out, const float* __restrict__ wt,
                                                                     float* __restrict__ dx, float* __restrict__ dpre, int T, int C, int d, int xs, float slope)
{
    extern __shared__ __attribute__((aligned(16))) float pwd_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, t0 = blockIdx.x * TM;
    const size_t row0 = (size_t)b * T;
    float* Ds = pwd_smem;
    const int K = 3 * C, kq = K >> 2;
    for (int e = tid; e < TM * kq; e += THREADS) {
        const int row = e / kq, k4 = (e - row * kq) * 4, t = t0 + row;
        const int j = k4 / C, g = k4 - j * C, ts = t - (j - 1) * d;      // tap j of the forward read x(t + (j - 1) d): x(u) is reached from t = u - (j - 1) d
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < T && ts >= 0 && ts < T) {
            const float4 gv = *reinterpret_cast<const float4*>(dout + (row0 + ts) * C + g), ov = *reinterpret_cast<const float4*>(out + (row0 + ts) * C + g);
            v = make_float4(lmask(gv.x, ov.x, slope), lmask(gv.y, ov.y, slope), lmask(gv.z, ov.z, slope), lmask(gv.w, ov.w, slope));
            if (j == 1 && dpre) *reinterpret_cast<float4*>(dpre + (row0 + t) * C + g) = v;
        }
        *reinterpret_cast<float4*>(Ds + row * xs + k4) = v;
    }
    __syncthreads();
    for (int n = wave; n < C / 16; n += WAVES) {
        const int col = n * 16 + r;                        // input channel
        f32x4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* da = Ds + r * xs + q;
        for (int k0 = 0; k0 < K; k0 += 4) {
            const float wk = wt[(size_t)(k0 + q) * C + col];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[rt] = mfma4(da[rt * 16 * xs + k0], wk, acc[rt]);
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + rt * 16 + q * 4 + i;
                if (t < T) dx[(row0 + t) * C + col] = acc[rt][i];
            }
    }
}

// ---- first layer, backward: grid (ceil(T / 256), B).  dout, out [B][T][C] of layer 0; w [3][C] ----
__global__ __launch_bounds__(THREADS) void pwg_disc_first_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out, const float* __restrict__ w,
                                                                     float* __restrict__ dwav, float* __restrict__ dpre, int T, int C, float slope)
{
    const int b = blockIdx.y, t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const size_t row0 = (size_t)b * T;
    float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int ts = t - (j - 1);
        if (ts < 0 || ts >= T) continue;
        const float* g = dout + (row0 + ts) * C;
        const float* o = out + (row0 + ts) * C;
        for (int c = 0; c < C; c += 4) {
            const float4 gv = *reinterpret_cast<const float4*>(g + c), ov = *reinterpret_cast<const float4*>(o + c);
            const float4 wv = *reinterpret_cast<const float4*>(w + j * C + c);
            const float4 v = make_float4(lmask(gv.x, ov.x, slope), lmask(gv.y, ov.y, slope), lmask(gv.z, ov.z, slope), lmask(gv.w, ov.w, slope));
            if (j == 1 && dpre) *reinterpret_cast<float4*>(dpre + (row0 + t) * C + c) = v;
            s[j] = fmaf(v.x, wv.x, s[j]); s[j] = fmaf(v.y, wv.y, s[j]); s[j] = fmaf(v.z, wv.z, s[j]); s[j] = fmaf(v.w, wv.w, s[j]);
        }
    }
    dwav[row0 + t] = (s[0] + s[1]) + s[2];
}

// ---- host side ----
int layer_lds(int C) { return TM * lds_stride_of(3 * C) * 4; }
bool bad_channels(int C) { return C < 16 || C > MAX_CHANNELS || C % 16 || layer_lds(C) > MAX_LDS; }
// every batch row of the full length T: the generator's limits with one sample per "frame", B T < 2^31
bool bad_rows(int B, int T) { return bad_train_batch(B, T, 1) || (int64_t)B * T >= ((int64_t)1 << 31); }
unsigned quad_blocks(int T, int C) { return (unsigned)(((int64_t)T * (C / 4) + THREADS - 1) / THREADS); }

}  // namespace

extern "C" int glowtts_pwg_disc_supported(int C, int layers, int max_dilation)
{
    return !bad_channels(C) && layers >= 3 && layers <= 16 && max_dilation >= 1 && max_dilation <= 1024;
}

extern "C" int64_t glowtts_pwg_disc_work_floats(int B, int T, int C)
{
    if (bad_rows(B, T) || bad_channels(C)) return 0;
    const int64_t splits = (int64_t)B * (((int64_t)T + WG_ROWS - 1) / WG_ROWS);
    const int64_t wg = splits * 256 * (int64_t)(2 * tiles16(C) + tiles16(C + 1)) * tiles16(C);
    const int64_t mse = 4 * (((int64_t)B * T + MSE_ELEMS - 1) / MSE_ELEMS);
    return std::max(wg, mse);
}

extern "C" int glowtts_pwg_disc_first(const float* wav, const float* w, const float* bias, float* out, int B, int T, int C, float slope, void* stream)
{
    if (!wav || !w || !bias || !out || bad_rows(B, T) || bad_channels(C)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("pwg_disc_first");
    hipLaunchKernelGGL(pwg_disc_first_kernel, dim3(quad_blocks(T, C), B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), wav, w, bias, out, T, C, slope);
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_disc_layer(const float* x, const float* w, const float* bias, float* out, int B, int T, int C, int dilation, float slope, void* stream)
{
    if (!x || !w || !bias || !out || x == out || bad_rows(B, T) || bad_channels(C) || dilation < 1 || dilation > 1024) return GLOWTTS_E_ARG;
    const int lds = layer_lds(C);
    if (allow_lds<&pwg_disc_layer_kernel>(lds) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("pwg_disc_layer");
    hipLaunchKernelGGL(pwg_disc_layer_kernel, dim3((T + TM - 1) / TM, B), dim3(THREADS), (size_t)lds, static_cast<hipStream_t>(stream), x, w, bias, out, T, C, dilation,
                       lds_stride_of(3 * C), slope);
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_disc_last(const float* x, const float* w, const float* bias, float* scores, int B, int T, int C, void* stream)
{
    if (!x || !w || !bias || !scores || bad_rows(B, T) || bad_channels(C)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("pwg_disc_last");
    hipLaunchKernelGGL(pwg_disc_last_kernel, dim3((T + THREADS - 1) / THREADS, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), x, w, bias, scores, T, C);
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_disc_mse(const float* p, float* dp, float* work, float* loss, int64_t N, int64_t split, float v0, float v1, float factor, void* stream)
{
    if (!p || !dp || !work || !loss || N < 1 || N >= ((int64_t)1 << 31) || split < 1 || split > N || (reinterpret_cast<uintptr_t>(work) & 7)) return GLOWTTS_E_ARG;
    const int blocks = (int)((N + MSE_ELEMS - 1) / MSE_ELEMS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    GLOWTTS_NOTE_STATIC("pwg_disc_mse");
    hipLaunchKernelGGL(pwg_disc_mse_kernel, dim3(blocks), dim3(THREADS), 0, s, p, dp, reinterpret_cast<double*>(work), N, split, v0, v1, factor);
    GLOWTTS_NOTE_STATIC("pwg_disc_mse_sum");
    hipLaunchKernelGGL(pwg_disc_mse_sum_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const double*>(work), loss, blocks, N, split, factor);
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_disc_last_bwd(const float* dp, const float* w, float* dh, int B, int T, int C, void* stream)
{
    if (!dp || !w || !dh || bad_rows(B, T) || bad_channels(C)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("pwg_disc_last_bwd");
    hipLaunchKernelGGL(pwg_disc_last_bwd_kernel, dim3(quad_blocks(T, C), B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), dp, w, dh, T, C);
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_disc_layer_bwd(const float* dout, const float* out, const float* wt, float* dx, float* dpre, int B, int T, int C, int dilation, float slope,
                                          void* stream)
{
    if (!dout || !out || !wt || !dx || dx == dout || dpre == dout || bad_rows(B, T) || bad_channels(C) || dilation < 1 || dilation > 1024) return GLOWTTS_E_ARG;
    const int lds = layer_lds(C);
    if (allow_lds<&pwg_disc_layer_bwd_kernel>(lds) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("pwg_disc_layer_bwd");
    hipLaunchKernelGGL(pwg_disc_layer_bwd_kernel, dim3((T + TM - 1) / TM, B), dim3(THREADS), (size_t)lds, static_cast<hipStream_t>(stream), dout, out, wt, dx, dpre, T, C,
                       dilation, lds_stride_of(3 * C), slope);
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_disc_first_bwd(const float* dout, const float* out, const float* w, float* dwav, float* dpre, int B, int T, int C, float slope, void* stream)
{
    if (!dout || !out || !w || !dwav || dpre == dout || bad_rows(B, T) || bad_channels(C)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("pwg_disc_first_bwd");
    hipLaunchKernelGGL(pwg_disc_first_bwd_kernel, dim3((T + THREADS - 1) / THREADS, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), dout, out, w, dwav, dpre, T, C,
                       slope);
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_disc_wgrad(const float* a, const float* dpre, const int32_t* lengths, float* work, float* dw, float* db, int B, int T, int Cin, int Cout,
                                      int dilation, void* stream)
{
    if (!a || !dpre || !lengths || !work || !dw || !db || bad_rows(B, T) || dilation < 1 || dilation > 1024 || (Cin != 1 && bad_channels(Cin)) ||
        (Cout != 1 && bad_channels(Cout)) || (Cin == 1 && Cout == 1))
        return GLOWTTS_E_ARG;
    wg_args args = {};
    for (int j = 0; j < 3; ++j)                                              // weight [Cout][Cin][3]: tap j read a(t + (j - 1) d)
        add_job(args, a, Cin, Cin, (j - 1) * dilation, dpre, Cout, Cout, dw + j, 3, 3 * Cin, j == 1 ? db : nullptr, 1.f);
    return wgrad_launch(args, lengths, work, B, T, 1, "pwg_disc_wgrad", "pwg_disc_wgrad_sum", stream);
}
