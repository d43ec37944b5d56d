// The HiFi-GAN multi-period discriminator for gfx950, f32: forward, data backward, weight gradients and the feature-matching loss (DESIGN.md "Training the
// HiFi-GAN discriminator").  One sub-network per period p: the waveform [B][T] is reflect-padded on the right to Tp = H0 p samples (sample T + j is sample
// T - 2 - j) and folded to rows (h, c) = (n / p, n % p); every convolution runs over h alone.  Activations are channels-last per period and layer,
// [B][H p][C] with the flat row n = h p + c; EVERY batch row has the full length, tiles are counted from a batch row's own row 0 and every tap is masked by
// the row's own [0, H): a row's result does not depend on the batch around it, and nothing beyond the B H p rows is read or written.  What is kept are
// PRE-activations: the LeakyReLU is the consumer's prologue and its mask is recomputed from them in the backward.  Every matrix product runs on
// v_mfma_f32_16x16x4_f32 (`mfma4`), no float atomics, no kernel waits on another workgroup, every sum has a fixed partition and order: every output is
// bit-identical from run to run.
//
//   hifigan_disc_first      1 -> C0, 5 taps, stride s: one thread per (row, 4 channels); bias, then taps ascending on the VALU.  The reflect pad and the fold
//                           are index arithmetic of the read; no padded copy of the waveform exists.
//   hifigan_disc_conv       Cin -> Cout, 5 taps, stride s (3, or 1 for the last width): the generator's tile body `hg_tile` (hifigan_common.h) with its FOLDED
//                           row source, per tile of 64 flat output rows and RT NT 16 output columns (the generator's wave layouts, `hg_by_layout`).  In K
//                           chunks of 64 channels the tile stages lrelu(x) of the 64 rows of EVERY tap ([5][64] rows through `hd_source_row`: tap m of row
//                           (h', c) is input row (s h' + m - 2) p + c, zero outside [0, H); at stride 3 the five taps of 64 rows are hardly more than the
//                           span they cover, and one staging serves both strides), then runs tap by tap against the K-major image [5 Cin][Cout].  K loop,
//                           summation order and epilogue are the generator's text, not a copy of it: per (chunk, tap) a chain from zero, k ascending, added
//                           to the bias-initialised accumulator.  Any Cout that is a multiple of 16 (1024: 16 chunks, 8 column groups).
//   hifigan_disc_post       C -> 1, 3 taps, stride 1: one wave per row; a lane owns the channels 4 lane + 256 i (taps, then i ascending), `wave_sum`, + bias.
//   hifigan_disc_fm         mean |lrelu(f_real) - lrelu(f_fake)| of one feature map kept as [2 B][N][C] (real rows first): float64 block sums of 4096
//                           elements in a fixed tree order, and the gradient the frozen backward injects, sign(diff) lrelu'(f_fake) / count, laid out as the
//                           fake rows of the map.  `hifigan_disc_fm_sum`: the blocks in ascending order -> the mean, written and (optionally) added to a running
//                           total: L_fm is the sum of the terms in launch order, no other reduction.
//   hifigan_disc_post_bwd   d pre of the last width from d scores: per (row, 4 channels), taps ascending, times lrelu'(kept pre-activation), + injected.
//   hifigan_disc_conv_bwd   the data gradient of hifigan_disc_conv: `hg_tile<.., BWD, FOLD>`, the same body under the inverse row map: input row (h, c)
//                           receives tap m from output row ((h + 2 - m) / s) p + c when s divides h + 2 - m; the other taps stage zero rows.  Against the
//                           channel-transposed image [5 Cout][Cin] (row = tap Cout + output channel).  Epilogue: the generator's BWD epilogue with scale 1,
//                           y = sum * lrelu'(kept pre-activation) + injected * *inj_scale.
//   hifigan_disc_first_bwd  d wav: per sample t the transposed first layer at the padded positions t and (where it lies in [T, Tp)) 2 T - 2 - t, a gather;
//                           written, or added to what d wav holds (the periods add up in period order).
//   hifigan_disc_wgrad      the generator's weight-gradient kernel and launch sequence (hifigan_wgrad.h: `hw_launch`) with the same row map; +
//                           `hifigan_disc_wgrad_sum`.
// The multi-scale discriminator (hifigan_msd_ops.hip) runs its dense last layer and its conv_post on these kernels at period 1, where `hd_source_row` is a
// zero-padded convolution over time: the entry points glowtts_hifigan_msd_dense* / _post* at the end, launch-log classes `hifigan_msd_dense*` / `_post*`.
// Period 1 stays refused by the multi-period entry points.  The bf16 mode of the middle convolutions is hifigan_disc_bf16_ops.hip.
#include "hifigan_disc_common.h"
#include "hifigan_wgrad.h"

namespace {

constexpr int HD_FM_ELEMS = 4096;                          // elements of one block of the feature-matching sum

// grid (ceil(Ndst / 64), Cdst / (RT NT 16), B); src [B][Hsrc p][Csrc] -> out [B][Ndst][Cdst]; dynamic LDS [taps][64] rows of lds_stride_of(min(Csrc, 64)) floats.
// `hg_tile` in its folded mode.  Forward: src = the pre-activation of the layer below (slope_in: its LeakyReLU), w [taps Csrc][Cdst], out = bias + sum.  BWD:
// src = d pre of the layer's output (slope_in 1), w the transposed image, out = sum * lrelu'(mask) + inj * *inj_scale (mask, inj laid out as out; inj may be
// NULL): the generator's BWD epilogue with divisor 1 and nothing accumulated.
template <int RT, int NT, bool BWD>
__global__ __launch_bounds__(THREADS) void hifigan_disc_conv_kernel(const float* __restrict__ src, const float* __restrict__ w, const float* __restrict__ bias,
                                                                    const float* __restrict__ mask, const float* __restrict__ inj,
                                                                    const float* __restrict__ inj_scale, float* __restrict__ out, int Hsrc, int Ndst, int taps, int p,
                                                                    int s, int Csrc, int Cdst, float slope_in, float mslope)
{
    extern __shared__ __attribute__((aligned(16))) float hd_smem[];
    const size_t out0 = (size_t)blockIdx.z * Ndst * Cdst;
    const HgTaps tp = {taps, 0, 0, 0, 1, p, s};
    hg_tile<RT, NT, BWD, true>(src + (size_t)blockIdx.z * Hsrc * p * Csrc, w, bias, (BWD && inj) ? inj + out0 : nullptr, out + out0, hd_smem, Hsrc, Ndst, 0,
                               blockIdx.x * TM, Csrc, Cdst, blockIdx.y, tp, slope_in, 0, 1, 0, 0, 1.f, BWD ? mask + out0 : nullptr, mslope,
                               (BWD && inj) ? inj_scale[0] : 0.f);
}

// ---- first layer: grid (ceil(N1 C / 4 / 256), B).  w [5][C]: row = tap ----
__global__ __launch_bounds__(THREADS) void hifigan_disc_first_kernel(const float* __restrict__ wav, const float* __restrict__ w, const float* __restrict__ bias,
                                                                     float* __restrict__ out, int T, int H0, int N1, int p, int s, int C)
{
    const int b = blockIdx.y, c4n = C >> 2;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t n = e / c4n;
    if (n >= N1) return;
    const int c = (int)(e - n * c4n) * 4;
    const float* x = wav + (size_t)b * T;
    float4 acc = *reinterpret_cast<const float4*>(bias + c);
#pragma unroll
    for (int m = 0; m < HD_TAPS; ++m) {
        int from;
        if (!hd_source_row<false>((int)n, m, (HD_TAPS - 1) / 2, p, s, H0, &from)) continue;
        const float xv = hd_padded(x, from, T);
        const float4 wv = *reinterpret_cast<const float4*>(w + m * C + c);
        acc.x = fmaf(wv.x, xv, acc.x); acc.y = fmaf(wv.y, xv, acc.y); acc.z = fmaf(wv.z, xv, acc.z); acc.w = fmaf(wv.w, xv, acc.w);
    }
    *reinterpret_cast<float4*>(out + ((size_t)b * N1 + n) * C + c) = acc;
}

// ---- conv_post: grid (ceil(N / 4), B), one wave per row.  w [3][C]: row = tap ----
__global__ __launch_bounds__(THREADS) void hifigan_disc_post_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                    float* __restrict__ scores, int H, int p, int C, float slope)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63, n = blockIdx.x * WAVES + (threadIdx.x >> 6), N = H * p;
    if (n >= N) return;                                    // (uniform over the wave)
    const int h = n / p;
    const float* xb = x + (size_t)b * N * C;
    float acc = 0.f;
    for (int j = 0; j < HD_POST_TAPS; ++j) {
        const int hs = h + j - 1;
        if (hs < 0 || hs >= H) continue;
        const float* row = xb + (size_t)(n + (j - 1) * p) * C;
        for (int c = lane * 4; c < C; c += 256) {
            const float4 xv = *reinterpret_cast<const float4*>(row + c), wv = *reinterpret_cast<const float4*>(w + j * C + c);
            acc = fmaf(lrelu(xv.x, slope), wv.x, acc); acc = fmaf(lrelu(xv.y, slope), wv.y, acc);
            acc = fmaf(lrelu(xv.z, slope), wv.z, acc); acc = fmaf(lrelu(xv.w, slope), wv.w, acc);
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) scores[(size_t)b * N + n] = acc + bias[0];
}

// ---- feature matching: grid (ceil(count / 4096)); f [2 B][N][C] as 2 count floats, real first -> partial [blocks] float64, inj [count] ----
__global__ __launch_bounds__(THREADS) void hifigan_disc_fm_kernel(const float* __restrict__ f, float* __restrict__ inj, double* __restrict__ partial, int64_t count,
                                                                  float slope)
{
    __shared__ double red[THREADS];
    const int tid = threadIdx.x;
    const float inv = 1.f / (float)count;
    double sum = 0.0;
    for (int k = 0; k < HD_FM_ELEMS / THREADS; ++k) {
        const int64_t e = (int64_t)blockIdx.x * HD_FM_ELEMS + k * THREADS + tid;
        if (e >= count) break;
        const float fr = f[e], ff = f[count + e];
        const float diff = lrelu(ff, slope) - lrelu(fr, slope);
        inj[e] = (diff > 0.f ? inv : diff < 0.f ? -inv : 0.f) * (ff > 0.f ? 1.f : slope);
        sum += (double)fabsf(diff);
    }
    const double total = block_sum(sum, red, tid);
    if (tid == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(64) void hifigan_disc_fm_sum_kernel(const double* __restrict__ partial, float* __restrict__ term, float* __restrict__ total, int blocks, int64_t count,
                                                                 int accumulate)
{
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < blocks; ++k) s += partial[k];
    const float mean = (float)(s / (double)count);
    term[0] = mean;
    if (total) total[0] = accumulate ? total[0] + mean : mean;      // L_fm: the terms in launch order
}

// ---- conv_post, backward: grid (ceil(N C / 4 / 256), B): d pre[n][c] = lrelu'(x[n][c]) sum_j ds((h - (j - 1)) p + col) w[j][c] + inj ----
__global__ __launch_bounds__(THREADS) void hifigan_disc_post_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ dp2, const float* __restrict__ x,
                                                                        const float* __restrict__ w, const float* __restrict__ inj,
                                                                        const float* __restrict__ inj_scale, float* __restrict__ dx, int H, int p, int C, float slope)
{
    const int b = blockIdx.y, c4n = C >> 2, N = H * p;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t n = e / c4n;
    if (n >= N) return;
    const int c = (int)(e - n * c4n) * 4, h = (int)(n / p);
    const float isc = (inj || dp2) ? inj_scale[0] : 0.f;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < HD_POST_TAPS; ++j) {
        const int hs = h - (j - 1);
        if (hs < 0 || hs >= H) continue;
        const size_t at = (size_t)b * N + n - (j - 1) * p;
        float d = dp[at];
        if (dp2) d += dp2[at] * isc;
        const float4 wv = *reinterpret_cast<const float4*>(w + j * C + c);
        g.x = fmaf(wv.x, d, g.x); g.y = fmaf(wv.y, d, g.y); g.z = fmaf(wv.z, d, g.z); g.w = fmaf(wv.w, d, g.w);
    }
    const size_t idx = ((size_t)b * N + n) * C + c;
    const float4 xv = *reinterpret_cast<const float4*>(x + idx);
    g.x *= xv.x > 0.f ? 1.f : slope; g.y *= xv.y > 0.f ? 1.f : slope; g.z *= xv.z > 0.f ? 1.f : slope; g.w *= xv.w > 0.f ? 1.f : slope;
    if (inj) {
        const float4 iv = *reinterpret_cast<const float4*>(inj + idx);
        g.x += iv.x * isc; g.y += iv.y * isc; g.z += iv.z * isc; g.w += iv.w * isc;
    }
    *reinterpret_cast<float4*>(dx + idx) = g;
}

// d(padded wav) at the padded position n: the taps ascending, each a chain over the channels
__device__ __forceinline__ float hd_dpad(const float* __restrict__ dpre, const float* __restrict__ w, int n, int H1, int p, int s, int C)
{
    float sum = 0.f;
    for (int m = 0; m < HD_TAPS; ++m) {
        int from;
        if (!hd_source_row<true>(n, m, (HD_TAPS - 1) / 2, p, s, H1, &from)) continue;
        const float* g = dpre + (size_t)from * C;
        float t = 0.f;
        for (int c = 0; c < C; c += 4) {
            const float4 gv = *reinterpret_cast<const float4*>(g + c), wv = *reinterpret_cast<const float4*>(w + m * C + c);
            t = fmaf(gv.x, wv.x, t); t = fmaf(gv.y, wv.y, t); t = fmaf(gv.z, wv.z, t); t = fmaf(gv.w, wv.w, t);
        }
        sum += t;
    }
    return sum;
}

// ---- first layer, backward: grid (ceil(T / 256), B).  dpre [B][H1 p][C]; w [5][C] ----
__global__ __launch_bounds__(THREADS) void hifigan_disc_first_bwd_kernel(const float* __restrict__ dpre, const float* __restrict__ w, float* __restrict__ dwav, int T,
                                                                         int H0, int H1, int p, int s, int C, int accumulate)
{
    const int b = blockIdx.y, t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const float* db = dpre + (size_t)b * H1 * p * C;
    float g = hd_dpad(db, w, t, H1, p, s, C);
    const int mirror = 2 * T - 2 - t;                      // the padded sample that is a copy of sample t, if any
    if (mirror >= T && mirror < H0 * p) g += hd_dpad(db, w, mirror, H1, p, s, C);
    dwav[(size_t)b * T + t] = accumulate ? dwav[(size_t)b * T + t] + g : g;
}

// ---- host side ----
// (the limits and the argument checks: hifigan_disc_common.h)
int hd_lds_bytes(int Csrc) { return hg_lds_bytes((HD_TAPS - 1) * TM, Csrc); }         // [5][64] rows
unsigned hd_quads(int64_t rows, int C) { return (unsigned)((rows * (C / 4) + THREADS - 1) / THREADS); }

// hifigan_disc_conv in either direction
template <bool BWD>
int hd_conv(const float* src, const float* w, const float* bias, const float* mask, const float* inj, const float* inj_scale, float* out, int B, int Hsrc, int Ndst,
            int p, int s, int Csrc, int Cdst, float slope_in, float mslope, void* stream)
{
    return hg_by_layout(Cdst, [&](auto rt, auto nt) {
        constexpr int RT = decltype(rt)::value, NT = decltype(nt)::value;
        return hg_launch<&hifigan_disc_conv_kernel<RT, NT, BWD>>(dim3((Ndst + TM - 1) / TM, Cdst / (RT * NT * 16), B), hd_lds_bytes(Csrc),
                                                                 static_cast<hipStream_t>(stream), src, w, bias, mask, inj, inj_scale, out, Hsrc, Ndst, HD_TAPS, p, s,
                                                                 Csrc, Cdst, slope_in, mslope);
    });
}

}  // namespace

extern "C" int glowtts_hifigan_disc_supported(int period, int Cin, int Cout)
{
    return hd_period(period) && (Cin == 1 || hd_width(Cin)) && (Cout == 1 || hd_width(Cout)) && !(Cin == 1 && Cout == 1) && hd_lds_bytes(Cin) <= MAX_LDS;
}

extern "C" int64_t glowtts_hifigan_disc_work_floats(int B, int rows_out, int Cin, int Cout, int taps)
{
    if (B < 1 || B > 65535 || rows_out < 1 || Cin < 1 || Cin > HD_MAX_CHANNELS || Cout < 1 || Cout > HD_MAX_CHANNELS || (taps != HD_TAPS && taps != HD_POST_TAPS)) return 0;
    const int64_t fm = 2 * (((int64_t)B * rows_out * Cout + HD_FM_ELEMS - 1) / HD_FM_ELEMS);       // float64 block sums of a feature map of B rows
    return std::max(hw_sizes(B, rows_out, Cin, Cout, taps).floats, fm);
}

extern "C" int glowtts_hifigan_disc_first(const float* wav, const float* w, const float* bias, float* out, int B, int T, int period, int stride, int C, void* stream)
{
    if (!wav || !w || !bias || !out || !hd_period(period) || T < 2 * period || !hd_stride(stride) || !hd_width(C)) return GLOWTTS_E_ARG;
    const int H0 = (T + period - 1) / period, H1 = hd_rows_out(H0, stride);
    if (hd_bad_rows(B, H0, period)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("hifigan_disc_first");
    hipLaunchKernelGGL(hifigan_disc_first_kernel, dim3(hd_quads((int64_t)H1 * period, C), B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), wav, w, bias, out, T,
                       H0, H1 * period, period, stride, C);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_disc_conv(const float* x, const float* w, const float* bias, float* out, int B, int H, int period, int stride, int Cin, int Cout,
                                         float slope, void* stream)
{
    if (!x || !w || !bias || !out || x == out || hd_bad_rows(B, H, period) || !hd_stride(stride) || !hd_width(Cin) || !hd_width(Cout)) return GLOWTTS_E_ARG;
    if (hd_conv<false>(x, w, bias, nullptr, nullptr, nullptr, out, B, H, hd_rows_out(H, stride) * period, period, stride, Cin, Cout, slope, 1.f, stream) != GLOWTTS_OK)
        return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_disc_conv");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_disc_post(const float* x, const float* w, const float* bias, float* scores, int B, int H, int period, int C, float slope, void* stream)
{
    if (!x || !w || !bias || !scores || hd_bad_rows(B, H, period) || !hd_width(C)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("hifigan_disc_post");
    hipLaunchKernelGGL(hifigan_disc_post_kernel, dim3((H * period + WAVES - 1) / WAVES, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), x, w, bias, scores, H,
                       period, C, slope);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_disc_fm(const float* f, float* inj, float* work, float* term, float* total, int64_t count, float slope, int accumulate,
                                       void* stream)
{
    if (!f || !inj || !work || !term || accumulate < 0 || accumulate > 1 || count < 1 || count >= ((int64_t)1 << 30) || (reinterpret_cast<uintptr_t>(work) & 7)) return GLOWTTS_E_ARG;
    const int blocks = (int)((count + HD_FM_ELEMS - 1) / HD_FM_ELEMS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLOWTTS_NOTE_STATIC("hifigan_disc_fm");
    hipLaunchKernelGGL(hifigan_disc_fm_kernel, dim3(blocks), dim3(THREADS), 0, st, f, inj, reinterpret_cast<double*>(work), count, slope);
    GLOWTTS_NOTE_STATIC("hifigan_disc_fm_sum");
    hipLaunchKernelGGL(hifigan_disc_fm_sum_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const double*>(work), term, total, blocks, count, accumulate);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_disc_post_bwd(const float* dscores, const float* dscores2, const float* x, const float* w, const float* inj, const float* inj_scale,
                                             float* dx, int B, int H, int period, int C, float slope, void* stream)
{
    if (!dscores || !x || !w || !dx || dx == x || ((inj || dscores2) && !inj_scale) || hd_bad_rows(B, H, period) || !hd_width(C)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("hifigan_disc_post_bwd");
    hipLaunchKernelGGL(hifigan_disc_post_bwd_kernel, dim3(hd_quads((int64_t)H * period, C), B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), dscores, dscores2, x,
                       w, inj, inj_scale, dx, H, period, C, slope);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_disc_conv_bwd(const float* dy, const float* wt, const float* x, const float* inj, const float* inj_scale, float* dx, int B, int H,
                                             int period, int stride, int Cin, int Cout, float slope, void* stream)
{
    if (!dy || !wt || !x || !dx || dx == dy || dx == x || (inj && !inj_scale) || hd_bad_rows(B, H, period) || !hd_stride(stride) || !hd_width(Cin) || !hd_width(Cout))
        return GLOWTTS_E_ARG;
    if (hd_conv<true>(dy, wt, nullptr, x, inj, inj_scale, dx, B, hd_rows_out(H, stride), H * period, period, stride, Cout, Cin, 1.f, slope, stream) != GLOWTTS_OK)
        return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_disc_conv_bwd");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_disc_first_bwd(const float* dpre, const float* w, float* dwav, int B, int T, int period, int stride, int C, int accumulate,
                                              void* stream)
{
    if (!dpre || !w || !dwav || accumulate < 0 || accumulate > 1 || !hd_period(period) || T < 2 * period || !hd_stride(stride) || !hd_width(C)) return GLOWTTS_E_ARG;
    const int H0 = (T + period - 1) / period;
    if (hd_bad_rows(B, H0, period)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("hifigan_disc_first_bwd");
    hipLaunchKernelGGL(hifigan_disc_first_bwd_kernel, dim3((T + THREADS - 1) / THREADS, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), dpre, w, dwav, T, H0,
                       hd_rows_out(H0, stride), period, stride, C, accumulate);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_disc_wgrad(const float* x, const float* dy, float* work, float* dw, float* dbias, int B, int H, int period, int stride, int Cin, int Cout,
                                          int taps, int wav_samples, float slope, void* stream)
{
    if (!x || !dy || !work || !dw || !dbias || hd_bad_rows(B, H, period) || !hd_stride(stride) || !glowtts_hifigan_disc_supported(period, Cin, Cout) ||
        (taps != HD_TAPS && taps != HD_POST_TAPS) || (taps == HD_POST_TAPS && stride != 1) || wav_samples < 0 || (wav_samples > 0 && Cin != 1) ||
        (wav_samples == 0 && Cin == 1) || (wav_samples > 0 && (wav_samples < 2 * period || (wav_samples + period - 1) / period != H)))
        return GLOWTTS_E_ARG;
    const HwArgs a = {x, dy, nullptr, work, B, hd_rows_out(H, stride) * period, 1, Cin, Cout, taps, 0, 0, 0, 0, 0, slope, period, stride, H, wav_samples};
    return hw_launch<true>(a, dw, dbias, 0, taps, 1.f, static_cast<hipStream_t>(stream));
}

// ---- the multi-scale discriminator's dense layers: the kernels above at period 1 (activations [B][L][C], stride 1) ----
namespace {
bool hd_bad_length(int B, int L) { return B < 1 || B > 65535 || L < 1 || (int64_t)B * L > ((int64_t)1 << 30); }
}  // namespace

extern "C" int glowtts_hifigan_msd_dense(const float* x, const float* w, const float* bias, float* out, int B, int L, int Cin, int Cout, float slope, void* stream)
{
    if (!x || !w || !bias || !out || x == out || hd_bad_length(B, L) || !hd_width(Cin) || !hd_width(Cout) || hd_lds_bytes(Cin) > MAX_LDS) return GLOWTTS_E_ARG;
    if (hd_conv<false>(x, w, bias, nullptr, nullptr, nullptr, out, B, L, L, 1, 1, Cin, Cout, slope, 1.f, stream) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_msd_dense");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_dense_bwd(const float* dy, const float* wt, const float* x, const float* inj, const float* inj_scale, float* dx, int B, int L,
                                             int Cin, int Cout, float slope, void* stream)
{
    if (!dy || !wt || !x || !dx || dx == dy || dx == x || (inj && !inj_scale) || hd_bad_length(B, L) || !hd_width(Cin) || !hd_width(Cout) ||
        hd_lds_bytes(Cout) > MAX_LDS)
        return GLOWTTS_E_ARG;
    if (hd_conv<true>(dy, wt, nullptr, x, inj, inj_scale, dx, B, L, L, 1, 1, Cout, Cin, 1.f, slope, stream) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_msd_dense_bwd");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_post(const float* x, const float* w, const float* bias, float* scores, int B, int L, int C, float slope, void* stream)
{
    if (!x || !w || !bias || !scores || hd_bad_length(B, L) || !hd_width(C)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("hifigan_msd_post");
    hipLaunchKernelGGL(hifigan_disc_post_kernel, dim3((L + WAVES - 1) / WAVES, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), x, w, bias, scores, L, 1, C,
                       slope);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_post_bwd(const float* dscores, const float* dscores2, const float* x, const float* w, const float* inj, const float* inj_scale,
                                            float* dx, int B, int L, int C, float slope, void* stream)
{
    if (!dscores || !x || !w || !dx || dx == x || ((inj || dscores2) && !inj_scale) || hd_bad_length(B, L) || !hd_width(C)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("hifigan_msd_post_bwd");
    hipLaunchKernelGGL(hifigan_disc_post_bwd_kernel, dim3(hd_quads(L, C), B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), dscores, dscores2, x, w, inj,
                       inj_scale, dx, L, 1, C, slope);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_dense_wgrad(const float* x, const float* dy, float* work, float* dw, float* dbias, int B, int L, int Cin, int Cout, int taps,
                                               float slope, void* stream)
{
    if (!x || !dy || !work || !dw || !dbias || hd_bad_length(B, L) || !hd_width(Cin) || !(Cout == 1 || hd_width(Cout)) ||
        !((taps == HD_TAPS && Cout != 1) || (taps == HD_POST_TAPS && Cout == 1)))
        return GLOWTTS_E_ARG;
    const HwArgs a = {x, dy, nullptr, work, B, L, 1, Cin, Cout, taps, 0, 0, 0, 0, 0, slope, 1, 1, L, 0};
    return hw_launch<true, true>(a, dw, dbias, 0, taps, 1.f, static_cast<hipStream_t>(stream));
}
