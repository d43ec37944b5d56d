// Training the HiFi-GAN generator: the backward of csrc/hifigan_ops.hip for gfx950, f32.  Layouts, lengths and ownership are the forward's: rows are samples,
// channels-last, an utterance owns rows [0, T_b) of its slab, nothing is read beyond them and nothing is written there.  Every matrix product runs on
// v_mfma_f32_16x16x4_f32, every sum has one fixed order that depends on the sizes alone, no float atomics, no workgroup waits on another: every gradient is
// bit-identical from run to run.
//
//   hifigan_conv_bwd      the data gradient of one dilated convolution, ONE launch: the convolution of dy with the tap-reversed, channel-transposed image
//                         wt [taps Cout][Cin] (row = (taps - 1 - tap) Cout + output channel) on the forward's tile body (`hg_tile<.., BWD>`: LDS staging, zero
//                         outside [0, T_b), chunked summation, sums from zero).  Epilogue: y = sum * lrelu'(x) * scale (x: the kept input of the forward's
//                         LeakyReLU; 1 where x > 0, the slope elsewhere, at x == 0 as well) + residual * res_scale (the skip branch's gradient, may be `out`),
//                         then out = y or out = out + y (the nk blocks of a stage add their input gradients into dU in block order).  The 1 / nk of the MRF mean
//                         is `scale` / `res_scale` of the launches that read d acc.  The discriminator's data gradient (hifigan_disc_ops.hip) is this body
//                         and this epilogue too, with its rows staged through the period-folded row map in place of the contiguous span.
//   hifigan_upsample_bwd  the data gradient of the transposed convolution, ONE launch on the same kernel: dy [T u][Cout] IS [T][u Cout] in memory, so
//                         dx[s] = sum over row offsets e in [lo, hi] of Wt_e^T dyview[s + e] is an ordinary few-tap convolution over rows with u Cout input
//                         channels, against an image [(hi - lo + 1) u Cout][Cin] that holds zeros where a (phase, offset) pair has no tap.
//   hifigan_post_bwd      d pre = d wav (1 - wav^2) (kept for the weight gradient); d rows = lrelu'(rows) * sum over the taps of w d pre, a fixed-order fmaf chain.
//   hifigan_wgrad         dW[tap][ci][co] = sum over the utterances' rows of lrelu(x)[t + offset(tap)][ci] dy[t][co] and the bias gradient (column sums of dy, added in double).
//                         A workgroup owns 32 x 32 (ci, co) of EVERY tap over one split of the rows: it stages 64 rows of lrelu(x) (with the taps' reach) and
//                         of dy in LDS once and takes every tap from that one tile - the tap only shifts the row index - so both MFMA operands are reads of 16
//                         consecutive channels of one row (row stride 48 floats: the four rows of a k step fall on distinct banks).  A wave owns one 16 x 16
//                         tile per tap (taps x 4 accumulators).  The partition is fixed: per utterance, chunks of 1024 rows; a split is `group` consecutive
//                         (utterance, chunk) units, walked in ascending order (group = 1024 / rows of a slab when that is below 1024, else 1).  The transposed
//                         convolution uses the same kernel on the [T][u Cout] view: tap = row offset, column = (phase, output channel).
//   hifigan_wgrad_sum     adds the splits in ascending order, scales, writes torch's layout (Conv1d [Cout][Cin][taps], ConvTranspose1d [Cin][Cout][k]; the view's
//                         (offset, phase) pairs without a tap are dropped, the bias adds the phases in ascending order).
#include "hifigan_common.h"
#include "hifigan_wgrad.h"                             // hifigan_wgrad_kernel, hifigan_wgrad_sum_kernel and the partition: shared with hifigan_disc_ops.hip

namespace {

constexpr int HB_MAX_VIEW = 4096;                          // u Cout of the transposed convolution's view

// The row offsets e = m - o0(ph) of the transposed convolution (k taps, rate u) in the [T][u Cout] view: [lo, hi]
void hg_up_reach(int k, int u, int* lo, int* hi)
{
    *lo = 1 << 20; *hi = -(1 << 20);
    for (int ph = 0; ph < u; ++ph) {
        const int shift = ph + (k - u) / 2, j0 = shift % u, o0 = shift / u, nt = (k - j0 + u - 1) / u;
        *lo = std::min(*lo, -o0);
        *hi = std::max(*hi, nt - 1 - o0);
    }
}

// grid (ceil(Lmax mult / 64), Cdx / (RT NT 16), B); dy [B][Lmax mult][Cdy] -> out [B][Lmax mult][Cdx];  dynamic LDS (64 + (taps - 1) |ts|) rows
template <int RT, int NT>
__global__ __launch_bounds__(THREADS) void hifigan_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ wt, const float* __restrict__ x,
                                                              const float* res, float* out, const int32_t* __restrict__ lengths, int Lmax, int mult, int Cdy,
                                                              int Cdx, int taps, int o0, int ts, float mslope, float scale, float res_scale, int accumulate)
{
    extern __shared__ __attribute__((aligned(16))) float hg_smem[];
    const int b = blockIdx.z, s0 = blockIdx.x * TM;
    const int Tmax = Lmax * mult, T = min(lengths[b], Lmax) * mult;
    if (s0 >= T) return;                                   // (uniform over the workgroup)
    const size_t row0 = (size_t)b * Tmax;
    const HgTaps tp = {taps, o0, ts, 0, 1};
    hg_tile<RT, NT, true>(dy + row0 * Cdy, wt, nullptr, res ? res + row0 * Cdx : nullptr, out + row0 * Cdx, hg_smem, T, T, Tmax, s0, Cdy, Cdx, blockIdx.y, tp, 1.f, 0,
                          1, 0, accumulate, scale, x + row0 * Cdx, mslope, res_scale);
}

// grid (ceil(Lmax mult Cin / 4 / 256), B): a thread owns four channels of one row
__global__ __launch_bounds__(THREADS) void hifigan_post_bwd_kernel(const float* __restrict__ dwav, const float* __restrict__ wav, const float* __restrict__ x,
                                                                   const float* __restrict__ w, float* __restrict__ dpre, float* __restrict__ dx,
                                                                   const int32_t* __restrict__ lengths, int Lmax, int mult, int Cin, int taps, float slope)
{
    const int b = blockIdx.y, cq = Cin >> 2;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int Tmax = Lmax * mult, T = min(lengths[b], Lmax) * mult;
    const int s = (int)(e / cq), c = (int)(e - (int64_t)s * cq) * 4;
    if (s >= T) return;                                    // rows beyond the utterance are never written
    const size_t row0 = (size_t)b * Tmax;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < taps; ++j) {                       // row s fed output t = s - (j - (taps - 1) / 2) through tap j
        const int t = s - j + (taps - 1) / 2;
        if (t < 0 || t >= T) continue;
        const float y = wav[row0 + t], d = dwav[row0 + t] * (1.f - y * y);
        const float4 wv = *reinterpret_cast<const float4*>(w + j * Cin + c);
        g.x = fmaf(wv.x, d, g.x); g.y = fmaf(wv.y, d, g.y); g.z = fmaf(wv.z, d, g.z); g.w = fmaf(wv.w, d, g.w);
    }
    const float4 xv = *reinterpret_cast<const float4*>(x + (row0 + s) * Cin + c);
    g.x *= xv.x > 0.f ? 1.f : slope; g.y *= xv.y > 0.f ? 1.f : slope; g.z *= xv.z > 0.f ? 1.f : slope; g.w *= xv.w > 0.f ? 1.f : slope;
    *reinterpret_cast<float4*>(dx + (row0 + s) * Cin + c) = g;
    if (c == 0) {
        const float y = wav[row0 + s];
        dpre[row0 + s] = dwav[row0 + s] * (1.f - y * y);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
// the weight gradient's walk of a convolution (rate 0) or of a transposed convolution's view: taps, first offset, step, columns of dy
bool hw_walk(int Cd, int taps, int dilation, int rate, int* wt, int* o0, int* ts, int* cd)
{
    if (rate == 0) {
        *wt = taps; *o0 = -((taps - 1) / 2) * dilation; *ts = dilation; *cd = Cd;
    } else {
        int lo, hi;
        hg_up_reach(taps, rate, &lo, &hi);
        *wt = hi - lo + 1; *o0 = -hi; *ts = 1; *cd = rate * Cd;
    }
    return *wt >= 1 && *wt <= HW_MAX_TAPS;
}

// both data gradients: `taps` row offsets from o0 in steps of ts over Cdy channels of dy
int hb_data_gradient(const float* dy, const float* wt, const float* x, const float* res, float* out, const int32_t* lengths, int B, int Lmax, int mult, int Cdy,
                     int Cdx, int taps, int o0, int ts, float mslope, float scale, float res_scale, int accumulate, void* stream)
{
    return hg_by_layout(Cdx, [&](auto rt, auto nt) {
        constexpr int RT = decltype(rt)::value, NT = decltype(nt)::value;
        return hg_launch<&hifigan_bwd_kernel<RT, NT>>(dim3((Lmax * mult + TM - 1) / TM, Cdx / (RT * NT * 16), B), hg_lds_bytes((taps - 1) * ts, Cdy),
                                                      static_cast<hipStream_t>(stream), dy, wt, x, res, out, lengths, Lmax, mult, Cdy, Cdx, taps, o0, ts, mslope,
                                                      scale, res_scale, accumulate);
    });
}

}  // namespace

extern "C" int glowtts_hifigan_train_supported(int Cin, int Cout, int taps, int dilation, int rate)
{
    if (!glowtts_hifigan_supported(Cin, Cout, taps, dilation, rate)) return 0;
    int wt, o0, ts, cd;
    if (!hw_walk(Cout, taps, dilation, rate, &wt, &o0, &ts, &cd)) return 0;
    if (rate == 0) return Cout == 1 || hg_lds_bytes((taps - 1) * dilation, Cout) <= MAX_LDS;      // (the data gradient also needs Cin % 16 == 0: conv_pre has none)
    return Cin % 16 == 0 && cd <= HB_MAX_VIEW && hg_lds_bytes(wt - 1, cd) <= MAX_LDS;
}

extern "C" int64_t glowtts_hifigan_wgrad_work_floats(int B, int Lmax, int mult, int Cin, int Cout, int taps, int rate)
{
    int wt, o0, ts, cd;
    if (bad_batch(B, Lmax, mult) || Cin < 1 || Cout < 1 || rate < 0 || rate > HG_MAX_RATE || taps < 1 || !hw_walk(Cout, taps, 1, rate, &wt, &o0, &ts, &cd)) return 0;
    return hw_sizes(B, Lmax * mult, Cin, cd, wt).floats;
}

extern "C" int glowtts_hifigan_conv_bwd(const float* dy, const float* wt, const float* x, const float* residual, float* out, const int32_t* frame_lengths, int B,
                                        int Lmax, int mult, int Cin, int Cout, int taps, int dilation, float mask_slope, float scale, float res_scale,
                                        int accumulate, void* stream)
{
    if (!dy || !wt || !x || !out || !frame_lengths || dy == out || bad_batch(B, Lmax, mult) || Cout == 1 || Cin % 16 ||
        !glowtts_hifigan_train_supported(Cin, Cout, taps, dilation, 0) || accumulate < 0 || accumulate > 1)
        return GLOWTTS_E_ARG;
    if (hb_data_gradient(dy, wt, x, residual, out, frame_lengths, B, Lmax, mult, Cout, Cin, taps, -((taps - 1) / 2) * dilation, dilation, mask_slope, scale, res_scale,
                         accumulate, stream) != GLOWTTS_OK)
        return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_conv_bwd");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_upsample_bwd(const float* dy, const float* wt, const float* x, float* out, const int32_t* frame_lengths, int B, int Lmax, int mult,
                                            int Cin, int Cout, int taps, int rate, float mask_slope, void* stream)
{
    if (!dy || !wt || !x || !out || !frame_lengths || dy == out || rate < 1 || rate > HG_MAX_RATE || bad_batch(B, Lmax, mult) || (int64_t)mult * rate > (1 << 16) ||
        bad_batch(B, Lmax, mult * rate) || !glowtts_hifigan_train_supported(Cin, Cout, taps, 1, rate))
        return GLOWTTS_E_ARG;
    int lo, hi;
    hg_up_reach(taps, rate, &lo, &hi);
    if (hb_data_gradient(dy, wt, x, nullptr, out, frame_lengths, B, Lmax, mult, rate * Cout, Cin, hi - lo + 1, lo, 1, mask_slope, 1.f, 1.f, 0, stream) != GLOWTTS_OK)
        return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_upsample_bwd");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_post_bwd(const float* dwav, const float* wav, const float* x, const float* w, float* dpre, float* dx, const int32_t* frame_lengths,
                                        int B, int Lmax, int mult, int Cin, int taps, float slope, void* stream)
{
    if (!dwav || !wav || !x || !w || !dpre || !dx || !frame_lengths || bad_batch(B, Lmax, mult) || !glowtts_hifigan_supported(Cin, 1, taps, 1, 0)) return GLOWTTS_E_ARG;
    const int64_t threads = (int64_t)Lmax * mult * (Cin / 4);
    hipLaunchKernelGGL(hifigan_post_bwd_kernel, dim3((unsigned)((threads + THREADS - 1) / THREADS), B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), dwav, wav, x,
                       w, dpre, dx, frame_lengths, Lmax, mult, Cin, taps, slope);
    GLOWTTS_NOTE_STATIC("hifigan_post_bwd");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_wgrad(const float* x, const float* dy, const int32_t* frame_lengths, float* work, float* dw, float* dbias, int B, int Lmax, int mult,
                                     int Cin, int Cout, int taps, int dilation, int rate, float slope, float scale, int channels_first, void* stream)
{
    int wt, o0, ts, cd;
    if (!x || !dy || !frame_lengths || !work || !dw || !dbias || bad_batch(B, Lmax, mult) || !glowtts_hifigan_train_supported(Cin, Cout, taps, dilation, rate) ||
        (channels_first && rate) || !hw_walk(Cout, taps, dilation, rate, &wt, &o0, &ts, &cd))
        return GLOWTTS_E_ARG;
    const HwArgs a = {x, dy, frame_lengths, work, B, Lmax, mult, Cin, cd, wt, o0, ts, channels_first, 0, 0, slope};
    return hw_launch<false>(a, dw, dbias, rate, taps, scale, static_cast<hipStream_t>(stream));
}
