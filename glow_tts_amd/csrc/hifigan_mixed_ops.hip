// Training the HiFi-GAN generator in mixed precision (DESIGN.md "Training the HiFi-GAN generator: mixed precision" has the contract).  The forward of the mode
// IS the fp16 inference forward (hifigan_f16_ops.hip); this file holds the backward's matrix products on v_mfma_f32_16x16x32_bf16 and the launch that builds
// every 16-bit weight image of a step.  Master weights, every tensor in memory, every sum and every epilogue stay fp32; conv_post's launches stay f32
// (hifigan_train_ops.hip).  No float atomics, one summation order that depends on the sizes alone: every gradient is bit-identical from run to run.
//
//   hifigan_conv_bwd_bf16      `hifigan_conv_bwd` on `hf_tile<.., HfBf16, BWD>` (hifigan_f16_tile.h): the staged rows of dy - as they lie in memory, before any
//                              scale - and the tap-reversed, channel-transposed image are bf16 (nearest even, no clamp), the sums fp32 from zero in the f32
//                              kernel's chunk and tap order, the epilogue the f32 kernel's: * lrelu'(x) * scale + residual * res_scale, then accumulate.
//   hifigan_upsample_bwd_bf16  the same kernel over dy read as [T][u Cout] against the view's image with its zero rows.
//   hifigan_wgrad_bf16         (the kernel is hifigan_wgrad_bf16.h's, shared with the discriminator's bf16 mode)  dW[tap][ci][co] = sum over rows of bf16(lrelu(x)[t + off(tap)][ci]) bf16(dy[t][co]), fp32 sums, on the f32 kernel's fixed partition
//                              and 32 x 32 workgroup tile, so `hw_sizes`, the partial layout [splits][taps CiP CoP + CoP] and `hifigan_wgrad_sum` serve both
//                              modes.  K is the ROW index, so a lane needs 8 consecutive rows of one channel: the tile stages lrelu(x) (with the taps' reach)
//                              and dy as bf16 ROW-major [row][32 channels] (row stride 80 bytes: a multiple of 8, odd in 16-byte slots) and reads both MFMA
//                              operands with the transposed LDS read ds_read_tr16_b64 - two reads of 4 rows x 16 channels per operand.  A tap is a row
//                              offset, so every address stays 8-byte aligned at any dilation.  The instruction needs EXEC all ones: every loop around it
//                              is uniform over the workgroup and nothing returns before it.  Each 64-row tile is one chain from zero (two MFMAs per tap);
//                              tiles, then splits, are added in ascending order.  The bias gradient is the column sum of the UNROUNDED fp32 dy, in double:
//                              each staging thread sums its own four columns, 32 row groups are added in ascending order at the end.
//   hifigan_pack_images        ONE launch builds every weight image of a step from the fp32 master weights through a device job table (built once by the
//                              caller): the fp16 forward images (conv / transposed conv: `vocoder.hifigan_pack_f16`'s bytes), the bf16 data-gradient images
//                              (tap-reversed and channel-transposed; the transposed convolution's view with its zero fill) and conv_post's f32 [taps][Cin]
//                              rows.  A thread writes one 16-byte group (eight k of one column).  Two more kinds serve the multi-period discriminator's
//                              bf16 mode (hifigan_disc_bf16_ops.hip): a Conv weight's bf16 forward image and its channel-transposed image WITHOUT the
//                              tap reversal (the discriminator's inverse row map reverses the taps).
#include "hifigan_f16_tile.h"
#include "hifigan_wgrad_bf16.h"

namespace {

constexpr int HM_MAX_VIEW = 4096;                          // u Cout of the transposed convolution's view (hifigan_train_ops.hip's limit)

// the row offsets of the transposed convolution in the [T][u Cout] view: [lo, hi] (hifigan_train_ops.hip's hg_up_reach)
__host__ __device__ __forceinline__ void hm_up_reach(int k, int u, int* lo, int* hi)
{
    *lo = 1 << 20; *hi = -(1 << 20);
    for (int ph = 0; ph < u; ++ph) {
        const int shift = ph + (k - u) / 2, j0 = shift % u, o0 = shift / u, nt = (k - j0 + u - 1) / u;
        *lo = -o0 < *lo ? -o0 : *lo;
        *hi = nt - 1 - o0 > *hi ? nt - 1 - o0 : *hi;
    }
}

// grid (ceil(Lmax mult / 64), Cdx / (RT NT 16), B); dy [B][Lmax mult][Cdy] -> out [B][Lmax mult][Cdx];  dynamic LDS (64 + (taps - 1) |ts|) rows
template <int RT, int NT>
__global__ __launch_bounds__(THREADS) void hifigan_bwd_bf16_kernel(const float* __restrict__ dy, const uint16_t* __restrict__ wt, const float* __restrict__ x,
                                                                   const float* res, float* out, const int32_t* __restrict__ lengths, int Lmax, int mult, int Cdy,
                                                                   int Cdx, int taps, int o0, int ts, float mslope, float scale, float res_scale, int accumulate)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t hm_smem[];
    const int b = blockIdx.z, s0 = blockIdx.x * TM;
    const int Tmax = Lmax * mult, T = min(lengths[b], Lmax) * mult;
    if (s0 >= T) return;                                   // (uniform over the workgroup)
    const size_t row0 = (size_t)b * Tmax;
    const HgTaps tp = {taps, o0, ts, 0, 1};
    hf_tile<RT, NT, HfBf16, true>(dy + row0 * Cdy, wt, nullptr, res ? res + row0 * Cdx : nullptr, out + row0 * Cdx, hm_smem, T, Tmax, s0, Cdy, Cdx, blockIdx.y, tp,
                                  1.f, 0, 1, 0, accumulate, scale, x + row0 * Cdx, mslope, res_scale);
}

// ---- hifigan_pack_images ----
// A job is HP_WORDS int64: source (fp32 master weight), destination, kind, Cin, Cout, taps, rate, first block.  Cin, Cout, taps, rate name the FORWARD
// convolution.  Kinds 0 - 3 write [T'][Kp / 8][N][8] 16-bit images, element (tap t', k, n) with zeros for k from K to Kp = pad32(K):
//   0  fp16, Conv1d [Cout][Cin][taps]:           T' = taps, K = Cin, N = Cout, W[n][k][t']
//   1  fp16, ConvTranspose1d [Cin][Cout][taps]:  T' = taps, K = Cin, N = Cout, W[k][n][t']
//   2  bf16, the data gradient of 0:             T' = taps, K = Cout, N = Cin, W[k][n][taps - 1 - t']
//   3  bf16, the data gradient of 1 in the view: T' = hi - lo + 1, K = rate Cout (k = (phase, output channel)), N = Cin, W[n][co][tap of (lo + t', phase)] or zero
//   4  f32, conv_post [1][Cin][taps] -> [taps][Cin]
//   5  bf16, Conv [Cout][Cin][taps] (kind 0 in bf16): T' = taps, K = Cin, N = Cout, W[n][k][t']
//   6  bf16, the channel-transposed image of 5:  T' = taps, K = Cout, N = Cin, W[k][n][t'] (kind 2 without the tap reversal)
constexpr int HP_WORDS = 8;
enum { HP_CONV_F16 = 0, HP_UP_F16 = 1, HP_CONV_T_BF16 = 2, HP_UP_T_BF16 = 3, HP_POST_F32 = 4, HP_CONV_BF16 = 5, HP_CONV_KT_BF16 = 6 };

__global__ __launch_bounds__(THREADS) void hifigan_pack_images_kernel(const int64_t* __restrict__ jobs, int njobs)
{
    int jl = 0, jh = njobs - 1;
    while (jl < jh) {
        const int mid = (jl + jh + 1) >> 1;
        if (jobs[mid * HP_WORDS + 7] <= (int64_t)blockIdx.x) jl = mid; else jh = mid - 1;
    }
    const int64_t* j = jobs + (size_t)jl * HP_WORDS;
    const float* __restrict__ src = reinterpret_cast<const float*>(j[0]);
    const int kind = (int)j[2], Cin = (int)j[3], Cout = (int)j[4], taps = (int)j[5], rate = (int)j[6];
    const int64_t g = (int64_t)(blockIdx.x - j[7]) * THREADS + threadIdx.x;
    if (kind == HP_POST_F32) {
        if (g >= (int64_t)taps * Cin) return;
        const int t = (int)(g / Cin), c = (int)(g - (int64_t)t * Cin);
        reinterpret_cast<float*>(j[1])[g] = src[(size_t)c * taps + t];
        return;
    }
    int lo = 0, hi = taps - 1;
    if (kind == HP_UP_T_BF16) hm_up_reach(taps, rate, &lo, &hi);
    const int Tw = hi - lo + 1;
    const bool fwd = kind <= HP_UP_F16 || kind == HP_CONV_BF16;    // K = the forward's input channels
    const int K = fwd ? Cin : (kind == HP_UP_T_BF16 ? rate * Cout : Cout), N = fwd ? Cout : Cin, K8 = hf_pad32(K) >> 3;
    if (g >= (int64_t)Tw * K8 * N) return;
    const int n = (int)(g % N), kg = (int)((g / N) % K8), tw = (int)(g / ((int64_t)N * K8));
    uint32_t word[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        float v[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = kg * 8 + h * 2 + i;
            v[i] = 0.f;
            if (k < K) {
                if (kind == HP_CONV_F16 || kind == HP_CONV_BF16) v[i] = src[((size_t)n * Cin + k) * taps + tw];
                else if (kind == HP_UP_F16) v[i] = src[((size_t)k * Cout + n) * taps + tw];
                else if (kind == HP_CONV_T_BF16) v[i] = src[((size_t)k * Cin + n) * taps + (taps - 1 - tw)];
                else if (kind == HP_CONV_KT_BF16) v[i] = src[((size_t)k * Cin + n) * taps + tw];
                else {
                    const int ph = k / Cout, co = k - ph * Cout;
                    const int shift = ph + (taps - rate) / 2, j0 = shift % rate, m = tw + lo + shift / rate;
                    if (m >= 0 && j0 + m * rate < taps) v[i] = src[((size_t)n * Cout + co) * taps + j0 + m * rate];
                }
            }
        }
        word[h] = kind <= HP_UP_F16 ? pack_f16x2(v[0], v[1]) : pack_bf16x2(v[0], v[1]);
    }
    reinterpret_cast<Chunk16*>(j[1])[g] = Chunk16{word[0], word[1], word[2], word[3]};
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
// the weight gradient's walk, hifigan_train_ops.hip's `hw_walk`
bool hm_walk(int Cd, int taps, int dilation, int rate, int* wt, int* o0, int* ts, int* cd)
{
    if (rate == 0) {
        *wt = taps; *o0 = -((taps - 1) / 2) * dilation; *ts = dilation; *cd = Cd;
    } else {
        int lo, hi;
        hm_up_reach(taps, rate, &lo, &hi);
        *wt = hi - lo + 1; *o0 = -hi; *ts = 1; *cd = rate * Cd;
    }
    return *wt >= 1 && *wt <= HW_MAX_TAPS;
}

int hm_data_gradient(const float* dy, const uint16_t* wt, const float* x, const float* res, float* out, const int32_t* lengths, int B, int Lmax, int mult, int Cdy,
                     int Cdx, int taps, int o0, int ts, float mslope, float scale, float res_scale, int accumulate, void* stream)
{
    return hg_by_layout(Cdx, [&](auto rt, auto nt) {
        constexpr int RT = decltype(rt)::value, NT = decltype(nt)::value;
        return hg_launch<&hifigan_bwd_bf16_kernel<RT, NT>>(dim3((Lmax * mult + TM - 1) / TM, Cdx / (RT * NT * 16), B), hf_lds_bytes((taps - 1) * ts, Cdy),
                                                           static_cast<hipStream_t>(stream), dy, wt, x, res, out, lengths, Lmax, mult, Cdy, Cdx, taps, o0, ts, mslope,
                                                           scale, res_scale, accumulate);
    });
}

}  // namespace

// glowtts_hifigan_train_supported with the 16-bit tiles' LDS terms; Cout == 1 (conv_post) answers for the f32 launches that serve it
extern "C" int glowtts_hifigan_train_supported_mixed(int Cin, int Cout, int taps, int dilation, int rate)
{
    if (!glowtts_hifigan_train_supported(Cin, Cout, taps, dilation, rate)) return 0;
    if (Cout == 1) return 1;
    int wt, o0, ts, cd;
    if (!hm_walk(Cout, taps, dilation, rate, &wt, &o0, &ts, &cd)) return 0;
    if (!glowtts_hifigan_supported_f16(Cin, Cout, taps, dilation, rate)) return 0;             // the forward's tile
    if (hwb_lds_bytes((wt - 1) * ts) > MAX_LDS) return 0;
    if (rate == 0) return hf_lds_bytes((taps - 1) * dilation, Cout) <= MAX_LDS;
    return cd <= HM_MAX_VIEW && hf_lds_bytes(wt - 1, cd) <= MAX_LDS;
}

extern "C" int glowtts_hifigan_conv_bwd_bf16(const float* dy, const uint16_t* wt, const float* x, const float* residual, float* out, const int32_t* frame_lengths,
                                             int B, int Lmax, int mult, int Cin, int Cout, int taps, int dilation, float mask_slope, float scale, float res_scale,
                                             int accumulate, void* stream)
{
    if (!dy || !wt || !x || !out || !frame_lengths || dy == out || bad_batch(B, Lmax, mult) || Cout == 1 || Cin % 16 ||
        !glowtts_hifigan_train_supported_mixed(Cin, Cout, taps, dilation, 0) || accumulate < 0 || accumulate > 1)
        return GLOWTTS_E_ARG;
    if (hm_data_gradient(dy, wt, x, residual, out, frame_lengths, B, Lmax, mult, Cout, Cin, taps, -((taps - 1) / 2) * dilation, dilation, mask_slope, scale, res_scale,
                         accumulate, stream) != GLOWTTS_OK)
        return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_conv_bwd_bf16");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_upsample_bwd_bf16(const float* dy, const uint16_t* wt, const float* x, float* out, const int32_t* frame_lengths, int B, int Lmax,
                                                 int mult, int Cin, int Cout, int taps, int rate, float mask_slope, void* stream)
{
    if (!dy || !wt || !x || !out || !frame_lengths || dy == out || rate < 1 || rate > HG_MAX_RATE || bad_batch(B, Lmax, mult) || (int64_t)mult * rate > (1 << 16) ||
        bad_batch(B, Lmax, mult * rate) || Cout == 1 || !glowtts_hifigan_train_supported_mixed(Cin, Cout, taps, 1, rate))
        return GLOWTTS_E_ARG;
    int lo, hi;
    hm_up_reach(taps, rate, &lo, &hi);
    if (hm_data_gradient(dy, wt, x, nullptr, out, frame_lengths, B, Lmax, mult, rate * Cout, Cin, hi - lo + 1, lo, 1, mask_slope, 1.f, 1.f, 0, stream) != GLOWTTS_OK)
        return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_upsample_bwd_bf16");
    RET_LAUNCH();
}

// Cout == 1 (conv_post) is served by the f32 launches of glowtts_hifigan_wgrad
extern "C" int glowtts_hifigan_wgrad_bf16(const float* x, const float* dy, const int32_t* frame_lengths, float* work, float* dw, float* dbias, int B, int Lmax,
                                          int mult, int Cin, int Cout, int taps, int dilation, int rate, float slope, float scale, int channels_first, void* stream)
{
    if (Cout == 1) return glowtts_hifigan_wgrad(x, dy, frame_lengths, work, dw, dbias, B, Lmax, mult, Cin, Cout, taps, dilation, rate, slope, scale, channels_first, stream);
    int wt, o0, ts, cd;
    if (!x || !dy || !frame_lengths || !work || !dw || !dbias || bad_batch(B, Lmax, mult) || !glowtts_hifigan_train_supported_mixed(Cin, Cout, taps, dilation, rate) ||
        (channels_first && rate) || !hm_walk(Cout, taps, dilation, rate, &wt, &o0, &ts, &cd))
        return GLOWTTS_E_ARG;
    HwArgs a = {x, dy, frame_lengths, work, B, Lmax, mult, Cin, cd, wt, o0, ts, channels_first, 0, 0, slope};
    const int Tmax = Lmax * mult;
    const HwSizes z = hw_sizes(B, Tmax, Cin, cd, wt);
    if (z.splits > 65535) return GLOWTTS_E_ARG;
    a.nchunk = hw_nchunk(Tmax);
    a.group = hw_group(Tmax);
    const dim3 grid(z.CiP / HW_C, z.CoP / HW_C, z.splits);
    const int lds = hwb_lds_bytes((wt - 1) * ts);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int status;
    if (wt <= 3) status = hg_launch<&hifigan_wgrad_bf16_kernel<3>>(grid, lds, st, a);
    else if (wt <= 7) status = hg_launch<&hifigan_wgrad_bf16_kernel<7>>(grid, lds, st, a);
    else status = hg_launch<&hifigan_wgrad_bf16_kernel<HW_MAX_TAPS>>(grid, lds, st, a);
    if (status != GLOWTTS_OK) return status;
    GLOWTTS_NOTE_STATIC("hifigan_wgrad_bf16");
    hipLaunchKernelGGL(hifigan_wgrad_sum_kernel, dim3((unsigned)((z.per_split + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, work, dw, dbias, z.splits, wt, Cin, cd,
                       z.CiP, z.CoP, o0, rate, taps, scale);
    GLOWTTS_NOTE_STATIC("hifigan_wgrad_sum");
    RET_LAUNCH();
}

// jobs: a DEVICE table of njobs x 8 int64 (the layout above; first blocks ascending from 0), total_blocks: the sum of the jobs' blocks of 256 groups
extern "C" int glowtts_hifigan_pack_images(const int64_t* jobs, int njobs, int total_blocks, void* stream)
{
    if (!jobs || njobs < 1 || njobs > 4096 || total_blocks < 1) return GLOWTTS_E_ARG;
    hipLaunchKernelGGL(hifigan_pack_images_kernel, dim3((unsigned)total_blocks), dim3(THREADS), 0, static_cast<hipStream_t>(stream), jobs, njobs);
    GLOWTTS_NOTE_STATIC("hifigan_pack_images");
    RET_LAUNCH();
}
