// The bf16 mode of the HiFi-GAN multi-period discriminator for gfx950 (DESIGN.md "The multi-period discriminator in bf16" has the contract): the matrix
// products of the middle convolutions convs.1 .. convs.{n-1} of every period on v_mfma_f32_16x16x32_bf16, forward and backward alike.  bf16 has fp32's
// range, so nothing is clamped or scaled.  The master weights, every tensor in memory, every sum, every bias and every epilogue stay fp32; the first layer,
// conv_post, the feature-matching loss and their backwards are the f32 launches of hifigan_disc_ops.hip.  No float atomics, one summation order that depends
// on the sizes alone: every result is bit-identical from run to run, and a batch row's results do not depend on the batch around it.
//
//   hifigan_disc_conv_bf16      `hifigan_disc_conv` on `hf_tile<.., HfBf16, false, FOLD>` (hifigan_f16_tile.h): the f32 launch's grid, ownership, folded
//                               staging ([taps][64] rows through `hd_source_row`), chunk and tap walk and epilogue.  The staged rows lrelu(kept
//                               pre-activation) and the image are bf16 (nearest even); per (chunk, tap) a chain from zero of one or two MFMAs, added in the
//                               f32 kernel's order to the accumulator that starts at the fp32 bias.  w: the packed image [5][pad32(Cin) / 8][Cout][8] of
//                               `hifigan_pack_images` kind 5.
//   hifigan_disc_conv_bwd_bf16  the same body under the inverse row map: the staged rows of d pre as they lie in memory, against the channel-transposed image
//                               [5][pad32(Cout) / 8][Cin][8] (kind 6: no tap reversal, the inverse map does that); fp32 epilogue
//                               sum * lrelu'(kept pre-activation) + inj * *inj_scale.
//   hifigan_disc_wgrad_bf16     `hifigan_wgrad_bf16_kernel<5, MAP>` (hifigan_wgrad_bf16.h) + the unchanged `hifigan_wgrad_sum`: the f32 weight gradient's fixed
//                               partition with both operands rounded to bf16; the bias gradient from the unrounded d pre, in double.
#include "hifigan_disc_common.h"
#include "hifigan_f16_tile.h"
#include "hifigan_wgrad_bf16.h"

namespace {

// grid (ceil(Ndst / 64), Cdst / (RT NT 16), B); src [B][Hsrc p][Csrc] -> out [B][Ndst][Cdst]; dynamic LDS [taps][64] rows of min(pad32(Csrc), 64) + 8 bf16.
// The arguments of hifigan_disc_conv_kernel with the packed 16-bit image.
template <int RT, int NT, bool BWD>
__global__ __launch_bounds__(THREADS) void hifigan_disc_conv_bf16_kernel(const float* __restrict__ src, const uint16_t* __restrict__ w,
                                                                         const float* __restrict__ bias, const float* __restrict__ mask,
                                                                         const float* __restrict__ inj, const float* __restrict__ inj_scale, float* __restrict__ out,
                                                                         int Hsrc, int Ndst, int taps, int p, int s, int Csrc, int Cdst, float slope_in, float mslope)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t hdb_smem[];
    const size_t out0 = (size_t)blockIdx.z * Ndst * Cdst;
    const HgTaps tp = {taps, 0, 0, 0, 1, p, s};
    hf_tile<RT, NT, HfBf16, BWD, true>(src + (size_t)blockIdx.z * Hsrc * p * Csrc, w, bias, (BWD && inj) ? inj + out0 : nullptr, out + out0, hdb_smem, Ndst, 0,
                                       blockIdx.x * TM, Csrc, Cdst, blockIdx.y, tp, slope_in, 0, 1, 0, 0, 1.f, BWD ? mask + out0 : nullptr, mslope,
                                       (BWD && inj) ? inj_scale[0] : 0.f, Hsrc);
}

int hdb_lds_bytes(int Csrc) { return hf_lds_bytes((HD_TAPS - 1) * TM, Csrc); }                // [5][64] rows: 46080 bytes from 64 channels on

template <bool BWD>
int hdb_conv(const float* src, const uint16_t* w, const float* bias, const float* mask, const float* inj, const float* inj_scale, float* out, int B, int Hsrc,
             int Ndst, int p, int s, int Csrc, int Cdst, float slope_in, float mslope, void* stream)
{
    return hg_by_layout(Cdst, [&](auto rt, auto nt) {
        constexpr int RT = decltype(rt)::value, NT = decltype(nt)::value;
        return hg_launch<&hifigan_disc_conv_bf16_kernel<RT, NT, BWD>>(dim3((Ndst + TM - 1) / TM, Cdst / (RT * NT * 16), B), hdb_lds_bytes(Csrc),
                                                                      static_cast<hipStream_t>(stream), src, w, bias, mask, inj, inj_scale, out, Hsrc, Ndst, HD_TAPS, p,
                                                                      s, Csrc, Cdst, slope_in, mslope);
    });
}

bool hdb_middle(int period, int Cin, int Cout) { return hd_width(Cin) && hd_width(Cout) && glowtts_hifigan_disc_supported_bf16(period, Cin, Cout); }

}  // namespace

// glowtts_hifigan_disc_supported with the 16-bit tiles' LDS terms; Cin == 1 (the first layer) and Cout == 1 (conv_post) answer for the f32 launches that serve them
extern "C" int glowtts_hifigan_disc_supported_bf16(int period, int Cin, int Cout)
{
    if (!glowtts_hifigan_disc_supported(period, Cin, Cout)) return 0;
    if (Cin == 1 || Cout == 1) return 1;
    return hdb_lds_bytes(Cin) <= MAX_LDS && hdb_lds_bytes(Cout) <= MAX_LDS && hwb_lds_bytes((HD_TAPS - 1) * TM) <= MAX_LDS;
}

extern "C" int glowtts_hifigan_disc_conv_bf16(const float* x, const uint16_t* w, const float* bias, float* out, int B, int H, int period, int stride, int Cin,
                                              int Cout, float slope, void* stream)
{
    if (!x || !w || !bias || !out || x == out || hd_bad_rows(B, H, period) || !hd_stride(stride) || !hdb_middle(period, Cin, Cout)) return GLOWTTS_E_ARG;
    if (hdb_conv<false>(x, w, bias, nullptr, nullptr, nullptr, out, B, H, hd_rows_out(H, stride) * period, period, stride, Cin, Cout, slope, 1.f, stream) != GLOWTTS_OK)
        return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_disc_conv_bf16");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_disc_conv_bwd_bf16(const float* dy, const uint16_t* wt, const float* x, const float* inj, const float* inj_scale, float* dx, int B,
                                                  int H, int period, int stride, int Cin, int Cout, float slope, void* stream)
{
    if (!dy || !wt || !x || !dx || dx == dy || dx == x || (inj && !inj_scale) || hd_bad_rows(B, H, period) || !hd_stride(stride) || !hdb_middle(period, Cin, Cout))
        return GLOWTTS_E_ARG;
    if (hdb_conv<true>(dy, wt, nullptr, x, inj, inj_scale, dx, B, hd_rows_out(H, stride), H * period, period, stride, Cout, Cin, 1.f, slope, stream) != GLOWTTS_OK)
        return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_disc_conv_bwd_bf16");
    RET_LAUNCH();
}

// The middle convolutions alone (5 taps, both widths multiples of 16, no waveform source): the first layer and conv_post keep glowtts_hifigan_disc_wgrad.
extern "C" int glowtts_hifigan_disc_wgrad_bf16(const float* x, const float* dy, float* work, float* dw, float* dbias, int B, int H, int period, int stride, int Cin,
                                               int Cout, int taps, int wav_samples, float slope, void* stream)
{
    if (!x || !dy || !work || !dw || !dbias || hd_bad_rows(B, H, period) || !hd_stride(stride) || !hdb_middle(period, Cin, Cout) || taps != HD_TAPS || wav_samples != 0)
        return GLOWTTS_E_ARG;
    HwArgs a = {x, dy, nullptr, work, B, hd_rows_out(H, stride) * period, 1, Cin, Cout, taps, 0, 0, 0, 0, 0, slope, period, stride, H, 0};
    const int Tmax = a.Lmax;
    const HwSizes z = hw_sizes(B, Tmax, Cin, Cout, taps);
    if (z.splits > 65535) return GLOWTTS_E_ARG;
    a.nchunk = hw_nchunk(Tmax);
    a.group = hw_group(Tmax);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int status = hg_launch<&hifigan_wgrad_bf16_kernel<HD_TAPS, true>>(dim3(z.CiP / HW_C, z.CoP / HW_C, z.splits), hwb_lds_bytes((HD_TAPS - 1) * TM), st, a);
    if (status != GLOWTTS_OK) return status;
    GLOWTTS_NOTE_STATIC("hifigan_disc_wgrad_bf16");
    hipLaunchKernelGGL(hifigan_wgrad_sum_kernel, dim3((unsigned)((z.per_split + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, work, dw, dbias, z.splits, taps, Cin,
                       Cout, z.CiP, z.CoP, 0, 0, taps, 1.f);
    GLOWTTS_NOTE_STATIC("hifigan_disc_wgrad_sum");
    RET_LAUNCH();
}
