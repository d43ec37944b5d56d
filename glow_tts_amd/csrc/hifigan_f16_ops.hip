// Neural vocoder, fp16 inference mode: the HiFi-GAN generator's convolutions and transposed convolutions with fp16 operands and fp32 sums (DESIGN.md
// "HiFi-GAN generator: fp16 inference mode" has the contract).  Only the launches `hifigan_conv` (conv_pre included) and `hifigan_upsample` change;
// conv_post + tanh stays the f32 launch `hifigan_conv,post` of hifigan_ops.hip, and `hg_tile` and its instantiations are not touched: the tile
// body, `hf_tile`, lives in hifigan_f16_tile.h, shared with the mixed-precision training mode (hifigan_mixed_ops.hip).
//
//   hifigan_conv_f16      the f32 kernel's ownership: a workgroup owns 64 consecutive rows of one utterance and RT NT 16 output columns (blockIdx.y), the
//                         wave layouts by Cout are `hg_by_layout`'s.  It walks the input channels in chunks of 64:
//                           1. stages the rows [s0 - pad, s0 + 63 + pad] of the chunk into LDS: LeakyReLU(slope) in fp32, then CLAMPED to +-65504 and ROUNDED
//                              to fp16, nearest even (v_cvt_f16_f32 under the default rounding mode; never the round-toward-zero pack conversion); zero
//                              outside the utterance; the last chunk is padded with zero columns to a multiple of 32, the k step;
//                           2. per tap and k step of 32: one 16-byte LDS read per row tile, one 16-byte weight load per column tile (a lane's eight k values),
//                              RT x NT v_mfma_f32_16x16x32_f16.  fp16 x fp16 products are exact in fp32.  The products of one (chunk, tap) - 32 or 64 - are
//                              one MFMA chain from zero, k ascending; the chains are added to the fp32 sum, which starts at the fp32 bias, chunk by chunk and
//                              tap by tap: the f32 kernel's order.  The weights of the next tap are in flight while this tap's MFMAs issue.
//                         Epilogue: the f32 kernel's, all fp32: + residual (the UNROUNDED row), then out = y, out + y or (out + y) / divisor.
//   hifigan_upsample_f16  the polyphase form on the same body: blockIdx.y = (column group, phase), the tap walk of hifigan_upsample.
// Operand layout of v_mfma_f32_16x16x32_f16: lane l holds A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15], j = 0 .. 7; C as mfma4.
// Weight images (packed once at load on the host, vocoder.hifigan_pack_f16): [taps][Cp / 8][Cout][8] fp16 with Cp = Cin rounded up to a multiple of 32 -
// element (tap, k, n) at ((tap Cp / 8 + k / 8) Cout + n) 8 + k % 8, zero rows from Cin to Cp; chunk c0 starts at k step c0 / 32 of its tap.
// LDS rows are min(Cp, 64) fp16 + 16 bytes: the stride in 16-byte slots (9 or 5) is odd, as in pwg_bf16_ops.hip.
// Tiles start at the utterance's own row 0, every sum has one fixed order and padded rows are never written: a row's value depends on its utterance alone,
// bit-identical alone, in any batch, at any padding and from run to run.  It is not the f32 kernels' value.
#include "hifigan_f16_tile.h"

namespace {

// grid (ceil(Lmax mult / 64), Cout / (RT NT 16), B); dynamic LDS (64 + (taps - 1) d) rows
template <int RT, int NT>
__global__ __launch_bounds__(THREADS) void hifigan_conv_f16_kernel(const float* __restrict__ in, const uint16_t* __restrict__ w, const float* __restrict__ bias,
                                                                   const float* res, float* out, const int32_t* __restrict__ lengths, int Lmax, int mult, int Cin,
                                                                   int Cout, int taps, int d, float slope, int accumulate, float divisor, int cf)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t hf_smem[];
    const int b = blockIdx.z, s0 = blockIdx.x * TM;
    const int Tmax = Lmax * mult, T = min(lengths[b], Lmax) * mult;
    if (s0 >= T) return;                                   // (uniform over the workgroup)
    const size_t row0 = (size_t)b * Tmax;
    const HgTaps tp = {taps, -((taps - 1) / 2) * d, d, 0, 1};
    hf_tile<RT, NT>(in + row0 * Cin, w, bias, res ? res + row0 * Cout : nullptr, out + row0 * Cout, hf_smem, T, Tmax, s0, Cin, Cout, blockIdx.y, tp, slope, cf, 1, 0,
                    accumulate, divisor);
}

// grid (ceil(Lmax mult / 64), u Cout / (RT NT 16), B); in [B][Lmax mult][Cin] -> out [B][Lmax mult u][Cout]
template <int RT, int NT>
__global__ __launch_bounds__(THREADS) void hifigan_upsample_f16_kernel(const float* __restrict__ in, const uint16_t* __restrict__ w, const float* __restrict__ bias,
                                                                       float* __restrict__ out, const int32_t* __restrict__ lengths, int Lmax, int mult, int Cin,
                                                                       int Cout, int k, int u, float slope)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t hf_smem[];
    const int b = blockIdx.z, s0 = blockIdx.x * TM;
    const int Tmax = Lmax * mult, T = min(lengths[b], Lmax) * mult;
    if (s0 >= T) return;                                   // (uniform over the workgroup)
    const int ph = blockIdx.y % u, colgroup = blockIdx.y / u;
    const int shift = ph + (k - u) / 2, j0 = shift % u;
    const HgTaps tp = {(k - j0 + u - 1) / u, shift / u, -1, j0, u};
    const size_t row0 = (size_t)b * Tmax;
    hf_tile<RT, NT>(in + row0 * Cin, w, bias, nullptr, out + row0 * u * Cout, hf_smem, T, Tmax, s0, Cin, Cout, colgroup, tp, slope, 0, u, ph, 0, 1.f);
}


}  // namespace

// glowtts_hifigan_supported with the fp16 tile's LDS term; Cout == 1 (conv_post) has no fp16 form and answers for the f32 launch that serves it
extern "C" int glowtts_hifigan_supported_f16(int Cin, int Cout, int taps, int dilation, int rate)
{
    if (!glowtts_hifigan_supported(Cin, Cout, taps, dilation, rate)) return 0;
    if (Cout == 1) return 1;
    return hf_lds_bytes(rate == 0 ? (taps - 1) * dilation : (taps + rate - 1) / rate - 1, Cin) <= MAX_LDS;
}

extern "C" int glowtts_hifigan_conv_f16(const float* in, const uint16_t* w, const float* bias, const float* residual, float* out, const int32_t* frame_lengths,
                                        int B, int Lmax, int mult, int Cin, int Cout, int taps, int dilation, float slope, int accumulate, float divisor,
                                        int channels_first, void* stream)
{
    if (!in || !w || !bias || !out || !frame_lengths || in == out || bad_batch(B, Lmax, mult) || Cout == 1 ||
        !glowtts_hifigan_supported_f16(Cin, Cout, taps, dilation, 0) || accumulate < 0 || accumulate > 2 || (accumulate == 2 && !(divisor > 0.f)))
        return GLOWTTS_E_ARG;
    const int status = hg_by_layout(Cout, [&](auto rt, auto nt) {
        constexpr int RT = decltype(rt)::value, NT = decltype(nt)::value;
        return hg_launch<&hifigan_conv_f16_kernel<RT, NT>>(dim3((Lmax * mult + TM - 1) / TM, Cout / (RT * NT * 16), B), hf_lds_bytes((taps - 1) * dilation, Cin),
                                                           static_cast<hipStream_t>(stream), in, w, bias, residual, out, frame_lengths, Lmax, mult, Cin, Cout, taps,
                                                           dilation, slope, accumulate, divisor, channels_first);
    });
    if (status != GLOWTTS_OK) return status;
    GLOWTTS_NOTE_STATIC("hifigan_conv_f16");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_upsample_f16(const float* in, const uint16_t* w, const float* bias, float* out, const int32_t* frame_lengths, int B, int Lmax,
                                            int mult, int Cin, int Cout, int taps, int rate, float slope, void* stream)
{
    if (!in || !w || !bias || !out || !frame_lengths || in == out || rate < 1 || rate > HG_MAX_RATE || bad_batch(B, Lmax, mult) ||
        (int64_t)mult * rate > (1 << 16) || bad_batch(B, Lmax, mult * rate) || !glowtts_hifigan_supported_f16(Cin, Cout, taps, 1, rate))
        return GLOWTTS_E_ARG;
    const int status = hg_by_layout(Cout, [&](auto rt, auto nt) {
        constexpr int RT = decltype(rt)::value, NT = decltype(nt)::value;
        return hg_launch<&hifigan_upsample_f16_kernel<RT, NT>>(dim3((Lmax * mult + TM - 1) / TM, rate * (Cout / (RT * NT * 16)), B),
                                                               hf_lds_bytes((taps + rate - 1) / rate - 1, Cin), static_cast<hipStream_t>(stream), in, w, bias, out,
                                                               frame_lengths, Lmax, mult, Cin, Cout, taps, rate, slope);
    });
    if (status != GLOWTTS_OK) return status;
    GLOWTTS_NOTE_STATIC("hifigan_upsample_f16");
    RET_LAUNCH();
}
