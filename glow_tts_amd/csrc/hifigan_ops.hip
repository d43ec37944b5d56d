// Neural vocoder: the HiFi-GAN generator (Kong et al. 2020; transposed convolutions that raise the row rate, each followed by parallel residual stacks whose
// mean is the stage's output - the multi-receptive-field fusion, MRF) for gfx950, inference, f32.
// Rows are samples, channels-last: a stage's tensors are [B][Lmax mult][C] with mult rows per mel frame; an utterance of L frames owns rows [0, L mult) of
// its slab and nothing beyond them is read or (the waveform excepted) written.  Every matrix product runs on the exact-f32 MFMA v_mfma_f32_16x16x4_f32
// (A operand: lane l holds A[l & 15][l >> 4], B operand B[l >> 4][l & 15], result col = l & 15, row = 4 (l >> 4) + reg) against K-major weight images
// [taps Cin][Cout] (row = tap * Cin + input channel) streamed from L2 as B operands.
//
//   hifigan_conv      ONE launch per convolution: a dilated K-tap convolution over rows.  A workgroup owns 64 consecutive rows of one utterance and RT NT 16
//                     output columns (the column group is blockIdx.y).  It walks the input channels in chunks of 64:
//                       1. stages the rows [s0 - pad, s0 + 63 + pad] of the chunk into LDS, LeakyReLU(slope) applied, zero outside the utterance
//                          (LeakyReLU(0) = 0: prologue and padding commute); the mel of conv_pre is read channels-first as the caller gives it;
//                       2. per tap and k step of 4: one LDS read per row tile, one weight load per column tile, RT x NT MFMAs.  The products of one
//                          (chunk, tap) - at most 64 - are one fmaf chain from zero, channel ascending; the chains are added to the sum, which starts at the
//                          bias, chunk by chunk and tap by tap.  Summing in blocks keeps the rounding error of K = taps Cin up to 5632 products near that
//                          of sqrt(K) of them (one chain over all of K measured 2e-6 of the largest output at K = 1792, eight times the float32
//                          convolution of torch on the host); the sums live in registers across the chunks.
//                     Epilogue: + residual; then out = y, out = out + y (MRF accumulate) or out = (out + y) / nk (the stage's last block).
//   hifigan_upsample  the transposed convolution in polyphase form, the same tile body: blockIdx.y = (column group, phase).  Output row t = u s + ph sums the taps
//                     j = j0 + m u (j0 = (ph + p) % u, p = (k - u) / 2) of input row s + (ph + p) / u - m: per phase a dense product over K = Cin taps(ph), the
//                     phases of one (u, k) may have different tap counts.  LeakyReLU(slope) prologue; a workgroup owns 64 input positions, i.e. 64 output rows u apart.
//   hifigan_conv,post the single-channel form (conv_post): LeakyReLU, K taps x Cin -> 1 as a fixed-order fmaf chain per row, tanh; zeros beyond the utterance.
// The wave layout follows the width: RT row tiles x NT column tiles per wave - (4, 2) for Cout % 128 == 0, (4, 1) for % 64, (1, 2) for % 32, else (1, 1) - so
// every wave of a narrow late stage still owns MFMA work.  Tiles start at the utterance's own row 0 and every sum has one fixed order: a row's value depends on
// its utterance alone, bit-identical alone, in any batch, at any padding and from run to run.  No atomics, no workgroup waits on another.
// The tile body `hg_tile`, the limits and the layout dispatcher `hg_by_layout` live in hifigan_common.h.  It is ONE body with two row sources: these kernels
// and the backward (hifigan_train_ops.hip) stage the contiguous span of rows described above; the multi-period discriminator (hifigan_disc_ops.hip) stages
// the rows of every tap through its period-folded row map and runs the same k loop, chains and epilogues.
#include "hifigan_common.h"

namespace {

// grid (ceil(Lmax mult / 64), Cout / (RT NT 16), B); dynamic LDS (64 + (taps - 1) d) rows
template <int RT, int NT>
__global__ __launch_bounds__(THREADS) void hifigan_conv_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                               const float* res, float* out, const int32_t* __restrict__ lengths, int Lmax, int mult, int Cin,
                                                               int Cout, int taps, int d, float slope, int accumulate, float divisor, int cf)
{
    extern __shared__ __attribute__((aligned(16))) float hg_smem[];
    const int b = blockIdx.z, s0 = blockIdx.x * TM;
    const int Tmax = Lmax * mult, T = min(lengths[b], Lmax) * mult;
    if (s0 >= T) return;                                   // (uniform over the workgroup)
    const size_t row0 = (size_t)b * Tmax;
    const HgTaps tp = {taps, -((taps - 1) / 2) * d, d, 0, 1};
    hg_tile<RT, NT>(in + row0 * Cin, w, bias, res ? res + row0 * Cout : nullptr, out + row0 * Cout, hg_smem, T, T, Tmax, s0, Cin, Cout, blockIdx.y, tp, slope, cf, 1, 0,
                    accumulate, divisor);
}

// grid (ceil(Lmax mult / 64), u Cout / (RT NT 16), B); in [B][Lmax mult][Cin] -> out [B][Lmax mult u][Cout];  w [k Cin][Cout]: row = tap * Cin + input channel
template <int RT, int NT>
__global__ __launch_bounds__(THREADS) void hifigan_upsample_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                                   float* __restrict__ out, const int32_t* __restrict__ lengths, int Lmax, int mult, int Cin,
                                                                   int Cout, int k, int u, float slope)
{
    extern __shared__ __attribute__((aligned(16))) float hg_smem[];
    const int b = blockIdx.z, s0 = blockIdx.x * TM;
    const int Tmax = Lmax * mult, T = min(lengths[b], Lmax) * mult;
    if (s0 >= T) return;                                   // (uniform over the workgroup)
    const int ph = blockIdx.y % u, colgroup = blockIdx.y / u;
    const int shift = ph + (k - u) / 2, j0 = shift % u;
    const HgTaps tp = {(k - j0 + u - 1) / u, shift / u, -1, j0, u};
    const size_t row0 = (size_t)b * Tmax;
    hg_tile<RT, NT>(in + row0 * Cin, w, bias, nullptr, out + row0 * u * Cout, hg_smem, T, T, Tmax, s0, Cin, Cout, colgroup, tp, slope, 0, u, ph, 0, 1.f);
}

// ---- conv_post: grid (ceil(Lmax mult / 256), B), a row per thread;  w [taps Cin] (row = tap * Cin + input channel), bias [1] -----------------------------
__global__ __launch_bounds__(THREADS) void hifigan_post_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ wav, const int32_t* __restrict__ lengths, int Lmax, int mult, int Cin, int taps,
                                                               float slope)
{
    const int b = blockIdx.y, t = blockIdx.x * THREADS + threadIdx.x;
    const int Tmax = Lmax * mult, T = min(lengths[b], Lmax) * mult;
    if (t >= Tmax) return;
    const size_t row0 = (size_t)b * Tmax;
    float v = 0.f;                                         // beyond the utterance: zeros
    if (t < T) {
        v = bias[0];
        for (int j = 0; j < taps; ++j) {
            const int ts = t + j - (taps - 1) / 2;
            if (ts < 0 || ts >= T) continue;               // zero padding at the utterance's own ends
            const float* x = in + (row0 + ts) * Cin;
            const float* wj = w + j * Cin;
            for (int c = 0; c < Cin; c += 4) {
                const float4 xv = *reinterpret_cast<const float4*>(x + c), wv = *reinterpret_cast<const float4*>(wj + c);
                v = fmaf(wv.x, lrelu(xv.x, slope), v); v = fmaf(wv.y, lrelu(xv.y, slope), v);
                v = fmaf(wv.z, lrelu(xv.z, slope), v); v = fmaf(wv.w, lrelu(xv.w, slope), v);
            }
        }
        v = tanhf(v);
    }
    wav[row0 + t] = v;
}

}  // namespace

extern "C" int glowtts_hifigan_supported(int Cin, int Cout, int taps, int dilation, int rate)
{
    if (rate == 0) {                                       // a convolution; Cout == 1: the conv_post form
        if (taps < 1 || taps > HG_MAX_TAPS || taps % 2 == 0 || dilation < 1 || dilation > HG_MAX_DILATION) return 0;
        if (Cout == 1) return Cin >= 4 && Cin <= HG_MAX_CHANNELS && Cin % 4 == 0 && dilation == 1;
        return hg_channels(Cin, Cout) && hg_lds_bytes((taps - 1) * dilation, Cin) <= MAX_LDS;
    }
    return dilation == 1 && rate >= 1 && rate <= HG_MAX_RATE && taps >= rate && taps <= HG_MAX_UP_TAPS && (taps - rate) % 2 == 0 &&
           (taps + rate - 1) / rate <= HG_MAX_PHASE_TAPS && hg_channels(Cin, Cout);
}

extern "C" int glowtts_hifigan_conv(const float* in, const float* w, const float* bias, const float* residual, float* out, const int32_t* frame_lengths, int B,
                                    int Lmax, int mult, int Cin, int Cout, int taps, int dilation, float slope, int accumulate, float divisor, int channels_first,
                                    void* stream)
{
    if (!in || !w || !bias || !out || !frame_lengths || in == out || bad_batch(B, Lmax, mult) || Cout == 1 || !glowtts_hifigan_supported(Cin, Cout, taps, dilation, 0) ||
        accumulate < 0 || accumulate > 2 || (accumulate == 2 && !(divisor > 0.f)))
        return GLOWTTS_E_ARG;
    const int status = hg_by_layout(Cout, [&](auto rt, auto nt) {
        constexpr int RT = decltype(rt)::value, NT = decltype(nt)::value;
        return hg_launch<&hifigan_conv_kernel<RT, NT>>(dim3((Lmax * mult + TM - 1) / TM, Cout / (RT * NT * 16), B), hg_lds_bytes((taps - 1) * dilation, Cin),
                                                       static_cast<hipStream_t>(stream), in, w, bias, residual, out, frame_lengths, Lmax, mult, Cin, Cout, taps,
                                                       dilation, slope, accumulate, divisor, channels_first);
    });
    if (status != GLOWTTS_OK) return status;
    GLOWTTS_NOTE_STATIC("hifigan_conv");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_upsample(const float* in, const float* w, const float* bias, float* out, const int32_t* frame_lengths, int B, int Lmax, int mult,
                                        int Cin, int Cout, int taps, int rate, float slope, void* stream)
{
    if (!in || !w || !bias || !out || !frame_lengths || in == out || rate < 1 || rate > HG_MAX_RATE || bad_batch(B, Lmax, mult) ||
        (int64_t)mult * rate > (1 << 16) || bad_batch(B, Lmax, mult * rate) || !glowtts_hifigan_supported(Cin, Cout, taps, 1, rate))
        return GLOWTTS_E_ARG;
    const int status = hg_by_layout(Cout, [&](auto rt, auto nt) {
        constexpr int RT = decltype(rt)::value, NT = decltype(nt)::value;
        return hg_launch<&hifigan_upsample_kernel<RT, NT>>(dim3((Lmax * mult + TM - 1) / TM, rate * (Cout / (RT * NT * 16)), B),
                                                           hg_lds_bytes((taps + rate - 1) / rate - 1, Cin), static_cast<hipStream_t>(stream), in, w, bias, out,
                                                           frame_lengths, Lmax, mult, Cin, Cout, taps, rate, slope);
    });
    if (status != GLOWTTS_OK) return status;
    GLOWTTS_NOTE_STATIC("hifigan_upsample");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_post(const float* in, const float* w, const float* bias, float* wav, const int32_t* frame_lengths, int B, int Lmax, int mult, int Cin,
                                    int taps, float slope, void* stream)
{
    if (!in || !w || !bias || !wav || !frame_lengths || bad_batch(B, Lmax, mult) || !glowtts_hifigan_supported(Cin, 1, taps, 1, 0)) return GLOWTTS_E_ARG;
    hipLaunchKernelGGL(hifigan_post_kernel, dim3((Lmax * mult + THREADS - 1) / THREADS, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), in, w, bias, wav,
                       frame_lengths, Lmax, mult, Cin, taps, slope);
    GLOWTTS_NOTE_STATIC("hifigan_conv,post");
    RET_LAUNCH();
}
