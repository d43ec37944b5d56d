// Neural vocoder, fp16 inference mode: the HiFi-GAN generator's convolutions and transposed convolutions with fp16 operands and fp32 sums (DESIGN.md
// "HiFi-GAN generator: fp16 inference mode" has the contract).  Only the launches `hifigan_conv` (conv_pre included) and `hifigan_upsample` change;
// conv_post + tanh stays the f32 launch `hifigan_conv,post` of hifigan_ops.hip, and `hg_tile` and its instantiations are not touched: this file has a tile
// body of its own, `hf_tile`.
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
#include "hifigan_common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr float F16_MAX = 65504.f;

__host__ __device__ __forceinline__ int hf_pad32(int K) { return (K + 31) & ~31; }

__device__ __forceinline__ f32x4 mfma32h(const Chunk16& a, const Chunk16& b, const f32x4& c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(&a), *reinterpret_cast<const f16x8*>(&b), c, 0, 0, 0);
}

// clamp to the largest finite fp16, then round to nearest even (the cast is v_cvt_f16_f32 under the kernel's default rounding mode)
__device__ __forceinline__ _Float16 to_f16(float v) { return (_Float16)fminf(fmaxf(v, -F16_MAX), F16_MAX); }
__device__ __forceinline__ uint32_t pack_f16x2(float lo, float hi)
{
    f16x2 v;
    v[0] = to_f16(lo);
    v[1] = to_f16(hi);
    return *reinterpret_cast<uint32_t*>(&v);
}
__device__ __forceinline__ uint16_t f16_bits(float x)
{
    const _Float16 h = to_f16(x);
    return *reinterpret_cast<const uint16_t*>(&h);
}

// The tile body.  inb: the utterance's slab (channels-last [..][Cin], or channels-first [Cin][tin_max] with cf); position s0 + i writes output row
// (s0 + i) os + oph of outb ([..][Cout]) when it is below T, the utterance's rows at the input's rate.  Xs: LDS, (64 + reach) rows of min(Cp, 64) + 8 fp16.
template <int RT, int NT>
__device__ __forceinline__ void hf_tile(const float* __restrict__ inb, const uint16_t* __restrict__ w, const float* __restrict__ bias, const float* resb,
                                        float* outb, uint16_t* Xs, int T, int tin_max, int s0, int Cin, int Cout, int colgroup, HgTaps tp, float slope, int cf,
                                        int os, int oph, int accumulate, float divisor)
{
    constexpr int WR = WAVES / RT, WC = WAVES / WR;        // the waves as WR row groups x WC column groups
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int wr = wave % WR, wc = wave / WR;
    const int col0 = (colgroup * WC + wc) * NT * 16;
    const int last = tp.o0 + (tp.nt - 1) * tp.ts;
    const int lo = min(tp.o0, last), span = TM + max(tp.o0, last) - lo;
    const int Cp = hf_pad32(Cin), xs = min(Cp, HG_CK) + 8; // the image's rows per tap; the LDS row stride in fp16
    const Chunk16* wv = reinterpret_cast<const Chunk16*>(w);

    f32x4 acc[RT][NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const float bv = bias[col0 + n * 16 + r];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][n] = f32x4{bv, bv, bv, bv};
    }

    for (int c0 = 0; c0 < Cin; c0 += HG_CK) {
        const int ck = min(HG_CK, Cin - c0), ckp = hf_pad32(ck), ns = ckp >> 5;        // ns: k steps of this chunk, 1 or 2
        // the weights of (tap m, k step s, column tile n) of this chunk
        const Chunk16* wc0 = wv + ((size_t)(c0 >> 3) + q) * Cout + col0 + r;
        auto load_tap = [&](int m, Chunk16 (&b)[2][NT]) {
            const Chunk16* wp = wc0 + (size_t)(tp.w0 + m * tp.wstep) * (Cp >> 3) * Cout;
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (s < ns) {                              // (uniform)
#pragma unroll
                    for (int n = 0; n < NT; ++n) b[s][n] = wp[(size_t)s * 4 * Cout + n * 16];
                }
        };
        Chunk16 cur[2][NT];
        load_tap(0, cur);                                  // in flight while the chunk is staged

        if (c0) __syncthreads();                           // every wave is done with the previous chunk
        if (cf) {                                          // channels-first source (the mel): consecutive threads along the rows
            for (int e = tid; e < span * ckp; e += THREADS) {
                const int c = e / span, row = e - c * span, t = s0 + lo + row;
                Xs[row * xs + c] = (c < ck && t >= 0 && t < T) ? f16_bits(lrelu(inb[(size_t)(c0 + c) * tin_max + t], slope)) : (uint16_t)0;
            }
        } else {
            // four channels (8 bytes of fp16) per access.  Every load is unconditional, from an address clamped into the utterance's own rows and the
            // chunk's own channels, and zeroed afterwards where the element is padding: four of them are in flight per thread.
            const int ksh = ckp == 64 ? 4 : 3, kq = 1 << ksh, total = span << ksh;
            for (int e0 = tid; e0 < total; e0 += 4 * THREADS) {
                float4 v[4];
                bool ok[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * THREADS, row = e >> ksh, k4 = (e & (kq - 1)) * 4, t = s0 + lo + row;
                    ok[u] = e < total && t >= 0 && t < T && k4 < ck;
                    v[u] = *reinterpret_cast<const float4*>(inb + (size_t)min(max(t, 0), T - 1) * Cin + c0 + min(k4, ck - 4));
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * THREADS, row = e >> ksh, k4 = (e & (kq - 1)) * 4;
                    if (e >= total) break;
                    const float4 x = ok[u] ? v[u] : make_float4(0.f, 0.f, 0.f, 0.f);
                    *reinterpret_cast<u32x2*>(Xs + row * xs + k4) =
                        u32x2{pack_f16x2(lrelu(x.x, slope), lrelu(x.y, slope)), pack_f16x2(lrelu(x.z, slope), lrelu(x.w, slope))};
                }
            }
        }
        __syncthreads();

        for (int m = 0; m < tp.nt; ++m) {
            Chunk16 nxt[2][NT];
            if (m + 1 < tp.nt) load_tap(m + 1, nxt);
            const uint16_t* xa = Xs + (wr * RT * 16 + r + tp.o0 + m * tp.ts - lo) * xs + q * 8;
            f32x4 part[RT][NT];                            // this (chunk, tap)'s chain
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int n = 0; n < NT; ++n) part[rt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (s < ns) {
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const Chunk16 a = *reinterpret_cast<const Chunk16*>(xa + rt * 16 * xs + s * 32);
#pragma unroll
                        for (int n = 0; n < NT; ++n) part[rt][n] = mfma32h(a, cur[s][n], part[rt][n]);
                    }
                }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[rt][n] += part[rt][n];
            if (m + 1 < tp.nt) {
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int n = 0; n < NT; ++n) cur[s][n] = nxt[s][n];
            }
        }
    }

#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int s = s0 + (wr * RT + rt) * 16 + q * 4 + i;
            if (s >= T) continue;                          // padded rows are never written
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const size_t idx = ((size_t)s * os + oph) * Cout + col0 + n * 16 + r;
                float y = acc[rt][n][i];
                if (resb) y += resb[idx];
                if (accumulate == 1) y = outb[idx] + y;
                else if (accumulate == 2) y = (outb[idx] + y) / divisor;
                outb[idx] = y;
            }
        }
}

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

int hf_lds_bytes(int reach, int Cin) { return (TM + reach) * (std::min(hf_pad32(Cin), HG_CK) + 8) * 2; }

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
