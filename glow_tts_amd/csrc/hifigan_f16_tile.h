// The 16-bit-operand tile body of the HiFi-GAN generator, `hf_tile`, shared by the fp16 inference mode (hifigan_f16_ops.hip) and the mixed-precision training
// mode (hifigan_mixed_ops.hip).  It is the f32 body's ownership, tap walk and summation order on v_mfma_f32_16x16x32_{f16,bf16}: the head of
// hifigan_f16_ops.hip describes the tile.  Two things are compile-time parameters:
//   OP   the operand type: `HfF16` (clamped to +-65504, rounded to fp16, nearest even) or `HfBf16` (rounded to bf16, nearest even, no clamp: bf16 has fp32's
//        range; `pack_bf16x2` / `bf16_bits` / `mfma16_bf16` of device_common.h).  The packed weight image has one layout for both, 2 bytes per element.
//   BWD  a data gradient (`hg_tile<.., true>`'s epilogue): the sums start at zero and y = sum * (maskb > 0 ? 1 : mslope) * divisor + resb * res_scale, then
//        out = y or (accumulate) out = out + y; maskb: the kept fp32 input of the forward's LeakyReLU, laid out as outb.  The staged rows (dy) are taken as they
//        lie in memory (slope 1).
//   FOLD the folded row source of `hg_tile` (hifigan_common.h), for the multi-period discriminator (hifigan_disc_bf16_ops.hip): the tile stages the 64 rows
//        of EVERY tap, [taps][64] rows through `hd_source_row<BWD>` - tap m's rows at LDS row m * 64, zero rows where the map gives none - with the span
//        mode's loads (unconditional, from an address clamped into the slab, zeroed afterwards) and its K padding to 32 per chunk.  T is then the count of
//        flat OUTPUT rows and Hsrc the source's rows h; tp.p, tp.s are the period and the row stride.  Channels-last sources alone.
// Every BWD / OP / FOLD term is a compile-time branch: the <RT, NT, HfF16, false> instantiations are the code they were.
#pragma once
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

// the two operand types of the body
struct HfF16 {
    static __device__ __forceinline__ uint32_t pack2(float lo, float hi) { return pack_f16x2(lo, hi); }
    static __device__ __forceinline__ uint16_t bits(float x) { return f16_bits(x); }
    static __device__ __forceinline__ f32x4 mfma(const Chunk16& a, const Chunk16& b, const f32x4& c) { return mfma32h(a, b, c); }
};
struct HfBf16 {
    static __device__ __forceinline__ uint32_t pack2(float lo, float hi) { return pack_bf16x2(lo, hi); }
    static __device__ __forceinline__ uint16_t bits(float x) { return bf16_bits(x); }
    static __device__ __forceinline__ f32x4 mfma(const Chunk16& a, const Chunk16& b, const f32x4& c) { return mfma16_bf16(a, b, c); }
};

// The tile body.  inb: the utterance's slab (channels-last [..][Cin], or channels-first [Cin][tin_max] with cf); position s0 + i writes output row
// (s0 + i) os + oph of outb ([..][Cout]) when it is below T, the utterance's rows at the input's rate.  Xs: LDS, (64 + reach) rows of min(Cp, 64) + 8 elements
// (FOLD: taps 64 rows).
template <int RT, int NT, typename OP = HfF16, bool BWD = false, bool FOLD = false>
__device__ __forceinline__ void hf_tile(const float* __restrict__ inb, const uint16_t* __restrict__ w, const float* __restrict__ bias, const float* resb,
                                        float* outb, uint16_t* Xs, int T, int tin_max, int s0, int Cin, int Cout, int colgroup, HgTaps tp, float slope, int cf,
                                        int os, int oph, int accumulate, float divisor, const float* maskb = nullptr, float mslope = 1.f, float res_scale = 1.f,
                                        int Hsrc = 0)
{
    constexpr int WR = WAVES / RT, WC = WAVES / WR;        // the waves as WR row groups x WC column groups
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int wr = wave % WR, wc = wave / WR;
    const int col0 = (colgroup * WC + wc) * NT * 16;
    const int last = tp.o0 + (tp.nt - 1) * tp.ts;
    const int lo = FOLD ? 0 : min(tp.o0, last), span = FOLD ? tp.nt * TM : TM + max(tp.o0, last) - lo;
    const int Cp = hf_pad32(Cin), xs = min(Cp, HG_CK) + 8; // the image's rows per tap; the LDS row stride in elements
    const Chunk16* wv = reinterpret_cast<const Chunk16*>(w);

    f32x4 acc[RT][NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        float bv = 0.f;
        if constexpr (!BWD) bv = bias[col0 + n * 16 + r];
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
        if (!FOLD && cf) {                                 // channels-first source (the mel): consecutive threads along the rows
            for (int e = tid; e < span * ckp; e += THREADS) {
                const int c = e / span, row = e - c * span, t = s0 + lo + row;
                Xs[row * xs + c] = (c < ck && t >= 0 && t < T) ? OP::bits(lrelu(inb[(size_t)(c0 + c) * tin_max + t], slope)) : (uint16_t)0;
            }
        } else {
            // four channels (8 bytes) per access.  Every load is unconditional, from an address clamped into the utterance's own rows and the
            // chunk's own channels, and zeroed afterwards where the element is padding: four of them are in flight per thread.
            const int ksh = ckp == 64 ? 4 : 3, kq = 1 << ksh, total = span << ksh;
            for (int e0 = tid; e0 < total; e0 += 4 * THREADS) {
                float4 v[4];
                bool ok[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * THREADS, row = e >> ksh, k4 = (e & (kq - 1)) * 4;
                    int t;
                    if constexpr (FOLD) {                  // the source row of (output row, tap); row 0 of the slab where there is none
                        const int m = row / TM, n = s0 + row - m * TM;
                        int from = 0;
                        ok[u] = e < total && n < T && hd_source_row<BWD>(n, m, (tp.nt - 1) / 2, tp.p, tp.s, Hsrc, &from) && k4 < ck;
                        t = ok[u] ? from : 0;
                    } else {
                        t = s0 + lo + row;
                        ok[u] = e < total && t >= 0 && t < T && k4 < ck;
                        t = min(max(t, 0), T - 1);
                    }
                    v[u] = *reinterpret_cast<const float4*>(inb + (size_t)t * Cin + c0 + min(k4, ck - 4));
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * THREADS, row = e >> ksh, k4 = (e & (kq - 1)) * 4;
                    if (e >= total) break;
                    const float4 x = ok[u] ? v[u] : make_float4(0.f, 0.f, 0.f, 0.f);
                    *reinterpret_cast<u32x2*>(Xs + row * xs + k4) =
                        u32x2{OP::pack2(lrelu(x.x, slope), lrelu(x.y, slope)), OP::pack2(lrelu(x.z, slope), lrelu(x.w, slope))};
                }
            }
        }
        __syncthreads();

        for (int m = 0; m < tp.nt; ++m) {
            Chunk16 nxt[2][NT];
            if (m + 1 < tp.nt) load_tap(m + 1, nxt);
            const uint16_t* xa = Xs + (wr * RT * 16 + r + (FOLD ? m * TM : tp.o0 + m * tp.ts - lo)) * xs + q * 8;
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
                        for (int n = 0; n < NT; ++n) part[rt][n] = OP::mfma(a, cur[s][n], part[rt][n]);
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
                if constexpr (BWD) {
                    y = y * (maskb[idx] > 0.f ? 1.f : mslope) * divisor;
                    if (resb) y += resb[idx] * res_scale;
                    if (accumulate) y = outb[idx] + y;
                } else {
                    if (resb) y += resb[idx];
                    if (accumulate == 1) y = outb[idx] + y;
                    else if (accumulate == 2) y = (outb[idx] + y) / divisor;
                }
                outb[idx] = y;
            }
        }
}

int hf_lds_bytes(int reach, int Cin) { return (TM + reach) * (std::min(hf_pad32(Cin), HG_CK) + 8) * 2; }         // FOLD: reach = (taps - 1) 64

}  // namespace
