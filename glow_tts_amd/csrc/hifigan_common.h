// What the HiFi-GAN family shares: the generator's forward (hifigan_ops.hip) and backward (hifigan_train_ops.hip) and the multi-period discriminator
// (hifigan_disc_ops.hip).  The limits, the tap walk, the discriminator's row map, ONE tile body (`hg_tile`) and ONE layout dispatcher (`hg_by_layout`).  A data
// gradient is the same convolution over rows against the tap-reversed (generator) or tap-kept (discriminator), channel-transposed weight image, so every
// backward runs `hg_tile` with its sums started at zero and the `BWD` epilogue.  The body has two ROW SOURCES, chosen at compile time:
//   span    (the generator) tap m of position s reads source row s + o0 + m ts: the tile stages ONE contiguous span of rows, the tap shifts the row index.
//   folded  (the discriminator) rows are (h, c) of a waveform folded by the period p, flat row h p + c, and the convolution runs over h with stride s: the tile
//           stages the 64 rows of EVERY tap, [taps][64] rows, through `hd_source_row` - the forward map, or with BWD its inverse - and tap m's rows sit at
//           m * 64.  Taps that leave [0, Hsrc), and in the inverse map taps that the stride does not divide, are zero rows.
//   strided span  (the multi-scale discriminator's grouped, strided convolutions, `GRP`) the span mode with a row stride rs: tap m of position s reads
//           source row s rs + o0 + m ts, so the tile stages ONE contiguous span of 63 rs + 1 + reach rows and position i's tap m sits at LDS row
//           i rs + m.  The source's row pitch is not the K extent (a group's channels of a wider slab; the caller's pointers carry the channel offset), and
//           the output's pitch and valid columns are not the weight image's column count.  With rs = 1 and the output phase (os, oph) it is one phase of
//           the transposed convolution: hifigan_msd_ops.hip.
// Everything after the staging - the k loop, the chains, the epilogue - is one text.  The comment at the head of hifigan_ops.hip describes the tile.
#pragma once
#include <algorithm>
#include <type_traits>

#include "launch_log.h"
#include "pwg_common.h"

namespace {

constexpr int HG_MAX_CHANNELS = 512, HG_MAX_TAPS = 11, HG_MAX_DILATION = 16, HG_MAX_RATE = 16, HG_MAX_UP_TAPS = 64, HG_MAX_PHASE_TAPS = 8;
constexpr int HG_CK = 64;                                  // input channels per LDS chunk

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// The discriminator's row map: whether tap m of `2 half + 1` gives the flat row n a source row, and that flat row (false: a zero row).  Forward: n is an
// output row, the source the input row (s h + m - half) p + c.  INV (data gradient): n is an input row, the source the output row ((h + half - m) / s) p + c
// where s divides h + half - m.  Hsrc: rows h of the source.  (A flag and not a row of -1: the caller's branch is then the only compare; DESIGN.md has the
// measurement.)
template <bool INV>
__device__ __forceinline__ bool hd_source_row(int n, int m, int half, int p, int s, int Hsrc, int* src)
{
    const int h = n / p, c = n - h * p;
    int hs;
    if constexpr (INV) {
        const int t = h + half - m;
        if (t < 0 || t % s) return false;
        hs = t / s;
    } else {
        hs = s * h + m - half;
    }
    if (hs < 0 || hs >= Hsrc) return false;
    *src = hs * p + c;
    return true;
}

// the reflect-padded waveform's sample n of a row of T samples (n >= T is sample 2 T - 2 - n): no padded copy exists
__device__ __forceinline__ float hd_padded(const float* __restrict__ x, int n, int T) { return x[n < T ? n : 2 * T - 2 - n]; }

// How a launch walks its taps: the weight rows of tap m start at (w0 + m wstep) Cin.  Span: the input row of (position s, tap m) is s + o0 + m ts.
// Folded: period p and row stride s of `hd_source_row` (o0, ts unused).  Strided span (GRP): p is the source's row pitch in floats, s the row stride rs.
struct HgTaps {
    int nt, o0, ts, w0, wstep, p, s;
};

// The tile body of every kernel.  inb: the utterance's slab (channels-last [..][Cin], or channels-first [Cin][tin_max] with cf); position s0 + i writes output
// row (s0 + i) os + oph of outb ([..][Cout]) when it is below Tdst.  Tsrc bounds the source rows: span: the slab's own rows (= Tdst); FOLD: its rows h, against
// Tdst flat rows.  Xs: LDS, (64 + reach) rows of lds_stride_of(min(Cin, 64)) floats; FOLD: nt 64 rows.
// BWD (the data gradients; FOLD: the inverse row map): the sums start at zero and the epilogue is
// y = sum * (maskb > 0 ? 1 : mslope) * divisor + resb * res_scale, then out = y or (accumulate) out = out + y; maskb: the kept input of the forward's
// LeakyReLU, laid out as outb.
// FOLD takes its tap count at run time like the span mode (tp.nt is a kernel argument, not a template one): the tap loop stays a loop, as in the generator's
// kernels, whose register figures the discriminator's kernels then share (DESIGN.md has both tables).  Unrolled over a constant five taps the body took 233
// VGPRs at (4, 2), one wave per SIMD; with run-time taps no launch got slower and the discriminator's launches of a training step went from 64.0 to 47.3 ms
// on an MI355X, so the template variant was not needed.
// GRP (never with FOLD; channels-last sources alone): Cin is the K extent and the weight image's rows per tap, Cout the image's columns; the source rows are
// tp.p floats apart, the output rows (and maskb's, resb's) opitch floats, and columns from ovalid on are computed (against zero columns of the image) but
// never written.  Every GRP term below is a compile-time branch: the other instantiations are the code they were.
template <int RT, int NT, bool BWD = false, bool FOLD = false, bool GRP = false>
__device__ __forceinline__ void hg_tile(const float* __restrict__ inb, const float* __restrict__ w, const float* __restrict__ bias, const float* resb,
                                        float* outb, float* Xs, int Tsrc, int Tdst, int tin_max, int s0, int Cin, int Cout, int colgroup, HgTaps tp, float slope,
                                        int cf, int os, int oph, int accumulate, float divisor, const float* maskb = nullptr, float mslope = 1.f,
                                        float res_scale = 1.f, int opitch = 0, int ovalid = 0)
{
    static_assert(!(GRP && FOLD), "the strided span is a span mode");
    constexpr int WR = WAVES / RT, WC = WAVES / WR;        // the waves as WR row groups x WC column groups
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int wr = wave % WR, wc = wave / WR;
    const int col0 = (colgroup * WC + wc) * NT * 16;
    const int last = tp.o0 + (tp.nt - 1) * tp.ts;
    const int rs = GRP ? tp.s : 1;                         // rows of the source between two positions
    const int lo = FOLD ? 0 : min(tp.o0, last), span = FOLD ? tp.nt * TM : (GRP ? (TM - 1) * rs + 1 : TM) + max(tp.o0, last) - lo;
    const int xs = lds_stride_of(min(Cin, HG_CK));

    f32x4 acc[RT][NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        float bv = 0.f;
        if constexpr (!BWD) bv = bias[col0 + n * 16 + r];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][n] = f32x4{bv, bv, bv, bv};
    }

    for (int c0 = 0; c0 < Cin; c0 += HG_CK) {
        const int ck = min(HG_CK, Cin - c0);
        if (c0) __syncthreads();                           // every wave is done with the previous chunk
        if (!FOLD && !GRP && cf) {                               // channels-first source (the mel): consecutive threads along the rows
            for (int e = tid; e < span * ck; e += THREADS) {
                const int c = e / span, row = e - c * span, t = s0 + lo + row;
                Xs[row * xs + c] = (t >= 0 && t < Tsrc) ? lrelu(inb[(size_t)(c0 + c) * tin_max + t], slope) : 0.f;
            }
        } else {
            const int kq = ck >> 2;
            for (int e = tid; e < span * kq; e += THREADS) {
                const int row = e / kq, k4 = (e - row * kq) * 4;
                int t;                                     // the source row; a row without one is zeros
                bool live;
                if constexpr (FOLD) {
                    const int m = row / TM, n = s0 + row - m * TM;
                    live = n < Tdst && hd_source_row<BWD>(n, m, (tp.nt - 1) / 2, tp.p, tp.s, Tsrc, &t);
                } else {
                    t = s0 * rs + lo + row;
                    live = t >= 0 && t < Tsrc;
                }
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (live) {
                    v = *reinterpret_cast<const float4*>(inb + (size_t)t * (GRP ? tp.p : Cin) + c0 + k4);
                    v.x = lrelu(v.x, slope); v.y = lrelu(v.y, slope); v.z = lrelu(v.z, slope); v.w = lrelu(v.w, slope);
                }
                *reinterpret_cast<float4*>(Xs + row * xs + k4) = v;
            }
        }
        __syncthreads();
        for (int m = 0; m < tp.nt; ++m) {
            const float* xa = Xs + ((wr * RT * 16 + r) * rs + (FOLD ? m * TM : tp.o0 + m * tp.ts - lo)) * xs + q;
            const float* wp = w + ((size_t)(tp.w0 + m * tp.wstep) * Cin + c0 + q) * Cout + col0 + r;
            f32x4 part[RT][NT];                            // this (chunk, tap)'s chain
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int n = 0; n < NT; ++n) part[rt][n] = f32x4{0.f, 0.f, 0.f, 0.f};
            auto step = [&](int k0) {
                float bw[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) bw[n] = wp[(size_t)k0 * Cout + n * 16];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const float a = xa[rt * 16 * rs * xs + k0];
#pragma unroll
                    for (int n = 0; n < NT; ++n) part[rt][n] = mfma4(a, bw[n], part[rt][n]);
                }
            };
            int k0 = 0;
            for (; k0 + 16 <= ck; k0 += 16) {              // four k steps at a time: their weight loads are in flight together
#pragma unroll
                for (int u = 0; u < 4; ++u) step(k0 + 4 * u);
            }
            for (; k0 < ck; k0 += 4) step(k0);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[rt][n] += part[rt][n];
        }
    }

#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int s = s0 + (wr * RT + rt) * 16 + q * 4 + i;
            if (s >= Tdst) continue;                       // padded rows are never written
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                if (GRP && col0 + n * 16 + r >= ovalid) continue;
                const size_t idx = ((size_t)s * os + oph) * (GRP ? opitch : Cout) + col0 + n * 16 + r;
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

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
bool hg_channels(int Cin, int Cout)
{
    return Cin >= 4 && Cin <= HG_MAX_CHANNELS && Cin % 4 == 0 && Cout >= 16 && Cout <= HG_MAX_CHANNELS && Cout % 16 == 0;
}

int hg_lds_bytes(int reach, int Cin) { return (TM + reach) * lds_stride_of(std::min(Cin, HG_CK)) * 4; }

// Raises `Kernel`'s dynamic LDS limit where needed and launches it with 256 threads -> GLOWTTS_OK or GLOWTTS_E_LAUNCH (the limit was refused).
template <auto Kernel, typename... Args>
int hg_launch(dim3 grid, int lds, hipStream_t stream, Args... args)
{
    if (allow_lds<Kernel>(lds) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    hipLaunchKernelGGL(Kernel, grid, dim3(THREADS), (size_t)lds, stream, args...);
    return GLOWTTS_OK;
}

// The wave layout of an output width, RT row tiles x NT column tiles per wave (columns per workgroup = RT NT 16): `launch(RT, NT)` with both as
// std::integral_constant, so that the caller's lambda names its kernel's instantiation; returns what it returns.
template <typename Launch>
int hg_by_layout(int Cout, Launch launch)
{
    using std::integral_constant;
    if (Cout % 128 == 0) return launch(integral_constant<int, 4>{}, integral_constant<int, 2>{});
    if (Cout % 64 == 0) return launch(integral_constant<int, 4>{}, integral_constant<int, 1>{});
    if (Cout % 32 == 0) return launch(integral_constant<int, 1>{}, integral_constant<int, 2>{});
    return launch(integral_constant<int, 1>{}, integral_constant<int, 1>{});
}

}  // namespace
