// What the HiFi-GAN generator's forward (hifigan_ops.hip) and backward (hifigan_train_ops.hip) share: the limits, the tap walk and the tile body - a data
// gradient is the same convolution over rows against the tap-reversed, channel-transposed weight image, so the backward runs `hg_tile` with its sums started at
// zero and an epilogue of its own.  The comment at the head of hifigan_ops.hip describes the tile.
#pragma once
#include <algorithm>

#include "launch_log.h"
#include "pwg_common.h"

namespace {

constexpr int HG_MAX_CHANNELS = 512, HG_MAX_TAPS = 11, HG_MAX_DILATION = 16, HG_MAX_RATE = 16, HG_MAX_UP_TAPS = 64, HG_MAX_PHASE_TAPS = 8;
constexpr int HG_CK = 64;                                  // input channels per LDS chunk

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// How a launch walks its taps: the input row of (position s, tap m) is s + o0 + m ts; the weight rows of tap m start at (w0 + m wstep) Cin.
struct HgTaps {
    int nt, o0, ts, w0, wstep;
};

// The tile body of every kernel.  inb: the utterance's slab (channels-last [Tin_max][Cin], or channels-first [Cin][tin_max] with cf); Tin: its own rows;
// position s writes output row s os + oph of outb ([..][Cout]).  Xs: LDS, (64 + reach) rows of lds_stride_of(min(Cin, 64)) floats.
// BWD (hifigan_train_ops.hip; the data gradient is this convolution of dy against the tap-reversed, channel-transposed image): the sums start at zero and the
// epilogue is y = sum * (maskb > 0 ? 1 : mslope) * divisor + resb * res_scale, then out = y or (accumulate) out = out + y; maskb: the kept input of the
// forward's LeakyReLU, laid out as outb.
template <int RT, int NT, bool BWD = false>
__device__ __forceinline__ void hg_tile(const float* __restrict__ inb, const float* __restrict__ w, const float* __restrict__ bias, const float* resb,
                                        float* outb, float* Xs, int Tin, int tin_max, int s0, int Cin, int Cout, int colgroup, HgTaps tp, float slope, int cf,
                                        int os, int oph, int accumulate, float divisor, const float* maskb = nullptr, float mslope = 1.f, float res_scale = 1.f)
{
    constexpr int WR = WAVES / RT, WC = WAVES / WR;        // the waves as WR row groups x WC column groups
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int wr = wave % WR, wc = wave / WR;
    const int col0 = (colgroup * WC + wc) * NT * 16;
    const int last = tp.o0 + (tp.nt - 1) * tp.ts;
    const int lo = min(tp.o0, last), span = TM + max(tp.o0, last) - lo;
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
        if (cf) {                                          // channels-first source (the mel): consecutive threads along the rows
            for (int e = tid; e < span * ck; e += THREADS) {
                const int c = e / span, row = e - c * span, t = s0 + lo + row;
                Xs[row * xs + c] = (t >= 0 && t < Tin) ? lrelu(inb[(size_t)(c0 + c) * tin_max + t], slope) : 0.f;
            }
        } else {
            const int kq = ck >> 2;
            for (int e = tid; e < span * kq; e += THREADS) {
                const int row = e / kq, k4 = (e - row * kq) * 4, t = s0 + lo + row;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t >= 0 && t < Tin) {
                    v = *reinterpret_cast<const float4*>(inb + (size_t)t * Cin + c0 + k4);
                    v.x = lrelu(v.x, slope); v.y = lrelu(v.y, slope); v.z = lrelu(v.z, slope); v.w = lrelu(v.w, slope);
                }
                *reinterpret_cast<float4*>(Xs + row * xs + k4) = v;
            }
        }
        __syncthreads();
        for (int m = 0; m < tp.nt; ++m) {
            const float* xa = Xs + (wr * RT * 16 + r + tp.o0 + m * tp.ts - lo) * xs + q;
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
                    const float a = xa[rt * 16 * xs + k0];
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
            if (s >= Tin) continue;                        // padded rows are never written
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

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
bool hg_channels(int Cin, int Cout)
{
    return Cin >= 4 && Cin <= HG_MAX_CHANNELS && Cin % 4 == 0 && Cout >= 16 && Cout <= HG_MAX_CHANNELS && Cout % 16 == 0;
}

int hg_lds_bytes(int reach, int Cin) { return (TM + reach) * lds_stride_of(std::min(Cin, HG_CK)) * 4; }

// the wave layout of an output width: columns per workgroup = RT NT 16
void hg_layout(int Cout, int* rt, int* nt)
{
    *rt = Cout % 64 == 0 ? 4 : 1;
    *nt = (Cout % 128 == 0 || (Cout % 64 != 0 && Cout % 32 == 0)) ? 2 : 1;
}

}  // namespace
