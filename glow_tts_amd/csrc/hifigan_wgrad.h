// The weight-gradient kernels of the HiFi-GAN family, shared by the generator (hifigan_train_ops.hip) and the multi-period discriminator
// (hifigan_disc_ops.hip): one body, two ways to reach the rows of x that a tap reads.
//   MAP = false  the generator: tap j of output row t reads input row t + o0 + j ts - the tile stages one contiguous span of rows and the tap shifts the index.
//   MAP = true   the discriminator: rows are (h, c) of a waveform folded by the period p (flat row h p + c), the convolution runs over h with stride s, so
//                tap j of output row (h', c) reads the input row that `hd_source_row` (hifigan_common.h: the map of the tile body's folded mode) gives it,
//                zero outside [0, Hin).  The tile stages the 64 rows of every tap ([taps][64] rows) - at stride 3 five taps of 64 rows are hardly more than
//                the span they cover.  A source of ONE channel may be the waveform itself (Twav > 0) through the reflect index `hd_padded`: no padded copy.
// hifigan_train_ops.hip's head describes the partition, the tile and the summation order; they are the same in both modes.  So is the launch: `hw_sizes`
// is the one place that knows the partials' sizes and `hw_launch` the one launch sequence (kernel by tap bucket, then the sum) of both C entries.
#pragma once
#include "hifigan_common.h"

namespace {

constexpr int HW_ROWS = 1024;                              // rows of one chunk of the weight-gradient partition
constexpr int HW_C = 32, HW_LD = 48;                       // channels of x and of dy per workgroup; LDS row stride (48 % 32 == 16: rows k .. k + 3 hit distinct banks)
constexpr int HW_MAX_TAPS = 11;

struct HwArgs {
    const float* a;            // x: [B][Tmax][Ca], or channels-first [B][Ca][Tmax]; MAP: [B][Hin p][Ca], or the waveform [B][Twav]
    const float* dy;           // [B][Tmax][Cd]
    const int32_t* lengths;    // (MAP: unused, every utterance has Lmax mult rows)
    float* partial;            // [splits][taps CiP CoP + CoP], CiP = 32 gridDim.x, CoP = 32 gridDim.y
    int B, Lmax, mult, Ca, Cd, taps, o0, ts, cf, nchunk, group;
    float slope;
    int p, s, Hin, Twav;       // MAP alone: period, row stride, rows h of the input, samples of the waveform source (0: none)
};

// grid (ceil(Ca / 32), ceil(Cd / 32), splits); dynamic LDS (64 + reach + 64) rows of 48 floats (MAP: (taps 64 + 64) rows)
template <int MAXT, bool MAP = false>
__global__ __launch_bounds__(THREADS) void hifigan_wgrad_kernel(const HwArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float hw_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int wr = wave & 1, wc = wave >> 1;               // the wave's tile: 16 channels of x, 16 of dy
    const int ci0 = blockIdx.x * HW_C, co0 = blockIdx.y * HW_C;
    const int last = a.o0 + (a.taps - 1) * a.ts, lo = min(a.o0, last), span = MAP ? a.taps * TM : TM + max(a.o0, last) - lo;
    float* Xs = hw_smem;
    float* Ds = hw_smem + span * HW_LD;
    const int Tmax = a.Lmax * a.mult;
    const bool with_bias = blockIdx.x == 0 && wr == 0;     // (uniform over the wave)

    f32x4 acc[MAXT];
    double sb = 0.0;                                       // the bias gradient: column r of dy over the rows k = q (mod 4), in double
#pragma unroll
    for (int j = 0; j < MAXT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int units = a.B * a.nchunk, u_end = min(((int)blockIdx.z + 1) * a.group, units);
    for (int unit = blockIdx.z * a.group; unit < u_end; ++unit) {
        const int b = unit / a.nchunk, chunk = unit - b * a.nchunk;
        const int T = MAP ? Tmax : min(a.lengths[b], a.Lmax) * a.mult, t_end = min((chunk + 1) * HW_ROWS, T);
        const float* ab = a.a + (MAP ? (a.Twav ? (size_t)b * a.Twav : (size_t)b * a.Hin * a.p * a.Ca) : (size_t)b * Tmax * a.Ca);
        const float* db = a.dy + (size_t)b * Tmax * a.Cd;
        for (int t0 = chunk * HW_ROWS; t0 < t_end; t0 += TM) {
            __syncthreads();                               // every wave is done with the previous tile
            if constexpr (MAP) {                           // [tap][64 rows]: the row map above, zero where the tap leaves [0, Hin) or the row the chunk
                for (int e = tid; e < span * (HW_C / 4); e += THREADS) {
                    const int sr = e / (HW_C / 4), k4 = (e - sr * (HW_C / 4)) * 4, j = sr / TM, n = t0 + sr - j * TM;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    int src;
                    if (n < t_end && ci0 + k4 < a.Ca && hd_source_row<false>(n, j, (a.taps - 1) / 2, a.p, a.s, a.Hin, &src)) {
                        if (a.Twav) {
                            v.x = hd_padded(ab, src, a.Twav);
                        } else {
                            v = *reinterpret_cast<const float4*>(ab + (size_t)src * a.Ca + ci0 + k4);
                            v.x = lrelu(v.x, a.slope); v.y = lrelu(v.y, a.slope); v.z = lrelu(v.z, a.slope); v.w = lrelu(v.w, a.slope);
                        }
                    }
                    *reinterpret_cast<float4*>(Xs + sr * HW_LD + k4) = v;
                }
            } else if (a.cf) {                             // channels-first source (the mel): consecutive threads along the rows
                for (int e = tid; e < span * HW_C; e += THREADS) {
                    const int c = e / span, row = e - c * span, t = t0 + lo + row;
                    Xs[row * HW_LD + c] = (t >= 0 && t < T && ci0 + c < a.Ca) ? lrelu(ab[(size_t)(ci0 + c) * Tmax + t], a.slope) : 0.f;
                }
            } else {
                for (int e = tid; e < span * (HW_C / 4); e += THREADS) {
                    const int row = e / (HW_C / 4), k4 = (e - row * (HW_C / 4)) * 4, t = t0 + lo + row;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (t >= 0 && t < T && ci0 + k4 < a.Ca) {
                        v = *reinterpret_cast<const float4*>(ab + (size_t)t * a.Ca + ci0 + k4);
                        v.x = lrelu(v.x, a.slope); v.y = lrelu(v.y, a.slope); v.z = lrelu(v.z, a.slope); v.w = lrelu(v.w, a.slope);
                    }
                    *reinterpret_cast<float4*>(Xs + row * HW_LD + k4) = v;
                }
            }
            if (a.Cd & 3) {                                // conv_post: one column
                for (int e = tid; e < TM * HW_C; e += THREADS) {
                    const int row = e / HW_C, c = e - row * HW_C, t = t0 + row;
                    Ds[row * HW_LD + c] = (t < t_end && co0 + c < a.Cd) ? db[(size_t)t * a.Cd + co0 + c] : 0.f;
                }
            } else {
                for (int e = tid; e < TM * (HW_C / 4); e += THREADS) {
                    const int row = e / (HW_C / 4), k4 = (e - row * (HW_C / 4)) * 4, t = t0 + row;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (t < t_end && co0 + k4 < a.Cd) v = *reinterpret_cast<const float4*>(db + (size_t)t * a.Cd + co0 + k4);
                    *reinterpret_cast<float4*>(Ds + row * HW_LD + k4) = v;
                }
            }
            __syncthreads();
            const int k_end = min(TM, (t_end - t0 + 3) & ~3);      // rows of dy beyond the chunk are zero
            const int tstep = MAP ? TM : a.ts;                     // rows between two taps of one output row in Xs
            const float* xa = Xs + (q + (MAP ? 0 : a.o0 - lo)) * HW_LD + wr * 16 + r;
            const float* da = Ds + q * HW_LD + wc * 16 + r;
            // this tile's chains start at zero: summing in blocks keeps the rounding error of thousands of rows near that of sqrt of them
            f32x4 part[MAXT];
#pragma unroll
            for (int j = 0; j < MAXT; ++j) part[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < k_end; k0 += 4) {
                const float bv = da[k0 * HW_LD];
#pragma unroll
                for (int j = 0; j < MAXT; ++j)
                    if (j < a.taps) part[j] = mfma4(xa[(k0 + j * tstep) * HW_LD], bv, part[j]);
                if (with_bias) sb += (double)bv;
            }
#pragma unroll
            for (int j = 0; j < MAXT; ++j) acc[j] += part[j];
        }
    }

    const int CiP = gridDim.x * HW_C, CoP = gridDim.y * HW_C;
    float* out = a.partial + (size_t)blockIdx.z * ((size_t)a.taps * CiP * CoP + CoP);
#pragma unroll
    for (int j = 0; j < MAXT; ++j)
        if (j < a.taps) {
#pragma unroll
            for (int i = 0; i < 4; ++i) out[((size_t)j * CiP + ci0 + wr * 16 + q * 4 + i) * CoP + co0 + wc * 16 + r] = acc[j][i];
        }
    if (with_bias) {                                       // (q0 + q1) + (q2 + q3): a column sum is a handful of numbers that nearly cancel, and a float32 chain
        sb += __shfl_xor(sb, 16);                          // over 1200 rows missed the bar on conv_post's single bias
        sb += __shfl_xor(sb, 32);
        if (q == 0) out[(size_t)a.taps * CiP * CoP + co0 + wc * 16 + r] = (float)sb;
    }
}

// One thread per element of a split's partial, in its order (coalesced reads); rate 0: dw [Cd][Ca][taps]; rate u: the view's column is (phase, output
// channel), its tap the row offset o0 + j: dw [Ca][Cout][k] with Cout = Cd / u.
__global__ __launch_bounds__(THREADS) void hifigan_wgrad_sum_kernel(const float* __restrict__ partial, float* __restrict__ dw, float* __restrict__ dbias, int splits,
                                                                    int taps, int Ca, int Cd, int CiP, int CoP, int o0, int rate, int k, float scale)
{
    const int64_t body = (int64_t)taps * CiP * CoP, P = body + CoP, e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= P) return;
    if (e >= body) {                                       // the bias: the phases of an output channel in ascending order
        const int co = (int)(e - body), u = rate ? rate : 1, Cout = Cd / u;
        if (co >= Cout || !dbias) return;
        double s = 0.0;
        for (int ph = 0; ph < u; ++ph)
            for (int z = 0; z < splits; ++z) s += (double)partial[(size_t)z * P + e + ph * Cout];
        dbias[co] = (float)s * scale;
        return;
    }
    const int n = (int)(e % CoP), ci = (int)((e / CoP) % CiP), j = (int)(e / ((int64_t)CoP * CiP));
    if (n >= Cd || ci >= Ca) return;
    size_t dst;
    if (rate == 0) {
        dst = ((size_t)n * Ca + ci) * taps + j;
    } else {
        const int Cout = Cd / rate, ph = n / Cout, co = n - ph * Cout;
        const int shift = ph + (k - rate) / 2, j0 = shift % rate, m = shift / rate - (o0 + j);
        if (m < 0 || j0 + m * rate >= k) return;           // this (phase, offset) pair has no tap
        dst = ((size_t)ci * Cout + co) * k + j0 + m * rate;
    }
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += partial[(size_t)z * P + e];
    dw[dst] = s * scale;
}

// ---- host side: the fixed partition ----
int hw_group(int Tmax) { return Tmax < HW_ROWS ? HW_ROWS / Tmax : 1; }
int hw_nchunk(int Tmax) { return (Tmax + HW_ROWS - 1) / HW_ROWS; }
int hw_splits(int B, int Tmax)
{
    const int64_t units = (int64_t)B * hw_nchunk(Tmax), g = hw_group(Tmax);
    return (int)((units + g - 1) / g);
}

// the grid of a weight gradient over B slabs of Tmax rows, Ca x Cd channels, and the floats of its partials: [splits][taps CiP CoP + CoP]
struct HwSizes {
    int splits, CiP, CoP;
    int64_t per_split, floats;
};
HwSizes hw_sizes(int B, int Tmax, int Ca, int Cd, int taps)
{
    HwSizes z;
    z.splits = hw_splits(B, Tmax);
    z.CiP = (Ca + HW_C - 1) / HW_C * HW_C;
    z.CoP = (Cd + HW_C - 1) / HW_C * HW_C;
    z.per_split = (int64_t)taps * z.CiP * z.CoP + z.CoP;
    z.floats = z.splits * z.per_split;
    return z;
}

// The launch pair of a weight gradient.  a: everything but nchunk and group, which follow from the rows; dw, dbias, rate, k, scale: the sum kernel's
// layout arguments (rate 0, k = taps: a convolution).  The kernel's accumulators come in buckets of taps: 3 / 7 / 11 for the generator's kernel sizes (and its
// views' few offsets), 3 / 5 under MAP, whose callers have no other.  Notes `hifigan_wgrad` + `hifigan_wgrad_sum`, MAP: `hifigan_disc_wgrad` + `.._sum`, MSD
// (the multi-scale discriminator's dense layers: MAP at period 1): `hifigan_msd_dense_wgrad` + `.._sum`.
template <bool MAP, bool MSD = false>
int hw_launch(HwArgs a, float* dw, float* dbias, int rate, int k, float scale, hipStream_t st)
{
    const int Tmax = a.Lmax * a.mult;
    const HwSizes z = hw_sizes(a.B, Tmax, a.Ca, a.Cd, a.taps);
    if (z.splits > 65535 || a.taps > (MAP ? 5 : HW_MAX_TAPS)) return GLOWTTS_E_ARG;
    a.nchunk = hw_nchunk(Tmax);
    a.group = hw_group(Tmax);
    const dim3 grid(z.CiP / HW_C, z.CoP / HW_C, z.splits);
    const int lds = ((MAP ? a.taps * TM : TM + (a.taps - 1) * a.ts) + TM) * HW_LD * 4;     // MAP with 5 taps: 6 x 64 rows, 73728 bytes, above the default limit
    int status;
    if (a.taps <= 3) status = hg_launch<&hifigan_wgrad_kernel<3, MAP>>(grid, lds, st, a);
    else if constexpr (MAP) status = hg_launch<&hifigan_wgrad_kernel<5, true>>(grid, lds, st, a);
    else if (a.taps <= 7) status = hg_launch<&hifigan_wgrad_kernel<7>>(grid, lds, st, a);
    else status = hg_launch<&hifigan_wgrad_kernel<HW_MAX_TAPS>>(grid, lds, st, a);
    if (status != GLOWTTS_OK) return status;
    GLOWTTS_NOTE_STATIC("%s", MSD ? "hifigan_msd_dense_wgrad" : MAP ? "hifigan_disc_wgrad" : "hifigan_wgrad");
    hipLaunchKernelGGL(hifigan_wgrad_sum_kernel, dim3((unsigned)((z.per_split + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, a.partial, dw, dbias, z.splits, a.taps,
                       a.Ca, a.Cd, z.CiP, z.CoP, a.o0, rate, k, scale);
    GLOWTTS_NOTE_STATIC("%s", MSD ? "hifigan_msd_dense_wgrad_sum" : MAP ? "hifigan_disc_wgrad_sum" : "hifigan_wgrad_sum");
    RET_LAUNCH();
}

}  // namespace
