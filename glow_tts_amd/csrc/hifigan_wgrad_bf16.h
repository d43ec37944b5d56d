// The bf16 weight-gradient kernel of the HiFi-GAN family, shared by the generator's mixed-precision mode (hifigan_mixed_ops.hip) and the multi-period
// discriminator's bf16 mode (hifigan_disc_bf16_ops.hip): hifigan_wgrad.h's partition, 32 x 32 workgroup tile, partial layout and sum kernel, with both MFMA
// operands rounded to bf16 and read through the transposed LDS read.  The head of hifigan_mixed_ops.hip describes the tile.  As in hifigan_wgrad.h there are
// two ways to reach the rows of x that a tap reads:
//   MAP = false  the generator: the tile stages one contiguous span of rows and tap j shifts the row index by j ts.
//   MAP = true   the discriminator: the tile stages the 64 rows of EVERY tap, [taps][64] rows of 40 bf16 through `hd_source_row<false>`, and tap j's operand
//                starts j * 64 rows further on.  A row outside [0, Hin), or beyond the chunk, is staged as ZEROS: ds_read_tr16_b64 needs EXEC all ones, so
//                the mask is never a branch around the read.  (The waveform source of the first layer stays with the f32 kernel.)
// Every MAP term is a compile-time branch: the <MAXT, false> instantiations are the code they were.
#pragma once
#include "hifigan_wgrad.h"

namespace {

constexpr int HWB_LD = 40;                                 // bf16 per LDS row of the weight gradient: 32 channels + 16 bytes
constexpr int HWB_BIAS_BYTES = 32 * HW_C * 8;              // the bias gradient's [32 row groups][32 columns] doubles

typedef short s16x4 __attribute__((ext_vector_type(4)));

// one MFMA operand: rows p .. p + 7 (LDS rows) of 16 channels, transposed; every lane of the wave supplies an address (EXEC all ones)
__device__ __forceinline__ Chunk16 hwb_frag(const uint16_t* p)
{
    s16x4 v[2] = {__builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p)),
                  __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p + 4 * HWB_LD))};
    return *reinterpret_cast<Chunk16*>(v);
}

// grid (ceil(Ca / 32), ceil(Cd / 32), splits); dynamic LDS (64 + reach + 64) rows of 40 bf16 (MAP: (taps 64 + 64) rows), then the bias gradient's doubles
template <int MAXT, bool MAP = false>
__global__ __launch_bounds__(THREADS) void hifigan_wgrad_bf16_kernel(const HwArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t hwb_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int wr = wave & 1, wc = wave >> 1;               // the wave's tile: 16 channels of x, 16 of dy
    const int ci0 = blockIdx.x * HW_C, co0 = blockIdx.y * HW_C;
    const int last = a.o0 + (a.taps - 1) * a.ts, lo = min(a.o0, last), span = MAP ? a.taps * TM : TM + max(a.o0, last) - lo;
    uint16_t* Xs = hwb_smem;
    uint16_t* Ds = hwb_smem + span * HWB_LD;
    const int Tmax = a.Lmax * a.mult;
    const bool with_bias = blockIdx.x == 0;                // (uniform over the workgroup)
    const int srow = tid >> 3, sk4 = (tid & 7) * 4;        // the staging thread's rows srow, srow + 32, .. and its four channels

    f32x4 acc[MAXT];
    double sb[4] = {0.0, 0.0, 0.0, 0.0};                   // the bias gradient: this thread's four columns of the unrounded dy, in double
#pragma unroll
    for (int j = 0; j < MAXT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int units = a.B * a.nchunk, u_end = min(((int)blockIdx.z + 1) * a.group, units);
    for (int unit = blockIdx.z * a.group; unit < u_end; ++unit) {
        const int b = unit / a.nchunk, chunk = unit - b * a.nchunk;
        int T;
        if constexpr (MAP) T = Tmax; else T = min(a.lengths[b], a.Lmax) * a.mult;
        const int t_end = min((chunk + 1) * HW_ROWS, T);
        const float* ab = a.a + (MAP ? (size_t)b * a.Hin * a.p * a.Ca : (size_t)b * Tmax * a.Ca);
        const float* db = a.dy + (size_t)b * Tmax * a.Cd;
        for (int t0 = chunk * HW_ROWS; t0 < t_end; t0 += TM) {
            __syncthreads();                               // every wave is done with the previous tile
            if constexpr (MAP) {                           // [tap][64 rows]: the row map, zeros where the tap leaves [0, Hin) or the row the chunk
                for (int row = srow; row < span; row += THREADS / 8) {
                    const int j = row / TM, n = t0 + row - j * TM;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    int src;
                    if (n < t_end && ci0 + sk4 < a.Ca && hd_source_row<false>(n, j, (a.taps - 1) / 2, a.p, a.s, a.Hin, &src)) {
                        v = *reinterpret_cast<const float4*>(ab + (size_t)src * a.Ca + ci0 + sk4);
                        v.x = lrelu(v.x, a.slope); v.y = lrelu(v.y, a.slope); v.z = lrelu(v.z, a.slope); v.w = lrelu(v.w, a.slope);
                    }
                    *reinterpret_cast<u32x2*>(Xs + row * HWB_LD + sk4) = u32x2{pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
                }
            } else if (a.cf) {                             // channels-first source (the mel): consecutive threads along the rows
                for (int e = tid; e < span * HW_C; e += THREADS) {
                    const int c = e / span, row = e - c * span, t = t0 + lo + row;
                    Xs[row * HWB_LD + c] = (t >= 0 && t < T && ci0 + c < a.Ca) ? bf16_bits(lrelu(ab[(size_t)(ci0 + c) * Tmax + t], a.slope)) : (uint16_t)0;
                }
            } else {
                for (int row = srow; row < span; row += THREADS / 8) {
                    const int t = t0 + lo + row;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (t >= 0 && t < T && ci0 + sk4 < a.Ca) {
                        v = *reinterpret_cast<const float4*>(ab + (size_t)t * a.Ca + ci0 + sk4);
                        v.x = lrelu(v.x, a.slope); v.y = lrelu(v.y, a.slope); v.z = lrelu(v.z, a.slope); v.w = lrelu(v.w, a.slope);
                    }
                    *reinterpret_cast<u32x2*>(Xs + row * HWB_LD + sk4) = u32x2{pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
                }
            }
            for (int row = srow; row < TM; row += THREADS / 8) {
                const int t = t0 + row;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t < t_end && co0 + sk4 < a.Cd) v = *reinterpret_cast<const float4*>(db + (size_t)t * a.Cd + co0 + sk4);
                *reinterpret_cast<u32x2*>(Ds + row * HWB_LD + sk4) = u32x2{pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
                if (with_bias) {
                    sb[0] += (double)v.x; sb[1] += (double)v.y; sb[2] += (double)v.z; sb[3] += (double)v.w;
                }
            }
            __syncthreads();
            const int k_end = min(TM, (t_end - t0 + 31) & ~31);    // rows of dy beyond the chunk are zero (uniform over the workgroup)
            const int tstep = MAP ? TM : a.ts;                     // rows between two taps of one output row in Xs
            // lane 4 q' + p of a 16-lane group supplies row q', channels 4 p .. 4 p + 3 of the group's 4 x 16 block; the group l >> 4 takes k = 8 (l >> 4) ..
            const uint16_t* xa = Xs + (8 * q + (r >> 2) + (MAP ? 0 : a.o0 - lo)) * HWB_LD + wr * 16 + 4 * (r & 3);
            const uint16_t* da = Ds + (8 * q + (r >> 2)) * HWB_LD + wc * 16 + 4 * (r & 3);
            f32x4 part[MAXT];                              // this tile's chains start at zero
#pragma unroll
            for (int j = 0; j < MAXT; ++j) part[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < k_end; k0 += 32) {
                const Chunk16 bv = hwb_frag(da + k0 * HWB_LD);
#pragma unroll
                for (int j = 0; j < MAXT; ++j)
                    if (j < a.taps) part[j] = mfma16_bf16(hwb_frag(xa + (k0 + j * tstep) * HWB_LD), bv, part[j]);      // (uniform)
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
    if (with_bias) {                                       // the 32 row groups of a column in ascending order
        double* Bs = reinterpret_cast<double*>(hwb_smem + (span + TM) * HWB_LD);
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[srow * HW_C + sk4 + i] = sb[i];
        __syncthreads();
        if (tid < HW_C) {
            double s = 0.0;
            for (int g = 0; g < THREADS / 8; ++g) s += Bs[g * HW_C + tid];
            out[(size_t)a.taps * CiP * CoP + co0 + tid] = (float)s;
        }
    }
}

// reach: the rows a tile stages beyond its 64 (span: (taps - 1) |ts|; MAP: (taps - 1) 64)
int hwb_lds_bytes(int reach) { return (TM + reach + TM) * HWB_LD * 2 + HWB_BIAS_BYTES; }

}  // namespace
