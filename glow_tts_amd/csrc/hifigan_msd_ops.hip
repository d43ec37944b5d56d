// The HiFi-GAN multi-scale discriminator for gfx950, f32: forward, data backward and weight gradients (DESIGN.md "The multi-scale discriminator").  Scale 0
// sees the waveform [B][T], scale i the waveform after i average pools (4 taps, stride 2, zero padding 2, always divided by 4: T' = T / 2 + 1).  A scale's
// network is a stack of Conv1d over time with zero padding k / 2: a first layer 1 -> C0, grouped strided middle layers, a dense last layer and conv_post.
// Activations are channels-last per scale and layer, [B][L][C]; every batch row has the full length, tiles are counted from a batch row's own row 0 and every
// tap is masked by the row's own [0, L): a row's result does not depend on the batch around it, and nothing beyond the B L rows is read or written.  What is
// kept are PRE-activations: the LeakyReLU is the consumer's prologue and its mask is recomputed from them in the backward.  Every matrix product runs on
// v_mfma_f32_16x16x4_f32 (`mfma4`), no float atomics, no kernel waits on another workgroup, every sum has a fixed partition and order: every output is
// bit-identical from run to run.
//
//   hifigan_msd_pool         y[j] = (x[2 j - 2] + x[2 j - 1] + x[2 j] + x[2 j + 1]) / 4, samples outside [0, T) zero; one thread per output sample.
//   hifigan_msd_pool_bwd     the pool's gradient as a gather: sample n is read by the outputs n / 2 and n / 2 + 1 (where that exists), dx[n] = their sum / 4;
//                            written, or added to what dx holds (the scales add up from the coarsest to the finest).
//   hifigan_msd_first        1 -> C0, up to 15 taps, stride 1: one thread per (row, 4 channels); bias, then taps ascending on the VALU.
//   hifigan_msd_conv         the grouped strided convolution: the family's tile body `hg_tile` (hifigan_common.h) with its STRIDED SPAN row source.  One workgroup
//                            per (batch row, 64 output rows, group, RT NT 16 output columns of the group: `hg_by_layout(Cout_g)`).  It stages lrelu(x) of ONE
//                            contiguous span of 63 stride + k source rows of the group's Cin_g <= 64 channels (293 rows at stride 4 and 41 taps, about 80 KB at
//                            64 channels), zero outside [0, L); tap m of output row i reads LDS row i stride + m, against the group's K-major image
//                            [k Cin_g][Cout_g].  K loop, summation order and epilogue are the generator's text.
//   hifigan_msd_conv_bwd     its data gradient, the transposed convolution in polyphase form: input row n = i stride + ph receives only the taps
//                            m = r + j stride, r = (ph + k / 2) % stride, from output row i + (ph + k / 2) / stride - j.  A phase is a dense unit-stride
//                            product over ceil((k - r) / stride) taps: `hg_tile<.., BWD, false, GRP>` with tap step -1 on the rows, tap stride `stride` on the
//                            channel-transposed image [k][Cout_g][Cin_g padded to 16 columns] and the output phase (stride, ph); no zero row is multiplied.
//                            One launch: the phases are part of the grid.  Epilogue: y = sum * lrelu'(kept pre-activation) + injected * *inj_scale.
//   hifigan_msd_first_bwd    d wav of a scale: per sample t the transposed first layer, a gather; taps ascending, each a chain over the channels.
//   hifigan_msd_wgrad        dw[g][co][ci][m] = sum_t dy[t][g, co] lrelu(x[stride t + m - k / 2][g, ci]): the scheme of hifigan_wgrad.h under the strided
//                            span.  A workgroup owns 32 x 32 (ci, co) of one group and one split; per tile of 64 output rows it stages the 63 stride + k rows of
//                            x and the 64 rows of dy ONCE and takes every tap from them: tap m of row t is LDS row t stride + m.  Per (tile, tap) a chain from
//                            zero added to the tap's accumulator.  The fixed partition: per batch row chunks of 1024 output rows (short rows: 1024 / L batch
//                            rows per split); `hifigan_msd_wgrad_sum` adds the splits in ascending order into torch's layout [Cout][Cin_g][k].  The bias
//                            gradient: column sums of dy in double.
//   hifigan_msd_first_wgrad  the first layer's (Cin = 1): one lane per output channel, the waves take the rows of a chunk in turn, the taps are VALU chains;
//                            the waves' sums are added in wave order through LDS, the splits by `hifigan_msd_first_wgrad_sum`.
// The dense last layer (5 taps, stride 1), conv_post and their backwards and weight gradients are the multi-period discriminator's kernels at period 1
// (hifigan_disc_ops.hip: glowtts_hifigan_msd_dense* / _post*); feature matching is glowtts_hifigan_disc_fm unchanged.
#include "hifigan_common.h"
#include "hifigan_wgrad.h"

namespace {

constexpr int HM_MAX_TAPS = 41, HM_FIRST_TAPS = 15, HM_MAX_CHANNELS = 1024, HM_MAX_GROUP_IN = 64;

// ---- pool: grid (ceil(Tout / 256), B) ----
__global__ __launch_bounds__(THREADS) void hifigan_msd_pool_kernel(const float* __restrict__ x, float* __restrict__ y, int T, int Tout)
{
    const int b = blockIdx.y, j = blockIdx.x * THREADS + threadIdx.x;
    if (j >= Tout) return;
    const float* xb = x + (size_t)b * T;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = 2 * j - 2 + i;
        if (n >= 0 && n < T) s += xb[n];
    }
    y[(size_t)b * Tout + j] = s * 0.25f;
}

// ---- pool, backward: grid (ceil(T / 256), B) ----
__global__ __launch_bounds__(THREADS) void hifigan_msd_pool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int T, int Tout, int accumulate)
{
    const int b = blockIdx.y, n = blockIdx.x * THREADS + threadIdx.x;
    if (n >= T) return;
    const float* db = dy + (size_t)b * Tout;
    const int a = n >> 1;                                  // (a < Tout = T / 2 + 1 always)
    float g = db[a];
    if (a + 1 < Tout) g += db[a + 1];
    g *= 0.25f;
    const size_t at = (size_t)b * T + n;
    dx[at] = accumulate ? dx[at] + g : g;
}

// ---- first layer: grid (ceil(T C / 4 / 256), B).  w [k][C]: row = tap ----
__global__ __launch_bounds__(THREADS) void hifigan_msd_first_kernel(const float* __restrict__ wav, const float* __restrict__ w, const float* __restrict__ bias,
                                                                    float* __restrict__ out, int T, int k, int C)
{
    const int b = blockIdx.y, c4n = C >> 2, half = k >> 1;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t n = e / c4n;
    if (n >= T) return;
    const int c = (int)(e - n * c4n) * 4;
    const float* x = wav + (size_t)b * T;
    float4 acc = *reinterpret_cast<const float4*>(bias + c);
    for (int m = 0; m < k; ++m) {
        const int t = (int)n + m - half;
        if (t < 0 || t >= T) continue;
        const float xv = x[t];
        const float4 wv = *reinterpret_cast<const float4*>(w + m * C + c);
        acc.x = fmaf(wv.x, xv, acc.x); acc.y = fmaf(wv.y, xv, acc.y); acc.z = fmaf(wv.z, xv, acc.z); acc.w = fmaf(wv.w, xv, acc.w);
    }
    *reinterpret_cast<float4*>(out + ((size_t)b * T + n) * C + c) = acc;
}

// ---- first layer, backward: grid (ceil(T / 256), B).  dpre [B][T][C]; w [k][C] ----
__global__ __launch_bounds__(THREADS) void hifigan_msd_first_bwd_kernel(const float* __restrict__ dpre, const float* __restrict__ w, float* __restrict__ dwav, int T,
                                                                        int k, int C, int accumulate)
{
    const int b = blockIdx.y, t = blockIdx.x * THREADS + threadIdx.x, half = k >> 1;
    if (t >= T) return;
    const float* db = dpre + (size_t)b * T * C;
    float sum = 0.f;
    for (int m = 0; m < k; ++m) {
        const int n = t + half - m;                        // the output row whose tap m read sample t
        if (n < 0 || n >= T) continue;
        const float* g = db + (size_t)n * C;
        float ch = 0.f;
        for (int c = 0; c < C; c += 4) {
            const float4 gv = *reinterpret_cast<const float4*>(g + c), wv = *reinterpret_cast<const float4*>(w + m * C + c);
            ch = fmaf(gv.x, wv.x, ch); ch = fmaf(gv.y, wv.y, ch); ch = fmaf(gv.z, wv.z, ch); ch = fmaf(gv.w, wv.w, ch);
        }
        sum += ch;
    }
    const size_t at = (size_t)b * T + t;
    dwav[at] = accumulate ? dwav[at] + sum : sum;
}

// ---- first layer, weight gradient: grid (ceil(C / 64), splits); partial [splits][k + 1][C], row k: the bias ----
__global__ __launch_bounds__(THREADS) void hifigan_msd_first_wgrad_kernel(const float* __restrict__ wav, const float* __restrict__ dy, float* __restrict__ partial,
                                                                          int B, int T, int k, int C, int nchunk, int group)
{
    __shared__ float red[WAVES][HM_FIRST_TAPS][64];
    __shared__ double redb[WAVES][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, co = blockIdx.x * 64 + lane, half = k >> 1;
    const bool live = co < C;
    float acc[HM_FIRST_TAPS];
    double sb = 0.0;
#pragma unroll
    for (int m = 0; m < HM_FIRST_TAPS; ++m) acc[m] = 0.f;
    const int units = B * nchunk, u_end = min(((int)blockIdx.y + 1) * group, units);
    for (int unit = blockIdx.y * group; unit < u_end; ++unit) {
        const int b = unit / nchunk, chunk = unit - b * nchunk, t_end = min((chunk + 1) * HW_ROWS, T);
        const float* xb = wav + (size_t)b * T;
        const float* db = dy + (size_t)b * T * C;
        for (int t = chunk * HW_ROWS + wave; t < t_end; t += WAVES) {      // the waves take the rows in turn
            const float d = live ? db[(size_t)t * C + co] : 0.f;
            sb += (double)d;
#pragma unroll
            for (int m = 0; m < HM_FIRST_TAPS; ++m) {
                const int ts = t + m - half;
                if (m < k && ts >= 0 && ts < T) acc[m] = fmaf(d, xb[ts], acc[m]);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < HM_FIRST_TAPS; ++m) red[wave][m][lane] = acc[m];
    redb[wave][lane] = sb;
    __syncthreads();
    float* out = partial + (size_t)blockIdx.y * (k + 1) * C;
    for (int e = tid; e < (k + 1) * 64; e += THREADS) {    // the waves' sums in wave order
        const int m = e >> 6, l = e & 63, c = blockIdx.x * 64 + l;
        if (c >= C) continue;
        if (m < k) out[(size_t)m * C + c] = ((red[0][m][l] + red[1][m][l]) + red[2][m][l]) + red[3][m][l];
        else out[(size_t)k * C + c] = (float)(((redb[0][l] + redb[1][l]) + redb[2][l]) + redb[3][l]);
    }
}

// one thread per (tap or bias, channel): the splits in ascending order -> dw [C][1][k], dbias [C]
__global__ __launch_bounds__(THREADS) void hifigan_msd_first_wgrad_sum_kernel(const float* __restrict__ partial, float* __restrict__ dw, float* __restrict__ dbias,
                                                                              int splits, int k, int C)
{
    const int e = blockIdx.x * THREADS + threadIdx.x, P = (k + 1) * C;
    if (e >= P) return;
    const int m = e / C, c = e - m * C;
    if (m == k) {
        double s = 0.0;
        for (int z = 0; z < splits; ++z) s += (double)partial[(size_t)z * P + e];
        dbias[c] = (float)s;
        return;
    }
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += partial[(size_t)z * P + e];
    dw[(size_t)c * k + m] = s;
}

// ---- the grouped strided convolution and its data gradient ----
// Forward: grid (ceil(Ldst / 64), groups NdP / (RT NT 16), B); src [B][Lsrc][Cs] -> out [B][Ldst][Cd]; a group reads its Ks channels of src and writes its
// Nd (= NdP) channels of out; w [groups][k Ks][NdP], bias [Cd].  Dynamic LDS: 63 stride + k rows of lds_stride_of(min(Ks, 64)) floats.
// BWD: grid (ceil(ceil(Ldst / stride) / 64), stride groups NdP / (RT NT 16), B); src = dy [B][Lsrc][Cs] (d pre of the layer's output; a group reads its Ks
// output channels), out = dx [B][Ldst][Cd] (a group writes its Nd input channels, NdP = Nd rounded up to 16), w [groups][k][Ks][NdP] (columns from Nd on:
// zero); mask, inj laid out as out.  Dynamic LDS: 64 + ceil(k / stride) rows.
template <int RT, int NT, bool BWD>
__global__ __launch_bounds__(THREADS) void hifigan_msd_conv_kernel(const float* __restrict__ src, const float* __restrict__ w, const float* __restrict__ bias,
                                                                   const float* __restrict__ mask, const float* __restrict__ inj,
                                                                   const float* __restrict__ inj_scale, float* __restrict__ out, int Lsrc, int Ldst, int k,
                                                                   int stride, int groups, int Cs, int Cd, int Ks, int Nd, int NdP, float slope_in, float mslope)
{
    extern __shared__ __attribute__((aligned(16))) float hm_smem[];
    const int ncg = NdP / (RT * NT * 16), half = k >> 1;
    const int cg = blockIdx.y % ncg, gy = blockIdx.y / ncg, g = gy % groups, ph = gy / groups;     // (forward: ph = 0)
    const size_t out0 = (size_t)blockIdx.z * Ldst * Cd + (size_t)g * Nd;
    const float* sb = src + (size_t)blockIdx.z * Lsrc * Cs + (size_t)g * Ks;
    const float* wg = w + (size_t)g * k * Ks * NdP;
    if constexpr (BWD) {
        const int rows = (Ldst - ph + stride - 1) / stride;                    // input rows of this phase
        if ((int)blockIdx.x * TM >= rows) return;                              // (uniform over the workgroup)
        const int r = (ph + half) % stride, nt = r < k ? (k - r + stride - 1) / stride : 0;
        const HgTaps tp = {nt, (ph + half) / stride, -1, r, stride, Cs, 1};
        hg_tile<RT, NT, true, false, true>(sb, wg, nullptr, inj ? inj + out0 : nullptr, out + out0, hm_smem, Lsrc, rows, 0, blockIdx.x * TM, Ks, NdP, cg, tp, slope_in,
                                           0, stride, ph, 0, 1.f, mask + out0, mslope, inj ? inj_scale[0] : 0.f, Cd, Nd);
    } else {
        const HgTaps tp = {k, -half, 1, 0, 1, Cs, stride};
        hg_tile<RT, NT, false, false, true>(sb, wg, bias + (size_t)g * Nd, nullptr, out + out0, hm_smem, Lsrc, Ldst, 0, blockIdx.x * TM, Ks, NdP, cg, tp, slope_in, 0,
                                            1, 0, 0, 1.f, nullptr, 1.f, 0.f, Cd, Nd);
    }
}

// ---- the grouped weight gradient ----
struct HmWgrad {
    const float* x;            // [B][Lin][Cx]: the kept pre-activation of the layer's input
    const float* dy;           // [B][Lout][Cy]: d pre of its output
    float* partial;            // [splits][groups][k CiP CoP + CoP], CiP = 32 cib, CoP = 32 cob
    int B, Lin, Lout, Cx, Cy, Kx, Ky, k, stride, nchunk, group, cib, cob;
    float slope;
};

// grid (cib cob, groups, splits); dynamic LDS (63 stride + k + 64) rows of 48 floats
template <int MAXT>
__global__ __launch_bounds__(THREADS) void hifigan_msd_wgrad_kernel(const HmWgrad a)
{
    extern __shared__ __attribute__((aligned(16))) float hm_wsmem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int wr = wave & 1, wc = wave >> 1;               // the wave's tile: 16 channels of x, 16 of dy
    const int bx = blockIdx.x % a.cib, by = blockIdx.x / a.cib, g = blockIdx.y;
    const int ci0 = bx * HW_C, co0 = by * HW_C, half = a.k >> 1, span = (TM - 1) * a.stride + a.k;
    float* Xs = hm_wsmem;
    float* Ds = hm_wsmem + span * HW_LD;
    const bool with_bias = bx == 0 && wr == 0;             // (uniform over the wave)

    f32x4 acc[MAXT];
    double sb = 0.0;                                       // the bias gradient: column r of dy over the rows k = q (mod 4), in double
#pragma unroll
    for (int j = 0; j < MAXT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int units = a.B * a.nchunk, u_end = min(((int)blockIdx.z + 1) * a.group, units);
    for (int unit = blockIdx.z * a.group; unit < u_end; ++unit) {
        const int b = unit / a.nchunk, chunk = unit - b * a.nchunk, t_end = min((chunk + 1) * HW_ROWS, a.Lout);
        const float* xb = a.x + (size_t)b * a.Lin * a.Cx + (size_t)g * a.Kx;
        const float* db = a.dy + (size_t)b * a.Lout * a.Cy + (size_t)g * a.Ky;
        for (int t0 = chunk * HW_ROWS; t0 < t_end; t0 += TM) {
            __syncthreads();                               // every wave is done with the previous tile
            for (int e = tid; e < span * (HW_C / 4); e += THREADS) {           // the span of x: zero outside [0, Lin) and beyond the group's channels
                const int row = e / (HW_C / 4), k4 = (e - row * (HW_C / 4)) * 4, t = t0 * a.stride - half + row;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t >= 0 && t < a.Lin && ci0 + k4 < a.Kx) {
                    v = *reinterpret_cast<const float4*>(xb + (size_t)t * a.Cx + ci0 + k4);
                    v.x = lrelu(v.x, a.slope); v.y = lrelu(v.y, a.slope); v.z = lrelu(v.z, a.slope); v.w = lrelu(v.w, a.slope);
                }
                *reinterpret_cast<float4*>(Xs + row * HW_LD + k4) = v;
            }
            for (int e = tid; e < TM * (HW_C / 4); e += THREADS) {             // dy: zero beyond the chunk and beyond the group's channels
                const int row = e / (HW_C / 4), k4 = (e - row * (HW_C / 4)) * 4, t = t0 + row;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t < t_end && co0 + k4 < a.Ky) v = *reinterpret_cast<const float4*>(db + (size_t)t * a.Cy + co0 + k4);
                *reinterpret_cast<float4*>(Ds + row * HW_LD + k4) = v;
            }
            __syncthreads();
            const int k_end = min(TM, (t_end - t0 + 3) & ~3);      // rows of dy beyond the chunk are zero
            const float* xa = Xs + q * a.stride * HW_LD + wr * 16 + r;         // row (k0 + q) stride + tap
            const float* da = Ds + q * HW_LD + wc * 16 + r;
#pragma unroll
            for (int j = 0; j < MAXT; ++j)
                if (j < a.k) {                             // this (tile, tap)'s chain starts at zero (hifigan_wgrad.h)
                    f32x4 part = f32x4{0.f, 0.f, 0.f, 0.f};
                    for (int k0 = 0; k0 < k_end; k0 += 4) part = mfma4(xa[(k0 * a.stride + j) * HW_LD], da[k0 * HW_LD], part);
                    acc[j] += part;
                }
            if (with_bias)
                for (int k0 = 0; k0 < k_end; k0 += 4) sb += (double)da[k0 * HW_LD];
        }
    }

    const int CiP = a.cib * HW_C, CoP = a.cob * HW_C;
    float* out = a.partial + ((size_t)blockIdx.z * gridDim.y + g) * ((size_t)a.k * CiP * CoP + CoP);
#pragma unroll
    for (int j = 0; j < MAXT; ++j)
        if (j < a.k) {
#pragma unroll
            for (int i = 0; i < 4; ++i) out[((size_t)j * CiP + ci0 + wr * 16 + q * 4 + i) * CoP + co0 + wc * 16 + r] = acc[j][i];
        }
    if (with_bias) {                                       // (q0 + q1) + (q2 + q3)
        sb += __shfl_xor(sb, 16);
        sb += __shfl_xor(sb, 32);
        if (q == 0) out[(size_t)a.k * CiP * CoP + co0 + wc * 16 + r] = (float)sb;
    }
}

// grid (ceil(per / 256), groups): one thread per element of a split's partial, in its order; the splits ascending -> dw [groups Ky][Kx][k], dbias [groups Ky]
__global__ __launch_bounds__(THREADS) void hifigan_msd_wgrad_sum_kernel(const float* __restrict__ partial, float* __restrict__ dw, float* __restrict__ dbias,
                                                                        int splits, int k, int Kx, int Ky, int CiP, int CoP)
{
    const int64_t body = (int64_t)k * CiP * CoP, P = body + CoP, e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= P) return;
    const int g = blockIdx.y, groups = gridDim.y;
    const float* from = partial + (size_t)g * P + e;
    const size_t step = (size_t)groups * P;
    if (e >= body) {
        const int co = (int)(e - body);
        if (co >= Ky) return;
        double s = 0.0;
        for (int z = 0; z < splits; ++z) s += (double)from[z * step];
        dbias[g * Ky + co] = (float)s;
        return;
    }
    const int n = (int)(e % CoP), ci = (int)((e / CoP) % CiP), j = (int)(e / ((int64_t)CoP * CiP));
    if (n >= Ky || ci >= Kx) return;
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += from[z * step];
    dw[(((size_t)g * Ky + n) * Kx + ci) * k + j] = s;
}

// ---- host side ----
bool hm_width(int C) { return C >= 16 && C <= HM_MAX_CHANNELS && C % 16 == 0; }
bool hm_stride(int s) { return s == 1 || s == 2 || s == 4; }
bool hm_taps(int k, int most) { return k >= 1 && k <= most && (k & 1); }
int hm_rows_out(int L, int s) { return (L - 1) / s + 1; }
int hm_pad16(int C) { return (C + 15) / 16 * 16; }
// every batch row of the full length: B L <= 2^30 rows (a grid of one thread per row and four channels stays below 2^31 workgroups at 1024 channels)
bool hm_bad_rows(int B, int L) { return B < 1 || B > 65535 || L < 1 || (int64_t)B * L > ((int64_t)1 << 30); }
bool hm_grouped(int Cin, int Cout, int k, int stride, int groups)
{
    if (!hm_width(Cin) || !hm_width(Cout) || !hm_taps(k, HM_MAX_TAPS) || !hm_stride(stride) || groups < 1 || Cin % groups || Cout % groups) return false;
    const int Kx = Cin / groups, Ky = Cout / groups;
    return Ky % 16 == 0 && Kx % 4 == 0 && Kx <= HM_MAX_GROUP_IN;
}
int hm_conv_lds(int k, int stride, int Kx) { return ((TM - 1) * stride + k) * lds_stride_of(std::min(Kx, HG_CK)) * 4; }
int hm_bwd_lds(int k, int stride, int Ky) { return (TM + (k + stride - 1) / stride + 1) * lds_stride_of(std::min(Ky, HG_CK)) * 4; }
int hm_wgrad_lds(int k, int stride) { return ((TM - 1) * stride + k + TM) * HW_LD * 4; }
unsigned hm_quads(int64_t rows, int C) { return (unsigned)((rows * (C / 4) + THREADS - 1) / THREADS); }

struct HmSizes {
    int splits, cib, cob;
    int64_t per, floats;
};
HmSizes hm_sizes(int B, int Lout, int Kx, int Ky, int k, int groups)
{
    HmSizes z;
    z.splits = hw_splits(B, Lout);
    z.cib = (Kx + HW_C - 1) / HW_C;
    z.cob = (Ky + HW_C - 1) / HW_C;
    z.per = (int64_t)k * z.cib * HW_C * z.cob * HW_C + z.cob * HW_C;
    z.floats = (int64_t)z.splits * groups * z.per;
    return z;
}

}  // namespace

extern "C" int glowtts_hifigan_msd_supported(int Cin, int Cout, int taps, int stride, int groups)
{
    if (Cin == 1 && Cout == 1) return 0;
    if (Cin == 1) return hm_width(Cout) && hm_taps(taps, HM_FIRST_TAPS) && stride == 1 && groups == 1;
    if (Cout == 1) return hm_width(Cin) && taps == 3 && stride == 1 && groups == 1;
    if (groups == 1 && taps == 5 && stride == 1 && hm_width(Cin) && hm_width(Cout)) return 1;             // the dense layer (hifigan_disc_ops.hip)
    return hm_grouped(Cin, Cout, taps, stride, groups) && hm_conv_lds(taps, stride, Cin / groups) <= MAX_LDS &&
           hm_bwd_lds(taps, stride, Cout / groups) <= MAX_LDS && hm_wgrad_lds(taps, stride) <= MAX_LDS;
}

extern "C" int64_t glowtts_hifigan_msd_work_floats(int B, int rows_out, int Cin, int Cout, int taps, int groups)
{
    if (hm_bad_rows(B, rows_out) || groups < 1 || Cin < 1 || Cout < 1 || Cin % groups || Cout % groups || Cin > HM_MAX_CHANNELS || Cout > HM_MAX_CHANNELS ||
        !hm_taps(taps, HM_MAX_TAPS))
        return 0;
    const int64_t fm = 2 * (((int64_t)B * rows_out * Cout + 4095) / 4096);                 // glowtts_hifigan_disc_fm's float64 block sums on this layer's output
    const int64_t wg = Cin == 1 ? (int64_t)hw_splits(B, rows_out) * (taps + 1) * Cout : hm_sizes(B, rows_out, Cin / groups, Cout / groups, taps, groups).floats;
    return std::max(wg, fm);
}

extern "C" int glowtts_hifigan_msd_pool(const float* x, float* y, int B, int T, void* stream)
{
    if (!x || !y || x == y || hm_bad_rows(B, T)) return GLOWTTS_E_ARG;
    const int Tout = T / 2 + 1;
    GLOWTTS_NOTE_STATIC("hifigan_msd_pool");
    hipLaunchKernelGGL(hifigan_msd_pool_kernel, dim3((Tout + THREADS - 1) / THREADS, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), x, y, T, Tout);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_pool_bwd(const float* dy, float* dx, int B, int T, int accumulate, void* stream)
{
    if (!dy || !dx || dx == dy || accumulate < 0 || accumulate > 1 || hm_bad_rows(B, T)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("hifigan_msd_pool_bwd");
    hipLaunchKernelGGL(hifigan_msd_pool_bwd_kernel, dim3((T + THREADS - 1) / THREADS, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), dy, dx, T, T / 2 + 1,
                       accumulate);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_first(const float* wav, const float* w, const float* bias, float* out, int B, int T, int taps, int C, void* stream)
{
    if (!wav || !w || !bias || !out || hm_bad_rows(B, T) || !hm_taps(taps, HM_FIRST_TAPS) || !hm_width(C)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("hifigan_msd_first");
    hipLaunchKernelGGL(hifigan_msd_first_kernel, dim3(hm_quads(T, C), B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), wav, w, bias, out, T, taps, C);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_first_bwd(const float* dpre, const float* w, float* dwav, int B, int T, int taps, int C, int accumulate, void* stream)
{
    if (!dpre || !w || !dwav || accumulate < 0 || accumulate > 1 || hm_bad_rows(B, T) || !hm_taps(taps, HM_FIRST_TAPS) || !hm_width(C)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("hifigan_msd_first_bwd");
    hipLaunchKernelGGL(hifigan_msd_first_bwd_kernel, dim3((T + THREADS - 1) / THREADS, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), dpre, w, dwav, T, taps,
                       C, accumulate);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_first_wgrad(const float* wav, const float* dy, float* work, float* dw, float* dbias, int B, int T, int taps, int C, void* stream)
{
    if (!wav || !dy || !work || !dw || !dbias || hm_bad_rows(B, T) || !hm_taps(taps, HM_FIRST_TAPS) || !hm_width(C)) return GLOWTTS_E_ARG;
    const int splits = hw_splits(B, T);
    if (splits > 65535) return GLOWTTS_E_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLOWTTS_NOTE_STATIC("hifigan_msd_first_wgrad");
    hipLaunchKernelGGL(hifigan_msd_first_wgrad_kernel, dim3((C + 63) / 64, splits), dim3(THREADS), 0, st, wav, dy, work, B, T, taps, C, hw_nchunk(T), hw_group(T));
    GLOWTTS_NOTE_STATIC("hifigan_msd_first_wgrad_sum");
    hipLaunchKernelGGL(hifigan_msd_first_wgrad_sum_kernel, dim3(((taps + 1) * C + THREADS - 1) / THREADS), dim3(THREADS), 0, st, work, dw, dbias, splits, taps, C);
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_conv(const float* x, const float* w, const float* bias, float* out, int B, int L, int taps, int stride, int groups, int Cin,
                                        int Cout, float slope, void* stream)
{
    if (!x || !w || !bias || !out || x == out || hm_bad_rows(B, L) || !hm_grouped(Cin, Cout, taps, stride, groups)) return GLOWTTS_E_ARG;
    const int Kx = Cin / groups, Ky = Cout / groups, Lout = hm_rows_out(L, stride), lds = hm_conv_lds(taps, stride, Kx);
    if (lds > MAX_LDS) return GLOWTTS_E_ARG;
    const int status = hg_by_layout(Ky, [&](auto rt, auto nt) {
        constexpr int RT = decltype(rt)::value, NT = decltype(nt)::value;
        return hg_launch<&hifigan_msd_conv_kernel<RT, NT, false>>(dim3((Lout + TM - 1) / TM, groups * (Ky / (RT * NT * 16)), B), lds, static_cast<hipStream_t>(stream), x,
                                                                  w, bias, nullptr, nullptr, nullptr, out, L, Lout, taps, stride, groups, Cin, Cout, Kx, Ky, Ky, slope,
                                                                  1.f);
    });
    if (status != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_msd_conv");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_conv_bwd(const float* dy, const float* wt, const float* x, const float* inj, const float* inj_scale, float* dx, int B, int L,
                                            int taps, int stride, int groups, int Cin, int Cout, float slope, void* stream)
{
    if (!dy || !wt || !x || !dx || dx == dy || dx == x || (inj && !inj_scale) || hm_bad_rows(B, L) || !hm_grouped(Cin, Cout, taps, stride, groups))
        return GLOWTTS_E_ARG;
    const int Kx = Cin / groups, Ky = Cout / groups, KxP = hm_pad16(Kx), Lout = hm_rows_out(L, stride), lds = hm_bwd_lds(taps, stride, Ky);
    if (lds > MAX_LDS) return GLOWTTS_E_ARG;
    const int rows = (L + stride - 1) / stride;            // the input rows of phase 0, the longest
    const int status = hg_by_layout(KxP, [&](auto rt, auto nt) {
        constexpr int RT = decltype(rt)::value, NT = decltype(nt)::value;
        return hg_launch<&hifigan_msd_conv_kernel<RT, NT, true>>(dim3((rows + TM - 1) / TM, stride * groups * (KxP / (RT * NT * 16)), B), lds,
                                                                 static_cast<hipStream_t>(stream), dy, wt, nullptr, x, inj, inj_scale, dx, Lout, L, taps, stride, groups,
                                                                 Cout, Cin, Ky, Kx, KxP, 1.f, slope);
    });
    if (status != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("hifigan_msd_conv_bwd");
    RET_LAUNCH();
}

extern "C" int glowtts_hifigan_msd_wgrad(const float* x, const float* dy, float* work, float* dw, float* dbias, int B, int L, int taps, int stride, int groups,
                                         int Cin, int Cout, float slope, void* stream)
{
    if (!x || !dy || !work || !dw || !dbias || hm_bad_rows(B, L) || !hm_grouped(Cin, Cout, taps, stride, groups)) return GLOWTTS_E_ARG;
    const int Kx = Cin / groups, Ky = Cout / groups, Lout = hm_rows_out(L, stride), lds = hm_wgrad_lds(taps, stride);
    const HmSizes z = hm_sizes(B, Lout, Kx, Ky, taps, groups);
    if (z.splits > 65535 || groups > 65535 || lds > MAX_LDS) return GLOWTTS_E_ARG;
    const HmWgrad a = {x, dy, work, B, L, Lout, Cin, Cout, Kx, Ky, taps, stride, hw_nchunk(Lout), hw_group(Lout), z.cib, z.cob, slope};
    const dim3 grid(z.cib * z.cob, groups, z.splits);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int status = taps <= 15 ? hg_launch<&hifigan_msd_wgrad_kernel<15>>(grid, lds, st, a) : hg_launch<&hifigan_msd_wgrad_kernel<HM_MAX_TAPS>>(grid, lds, st, a);
    if (status != GLOWTTS_OK) return status;
    GLOWTTS_NOTE_STATIC("hifigan_msd_wgrad");
    hipLaunchKernelGGL(hifigan_msd_wgrad_sum_kernel, dim3((unsigned)((z.per + THREADS - 1) / THREADS), groups), dim3(THREADS), 0, st, work, dw, dbias, z.splits, taps,
                       Kx, Ky, z.cib * HW_C, z.cob * HW_C);
    GLOWTTS_NOTE_STATIC("hifigan_msd_wgrad_sum");
    RET_LAUNCH();
}
