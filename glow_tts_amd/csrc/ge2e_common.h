// What the GE2E speaker encoder's inference (ge2e_ops.hip) and training (ge2e_train_ops.hip) share: the tile constants, the packed image's geometry,
// ONE LSTM cell kernel and its diagonal launch loop, and the head projection.  The training forward is the inference forward bit for bit
// because both are instantiations of the text below: every arithmetic expression of the cell and of the head's sum is spelled exactly once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glowtts_hip.h"
#include "device_common.h"
#include "launch_log.h"

namespace {

constexpr int TM = 16;                                    // sequences (rows) per workgroup: one MFMA tile
constexpr int TU = 16;                                    // hidden units per workgroup (x 4 gates = 64 image columns)
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int RED_FLOATS = WAVES * 4 * TM * TU;           // the waves' partial gate sums

__host__ __device__ __forceinline__ int64_t image_offset(int layer, int Mel, int H)
{
    return layer == 0 ? 0 : ((int64_t)(Mel + H) + (int64_t)(layer - 1) * 2 * H) * 4 * H;
}
int cell_lds_bytes(int Mel, int H) { return (TM * lds_stride_of(Mel > H ? Mel + H : 2 * H) + RED_FLOATS) * 4; }

// ---- one diagonal of cells.  dynamic LDS: As [16][as] | red [WAVES][4][16 x 16] ---------------------------------------------------------------------
// KEEP selects only where c lives and whether the activated gates are stored:
//   KEEP == false (inference)  c [Stacks][N][H], updated in place; `gates` is not used
//   KEEP == true  (training)   c [Stacks][N][T][H] kept whole, gates [Stacks][N][T][4 H] in the image's column order (64 s + 4 u + g: one 16-byte store per unit)
template <bool KEEP>
__global__ __launch_bounds__(THREADS) void ge2e_cell_kernel(const float* __restrict__ x, const float* __restrict__ images, const float* __restrict__ biases,
                                                            float* __restrict__ hs, float* __restrict__ cs, int N, int Mel, int T, int H, int d, int kmin,
                                                            float* __restrict__ gates)
{
    extern __shared__ __attribute__((aligned(16))) float ge2e_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int k = kmin + blockIdx.z, t = d - k;            // the cell (uniform over the workgroup)
    const int s = blockIdx.x, n0 = blockIdx.y * TM;
    const int in = k == 0 ? Mel : H, K = in + H, G = 4 * H;
    const int as = lds_stride_of(K);
    float* As = ge2e_smem;
    float* red = ge2e_smem + TM * lds_stride_of(Mel > H ? Mel + H : 2 * H);      // (the same offset in every launch)
    const size_t layer_rows = (size_t)N * T;               // rows of one layer of hs

    // 1. gather [input | h_prev] of the tile's rows; rows beyond N and h_{-1} are zero
    if (k == 0) {
        for (int e = tid; e < TM * Mel; e += THREADS) {
            const int row = e / Mel, m = e - row * Mel, n = n0 + row;
            As[row * as + m] = n < N ? x[((size_t)n * Mel + m) * T + t] : 0.f;
        }
    } else {
        const int hq = H >> 2;
        for (int e = tid; e < TM * hq; e += THREADS) {
            const int row = e / hq, j4 = (e - row * hq) * 4, n = n0 + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < N) v = *reinterpret_cast<const float4*>(hs + (((size_t)(k - 1) * layer_rows + (size_t)n * T + t) * H + j4));
            *reinterpret_cast<float4*>(As + row * as + j4) = v;
        }
    }
    {
        const int hq = H >> 2;
        for (int e = tid; e < TM * hq; e += THREADS) {
            const int row = e / hq, j4 = (e - row * hq) * 4, n = n0 + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < N && t > 0) v = *reinterpret_cast<const float4*>(hs + (((size_t)k * layer_rows + (size_t)n * T + (t - 1)) * H + j4));
            *reinterpret_cast<float4*>(As + row * as + in + j4) = v;
        }
    }
    __syncthreads();

    // 2. the four gates of 16 units for 16 rows; wave w owns the k steps w, w + 4, ...
    const float* img = images + image_offset(k, Mel, H) + (size_t)s * 64 + r * 4;
    const float* aa = As + r * as + q;
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k0 = 4 * wave; k0 < K; k0 += 4 * WAVES) {
        const float4 w = *reinterpret_cast<const float4*>(img + (size_t)(k0 + q) * G);
        const float a = aa[k0];
        acc[0] = mfma4(a, w.x, acc[0]);
        acc[1] = mfma4(a, w.y, acc[1]);
        acc[2] = mfma4(a, w.z, acc[2]);
        acc[3] = mfma4(a, w.w, acc[3]);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[((wave * 4 + g) * TM + q * 4 + i) * TU + r] = acc[g][i];
    __syncthreads();

    // 3. thread (row, unit): fixed-order sum, gates, c, h
    const int row = tid >> 4, u = tid & 15, n = n0 + row;
    if (n >= N) return;
    const int j = s * TU + u;
    const float4 b = *reinterpret_cast<const float4*>(biases + (size_t)k * G + s * 64 + u * 4);
    float pre[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int w = 0; w < WAVES; ++w)
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] += red[((w * 4 + g) * TM + row) * TU + u];
    const size_t cell = (size_t)k * layer_rows + (size_t)n * T + t;
    float* cp = cs + (KEEP ? cell : (size_t)k * N + n) * H + j;
    const float c_prev = t > 0 ? *(KEEP ? cp - H : cp) : 0.f;
    const float gf = sigmoidf_(pre[1]), gi = sigmoidf_(pre[0]), gg = tanhf(pre[2]);
    const float c = fmaf(gf, c_prev, gi * gg);             // one rounding of f c: written out, not left to the compiler's contraction
    *cp = c;
    const float go = sigmoidf_(pre[3]);
    hs[cell * H + j] = go * tanhf(c);
    if (KEEP) *reinterpret_cast<float4*>(gates + cell * G + s * 64 + u * 4) = make_float4(gi, gf, gg, go);
}

// The diagonal wavefront: launch dg computes every cell (layer k, step t = dg - k); T + Stacks - 1 launches whose order on the stream is the only
// synchronisation.  The caller has checked the shapes.
template <bool KEEP>
int ge2e_launch_cells(const float* x, const float* images, const float* biases, float* hs, float* cs, float* gates, int N, int Mel, int T, int H, int Stacks,
                      hipStream_t s)
{
    const int lds = cell_lds_bytes(Mel, H);
    static int allowed = 0;                                // (grows monotonically; a racing second caller sets the same or a larger value)
    if (lds > allowed) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&ge2e_cell_kernel<KEEP>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
            return GLOWTTS_E_LAUNCH;
        allowed = lds;
    }
    for (int dg = 0; dg < T + Stacks - 1; ++dg) {
        const int kmin = dg - (T - 1) > 0 ? dg - (T - 1) : 0, kmax = dg < Stacks - 1 ? dg : Stacks - 1;
        hipLaunchKernelGGL(ge2e_cell_kernel<KEEP>, dim3(H / TU, (N + TM - 1) / TM, kmax - kmin + 1), dim3(THREADS), (size_t)lds, s, x, images, biases, hs, cs, N, Mel, T,
                           H, dg, kmin, gates);
        GLOWTTS_NOTE_STATIC("ge2e_cell");
    }
    return GLOWTTS_OK;
}

// The head projection of one sequence: stages h = h_{T-1}^{top} into hl [H] (LDS), then e_j = W_j . h + b_j with a wave per output, lanes over H and the fixed
// shuffle tree; lane 0 of the owning wave hands (j, e_j) to `store`.  Called by the whole workgroup (it holds a barrier); w [E][H], bias [E] are torch.nn.Linear's.
template <typename Store>
__device__ __forceinline__ void ge2e_head_project(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ bias, float* hl, int H, int E,
                                                  Store store)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < H; j += THREADS) hl[j] = h[j];
    __syncthreads();
    for (int j = wave; j < E; j += WAVES) {
        float p = 0.f;
        for (int kk = lane; kk < H; kk += 64) p = fmaf(w[(size_t)j * H + kk], hl[kk], p);
        p = wave_sum(p) + bias[j];
        if (lane == 0) store(j, p);
    }
}

}  // namespace
