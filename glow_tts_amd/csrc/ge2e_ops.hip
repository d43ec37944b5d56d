// GE2E speaker encoder (DESIGN.md "GE2E speaker encoder"): a stack of LSTM layers over mel slices, a linear head and the d-vector normalisation, for
// gfx950, forward only (the encoder is pre-trained and detached), f32.  torch.nn.LSTM's definition: gates i, f, g, o, bias b_ih + b_hh, h0 = c0 = 0.
//
//   ge2e_pack   one launch per layer at load: W_ih | W_hh -> ONE K-major image [in + H][4 H] (rows: the layer's input channels, then its own hidden units) and the
//               summed bias [4 H].  Column order: hidden unit j = 16 s + u, gate g -> column 64 s + 4 u + g, so that a slice s of 16 units owns 64 adjacent columns,
//               all four gates of a unit are one 16-byte load, and the c update needs nothing from another workgroup.
//   ge2e_cell   a diagonal wavefront: launch d computes every cell (layer k, step t = d - k).  Such a cell reads h^{k-1}_t, h^k_{t-1} and c^k_{t-1}, all written
//               by launch d - 1, and h is kept whole ([Stacks][N][T][H]): no kernel waits on another workgroup, there is no flag, barrier or cooperative launch;
//               the order of the launches on the stream is the only synchronisation.  T + Stacks - 1 launches.
//               grid (H / 16 unit slices, ceil(N / 16) sequence tiles, cells on the diagonal), 256 threads.  A workgroup gathers its 16 rows [input | h_prev]
//               (layer 0: x[n][:][t] read in place) into LDS, its four waves split the K range (k step 4 (w + 4 i): a fixed partition), each running
//               v_mfma_f32_16x16x4_f32 for the four gates against the image streamed from L2; the partial sums meet in LDS and thread (row, unit) adds them in
//               the fixed order bias + w0 + w1 + w2 + w3, applies the gates (expf / tanhf, not the fast intrinsics), updates c in place and writes h.
//               A row's sums never involve another row (an MFMA row depends on its own A row only): a sequence's values are the same in any batch.
//   ge2e_head   one workgroup per utterance: e = W h_{T-1}^{top} + b per slice (a wave per output, lanes over H, fixed shuffle tree), w = e / max(|e|, 1e-12),
//               d = normalize(mean over the utterance's slices of w).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glowtts_hip.h"
#include "launch_log.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int TM = 16;                                    // sequences (rows) per workgroup: one MFMA tile
constexpr int TU = 16;                                    // hidden units per workgroup (x 4 gates = 64 image columns)
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_LDS = 160 * 1024;
constexpr int RED_FLOATS = WAVES * 4 * TM * TU;           // the waves' partial gate sums

__device__ __forceinline__ v4f mfma4(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

__host__ __device__ __forceinline__ int as_stride_of(int K) { return ((K >> 2) & 1) ? K : K + 4; }      // (stride / 4) odd: 16 rows x 4 k hit distinct banks
__host__ __device__ __forceinline__ int64_t image_offset(int layer, int Mel, int H)
{
    return layer == 0 ? 0 : ((int64_t)(Mel + H) + (int64_t)(layer - 1) * 2 * H) * 4 * H;
}

// ---- pack: grid (ceil((in + H) * 4 H / 256)) -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void ge2e_pack_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                                                            const float* __restrict__ b_hh, float* __restrict__ image, float* __restrict__ bias, int in, int H)
{
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int G = 4 * H;
    if (e >= (int64_t)(in + H) * G) return;
    const int kk = (int)(e / G), col = (int)(e - (int64_t)kk * G);
    const int s = col >> 6, u = (col >> 2) & 15, g = col & 3;
    const int row = g * H + s * TU + u;                    // torch's row: gate-major
    image[e] = kk < in ? w_ih[(size_t)row * in + kk] : w_hh[(size_t)row * H + (kk - in)];
    if (kk == 0) bias[col] = b_ih[row] + b_hh[row];
}

// ---- one diagonal of cells.  dynamic LDS: As [16][as] | red [WAVES][4][16 x 16] ---------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void ge2e_cell_kernel(const float* __restrict__ x, const float* __restrict__ images, const float* __restrict__ biases,
                                                            float* __restrict__ hs, float* __restrict__ cs, int N, int Mel, int T, int H, int d, int kmin)
{
    extern __shared__ __attribute__((aligned(16))) float ge2e_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int k = kmin + blockIdx.z, t = d - k;            // the cell (uniform over the workgroup)
    const int s = blockIdx.x, n0 = blockIdx.y * TM;
    const int in = k == 0 ? Mel : H, K = in + H, G = 4 * H;
    const int as = as_stride_of(K);
    float* As = ge2e_smem;
    float* red = ge2e_smem + TM * as_stride_of(Mel > H ? Mel + H : 2 * H);      // (the same offset in every launch)
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
    v4f acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = v4f{0.f, 0.f, 0.f, 0.f};
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

    // 3. thread (row, unit): fixed-order sum, gates, c in place, h
    const int row = tid >> 4, u = tid & 15, n = n0 + row;
    if (n >= N) return;
    const int j = s * TU + u;
    const float4 b = *reinterpret_cast<const float4*>(biases + (size_t)k * G + s * 64 + u * 4);
    float pre[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int w = 0; w < WAVES; ++w)
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] += red[((w * 4 + g) * TM + row) * TU + u];
    float* cp = cs + ((size_t)k * N + n) * H + j;
    const float c_prev = t > 0 ? *cp : 0.f;
    const float c = sigmoidf_(pre[1]) * c_prev + sigmoidf_(pre[0]) * tanhf(pre[2]);
    *cp = c;
    hs[((size_t)k * layer_rows + (size_t)n * T + t) * H + j] = sigmoidf_(pre[3]) * tanhf(c);
}

// ---- head: grid (B), dynamic LDS hl [H] | es [E] | sc [2].  w [E][H], bias [E] are torch.nn.Linear's own ------------------------------------------------
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);      // a fixed tree: every lane ends with the same value
    return v;
}

__global__ __launch_bounds__(THREADS) void ge2e_head_kernel(const float* __restrict__ h_top, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ e_out, float* __restrict__ d_out, int Samples, int T, int H, int E)
{
    extern __shared__ __attribute__((aligned(16))) float ge2e_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    float* hl = ge2e_smem;
    float* es = hl + H;
    float* sc = es + E;
    float mean[GLOWTTS_GE2E_MAX_E / THREADS];               // output j = tid + 256 i of this thread
#pragma unroll
    for (int i = 0; i < GLOWTTS_GE2E_MAX_E / THREADS; ++i) mean[i] = 0.f;
    for (int sl = 0; sl < Samples; ++sl) {
        const size_t n = (size_t)b * Samples + sl;
        __syncthreads();                                   // the previous slice's hl / es / sc are read no more
        for (int j = tid; j < H; j += THREADS) hl[j] = h_top[(n * T + (T - 1)) * H + j];
        __syncthreads();
        for (int j = wave; j < E; j += WAVES) {
            float p = 0.f;
            for (int kk = lane; kk < H; kk += 64) p = fmaf(w[(size_t)j * H + kk], hl[kk], p);
            p = wave_sum(p) + bias[j];
            if (lane == 0) {
                es[j] = p;
                if (e_out) e_out[n * E + j] = p;
            }
        }
        __syncthreads();
        if (wave == 0) {
            float p = 0.f;
            for (int j = lane; j < E; j += 64) p = fmaf(es[j], es[j], p);
            p = wave_sum(p);
            if (lane == 0) sc[0] = fmaxf(sqrtf(p), 1e-12f);
        }
        __syncthreads();
        const float norm = sc[0];
#pragma unroll
        for (int i = 0; i < GLOWTTS_GE2E_MAX_E / THREADS; ++i) {
            const int j = tid + i * THREADS;
            if (j < E) mean[i] += es[j] / norm;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < GLOWTTS_GE2E_MAX_E / THREADS; ++i) {
        const int j = tid + i * THREADS;
        if (j < E) es[j] = mean[i] = mean[i] / (float)Samples;
    }
    __syncthreads();
    if (wave == 0) {
        float p = 0.f;
        for (int j = lane; j < E; j += 64) p = fmaf(es[j], es[j], p);
        p = wave_sum(p);
        if (lane == 0) sc[1] = fmaxf(sqrtf(p), 1e-12f);
    }
    __syncthreads();
    const float norm = sc[1];
#pragma unroll
    for (int i = 0; i < GLOWTTS_GE2E_MAX_E / THREADS; ++i) {
        const int j = tid + i * THREADS;
        if (j < E) d_out[(size_t)b * E + j] = mean[i] / norm;
    }
}

int cell_lds_bytes(int Mel, int H) { return (TM * as_stride_of(Mel > H ? Mel + H : 2 * H) + RED_FLOATS) * 4; }

}  // namespace

extern "C" int glowtts_ge2e_supported(int Mel, int H, int Stacks, int E)
{
    return Mel >= 4 && Mel % 4 == 0 && Mel <= GLOWTTS_GE2E_MAX_MEL && H >= 16 && H % 16 == 0 && H <= GLOWTTS_GE2E_MAX_H && Stacks >= 1 &&
           Stacks <= GLOWTTS_GE2E_MAX_STACKS && E >= 1 && E <= GLOWTTS_GE2E_MAX_E && cell_lds_bytes(Mel, H) <= MAX_LDS;
}

extern "C" int64_t glowtts_ge2e_image_floats(int Mel, int H, int Stacks)
{
    if (!glowtts_ge2e_supported(Mel, H, Stacks, 1)) return -1;
    return image_offset(Stacks, Mel, H);
}

extern "C" int64_t glowtts_ge2e_work_floats(int64_t N, int T, int H, int Stacks)
{
    if (N < 1 || T < 1 || H < 1 || Stacks < 1) return -1;
    return (int64_t)Stacks * N * H * ((int64_t)T + 1);
}

extern "C" int glowtts_ge2e_pack(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* images, float* biases, int layer, int Mel,
                                 int H, int Stacks, void* stream)
{
    if (!w_ih || !w_hh || !b_ih || !b_hh || !images || !biases || !glowtts_ge2e_supported(Mel, H, Stacks, 1) || layer < 0 || layer >= Stacks) return GLOWTTS_E_ARG;
    const int in = layer == 0 ? Mel : H;
    const int64_t total = (int64_t)(in + H) * 4 * H;
    hipLaunchKernelGGL(ge2e_pack_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), w_ih, w_hh, b_ih, b_hh,
                       images + image_offset(layer, Mel, H), biases + (size_t)layer * 4 * H, in, H);
    GLOWTTS_NOTE_STATIC("ge2e_pack");
    return hipGetLastError() == hipSuccess ? GLOWTTS_OK : GLOWTTS_E_LAUNCH;
}

extern "C" int glowtts_ge2e_forward(const float* x, const float* images, const float* biases, const float* head_w, const float* head_b, float* work, float* hs,
                                    float* e, float* d, int N, int Samples, int Mel, int T, int H, int Stacks, int E, void* stream)
{
    if (!x || !images || !biases || !head_w || !head_b || !work || !d || !glowtts_ge2e_supported(Mel, H, Stacks, E) || N < 1 || Samples < 1 || N % Samples ||
        T < 1 || T > (1 << 20) || (N + TM - 1) / TM > 65535)
        return GLOWTTS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* cs = work;                                      // [Stacks][N][H]
    float* hbuf = hs ? hs : work + (size_t)Stacks * N * H;  // [Stacks][N][T][H]
    const int lds = cell_lds_bytes(Mel, H);
    static int allowed = 0;                                // (grows monotonically; a racing second caller sets the same or a larger value)
    if (lds > allowed) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&ge2e_cell_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return GLOWTTS_E_LAUNCH;
        allowed = lds;
    }
    for (int dg = 0; dg < T + Stacks - 1; ++dg) {
        const int kmin = dg - (T - 1) > 0 ? dg - (T - 1) : 0, kmax = dg < Stacks - 1 ? dg : Stacks - 1;
        hipLaunchKernelGGL(ge2e_cell_kernel, dim3(H / TU, (N + TM - 1) / TM, kmax - kmin + 1), dim3(THREADS), (size_t)lds, s, x, images, biases, hbuf, cs, N, Mel, T, H,
                           dg, kmin);
        GLOWTTS_NOTE_STATIC("ge2e_cell");
    }
    hipLaunchKernelGGL(ge2e_head_kernel, dim3(N / Samples), dim3(THREADS), (size_t)(H + E + 2) * 4, s, hbuf + (size_t)(Stacks - 1) * N * T * H, head_w, head_b, e, d,
                       Samples, T, H, E);
    GLOWTTS_NOTE_STATIC("ge2e_head");
    return hipGetLastError() == hipSuccess ? GLOWTTS_OK : GLOWTTS_E_LAUNCH;
}
