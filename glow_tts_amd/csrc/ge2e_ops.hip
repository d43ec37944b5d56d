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
// The cell kernel, its launch loop, the head's projection and the constants live in ge2e_common.h, which the training (ge2e_train_ops.hip) shares.
#include "ge2e_common.h"

namespace {

constexpr int MAX_LDS = 160 * 1024;

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

// ---- head: grid (B), dynamic LDS hl [H] | es [E] | sc [2].  w [E][H], bias [E] are torch.nn.Linear's own ------------------------------------------------
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
        ge2e_head_project(h_top + (n * T + (T - 1)) * H, w, bias, hl, H, E, [&](int j, float p) {
            es[j] = p;
            if (e_out) e_out[n * E + j] = p;
        });
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
    RET_LAUNCH();
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
    if (ge2e_launch_cells<false>(x, images, biases, hbuf, cs, nullptr, N, Mel, T, H, Stacks, s) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    hipLaunchKernelGGL(ge2e_head_kernel, dim3(N / Samples), dim3(THREADS), (size_t)(H + E + 2) * 4, s, hbuf + (size_t)(Stacks - 1) * N * T * H, head_w, head_b, e, d,
                       Samples, T, H, E);
    GLOWTTS_NOTE_STATIC("ge2e_head");
    RET_LAUNCH();
}
