// Training of the GE2E speaker encoder (DESIGN.md "Training the GE2E speaker encoder"): the LSTM stack's backward, the GE2E softmax loss and the head's
// backward, for gfx950, f32.  The rules are the forward's (ge2e_ops.hip): no kernel waits on another workgroup, no float atomics, every sum has a fixed
// partition and a fixed order, every matrix product of the stack runs on v_mfma_f32_16x16x4_f32.
//
//   ge2e_cell (training)  ge2e_common.h's cell kernel with KEEP = true (the inference runs the same text with KEEP = false): keeps c whole
//                         [Stacks][N][T][H] and the activated gates [Stacks][N][T][4 H] in the image's column order.
//   ge2e_head_fwd         e = W h_{T-1}^{top} + b for every sequence: ge2e_common.h's head projection, which the inference head calls too.
//   ge2e_loss_*           six small launches: unit vectors, speaker sums and norms, scores + softmax, centroid gradients, du -> de, the two scalars.
//   ge2e_head_bwd         dh_top = de W, dW_lin = de^T h_top (MFMA, one wave per 16 x 16 tile, K serial), db_lin = sum de.
//   ge2e_pack_bwd         per layer the transposed image [W_hh^k ; W_ih^{k+1}] with rows in da's packed column order and columns = hidden units of layer k.
//   ge2e_cell_bwd         the reverse wavefront: launch d (descending) handles every cell (k, t = d - k).  dh^k_t = [da^k_{t+1} | da^{k+1}_t] . image_t, a K
//                         range of up to 8 H staged through LDS in chunks of BWD_CHUNK floats per row (fixed partition: chunk after chunk, within a chunk wave
//                         w owns the k steps w, w + 4, ...; the waves meet in LDS and are added in the order w0 + w1 + w2 + w3).  Thread (row, unit) then forms
//                         dc and the four pre-activation gradients from the kept gates and c, carries dc f to step t - 1 and writes da as one float4.
//   ge2e_wgrad            per layer [4 H x N T] . [N T x (in + H + 1)] (the last column is the constant 1: the bias gradient): 64 x 64 output tiles, rows
//                         staged 16 at a time, the reduction split in fixed chunks of rows; a second launch adds the chunks in order and writes torch's
//                         gate-major rows.
#include "ge2e_common.h"

namespace {

constexpr int BWD_CHUNK = 512;                            // floats of the K range per row and staging step of ge2e_cell_bwd
constexpr int BWD_AS = BWD_CHUNK + 4;                     // (stride / 4) odd
constexpr int WG_TILE = 64, WG_ROWS = 16, WG_LD = 80;     // ge2e_wgrad: output tile, rows per staging step, LDS stride (16 q + r: 64 distinct banks)
constexpr int WG_MAX_SPLITS = 8, WG_SPLIT_ROWS = 256;
constexpr float EPS = 1e-12f;

__host__ __device__ __forceinline__ int64_t image_t_offset(int layer, int H) { return (int64_t)layer * 8 * H * H; }
int wgrad_splits(int64_t rows) { const int64_t s = (rows + WG_SPLIT_ROWS - 1) / WG_SPLIT_ROWS; return (int)(s < 1 ? 1 : s > WG_MAX_SPLITS ? WG_MAX_SPLITS : s); }
int64_t wgrad_chunk_rows(int64_t rows) { const int sp = wgrad_splits(rows); return ((rows + sp - 1) / sp + WG_ROWS - 1) / WG_ROWS * WG_ROWS; }

// the sum over the workgroup in a fixed order (lanes: the shuffle tree; waves: 0 + 1 + 2 + 3); sc: WAVES floats of LDS; every thread gets the value
__device__ __forceinline__ float block_sum(float v, float* sc)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sc[0] + sc[1]) + sc[2]) + sc[3];
}

// ---- e = W h_{T-1}^{top} + b: grid (N), dynamic LDS hl [H] ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void ge2e_head_fwd_kernel(const float* __restrict__ h_top, const float* __restrict__ w, const float* __restrict__ bias,
                                                                float* __restrict__ e_out, int T, int H, int E)
{
    extern __shared__ __attribute__((aligned(16))) float ge2e_smem[];
    const size_t n = blockIdx.x;
    ge2e_head_project(h_top + (n * T + (T - 1)) * H, w, bias, ge2e_smem, H, E, [&](int j, float p) { e_out[n * E + j] = p; });
}

// ---- the loss.  Scratch (loss_work_floats): u [N][E] | sums [S][E] | dcent [S][E] | g [N][S] | cosv [N][S] | norm_c [S] | norm_x [N] | row_l [N] | row_dw [N]
struct LossWork {
    float *u, *sums, *dcent, *g, *cosv, *norm_c, *norm_x, *row_l, *row_dw;
};
__host__ __device__ inline LossWork loss_work(float* w, int64_t N, int64_t S, int64_t E)
{
    LossWork o;
    o.u = w; w += N * E;
    o.sums = w; w += S * E;
    o.dcent = w; w += S * E;
    o.g = w; w += N * S;
    o.cosv = w; w += N * S;
    o.norm_c = w; w += S;
    o.norm_x = w; w += N;
    o.row_l = w; w += N;
    o.row_dw = w;
    return o;
}
int64_t loss_work_floats(int64_t N, int64_t S, int64_t E) { return N * E + 2 * S * E + 2 * N * S + 3 * N + S; }

// grid (N): u = e / max(|e|, eps)
__global__ __launch_bounds__(THREADS) void ge2e_loss_norm_kernel(const float* __restrict__ e, LossWork W, int E)
{
    __shared__ float sc[WAVES];
    const size_t n = blockIdx.x;
    float p = 0.f;
    for (int j = threadIdx.x; j < E; j += THREADS) p = fmaf(e[n * E + j], e[n * E + j], p);
    const float norm = fmaxf(sqrtf(block_sum(p, sc)), EPS);
    for (int j = threadIdx.x; j < E; j += THREADS) W.u[n * E + j] = e[n * E + j] / norm;
}

// grid (S): sums_k = sum_i u_ki (i ascending); |c_k| with c_k = sums_k / M; |x_ki| with x_ki = (sums_k - u_ki) / (M - 1)
__global__ __launch_bounds__(THREADS) void ge2e_loss_centroid_kernel(LossWork W, int M, int E)
{
    __shared__ float sc[WAVES];
    const size_t k = blockIdx.x;
    float p = 0.f;
    for (int j = threadIdx.x; j < E; j += THREADS) {
        float a = 0.f;
        for (int i = 0; i < M; ++i) a += W.u[(k * M + i) * E + j];
        W.sums[k * E + j] = a;
        const float c = a / (float)M;
        p = fmaf(c, c, p);
    }
    p = block_sum(p, sc);
    if (threadIdx.x == 0) W.norm_c[k] = sqrtf(p);
    for (int i = 0; i < M; ++i) {
        float pe = 0.f;
        for (int j = threadIdx.x; j < E; j += THREADS) {
            const float xv = (W.sums[k * E + j] - W.u[(k * M + i) * E + j]) / (float)(M - 1);
            pe = fmaf(xv, xv, pe);
        }
        pe = block_sum(pe, sc);
        if (threadIdx.x == 0) W.norm_x[k * M + i] = sqrtf(pe);
    }
}

// grid (N): the row's S scores, their softmax; g = dL / ds, the row's loss and its share of dL / dw.  The row's scores live in cosv / g (global) between the phases.
__global__ __launch_bounds__(THREADS) void ge2e_loss_scores_kernel(LossWork W, const float* __restrict__ wp, int S, int M, int E)
{
    __shared__ float sc[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = blockIdx.x;
    const int own = (int)(n / M);
    const float w = *wp;
    for (int k = wave; k < S; k += WAVES) {
        float p = 0.f;
        if (k == own) {
            for (int j = lane; j < E; j += 64) p = fmaf(W.u[n * E + j], (W.sums[(size_t)k * E + j] - W.u[n * E + j]) / (float)(M - 1), p);
            p = wave_sum(p) / fmaxf(W.norm_x[n], EPS);
        } else {
            for (int j = lane; j < E; j += 64) p = fmaf(W.u[n * E + j], W.sums[(size_t)k * E + j] / (float)M, p);
            p = wave_sum(p) / fmaxf(W.norm_c[k], EPS);
        }
        if (lane == 0) W.cosv[n * S + k] = p;
    }
    __syncthreads();                                       // (the workgroup's own global writes are visible to it after the barrier)
    float mx = -INFINITY;
    for (int k = tid; k < S; k += THREADS) mx = fmaxf(mx, w * W.cosv[n * S + k]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    __syncthreads();
    if (lane == 0) sc[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
    float se = 0.f;
    for (int k = tid; k < S; k += THREADS) se += expf(w * W.cosv[n * S + k] - mx);
    se = block_sum(se, sc);
    const float lg = logf(se), lse = mx + lg;
    const float invN = 1.f / (float)(gridDim.x);
    float dwp = 0.f;
    for (int k = tid; k < S; k += THREADS) {
        const float cv = W.cosv[n * S + k];
        const float gk = (expf(w * cv - lse) - (k == own ? 1.f : 0.f)) * invN;
        W.g[n * S + k] = gk;
        dwp = fmaf(gk, cv, dwp);
    }
    dwp = block_sum(dwp, sc);
    if (tid == 0) {
        W.row_dw[n] = dwp;
        W.row_l[n] = lg - (w * W.cosv[n * S + own] - mx);        // (both terms small: no rounding at the scores' magnitude)
    }
}

// grid (S): dL / dc_k = sum over the rows n of OTHER speakers (n ascending) of g_nk w (u_n - [|c_k| > eps] cos_nk c_k / |c_k|) / max(|c_k|, eps)
__global__ __launch_bounds__(THREADS) void ge2e_loss_dcent_kernel(LossWork W, const float* __restrict__ wp, int N, int S, int M, int E)
{
    const int k = blockIdx.x;
    const float w = *wp, nc = W.norm_c[k], inv = 1.f / fmaxf(nc, EPS), proj = nc > EPS ? 1.f : 0.f;
    for (int j = threadIdx.x; j < E; j += THREADS) {
        const float chat = W.sums[(size_t)k * E + j] / (float)M * inv;
        float a = 0.f;
        for (int n = 0; n < N; ++n) {
            if (n / M == k) continue;
            a += W.g[(size_t)n * S + k] * (W.u[(size_t)n * E + j] - proj * W.cosv[(size_t)n * S + k] * chat);
        }
        W.dcent[(size_t)k * E + j] = a * w * inv;
    }
}

// dL / dx_n[j] of row n's exclusive centroid x_n = (sums - u_n) / (M - 1)
__device__ __forceinline__ float dexcl(const LossWork& W, float w, size_t n, int own, int S, int M, int E, int j)
{
    const float nx = W.norm_x[n], inv = 1.f / fmaxf(nx, EPS), proj = nx > EPS ? 1.f : 0.f;
    const float xhat = (W.sums[(size_t)own * E + j] - W.u[n * E + j]) / (float)(M - 1) * inv;
    return W.g[n * S + own] * w * inv * (W.u[n * E + j] - proj * W.cosv[n * S + own] * xhat);
}

// grid (N): du_n (direct terms k ascending, then the centroid's share, then the speaker's other rows' exclusive centroids m ascending), de_n through the normalisation
__global__ __launch_bounds__(THREADS) void ge2e_loss_du_kernel(const float* __restrict__ e, LossWork W, const float* __restrict__ wp, float* __restrict__ de, int S,
                                                               int M, int E)
{
    __shared__ float sc[WAVES];
    const size_t n = blockIdx.x;
    const int own = (int)(n / M), i = (int)(n - (size_t)own * M);
    const float w = *wp;
    float du[GLOWTTS_GE2E_MAX_E / THREADS];
    float dot = 0.f;
#pragma unroll
    for (int z = 0; z < GLOWTTS_GE2E_MAX_E / THREADS; ++z) {
        const int j = threadIdx.x + z * THREADS;
        du[z] = 0.f;
        if (j >= E) continue;
        float a = 0.f;
        for (int k = 0; k < S; ++k) {
            if (k == own) {
                const float xv = (W.sums[(size_t)k * E + j] - W.u[n * E + j]) / (float)(M - 1);
                a += W.g[n * S + k] * w * (xv / fmaxf(W.norm_x[n], EPS));
            } else {
                a += W.g[n * S + k] * w * (W.sums[(size_t)k * E + j] / (float)M / fmaxf(W.norm_c[k], EPS));
            }
        }
        a += W.dcent[(size_t)own * E + j] / (float)M;
        float b = 0.f;
        for (int m = 0; m < M; ++m)
            if (m != i) b += dexcl(W, w, (size_t)own * M + m, own, S, M, E, j);
        a += b / (float)(M - 1);
        du[z] = a;
        dot = fmaf(a, W.u[n * E + j], dot);
    }
    dot = block_sum(dot, sc);
    float sq = 0.f;
    for (int j = threadIdx.x; j < E; j += THREADS) sq = fmaf(e[n * E + j], e[n * E + j], sq);
    const float norm = sqrtf(block_sum(sq, sc));
#pragma unroll
    for (int z = 0; z < GLOWTTS_GE2E_MAX_E / THREADS; ++z) {
        const int j = threadIdx.x + z * THREADS;
        if (j < E) de[n * E + j] = norm > EPS ? (du[z] - W.u[n * E + j] * dot) / norm : du[z] / EPS;
    }
}

// grid (1): L = (1 / N) sum_n row_l, dL / dw = sum_n row_dw (thread-strided partial sums n ascending, then the block's fixed tree)
__global__ __launch_bounds__(THREADS) void ge2e_loss_final_kernel(LossWork W, float* __restrict__ loss, float* __restrict__ dw, int N)
{
    __shared__ float sc[WAVES];
    float a = 0.f, b = 0.f;
    for (int n = threadIdx.x; n < N; n += THREADS) {
        a += W.row_l[n];
        b += W.row_dw[n];
    }
    a = block_sum(a, sc);
    b = block_sum(b, sc);
    if (threadIdx.x == 0) {
        *loss = a / (float)N;
        *dw = b;
    }
}

// ---- head backward: grid (tiles, 1, 3).  z = 0: dh_top [N][H] = de [N][E] . W [E][H]; z = 1: dW [E][H] = de^T . h_top; z = 2: db [E] = sum_n de (n ascending).
// One wave per 16 x 16 output tile, the K range serial in steps of 4; operands out of range are zero.
__global__ __launch_bounds__(THREADS) void ge2e_head_bwd_kernel(const float* __restrict__ de, const float* __restrict__ w, const float* __restrict__ h_top,
                                                                float* __restrict__ dh_top, float* __restrict__ dw, float* __restrict__ db, int N, int T, int H, int E)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int role = blockIdx.z;
    if (role == 2) {
        const int j = blockIdx.x * THREADS + tid;
        if (j >= E) return;
        float a = 0.f;
        for (int n = 0; n < N; ++n) a += de[(size_t)n * E + j];
        db[j] = a;
        return;
    }
    const int Mo = role == 0 ? N : E, K = role == 0 ? E : N;           // output [Mo][H]
    const int tiles_n = H / 16, tiles_m = (Mo + 15) / 16;
    const int tile = blockIdx.x * WAVES + wave;
    if (tile >= tiles_m * tiles_n) return;
    const int m0 = (tile / tiles_n) * 16, c0 = (tile % tiles_n) * 16;
    const size_t hstride = (size_t)T * H;
    const float* hl = h_top + (size_t)(T - 1) * H;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int kk = k0 + q, m = m0 + r;
        float a = 0.f, b = 0.f;
        if (kk < K) {
            if (role == 0) {
                if (m < N) a = de[(size_t)m * E + kk];
                b = w[(size_t)kk * H + c0 + r];
            } else {
                if (m < E) a = de[(size_t)kk * E + m];
                b = hl[(size_t)kk * hstride + c0 + r];
            }
        }
        acc = mfma4(a, b, acc);
    }
    float* out = role == 0 ? dh_top : dw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + q * 4 + i;
        if (m < Mo) out[(size_t)m * H + c0 + r] = acc[i];
    }
}

// ---- pack of the transposed image of one layer: rows c (da's packed column order) of W_hh^k [4 H][H], then of W_ih^{k+1} [4 H][H] (not for the top layer) ----
__global__ __launch_bounds__(THREADS) void ge2e_pack_bwd_kernel(const float* __restrict__ w_hh, const float* __restrict__ w_ih_next, float* __restrict__ image_t, int H)
{
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t part = (int64_t)4 * H * H;
    if (e >= (w_ih_next ? 2 * part : part)) return;
    const int64_t el = e >= part ? e - part : e;
    const int col = (int)(el / H), j = (int)(el - (int64_t)col * H);
    const int s = col >> 6, u = (col >> 2) & 15, g = col & 3;
    const size_t row = (size_t)g * H + s * TU + u;
    image_t[e] = (e >= part ? w_ih_next : w_hh)[row * H + j];
}

// ---- one reverse diagonal.  LDS: As [16][BWD_AS] | red [WAVES][16 x 16] ------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void ge2e_cell_bwd_kernel(const float* __restrict__ images_t, const float* __restrict__ cs, const float* __restrict__ gates,
                                                                const float* __restrict__ dh_top, float* __restrict__ da, float* __restrict__ dcs, int N, int T,
                                                                int H, int Stacks, int d, int kmin)
{
    __shared__ __attribute__((aligned(16))) float As[TM * BWD_AS];
    __shared__ float red[WAVES * TM * TU];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int k = kmin + blockIdx.z, t = d - k;
    const int s = blockIdx.x, n0 = blockIdx.y * TM;
    const int G = 4 * H;
    const size_t layer_rows = (size_t)N * T;
    const float* img = images_t + image_t_offset(k, H) + s * TU + r;

    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int seg = 0; seg < 2; ++seg) {
        // seg 0: da^k_{t+1} against W_hh^k; seg 1: da^{k+1}_t against W_ih^{k+1}
        if (seg == 0 ? t + 1 >= T : k + 1 >= Stacks) continue;                 // (uniform over the workgroup)
        const float* src = da + ((size_t)(k + seg) * layer_rows + (size_t)(t + 1 - seg)) * G;      // + n T G per sequence
        const float* simg = img + (size_t)seg * G * H;
        for (int c0 = 0; c0 < G; c0 += BWD_CHUNK) {
            const int len = G - c0 < BWD_CHUNK ? G - c0 : BWD_CHUNK, lq = len >> 2;
            __syncthreads();                               // the previous chunk is read no more
            for (int e = tid; e < TM * lq; e += THREADS) {
                const int row = e / lq, j4 = (e - row * lq) * 4, n = n0 + row;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (n < N) v = *reinterpret_cast<const float4*>(src + (size_t)n * T * G + c0 + j4);
                *reinterpret_cast<float4*>(As + row * BWD_AS + j4) = v;
            }
            __syncthreads();
            const float* aa = As + r * BWD_AS + q;
            const float* bb = simg + (size_t)(c0 + q) * H;
            for (int k0 = 4 * wave; k0 < len; k0 += 4 * WAVES) acc = mfma4(aa[k0], bb[(size_t)k0 * H], acc);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[(wave * TM + q * 4 + i) * TU + r] = acc[i];
    __syncthreads();

    const int row = tid >> 4, u = tid & 15, n = n0 + row;
    if (n >= N) return;
    const int j = s * TU + u;
    float dh = ((red[(0 * TM + row) * TU + u] + red[(1 * TM + row) * TU + u]) + red[(2 * TM + row) * TU + u]) + red[(3 * TM + row) * TU + u];
    if (k == Stacks - 1 && t == T - 1) dh += dh_top[(size_t)n * H + j];
    const size_t cell = (size_t)k * layer_rows + (size_t)n * T + t;
    const float4 gt = *reinterpret_cast<const float4*>(gates + cell * G + s * 64 + u * 4);      // i, f, g, o (activated)
    const float c = cs[cell * H + j], c_prev = t > 0 ? cs[(cell - 1) * H + j] : 0.f;
    const float tc = tanhf(c);
    float* carry = dcs + ((size_t)k * N + n) * H + j;
    float dc = dh * gt.w * (1.f - tc * tc);
    if (t + 1 < T) dc += *carry;
    *carry = dc * gt.y;
    const float4 o = make_float4(dc * gt.z * gt.x * (1.f - gt.x), dc * c_prev * gt.y * (1.f - gt.y), dc * gt.x * (1.f - gt.z * gt.z), dh * tc * gt.w * (1.f - gt.w));
    *reinterpret_cast<float4*>(da + cell * G + s * 64 + u * 4) = o;
}

// ---- weight gradients of one layer, stage 1: grid (4 H / 64, ceil((in + H + 1) / 64), splits); partial [splits][4 H][in + H + 1], rows in da's column order ----
__global__ __launch_bounds__(THREADS) void ge2e_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ h_below, const float* __restrict__ h_own,
                                                             const float* __restrict__ da, float* __restrict__ partial, int64_t rows, int64_t chunk, int Mel, int T,
                                                             int H, int in)
{
    __shared__ __attribute__((aligned(16))) float As[WG_ROWS * WG_LD];
    __shared__ float Bs[WG_ROWS * WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int G = 4 * H, Ka = in + H + 1;
    const int m0 = blockIdx.x * WG_TILE, c0 = blockIdx.y * WG_TILE;
    const int64_t r0 = (int64_t)blockIdx.z * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lrow = tid >> 4, lc4 = (tid & 15) * 4;
    for (int64_t rb = r0; rb < r1; rb += WG_ROWS) {
        __syncthreads();
        const int64_t row = rb + lrow;
        {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < r1) v = *reinterpret_cast<const float4*>(da + (size_t)row * G + m0 + lc4);
            *reinterpret_cast<float4*>(As + lrow * WG_LD + lc4) = v;
        }
        {
            const int64_t n = row / T;
            const int t = (int)(row - n * T);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = c0 + lc4 + i;
                float v = 0.f;
                if (row < r1) {
                    if (kk < in) v = x ? x[((size_t)n * Mel + kk) * T + t] : h_below[(size_t)row * H + kk];
                    else if (kk < in + H) v = t > 0 ? h_own[(size_t)(row - 1) * H + (kk - in)] : 0.f;
                    else if (kk == in + H) v = 1.f;
                }
                Bs[lrow * WG_LD + lc4 + i] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < WG_ROWS; k0 += 4) {
            const float a = As[(k0 + q) * WG_LD + wave * 16 + r];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = mfma4(a, Bs[(k0 + q) * WG_LD + i * 16 + r], acc[i]);
        }
    }
    float* out = partial + (size_t)blockIdx.z * G * Ka;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + wave * 16 + q * 4 + i, kk = c0 + nt * 16 + r;
            if (kk < Ka) out[(size_t)m * Ka + kk] = acc[nt][i];
        }
}

// stage 2: the chunks added in order, written at torch's gate-major rows
__global__ __launch_bounds__(THREADS) void ge2e_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw_ih, float* __restrict__ dw_hh,
                                                                    float* __restrict__ db_ih, float* __restrict__ db_hh, int splits, int H, int in)
{
    const int G = 4 * H, Ka = in + H + 1;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= (int64_t)G * Ka) return;
    float a = 0.f;
    for (int z = 0; z < splits; ++z) a += partial[(size_t)z * G * Ka + e];
    const int col = (int)(e / Ka), kk = (int)(e - (int64_t)col * Ka);
    const int s = col >> 6, u = (col >> 2) & 15, g = col & 3;
    const size_t row = (size_t)g * H + s * TU + u;
    if (kk < in) dw_ih[row * in + kk] = a;
    else if (kk < in + H) dw_hh[row * H + (kk - in)] = a;
    else db_ih[row] = db_hh[row] = a;
}

bool launched() { return hipGetLastError() == hipSuccess; }
bool batch_ok(int64_t N, int T) { return N >= 1 && T >= 1 && T <= (1 << 20) && (N + TM - 1) / TM <= 65535 && N * T < ((int64_t)1 << 31); }

}  // namespace

extern "C" int64_t glowtts_ge2e_train_image_floats(int H, int Stacks)
{
    if (!glowtts_ge2e_supported(4, H, Stacks, 1)) return -1;
    return image_t_offset(Stacks, H) - (int64_t)4 * H * H;
}

extern "C" int64_t glowtts_ge2e_train_keep_floats(int64_t N, int T, int H, int Stacks)
{
    if (!batch_ok(N, T) || H < 1 || Stacks < 1) return -1;
    return (int64_t)Stacks * N * T * H * 6;
}

extern "C" int64_t glowtts_ge2e_train_loss_work_floats(int64_t N, int S, int E)
{
    if (N < 1 || S < 1 || E < 1) return -1;
    return loss_work_floats(N, S, E);
}

extern "C" int64_t glowtts_ge2e_train_work_floats(int64_t N, int T, int Mel, int H, int Stacks)
{
    if (!batch_ok(N, T) || !glowtts_ge2e_supported(Mel, H, Stacks, 1)) return -1;
    const int64_t inmax = Mel > H ? Mel : H;
    const int64_t wg = (int64_t)wgrad_splits(N * T) * 4 * H * (inmax + H + 1);
    const int64_t cell = (int64_t)N * H + (int64_t)Stacks * N * H;          // dh_top | the dc carry
    return wg > cell ? wg : cell;
}

extern "C" int glowtts_ge2e_train_pack(const float* w_hh, const float* w_ih_next, float* images_t, int layer, int H, int Stacks, void* stream)
{
    if (!w_hh || !images_t || !glowtts_ge2e_supported(4, H, Stacks, 1) || layer < 0 || layer >= Stacks || (layer + 1 < Stacks) != (w_ih_next != nullptr))
        return GLOWTTS_E_ARG;
    const int64_t total = (int64_t)(w_ih_next ? 8 : 4) * H * H;
    hipLaunchKernelGGL(ge2e_pack_bwd_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), w_hh, w_ih_next,
                       images_t + image_t_offset(layer, H), H);
    GLOWTTS_NOTE_STATIC("ge2e_pack_bwd");
    return launched() ? GLOWTTS_OK : GLOWTTS_E_LAUNCH;
}

extern "C" int glowtts_ge2e_train_forward(const float* x, const float* images, const float* biases, const float* head_w, const float* head_b, float* keep, float* e,
                                          int N, int Mel, int T, int H, int Stacks, int E, void* stream)
{
    if (!x || !images || !biases || !head_w || !head_b || !keep || !e || !glowtts_ge2e_supported(Mel, H, Stacks, E) || !batch_ok(N, T)) return GLOWTTS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t cells = (size_t)Stacks * N * T * H;
    float *hs = keep, *cs = keep + cells, *gates = keep + 2 * cells;
    if (ge2e_launch_cells<true>(x, images, biases, hs, cs, gates, N, Mel, T, H, Stacks, s) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    hipLaunchKernelGGL(ge2e_head_fwd_kernel, dim3(N), dim3(THREADS), (size_t)H * 4, s, hs + (size_t)(Stacks - 1) * N * T * H, head_w, head_b, e, T, H, E);
    GLOWTTS_NOTE_STATIC("ge2e_head_fwd");
    return launched() ? GLOWTTS_OK : GLOWTTS_E_LAUNCH;
}

extern "C" int glowtts_ge2e_train_loss(const float* e, const float* w, float* work, float* loss, float* de, float* dw, int S, int M, int E, void* stream)
{
    if (!e || !w || !work || !loss || !de || !dw || S < 2 || M < 2 || S > 65535 || M > 65535 || E < 1 || E > GLOWTTS_GE2E_MAX_E) return GLOWTTS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int N = S * M;
    const LossWork W = loss_work(work, N, S, E);
    hipLaunchKernelGGL(ge2e_loss_norm_kernel, dim3(N), dim3(THREADS), 0, s, e, W, E);
    GLOWTTS_NOTE_STATIC("ge2e_loss_norm");
    hipLaunchKernelGGL(ge2e_loss_centroid_kernel, dim3(S), dim3(THREADS), 0, s, W, M, E);
    GLOWTTS_NOTE_STATIC("ge2e_loss_centroid");
    hipLaunchKernelGGL(ge2e_loss_scores_kernel, dim3(N), dim3(THREADS), 0, s, W, w, S, M, E);
    GLOWTTS_NOTE_STATIC("ge2e_loss_scores");
    hipLaunchKernelGGL(ge2e_loss_dcent_kernel, dim3(S), dim3(THREADS), 0, s, W, w, N, S, M, E);
    GLOWTTS_NOTE_STATIC("ge2e_loss_dcent");
    hipLaunchKernelGGL(ge2e_loss_du_kernel, dim3(N), dim3(THREADS), 0, s, e, W, w, de, S, M, E);
    GLOWTTS_NOTE_STATIC("ge2e_loss_du");
    hipLaunchKernelGGL(ge2e_loss_final_kernel, dim3(1), dim3(THREADS), 0, s, W, loss, dw, N);
    GLOWTTS_NOTE_STATIC("ge2e_loss_final");
    return launched() ? GLOWTTS_OK : GLOWTTS_E_LAUNCH;
}

extern "C" int glowtts_ge2e_train_backward(const float* images_t, const float* keep, const float* head_w, const float* de, float* da, float* work, float* dhead_w,
                                           float* dhead_b, int N, int T, int H, int Stacks, int E, void* stream)
{
    if (!images_t || !keep || !head_w || !de || !da || !work || !dhead_w || !dhead_b || !glowtts_ge2e_supported(4, H, Stacks, E) || !batch_ok(N, T))
        return GLOWTTS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t cells = (size_t)Stacks * N * T * H;
    const float *hs = keep, *cs = keep + cells, *gates = keep + 2 * cells;
    float *dh_top = work, *dcs = work + (size_t)N * H;
    const int big = N > E ? N : E;
    const int tiles = ((big + 15) / 16) * (H / 16);
    const int gx = (tiles + WAVES - 1) / WAVES, gb = (E + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(ge2e_head_bwd_kernel, dim3(gx > gb ? gx : gb, 1, 3), dim3(THREADS), 0, s, de, head_w, hs + (size_t)(Stacks - 1) * N * T * H, dh_top, dhead_w,
                       dhead_b, N, T, H, E);
    GLOWTTS_NOTE_STATIC("ge2e_head_bwd");
    for (int dg = T + Stacks - 2; dg >= 0; --dg) {
        const int kmin = dg - (T - 1) > 0 ? dg - (T - 1) : 0, kmax = dg < Stacks - 1 ? dg : Stacks - 1;
        hipLaunchKernelGGL(ge2e_cell_bwd_kernel, dim3(H / TU, (N + TM - 1) / TM, kmax - kmin + 1), dim3(THREADS), 0, s, images_t, cs, gates, dh_top, da, dcs, N, T, H,
                           Stacks, dg, kmin);
        GLOWTTS_NOTE_STATIC("ge2e_cell_bwd");
    }
    return launched() ? GLOWTTS_OK : GLOWTTS_E_LAUNCH;
}

extern "C" int glowtts_ge2e_train_wgrad(const float* x, const float* keep, const float* da, float* work, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh,
                                        int layer, int N, int Mel, int T, int H, int Stacks, void* stream)
{
    if (!x || !keep || !da || !work || !dw_ih || !dw_hh || !db_ih || !db_hh || !glowtts_ge2e_supported(Mel, H, Stacks, 1) || !batch_ok(N, T) || layer < 0 ||
        layer >= Stacks)
        return GLOWTTS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t rows = (int64_t)N * T;
    const int in = layer == 0 ? Mel : H, Ka = in + H + 1, splits = wgrad_splits(rows);
    const int64_t chunk = wgrad_chunk_rows(rows);
    const size_t lay = (size_t)rows * H;
    hipLaunchKernelGGL(ge2e_wgrad_kernel, dim3(4 * H / WG_TILE, (Ka + WG_TILE - 1) / WG_TILE, splits), dim3(THREADS), 0, s, layer == 0 ? x : nullptr,
                       layer == 0 ? nullptr : keep + (size_t)(layer - 1) * lay, keep + (size_t)layer * lay, da + (size_t)layer * rows * 4 * H, work, rows, chunk, Mel, T, H,
                       in);
    GLOWTTS_NOTE_STATIC("ge2e_wgrad");
    const int64_t total = (int64_t)4 * H * Ka;
    hipLaunchKernelGGL(ge2e_wgrad_reduce_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, work, dw_ih, dw_hh, db_ih, db_hh, splits, H, in);
    GLOWTTS_NOTE_STATIC("ge2e_wgrad");
    return launched() ? GLOWTTS_OK : GLOWTTS_E_LAUNCH;
}
