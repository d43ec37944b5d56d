// Embedding maps (glow_tts_amd/projection.py, Prosody_Visualization.py): exact t-SNE of N points x [N][D] into two dimensions; the contract is DESIGN.md "Embedding maps".
// One N x N f32 matrix of row pitch ld = (N + 3) & ~3 (rows 16-byte aligned) is the squared distances, then the conditional affinities, then the joint ones P, in place.
//
// tsne_sqdist_kernel, one 256-thread workgroup per 64 x 64 tile of d2, grid (ceil(N / 64), ceil(N / 64)):
//   HBM -> LDS   the tile's two row blocks of x in chunks of 32 features, transposed to [k][row] (pitch 65: the staging writes, whose lanes differ in k, hit distinct banks)
//   LDS -> reg   a thread owns 4 rows x 4 columns (columns 16 apart): d2[i][j] = sum_k (x_ik - x_jk)^2 by direct differences, k ascending, one fused multiply-add per
//                term; features beyond D are staged as zeros and add exactly nothing.  Two identical rows give exactly 0.
// tsne_affinity_kernel, one 256-thread workgroup per row i:
//   LDS          the row of d2 less its minimum over j != i (<= 32 KiB at N = 8192)
//   64 steps     of the contract's bisection of beta; each evaluates e_j = exp(-beta d_j) and reduces sum e_j and sum d_j e_j over the workgroup: per-thread float64
//                partial sums (j ascending in steps of 256), the xor tree of the wave, the four waves' sums added in wave order - the same bits in every thread, so the
//                search is uniform without a broadcast.  H and the comparison are f32.
//   LDS -> HBM   p_{j|i} = e_j / s of the last beta evaluated, over the row in place; p_{i|i} = 0
// tsne_symmetrize_kernel, one workgroup per tile pair (I, J), I <= J (the others leave at once): both tiles through LDS, then P_ij = max((p_{j|i} + p_{i|j}) / (2N), 1e-12)
//   written to both, in place; 0 on the diagonal and in the pad columns.  a + b is b + a: P is symmetric bit for bit.
// tsne_forces_kernel<KL>, 512 threads, grid min(ceil(N / 8), 1024): the hot one, once per iteration.
//   HBM -> LDS   y [N][2] (<= 64 KiB)
//   one wave per row i (rows dealt round-robin over the waves of the grid): lane l reads P's row in 16-byte pieces 4 (l + 64 k) .. + 3, k ascending, and keeps, per lane,
//                sum_j P_ij w_ij (y_i - y_j) and sum_j w_ij^2 (y_i - y_j) in f32, the row's share of Z = sum_j w_ij (the f32 w added in float64); KL, the
//                measuring variant: the Z share from float64 w, and sum_j P_ij (ln P_ij - ln w_ij), its terms in float64, and sum_j P_ij.  Then the xor tree of the
//                wave; lane 0 writes the row's partials: sums [N][4] f32 (attractive
//                x, y, repulsive x, y), shares [N][4] float64 (Z, KL term, sum P, 0).  P is read exactly once, nothing of size N^2 is written.
// tsne_step_kernel, ONE 1024-thread workgroup:
//   Z = sum_i shares (float64: thread t adds rows t, t + 1024, ..; xor tree; the 16 waves' sums in wave order); on a measuring launch KL = sum_i KL term + ln Z sum P
//   into kl[slot] (float64); on an updating launch the gradient, gains, momentum and update of every point, the mean of the new y by the same tree, and y -= mean.
//   No atomics, no workgroup waits on another, every reduction order is fixed: a map is bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/glowtts_hip.h"
#include "launch_log.h"
#include "device_common.h"

namespace {

constexpr int TS_TILE = 64, TS_KC = 32, TS_PITCH = TS_TILE + 1;
constexpr int TS_FORCE_NT = 512, TS_FORCE_MAX_GRID = 1024, TS_STEP_NT = 1024;
constexpr float TS_EXAGGERATION = 12.f, TS_MOMENTUM_EARLY = 0.5f, TS_MOMENTUM_LATE = 0.8f, TS_P_FLOOR = 1e-12f;

__host__ __device__ __forceinline__ int ts_pitch(int N) { return (N + 3) & ~3; }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// sums of K values per thread over a workgroup of NW waves: the xor tree of each wave, then the waves' sums in wave order; every thread returns the same bits.
// scr: K * NW doubles of LDS, free again when the call returns.
template <int K, int NW> __device__ __forceinline__ void block_sum_d(double (&v)[K], double* scr)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = wave_sum_d(v[k]);
        if (lane == 0) scr[k * NW + wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int w = 0; w < NW; ++w) s += scr[k * NW + w];
        v[k] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void tsne_sqdist_kernel(const float* __restrict__ x, float* __restrict__ d2, int N, int D, int ld)
{
    __shared__ float xa[TS_KC * TS_PITCH], xb[TS_KC * TS_PITCH];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * TS_TILE, j0 = blockIdx.x * TS_TILE;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int k0 = 0; k0 < D; k0 += TS_KC) {
        for (int o = tid; o < TS_TILE * TS_KC; o += 256) {
            const int r = o / TS_KC, k = o - r * TS_KC, gk = k0 + k;
            xa[k * TS_PITCH + r] = (i0 + r < N && gk < D) ? x[(int64_t)(i0 + r) * D + gk] : 0.f;
            xb[k * TS_PITCH + r] = (j0 + r < N && gk < D) ? x[(int64_t)(j0 + r) * D + gk] : 0.f;
        }
        __syncthreads();
        for (int k = 0; k < TS_KC; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = xa[k * TS_PITCH + ty * 4 + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = xb[k * TS_PITCH + tx + 16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float df = a[r] - b[c];
                    acc[r][c] = fmaf(df, df, acc[r][c]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty * 4 + r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx + 16 * c;
            if (i < N && j < N) d2[(int64_t)i * ld + j] = acc[r][c];
        }
    }
}

constexpr int TS_AFF_HEAD = 128;                                               // bytes of reduction scratch in front of the row

__global__ __launch_bounds__(256) void tsne_affinity_kernel(float* __restrict__ c, int N, int ld, float log_perplexity)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ts_smem[];
    double* const scr = reinterpret_cast<double*>(ts_smem);                    // [2][4]
    float* const mins = reinterpret_cast<float*>(ts_smem + 64);                // [4]
    float* const row = reinterpret_cast<float*>(ts_smem + TS_AFF_HEAD);        // [N]
    const int tid = threadIdx.x, i = blockIdx.x;
    float* const g = c + (int64_t)i * ld;
    float m = INFINITY;
    for (int j = tid; j < N; j += 256) {
        const float v = g[j];
        row[j] = v;
        if (j != i) m = fminf(m, v);
    }
    m = wave_min(m);
    if ((tid & 63) == 0) mins[tid >> 6] = m;
    __syncthreads();
    m = fminf(fminf(mins[0], mins[1]), fminf(mins[2], mins[3]));
    for (int j = tid; j < N; j += 256) row[j] -= m;                            // (each thread its own elements: no barrier needed before the search reads them)
    float beta = 1.f, lo = 0.f, hi = INFINITY, beta_e = 1.f, s_e = 1.f;
    for (int step = 0; step < 64; ++step) {
        double v[2] = {0.0, 0.0};
        for (int j = tid; j < N; j += 256) {
            if (j == i) continue;
            const float d = row[j], e = expf(-beta * d);
            v[0] += (double)e;
            v[1] += (double)(d * e);
        }
        block_sum_d<2, 4>(v, scr);
        const float s = (float)v[0], sde = (float)v[1];
        const float H = logf(s) + beta * sde / s;
        beta_e = beta; s_e = s;
        if (H > log_perplexity) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.f : (beta + hi) * 0.5f;
        } else {
            hi = beta;
            beta = (beta + lo) * 0.5f;
        }
    }
    for (int j = tid; j < N; j += 256) g[j] = j == i ? 0.f : expf(-beta_e * row[j]) / s_e;
}

__global__ __launch_bounds__(256) void tsne_symmetrize_kernel(float* __restrict__ c, int N, int ld)
{
    const int I = blockIdx.y, J = blockIdx.x;
    if (I > J) return;
    __shared__ float A[TS_TILE * TS_PITCH], B[TS_TILE * TS_PITCH];             // A: rows of block I, columns of block J; B: rows of J, columns of I
    const int tid = threadIdx.x;
    for (int o = tid; o < TS_TILE * TS_TILE; o += 256) {
        const int r = o >> 6, q = o & 63;
        const int ia = I * TS_TILE + r, ja = J * TS_TILE + q, ib = J * TS_TILE + r, jb = I * TS_TILE + q;
        A[r * TS_PITCH + q] = (ia < N && ja < N) ? c[(int64_t)ia * ld + ja] : 0.f;
        B[r * TS_PITCH + q] = (ib < N && jb < N) ? c[(int64_t)ib * ld + jb] : 0.f;
    }
    __syncthreads();
    const float den = 2.f * (float)N;
    for (int o = tid; o < TS_TILE * TS_TILE; o += 256) {
        const int r = o >> 6, q = o & 63;
        const int i = I * TS_TILE + r, j = J * TS_TILE + q;
        if (i < N && j < ld) c[(int64_t)i * ld + j] = (i == j || j >= N) ? 0.f : fmaxf((A[r * TS_PITCH + q] + B[q * TS_PITCH + r]) / den, TS_P_FLOOR);
    }
    if (I == J) return;
    for (int o = tid; o < TS_TILE * TS_TILE; o += 256) {
        const int r = o >> 6, q = o & 63;
        const int i = J * TS_TILE + r, j = I * TS_TILE + q;                    // (block I is not the last one: no pad columns here)
        if (i < N && j < N) c[(int64_t)i * ld + j] = fmaxf((B[r * TS_PITCH + q] + A[q * TS_PITCH + r]) / den, TS_P_FLOOR);
    }
}

template <bool KL>
__global__ __launch_bounds__(TS_FORCE_NT) void tsne_forces_kernel(const float* __restrict__ P, const float* __restrict__ y, float* __restrict__ sums,
                                                                  double* __restrict__ shares, int N, int ld)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ts_smem[];
    float2* const ys = reinterpret_cast<float2*>(ts_smem);                     // [ld]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = TS_FORCE_NT / 64;
    for (int j = tid; j < ld; j += TS_FORCE_NT) ys[j] = j < N ? reinterpret_cast<const float2*>(y)[j] : make_float2(0.f, 0.f);
    __syncthreads();
    const int quads = ld >> 2;
    for (int i = blockIdx.x * NW + wave; i < N; i += gridDim.x * NW) {
        const float2 yi = ys[i];
        const float4* const prow = reinterpret_cast<const float4*>(P + (int64_t)i * ld);
        float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f;
        double z = 0.0, kl = 0.0, ps = 0.0;
        for (int q = lane; q < quads; q += 64) {
            const float4 p4 = prow[q];
            const float pv[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * q + e;
                const float2 yj = ys[j];
                const float dx = yi.x - yj.x, dy = yi.y - yj.y;
                float w = 1.f / (1.f + (dx * dx + dy * dy));
                if (j == i || j >= N) w = 0.f;
                const float p = pv[e], pw = p * w, w2 = w * w;
                ax = fmaf(pw, dx, ax); ay = fmaf(pw, dy, ay);
                rx = fmaf(w2, dx, rx); ry = fmaf(w2, dy, ry);
                if (KL) {
                    // measuring launches are one in fifty: what they REPORT - the Z share and the cost's terms - is float64 arithmetic on the exact differences of
                    // the f32 y, -ln w taken as ln(1 + |y_i - y_j|^2) (the device's logf is up to an ulp out on one side: at |ln P| ~ 8 .. 17 that was a systematic
                    // 5e-7 on the cost; and 56 f32-rounded w at N = 8 miss their float64 sum by 0.4 ulp of Z).  p > 0 excludes the diagonal and the pads
                    const double ddx = (double)yi.x - (double)yj.x, ddy = (double)yi.y - (double)yj.y, dd = ddx * ddx + ddy * ddy;
                    if (j != i && j < N) z += 1.0 / (1.0 + dd);
                    if (p > 0.f) kl += (double)p * (log((double)p) + log1p(dd));
                    ps += (double)p;
                } else {
                    z += (double)w;
                }
            }
        }
        ax = wave_sum(ax); ay = wave_sum(ay); rx = wave_sum(rx); ry = wave_sum(ry);
        z = wave_sum_d(z);
        if (KL) { kl = wave_sum_d(kl); ps = wave_sum_d(ps); }
        if (lane == 0) {
            reinterpret_cast<float4*>(sums)[i] = make_float4(ax, ay, rx, ry);
            double* const s = shares + (int64_t)i * 4;
            s[0] = z; s[1] = kl; s[2] = ps; s[3] = 0.0;
        }
    }
}

struct step_args {
    const float* sums;         // [N][4]
    const double* shares;      // [N][4]
    float* y;                  // [N][2]
    float* u;
    float* gain;
    double* kl;
    int N, kl_slot, update;    // kl_slot < 0: not a measuring launch
    float a, mu, lr;
};

__device__ __forceinline__ int sign_of(float v) { return (v > 0.f) - (v < 0.f); }

__global__ __launch_bounds__(TS_STEP_NT) void tsne_step_kernel(const step_args s)
{
    constexpr int NW = TS_STEP_NT / 64;
    __shared__ double scr[3 * NW];
    const int tid = threadIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < s.N; i += TS_STEP_NT) {
        const double* r = s.shares + (int64_t)i * 4;
        v[0] += r[0];
        if (s.kl_slot >= 0) { v[1] += r[1]; v[2] += r[2]; }
    }
    block_sum_d<3, NW>(v, scr);
    const double Z = v[0];
    if (s.kl_slot >= 0 && tid == 0) s.kl[s.kl_slot] = v[1] + log(Z) * v[2];
    if (!s.update) return;
    const float Zf = (float)Z;
    double m[2] = {0.0, 0.0};
    for (int i = tid; i < s.N; i += TS_STEP_NT) {
        const float4 f = reinterpret_cast<const float4*>(s.sums)[i];
        const float at[2] = {f.x, f.y}, rp[2] = {f.z, f.w};
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const int o = 2 * i + d;
            const float g = 4.f * (s.a * at[d] - rp[d] / Zf);
            const float u0 = s.u[o], g0 = s.gain[o];
            const float gn = fmaxf(sign_of(g) != sign_of(u0) ? g0 + 0.2f : g0 * 0.8f, 0.01f);
            const float un = s.mu * u0 - s.lr * gn * g;
            const float yn = s.y[o] + un;
            s.gain[o] = gn; s.u[o] = un; s.y[o] = yn;
            m[d] += (double)yn;
        }
    }
    block_sum_d<2, NW>(m, scr);
    const float mx = (float)(m[0] / (double)s.N), my = (float)(m[1] / (double)s.N);
    for (int i = tid; i < s.N; i += TS_STEP_NT) {                              // (each thread re-reads what it wrote itself)
        s.y[2 * i] -= mx;
        s.y[2 * i + 1] -= my;
    }
}

bool ts_supported(int N, int D) { return N >= 8 && N <= GLOWTTS_TSNE_MAX_N && D >= 1 && D <= GLOWTTS_TSNE_MAX_D; }

struct ts_work {
    float* P;
    float* sums;
    double* shares;
};
ts_work ts_carve(void* work, int N)
{
    ts_work w;
    w.P = static_cast<float*>(work);
    w.sums = w.P + (int64_t)N * ts_pitch(N);
    w.shares = reinterpret_cast<double*>(w.sums + (int64_t)N * 4);
    return w;
}

void launch_forces(const float* P, const float* y, float* sums, double* shares, int N, bool kl, hipStream_t st)
{
    const int ld = ts_pitch(N);
    const int rows_per = TS_FORCE_NT / 64;
    int grid = (N + rows_per - 1) / rows_per;
    if (grid > TS_FORCE_MAX_GRID) grid = TS_FORCE_MAX_GRID;
    const size_t lds = (size_t)ld * 8;
    if (kl) {
        GLOWTTS_NOTE_STATIC("tsne_forces,kl");
        hipLaunchKernelGGL(tsne_forces_kernel<true>, dim3(grid), dim3(TS_FORCE_NT), lds, st, P, y, sums, shares, N, ld);
    } else {
        GLOWTTS_NOTE_STATIC("tsne_forces");
        hipLaunchKernelGGL(tsne_forces_kernel<false>, dim3(grid), dim3(TS_FORCE_NT), lds, st, P, y, sums, shares, N, ld);
    }
}

void launch_sqdist(const float* x, float* d2, int N, int D, int ld, hipStream_t st)
{
    const int nt = (N + TS_TILE - 1) / TS_TILE;
    GLOWTTS_NOTE_STATIC("tsne_sqdist");
    hipLaunchKernelGGL(tsne_sqdist_kernel, dim3(nt, nt), dim3(256), 0, st, x, d2, N, D, ld);
}

}  // namespace

extern "C" int glowtts_tsne_supported(int N, int D) { return ts_supported(N, D) ? 1 : 0; }

extern "C" int64_t glowtts_tsne_work_bytes(int N)
{
    if (N < 8 || N > GLOWTTS_TSNE_MAX_N) return 0;
    return (int64_t)N * ts_pitch(N) * 4 + (int64_t)N * 16 + (int64_t)N * 32;
}

extern "C" int glowtts_tsne_sqdist(const float* x, float* d2, int N, int D, int ld, void* stream)
{
    if (!x || !d2 || !ts_supported(N, D) || ld < N) return GLOWTTS_E_ARG;
    launch_sqdist(x, d2, N, D, ld, static_cast<hipStream_t>(stream));
    RET_LAUNCH();
}

extern "C" int glowtts_tsne_affinities(const float* x, void* work, int N, int D, float perplexity, int joint, void* stream)
{
    if (!x || !work || !ts_supported(N, D) || !(perplexity >= 1.f) || !(perplexity * 3.f <= (float)(N - 1))) return GLOWTTS_E_ARG;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const ts_work w = ts_carve(work, N);
    const int ld = ts_pitch(N), nt = (N + TS_TILE - 1) / TS_TILE;
    launch_sqdist(x, w.P, N, D, ld, st);
    if (hipGetLastError() != hipSuccess) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("tsne_affinity");
    hipLaunchKernelGGL(tsne_affinity_kernel, dim3(N), dim3(256), (size_t)TS_AFF_HEAD + (size_t)N * 4, st, w.P, N, ld, logf(perplexity));
    if (joint) {
        if (hipGetLastError() != hipSuccess) return GLOWTTS_E_LAUNCH;
        GLOWTTS_NOTE_STATIC("tsne_symmetrize");
        hipLaunchKernelGGL(tsne_symmetrize_kernel, dim3(nt, nt), dim3(256), 0, st, w.P, N, ld);
    }
    RET_LAUNCH();
}

extern "C" int glowtts_tsne_forces(const float* p, const float* y, float* sums, double* shares, int N, int kl, void* stream)
{
    if (!p || !y || !sums || !shares || N < 8 || N > GLOWTTS_TSNE_MAX_N) return GLOWTTS_E_ARG;
    launch_forces(p, y, sums, shares, N, kl != 0, static_cast<hipStream_t>(stream));
    RET_LAUNCH();
}

extern "C" int glowtts_tsne_iterate(void* work, float* y, float* u, float* gain, double* kl, int N, int t0, int t1, int exaggeration_iterations,
                                    float learning_rate, int kl_every, int kl_final, void* stream)
{
    if (!work || !y || !u || !gain || N < 8 || N > GLOWTTS_TSNE_MAX_N || t0 < 0 || t1 < t0 || exaggeration_iterations < 0 || !(learning_rate > 0.f) ||
        ((kl_every > 0 || kl_final) && !kl))
        return GLOWTTS_E_ARG;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const ts_work w = ts_carve(work, N);
    step_args s = {};
    s.sums = w.sums; s.shares = w.shares; s.y = y; s.u = u; s.gain = gain; s.kl = kl; s.N = N; s.lr = learning_rate;
    for (int t = t0; t < t1; ++t) {
        const bool measure = kl_every > 0 && t % kl_every == 0;
        launch_forces(w.P, y, w.sums, w.shares, N, measure, st);
        const bool early = t < exaggeration_iterations;
        s.a = early ? TS_EXAGGERATION : 1.f;
        s.mu = early ? TS_MOMENTUM_EARLY : TS_MOMENTUM_LATE;
        s.kl_slot = measure ? t / kl_every : -1;
        s.update = 1;
        GLOWTTS_NOTE_STATIC("tsne_step");
        hipLaunchKernelGGL(tsne_step_kernel, dim3(1), dim3(TS_STEP_NT), 0, st, s);
        if (hipGetLastError() != hipSuccess) return GLOWTTS_E_LAUNCH;
    }
    if (kl_final) {
        launch_forces(w.P, y, w.sums, w.shares, N, true, st);
        s.a = 1.f; s.mu = 0.f; s.update = 0;
        s.kl_slot = kl_every > 0 ? (t1 + kl_every - 1) / kl_every : 0;
        GLOWTTS_NOTE_STATIC("tsne_step,finish");
        hipLaunchKernelGGL(tsne_step_kernel, dim3(1), dim3(TS_STEP_NT), 0, st, s);
    }
    RET_LAUNCH();
}
