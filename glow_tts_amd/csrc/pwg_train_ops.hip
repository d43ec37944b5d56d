// Training the Parallel WaveGAN generator: the backward of csrc/pwg_ops.hip for gfx950, f32.  The training forward IS the inference forward (the same entry
// points, so the waveform is bit-identical); it differs only in where it writes: every layer's input x gets its own slab [Layers + 1][B][Tmax][R] (the
// ping-pong buffers do not survive 30 layers), the gate is recomputed here.  Rows are samples, channels-last, as in the forward; an utterance owns rows
// [0, L hop) of its slab, tiles are counted from its own sample 0 and nothing beyond those rows is read or written.  Every matrix product runs on
// v_mfma_f32_16x16x4_f32 (operand layout: see pwg_ops.hip).  The layer's row gather and the head's first stage are the forward's own (pwg_common.h).
// No float atomics, no kernel waits on another workgroup, every sum has a fixed partition and order: every gradient is bit-identical from run to run.
//
//   pwg_head_bwd        per 64-row tile: y = relu(scale skips), h' = W1 y + b1 (MFMA), dh = dwav w2 [h' > 0], dy = W1^T dh (MFMA), dskips = scale dy [y > 0];
//                       y, h = relu(h'), dh go to HBM for the weight gradients.  dskips is the same tensor for every layer (skips is a plain sum).
//   pwg_layer_bwd_gate  per 64-row tile of one layer: the forward's gather (pwg_common.h) and GEMM 1 again (tanh / sigmoid halves stay in the accumulators), dgate =
//                       [sqrt(1/2) dx' | dskips] W2^T (K = R + S, MFMA, same column ownership), dpre = dgate (sigma (1 - tanh^2) | tanh sigma (1 - sigma));
//                       gate [rows][R] and dpre [rows][G] go to HBM - the dilated taps reach across tiles, so dpre must exist before dx can be formed.
//   pwg_layer_bwd_data  per 64-row tile: dx(t) = sqrt(1/2) dx'(t) + [dpre(t + d) | dpre(t) | dpre(t - d)] W1_taps^T (K = 3 G, zero outside the utterance,
//                       mirroring the forward gather) and dc(t) (+)= dpre(t) W_aux^T; the first layer processed overwrites dc.
//   pwg_wgrad           (pwg_wgrad.h, shared with the discriminator's backward) every weight gradient is a product A^T B over the rows.  A job names A (with a row shift for the dilated taps, or the noise hash for
//                       first_conv, and an optional constant-one column that yields the bias), B and where the result goes in torch's layout.  One wave owns
//                       a 16 x 16 output tile of one job over one split of the rows; the split partition is fixed: per utterance, chunks of 1024 rows.
//   pwg_wgrad_sum       adds the splits in ascending order, scales, writes torch's layout (overwrites).
//   pwg_first_bwd       the same two kernels for first_conv (A = z).
//   pwg_upsample_bwd    per scale, descending: the gradient of the coarser rows (gather form of repeat + FIR); `pwg_upsample_bwd_fir`: the FIR's gradient
//                       as per-block float64 sums in a fixed order; `pwg_upsample_bwd_sum`: their ordered sum.
//   pwg_cond_in_bwd     dW_in, one thread per weight over all frames in ascending order (float64 sum); the gradient of the mel is not computed.
#include <algorithm>

#include "gauss_hash.h"
#include "launch_log.h"
#include "pwg_common.h"
#include "pwg_wgrad.h"

namespace {

constexpr int FIR_ROWS = 256;                             // output rows of one block of the FIR gradient

// ---- head: grid (ceil(Tmax / 64), B), LDS Ys [64][S + 4] | DHs [64][S + 4].  w1 [S][S] row = input channel (the forward's image), w1t [S][S] row = output
// channel (torch's own tensor) ----
__global__ __launch_bounds__(THREADS) void pwg_head_bwd_kernel(const float* __restrict__ skips, const int32_t* __restrict__ lengths, const float* __restrict__ w1,
                                                               const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ w2,
                                                               const float* __restrict__ dwav, float* __restrict__ y, float* __restrict__ h, float* __restrict__ dh,
                                                               float* __restrict__ dskips, int Lmax, int hop, int S, float scale)
{
    extern __shared__ __attribute__((aligned(16))) float pwt_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, t0 = blockIdx.x * TM;
    const int Tmax = Lmax * hop, T = min(lengths[b], Lmax) * hop;
    if (t0 >= T) return;                                   // (uniform over the workgroup)
    const size_t row0 = (size_t)b * Tmax;
    const int st = S + 4;
    float* Ys = pwt_smem;
    float* DHs = pwt_smem + TM * st;
    pwg_head_stage(skips, Ys, row0, t0, T, S, scale, [&](size_t off, float4 v) { *reinterpret_cast<float4*>(y + off) = v; });
    for (int n = wave; n < S / 16; n += WAVES) {
        const int col = n * 16 + r;
        const float w2v = w2[col];
        f32x4 acc[4];
        pwg_head_w1(Ys, w1, b1, S, col, acc);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rt * 16 + q * 4 + i, t = t0 + row;
                float dv = 0.f;
                if (t < T) {
                    dv = acc[rt][i] > 0.f ? dwav[row0 + t] * w2v : 0.f;
                    h[(row0 + t) * S + col] = fmaxf(acc[rt][i], 0.f);
                    dh[(row0 + t) * S + col] = dv;
                }
                DHs[row * st + col] = dv;
            }
    }
    __syncthreads();
    for (int n = wave; n < S / 16; n += WAVES) {
        const int col = n * 16 + r;                        // input channel
        f32x4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* da = DHs + r * st + q;
        for (int k0 = 0; k0 < S; k0 += 4) {
            const float wk = w1t[(size_t)(k0 + q) * S + col];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[rt] = mfma4(da[rt * 16 * st + k0], wk, acc[rt]);
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rt * 16 + q * 4 + i, t = t0 + row;
                if (t < T) dskips[(row0 + t) * S + col] = Ys[row * st + col] > 0.f ? acc[rt][i] * scale : 0.f;
            }
    }
}

// ---- layer, first launch: grid (ceil(Tmax / 64), B), LDS Xs [64][xs] | Dy [64][R + S + 4].  w1, b1: the forward's; w2t [R + S][R] = the forward's w2 transposed ----
__global__ __launch_bounds__(THREADS) void pwg_layer_bwd_gate_kernel(const float* __restrict__ x, const float* __restrict__ c, const float* __restrict__ w1,
                                                                     const float* __restrict__ b1, const float* __restrict__ w2t, const float* __restrict__ dxp,
                                                                     const float* __restrict__ dskips, float* __restrict__ gate, float* __restrict__ dpre,
                                                                     const int32_t* __restrict__ lengths, int Lmax, int hop, int R, int S, int A, int d, int xs)
{
    extern __shared__ __attribute__((aligned(16))) float pwt_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, t0 = blockIdx.x * TM;
    const int T = min(lengths[b], Lmax) * hop;
    if (t0 >= T) return;                                   // (uniform over the workgroup)
    const int KA = 3 * R + A, G = 2 * R, N2 = R + S, dys = N2 + 4;
    const size_t row0 = (size_t)b * Lmax * hop;
    float* Xs = pwt_smem;
    float* Dy = pwt_smem + TM * xs;
    pwg_gather_rows(x, c, Xs, row0, t0, T, R, A, d, xs);
    const int nq = N2 >> 2;
    for (int e = tid; e < TM * nq; e += THREADS) {         // [sqrt(1/2) dx' | dskips]
        const int row = e / nq, k4 = (e - row * nq) * 4, t = t0 + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < T) {
            if (k4 < R) {
                v = *reinterpret_cast<const float4*>(dxp + (row0 + t) * R + k4);
                v.x *= RSQRT2; v.y *= RSQRT2; v.z *= RSQRT2; v.w *= RSQRT2;
            } else {
                v = *reinterpret_cast<const float4*>(dskips + (row0 + t) * S + (k4 - R));
            }
        }
        *reinterpret_cast<float4*>(Dy + row * dys + k4) = v;
    }
    __syncthreads();
    for (int p = wave; p < R / 16; p += WAVES) {
        const int col = p * 16 + r;
        const float* wt = w1 + col;                        // tanh column; its sigmoid column lies R further
        const float bt = b1[col], bs = b1[R + col];
        f32x4 at[4], as[4], dg[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) { at[rt] = f32x4{bt, bt, bt, bt}; as[rt] = f32x4{bs, bs, bs, bs}; dg[rt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        const float* xa = Xs + r * xs + q;
        // (pwg_layer_kernel runs this sum with a weight prefetch; both start from the bias and take k ascending in steps of 4)
        for (int k0 = 0; k0 < KA; k0 += 4) {
            const float wtk = wt[(size_t)(k0 + q) * G], wsk = wt[(size_t)(k0 + q) * G + R];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                const float a = xa[rt * 16 * xs + k0];
                at[rt] = mfma4(a, wtk, at[rt]);
                as[rt] = mfma4(a, wsk, as[rt]);
            }
        }
        const float* ya = Dy + r * dys + q;
        for (int k0 = 0; k0 < N2; k0 += 4) {
            const float wk = w2t[(size_t)(k0 + q) * R + col];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) dg[rt] = mfma4(ya[rt * 16 * dys + k0], wk, dg[rt]);
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + rt * 16 + q * 4 + i;
                if (t >= T) continue;
                const float ta = tanhf(at[rt][i]), sg = sigmoidf_(as[rt][i]), g = dg[rt][i];
                gate[(row0 + t) * R + col] = ta * sg;
                dpre[(row0 + t) * G + col] = g * sg * (1.f - ta * ta);
                dpre[(row0 + t) * G + R + col] = g * ta * sg * (1.f - sg);
            }
    }
}

// ---- layer, second launch: grid (ceil(Tmax / 64), B), LDS Ds [64][3 G + 4] = dpre(t + d) | dpre(t) | dpre(t - d).  w1t [3 G][R]: row = tap * G + gate column;
// wauxt [G][A].  dx != dxp is not required (an element is read and written by one thread) but the caller keeps dx' for the weight gradients. ----
__global__ __launch_bounds__(THREADS) void pwg_layer_bwd_data_kernel(const float* __restrict__ dpre, const float* __restrict__ w1t, const float* __restrict__ wauxt,
                                                                     const float* __restrict__ dxp, float* __restrict__ dx, float* __restrict__ dc,
                                                                     const int32_t* __restrict__ lengths, int Lmax, int hop, int R, int A, int d, int first)
{
    extern __shared__ __attribute__((aligned(16))) float pwt_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, t0 = blockIdx.x * TM;
    const int T = min(lengths[b], Lmax) * hop;
    if (t0 >= T) return;                                   // (uniform over the workgroup)
    const int G = 2 * R, K3 = 3 * G, ds = K3 + 4;
    const size_t row0 = (size_t)b * Lmax * hop;
    float* Ds = pwt_smem;
    const int kq = K3 >> 2;
    for (int e = tid; e < TM * kq; e += THREADS) {
        const int row = e / kq, k4 = (e - row * kq) * 4, t = t0 + row;
        const int j = k4 / G, g = k4 - j * G, ts = t - (j - 1) * d;     // tap j of the forward read x(t + (j - 1) d): x(u) is reached from t = u - (j - 1) d
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < T && ts >= 0 && ts < T) v = *reinterpret_cast<const float4*>(dpre + (row0 + ts) * G + g);
        *reinterpret_cast<float4*>(Ds + row * ds + k4) = v;
    }
    __syncthreads();
    const int nr = R / 16, na = (A + 15) / 16;
    for (int n = wave; n < nr + na; n += WAVES) {
        const bool res = n < nr;                           // (uniform over the wave)
        const int col = (res ? n : n - nr) * 16 + r;
        const bool ok = res || col < A;
        f32x4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* da = Ds + r * ds + q + (res ? 0 : G);
        const int K = res ? K3 : G, ldw = res ? R : A;
        const float* wsrc = res ? w1t : wauxt;
        for (int k0 = 0; k0 < K; k0 += 4) {
            const float wk = ok ? wsrc[(size_t)(k0 + q) * ldw + col] : 0.f;
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[rt] = mfma4(da[rt * 16 * ds + k0], wk, acc[rt]);
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + rt * 16 + q * 4 + i;
                if (t >= T || !ok) continue;
                if (res) {
                    dx[(row0 + t) * R + col] = acc[rt][i] + RSQRT2 * dxp[(row0 + t) * R + col];
                } else {
                    float* p = dc + (row0 + t) * A + col;
                    *p = first ? acc[rt][i] : *p + acc[rt][i];
                }
            }
    }
}

// ---- conditioning chain ----
// d in[u] = sum_{v in [u s, u s + s)} sum_j fir[j] d out[v - j + s]: grid (ceil(Lmax mult A / 4 / 256), B)
__global__ __launch_bounds__(THREADS) void pwg_upsample_bwd_kernel(const float* __restrict__ dout, const int32_t* __restrict__ lengths, const float* __restrict__ fir,
                                                                   float* __restrict__ din, int A, int Lmax, int mult, int s)
{
    const int b = blockIdx.y, a4n = A >> 2;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t u = e / a4n;
    const int a = (int)(e - u * a4n) * 4;
    const int64_t Tin = (int64_t)min(lengths[b], Lmax) * mult, Tout = Tin * s;
    if (u >= Tin) return;
    const float* src = dout + (size_t)b * Lmax * mult * s * A + a;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t v = u * s; v < u * s + s; ++v)
        for (int j = 0; j <= 2 * s; ++j) {
            const int64_t t = v - j + s;
            if (t < 0 || t >= Tout) continue;
            const float4 g = *reinterpret_cast<const float4*>(src + (size_t)t * A);
            const float wj = fir[j];
            acc.x = fmaf(wj, g.x, acc.x); acc.y = fmaf(wj, g.y, acc.y); acc.z = fmaf(wj, g.z, acc.z); acc.w = fmaf(wj, g.w, acc.w);
        }
    *reinterpret_cast<float4*>(din + ((size_t)b * Lmax * mult + u) * A + a) = acc;
}

// d fir[j] of one block of 256 output rows: grid (nblk, B) -> partial [B nblk][2 s + 1] (float64)
__global__ __launch_bounds__(THREADS) void pwg_upsample_bwd_fir_kernel(const float* __restrict__ dout, const float* __restrict__ in, const int32_t* __restrict__ lengths,
                                                                       double* __restrict__ partial, int A, int Lmax, int mult, int s)
{
    __shared__ double red[THREADS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t Tin = (int64_t)min(lengths[b], Lmax) * mult, Tout = Tin * s;
    const int64_t t0 = (int64_t)blockIdx.x * FIR_ROWS;
    const float* go = dout + (size_t)b * Lmax * mult * s * A;
    const float* xi = in + (size_t)b * Lmax * mult * A;
    double* out = partial + ((size_t)b * gridDim.x + blockIdx.x) * (2 * s + 1);
    for (int j = 0; j <= 2 * s; ++j) {
        double acc = 0.0;
        for (int e = tid; e < FIR_ROWS * A; e += THREADS) {
            const int64_t t = t0 + e / A, v = t + j - s;
            const int ch = e % A;
            if (t < Tout && v >= 0 && v < Tout) acc += (double)(go[(size_t)t * A + ch] * xi[(size_t)(v / s) * A + ch]);
        }
        const double total = block_sum(acc, red, tid);
        if (tid == 0) out[j] = total;
    }
}

__global__ __launch_bounds__(64) void pwg_sum_parts_kernel(const double* __restrict__ partial, float* __restrict__ dst, int parts, int n)
{
    const int j = threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int k = 0; k < parts; ++k) s += partial[(size_t)k * n + j];
    dst[j] = (float)s;
}

// dW_in [A][A][2 ctx + 1] (torch's layout), one thread per weight: grid (ceil(A A (2 ctx + 1) / 256))
__global__ __launch_bounds__(THREADS) void pwg_cond_in_bwd_kernel(const float* __restrict__ mel, const float* __restrict__ dcond, const int32_t* __restrict__ lengths,
                                                                  float* __restrict__ dw, int B, int A, int Lmax, int ctx)
{
    const int taps = 2 * ctx + 1, e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= A * A * taps) return;
    const int o = e / (A * taps), i = (e - o * A * taps) / taps, k = e - (o * A + i) * taps;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        const int L = min(lengths[b], Lmax);
        const float* m = mel + ((size_t)b * A + i) * Lmax;
        const float* g = dcond + (size_t)b * Lmax * A + o;
        for (int f = 0; f < L; ++f) acc += (double)(g[(size_t)f * A] * m[min(max(f + k - ctx, 0), L - 1)]);
    }
    dw[e] = (float)acc;
}

// ---- host side ----
int gate_lds(int R, int S, int A) { return TM * (lds_stride_of(3 * R + A) + R + S + 4) * 4; }
int data_lds(int R) { return TM * (6 * R + 4) * 4; }
int head_lds(int S) { return 2 * TM * (S + 4) * 4; }

int64_t layer_elems(int R, int S, int A)
{
    const int G = 2 * R;
    // the jobs of glowtts_pwg_train_layer_wgrad: three taps (the centre one with the bias column), aux, out and skip (both with the bias column)
    return 256 * ((int64_t)(2 * tiles16(R) + tiles16(R + 1)) * tiles16(G) + (int64_t)tiles16(A) * tiles16(G) + (int64_t)tiles16(R + 1) * (tiles16(R) + tiles16(S)));
}

}  // namespace

extern "C" int glowtts_pwg_train_supported(int R, int S, int A, int max_dilation)
{
    return glowtts_pwg_supported(R, 2 * R, S, A, max_dilation) && gate_lds(R, S, A) <= MAX_LDS && data_lds(R) <= MAX_LDS && head_lds(S) <= MAX_LDS;
}

extern "C" int64_t glowtts_pwg_train_work_floats(int B, int Lmax, int hop, int R, int S, int A)
{
    if (bad_train_batch(B, Lmax, hop) || R < 1 || S < 1 || A < 1) return 0;
    const int64_t T = (int64_t)Lmax * hop, splits = B * ((T + WG_ROWS - 1) / WG_ROWS);
    const int64_t head = 256 * ((int64_t)tiles16(S + 1) * tiles16(S) + (int64_t)tiles16(S + 1)), first = 256 * (int64_t)tiles16(R);
    const int64_t wg = splits * std::max(layer_elems(R, S, A), std::max(head, first));
    const int64_t fir = 2 * (int64_t)B * ((T + FIR_ROWS - 1) / FIR_ROWS) * (2 * MAX_SCALE + 1);
    return std::max(wg, fir);
}

extern "C" int glowtts_pwg_train_head_bwd(const float* skips, const int32_t* frame_lengths, const float* w1, const float* w1t, const float* b1, const float* w2,
                                          const float* dwav, float* y, float* h, float* dh, float* dskips, int B, int Lmax, int hop, int S, float scale, void* stream)
{
    if (!skips || !frame_lengths || !w1 || !w1t || !b1 || !w2 || !dwav || !y || !h || !dh || !dskips || bad_train_batch(B, Lmax, hop) || S < 16 || S > MAX_CHANNELS || S % 16 ||
        head_lds(S) > MAX_LDS)
        return GLOWTTS_E_ARG;
    const int lds = head_lds(S);
    if (allow_lds<&pwg_head_bwd_kernel>(lds) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("pwg_head_bwd");
    hipLaunchKernelGGL(pwg_head_bwd_kernel, dim3((Lmax * hop + TM - 1) / TM, B), dim3(THREADS), (size_t)lds, static_cast<hipStream_t>(stream), skips, frame_lengths, w1,
                       w1t, b1, w2, dwav, y, h, dh, dskips, Lmax, hop, S, scale);
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_train_head_wgrad(const float* y, const float* h, const float* dh, const float* dwav, const int32_t* frame_lengths, float* work, float* dw1,
                                            float* db1, float* dw2, float* db2, int B, int Lmax, int hop, int S, void* stream)
{
    if (!y || !h || !dh || !dwav || !frame_lengths || !work || !dw1 || !db1 || !dw2 || !db2 || bad_train_batch(B, Lmax, hop) || S < 16 || S > MAX_CHANNELS || S % 16)
        return GLOWTTS_E_ARG;
    wg_args a = {};
    add_job(a, y, S, S, 0, dh, S, S, dw1, 1, S, db1, 1.f);                  // last_conv_layers.1.weight [out][in]
    add_job(a, h, S, S, 0, dwav, 1, 1, dw2, 1, S, db2, 1.f);                // last_conv_layers.3.weight [1][in]
    return wgrad_launch(a, frame_lengths, work, B, Lmax, hop, "pwg_wgrad", "pwg_wgrad_sum", stream);
}

extern "C" int glowtts_pwg_train_layer_bwd(const float* x, const float* c, const float* w1, const float* b1, const float* w2t, const float* w1t, const float* wauxt,
                                           const float* dxp, const float* dskips, float* gate, float* dpre, float* dx, float* dc, const int32_t* frame_lengths, int B,
                                           int Lmax, int hop, int R, int S, int A, int dilation, int first, void* stream)
{
    if (!x || !c || !w1 || !b1 || !w2t || !w1t || !wauxt || !dxp || !dskips || !gate || !dpre || !dx || !dc || !frame_lengths || bad_train_batch(B, Lmax, hop) ||
        !glowtts_pwg_train_supported(R, S, A, dilation))
        return GLOWTTS_E_ARG;
    const int lds1 = gate_lds(R, S, A), lds2 = data_lds(R);
    if (allow_lds<&pwg_layer_bwd_gate_kernel>(lds1) != GLOWTTS_OK || allow_lds<&pwg_layer_bwd_data_kernel>(lds2) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    const dim3 grid((Lmax * hop + TM - 1) / TM, B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    GLOWTTS_NOTE_STATIC("pwg_layer_bwd_gate");
    hipLaunchKernelGGL(pwg_layer_bwd_gate_kernel, grid, dim3(THREADS), (size_t)lds1, s, x, c, w1, b1, w2t, dxp, dskips, gate, dpre, frame_lengths, Lmax, hop, R, S, A,
                       dilation, lds_stride_of(3 * R + A));
    GLOWTTS_NOTE_STATIC("pwg_layer_bwd_data");
    hipLaunchKernelGGL(pwg_layer_bwd_data_kernel, grid, dim3(THREADS), (size_t)lds2, s, dpre, w1t, wauxt, dxp, dx, dc, frame_lengths, Lmax, hop, R, A, dilation, first);
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_train_layer_wgrad(const float* x, const float* c, const float* gate, const float* dpre, const float* dxp, const float* dskips,
                                             const int32_t* frame_lengths, float* work, float* dconv_w, float* dconv_b, float* daux_w, float* dout_w, float* dout_b,
                                             float* dskip_w, float* dskip_b, int B, int Lmax, int hop, int R, int S, int A, int dilation, void* stream)
{
    if (!x || !c || !gate || !dpre || !dxp || !dskips || !frame_lengths || !work || !dconv_w || !dconv_b || !daux_w || !dout_w || !dout_b || !dskip_w || !dskip_b ||
        bad_train_batch(B, Lmax, hop) || !glowtts_pwg_train_supported(R, S, A, dilation))
        return GLOWTTS_E_ARG;
    const int G = 2 * R;
    wg_args a = {};
    for (int j = 0; j < 3; ++j)                                              // conv.weight [G][R][3]: tap j read x(t + (j - 1) d)
        add_job(a, x, R, R, (j - 1) * dilation, dpre, G, G, dconv_w + j, 3, 3 * R, j == 1 ? dconv_b : nullptr, 1.f);
    add_job(a, c, A, A, 0, dpre, G, G, daux_w, 1, A, nullptr, 1.f);          // conv1x1_aux.weight [G][A]
    add_job(a, gate, R, R, 0, dxp, R, R, dout_w, 1, R, dout_b, RSQRT2);      // conv1x1_out.weight [R][G / 2]
    add_job(a, gate, R, R, 0, dskips, S, S, dskip_w, 1, R, dskip_b, 1.f);    // conv1x1_skip.weight [S][G / 2]
    return wgrad_launch(a, frame_lengths, work, B, Lmax, hop, "pwg_wgrad", "pwg_wgrad_sum", stream);
}

extern "C" int glowtts_pwg_train_first_bwd(const float* noises, const uint32_t* seeds, const float* dx0, const int32_t* frame_lengths, float* work, float* dw, float* db,
                                           int B, int Lmax, int hop, int R, void* stream)
{
    if ((!noises) == (!seeds) || !dx0 || !frame_lengths || !work || !dw || !db || bad_train_batch(B, Lmax, hop) || R < 16 || R > MAX_CHANNELS || R % 16) return GLOWTTS_E_ARG;
    wg_args a = {};
    a.seeds = seeds; a.noise = noises;
    add_job(a, nullptr, 1, 1, 0, dx0, R, R, dw, 0, 1, db, 1.f);              // first_conv.weight [R][1][1]
    return wgrad_launch(a, frame_lengths, work, B, Lmax, hop, "pwg_first_bwd", "pwg_wgrad_sum", stream);
}

extern "C" int glowtts_pwg_train_upsample_bwd(const float* dout, const float* in, const float* fir, const int32_t* frame_lengths, float* work, float* din, float* dfir,
                                              int B, int A, int Lmax, int mult, int s, void* stream)
{
    if (!dout || !in || !fir || !frame_lengths || !work || !din || !dfir || B < 1 || B > 65535 || A < 4 || A > MAX_CHANNELS || A % 4 || Lmax < 1 || mult < 1 || s < 1 ||
        s > MAX_SCALE || (int64_t)Lmax * mult * s > ((int64_t)1 << 30) || (reinterpret_cast<uintptr_t>(work) & 7))
        return GLOWTTS_E_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t quads = (int64_t)Lmax * mult * (A / 4);
    const int nblk = (int)(((int64_t)Lmax * mult * s + FIR_ROWS - 1) / FIR_ROWS);
    GLOWTTS_NOTE_STATIC("pwg_upsample_bwd");
    hipLaunchKernelGGL(pwg_upsample_bwd_kernel, dim3((unsigned)((quads + THREADS - 1) / THREADS), B), dim3(THREADS), 0, st, dout, frame_lengths, fir, din, A, Lmax, mult, s);
    GLOWTTS_NOTE_STATIC("pwg_upsample_bwd_fir");
    hipLaunchKernelGGL(pwg_upsample_bwd_fir_kernel, dim3(nblk, B), dim3(THREADS), 0, st, dout, in, frame_lengths, reinterpret_cast<double*>(work), A, Lmax, mult, s);
    GLOWTTS_NOTE_STATIC("pwg_upsample_bwd_sum");
    hipLaunchKernelGGL(pwg_sum_parts_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const double*>(work), dfir, B * nblk, 2 * s + 1);
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_train_cond_in_bwd(const float* mel, const float* dcond, const int32_t* frame_lengths, float* dw, int B, int A, int Lmax, int ctx, void* stream)
{
    if (!mel || !dcond || !frame_lengths || !dw || B < 1 || B > 65535 || A < 4 || A > MAX_CHANNELS || A % 4 || Lmax < 1 || ctx < 0 || ctx > 16) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("pwg_cond_in_bwd");
    hipLaunchKernelGGL(pwg_cond_in_bwd_kernel, dim3((A * A * (2 * ctx + 1) + THREADS - 1) / THREADS), dim3(THREADS), 0, static_cast<hipStream_t>(stream), mel, dcond,
                       frame_lengths, dw, B, A, Lmax, ctx);
    RET_LAUNCH();
}
