// Neural vocoder: the Parallel WaveGAN generator (Yamamoto et al. 2020; a non-causal gated WaveNet over sample-rate rows) for gfx950, inference, f32.
// Rows are samples, channels-last: x [B][Tmax][R], c [B][Tmax][A], skips [B][Tmax][S]; an utterance of L frames owns rows [0, L hop) of its slab and
// nothing beyond them is read or (the waveform excepted) written.  Every matrix product runs on the exact-f32 MFMA v_mfma_f32_16x16x4_f32
// (A operand: lane l holds A[l & 15][l >> 4], B operand B[l >> 4][l & 15], result col = l & 15, row = 4 (l >> 4) + reg); the shape is the 16-wide one
// because the supported channel counts are multiples of 16 (R, S) and of 4 (A), not of 32.
//
//   pwg_cond_in    conv_in over the frames: replicate padding is a clamp of the gathered frame index; [B][A][Lmax] -> rows [B][Lmax][A]
//   pwg_upsample   one launch per scale: nearest-neighbour repeat + the shared (2 s + 1)-tap FIR, zero beyond the utterance's own ends
//   pwg_first      z (the counter hash of gauss_hash.h evaluated in the kernel, or the caller's noise) and first_conv
//   pwg_layer      ONE launch per WaveNet layer.  A workgroup owns 64 consecutive samples of one utterance:
//                    1. gathers [x(t - d) | x(t) | x(t + d) | c(t)] (zero outside the utterance) into LDS, K = 3 R + A floats per row;
//                    2. GEMM 1 against the layer's [K][G] weight image streamed from L2 as MFMA B operands (171 KB at the default sizes: more than LDS
//                       holds, and every workgroup of the launch reads the same image); a wave owns 16 tanh columns and their 16 sigmoid columns for all
//                       four row tiles, so the gate tanh * sigmoid is formed in its accumulators - the G-wide pre-activation never exists in memory;
//                    3. the gate goes to LDS (over the gathered rows when every wave owns at most one column pair), GEMM 2 against [G / 2][R + S]
//                       (conv1x1_out | conv1x1_skip); the epilogue writes x' = (out + x) sqrt(0.5) to the OTHER x buffer (neighbours still read x) and
//                       adds the skip columns into `skips` (each element has exactly one owner: no atomics).
//   pwg_head       skips sqrt(1 / Layers), ReLU, S x S 1x1 (MFMA), ReLU, S -> 1 as a fixed-order dot product; zeros beyond the utterance
// Tiles start at the utterance's own sample 0 and every sum has one fixed order, so a row's value depends on its utterance alone: the waveform is
// bit-identical alone, in any batch, at any padding and from run to run.
// The constants, the layer's row gather (step 1) and the head's first stage live in pwg_common.h, which the backward (pwg_train_ops.hip) shares.
#include <algorithm>

#include "gauss_hash.h"
#include "launch_log.h"
#include "pwg_common.h"

namespace {

constexpr int PF = 4;                                     // k steps of GEMM 1 whose weights are prefetched into registers
constexpr int MAX_DILATION = 1024, MAX_SCALES = 8;

// ---- conditioning ---------------------------------------------------------------------------------------------------------------------------
// grid (ceil(Lmax / 64), B); a wave owns 16 frames and walks the column tiles.  w: [(2 ctx + 1) A][A], row = tap * A + input channel.
__global__ __launch_bounds__(THREADS) void pwg_cond_in_kernel(const float* __restrict__ mel, const int32_t* __restrict__ lengths, const float* __restrict__ w,
                                                              float* __restrict__ out, int A, int Lmax, int ctx)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, L = min(lengths[b], Lmax);
    const int f0 = blockIdx.x * TM + wave * 16;
    if (f0 >= L) return;                                   // (no barrier in this kernel)
    const int K = (2 * ctx + 1) * A;
    const float* m = mel + (size_t)b * A * Lmax;
    const int f = f0 + r;
    for (int n0 = 0; n0 < A; n0 += 16) {
        const bool col_ok = n0 + r < A;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < K; k0 += 4) {
            const int k = k0 + q, j = k / A, ci = k - j * A;
            const int src = min(max(f + j - ctx, 0), L - 1);                  // replicate padding by the utterance's own first / last frame
            const float a = f < L ? m[(size_t)ci * Lmax + src] : 0.f;
            const float bw = col_ok ? w[(size_t)k * A + n0 + r] : 0.f;
            acc = mfma4(a, bw, acc);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int fo = f0 + q * 4 + i;
            if (fo < L && col_ok) out[((size_t)b * Lmax + fo) * A + n0 + r] = acc[i];
        }
    }
}

// in rows [B][Lmax * mult][A] (valid: L * mult) -> out rows [B][Lmax * mult * s][A]; grid (ceil(Lmax * mult * s * A / 4 / 256), B)
__global__ __launch_bounds__(THREADS) void pwg_upsample_kernel(const float* __restrict__ in, const int32_t* __restrict__ lengths, const float* __restrict__ fir,
                                                               float* __restrict__ out, int A, int Lmax, int mult, int s)
{
    const int b = blockIdx.y, a4n = A >> 2;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t t = e / a4n;
    const int a = (int)(e - t * a4n) * 4;
    const int64_t Tin = (int64_t)min(lengths[b], Lmax) * mult, Tout = Tin * s;
    if (t >= Tout) return;
    const float* src = in + (size_t)b * Lmax * mult * A + a;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j <= 2 * s; ++j) {
        const int64_t u = t + j - s;
        if (u < 0 || u >= Tout) continue;                  // zero padding at the utterance's own ends
        const float4 v = *reinterpret_cast<const float4*>(src + (size_t)(u / s) * A);
        const float wj = fir[j];
        acc.x = fmaf(wj, v.x, acc.x); acc.y = fmaf(wj, v.y, acc.y); acc.z = fmaf(wj, v.z, acc.z); acc.w = fmaf(wj, v.w, acc.w);
    }
    *reinterpret_cast<float4*>(out + ((size_t)b * Lmax * mult * s + t) * A + a) = acc;
}

// ---- noise and first_conv: grid (ceil(Tmax * R / 4 / 256), B) -----------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void pwg_first_kernel(const float* __restrict__ noises, const uint32_t* __restrict__ seeds, const int32_t* __restrict__ lengths,
                                                            const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ x, int Lmax, int hop,
                                                            int R)
{
    const int b = blockIdx.y, r4n = R >> 2;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t t = e / r4n, Tmax = (int64_t)Lmax * hop;
    const int c = (int)(e - t * r4n) * 4;
    if (t >= (int64_t)min(lengths[b], Lmax) * hop) return;
    const float z = noises ? noises[(size_t)b * Tmax + t] : gauss_hash::gauss(seeds[2 * b], seeds[2 * b + 1], 0u, (uint32_t)t, 1u);
    const float4 wv = *reinterpret_cast<const float4*>(w + c), bv = *reinterpret_cast<const float4*>(bias + c);
    *reinterpret_cast<float4*>(x + ((size_t)b * Tmax + t) * R + c) = make_float4(fmaf(wv.x, z, bv.x), fmaf(wv.y, z, bv.y), fmaf(wv.z, z, bv.z), fmaf(wv.w, z, bv.w));
}

// ---- one WaveNet layer: grid (ceil(Tmax / 64), B), dynamic LDS: Xs [64][xs] (+ Gs [64][R + 4] when it cannot lie over Xs) ----------------------------
// w1 [3 R + A][2 R]: rows tap-major (x(t - d), x(t), x(t + d)) then the aux channels, columns tanh half | sigmoid half;  w2 [R][R + S]: out | skip
__global__ __launch_bounds__(THREADS) void pwg_layer_kernel(const float* __restrict__ x, const float* __restrict__ c, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                            float* __restrict__ xo, float* __restrict__ skips, const int32_t* __restrict__ lengths, int Lmax, int hop,
                                                            int R, int S, int A, int d, int accumulate, int xs, int gs_off)
{
    extern __shared__ __attribute__((aligned(16))) float pwg_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, t0 = blockIdx.x * TM;
    const int T = min(lengths[b], Lmax) * hop;
    if (t0 >= T) return;                                   // (uniform over the workgroup)
    const int KA = 3 * R + A, G = 2 * R, N2 = R + S, gst = R + 4;
    const size_t row0 = (size_t)b * Lmax * hop;
    float* Xs = pwg_smem;
    float* Gs = pwg_smem + gs_off;

    // 1. gather
    pwg_gather_rows(x, c, Xs, row0, t0, T, R, A, d, xs);
    __syncthreads();

    // 2. GEMM 1 + gate.  (pwg_layer_bwd_gate_kernel runs this sum without the prefetch; both start from the bias and take k ascending in steps of 4)
    const bool alias = gs_off == 0;                        // then R / 16 <= WAVES: at most one column pair per wave
    f32x4 gate[4];
    int pending = -1;
    for (int p = wave; p < R / 16; p += WAVES) {
        const float* wt = w1 + p * 16 + r;                 // tanh column; its sigmoid column lies R further
        const float bt = b1[p * 16 + r], bs = b1[R + p * 16 + r];
        f32x4 at[4], as[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) { at[rt] = f32x4{bt, bt, bt, bt}; as[rt] = f32x4{bs, bs, bs, bs}; }
        const float* xa = Xs + r * xs + q;
        float wtr[PF], wsr[PF];                            // the weights of the next PF k steps are in flight while the MFMAs of this one issue
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int k = 4 * u + q;                       // (KA >= 4 PF: R >= 16)
            wtr[u] = wt[(size_t)k * G];
            wsr[u] = wt[(size_t)k * G + R];
        }
        for (int k0 = 0; k0 < KA; k0 += 4 * PF) {
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int kk = k0 + 4 * u;
                if (kk >= KA) break;                       // (uniform)
                const float wtk = wtr[u], wsk = wsr[u];
                const int kn = kk + 4 * PF + q;
                if (kn < KA) {
                    wtr[u] = wt[(size_t)kn * G];
                    wsr[u] = wt[(size_t)kn * G + R];
                }
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) {
                    const float a = xa[rt * 16 * xs + kk];
                    at[rt] = mfma4(a, wtk, at[rt]);
                    as[rt] = mfma4(a, wsk, as[rt]);
                }
            }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) gate[rt][i] = tanhf(at[rt][i]) * sigmoidf_(as[rt][i]);
        if (alias) { pending = p; }
        else {
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i) Gs[(rt * 16 + q * 4 + i) * gst + p * 16 + r] = gate[rt][i];
        }
    }
    __syncthreads();                                       // every wave is done with Xs
    if (pending >= 0) {
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) Gs[(rt * 16 + q * 4 + i) * gst + pending * 16 + r] = gate[rt][i];
    }
    __syncthreads();

    // 3. GEMM 2: residual and skip 1x1s
    for (int n = wave; n < N2 / 16; n += WAVES) {
        const int col = n * 16 + r;
        const float bv = b2[col];
        f32x4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{bv, bv, bv, bv};
        const float* ga = Gs + r * gst + q;
        const float* wc = w2 + col;
        for (int k0 = 0; k0 < R; k0 += 4) {
            const float wk = wc[(size_t)(k0 + q) * N2];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[rt] = mfma4(ga[rt * 16 * gst + k0], wk, acc[rt]);
        }
        const bool res = n * 16 < R;                       // (uniform over the wave: R is a multiple of 16)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + rt * 16 + q * 4 + i;
                if (t >= T) continue;
                if (res) {
                    xo[(row0 + t) * R + col] = (acc[rt][i] + x[(row0 + t) * R + col]) * RSQRT2;
                } else {
                    float* sp = skips + (row0 + t) * S + (col - R);
                    *sp = accumulate ? *sp + acc[rt][i] : acc[rt][i];
                }
            }
    }
}

// ---- head: grid (ceil(Tmax / 64), B), dynamic LDS Ys [64][S + 4] | Hs [64][S + 4];  w1 [S][S] (row = input channel) ----------------------------------
__global__ __launch_bounds__(THREADS) void pwg_head_kernel(const float* __restrict__ skips, const int32_t* __restrict__ lengths, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                           float* __restrict__ wav, int Lmax, int hop, int S, float scale)
{
    extern __shared__ __attribute__((aligned(16))) float pwg_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, t0 = blockIdx.x * TM;
    const int Tmax = Lmax * hop, T = min(lengths[b], Lmax) * hop;
    const size_t row0 = (size_t)b * Tmax;
    if (t0 >= T) {                                         // beyond the utterance: zeros (uniform over the workgroup)
        if (tid < TM && t0 + tid < Tmax) wav[row0 + t0 + tid] = 0.f;
        return;
    }
    const int st = S + 4;
    float* Ys = pwg_smem;
    float* Hs = pwg_smem + TM * st;
    pwg_head_stage(skips, Ys, row0, t0, T, S, scale, [](size_t, float4) {});
    for (int n = wave; n < S / 16; n += WAVES) {
        const int col = n * 16 + r;
        f32x4 acc[4];
        pwg_head_w1(Ys, w1, b1, S, col, acc);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) Hs[(rt * 16 + q * 4 + i) * st + col] = fmaxf(acc[rt][i], 0.f);
    }
    __syncthreads();
    if (tid < TM && t0 + tid < Tmax) {
        float v = 0.f;
        if (t0 + tid < T) {
            v = b2[0];
            for (int k = 0; k < S; ++k) v = fmaf(w2[k], Hs[tid * st + k], v);
        }
        wav[row0 + t0 + tid] = v;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
int layer_lds_bytes(int R, int A, int* xs, int* gs_off)
{
    const int stride = lds_stride_of(3 * R + A);
    const bool alias = R / 16 <= WAVES;
    if (xs) *xs = stride;
    if (gs_off) *gs_off = alias ? 0 : TM * stride;
    return (TM * stride + (alias ? 0 : TM * (R + 4))) * 4;
}

}  // namespace

extern "C" int glowtts_pwg_supported(int R, int G, int S, int A, int max_dilation)
{
    return R >= 16 && R <= MAX_CHANNELS && R % 16 == 0 && G == 2 * R && S >= 16 && S <= MAX_CHANNELS && S % 16 == 0 && A >= 4 && A <= MAX_CHANNELS && A % 4 == 0 &&
           max_dilation >= 1 && max_dilation <= MAX_DILATION && layer_lds_bytes(R, A, nullptr, nullptr) <= MAX_LDS && 2 * TM * (S + 4) * 4 <= MAX_LDS;
}

extern "C" int glowtts_pwg_condition(const float* mel, const int32_t* frame_lengths, const float* w_in, const float* firs, const int* scales, int n_scales,
                                     float* work, float* c, int B, int A, int Lmax, int ctx, void* stream)
{
    if (!mel || !frame_lengths || !w_in || !firs || !scales || !work || !c || n_scales < 1 || n_scales > MAX_SCALES || A < 4 || A > MAX_CHANNELS || A % 4 ||
        ctx < 0 || ctx > 16 || Lmax < 1 || B < 1 || B > 65535)
        return GLOWTTS_E_ARG;
    int64_t hop = 1;
    for (int i = 0; i < n_scales; ++i) {
        if (scales[i] < 1 || scales[i] > MAX_SCALE) return GLOWTTS_E_ARG;
        hop *= scales[i];
    }
    if (bad_batch(B, Lmax, (int)std::min<int64_t>(hop, 1 << 20))) return GLOWTTS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // frames: conv_in into the first half of `work`; the scales then ping-pong between the halves, the last one writes c
    const size_t half = (size_t)B * Lmax * A * (size_t)(hop / scales[n_scales - 1]);
    float* cur = work;
    hipLaunchKernelGGL(pwg_cond_in_kernel, dim3((Lmax + TM - 1) / TM, B), dim3(THREADS), 0, s, mel, frame_lengths, w_in, cur, A, Lmax, ctx);
    GLOWTTS_NOTE_STATIC("pwg_cond_in");
    int mult = 1;
    const float* fir = firs;
    for (int i = 0; i < n_scales; ++i) {
        const int sc = scales[i];
        float* dst = i == n_scales - 1 ? c : (cur == work ? work + half : work);
        const int64_t quads = (int64_t)Lmax * mult * sc * (A / 4);
        hipLaunchKernelGGL(pwg_upsample_kernel, dim3((unsigned)((quads + THREADS - 1) / THREADS), B), dim3(THREADS), 0, s, cur, frame_lengths, fir, dst, A, Lmax, mult, sc);
        GLOWTTS_NOTE_STATIC("pwg_upsample");
        cur = dst;
        mult *= sc;
        fir += 2 * sc + 1;
    }
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_first(const float* noises, const uint32_t* seeds, const int32_t* frame_lengths, const float* w, const float* bias, float* x, int B,
                                 int Lmax, int hop, int R, void* stream)
{
    if ((!noises) == (!seeds) || !frame_lengths || !w || !bias || !x || bad_batch(B, Lmax, hop) || R < 16 || R > MAX_CHANNELS || R % 16) return GLOWTTS_E_ARG;
    const int64_t quads = (int64_t)Lmax * hop * (R / 4);
    hipLaunchKernelGGL(pwg_first_kernel, dim3((unsigned)((quads + THREADS - 1) / THREADS), B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), noises, seeds,
                       frame_lengths, w, bias, x, Lmax, hop, R);
    GLOWTTS_NOTE_STATIC("pwg_first");
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_layer(const float* x, const float* c, const float* w1, const float* b1, const float* w2, const float* b2, float* x_out, float* skips,
                                 const int32_t* frame_lengths, int B, int Lmax, int hop, int R, int S, int A, int dilation, int accumulate, void* stream)
{
    if (!x || !c || !w1 || !b1 || !w2 || !b2 || !x_out || !skips || !frame_lengths || x == x_out || bad_batch(B, Lmax, hop) ||
        !glowtts_pwg_supported(R, 2 * R, S, A, dilation))
        return GLOWTTS_E_ARG;
    int xs, gs_off;
    const int lds = layer_lds_bytes(R, A, &xs, &gs_off);
    if (allow_lds<&pwg_layer_kernel>(lds) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    const int Tmax = Lmax * hop;
    hipLaunchKernelGGL(pwg_layer_kernel, dim3((Tmax + TM - 1) / TM, B), dim3(THREADS), (size_t)lds, static_cast<hipStream_t>(stream), x, c, w1, b1, w2, b2, x_out, skips,
                       frame_lengths, Lmax, hop, R, S, A, dilation, accumulate, xs, gs_off);
    GLOWTTS_NOTE_STATIC("pwg_layer");
    RET_LAUNCH();
}

extern "C" int glowtts_pwg_head(const float* skips, const int32_t* frame_lengths, const float* w1, const float* b1, const float* w2, const float* b2, float* wav,
                                int B, int Lmax, int hop, int S, float scale, void* stream)
{
    if (!skips || !frame_lengths || !w1 || !b1 || !w2 || !b2 || !wav || bad_batch(B, Lmax, hop) || S < 16 || S > MAX_CHANNELS || S % 16) return GLOWTTS_E_ARG;
    const int lds = 2 * TM * (S + 4) * 4;
    if (allow_lds<&pwg_head_kernel>(lds) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    const int Tmax = Lmax * hop;
    hipLaunchKernelGGL(pwg_head_kernel, dim3((Tmax + TM - 1) / TM, B), dim3(THREADS), (size_t)lds, static_cast<hipStream_t>(stream), skips, frame_lengths, w1, b1, w2, b2,
                       wav, Lmax, hop, S, scale);
    GLOWTTS_NOTE_STATIC("pwg_head");
    RET_LAUNCH();
}
