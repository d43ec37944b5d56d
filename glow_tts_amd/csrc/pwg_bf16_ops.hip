// Neural vocoder, bf16 inference mode: the Parallel WaveGAN generator's WaveNet layer with bf16 operands (DESIGN.md "Neural vocoder", "bf16 inference
// mode").  Only the layer launches change; the conditioning, first and head launches of pwg_ops.hip and the noise contract stay f32.
//
//   pwg_layer_bf16  ONE launch per layer, the f32 kernel's row ownership: a workgroup owns 64 consecutive samples of one utterance, tiles start at the
//                   utterance's own sample 0, every sum has one fixed order - a row's value depends on its utterance alone.
//                     1. gathers [x(t - d) | x(t) | x(t + d) | c(t)] (zero outside the utterance), ROUNDED to bf16 (nearest even), into LDS: K1 = 3 R + A
//                        padded with zero columns to K1p, the next multiple of 32;
//                     2. GEMM 1 on v_mfma_f32_16x16x32_bf16 against the layer's packed bf16 image (zero rows beyond K1) streamed from L2: a lane's eight
//                        k values are one 16-byte load, the 16 lanes of a quarter read 256 consecutive bytes; fp32 accumulators start from the fp32 bias;
//                        a wave owns 16 tanh columns and their 16 sigmoid columns for all four row tiles, so tanh * sigmoid is formed from its fp32
//                        accumulators and the G-wide pre-activation never exists in memory (fp32 on the hardware exp and reciprocal, device_common.h's
//                        bf16-mode tanh_ / sigmoid_: absolute error about 1e-7, far below what the gate's rounding to bf16 keeps; libm's versions with
//                        their IEEE division were a quarter of the kernel's vector instructions);
//                     3. the gate is rounded to bf16 into LDS (K2 = R padded with zero columns to K2p), GEMM 2 against the packed [K2p][R + S] image; the
//                        epilogue is the f32 kernel's: x' = (out + x) sqrt(0.5) with the UNROUNDED fp32 x, skips = skip or skips + skip, both fp32 in HBM.
// Operand layout of v_mfma_f32_16x16x32_bf16: lane l holds A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15], j = 0 .. 7; C as mfma4.
// Images (packed once at load on the host, vocoder.pwg_pack_bf16): [Kp / 8][N][8] bf16 - element (k, n) at ((k / 8) N + n) 8 + k % 8.
// LDS rows are Kp bf16 + 16 bytes: the stride in 16-byte slots, Kp / 8 + 1, is odd, so the 16 rows of a ds_read_b128 group fall into 16 distinct slots.
#include "launch_log.h"
#include "pwg_common.h"

namespace {

constexpr int PF = 4;                                     // k steps (of 32) of GEMM 1 whose weights are prefetched into registers
constexpr int GU = 6;                                     // 16-byte loads of the gather that a thread keeps in flight (18 per thread at the default sizes)

__host__ __device__ __forceinline__ int pad32(int K) { return (K + 31) & ~31; }

__device__ __forceinline__ f32x4 mfma32(const Chunk16& a, const Chunk16& b, const f32x4& c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&a), *reinterpret_cast<const bf16x8*>(&b), c, 0, 0, 0);
}

// ---- one WaveNet layer: grid (ceil(Tmax / 64), B), dynamic LDS: Xs [64][K1p + 8] bf16 | Gs [64][K2p + 8] bf16 --------------------------------------
// w1p [K1p / 8][2 R][8]: k = x(t - d) | x(t) | x(t + d) | aux | zeros, columns tanh half | sigmoid half;  w2p [K2p / 8][R + S][8]: out | skip
// Three waves per SIMD is what the default sizes' 46 KB of LDS per workgroup allow (3 workgroups per CU), so the register budget is set to match it: 136 VGPRs,
// no scratch (left to itself the compiler took 240 for two waves).
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(3, 3)))
void pwg_layer_bf16_kernel(const float* __restrict__ x, const float* __restrict__ c, const uint16_t* __restrict__ w1p, const float* __restrict__ b1,
                           const uint16_t* __restrict__ w2p, const float* __restrict__ b2, float* __restrict__ xo, float* __restrict__ skips,
                           const int32_t* __restrict__ lengths, int Lmax, int hop, int R, int S, int A, int d, int accumulate)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t pwg_bf16_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, t0 = blockIdx.x * TM;
    const int T = min(lengths[b], Lmax) * hop;
    if (t0 >= T) return;                                   // (uniform over the workgroup)
    const int K1 = 3 * R + A, K1p = pad32(K1), K2p = pad32(R), G = 2 * R, N2 = R + S;
    const int xs = K1p + 8, gst = K2p + 8;                 // row strides in bf16
    const size_t row0 = (size_t)b * Lmax * hop;
    uint16_t* Xs = pwg_bf16_smem;
    uint16_t* Gs = pwg_bf16_smem + TM * xs;

    // 1. gather and round: four channels (8 bytes of bf16) per access; the columns K1 .. K1p - 1, and the gate's R .. K2p - 1, are zero
    // (element e = tid + n THREADS of the [64][K1p / 4] tile is walked as (row, cq) with a carry: one integer division per thread, none per element)
    const int kq = K1p >> 2, dr = THREADS / kq, dc = THREADS - dr * kq;
    // GU loads are issued before the first of them is rounded and stored, so a thread waits for HBM once per GU elements and not once per element
    for (int row = tid / kq, cq = tid - (tid / kq) * kq; row < TM;) {
        // (every load is unconditional, from an address clamped into the utterance's own rows, and zeroed afterwards where the element is padding: a
        // conditional load made the compiler wait for each one at the end of its branch)
        float4 v[GU];
        int at[GU];                                        // where element u goes in Xs; -1: beyond the tile
        bool ok[GU];                                       // it is a value of the utterance, not zero padding
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const int k4 = cq * 4, t = t0 + row;
            const bool tap = k4 < 3 * R;
            const int j = (k4 >= R) + (k4 >= 2 * R), ts = t + (j - 1) * d;
            at[u] = row < TM ? row * xs + k4 : -1;
            ok[u] = row < TM && t < T && (tap ? ts >= 0 && ts < T : k4 < K1);
            const float* src = tap ? x + (row0 + min(max(ts, 0), T - 1)) * R + (k4 - j * R) : c + (row0 + min(t, T - 1)) * A + min(k4 - 3 * R, A - 4);
            v[u] = *reinterpret_cast<const float4*>(src);
            row += dr;
            cq += dc;
            if (cq >= kq) { cq -= kq; ++row; }
        }
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            if (at[u] < 0) continue;
            const float4 w = ok[u] ? v[u] : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<u32x2*>(Xs + at[u]) = u32x2{pack_bf16x2(w.x, w.y), pack_bf16x2(w.z, w.w)};
        }
    }
    if (K2p > R) {                                         // (R = 16 mod 32: sixteen zero columns per row)
        const int zq = (K2p - R) >> 2;
        for (int e = tid; e < TM * zq; e += THREADS) {
            const int row = e / zq, k4 = R + (e - row * zq) * 4;
            *reinterpret_cast<u32x2*>(Gs + row * gst + k4) = u32x2{0u, 0u};
        }
    }
    __syncthreads();

    // 2. GEMM 1 + gate: fp32 accumulators from the fp32 bias, k ascending in steps of 32
    const Chunk16* w1v = reinterpret_cast<const Chunk16*>(w1p);
    const int n1 = K1p >> 5;                               // k steps
    for (int p = wave; p < R / 16; p += WAVES) {
        const Chunk16* wt = w1v + (size_t)q * G + p * 16 + r;       // k block q of the tanh column; its sigmoid column lies R further, the next k step 4 G
        const float bt = b1[p * 16 + r], bs = b1[R + p * 16 + r];
        f32x4 at[4], as[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) { at[rt] = f32x4{bt, bt, bt, bt}; as[rt] = f32x4{bs, bs, bs, bs}; }
        const uint16_t* xa = Xs + r * xs + q * 8;
        Chunk16 wtr[PF], wsr[PF];                          // the weights of the next PF k steps are in flight while the MFMAs of this one issue
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            if (u < n1) {
                wtr[u] = wt[(size_t)u * 4 * G];
                wsr[u] = wt[(size_t)u * 4 * G + R];
            }
        }
        for (int s0 = 0; s0 < n1; s0 += PF) {
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int s = s0 + u;
                if (s >= n1) break;                        // (uniform)
                const Chunk16 wtk = wtr[u], wsk = wsr[u];
                if (s + PF < n1) {
                    wtr[u] = wt[(size_t)(s + PF) * 4 * G];
                    wsr[u] = wt[(size_t)(s + PF) * 4 * G + R];
                }
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) {
                    const Chunk16 a = *reinterpret_cast<const Chunk16*>(xa + rt * 16 * xs + s * 32);
                    at[rt] = mfma32(a, wtk, at[rt]);
                    as[rt] = mfma32(a, wsk, as[rt]);
                }
            }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) Gs[(rt * 16 + q * 4 + i) * gst + p * 16 + r] = bf16_bits(tanh_<false>(at[rt][i]) * sigmoid_<false>(as[rt][i]));
    }
    __syncthreads();

    // 3. GEMM 2: residual and skip 1x1s
    const Chunk16* w2v = reinterpret_cast<const Chunk16*>(w2p);
    for (int n = wave; n < N2 / 16; n += WAVES) {
        const int col = n * 16 + r;
        const float bv = b2[col];
        f32x4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{bv, bv, bv, bv};
        const uint16_t* ga = Gs + r * gst + q * 8;
        const Chunk16* wc = w2v + (size_t)q * N2 + col;
        for (int s = 0; s < (K2p >> 5); ++s) {
            const Chunk16 wk = wc[(size_t)s * 4 * N2];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[rt] = mfma32(*reinterpret_cast<const Chunk16*>(ga + rt * 16 * gst + s * 32), wk, acc[rt]);
        }
        const bool res = n * 16 < R;                       // (uniform over the wave: R is a multiple of 16)
        // the lane's element of row tq + o, o = 16 rt + i: one lane-dependent base per tensor, the steps between rows are wave-uniform
        const int tq = t0 + q * 4;
        // What is added - x, or the skips so far - is loaded for all 16 elements before the first store, from rows clamped to the utterance's last one
        // (tq + min(o, T - 1 - tq) = min(tq + o, T - 1) >= 0), so the loads are unconditional and in flight together; only the stores are guarded.
        const int width = res ? R : S, lim = min(T - 1 - tq, TM) * width;
        const float* old = res ? x + (row0 + tq) * R + col : skips + (row0 + tq) * S + (col - R);
        float* out = res ? xo + (row0 + tq) * R + col : skips + (row0 + tq) * S + (col - R);
        f32x4 add[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) add[rt][i] = res || accumulate ? old[min((rt * 16 + i) * width, lim)] : 0.f;
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) add[rt][i] = res ? (acc[rt][i] + add[rt][i]) * RSQRT2 : add[rt][i] + acc[rt][i];
        if (t0 + TM <= T) {                                // a whole tile (uniform): 16 stores back to back, no branch between them
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i) out[(rt * 16 + i) * width] = add[rt][i];
        } else {
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (tq + rt * 16 + i < T) out[(rt * 16 + i) * width] = add[rt][i];
        }
    }
}

int layer_bf16_lds_bytes(int R, int A) { return TM * (pad32(3 * R + A) + 8 + pad32(R) + 8) * 2; }

}  // namespace

extern "C" int glowtts_pwg_supported_bf16(int R, int G, int S, int A, int max_dilation)
{
    return glowtts_pwg_supported(R, G, S, A, max_dilation) && layer_bf16_lds_bytes(R, A) <= MAX_LDS;
}

extern "C" int glowtts_pwg_layer_bf16(const float* x, const float* c, const uint16_t* w1p, const float* b1, const uint16_t* w2p, const float* b2, float* x_out,
                                      float* skips, const int32_t* frame_lengths, int B, int Lmax, int hop, int R, int S, int A, int dilation, int accumulate,
                                      void* stream)
{
    if (!x || !c || !w1p || !b1 || !w2p || !b2 || !x_out || !skips || !frame_lengths || x == x_out || bad_batch(B, Lmax, hop) ||
        !glowtts_pwg_supported_bf16(R, 2 * R, S, A, dilation))
        return GLOWTTS_E_ARG;
    const int lds = layer_bf16_lds_bytes(R, A);
    if (allow_lds<&pwg_layer_bf16_kernel>(lds) != GLOWTTS_OK) return GLOWTTS_E_LAUNCH;
    const int Tmax = Lmax * hop;
    hipLaunchKernelGGL(pwg_layer_bf16_kernel, dim3((Tmax + TM - 1) / TM, B), dim3(THREADS), (size_t)lds, static_cast<hipStream_t>(stream), x, c, w1p, b1, w2p, b2, x_out,
                       skips, frame_lengths, Lmax, hop, R, S, A, dilation, accumulate);
    GLOWTTS_NOTE_STATIC("pwg_layer_bf16");
    RET_LAUNCH();
}
