// The LDS FFT and the framing around it, shared by the Griffin-Lim vocoder (vocoder_ops.hip), the analysis front end (frontend_ops.hip), the STFT loss
// (stft_loss_ops.hip) and the mel loss (mel_loss_ops.hip): complex helpers, numpy's reflect index, the one-slot-per-32-elements pad of the spectrum buffer, the in-place radix-4 FFT of n_fft / 2
// complex points that a real frame of n_fft samples packs into, and - each written once - the LDS layout with its table staging, the frame packer (gather,
// window, pack bit-reversed), the real-input split of a bin pair and its inverse, the unpack of a frame's samples under the window, and the host's size and
// range checks.  256-thread workgroups.  Bank-conflict accounting of the pad: see the header of vocoder_ops.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int VOC_NT = 256;

__device__ __forceinline__ int voc_pad(int i) { return i + (i >> 5); }
__device__ __forceinline__ float2 voc_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 voc_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 voc_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 voc_mulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }      // a * conj(b)

// index of sample s of a signal of L samples under reflect padding (numpy's "reflect": period 2 (L - 1))
__device__ __forceinline__ int voc_reflect(int s, int L) {
    if (s >= 0 && s < L) return s;
    if (L == 1) return 0;
    const int p = 2 * (L - 1);
    s %= p;
    if (s < 0) s += p;
    return s < L ? s : p - s;
}

// In-place complex FFT of M = 2^logM points in LDS (elements at voc_pad(i)); tw[k] = exp(-2 pi i k / N), N = 2 M = 2^logN.
// Forward: decimation in time, input in bit-reversed order, output in natural order.  Inverse (unnormalised): decimation in frequency, natural order in,
// bit-reversed order out.  Ends with a barrier.
template <bool INV>
__device__ __forceinline__ void voc_fft(float2* X, const float2* tw, int logM, int logN, int tid)
{
    const int M = 1 << logM;
    if (!INV) {
        int lh = 0;
        if (logM & 1) {
            for (int j = tid; j < (M >> 1); j += VOC_NT) {
                const int i0 = voc_pad(2 * j), i1 = voc_pad(2 * j + 1);
                const float2 a = X[i0], b = X[i1];
                X[i0] = voc_add(a, b);
                X[i1] = voc_sub(a, b);
            }
            __syncthreads();
            lh = 1;
        }
        for (; lh < logM; lh += 2) {
            const int h = 1 << lh;
            for (int j = tid; j < (M >> 2); j += VOC_NT) {
                const int pos = j & (h - 1), base = ((j >> lh) << (lh + 2)) + pos;
                const float2 w1 = tw[pos << (logN - 1 - lh)], w2 = tw[pos << (logN - 2 - lh)];
                const int i0 = voc_pad(base), i1 = voc_pad(base + h), i2 = voc_pad(base + 2 * h), i3 = voc_pad(base + 3 * h);
                const float2 a0 = X[i0], a1 = X[i1], a2 = X[i2], a3 = X[i3];
                float2 t = voc_mul(a1, w1);
                const float2 b0 = voc_add(a0, t), b1 = voc_sub(a0, t);
                t = voc_mul(a3, w1);
                const float2 b2 = voc_add(a2, t), b3 = voc_sub(a2, t);
                t = voc_mul(b2, w2);
                X[i0] = voc_add(b0, t);
                X[i2] = voc_sub(b0, t);
                t = voc_mul(b3, w2);
                t = make_float2(t.y, -t.x);                    // W_{4h}^{pos + h} = -i W_{4h}^{pos}
                X[i1] = voc_add(b1, t);
                X[i3] = voc_sub(b1, t);
            }
            __syncthreads();
        }
    } else {
        for (int lh = logM - 2; lh >= 0; lh -= 2) {
            const int h = 1 << lh;
            for (int j = tid; j < (M >> 2); j += VOC_NT) {
                const int pos = j & (h - 1), base = ((j >> lh) << (lh + 2)) + pos;
                const float2 w1 = tw[pos << (logN - 1 - lh)], w2 = tw[pos << (logN - 2 - lh)];
                const int i0 = voc_pad(base), i1 = voc_pad(base + h), i2 = voc_pad(base + 2 * h), i3 = voc_pad(base + 3 * h);
                const float2 a0 = X[i0], a1 = X[i1], a2 = X[i2], a3 = X[i3];
                const float2 b0 = voc_add(a0, a2), b2 = voc_mulc(voc_sub(a0, a2), w2);
                const float2 b1 = voc_add(a1, a3);
                float2 t = voc_mulc(voc_sub(a1, a3), w2);
                const float2 b3 = make_float2(-t.y, t.x);      // conj(W_{4h}^{pos + h}) = i conj(W_{4h}^{pos})
                X[i0] = voc_add(b0, b1);
                X[i1] = voc_mulc(voc_sub(b0, b1), w1);
                X[i2] = voc_add(b2, b3);
                X[i3] = voc_mulc(voc_sub(b2, b3), w1);
            }
            __syncthreads();
        }
        if (logM & 1) {
            for (int j = tid; j < (M >> 1); j += VOC_NT) {
                const int i0 = voc_pad(2 * j), i1 = voc_pad(2 * j + 1);
                const float2 a = X[i0], b = X[i1];
                X[i0] = voc_add(a, b);
                X[i1] = voc_sub(a, b);
            }
            __syncthreads();
        }
    }
}

// ---- the framing around the FFT -------------------------------------------------------------------------------------------------------------------------
// The dynamic LDS of a frame kernel: tw [M] | X [voc_pad(M) + 1] | wnd [win] | rest (the caller's own floats, counted by voc_lds_bytes' extra_floats)
struct voc_lds {
    float2* tw;
    float2* X;
    float* wnd;
    float* rest;
};
// carves the layout out of `smem` and stages the twiddle and window tables; ends with a barrier
__device__ __forceinline__ voc_lds voc_lds_stage(unsigned char* smem, const float2* twiddle, const float* window, int M, int win)
{
    voc_lds l;
    l.tw = reinterpret_cast<float2*>(smem);
    l.X = l.tw + M;
    l.wnd = reinterpret_cast<float*>(l.X + voc_pad(M) + 1);
    l.rest = l.wnd + win;
    for (int i = threadIdx.x; i < M; i += VOC_NT) l.tw[i] = twiddle[i];
    for (int i = threadIdx.x; i < win; i += VOC_NT) l.wnd[i] = window[i];
    __syncthreads();
    return l;
}

// The frame whose position 0 is sample `start` (= t hop - n_fft / 2 under center = True) of a signal of L samples, reflect-padded: positions under the window
// (lpad <= n < lpad + win) take sample(s) at the reflected index s, times the window; the others are zero.  Packed z[m] = y[2m] + i y[2m+1] and written at the
// bit-reversed index, the order voc_fft<false> reads.  Ends with a barrier.
template <typename Sample>
__device__ __forceinline__ void voc_pack_frame(const voc_lds& l, int M, int logM, int lpad, int win, int start, int L, Sample sample)
{
    for (int m = threadIdx.x; m < M; m += VOC_NT) {
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int n = 2 * m + e, j = n - lpad;
            v[e] = 0.f;
            if (j >= 0 && j < win) v[e] = sample(voc_reflect(start + n, L)) * l.wnd[j];
        }
        l.X[voc_pad((int)(__brev((unsigned)m) >> (32 - logM)))] = make_float2(v[0], v[1]);
    }
    __syncthreads();
}

// The real-input split of the packed spectrum Z for the bin pair (k, M - k), 0 < k <= M / 2: Y[k] = E + W^k O and Y[M-k] = conj(E - W^k O).  (Bins 0 and M
// are real, Z[0].x +- Z[0].y: the callers' own lines.)
__device__ __forceinline__ void voc_split_pair(const float2* X, const float2* tw, int k, int M, float2& yk, float2& ymk)
{
    const float2 za = X[voc_pad(k)], zb = X[voc_pad(M - k)];
    const float2 e = make_float2(0.5f * (za.x + zb.x), 0.5f * (za.y - zb.y));          // (Z[k] + conj Z[M-k]) / 2
    const float2 d = make_float2(0.5f * (za.x - zb.x), 0.5f * (za.y + zb.y));          // (Z[k] - conj Z[M-k]) / 2
    const float2 wo = voc_mul(make_float2(d.y, -d.x), tw[k]);                          // W^k O,  O = d / i
    yk = voc_add(e, wo);
    ymk = voc_sub(e, wo);
    ymk.y = -ymk.y;
}
// its inverse: the packed spectrum's Z[k], Z[M-k] from Y[k], Y[M-k]
__device__ __forceinline__ void voc_unsplit_pair(float2* X, const float2* tw, int k, int M, float2 yk, float2 ymk)
{
    const float2 e = make_float2(0.5f * (yk.x + ymk.x), 0.5f * (yk.y - ymk.y));
    const float2 o = voc_mulc(make_float2(0.5f * (yk.x - ymk.x), 0.5f * (yk.y + ymk.y)), tw[k]);
    X[voc_pad(k)] = make_float2(e.x - o.y, e.y + o.x);                                 // Z[k] = E + i O
    X[voc_pad(M - k)] = make_float2(e.x + o.y, o.x - e.y);                             // Z[M-k] = conj(E - i O)
}

// After voc_fft<true>: hands put(j, y) the (unnormalised) sample at window position j < win, read from the bit-reversed packed frame.  Ends with a barrier.
template <typename Put>
__device__ __forceinline__ void voc_unpack_frame(const float2* X, int logM, int lpad, int win, Put put)
{
    for (int j = threadIdx.x; j < win; j += VOC_NT) {
        const int n = lpad + j;
        const float2 z = X[voc_pad((int)(__brev((unsigned)(n >> 1)) >> (32 - logM)))];
        put(j, (n & 1) ? z.y : z.x);
    }
    __syncthreads();
}

// ---- host ----
int voc_log2(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }
size_t voc_lds_bytes(int n_fft, int win, int extra_floats) { const int M = n_fft / 2; return (size_t)(M + M + (M >> 5) + 1) * 8 + (size_t)(win + extra_floats) * 4; }
bool voc_fft_supported(int n_fft, int win) { return n_fft >= 256 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0 && win >= 1 && win <= n_fft; }

}  // namespace
