// The LDS FFT shared by the Griffin-Lim vocoder (vocoder_ops.hip) and the analysis front end (frontend_ops.hip): complex helpers, numpy's reflect index,
// the one-slot-per-32-elements pad of the spectrum buffer and the in-place radix-4 FFT of n_fft / 2 complex points that a real frame of n_fft samples packs
// into.  256-thread workgroups.  Bank-conflict accounting of the pad: see the header of vocoder_ops.hip.
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

}  // namespace
