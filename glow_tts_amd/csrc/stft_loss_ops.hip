// Multi-resolution STFT loss of the Parallel WaveGAN recipe (vocoder.MultiResolutionSTFTLoss), ONE resolution (n_fft, hop, win) per call; f32 signals,
// float64 sums.  The contract ("STFT loss"):  X = stft(x) with center = True, reflect padding by n_fft / 2, a periodic Hann window of `win`
// centred in n_fft, frames t = 0 .. T / hop;  |X| = sqrt(max(re^2 + im^2, 1e-7));  L_sc = ||Y| - |X||_F / ||Y||_F over the whole batch,
// L_mag = mean |log |Y| - log |X||.  pred and target are [B][T], every row of the full length T (T > n_fft / 2: one reflection reaches every padded sample).
//
// Forward, two launches:
//   stft_loss_fwd     one 256-thread workgroup per frame at a time (workgroups stride over the B * (1 + T / hop) frames).  Per frame, first the target, then
//                     the prediction: gather under reflect padding, window, pack z[m] = x[2m] + i x[2m+1] bit-reversed, the LDS FFT of vocoder_fft.h, the
//                     real-input split per bin pair (k, n_fft/2 - k), magnitudes.  HBM gets |Y|, |X| and the prediction's complex spectrum (kept for the
//                     backward); the thread that wrote |Y|[k] is the one that reads it back beside |X|[k].  The frame's three sums - (|Y| - |X|)^2, |Y|^2,
//                     |log |Y| - log |X|| - are accumulated in float64 per thread in ascending bin order and reduced over the workgroup by a fixed tree.
//   stft_loss_reduce  one workgroup: thread i sums frames i, i + 256, ... in ascending order, the same tree, then L_sc, L_mag, the backward's coefficient
//                     1 / (||Y| - |X|| ||Y||) (0 when the two spectra are equal: the subgradient torch takes) and loss (+)= weight (L_sc + L_mag).
// Backward, two launches:
//   stft_loss_bwd_frames  per frame: G = g weight [(|X| - |Y|) coef + sign(|X| - |Y|) / (N |X|)] X / |X| per bin, 0 where the clamp is active
//                     (re^2 + im^2 < 1e-7); the transposed real DFT d x[n] = Re sum_{k <= n_fft/2} G[k] exp(+2 pi i k n / n_fft) as the inverse split and
//                     the inverse LDS FFT (bins 0 and n_fft / 2 count once, the others once too - NOT the Hermitian doubling of an inverse real FFT, hence
//                     the doubled end bins below); times the window -> dframes [B][frames][win].
//   stft_loss_bwd_fold    per sample: the overlap-add as a GATHER over the ceil(win / hop) frames that cover a padded position, in ascending frame order,
//                     taken at the sample's own position and at the at most two padded positions that reflect onto it (left edge first).
// No atomics, no workgroup waits on another: every value is bit-identical from run to run.  LDS per workgroup at n_fft = 2048, win 1200: 8 KiB twiddles +
// 8.3 KiB spectrum + 4.7 KiB window + 6 KiB reduction tree = 27 KiB.
// The LDS layout, the frame packer, the split and its inverse and the frame unpack are vocoder_fft.h's, shared with vocoder_ops.hip and frontend_ops.hip; the
// reduction tree and the fold (the overlap-add kernel, logged here as stft_loss_bwd_fold) are stft_frames.h's, shared with mel_loss_ops.hip; this file keeps the
// magnitudes with their float64 sums and the gradient per bin.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/glowtts_hip.h"
#include "launch_log.h"
#include "stft_frames.h"
#include "vocoder_fft.h"

namespace {

constexpr float SL_CLAMP = 1e-7f;

struct sl_args {
    const float* pred;         // [B][T]
    const float* target;       // [B][T]
    const float* window;       // [win]
    const float2* twiddle;     // [n_fft / 2]
    float* spec;               // keep: the prediction's spectrum [frames][F][2]
    float* mag_x;              // keep: |X| [frames][F]
    float* mag_y;              // keep: |Y| [frames][F]
    double* partial;           // forward: [frames][3]
    const float* terms;        // backward: (L_sc, L_mag, coef)
    const float* grad_out;     // backward: the upstream gradient, one device float
    float* dframes;            // backward: [frames][win]
    float weight;
    int B, T, NF, logN, win, hop;
};

__global__ __launch_bounds__(VOC_NT) void stft_loss_fwd_kernel(const sl_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sl_smem[];
    __shared__ double red[3][VOC_NT];
    const int N = 1 << a.logN, M = N >> 1, logM = a.logN - 1, F = M + 1;
    const int tid = threadIdx.x;
    const int lpad = (N - a.win) >> 1;
    const voc_lds lds = voc_lds_stage(sl_smem, a.twiddle, a.window, M, a.win);
    float2* const X = lds.X;
    const float2* const tw = lds.tw;
    const int total = a.B * a.NF;
    for (int f = blockIdx.x; f < total; f += gridDim.x) {
        const int b = f / a.NF, t = f - b * a.NF;
        float* const my = a.mag_y + (int64_t)f * F;
        float* const mx = a.mag_x + (int64_t)f * F;
        float2* const sp = reinterpret_cast<float2*>(a.spec) + (int64_t)f * F;
        double s_sc = 0.0, s_y = 0.0, s_mag = 0.0;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            const float* xb = (pass ? a.pred : a.target) + (int64_t)b * a.T;
            voc_pack_frame(lds, M, logM, lpad, a.win, t * a.hop - M, a.T, [&](int s) { return xb[s]; });
            voc_fft<false>(X, tw, logM, a.logN, tid);
            // one bin: the target's magnitude goes out; the prediction's is set beside the target's, which this very thread wrote in pass 0
            auto bin = [&](int k, float2 y) {
                const float m = sqrtf(fmaxf(y.x * y.x + y.y * y.y, SL_CLAMP));
                if (pass == 0) { my[k] = m; return; }
                sp[k] = y;
                mx[k] = m;
                const float ym = my[k], d = ym - m;
                s_sc += (double)(d * d);
                s_y += (double)(ym * ym);
                s_mag += (double)fabsf(logf(ym) - logf(m));
            };
            for (int k = tid; k <= (M >> 1); k += VOC_NT) {
                if (k == 0) {                                                  // bins 0 and M are real
                    const float2 z = X[0];
                    bin(0, make_float2(z.x + z.y, 0.f));
                    bin(M, make_float2(z.x - z.y, 0.f));
                    continue;
                }
                float2 yk, ymk;
                voc_split_pair(X, tw, k, M, yk, ymk);
                bin(k, yk);
                if (M - k != k) bin(M - k, ymk);
            }
            __syncthreads();                                                   // the spectrum is read: the next gather may overwrite it
        }
        red[0][tid] = s_sc;
        red[1][tid] = s_y;
        red[2][tid] = s_mag;
        voc_tree<3>(red, tid);
        if (tid < 3) a.partial[(int64_t)f * 3 + tid] = red[tid][0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(VOC_NT) void stft_loss_reduce_kernel(const double* __restrict__ partial, float* __restrict__ terms, float* __restrict__ loss, int frames,
                                                                  int F, float weight, int accumulate)
{
    __shared__ double red[3][VOC_NT];
    const int tid = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int f = tid; f < frames; f += VOC_NT) {
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] += partial[(int64_t)f * 3 + i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) red[i][tid] = s[i];
    voc_tree<3>(red, tid);
    if (tid == 0) {
        const double nd = sqrt(red[0][0]), ny = sqrt(red[1][0]);
        const float sc = (float)(nd / ny), mg = (float)(red[2][0] / ((double)frames * (double)F));
        terms[0] = sc;
        terms[1] = mg;
        terms[2] = nd > 0.0 ? (float)(1.0 / (nd * ny)) : 0.f;
        const float l = weight * (sc + mg);
        loss[0] = accumulate ? loss[0] + l : l;
    }
}

__global__ __launch_bounds__(VOC_NT) void stft_loss_bwd_frames_kernel(const sl_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sl_smem[];
    const int N = 1 << a.logN, M = N >> 1, logM = a.logN - 1, F = M + 1;
    const int tid = threadIdx.x;
    const int lpad = (N - a.win) >> 1;
    const voc_lds lds = voc_lds_stage(sl_smem, a.twiddle, a.window, M, a.win);
    float2* const X = lds.X;
    const float2* const tw = lds.tw;
    const int total = a.B * a.NF;
    const float g = a.grad_out[0] * a.weight, coef = a.terms[2], inv_n = (float)(1.0 / ((double)total * (double)F));
    for (int f = blockIdx.x; f < total; f += gridDim.x) {
        const float* const my = a.mag_y + (int64_t)f * F;
        const float* const mx = a.mag_x + (int64_t)f * F;
        const float2* const sp = reinterpret_cast<const float2*>(a.spec) + (int64_t)f * F;
        // dL / d(re, im) of one bin
        auto grad = [&](int k) {
            const float2 x = sp[k];
            if (x.x * x.x + x.y * x.y < SL_CLAMP) return make_float2(0.f, 0.f);
            const float m = mx[k], d = m - my[k];
            const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            const float q = g * (d * coef + sgn * inv_n / m) / m;
            return make_float2(q * x.x, q * x.y);
        };
        for (int k = tid; k <= (M >> 1); k += VOC_NT) {
            if (k == 0) {                                                      // the end bins count once: Re G[0] + (-1)^n Re G[M]
                const float g0 = grad(0).x, gm = grad(M).x;
                X[0] = make_float2(g0 + gm, g0 - gm);
                continue;
            }
            voc_unsplit_pair(X, tw, k, M, grad(k), grad(M - k));
        }
        __syncthreads();
        voc_fft<true>(X, tw, logM, a.logN, tid);
        float* fr = a.dframes + (int64_t)f * a.win;
        voc_unpack_frame(X, logM, lpad, a.win, [&](int j, float y) { fr[j] = y * lds.wnd[j]; });
    }
}

bool sl_bad_dims(int B, int T, int n_fft, int win, int hop)
{
    return !glowtts_stft_loss_supported(n_fft, win, hop, T) || voc_frames_bad_batch(B, T, hop);
}

}  // namespace

extern "C" int glowtts_stft_loss_supported(int n_fft, int win_length, int hop, int T)
{
    return voc_fft_supported(n_fft, win_length) && hop >= 1 && hop <= win_length && T > n_fft / 2 && T <= (1 << 29);
}

extern "C" int64_t glowtts_stft_loss_keep_floats(int B, int T, int n_fft, int hop)
{
    if (B < 1 || T < 1 || n_fft < 2 || hop < 1) return 0;
    return (int64_t)B * (1 + T / hop) * (n_fft / 2 + 1) * 4;
}

extern "C" int64_t glowtts_stft_loss_work_floats(int B, int T, int win_length, int hop)
{
    if (B < 1 || T < 1 || win_length < 1 || hop < 1) return 0;
    return (int64_t)B * (1 + T / hop) * (6 + win_length);
}

extern "C" int glowtts_stft_loss_forward(const float* pred, const float* target, const float* window, const float* twiddle, float* keep, float* work, float* terms,
                                         float* loss, int B, int T, int n_fft, int win_length, int hop, float weight, int accumulate, void* stream)
{
    if (!pred || !target || !window || !twiddle || !keep || !work || !terms || !loss || sl_bad_dims(B, T, n_fft, win_length, hop) ||
        (reinterpret_cast<uintptr_t>(work) & 7) || (reinterpret_cast<uintptr_t>(keep) & 7))
        return GLOWTTS_E_ARG;
    const int NF = 1 + T / hop, F = n_fft / 2 + 1;
    const int64_t frames = (int64_t)B * NF;
    sl_args a = {};
    a.pred = pred; a.target = target; a.window = window; a.twiddle = reinterpret_cast<const float2*>(twiddle);
    a.spec = keep; a.mag_x = keep + frames * F * 2; a.mag_y = keep + frames * F * 3; a.partial = reinterpret_cast<double*>(work);
    a.weight = weight; a.B = B; a.T = T; a.NF = NF; a.logN = voc_log2(n_fft); a.win = win_length; a.hop = hop;
    GLOWTTS_NOTE_STATIC("stft_loss_fwd");
    hipLaunchKernelGGL(stft_loss_fwd_kernel, dim3(voc_frames_grid((int)frames)), dim3(VOC_NT), voc_lds_bytes(n_fft, win_length, 0), static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("stft_loss_reduce");
    hipLaunchKernelGGL(stft_loss_reduce_kernel, dim3(1), dim3(VOC_NT), 0, static_cast<hipStream_t>(stream), a.partial, terms, loss, (int)frames, F, weight, accumulate);
    RET_LAUNCH();
}

extern "C" int glowtts_stft_loss_backward(const float* keep, const float* terms, const float* grad_out, const float* window, const float* twiddle, float* work,
                                          float* dpred, int B, int T, int n_fft, int win_length, int hop, float weight, int accumulate, void* stream)
{
    if (!keep || !terms || !grad_out || !window || !twiddle || !work || !dpred || sl_bad_dims(B, T, n_fft, win_length, hop) ||
        (reinterpret_cast<uintptr_t>(keep) & 7))
        return GLOWTTS_E_ARG;
    const int NF = 1 + T / hop, F = n_fft / 2 + 1;
    const int64_t frames = (int64_t)B * NF;
    sl_args a = {};
    a.window = window; a.twiddle = reinterpret_cast<const float2*>(twiddle);
    a.spec = const_cast<float*>(keep); a.mag_x = a.spec + frames * F * 2; a.mag_y = a.spec + frames * F * 3;
    a.terms = terms; a.grad_out = grad_out; a.dframes = work + frames * 6;
    a.weight = weight; a.B = B; a.T = T; a.NF = NF; a.logN = voc_log2(n_fft); a.win = win_length; a.hop = hop;
    GLOWTTS_NOTE_STATIC("stft_loss_bwd_frames");
    hipLaunchKernelGGL(stft_loss_bwd_frames_kernel, dim3(voc_frames_grid((int)frames)), dim3(VOC_NT), voc_lds_bytes(n_fft, win_length, 0), static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("stft_loss_bwd_fold");
    hipLaunchKernelGGL(voc_frames_fold_kernel, dim3((T + 255) / 256, B), dim3(256), 0, static_cast<hipStream_t>(stream), a.dframes, dpred, T, NF, n_fft, win_length, hop,
                       accumulate);
    RET_LAUNCH();
}
