// Mel-spectrogram L1 loss of the HiFi-GAN recipe (vocoder.MelSpectrogramLoss), ONE analysis geometry (n_fft, hop, win) x Mel filters per call; f32 signals,
// float64 sums.  The contract ("Mel loss"):  X = stft(x) framed exactly as the STFT loss frames it (center = True, reflect padding by n_fft / 2, a
// periodic Hann window of `win` centred in n_fft, frames t = 0 .. T / hop);  |X|[k] = sqrt(re^2 + im^2 + 1e-9) - the floor inside the root, so X / |X| is
// defined everywhere;  mel[j] = sum_k fb[j, k] |X|[k] in ascending bin order;  m[j] = ln(max(mel[j], floor));  L_mel = mean |m_target - m_pred| over
// (B, frames, Mel).  pred and target are [B][T], every row of the full length T > n_fft / 2.
//
// Forward, two launches:
//   mel_loss_fwd      one 256-thread workgroup per frame at a time (workgroups stride over the B * (1 + T / hop) frames).  Per frame, first the target, then
//                     the prediction: pack, the LDS FFT, the real-input split per bin pair, magnitudes into an LDS row, then thread j < Mel sums filter j
//                     over its run of bins (the sparse filterbank of frontend.sparse_filterbank, staged in LDS when it fits beside the rest) and takes the
//                     log.  Neither spectrum nor a magnitude reaches HBM: the frame leaves Mel coefficients c[j] = sign(m_pred - m_target) / mel_pred (0 at
//                     equality and where the prediction sits at the floor) and one float64 sum of |m_target - m_pred| (fixed tree over the workgroup).
//   mel_loss_reduce   one workgroup: thread i sums frames i, i + 256, ... in ascending order, the same tree, then L_mel and loss (+)= weight L_mel.
// Backward, two launches:
//   mel_loss_bwd_frames  per frame: the prediction's spectrum AGAIN (pack, FFT, split - the forward kept Mel floats per frame, not the spectrum), per bin
//                     G[k] = g weight / (B frames Mel) (sum_j fb[j, k] c[j]) X[k] / |X|[k] with the filterbank read through its transpose (bin -> its filters
//                     in ascending order, CSR), written back in place as the inverse split; the transposed real DFT exactly as stft_loss_bwd_frames has it
//                     (every bin once, the end bins folded into Z[0]); times the window -> dframes [B][frames][win].
//   mel_loss_bwd_fold    stft_frames.h's fold, the body the STFT loss runs.
// No atomics, no workgroup waits on another: every value is bit-identical from run to run.  LDS per workgroup at n_fft = 2048, win 1024, Mel 80: 8 KiB
// twiddles + 8.3 KiB spectrum + 4 KiB window + 4 KiB magnitudes + 4.9 KiB filterbank + 2 KiB tree = 31.2 KiB forward; the backward has Mel floats beside
// the first three.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/glowtts_hip.h"
#include "launch_log.h"
#include "stft_frames.h"
#include "vocoder_fft.h"

namespace {

constexpr float ML_EPS = 1e-9f;
constexpr size_t ML_LDS_LIMIT = 62 * 1024;             // dynamic LDS of the forward beside its 2 KiB tree: beyond it the filterbank stays in global memory

struct ml_args {
    const float* pred;         // [B][T]
    const float* target;       // [B][T] (forward)
    const float* window;       // [win]
    const float2* twiddle;     // [n_fft / 2]
    const int32_t* fb_index;   // forward: [Mel][3] = (first bin, bin count, offset into the weights); backward: the transpose's row starts [F + 1]
    const int32_t* fb_filter;  // backward: the filter of each transposed entry [n_weights]
    const float* fb_weights;   // [n_weights]
    float* coef;               // keep: c [frames][Mel]
    double* partial;           // forward: [frames]
    const float* grad_out;     // backward: the upstream gradient, one device float
    float* dframes;            // backward: [frames][win]
    float floor, weight;
    int B, T, NF, logN, win, hop, mel, n_weights, fb_in_lds;
};

__device__ __forceinline__ float ml_mag(float2 y) { return sqrtf(y.x * y.x + y.y * y.y + ML_EPS); }

__global__ __launch_bounds__(VOC_NT) void mel_loss_fwd_kernel(const ml_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ml_smem[];
    __shared__ double red[1][VOC_NT];
    const int N = 1 << a.logN, M = N >> 1, logM = a.logN - 1, F = M + 1;
    const int tid = threadIdx.x;
    const int lpad = (N - a.win) >> 1;
    const voc_lds lds = voc_lds_stage(ml_smem, a.twiddle, a.window, M, a.win);
    float2* const X = lds.X;
    const float2* const tw = lds.tw;
    float* const mag = lds.rest;                                               // [F]
    const float* fbw = a.fb_weights;
    if (a.fb_in_lds) {
        float* w = mag + F;
        for (int i = tid; i < a.n_weights; i += VOC_NT) w[i] = a.fb_weights[i];
        fbw = w;
        __syncthreads();
    }
    // filter tid's run of bins, held to the tables' sizes
    int first = 0, count = 0, off = 0;
    if (tid < a.mel) {
        first = min(max(a.fb_index[tid * 3], 0), F);
        off = min(max(a.fb_index[tid * 3 + 2], 0), a.n_weights);
        count = min(min(max(a.fb_index[tid * 3 + 1], 0), F - first), a.n_weights - off);
    }
    const int total = a.B * a.NF;
    for (int f = blockIdx.x; f < total; f += gridDim.x) {
        const int b = f / a.NF, t = f - b * a.NF;
        float m_target = 0.f;
        double s = 0.0;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            const float* xb = (pass ? a.pred : a.target) + (int64_t)b * a.T;
            voc_pack_frame(lds, M, logM, lpad, a.win, t * a.hop - M, a.T, [&](int i) { return xb[i]; });
            voc_fft<false>(X, tw, logM, a.logN, tid);
            for (int k = tid; k <= (M >> 1); k += VOC_NT) {
                if (k == 0) {                                                  // bins 0 and M are real
                    const float2 z = X[0];
                    mag[0] = ml_mag(make_float2(z.x + z.y, 0.f));
                    mag[M] = ml_mag(make_float2(z.x - z.y, 0.f));
                    continue;
                }
                float2 yk, ymk;
                voc_split_pair(X, tw, k, M, yk, ymk);
                mag[k] = ml_mag(yk);
                mag[M - k] = ml_mag(ymk);
            }
            __syncthreads();                                                   // the magnitudes are whole; the spectrum is read
            if (tid < a.mel) {
                float mel = 0.f;
                for (int i = 0; i < count; ++i) mel += fbw[off + i] * mag[first + i];
                const float m = logf(fmaxf(mel, a.floor));
                if (pass == 0) {
                    m_target = m;
                } else {
                    const float d = m - m_target;
                    s = (double)fabsf(d);
                    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                    a.coef[(int64_t)f * a.mel + tid] = mel > a.floor ? sgn / mel : 0.f;
                }
            }
            // (the next pass writes the magnitudes only after the barriers of its own pack and FFT)
        }
        red[0][tid] = s;
        voc_tree<1>(red, tid);
        if (tid == 0) a.partial[f] = red[0][0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(VOC_NT) void mel_loss_reduce_kernel(const double* __restrict__ partial, float* __restrict__ terms, float* __restrict__ loss, int frames,
                                                                 int mel, float weight, int accumulate)
{
    __shared__ double red[1][VOC_NT];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int f = tid; f < frames; f += VOC_NT) s += partial[f];
    red[0][tid] = s;
    voc_tree<1>(red, tid);
    if (tid == 0) {
        const float l = (float)(red[0][0] / ((double)frames * (double)mel));
        terms[0] = l;
        loss[0] = accumulate ? loss[0] + weight * l : weight * l;
    }
}

__global__ __launch_bounds__(VOC_NT) void mel_loss_bwd_frames_kernel(const ml_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ml_smem[];
    const int N = 1 << a.logN, M = N >> 1, logM = a.logN - 1;
    const int tid = threadIdx.x;
    const int lpad = (N - a.win) >> 1;
    const voc_lds lds = voc_lds_stage(ml_smem, a.twiddle, a.window, M, a.win);
    float2* const X = lds.X;
    const float2* const tw = lds.tw;
    float* const c = lds.rest;                                                 // [Mel]
    const int total = a.B * a.NF;
    const float scale = a.grad_out[0] * a.weight * (float)(1.0 / ((double)total * (double)a.mel));
    for (int f = blockIdx.x; f < total; f += gridDim.x) {
        const int b = f / a.NF, t = f - b * a.NF;
        const float* xb = a.pred + (int64_t)b * a.T;
        for (int j = tid; j < a.mel; j += VOC_NT) c[j] = a.coef[(int64_t)f * a.mel + j];
        voc_pack_frame(lds, M, logM, lpad, a.win, t * a.hop - M, a.T, [&](int i) { return xb[i]; });      // (its barrier publishes c too)
        voc_fft<false>(X, tw, logM, a.logN, tid);
        // dL / d(re, im) of bin k with spectrum y: the transposed filterbank's row k (held to the tables' sizes) over c, in ascending filter order
        auto grad = [&](int k, float2 y) {
            const int e0 = min(max(a.fb_index[k], 0), a.n_weights), e1 = min(max(a.fb_index[k + 1], e0), a.n_weights);
            float s = 0.f;
            for (int e = e0; e < e1; ++e) s += a.fb_weights[e] * c[min((unsigned)a.fb_filter[e], (unsigned)(a.mel - 1))];
            const float q = scale * s / ml_mag(y);
            return make_float2(q * y.x, q * y.y);
        };
        // in place: the thread that reads the pair (Z[k], Z[M-k]) writes the gradient's pair
        for (int k = tid; k <= (M >> 1); k += VOC_NT) {
            if (k == 0) {                                                      // the end bins count once: Re G[0] + (-1)^n Re G[M]
                const float2 z = X[0];
                const float g0 = grad(0, make_float2(z.x + z.y, 0.f)).x, gm = grad(M, make_float2(z.x - z.y, 0.f)).x;
                X[0] = make_float2(g0 + gm, g0 - gm);
                continue;
            }
            float2 yk, ymk;
            voc_split_pair(X, tw, k, M, yk, ymk);
            voc_unsplit_pair(X, tw, k, M, grad(k, yk), grad(M - k, ymk));
        }
        __syncthreads();
        voc_fft<true>(X, tw, logM, a.logN, tid);
        float* fr = a.dframes + (int64_t)f * a.win;
        voc_unpack_frame(X, logM, lpad, a.win, [&](int j, float y) { fr[j] = y * lds.wnd[j]; });
    }
}

bool ml_bad_dims(int B, int T, int n_fft, int win, int hop, int mel, int n_weights)
{
    return !glowtts_mel_loss_supported(n_fft, win, hop, T, mel) || voc_frames_bad_batch(B, T, hop) || n_weights < 1 || n_weights > mel * (n_fft / 2 + 1);
}

}  // namespace

extern "C" int glowtts_mel_loss_supported(int n_fft, int win_length, int hop, int T, int n_mel)
{
    return glowtts_stft_loss_supported(n_fft, win_length, hop, T) && n_mel >= 4 && n_mel <= 256;
}

extern "C" int64_t glowtts_mel_loss_keep_floats(int B, int T, int hop, int n_mel)
{
    if (B < 1 || T < 1 || hop < 1 || n_mel < 1) return 0;
    return (int64_t)B * (1 + T / hop) * n_mel;
}

extern "C" int64_t glowtts_mel_loss_work_floats(int B, int T, int win_length, int hop)
{
    if (B < 1 || T < 1 || win_length < 1 || hop < 1) return 0;
    return (int64_t)B * (1 + T / hop) * (2 + win_length);
}

extern "C" int glowtts_mel_loss_forward(const float* pred, const float* target, const float* window, const float* twiddle, const int32_t* fb_index,
                                        const float* fb_weights, float* keep, float* work, float* terms, float* loss, int B, int T, int n_fft, int win_length,
                                        int hop, int n_mel, int n_weights, float floor, float weight, int accumulate, void* stream)
{
    if (!pred || !target || !window || !twiddle || !fb_index || !fb_weights || !keep || !work || !terms || !loss ||
        ml_bad_dims(B, T, n_fft, win_length, hop, n_mel, n_weights) || !(floor > 0.f) || (reinterpret_cast<uintptr_t>(work) & 7))
        return GLOWTTS_E_ARG;
    const int NF = 1 + T / hop, F = n_fft / 2 + 1;
    const int64_t frames = (int64_t)B * NF;
    ml_args a = {};
    a.pred = pred; a.target = target; a.window = window; a.twiddle = reinterpret_cast<const float2*>(twiddle);
    a.fb_index = fb_index; a.fb_weights = fb_weights; a.coef = keep; a.partial = reinterpret_cast<double*>(work);
    a.floor = floor; a.weight = weight; a.B = B; a.T = T; a.NF = NF; a.logN = voc_log2(n_fft); a.win = win_length; a.hop = hop; a.mel = n_mel; a.n_weights = n_weights;
    a.fb_in_lds = voc_lds_bytes(n_fft, win_length, F + n_weights) <= ML_LDS_LIMIT;
    GLOWTTS_NOTE_STATIC("mel_loss_fwd");
    hipLaunchKernelGGL(mel_loss_fwd_kernel, dim3(voc_frames_grid((int)frames)), dim3(VOC_NT), voc_lds_bytes(n_fft, win_length, F + (a.fb_in_lds ? n_weights : 0)),
                       static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("mel_loss_reduce");
    hipLaunchKernelGGL(mel_loss_reduce_kernel, dim3(1), dim3(VOC_NT), 0, static_cast<hipStream_t>(stream), a.partial, terms, loss, (int)frames, n_mel, weight, accumulate);
    RET_LAUNCH();
}

extern "C" int glowtts_mel_loss_backward(const float* pred, const float* keep, const float* grad_out, const float* window, const float* twiddle,
                                         const int32_t* fbt_start, const int32_t* fbt_filter, const float* fbt_weights, float* work, float* dpred, int B, int T,
                                         int n_fft, int win_length, int hop, int n_mel, int n_weights, float weight, int accumulate, void* stream)
{
    if (!pred || !keep || !grad_out || !window || !twiddle || !fbt_start || !fbt_filter || !fbt_weights || !work || !dpred ||
        ml_bad_dims(B, T, n_fft, win_length, hop, n_mel, n_weights))
        return GLOWTTS_E_ARG;
    const int NF = 1 + T / hop;
    const int64_t frames = (int64_t)B * NF;
    ml_args a = {};
    a.pred = pred; a.window = window; a.twiddle = reinterpret_cast<const float2*>(twiddle);
    a.fb_index = fbt_start; a.fb_filter = fbt_filter; a.fb_weights = fbt_weights; a.coef = const_cast<float*>(keep);
    a.grad_out = grad_out; a.dframes = work + frames * 2;
    a.weight = weight; a.B = B; a.T = T; a.NF = NF; a.logN = voc_log2(n_fft); a.win = win_length; a.hop = hop; a.mel = n_mel; a.n_weights = n_weights;
    GLOWTTS_NOTE_STATIC("mel_loss_bwd_frames");
    hipLaunchKernelGGL(mel_loss_bwd_frames_kernel, dim3(voc_frames_grid((int)frames)), dim3(VOC_NT), voc_lds_bytes(n_fft, win_length, n_mel),
                       static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return GLOWTTS_E_LAUNCH;
    GLOWTTS_NOTE_STATIC("mel_loss_bwd_fold");
    hipLaunchKernelGGL(voc_frames_fold_kernel, dim3((T + 255) / 256, B), dim3(256), 0, static_cast<hipStream_t>(stream), a.dframes, dpred, T, NF, n_fft, win_length, hop,
                       accumulate);
    RET_LAUNCH();
}
