// Analysis front end on the device (what Pattern_Generator.py and the wav references of Inference.py need): wav -> normalised mel in ONE launch, and the
// YIN pitch track of GR mode.  The arithmetic is glow_tts_amd/audio.py's (`mel_generate`, `yin_pitch`) in fp32; the LDS FFT and the framing around it (LDS layout,
// frame packer, real-input split) are vocoder_fft.h's, shared with the vocoder and the STFT loss; the pre-emphasis is this file's sample lambda.
//
// mel_analysis_kernel, one 256-thread workgroup per frame at a time, workgroups stride over the B * T frames; window and twiddles are staged in LDS once:
//   HBM -> LDS   the win_length samples under the window, gathered with the pre-emphasis applied on the fly: y[s] = x[s] - p x[s-1], y[0] = x[0]; the reflect
//                padding applies to y (reflect the index, then difference).  Windowed, packed z[m] = y[2m] + i y[2m+1], written at the bit-reversed index
//   LDS          complex FFT of n_fft / 2 points (voc_fft), in place
//   LDS          per bin pair (k, n_fft/2 - k) the real-input split; |Y_k| goes to LDS (F floats) - the complex spectrum is never formed in HBM
//   LDS          mel projection with a SPARSE filterbank: filter j covers bins [first_j, first_j + count_j) (a Slaney triangle; every bin lies in at most two),
//                weights packed back to back.  A wave takes filters j = wave, wave + 4, ...; its lanes stride over the filter's bins, then a butterfly
//                reduction: a fixed order, no atomics - bit-identical from run to run and independent of the batch around the utterance
//   LDS -> HBM   20 log10(m + 1e-7), 2 max_abs (db - min_db) / (-min_db) - max_abs, clipped to +- max_abs: one coalesced row of Mel floats per frame
// Frames at t >= T_b = 1 + L_b / hop are written as -max_abs (the collater's pad value); so is every frame of an utterance with L_b > ldx (a caller error,
// as for glowtts_stft_f32: the kernel never reads beyond ldx).
// LDS per workgroup at n_fft = 2048, win 1024, 80 mels: 8 KiB twiddles + 8.3 KiB spectrum + 4 KiB window + 4 KiB magnitudes + 0.3 KiB mel row = 24.6 KiB
// -> 6 workgroups per CU (160 KiB).  Bank conflicts: the FFT's are the vocoder's (see vocoder_ops.hip).  The split writes mag[k] ascending and mag[M - k]
// descending with unit lane stride: conflict-free.  The projection reads mag[first + lane + 64 i] and the weights with unit lane stride: conflict-free.
//
// yin_kernel, one 256-thread workgroup per analysis frame at a time, striding over B * T:
//   HBM -> LDS   the w_len samples of the frame; the centred reflect padding of (w_step + w_len - L % w_step) / 2 samples is index arithmetic (it may fold
//                more than once on a short clip)
//   LDS          d(tau) = sum_{j < w_len - tau} (x_j - x_{j+tau})^2 DIRECTLY (a sum of squares: no cancellation; the FFT autocorrelation form loses digits
//                in fp32).  A wave takes four consecutive taus at a time (5 LDS reads per 4 terms), lanes stride over j, butterfly reduction: a fixed order
//   LDS          running sum over tau by one thread (sequential: the order is the definition's), cm(tau) = d tau / (sum + 1e-8) by all threads, then the
//                decision by one thread: the first tau >= tau_min with cm < thresh, walked forward while cm[tau + 1] < cm[tau]; pitch = sample_rate / tau
// LDS: (w_len + 2 tau_max) floats, 5.9 KiB at 1024 / 240.  x_j and x_{j+tau} are read with unit lane stride: conflict-free.
// Both kernels use no scratch and no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/glowtts_hip.h"
#include "launch_log.h"
#include "device_common.h"
#include "vocoder_fft.h"

namespace {

struct mel_args {
    const float* x;            // [B][ldx]
    const int32_t* lengths;    // [B] samples
    const float* window;       // [win]
    const float2* twiddle;     // [n_fft / 2]
    const int32_t* fb_index;   // [Mel][3]: first bin, bin count, offset into fb_weight
    const float* fb_weight;    // [nw]
    float* mel;                // [B][T][Mel]
    float p, min_db, max_abs;
    int B, T, ldx, Mel, nw, logN, win, hop;
};

__global__ __launch_bounds__(VOC_NT) void mel_analysis_kernel(const mel_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fe_smem[];
    const int N = 1 << a.logN, M = N >> 1, logM = a.logN - 1, F = M + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lpad = (N - a.win) >> 1;
    const voc_lds lds = voc_lds_stage(fe_smem, a.twiddle, a.window, M, a.win);
    float2* const X = lds.X;
    const float2* const tw = lds.tw;
    float* const mag = lds.rest;                                               // [F]
    float* const row = mag + F;                                                // [Mel]
    const int total = a.B * a.T;
    for (int f = blockIdx.x; f < total; f += gridDim.x) {
        const int b = f / a.T, t = f - b * a.T;
        const int L = a.lengths[b];
        int Tb = L > 0 ? 1 + L / a.hop : 0;
        if (Tb > a.T) Tb = a.T;
        float* out = a.mel + (int64_t)f * a.Mel;
        if (t >= Tb || L > a.ldx) {                                            // beyond the utterance: the pad value (uniform over the workgroup)
            for (int j = tid; j < a.Mel; j += VOC_NT) out[j] = -a.max_abs;
            continue;
        }
        // ---- the frame, with the pre-emphasis applied to the reflected index ----
        const float* xb = a.x + (int64_t)b * a.ldx;
        voc_pack_frame(lds, M, logM, lpad, a.win, t * a.hop - M, L, [&](int s) { return s > 0 ? xb[s] - a.p * xb[s - 1] : xb[s]; });
        voc_fft<false>(X, tw, logM, a.logN, tid);
        // ---- split: |Y_k| of the real-input spectrum, bin pairs (k, M - k) ----
        for (int k = tid; k <= (M >> 1); k += VOC_NT) {
            if (k == 0) {
                const float2 z = X[0];
                mag[0] = fabsf(z.x + z.y);
                mag[M] = fabsf(z.x - z.y);
                continue;
            }
            float2 yk, ymk;
            voc_split_pair(X, tw, k, M, yk, ymk);
            mag[k] = sqrtf(yk.x * yk.x + yk.y * yk.y);
            mag[M - k] = sqrtf(ymk.x * ymk.x + ymk.y * ymk.y);
        }
        __syncthreads();
        // ---- sparse mel projection + dB + normalisation ----
        for (int j = wave; j < a.Mel; j += VOC_NT / 64) {
            int first = a.fb_index[3 * j], cnt = a.fb_index[3 * j + 1], off = a.fb_index[3 * j + 2];
            if (first < 0 || first > F || off < 0) cnt = 0;                    // a malformed table reads nothing out of bounds
            if (cnt > F - first) cnt = F - first;
            if (cnt > a.nw - off) cnt = a.nw - off;
            float acc = 0.f;
            for (int i = lane; i < cnt; i += 64) acc = fmaf(a.fb_weight[off + i], mag[first + i], acc);
            acc = wave_sum(acc);
            if (lane == 0) {
                const float db = 20.f * log10f(acc + 1e-7f);
                const float v = (2.f * a.max_abs) * (db - a.min_db) / (-a.min_db) - a.max_abs;
                row[j] = fminf(fmaxf(v, -a.max_abs), a.max_abs);
            }
        }
        __syncthreads();
        for (int j = tid; j < a.Mel; j += VOC_NT) out[j] = row[j];
    }
}

struct yin_args {
    const float* x;            // [B][ldx]
    const int32_t* lengths;    // [B] samples
    float* pitch;              // [B][T]
    float* cmnd;               // [B][T][tau_max] or null
    float thresh, sr;
    int B, T, ldx, w_len, w_step, tau_min, tau_max;
};

constexpr int YIN_TG = 4;      // taus a wave accumulates at a time

__global__ __launch_bounds__(256) void yin_kernel(const yin_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fe_smem[];
    float* const x = reinterpret_cast<float*>(fe_smem);                        // [w_len]
    float* const d = x + a.w_len;                                              // [tau_max]: d(tau), then cm(tau)
    float* const cum = d + a.tau_max;                                          // [tau_max]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = a.B * a.T;
    for (int f = blockIdx.x; f < total; f += gridDim.x) {
        const int b = f / a.T, t = f - b * a.T;
        const int L = a.lengths[b];
        int Tb = 0, pad = 0;
        if (L > 0 && L <= a.ldx) {
            pad = (a.w_step + a.w_len - L % a.w_step) / 2;
            const int span = L + 2 * pad - a.w_len;                            // frames start at 0, w_step, ... < span
            Tb = span > 0 ? (span + a.w_step - 1) / a.w_step : 0;
            if (Tb > a.T) Tb = a.T;
        }
        float* cm_out = a.cmnd ? a.cmnd + (int64_t)f * a.tau_max : nullptr;
        if (t >= Tb) {                                                         // (uniform over the workgroup)
            if (tid == 0) a.pitch[f] = 0.f;
            if (cm_out) for (int i = tid; i < a.tau_max; i += 256) cm_out[i] = 0.f;
            continue;
        }
        const float* xb = a.x + (int64_t)b * a.ldx;
        for (int j = tid; j < a.w_len; j += 256) x[j] = xb[voc_reflect(t * a.w_step + j - pad, L)];
        __syncthreads();
        // ---- difference function ----
        for (int t0 = wave * YIN_TG; t0 < a.tau_max; t0 += 4 * YIN_TG) {
            float acc[YIN_TG];
#pragma unroll
            for (int i = 0; i < YIN_TG; ++i) acc[i] = 0.f;
            for (int j = lane; j < a.w_len - t0; j += 64) {
                const float xj = x[j];
#pragma unroll
                for (int i = 0; i < YIN_TG; ++i) {
                    if (j + t0 + i < a.w_len) {
                        const float df = xj - x[j + t0 + i];
                        acc[i] = fmaf(df, df, acc[i]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < YIN_TG; ++i) {
                const float s = wave_sum(acc[i]);
                if (lane == 0 && t0 + i < a.tau_max) d[t0 + i] = s;
            }
        }
        __syncthreads();
        // ---- cumulative-mean normalisation ----
        if (tid == 0) {
            float run = 0.f;
            cum[0] = 0.f;
            for (int tau = 1; tau < a.tau_max; ++tau) { run += d[tau]; cum[tau] = run; }
        }
        __syncthreads();
        for (int tau = tid; tau < a.tau_max; tau += 256) {
            const float cm = tau == 0 ? 1.f : d[tau] * (float)tau / (cum[tau] + 1e-8f);
            d[tau] = cm;
            if (cm_out) cm_out[tau] = cm;
        }
        __syncthreads();
        // ---- the first dip below the threshold, walked to its local minimum ----
        if (tid == 0) {
            float p = 0.f;
            for (int tau = a.tau_min; tau < a.tau_max; ++tau) {
                if (d[tau] < a.thresh) {
                    while (tau + 1 < a.tau_max && d[tau + 1] < d[tau]) ++tau;
                    p = a.sr / (float)tau;
                    break;
                }
            }
            a.pitch[f] = p;
        }
        // the next frame's first write to d follows a barrier that thread 0 reaches only after this decision
    }
}

bool fe_bad_batch(int B, int T, int ldx) { return B < 1 || B > 65535 || T < 1 || ldx < 1 || (int64_t)B * T > (int64_t)1 << 30; }

}  // namespace

extern "C" int glowtts_mel_analysis_f32(const float* wav, const int32_t* wav_lengths, const float* window, const float* twiddle, const int32_t* fb_index,
                                        const float* fb_weight, float* mel, int B, int ldx, int T, int Mel, int n_weights, int n_fft, int win_length, int hop,
                                        float pre_emphasis, float min_db, float max_abs, void* stream)
{
    if (!wav || !wav_lengths || !window || !twiddle || !fb_index || !fb_weight || !mel || fe_bad_batch(B, T, ldx) || Mel < 1 || Mel > 1024 || n_weights < 1 ||
        !voc_fft_supported(n_fft, win_length) || hop < 1 || !(max_abs > 0.f) || !(min_db < 0.f))
        return GLOWTTS_E_ARG;
    mel_args a = {};
    a.x = wav; a.lengths = wav_lengths; a.window = window; a.twiddle = reinterpret_cast<const float2*>(twiddle); a.fb_index = fb_index; a.fb_weight = fb_weight;
    a.mel = mel; a.p = pre_emphasis; a.min_db = min_db; a.max_abs = max_abs;
    a.B = B; a.T = T; a.ldx = ldx; a.Mel = Mel; a.nw = n_weights; a.logN = voc_log2(n_fft); a.win = win_length; a.hop = hop;
    const size_t lds = voc_lds_bytes(n_fft, win_length, n_fft / 2 + 1 + Mel);  // + magnitudes [F] | mel row [Mel]: <= 60.5 KiB at 4096 / 4096 / 1024
    const int frames = B * T, grid = frames < 1536 ? frames : 1536;            // 6 resident workgroups (by LDS at n_fft = 2048) on each of 256 CUs
    GLOWTTS_NOTE_STATIC("frontend_mel_analysis");
    hipLaunchKernelGGL(mel_analysis_kernel, dim3(grid), dim3(VOC_NT), lds, static_cast<hipStream_t>(stream), a);
    RET_LAUNCH();
}

extern "C" int glowtts_yin_f32(const float* wav, const int32_t* wav_lengths, float* pitch, float* cmnd, int B, int ldx, int T, int w_len, int w_step, int tau_min,
                               int tau_max, float thresh, float sample_rate, void* stream)
{
    if (!wav || !wav_lengths || !pitch || fe_bad_batch(B, T, ldx) || w_len < 2 || w_len > 2048 || w_step < 1 || tau_min < 1 || tau_min >= tau_max || tau_max > w_len ||
        !(sample_rate > 0.f))
        return GLOWTTS_E_ARG;
    yin_args a = {};
    a.x = wav; a.lengths = wav_lengths; a.pitch = pitch; a.cmnd = cmnd; a.thresh = thresh; a.sr = sample_rate;
    a.B = B; a.T = T; a.ldx = ldx; a.w_len = w_len; a.w_step = w_step; a.tau_min = tau_min; a.tau_max = tau_max;
    const int frames = B * T, grid = frames < 2048 ? frames : 2048;            // 8 workgroups of 4 waves on each of 256 CUs; more frames: strided
    GLOWTTS_NOTE_STATIC("frontend_yin");
    hipLaunchKernelGGL(yin_kernel, dim3(grid), dim3(256), (size_t)(w_len + 2 * tau_max) * 4, static_cast<hipStream_t>(stream), a);
    RET_LAUNCH();
}
