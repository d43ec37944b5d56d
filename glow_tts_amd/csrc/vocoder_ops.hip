// Griffin-Lim vocoder (waveform output of Inference.py; the reference stops at the mel): mel -> linear magnitudes, the STFT / inverse STFT that
// glow_tts_amd/audio.py's front end defines (center = True, reflect padding by n_fft / 2, periodic Hann of win_length centred in n_fft), and one FUSED
// Griffin-Lim iteration per launch.
//
// Data flow of an iteration (vocoder_frame_kernel<MODE_STEP>, one 256-thread workgroup per frame at a time, workgroups stride over the frames of the batch):
//   HBM -> LDS   y = x_n + alpha (x_n - x_{n-1}) gathered for the win_length samples the window covers (reflect at the ends), windowed, packed as
//                z[m] = y[2m] + i y[2m+1] and written at the bit-reversed index
//   LDS          complex FFT of n_fft / 2 points (decimation in time, radix 4 with one radix-2 stage when log2 is odd), in place
//   LDS          per bin pair (k, n_fft/2 - k): the real-input split Y = E + W^k O, the projection Y / max(|Y|, 1e-8) times the target magnitude (the only other HBM
//                read: n_fft/2 + 1 floats), and the inverse split back to a packed spectrum - all in registers, in place
//   LDS          inverse complex FFT (decimation in frequency: natural order in, bit-reversed out), in place
//   LDS -> HBM   the win_length samples under the window, windowed again: the frame's overlap-add contribution
// The complex spectrum never leaves LDS.  vocoder_ola_kernel then GATHERS every output sample from its win_length / hop contributing frames in ascending frame
// order and divides by the summed squared window (floored at 1e-8): no floating-point atomics, bit-identical from run to run.
// Twiddles exp(-2 pi i k / n_fft), k < n_fft / 2, and the window come from tables the host computes in float64 and rounds to fp32; no device sincos.
// LDS per workgroup at n_fft = 2048, win 1024: 8 KiB twiddles + 4 KiB window + 8.3 KiB spectrum = 20.3 KiB -> 7 workgroups per CU (160 KiB).
// Bank conflicts: element i of the spectrum lives at i + (i >> 5) (8-byte units), which shifts every 32-element row by one slot.  Counted with the
// ds_read_b64 rule (32-lane groups, 8-byte slot modulo 32) at n_fft = 2048: the bit-reversed accesses (lane stride n_fft / 64 elements) go from 32-way
// (scatter) and 16-way (final gather) to conflict-free and the h = 1 pass from 4-way to conflict-free; the h = 4 pass stays 4-way and the h = 16 pass
// 2-way (their four-element runs still overlap after the shift), h >= 64 is conflict-free either way, and the split's ascending read becomes 2-way.
// The stores are counted by the same rule although ds_write maps modulo 32 dwords: their true cost is not argued here.  The pad removes the worst conflicts, not all of them.
// Lengths: an utterance whose length exceeds what the signal buffer holds (wav_lengths[b] > ldx, or hop (frame_lengths[b] - 1) > ldx) is a caller error that
// the host cannot see without a synchronisation; the kernels never read beyond ldx, so such an utterance comes out as zeros (STFT) or is left unwritten
// (inverse STFT, step).  vocoder.GriffinLim derives lengths and buffers from the same shapes, so the product path cannot reach this.
// The LDS layout, the frame packer, the split and its inverse, the frame unpack and the FFT itself are vocoder_fft.h's, shared with frontend_ops.hip and
// stft_loss_ops.hip; this file keeps the projection, the MODE template, the overlap-add and the mel inversion.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/glowtts_hip.h"
#include "launch_log.h"
#include "vocoder_fft.h"

namespace {

enum { MODE_STFT = 0, MODE_ISTFT = 1, MODE_STEP = 2 };

struct voc_args {
    const float* x;            // STFT / STEP: signal [B][ldx]
    const float* xp;           // STEP: previous signal
    const float* spec;         // ISTFT: complex spectrum [B][T][F][2]
    const float* mag;          // STEP: target magnitudes [B][T][F]
    const int32_t* lengths;    // STFT: samples per utterance; ISTFT / STEP: frames per utterance
    const float* window;       // [win]
    const float2* twiddle;     // [n_fft / 2]
    float* spec_out;           // STFT: [B][T][F][2]
    float* frames;             // ISTFT / STEP: [B][T][win]
    float alpha;
    int B, T, ldx, logN, win, hop;
};

// Y -> target magnitude times the phase of Y (|Y| floored at 1e-8)
__device__ __forceinline__ float2 voc_project(float2 y, float s) {
    const float a = fmaxf(sqrtf(y.x * y.x + y.y * y.y), 1e-8f);
    return make_float2(s * (y.x / a), s * (y.y / a));
}

template <int MODE>
__global__ __launch_bounds__(VOC_NT) void vocoder_frame_kernel(const voc_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char voc_smem[];
    const int N = 1 << a.logN, M = N >> 1, logM = a.logN - 1, F = M + 1;
    const int tid = threadIdx.x;
    const int lpad = (N - a.win) >> 1;
    const voc_lds lds = voc_lds_stage(voc_smem, a.twiddle, a.window, M, a.win);
    float2* const X = lds.X;
    const float2* const tw = lds.tw;
    const int total = a.B * a.T;
    for (int f = blockIdx.x; f < total; f += gridDim.x) {
        const int b = f / a.T, t = f - b * a.T;
        int L, Tb;                                                             // samples and frames of this utterance
        if (MODE == MODE_STFT) { L = a.lengths[b]; Tb = L > 0 ? 1 + L / a.hop : 0; }
        else { Tb = a.lengths[b]; L = a.hop * (Tb - 1); }
        if (Tb > a.T) Tb = a.T;
        if (MODE == MODE_STFT && (t >= Tb || L > a.ldx)) {                     // a frame beyond the utterance: zeros
            float2* out = reinterpret_cast<float2*>(a.spec_out) + (int64_t)f * F;
            for (int k = tid; k < F; k += VOC_NT) out[k] = make_float2(0.f, 0.f);
            continue;
        }
        if (MODE != MODE_STFT && (t >= Tb || L < 1 || L > a.ldx)) continue;   // (uniform over the workgroup)
        if (MODE != MODE_ISTFT) {
            const float* xb = a.x + (int64_t)b * a.ldx;
            const float* xpb = MODE == MODE_STEP ? a.xp + (int64_t)b * a.ldx : nullptr;
            voc_pack_frame(lds, M, logM, lpad, a.win, t * a.hop - M, L, [&](int s) {
                const float y = xb[s];
                return MODE == MODE_STEP ? y + a.alpha * (y - xpb[s]) : y;
            });
            voc_fft<false>(X, tw, logM, a.logN, tid);
        }
        // ---- split (real-input spectrum from the packed one), projection, inverse split: bin pairs (k, M - k) ----
        {
            const float* sp = MODE == MODE_ISTFT ? a.spec + (int64_t)f * F * 2 : nullptr;
            const float* mg = MODE == MODE_STEP ? a.mag + (int64_t)f * F : nullptr;
            float2* out = MODE == MODE_STFT ? reinterpret_cast<float2*>(a.spec_out) + (int64_t)f * F : nullptr;
            for (int k = tid; k <= (M >> 1); k += VOC_NT) {
                if (k == 0) {
                    float y0, ym;                                             // bins 0 and M are real
                    if (MODE == MODE_ISTFT) { y0 = sp[0]; ym = sp[2 * M]; }
                    else {
                        const float2 z = X[0];
                        y0 = z.x + z.y;
                        ym = z.x - z.y;
                    }
                    if (MODE == MODE_STFT) { out[0] = make_float2(y0, 0.f); out[M] = make_float2(ym, 0.f); continue; }
                    if (MODE == MODE_STEP) { y0 = voc_project(make_float2(y0, 0.f), mg[0]).x; ym = voc_project(make_float2(ym, 0.f), mg[M]).x; }
                    X[0] = make_float2(0.5f * (y0 + ym), 0.5f * (y0 - ym));
                    continue;
                }
                float2 yk, ymk;
                if (MODE == MODE_ISTFT) {
                    yk = make_float2(sp[2 * k], sp[2 * k + 1]);
                    ymk = make_float2(sp[2 * (M - k)], sp[2 * (M - k) + 1]);
                } else {
                    voc_split_pair(X, tw, k, M, yk, ymk);
                }
                if (MODE == MODE_STFT) { out[k] = yk; out[M - k] = ymk; continue; }
                if (MODE == MODE_STEP) { yk = voc_project(yk, mg[k]); ymk = voc_project(ymk, mg[M - k]); }
                voc_unsplit_pair(X, tw, k, M, yk, ymk);
            }
            __syncthreads();
        }
        if (MODE != MODE_STFT) {
            voc_fft<true>(X, tw, logM, a.logN, tid);
            // ---- the samples under the window, windowed again: this frame's overlap-add contribution ----
            float* fr = a.frames + (int64_t)f * a.win;
            const float scale = 1.f / (float)M;
            voc_unpack_frame(X, logM, lpad, a.win, [&](int j, float y) { fr[j] = y * scale * lds.wnd[j]; });
        }
    }
}

// Overlap-add as a gather: sample s of utterance b sums frames t_lo .. t_hi (ascending) at window position j = s + n_fft / 2 - lpad - t hop, and is divided by the
// summed squared window, floored at 1e-8.  Samples at or beyond hop (T_b - 1) are written as zeros.
__global__ __launch_bounds__(256) void vocoder_ola_kernel(const float* __restrict__ frames, const int32_t* __restrict__ lengths, const float* __restrict__ window,
                                                          float* __restrict__ wav, int T, int ldx, int n_fft, int win, int hop)
{
    const int b = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ldx) return;
    int Tb = lengths[b];
    if (Tb > T) Tb = T;
    const int L = hop * (Tb - 1);
    float r = 0.f;
    if (s < L) {
        const int p = s + (n_fft >> 1) - ((n_fft - win) >> 1);   // position relative to the window start of frame 0
        int t_hi = p / hop, t_lo = p >= win ? (p - win) / hop + 1 : 0;
        if (t_hi > Tb - 1) t_hi = Tb - 1;
        float acc = 0.f, wss = 0.f;
        const float* fb = frames + (int64_t)b * T * win;
        for (int t = t_lo; t <= t_hi; ++t) {
            const int j = p - t * hop;
            const float w = window[j];
            acc += fb[(int64_t)t * win + j];
            wss += w * w;
        }
        r = acc / fmaxf(wss, 1e-8f);
    }
    wav[(int64_t)b * ldx + s] = r;
}

// mels [B][Mel][T] (normalised to +- max_abs) -> linear magnitudes [B][T][F]: a workgroup takes MTL_TF frames; the de-normalised mel amplitudes go to LDS
// (float64 arithmetic for the exponential, rounded once), every thread then owns output bins f, f + 256, ...
constexpr int MTL_TF = 8;
__global__ __launch_bounds__(256) void vocoder_mel_to_linear_kernel(const float* __restrict__ mels, const int32_t* __restrict__ lengths, const float* __restrict__ basis,
                                                                    float* __restrict__ mag, int Mel, int T, int F, float max_abs)
{
    extern __shared__ float mtl_amp[];                         // [MTL_TF][Mel]
    const int b = blockIdx.y, t0 = blockIdx.x * MTL_TF;
    int Tb = lengths[b];
    if (Tb > T) Tb = T;
    for (int i = threadIdx.x; i < MTL_TF * Mel; i += 256) {
        const int k = i / MTL_TF, tt = i - k * MTL_TF, t = t0 + tt;
        float v = 0.f;
        if (t < Tb) {
            const double m = fmin(fmax((double)mels[((int64_t)b * Mel + k) * T + t], -(double)max_abs), (double)max_abs);
            const double db = (m + (double)max_abs) / (2.0 * (double)max_abs) * 100.0 - 100.0;
            v = (float)fmax(exp10(db / 20.0) - 1e-7, 0.0);
        }
        mtl_amp[tt * Mel + k] = v;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < F; f += 256) {
        float acc[MTL_TF];
#pragma unroll
        for (int tt = 0; tt < MTL_TF; ++tt) acc[tt] = 0.f;
        const float* row = basis + (int64_t)f * Mel;
        for (int k = 0; k < Mel; ++k) {
            const float p = row[k];
#pragma unroll
            for (int tt = 0; tt < MTL_TF; ++tt) acc[tt] = fmaf(p, mtl_amp[tt * Mel + k], acc[tt]);
        }
#pragma unroll
        for (int tt = 0; tt < MTL_TF; ++tt) {
            const int t = t0 + tt;
            if (t < T) mag[((int64_t)b * T + t) * F + f] = t < Tb ? fmaxf(acc[tt], 1e-10f) : 0.f;
        }
    }
}

int voc_grid(int frames) { return frames < 1792 ? frames : 1792; }             // 7 resident workgroups (by LDS at n_fft = 2048) on each of 256 CUs: one wave; more frames: strided

template <int MODE>
int voc_launch(const voc_args& a, int n_fft, void* stream)
{
    hipLaunchKernelGGL(vocoder_frame_kernel<MODE>, dim3(voc_grid(a.B * a.T)), dim3(VOC_NT), voc_lds_bytes(n_fft, a.win, 0), static_cast<hipStream_t>(stream), a);
    RET_LAUNCH();
}
int voc_ola(const float* frames, const int32_t* lengths, const float* window, float* wav, int B, int T, int ldx, int n_fft, int win, int hop, void* stream)
{
    hipLaunchKernelGGL(vocoder_ola_kernel, dim3((ldx + 255) / 256, B), dim3(256), 0, static_cast<hipStream_t>(stream), frames, lengths, window, wav, T, ldx, n_fft, win, hop);
    RET_LAUNCH();
}
bool voc_bad_dims(int B, int T, int ldx, int n_fft, int win, int hop)
{
    return B < 1 || B > 65535 || T < 1 || ldx < 1 || !glowtts_vocoder_supported(n_fft, win, hop) || (int64_t)B * T > (int64_t)1 << 30;
}

}  // namespace

extern "C" int glowtts_vocoder_supported(int n_fft, int win_length, int hop)
{
    return voc_fft_supported(n_fft, win_length) && hop >= 1 && win_length % hop == 0;
}

extern "C" int glowtts_mel_to_linear_f32(const float* mels, const int32_t* frame_lengths, const float* basis, float* mag, int B, int Mel, int T, int F, float max_abs,
                                         void* stream)
{
    if (!mels || !frame_lengths || !basis || !mag || B < 1 || B > 65535 || Mel < 1 || Mel > 1024 || T < 1 || F < 1 || !(max_abs > 0.f)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("vocoder_mel_to_linear");
    hipLaunchKernelGGL(vocoder_mel_to_linear_kernel, dim3((T + MTL_TF - 1) / MTL_TF, B), dim3(256), (size_t)MTL_TF * Mel * 4, static_cast<hipStream_t>(stream), mels,
                       frame_lengths, basis, mag, Mel, T, F, max_abs);
    RET_LAUNCH();
}

extern "C" int glowtts_stft_f32(const float* wav, const int32_t* wav_lengths, const float* window, const float* twiddle, float* spec, int B, int ldx, int T, int n_fft,
                                int win_length, int hop, void* stream)
{
    if (!wav || !wav_lengths || !window || !twiddle || !spec || voc_bad_dims(B, T, ldx, n_fft, win_length, hop)) return GLOWTTS_E_ARG;
    voc_args a = {};
    a.x = wav; a.lengths = wav_lengths; a.window = window; a.twiddle = reinterpret_cast<const float2*>(twiddle); a.spec_out = spec;
    a.B = B; a.T = T; a.ldx = ldx; a.logN = voc_log2(n_fft); a.win = win_length; a.hop = hop;
    GLOWTTS_NOTE_STATIC("vocoder_stft");
    return voc_launch<MODE_STFT>(a, n_fft, stream);
}

extern "C" int glowtts_istft_f32(const float* spec, const int32_t* frame_lengths, const float* window, const float* twiddle, float* frames, float* wav, int B, int T,
                                 int ldx, int n_fft, int win_length, int hop, void* stream)
{
    if (!spec || !frame_lengths || !window || !twiddle || !frames || !wav || voc_bad_dims(B, T, ldx, n_fft, win_length, hop) || ldx < hop * (T - 1)) return GLOWTTS_E_ARG;
    voc_args a = {};
    a.spec = spec; a.lengths = frame_lengths; a.window = window; a.twiddle = reinterpret_cast<const float2*>(twiddle); a.frames = frames;
    a.B = B; a.T = T; a.ldx = ldx; a.logN = voc_log2(n_fft); a.win = win_length; a.hop = hop;
    GLOWTTS_NOTE_STATIC("vocoder_istft");
    const int rc = voc_launch<MODE_ISTFT>(a, n_fft, stream);
    return rc != GLOWTTS_OK ? rc : voc_ola(frames, frame_lengths, window, wav, B, T, ldx, n_fft, win_length, hop, stream);
}

extern "C" int glowtts_griffin_lim_step_f32(const float* x, const float* x_prev, const float* mag, const int32_t* frame_lengths, const float* window,
                                            const float* twiddle, float alpha, float* frames, int B, int T, int ldx, int n_fft, int win_length, int hop, void* stream)
{
    if (!x || !x_prev || !mag || !frame_lengths || !window || !twiddle || !frames || voc_bad_dims(B, T, ldx, n_fft, win_length, hop) || ldx < hop * (T - 1))
        return GLOWTTS_E_ARG;
    voc_args a = {};
    a.x = x; a.xp = x_prev; a.mag = mag; a.lengths = frame_lengths; a.window = window; a.twiddle = reinterpret_cast<const float2*>(twiddle); a.frames = frames;
    a.alpha = alpha; a.B = B; a.T = T; a.ldx = ldx; a.logN = voc_log2(n_fft); a.win = win_length; a.hop = hop;
    GLOWTTS_NOTE_STATIC("vocoder_griffin_lim_step");
    return voc_launch<MODE_STEP>(a, n_fft, stream);
}

extern "C" int glowtts_overlap_add_f32(const float* frames, const int32_t* frame_lengths, const float* window, float* wav, int B, int T, int ldx, int n_fft,
                                       int win_length, int hop, void* stream)
{
    if (!frames || !frame_lengths || !window || !wav || voc_bad_dims(B, T, ldx, n_fft, win_length, hop)) return GLOWTTS_E_ARG;
    GLOWTTS_NOTE_STATIC("vocoder_overlap_add");
    return voc_ola(frames, frame_lengths, window, wav, B, T, ldx, n_fft, win_length, hop, stream);
}
