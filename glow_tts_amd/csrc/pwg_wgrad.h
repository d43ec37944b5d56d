// The weight gradients of Parallel WaveGAN training, shared by the generator's backward (pwg_train_ops.hip) and the discriminator's (pwg_disc_ops.hip): every
// weight gradient is a product A^T B over the rows.  A job names A (with a row shift for the dilated taps, or the noise hash for first_conv, and an optional
// constant-one column that yields the bias), B and where the result goes in torch's layout.  `pwg_wgrad`: one wave owns a 16 x 16 output tile of one job
// over one split of the rows; the split partition is fixed: per utterance, chunks of 1024 rows.  `pwg_wgrad_sum` adds the splits in ascending order, scales,
// writes torch's layout (overwrites).  No float atomics, fixed partition and order: bit-identical from run to run.
#pragma once
#include "gauss_hash.h"
#include "launch_log.h"
#include "pwg_common.h"

namespace {

constexpr int WG_ROWS = 1024;                             // rows of one split of the weight-gradient partition
constexpr int WG_MAX_JOBS = 8;

// ---- weight gradients: out[i][n] = scale sum_rows A[row + shift][i] B[row][n], rows of every utterance's own [0, T_b) ----
struct wg_job {
    const float* a;            // [B][Tmax][lda], or NULL: the noise z (seeds given: the counter hash, else `noise` [B][Tmax])
    const float* b;            // [B][Tmax][ldb]
    float* dst;                // out[i][n] -> dst[i * dst_i + n * dst_n]
    float* dbias;              // ones: out[ka][n] -> dbias[n]
    int lda, ka, shift, ldb, n, dst_i, dst_n, ones, tiles_i, tiles_n, tile0, off;
    float scale;
};
struct wg_args {
    wg_job job[WG_MAX_JOBS];
    const int32_t* lengths;
    const uint32_t* seeds;
    const float* noise;
    float* partial;            // [splits][total_elems]
    int njobs, total_tiles, total_elems, Lmax, hop, nchunk;
};

// grid (total_tiles, B * nchunk), one wave: a 16 x 16 output tile of one job over rows [chunk * 1024, (chunk + 1) * 1024) of utterance b
__global__ __launch_bounds__(64) void pwg_wgrad_kernel(const wg_args a)
{
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    int j = 0;
    while (j + 1 < a.njobs && (int)blockIdx.x >= a.job[j + 1].tile0) ++j;
    const wg_job& J = a.job[j];
    const int tile = blockIdx.x - J.tile0, ti = tile / J.tiles_n, tn = tile - ti * J.tiles_n;
    const int b = blockIdx.y / a.nchunk, chunk = blockIdx.y - b * a.nchunk;
    const int Tmax = a.Lmax * a.hop, T = min(a.lengths[b], a.Lmax) * a.hop;
    const int i = ti * 16 + r, n = tn * 16 + r;
    const size_t row0 = (size_t)b * Tmax;
    const int t_end = min((chunk + 1) * WG_ROWS, T);
    const bool a_ok = i < J.ka, a_one = J.ones && i == J.ka, n_ok = n < J.n;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = chunk * WG_ROWS + q; t < t_end + 3; t += 4) {      // (t - q < t_end for every lane of the wave: the MFMA is issued by all 64)
        if (t - q >= t_end) break;
        float av = 0.f, bv = 0.f;
        if (t < t_end) {
            if (a_ok) {
                const int ts = t + J.shift;
                if (ts >= 0 && ts < T) {
                    if (J.a) av = J.a[(row0 + ts) * J.lda + i];
                    else av = a.noise ? a.noise[row0 + ts] : gauss_hash::gauss(a.seeds[2 * b], a.seeds[2 * b + 1], 0u, (uint32_t)ts, 1u);
                }
            } else if (a_one) av = 1.f;
            if (n_ok) bv = J.b[(row0 + t) * J.ldb + n];
        }
        acc = mfma4(av, bv, acc);
    }
    float* out = a.partial + (size_t)blockIdx.y * a.total_elems + J.off;
    const int npad = J.tiles_n * 16;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[(ti * 16 + q * 4 + k) * npad + tn * 16 + r] = acc[k];
}

__global__ __launch_bounds__(THREADS) void pwg_wgrad_sum_kernel(const wg_args a, int splits)
{
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= a.total_elems) return;
    int j = 0;
    while (j + 1 < a.njobs && e >= a.job[j + 1].off) ++j;
    const wg_job& J = a.job[j];
    const int npad = J.tiles_n * 16, local = e - J.off, i = local / npad, n = local - i * npad;
    if (n >= J.n || i > J.ka || (i == J.ka && !J.ones)) return;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += a.partial[(size_t)k * a.total_elems + e];
    s *= J.scale;
    if (i < J.ka) J.dst[(size_t)i * J.dst_i + (size_t)n * J.dst_n] = s;
    else J.dbias[n] = s;
}

// ---- host side ----
// the forward's limits, and the weight gradient's splits fit one grid dimension
bool bad_train_batch(int B, int Lmax, int hop) { return bad_batch(B, Lmax, hop) || (int64_t)B * ((Lmax * (int64_t)hop + WG_ROWS - 1) / WG_ROWS) > 65535; }

int tiles16(int n) { return (n + 15) / 16; }

// appends a job and lays out its tiles and partial sums
void add_job(wg_args& a, const float* A_, int lda, int ka, int shift, const float* B_, int ldb, int n, float* dst, int dst_i, int dst_n, float* dbias, float scale)
{
    wg_job& J = a.job[a.njobs++];
    J.a = A_; J.b = B_; J.dst = dst; J.dbias = dbias; J.lda = lda; J.ka = ka; J.shift = shift; J.ldb = ldb; J.n = n; J.dst_i = dst_i; J.dst_n = dst_n;
    J.ones = dbias != nullptr; J.tiles_i = tiles16(ka + (J.ones ? 1 : 0)); J.tiles_n = tiles16(n); J.tile0 = a.total_tiles; J.off = a.total_elems; J.scale = scale;
    a.total_tiles += J.tiles_i * J.tiles_n;
    a.total_elems += J.tiles_i * J.tiles_n * 256;
}

// `name`, `sum_name`: the launch log's names of the two launches
int wgrad_launch(wg_args& a, const int32_t* lengths, float* work, int B, int Lmax, int hop, const char* name, const char* sum_name, void* stream)
{
    a.lengths = lengths; a.partial = work; a.Lmax = Lmax; a.hop = hop;
    a.nchunk = (int)(((int64_t)Lmax * hop + WG_ROWS - 1) / WG_ROWS);
    const int splits = B * a.nchunk;
    hipStream_t s = static_cast<hipStream_t>(stream);
    glowtts_note_launch(name);
    hipLaunchKernelGGL(pwg_wgrad_kernel, dim3(a.total_tiles, splits), dim3(64), 0, s, a);
    hipLaunchKernelGGL(pwg_wgrad_sum_kernel, dim3((a.total_elems + THREADS - 1) / THREADS), dim3(THREADS), 0, s, a, splits);
    glowtts_note_launch(sum_name);
    RET_LAUNCH();
}

}  // namespace
