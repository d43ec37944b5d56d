/* glowtts_hip.h - C ABI of libglowtts_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary of the MI355X-native Glow-TTS hot path.  Plain pointers and sizes only:
 * every pointer is a DEVICE pointer unless stated otherwise, `stream` is a hipStream_t passed as
 * void* (NULL = default stream), every function is asynchronous on `stream` and returns 0 on
 * success or a negative GLOWTTS_E_* code (no exceptions cross the boundary).
 *
 * The reference (CODEJIN/Glow_TTS) has no FFI layer; each entry point cites the reference
 * interface it replaces (file:line relative to the reference repository).  INTEGRATION.md shows
 * the binding a reference maintainer would add.
 */
#ifndef GLOWTTS_HIP_H
#define GLOWTTS_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOWTTS_OK            0
#define GLOWTTS_E_ARG        -1   /* bad argument / unsupported size */
#define GLOWTTS_E_LAUNCH     -2   /* hip launch error */
#define GLOWTTS_ABI_VERSION    7

/* Library / device identification.  Returns the ABI version (currently 7: glowtts_prior_loss, glowtts_dur_proj_*, glowtts_prior_split_*, the `path` argument of
 * glowtts_expand_pair_targets, the `da_unit` argument of glowtts_mse_loss_fwd, glowtts_gate_bwd_io with out == NULL, glowtts_fx_to_float and glowtts_flow_grads.dcond typed int64_t *; 6: glowtts_cond_linear_supported, the direct 3x3 stride-2 conv trio glowtts_conv3x3s2_*; 5: additions only - glowtts_cond_linear_fwd / _bwd, glowtts_prep_launch_dev,
 * glowtts_rpr_attention_bwd_partial_rows (and NULL drelk / drelv), glowtts_sum_slices / _seg, GLOWTTS_F_GATE_IN0, GLOWTTS_F_COND_FX, glowtts_flow_acts.skip may be NULL on
 * the fused forward launch, glowtts_flow_grads.dcond holds 64-bit fixed-point accumulators; 4: glowtts_flow_acts grew next_* / actnorm_done - the next flow's ActNorm + 1x1 conv in the
 * fused coupling launch's epilogue - and glowtts_proj_layernorm / glowtts_layernorm_qkv were added; 3: glowtts_prep_job / glowtts_prep_launch / glowtts_wavenet_prep_jobs,
 * glowtts_actnorm_inv1x1_pass_bf, glowtts_flow_acts.xa_bf, glowtts_flow_grads.dh0_bf16, GLOWTTS_WIO_DMA; 2: glowtts_flow_params grew wn_img / wn_img_t; round 2's additions to
 * glowtts_mle_loss_bwd, glowtts_flow_params.cond_rows and glowtts_flow_grads.pitch_rows belong to version 2 as well). */
int glowtts_abi_version(void);
/* Writes the gfx arch string of device 0 into buf (host pointer).  0 on success. */
int glowtts_device_arch(char *buf, int buflen);

/* Launch log (diagnostics; no reference counterpart).  The library counts, on the host, the launches it issues per kernel class
 * ("conv_dma<GATE,5>", "conv_chain<LINEAR,DGATE>", "conv_cl<LINEAR,1,f32>", "wgrad<5,bf16,dybf16,xbf16,wide>/grouped", ...), so a
 * parity test can assert which kernel served a call.  glowtts_launch_count sums every class whose name starts with `kernel_class`
 * (host string); _dump writes "name count" lines into buf (host pointer). */
int64_t glowtts_launch_count(const char *kernel_class);
void glowtts_launch_log_reset(void);
int glowtts_launch_log_dump(char *buf, int buflen);

/* Sustained matrix clock (measurement aid for bench.py's roofline; no reference counterpart).  Launches `nwg` workgroups of four waves
 * (one per SIMD), each issuing 4 * iters back-to-back v_mfma_f32_32x32x16_bf16 on pseudo-random operands; workgroup i writes the shader
 * cycles (s_memtime) and the constant-rate wall ticks its loop took to out[2i], out[2i+1] (device pointer, 2 * nwg int64).  *wall_khz
 * (host pointer, optional) receives the wall counter's rate.  cycles / ticks * rate = the clock the chip holds under a dense bf16 MFMA
 * load, which on MI355X is well below the 2.4 GHz the 2.5 PFLOP/s datasheet peak assumes. */
int glowtts_mfma_clock_probe(long long *out, int nwg, int iters, int *wall_khz, void *stream);
/* Diagnostics: a one-thread kernel that writes the constant-rate wall counter (the rate glowtts_mfma_clock_probe reports) to *slot when the
 * stream reaches it - a timeline of a replayed hipGraph from inside the graph (tools/step_timeline.py). */
int glowtts_debug_stamp(long long *slot, void *stream);
/* The dropout seed word of a training step (ABI 6; Modules.py:481, 561-569, 862: torch's Dropout draws from the global generator).  state (device, 2 words:
 * counter, base - the base drawn once from torch's generator) -> counter += 1, out[0] = a 31-bit hash of (base, counter): every dropout kernel of the step adds its own
 * layer constant to this word (the `seed_ptr` arguments).  A launch of its own instead of torch.randint: inside a replayed hipGraph the philox draw costs two fills of
 * the generator's offset words in front of EVERY replay and an RNG launch on each of the two streams' chains. */
int glowtts_step_seed(uint32_t *state, uint32_t *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Monotonic Alignment Search.
 * Replaces monotonic_align/core.pyx:40 `maximum_path_c(paths, values, t_xs, t_ys, max_neg_val)`
 * (and the pure-Python twin Modules.py:951-980).  Bit-exact with core.pyx:9-35 on identical fp32 input.
 *
 *   value    [B][Tx][Ty] f32, already multiplied by the mask (monotonic_align/__init__.py:11).
 *            Read-only unless q_out == value (then clobbered into cumulative scores like core.pyx:30).
 *   t_xs,t_ys[B] i32      valid tokens / frames per utterance, 1 <= t_x <= Tx, 0 <= t_y <= Ty (else: all-zero path, idx = -1).
 *            t_x > t_y (no monotonic alignment exists) is reproduced as core.pyx behaves: nothing is accumulated and the
 *            backtrack walks the raw inputs from row t_x - 1.
 *   idx_out  [B][Ty] i32  token index aligned to each frame, -1 for y >= t_y.           (may be NULL)
 *   q_out    [B][Tx][Ty] f32 cumulative scores exactly as core.pyx leaves `values`      (may be NULL)
 *   Tx <= 512.
 */
int glowtts_mas_dp_f32(const float *value, const int32_t *t_xs, const int32_t *t_ys,
                       int32_t *idx_out, float *q_out, int B, int Tx, int Ty,
                       float max_neg_val, void *stream);
/* Same search on the transposed score matrix value_t [B][Ty][Tx] (token index contiguous) - the layout the
 * fused log-prior GEMM writes, where one frame of scores is one coalesced row.  q_out_t likewise transposed.
 * 64 < Tx <= 128 with Tx even and value_t 16-byte aligned (the training shapes) takes the hand-scheduled kernel of
 * csrc/mas_dp2.hip; every other shape the general one of csrc/mas.hip.  Same results bit for bit. */
int glowtts_mas_dp_f32_t(const float *value_t, const int32_t *t_xs, const int32_t *t_ys,
                         int32_t *idx_out, float *q_out_t, int B, int Tx, int Ty,
                         float max_neg_val, void *stream);
/* Dense 0/1 path from idx (core.pyx:32-35 writes these ones into a pre-zeroed array; here every
 * element is written, so `path` need not be zeroed).  out_dtype: 0 = int32, 1 = float32. */
int glowtts_mas_path_from_idx(const int32_t *idx, void *path, int B, int Tx, int Ty,
                              int out_dtype, void *stream);
/* Both steps: the direct replacement of maximum_path_c.  `scratch_idx` [B][Ty] i32. */
int glowtts_mas_f32(const float *value, int32_t *path, const int32_t *t_xs, const int32_t *t_ys,
                    int32_t *scratch_idx, int B, int Tx, int Ty, float max_neg_val, void *stream);
/* HOST twin (no stream, every pointer is a HOST pointer): exactly `maximum_path_c` of core.pyx:40 - `value` [B][Tx][Ty] is clobbered into
 * the cumulative scores, `path` must arrive zeroed; an utterance with t_x > t_y (no monotonic alignment exists) is treated as core.pyx
 * treats it: nothing is accumulated into `value`, the backtrack walks the RAW scores from row t_x - 1 and writes its ones into `path` (same
 * as the device entry points above).  num_threads <= 0: one thread per
 * hardware thread (core.pyx:44 `prange`).  An explicit entry point for host-resident score matrices, never a fallback of the GPU path. */
int glowtts_mas_f32_host(float *value, int32_t *path, const int32_t *t_xs, const int32_t *t_ys,
                         int B, int Tx, int Ty, float max_neg_val, int num_threads);


/* ------------------------------------------------------------------------------------------
 * Channels-last implicit-GEMM convolution on MFMA (the dense contractions of the path):
 *     Y[r][n] = epilogue( sum_{t<taps} sum_{c<ca} A[r + t - pad][c] * W[n][c][t] )
 * Replaces every torch.nn.Conv1d / conv2d / bmm call site on the hot path
 * (Modules.py:791 Start, :861 In_i k=5, :871 Res_Skip_i, :793 End, and their autograd
 * transposes; encoder convs Modules.py:484,565,568 and RPR_MHA.py:82-84,93).
 *
 * Layout: activations are fp32 "rows x channels" (channels contiguous).  A row is one (utterance,
 * frame); utterances are laid out back to back with >= pad zero rows between them so that the taps
 * of one utterance never read another's frames (rows < 0 or >= rows read as zero).
 * precision: GLOWTTS_F32 uses v_mfma_f32_32x32x2_f32 (exact fp32, the reference's arithmetic),
 *            GLOWTTS_BF16 rounds operands to bf16 (v_mfma_f32_32x32x16_bf16), fp32 accumulate.
 */
#define GLOWTTS_F32   0
#define GLOWTTS_BF16  1

/* weight permutations applied by glowtts_pack_weight to the packed N (or K, when transposed) index */
#define GLOWTTS_PERM_NONE 0
#define GLOWTTS_PERM_PAIR 1   /* packed p*64 + h*32 + j  <->  original h*H + (p*32 + j): halves interleaved per 32 */

/* Packs W_eff fp32 [O][I][taps] (torch Conv1d weight layout) into MFMA tile order
 * [tap][kchunk][npad][KC] in the requested precision.
 *   transpose = 0: N = O, K = I                       (forward)
 *   transpose = 1: N = I, K = O, taps flipped          (data gradient)
 *   perm/perm_h : permutation of the O index (PAIR for gate / coupling halves), applied to whichever
 *                 of N / K is O.  npad_out / kchunks_out (host pointers, may be NULL) receive the
 *                 padded sizes; `packed` must hold taps*kchunks*npad*64 bytes
 *                 (query with packed == NULL). */
int glowtts_pack_weight(const float *w, int O, int I, int taps, int transpose, int perm, int perm_h,
                        int precision, void *packed, int *npad_out, int *kchunks_out, void *stream);

/* Many weights of different shapes packed by ONE launch (the encoder's convs, forward and transposed: ~70 launches of
 * glowtts_pack_weight per training step otherwise).  Jobs live in device memory; fill them on the host with glowtts_pack_job_init
 * (same arguments as glowtts_pack_weight; block0 = running sum of the previous jobs' *blocks_out), copy the table to the device
 * once - it stays valid while the weight and packed pointers do - and launch with total_blocks = the final running sum. */
typedef struct glowtts_pack_job {
    const float *w; void *packed;
    int O, I, taps, transpose, perm, perm_h;
    int N, K, npad, kchunks;               /* derived (glowtts_pack_job_init) */
    int block0, reserved;
} glowtts_pack_job;
int glowtts_pack_job_init(glowtts_pack_job *job, const float *w, int O, int I, int taps, int transpose, int perm, int perm_h,
                          int precision, void *packed, int block0, int *blocks_out, int64_t *bytes_out);
int glowtts_pack_weight_multi(const glowtts_pack_job *dev_jobs, int njobs, int total_blocks, int precision, void *stream);

/* `batch` independent weights of identical shape, w [batch][O][I][taps] -> packed [batch][taps*kchunks*npad*64 bytes] */
int glowtts_pack_weight_batched(const float *w, int batch, int O, int I, int taps, int transpose, int perm, int perm_h,
                                int precision, void *packed, int *npad_out, int *kchunks_out, void *stream);

/* The same with a two-level destination: weight b (0 <= b < batch) is written at packed + (b / inner) * outer_stride + (b % inner) *
 * inner_stride (bytes, may be negative) - how glowtts_wavenet_pack_images places every conv of a flow inside that flow's weight image.
 * w_stride: elements between consecutive source weights (0 = O * I * taps; larger: each weight is the leading [O] slice of a bigger tensor). */
int glowtts_pack_weight_strided(const float *w, int batch, int inner, int O, int I, int taps, int transpose, int perm, int perm_h,
                                int precision, void *packed, int64_t outer_stride, int64_t inner_stride, int64_t w_stride, void *stream);

/* Weight preparation of a training step in ONE launch (round 4; replaces glowtts_weightnorm_fwd + the glowtts_pack_weight_* launches of the decoder:
 * Modules.py:766, 818, 825 weight_norm + the tile images of every conv).  A job = one glowtts_pack_weight_strided call whose source is the
 * weight-norm pair (v [batch][O][I][taps], g [batch][O]) instead of w: w = g * v / ||v|| (norm over (I, taps) per output channel, old-style
 * torch weight_norm) is formed on the fly in fp32, rounded to bf16 exactly as the two-step path rounds it, and never written.  g == NULL: v is a
 * plain weight.  inv_out (optional) [batch][O] receives 1 / ||v|| for glowtts_weightnorm_bwd.  g_stride: elements between consecutive convs'
 * g / inv_out rows (0 = O; larger when a job covers the leading [O] slice of a bigger conv).  bf16 images only.  I * taps <= 1024 (plain weights: 4096).
 * Jobs are a HOST array (fill with glowtts_prep_job_init, block0 = running sum of *blocks_out; at most GLOWTTS_PREP_MAX_JOBS per launch): the launch
 * carries the table in its argument segment, so a captured step needs no copy node for it. */
#define GLOWTTS_PREP_MAX_JOBS 22
typedef struct glowtts_prep_job {
    const float *v; const float *g; float *inv_out; void *packed;
    int64_t outer_stride, inner_stride, w_stride, g_stride;
    int batch, inner, O, I, taps, transpose, perm, perm_h;
    int o_ext, npad, kchunks, tiles;       /* derived (glowtts_prep_job_init) */
    int block0, reserved;
    /* ABI 7: twin output (glowtts_prep_jobs_twin_in): a forward PAIR-packed job whose tiles ALSO write the transposed half images of the same rows - the pairs
     * are read once for all three images.  twin == NULL: none */
    void *twin; int64_t twin_outer, twin_inner, twin_half;
    int twin_batch, twin_npad;
} glowtts_prep_job;
/* Folds the two transposed In_l half jobs of a table built by glowtts_wavenet_prep_jobs (forward images, then the backward images of the FIRST F_bwd flows)
 * into the forward In_l job as its twin output, removes them and renumbers block0.  No-op (returns GLOWTTS_OK) when the pattern is not found. */
int glowtts_prep_jobs_twin_in(glowtts_prep_job *jobs /* host */, int *njobs, int *blocks);
int glowtts_prep_job_init(glowtts_prep_job *job /* host */, const float *v, const float *g, float *inv_out, int batch, int inner, int O, int I, int taps,
                          int transpose, int perm, int perm_h, void *packed, int64_t outer_stride, int64_t inner_stride, int64_t w_stride,
                          int64_t g_stride, int block0, int *blocks_out /* host */);
/* max_cols = the largest I * taps among the jobs (sizes the LDS tile) */
int glowtts_prep_launch(const glowtts_prep_job *host_jobs, int njobs, int total_blocks, int max_cols, void *stream);
/* Round 5: the same kernel over a job table in DEVICE memory, any number of jobs - for tables that do not change between steps (the text encoder's ~60
 * images of plain conv weights: built and uploaded once).  Measured against glowtts_pack_weight_multi's element-wise gather on those images: 47 vs 33 us
 * alone - the host library keeps the gather and no longer calls this entry point (round 6). */
int glowtts_prep_launch_dev(const glowtts_prep_job *dev_jobs, int njobs, int total_blocks, int max_cols, void *stream);

#define GLOWTTS_APRO_NONE    0
#define GLOWTTS_APRO_PAIRMUL 1  /* a[r][c] = A[r][2c] * A[r][2c+1]   (tanh*sigmoid gates, Modules.py:885-887) */
#define GLOWTTS_APRO_SQNEG   2  /* a[r][c] = c < ca1 ? -0.5 * A[r][c]^2 : A[r][c - ca1]   (log-prior operand, Modules.py:112-113) */

#define GLOWTTS_EPI_LINEAR   0  /* v = acc (+bias[n]) (relu) (+in0[r][n]) (*rowmask[r]) (+= out0) -> out0[r][n]      */
#define GLOWTTS_EPI_GATE     1  /* PAIR-packed cols: out0[r][2j],[2j+1] = tanh(a), sigmoid(s)   Modules.py:861-870   */
#define GLOWTTS_EPI_RESSKIP  2  /* n<h: out0 = (in0+acc+b)*mask ; n>=h: out1 (+)= acc+b         Modules.py:871-881   */
#define GLOWTTS_EPI_COUPLE   3  /* PAIR-packed (m,logs): out0 = x_b' ; out1 = (m,logs) kept     Modules.py:795-806   */
#define GLOWTTS_EPI_DGATE    4  /* dacts -> (da, ds) through tanh/sigmoid, PAIR-packed out0      (autograd of :885-887) */

#define GLOWTTS_F_BIAS     1
#define GLOWTTS_F_RELU     2
#define GLOWTTS_F_ADD_IN0  4
#define GLOWTTS_F_MASK     8
#define GLOWTTS_F_ACCUM   16
#define GLOWTTS_F_FIRST   32   /* RESSKIP: skip accumulator is written, not accumulated */
#define GLOWTTS_F_LAST    64   /* RESSKIP: last WaveNet layer (n = h outputs, all skip, *mask) */
#define GLOWTTS_F_REVERSE 128  /* COUPLE: inverse coupling x_b = (x_b - m) * exp(-logs) * mask */
#define GLOWTTS_IO_A_BF16    1
#define GLOWTTS_IO_IN0_BF16  2
#define GLOWTTS_IO_OUT0_BF16 4
#define GLOWTTS_F_DROPOUT 512  /* LINEAR: dropout(p = drop_p, seed) after the optional ReLU, before residual / mask */
#define GLOWTTS_F_COLMASK 256  /* LINEAR: zero columns n >= ncols_valid[batch]  (attention mask, Modules.py:102) */
#define GLOWTTS_F_COND_FX 4096  /* DGATE (round 5): out1 is an array of int64 FIXED-POINT accumulators (units of 2^-40, same shape and ld1 in elements) instead of
                                  * floats; the per-utterance sums are added with 64-bit integer atomics - order-independent, bit-reproducible.  value = (double)acc * 2^-40 */
#define GLOWTTS_F_GATE_IN0 2048 /* LINEAR (round 5): in0 is the KEPT OUTPUT of a relu / dropout layer and gates the result instead of being added:
                                  * out = value * (in0 != 0 ? 1 / (1 - drop_p) : 0) - the backward of relu and dropout (Modules.py:566-567) in the epilogue of
                                  * the data-gradient conv that feeds it (was a pass of its own: glowtts_gate_bwd).  Not with GLOWTTS_F_ADD_IN0 / _DROPOUT. */
#define GLOWTTS_F_COND_ROWS 1024 /* GATE: `cond` holds one row per ACTIVATION row, [rows][ldcond] (per-frame conditioning: the GR-mode
                                  * pitch term, Modules.py:867-869, summed with the per-utterance speaker / prosody terms by the caller) */

typedef struct glowtts_conv_args {
    const float *a;  int64_t lda;      /* A rows (floats per row = lda) */
    const float *a2; int64_t lda2;     /* optional second source for channels >= ca1 */
    int ca1, ca;                       /* channels taken from a / total K per tap */
    int apro;                          /* GLOWTTS_APRO_* */
    int rows;                          /* number of rows R */
    const void *w;                     /* packed weights */
    int n, npad, kchunks;              /* logical columns, padded columns, K chunks (from pack) */
    int taps, pad;
    int precision;                     /* GLOWTTS_F32 / GLOWTTS_BF16 */
    int epi, flags;
    int h;                             /* half size for PAIR epilogues / RESSKIP split */
    int rows_per_utt;                  /* rows per utterance (for cond lookup) */
    const float *bias;                 /* [n] original (un-permuted) order */
    const float *rowmask;              /* [rows] 1 = valid frame */
    const float *cond; int64_t ldcond; /* GATE: per-utterance conditioning [B][ldcond], original order */
    float *out0; int64_t ld0;
    float *out1; int64_t ld1;          /* (DGATE: optional d conditioning [B][ld1], original order, accumulated with atomic adds BEFORE the
                                        *  dropout mask is applied to the gate gradients - zero it first) */
    const float *in0; int64_t ldi0;
    /* batched problems (gridDim.z): `rows` rows per problem; element strides between problems (0 = shared) */
    int batch;
    int64_t a_bstride, w_bstride /* bytes */, bias_bstride, out_bstride, mask_bstride;
    const int32_t *ncols_valid;        /* [batch] for GLOWTTS_F_COLMASK */
    /* GATE / DGATE: dropout on the conv output before the conditioning is added (Modules.py:861-862), p = drop_p.
     * The keep mask is a counter hash of (seed, row, channel): the backward regenerates it from the same seed. */
    uint32_t seed; float drop_p;
    const uint32_t *seed_ptr;          /* optional DEVICE word added to `seed` (lets a captured hipGraph draw new masks per replay) */
    /* bf16 activation storage (GLOWTTS_BF16 precision only): which of the `const float*` tensors actually hold bf16 elements
     * (strides then count bf16 elements).  A_BF16: a / a2 (GATE, RESSKIP+PAIRMUL, LINEAR only; ca, lda multiples of 8);
     * IN0_BF16: in0 (RESSKIP residual, DGATE gates); OUT0_BF16: out0 (GATE gates, RESSKIP state, DGATE gate gradients). */
    int io_flags;
} glowtts_conv_args;

/* Two chained 1x1 convs over the same rows in ONE launch (bf16 precision, bf16-stored `first->a`, 192 intermediate channels): the first
 * conv's output is handed to the second through LDS.  Supported pairs: (RESSKIP with F_LAST -> COUPLE): first->out1 = fp32 skip sum of the
 * earlier layers (read), first->out0 = bf16 final skip rows (written; the A operand `second->a` is ignored); (LINEAR with F_MASK -> DGATE):
 * first->out0 = bf16 d(skip) rows (written).  Everything else as in glowtts_conv_cl for the two epilogues. */
int glowtts_conv_chain(const glowtts_conv_args *first, const glowtts_conv_args *second, void *stream);
int glowtts_conv_cl(const glowtts_conv_args *args /* host pointer */, void *stream);

/* ------------------------------------------------------------------------------------------
 * Flow-decoder elementwise / reduction steps ("rows" layout).
 * rows tensors are fp32 [B][Tp][C], Tp = T + 2*GLOWTTS_ROW_PAD, channels contiguous; the first and last
 * GLOWTTS_ROW_PAD rows of every utterance are zero so the k=5 taps never cross utterances.
 * rowmask [B*Tp] is 1 for valid squeezed frames (Modules.py:903), 0 for padding and pad rows.
 */
#define GLOWTTS_ROW_PAD 2

/* Squeeze (Modules.py:895-907): mel [B][Cm][Tm] -> rows [B][Tp][ns*Cm], rows[b][PAD+t][s*Cm+c] = mel[b][c][ns*t+s]*mask;
 * also writes rowmask (may be NULL).  T = Tm / ns (an odd tail frame is dropped like :897-898). lengths: i64 [B]. */
int glowtts_squeeze_rows(const float *mel, float *rows, float *rowmask, const int64_t *lengths,
                         int B, int Cm, int Tm, int ns, void *stream);
/* Unsqueeze (Modules.py:914-924) back to [B][Cm][Tm] (* mask); with use_fill the masked frames are set to `fill`
 * (GlowTTS.inference masked_fill_, Modules.py:202). */
int glowtts_unsqueeze_rows(const float *rows, float *mel, const int64_t *lengths,
                           int B, int Cm, int Tm, int ns, int use_fill, float fill, void *stream);
/* Per-flow 4x4 inverse and log|det| (torch.inverse / torch.logdet, Modules.py:743,747).
 * W [F][4][4] -> winfo [F][36] = { W[16], W^-1[16], logdet, sign, 0, 0 }. */
int glowtts_inv1x1_prepare(const float *W, float *winfo, int F, void *stream);
/* ActNorm (Modules.py:689-694) + invertible 1x1 conv (Modules.py:738-756) in one pass over the rows.
 * reverse = 0: xout = W (bias + exp(logs) xin) ; reverse = 1: xout = (W^-1 xin - bias) exp(-logs).  In-place allowed. */
int glowtts_actnorm_inv1x1(const float *xin, float *xout, const float *logs, const float *bias,
                           const float *winfo, const float *rowmask, int64_t rows, int C, int reverse, void *stream);
/* forward form that also writes the first C/2 output channels to xpass (the coupling layer's pass-through half, Modules.py:808) */
/* ... and (xa_bf != NULL) a bf16 copy of the first C/2 output channels [rows][C/2] (glowtts_flow_acts.xa_bf) */
int glowtts_actnorm_inv1x1_pass_bf(const float *xin, float *xout, float *xpass, void *xa_bf, const float *logs, const float *bias, const float *winfo,
                                   const float *rowmask, int64_t rows, int C, void *stream);
int glowtts_actnorm_inv1x1_pass(const float *xin, float *xout, float *xpass, const float *logs, const float *bias, const float *winfo,
                                const float *rowmask, int64_t rows, int C, void *stream);
/* ActNorm data-dependent init statistics (Modules.py:698-703): stats [2C+1] = { sum x*m [C], sum x^2*m [C], sum m }.
 * Deterministic two-stage reduction; scratch holds glowtts_actnorm_stats_scratch_floats(rows, C) floats.
 * Under data parallelism the caller all-reduces `stats` before glowtts_actnorm_from_stats. */
int glowtts_actnorm_stats(const float *x, const float *rowmask, float *stats, float *scratch,
                          int64_t rows, int C, void *stream);
int64_t glowtts_actnorm_stats_scratch_floats(int64_t rows, int C);
/* logs = -0.5 log(max(var, 1e-7)), bias = -mean exp(logs)   (Modules.py:704-711) */
int glowtts_actnorm_from_stats(const float *stats, float *logs, float *bias, int C, void *stream);
/* Backward of the affine coupling transform (autograd of Modules.py:805-806).  dz [rows][C] in/out (x_b half becomes
 * d x_b), xmid = coupling input, outs/douts PAIR-packed (m, logs) [rows][ldo], dlogdet [B] = dL/dlogdet. */
int glowtts_coupling_bwd(float *dz, const float *xmid, const float *outs, float *douts, const float *rowmask,
                         const float *dlogdet, int64_t rows, int C, int ldo, int rows_per_utt, void *stream);
/* same, and a second bf16 copy of douts (act_bf16 mode: the A operand of the End conv's data gradient on the LDS-DMA / chained path) */
int glowtts_coupling_bwd_bf16(float *dz, const float *xmid, const float *outs, float *douts, void *douts_bf16, const float *rowmask,
                              const float *dlogdet, int64_t rows, int C, int ldo, int rows_per_utt, void *stream);
int glowtts_fill_zero(float *p, int64_t n, void *stream);
/* Backward of inv-1x1 + ActNorm (autograd of Modules.py:693,749-756).  dz -> dx (may alias), x = flow input.
 * param_grads [2C+16] = { dlogs[C], dbias[C], dW[16] } (data terms only; the log-det terms are added by the caller).
 * scratch: glowtts_actnorm_stats_scratch_floats(rows, C) floats. */
int glowtts_actnorm_inv1x1_bwd(const float *dz, float *dx, const float *x, const float *logs, const float *bias,
                               const float *winfo, const float *rowmask, float *param_grads, float *scratch,
                               int64_t rows, int C, void *stream);
/* number of per-block partial rows glowtts_actnorm_inv1x1_bwd leaves in scratch (each 2C+16 floats) when param_grads == NULL */
int64_t glowtts_actnorm_bwd_blocks(int64_t rows);
/* glowtts_actnorm_inv1x1_bwd (param_grads = NULL form) of flow f FUSED with glowtts_coupling_bwd(_bf16) of flow f-1: dx leaves as the
 * gradient of flow f-1's coupling input, prev_douts (+ optional bf16 copy) are filled.  One launch and one pass over the rows fewer per flow. */
int glowtts_actnorm_inv1x1_bwd_coupling(const float *dz, float *dx, const float *x, const float *logs, const float *bias, const float *winfo,
                                        const float *rowmask, float *scratch, int64_t rows, int C,
                                        const float *prev_xmid, const float *prev_outs, float *prev_douts, void *prev_douts_bf16,
                                        const float *dlogdet, int ldo, int rows_per_utt, void *stream);
/* out[b][i] = sum_r partial[b][r][i], i < n, r < nrows (deterministic): reduces the per-block partials of several
 * glowtts_actnorm_inv1x1_bwd calls made with param_grads = NULL (their `scratch` buffers, part_stride floats apart) in one launch */
int glowtts_colsum_batched(const float *partial, float *out, int nrows, int n, int batch, int64_t part_stride, int64_t out_stride, void *stream);
/* Parameter gradients of ActNorm / inv-1x1 of all F flows from the reduced data terms d_an [F][2C+16] (glowtts_colsum_batched) plus the
 * log-determinant terms of Modules.py:694, 747: dlogs [F][C], dbias [F][C], dw [F][4][4]; rowmask [B][Tp], dlogdet [B], winfo [F][36]. */
int glowtts_decoder_param_grads(const float *d_an, const float *dlogdet, const float *rowmask, const float *winfo,
                                float *dlogs, float *dbias, float *dw, int F, int B, int Tp, int C, void *stream);
/* Decoder log-determinant (Modules.py:309): logdet[b] = sum_f [ (sum logs_f + logdet W_f * C/4) * len_b + sum logs^coupling ].
 * outs_all: the F kept (m, logs) buffers, flow_stride floats apart; part [F*B] scratch. */
int glowtts_decoder_logdet(const float *outs_all, int64_t flow_stride, const float *logs_all, const float *winfo_all,
                           const float *rowmask, float *part, float *logdet, int F, int B, int Tp, int C, int ldo, void *stream);

/* ------------------------------------------------------------------------------------------
 * Weight / bias gradient of the channels-last convolution (autograd of the conv call sites above):
 *     dW[o][c][t] (+)= sum_r DY[r][o] * X[r + t - pad][c]        dbias[o] (+)= sum_r DY[r][o]
 * DY columns may be PAIR-packed (gate / coupling buffers): perm maps packed column -> o.
 * dW is written in torch Conv1d layout [O][ca][taps] fp32.  With splits > 1 (or splits = 0: automatic) or
 * accumulate != 0 the result is ADDED with fp32 atomics: the caller zeroes dW / dbias first.
 */
typedef struct glowtts_wgrad_args {
    const float *dy; int64_t lddy;     /* [rows][lddy], columns [0, m) used */
    const float *x;  int64_t ldx;      /* [rows][ldx] */
    int xpro;                          /* GLOWTTS_APRO_NONE / GLOWTTS_APRO_PAIRMUL */
    const float *xmask;                /* optional [rows] multiplier on X rows */
    int rows, m, ca, taps, pad;
    int perm, perm_h;                  /* DY column permutation */
    int precision;
    int splits, accumulate;
    float *dw;                         /* [O][ca][taps] */
    float *dbias;                      /* [O] or NULL */
    int io_flags;                      /* GLOWTTS_WIO_*: dy / x hold bf16 elements (bf16 precision only; strides count elements).
                                        * Supported: DY|X with no prologue, X alone with or without PAIRMUL. */
} glowtts_wgrad_args;
#define GLOWTTS_WIO_DY_BF16 1
#define GLOWTTS_WIO_X_BF16  2
#define GLOWTTS_WIO_WIDE    4   /* bf16 precision, no prologue, both operands stored alike (both bf16 or both fp32): the caller promises m, ca, lddy,
                                  ldx multiples of 8 and 16-byte aligned dy / x for EVERY job: operands are then staged 8 channels per item */
#define GLOWTTS_WIO_DMA     8   /* glowtts_wgrad_grouped_io only (ABI 3): the LDS-DMA kernel (192 (o) x 64 (c) x taps tiles; 192 x 192 at one tap; edge tiles are
                                 * masked on store); on top of WIDE with both operands bf16 (GLOWTTS_WIO_DY_BF16 | GLOWTTS_WIO_X_BF16) the caller promises for EVERY job: m, ca, lddy, ldx
                                 * multiples of 8, dy / x 16-byte aligned, each operand below 2 GiB, and (mt, nt) / tile0 / total_tiles counted in THAT tiling - mt = ceil(m / 192),
                                 * nt = ceil(ca / 64) (ceil(ca / 192) at one tap); precision bf16, no prologue, pad = (taps - 1) / 2, splits = 1, no accumulation (else GLOWTTS_E_ARG) */
int glowtts_wgrad_cl(const glowtts_wgrad_args *args /* host pointer */, void *stream);

/* Grouped form: many weight-gradient problems that share (rows, taps, pad, precision) in ONE launch, so that the
 * chip is filled by output tiles of different layers instead of by split-K over rows (no atomics, deterministic).
 * `dev_jobs` is a DEVICE array; tile0 = running sum of mt*nt over the preceding jobs (mt = ceil(m/128), nt = ceil(ca/64)),
 * total_tiles = sum over all jobs. */
typedef struct glowtts_wgrad_job {
    const float *dy; const float *x; const float *xmask; float *dw; float *dbias;
    int64_t lddy, ldx;
    int m, ca, xpro, perm, perm_h;
    int tile0, mt, nt;
    int rows;                          /* ABI 7 (was reserved, 0): > 0 = this job's own row count (glowtts_wgrad_grouped_phased), 0 = the launch's */
    int reserved;
} glowtts_wgrad_job;
/* every job of one launch uses the same X prologue `xpro` (job.xpro is ignored); m and ca must be multiples of 4 */
int glowtts_wgrad_grouped(const glowtts_wgrad_job *dev_jobs, int njobs, int total_tiles, int rows, int taps, int pad,
                          int xpro, int precision, int splits, int accumulate, void *stream);
/* same, with the storage types of DY / X (GLOWTTS_WIO_*) shared by every job of the launch */
int glowtts_wgrad_grouped_io(const glowtts_wgrad_job *dev_jobs, int njobs, int total_tiles, int rows, int taps, int pad,
                             int xpro, int precision, int splits, int accumulate, int io_flags, void *stream);

/* ABI 7.  The LDS-DMA kernel (GLOWTTS_WIO_DMA's conditions: bf16 rows operands, no prologue, 192 x 64 tiles - 192 x 192 at one tap) over a job table in TWO
 * PHASES for load balance: a launch of one-workgroup-per-CU tiles that exceeds the CU count by a fraction runs a second, almost empty round (288 tiles on 256
 * CUs: 2 x 169 us).  The caller puts whole problems first (`whole_tiles` tiles, at most the CU count) and the remaining problems behind them cut into row
 * splits (job.rows = rows / S, row-offset operand pointers, partial outputs summed afterwards by glowtts_sum_slices_seg): the short tiles fill the idle CUs and
 * the tail of the round.  Workgroup -> tile mapping stays XCD-contiguous inside each phase.  A cut must fall on an utterance boundary of the rows layout (the
 * pad rows make it exact for any tap count). */
int glowtts_wgrad_grouped_phased(const glowtts_wgrad_job *dev_jobs, int njobs, int total_tiles, int whole_tiles, int rows, int taps, void *stream);

/* ------------------------------------------------------------------------------------------
 * One flow step of the decoder = Activation_Norm -> Invertible_1x1_Conv -> Affine_Coupling_Layer
 * (Modules.py:653-668 AIA), launched as one host call: forward (training, keeps the activations the
 * backward needs), inverse (inference, Modules.py:664 reversed order) and backward.
 */
#define GLOWTTS_MAX_WN_LAYERS 8

typedef struct glowtts_packed {           /* result of glowtts_pack_weight */
    const void *w; int npad, kchunks;
} glowtts_packed;

typedef struct glowtts_flow_dims {
    int B, T;          /* utterances, squeezed frames per utterance (rows per utterance = T + 2*GLOWTTS_ROW_PAD) */
    int C;             /* flow channels = Mel_Dim * Num_Squeeze            (160) */
    int H;             /* Affine_Coupling.Calc_Channels                     (192) */
    int L;             /* WaveNet.Num_Layers                                (4)   */
    int ksize;         /* WaveNet.Kernel_Size                               (5)   */
    int precision;     /* GLOWTTS_F32 / GLOWTTS_BF16 for the MFMA contractions */
    float drop_p;      /* WaveNet.Dropout_Rate in training mode, 0 in eval mode          (Modules.py:854-862) */
    uint32_t seed;     /* dropout seed of this flow step (layer l uses seed + l); same value in forward and backward */
    const uint32_t *seed_ptr;  /* optional device word added to the seed (graph replay) */
    int act_bf16;      /* 1 (bf16 precision only): the GEMM-only activations - WaveNet states hs[], gates[], gate gradients dins[] -
                        * and, in the backward, dskip and dh[l >= 1] are bf16 tensors (same shapes; halves their HBM traffic and lets
                        * the LDS-DMA conv kernel stage them).  skip, outs, dh[0], the flow variable stay fp32. */
} glowtts_flow_dims;

typedef struct glowtts_flow_params {
    const float *an_logs, *an_bias;       /* ActNorm [C]                                   Modules.py:675-680 */
    const float *winfo;                   /* [36] from glowtts_inv1x1_prepare              Modules.py:725     */
    glowtts_packed start, in[GLOWTTS_MAX_WN_LAYERS], rs[GLOWTTS_MAX_WN_LAYERS], end;          /* forward images  */
    glowtts_packed start_t, in_t[GLOWTTS_MAX_WN_LAYERS], rs_t[GLOWTTS_MAX_WN_LAYERS], end_t;  /* transposed (backward only) */
    const float *b_start, *b_in[GLOWTTS_MAX_WN_LAYERS], *b_rs[GLOWTTS_MAX_WN_LAYERS], *b_end; /* biases, original order */
    const float *cond; int64_t ldcond;    /* optional conditioning [B][ldcond]; layer l reads cond + l*2H   Modules.py:863-866 */
    int cond_rows;                        /* 1: cond is per ROW, [R][ldcond] (forward / inverse only; GR-mode pitch, Modules.py:867-869) */
    const void *wn_img, *wn_img_t;        /* optional (ABI 2): this flow's weight images for the fused coupling-network kernels
                                           * (glowtts_wavenet_pack_images); NULL: the per-conv launches above are used */
} glowtts_flow_params;

typedef struct glowtts_flow_acts {        /* rows tensors, R = B*(T+2*PAD) rows */
    float *xin;                           /* [R][C] flow input                                   (kept) */
    float *xmid;                          /* [R][C] after ActNorm + inv-1x1 = coupling input     (kept) */
    float *xout;                          /* [R][C] flow output                                         */
    float *hs[GLOWTTS_MAX_WN_LAYERS];     /* [R][H]  WaveNet state entering layer l              (kept) */
    float *gates[GLOWTTS_MAX_WN_LAYERS];  /* [R][2H] (tanh, sigmoid) interleaved                 (kept) */
    float *skip;                          /* [R][H]  sum of skip outputs * mask                  (kept) */
    float *outs;                          /* [R][ldo] PAIR-packed (m, logs), ldo = end.npad      (kept) */
    const float *rowmask;                 /* [R] */
    float *acts[GLOWTTS_MAX_WN_LAYERS];   /* act_bf16 only (else NULL): [R][H] bf16 tanh * sigmoid of layer l                (kept) */
    float *skip_bf;                       /* act_bf16 only (else NULL): [R][H] bf16 copy of `skip` (End conv / its weight gradient) (kept) */
    void *xa_bf;                          /* optional (ABI 3): [R][C/2] bf16 copy of xmid[:, :C/2] = x_a, written by the flow's ActNorm + 1x1 pass: the X operand
                                           * of the Start conv's weight gradient at half the bytes (kept) */
    /* ABI 4, glowtts_flow_forward on the fused coupling network only (params->wn_img set): when next_xmid is given, the launch's coupling epilogue also
     * applies the NEXT flow's ActNorm + invertible 1x1 conv (Modules.py:693-694, 738-756; parameters next_an_logs / next_an_bias [C], next_winfo) to the
     * rows it has just produced and writes what that flow's own pass would have written: next_xmid [R][C], the x_a half of next_xout [R][C],
     * next_xa_bf (may be NULL).  The next flow is then called with actnorm_done != 0 and skips its pass. */
    const float *next_an_logs, *next_an_bias, *next_winfo;
    float *next_xmid, *next_xout;
    void *next_xa_bf;
    int actnorm_done;
} glowtts_flow_acts;

typedef struct glowtts_flow_grads {       /* backward outputs; weight grads are ADDED (zero them first) */
    float *dx;                            /* [R][C] in: dL/dxout, out: dL/dxin (in place) */
    const float *dlogdet;                 /* [B] dL/dlogdet */
    float *douts;                         /* [R][ldo] scratch (pad columns must be zero on entry).  ABI 6: may be NULL with douts_bf given and defer_wgrad set -
                                           * the coupling backward then writes the bf16 copy alone (no reader of the fp32 rows is left on that path) */
    float *dskip;                         /* [R][H] scratch */
    float *dh[GLOWTTS_MAX_WN_LAYERS];     /* [R][H] d(WaveNet state entering layer l) * mask; may alias as a ping-pong pair
                                             (dh[l] != dh[l+1]) unless defer_wgrad, which needs them all distinct */
    float *dins[GLOWTTS_MAX_WN_LAYERS];   /* [R][ldin] PAIR-packed gate pre-activation grads (pad columns zero on entry);
                                             may all alias unless defer_wgrad */
    int defer_wgrad;                      /* 1: skip every weight-gradient launch (the caller runs glowtts_wgrad_grouped later) */
    float *scratch;                       /* glowtts_actnorm_stats_scratch_floats(R, C) floats */
    float *d_an;                          /* [2C+16] = dlogs, dbias, dW(inv-1x1) data terms (overwritten); NULL: left as per-block partials
                                           * in `scratch` ([ceil(R/64)][2C+16]) for one glowtts_colsum_batched over all flows */
    float *dw_start, *db_start;           /* [H][C/2][1], [H] */
    float *dw_in[GLOWTTS_MAX_WN_LAYERS], *db_in[GLOWTTS_MAX_WN_LAYERS];   /* [2H][H][k], [2H] */
    float *dw_rs[GLOWTTS_MAX_WN_LAYERS], *db_rs[GLOWTTS_MAX_WN_LAYERS];   /* [2H|H][H][1], [2H|H] */
    float *dw_end, *db_end;               /* [C][H][1], [C] */
    int64_t *dcond;                       /* [B][ldcond] or NULL: grad of the conditioning, ACCUMULATED (zero it first): int64 fixed-point accumulators in units of
                                           * 2^-40 (integer atomics: reproducible sums; ABI 5 - typed int64_t since ABI 7, a float buffer no longer compiles).  A non-finite
                                           * or out-of-range (|v| >= 2^21) addend POISONS its accumulator (|acc| >= 2^61); glowtts_fx_to_float turns it into NaN */
    float *douts_bf;                      /* act_bf16 only (else NULL): [R][ldo] bf16 copy of douts, scratch (End data gradient operand) */
    /* fusion across flows (backward runs flow F-1 .. 0): */
    int coupling_done;                    /* 1: the previous call already applied THIS flow's coupling backward (dx, douts, douts_bf are ready) */
    const float *prev_xmid, *prev_outs;   /* not NULL: after this flow's ActNorm / 1x1 backward, apply the coupling backward of the flow that */
    float *prev_douts, *prev_douts_bf;    /*           runs next (f-1) in the same kernel; that call must then set coupling_done */
    /* GR-mode per-frame pitch conditioning (Modules.py:846-852, 867-869): the Pitch_l conv's weight gradient is
     * sum_r dpre[r][n] * pitch[r][j] over the gate-pre-activation gradients BEFORE the dropout mask, which only exist in the gate-derivative
     * epilogue.  pitch_rows [R][pitch_ns] (the squeezed pitch in the rows layout, pitch_ns <= 2) or NULL; when given, `dcond` has
     * B + pitch_ns rows and row B + j accumulates that sum for tap j (columns as in the rows above). */
    const float *pitch_rows; int pitch_ns;
    int dh0_bf16;                         /* ABI 3: dh[0] is stored as bf16 like dh[l >= 1] (act_bf16 only): the Start conv's data gradient reads it as bf16 rows and its
                                           * weight gradient takes it as a raw bf16 operand (with acts->xa_bf as X) */
} glowtts_flow_grads;

/* training forward: xin -> xout, fills every kept buffer of `acts` */
int glowtts_flow_forward(const glowtts_flow_dims *d, const glowtts_flow_params *p, const glowtts_flow_acts *a, void *stream);
/* inference inverse: xout(in) -> xin(out).  Uses hs[0], hs[1], gates[0], skip as scratch; xmid as scratch. */
int glowtts_flow_inverse(const glowtts_flow_dims *d, const glowtts_flow_params *p, const glowtts_flow_acts *a, void *stream);
/* ABI 7 (additive): glowtts_flow_forward's arithmetic in eval mode (drop_p must be 0) under glowtts_flow_inverse's scratch contract: xin -> xout,
 * reading hs[0], hs[1], gates[0], skip, acts[0] (act_bf16) and xmid as scratch and keeping nothing (outs, xa_bf may be NULL).  Honours actnorm_done
 * and, on the fused coupling network, the next_* chaining fields; a launch's reads (xmid) must not alias its writes (xout, next_xmid, next_xout). */
int glowtts_flow_encode(const glowtts_flow_dims *d, const glowtts_flow_params *p, const glowtts_flow_acts *a, void *stream);
/* backward of glowtts_flow_forward */
int glowtts_flow_backward(const glowtts_flow_dims *d, const glowtts_flow_params *p, const glowtts_flow_acts *a,
                          const glowtts_flow_grads *g, void *stream);
/* ------------------------------------------------------------------------------------------
 * Fused coupling network (Modules.py:785-806 Affine_Coupling_Layer.forward with its WaveNet, :858-887): Start conv, L x [In_l k = 5 +
 * dropout + conditioning + tanh * sigmoid, Res_Skip_l + residual / skip], End conv + affine coupling in ONE launch per flow - one
 * persistent workgroup per 64-row window (64 - 4 (L - 1) valid rows, recomputed halo), the WaveNet state in LDS, every weight of the flow
 * streamed as 24-KiB slabs through an LDS ring by LDS-DMA.  bf16 precision with act_bf16, H = 192, k = 5, L <= 4, 64 < C/2 <= 96 (the
 * reference's default decoder); anything else returns GLOWTTS_E_ARG and the caller uses the per-conv launches.
 * Weight image of one flow (forward): slabs of GLOWTTS_WN_SLAB_BYTES = [384 n][64 B]:
 *   [Start: 2 slabs][layer l: In_l 30 slabs = (tap, K chunk), Res_Skip_l 6 slabs (PAIR-packed: residual | skip per 32 channels; last
 *   layer: 3 slabs of two K chunks x 192 columns)][End: 3 slabs]  = 36 L + 2 slabs. */
#define GLOWTTS_WN_SLAB_BYTES 24576
#define GLOWTTS_WN_FUSED_MAX_LAYERS 4
int glowtts_wavenet_image_bytes(int L, int transposed, int64_t *bytes_out /* host */);
/* Packs the effective weights of F flows (stacked fp32, torch Conv1d layouts: w_start [F][H][C2][1], w_in [F][L][2H][H][5], w_rs
 * [F][L-1][2H][H][1] (NULL when L = 1), w_rs_last [F][H][H][1], w_end [F][2 C2][H][1]) into F forward images (img_fwd) and, when
 * img_bwd != NULL, F images of the transposed weights for the fused backward; image f starts at f * glowtts_wavenet_image_bytes(). */
int glowtts_wavenet_pack_images(const float *w_start, const float *w_in, const float *w_rs, const float *w_rs_last, const float *w_end,
                                int F, int L, int C2, void *img_fwd, void *img_bwd, void *stream);
/* The same images described as glowtts_prep_job entries (host array `jobs`, capacity max_jobs; appends at *njobs and advances *njobs / *block), from
 * the weight-norm pairs of the four normalised convs (v_* / g_* stacked like w_* above) and the plain End weight.  img_fwd: F forward images (its jobs
 * also write inv_* [F (* L)][O]); img_bwd: the transposed images of the first F_bwd flows (either may be NULL). */
int glowtts_wavenet_prep_jobs(glowtts_prep_job *jobs, int max_jobs, int *njobs, int *block,
                              const float *v_start, const float *g_start, float *inv_start, const float *v_in, const float *g_in, float *inv_in,
                              const float *v_rs, const float *g_rs, float *inv_rs, const float *v_rsl, const float *g_rsl, float *inv_rsl,
                              const float *w_end, int F, int L, int C2, void *img_fwd, int F_bwd, void *img_bwd);
/* xsrc [R][C]: channels [0, C/2) = x_a (WaveNet input), [C/2, C) = x_b; writes x_b' = m + exp(logs) x_b (reverse: (x_b - m) exp(-logs)),
 * masked, to xdst[r][C/2 ...].  keep != 0: fills a->hs / gates / acts / skip / outs (the activations glowtts_flow_backward reads).
 * Needs p->wn_img. */
int glowtts_wavenet_fwd(const glowtts_flow_dims *d, const glowtts_flow_params *p, const glowtts_flow_acts *a,
                        const float *xsrc, float *xdst, int reverse, int keep, void *stream);
/* Its backward, data gradients only (steps 2-4 of glowtts_flow_backward: End^T, per layer Res_Skip^T + gate derivative + In^T, Start^T), in
 * ONE launch: reads g->douts_bf (the coupling backward's bf16 d(m, logs)) and a->gates, writes g->dskip, g->dins[l] (PAIR-packed), g->dh[l]
 * and accumulates d x_a into g->dx - the operands the grouped weight-gradient launches read.  Needs p->wn_img_t (the transposed image:
 * [End^T 3 slabs][layer L-1 .. 0: Res_Skip^T 3 / 6, In^T tanh-side 15, In^T sigmoid-side 15][Start^T 2]) and g->defer_wgrad.  With g->dcond and
 * p->cond set it also ACCUMULATES the per-utterance conditioning gradient (atomic adds, like the per-conv path).  Not served: the GR-mode
 * per-row conditioning (p->cond_rows / g->pitch_rows) - GLOWTTS_E_ARG, the caller packs the per-conv images for those flows instead. */
int glowtts_wavenet_bwd(const glowtts_flow_dims *d, const glowtts_flow_params *p, const glowtts_flow_acts *a, const glowtts_flow_grads *g,
                        void *stream);

/* Diagnostics (no reference counterpart): on != 0 makes the fused kernels wait conservatively (drain their own stores) at every slab instead
 * of with exact operation counts; results must be bit-identical either way (tests/test_gpu_wavenet_fused.py). */
void glowtts_wavenet_debug_safe_waits(int on);

/* per-utterance column sums: out[b][n] = sum over the rows of utterance b of x[r][col(n)]  (conditioning grads) */
int glowtts_utt_colsum(const float *x, int64_t ldx, float *out, int64_t ldout, int B, int rows_per_utt, int n,
                       int perm, int perm_h, void *stream);

/* ------------------------------------------------------------------------------------------
 * Per-utterance conditioning of the WaveNet gates (Modules.py:832-845: Speaker_l / Prosody_l, weight-normalised Conv1d(D -> 2H, k = 1), and :863-866 where
 * their outputs join the gate pre-activation; round 5, csrc/cond_ops.hip).  All N = F * L * 2H output channels of one kind in one launch, straight from
 * the (weight_g, weight_v) pairs:   out[b][n] = (accumulate ? out[b][n] : 0) + bias[n] + g[n] / ||v[n]|| <v[n], vec[b]>
 *   v [N][D] (D <= 512), g [N], bias [N] (may be NULL), vec [B][D] (B <= 64), out [B][N]; inv_out [N] (may be NULL) receives 1 / ||v[n]|| for the backward.
 * _bwd: from dcond [B][ldd] (this kind's channel n at column n, ldd >= N): dv [N][D], dg [N], dbias [N] (may be NULL) - the weight-norm backward applied in
 * place - and, when dvec [B][D] is given, the vectors' gradient as a deterministic two-stage sum through `scratch`
 * (glowtts_cond_linear_bwd_scratch_floats(N, D, B) floats; always required). */
int glowtts_cond_linear_fwd(const float *v, const float *g, const float *bias, const float *vec, float *out, float *inv_out,
                            int N, int D, int B, int accumulate, void *stream);
int64_t glowtts_cond_linear_bwd_scratch_floats(int N, int D, int B);
/* 1 when glowtts_cond_linear_fwd AND _bwd take (N, D, B) - D in {128, 256, 384, 512}, B <= 64 and both kernels' LDS tiles ((32 + B') (D + 4) floats
 * plus the backward's extras) within 160 KiB, e.g. not D = 512 with B > 40 - else 0: the caller then forms the product itself (ABI 6). */
int glowtts_cond_linear_supported(int N, int D, int B);
/* ABI 7.  The fixed-point accumulators of glowtts_flow_grads.dcond -> float: out[i] = (float)((double)acc[i] * 2^-40), NaN where the accumulator is poisoned
 * (a NaN / Inf / out-of-range addend: the conditioning gradients propagate non-finite values like fp32 sums would). */
int glowtts_fx_to_float(const int64_t *acc, float *out, int64_t n, void *stream);
int glowtts_cond_linear_bwd(const float *dcond, int64_t ldd, const float *v, const float *g, const float *inv, const float *vec,
                            float *dv, float *dg, float *dbias, float *dvec, float *scratch, int N, int D, int B, void *stream);

/* ------------------------------------------------------------------------------------------
 * GRU recurrence of the GST prosody encoder (Modules.py:338-343, 371: torch.nn.GRU, one layer, batch_first, h0 = 0), one launch per
 * direction instead of MIOpen's ~30 launches per time step.  The caller does the GEMMs around it: gi = x W_ih^T + b_ih before,
 * dx = dgi W_ih, dW_ih = dgi^T x, dW_hh = dgh^T h_prev, db = column sums after.   3H <= 1024.
 *   gi [B][T][3H] (r | z | n pre-activations of the input side), w_hh [3H][H], b_hh [3H]
 *   hs [B][T][H] every step's state; keep [B][T][4H] = (r, z, n, W_hn h + b_hn) for the backward
 *   dhs [B][T][H] gradient w.r.t. every step's output -> dgi, dgh [B][T][3H] (gradients of the input- / hidden-side pre-activations) */
int glowtts_gru_fwd(const float *gi, const float *w_hh, const float *b_hh, float *hs, float *keep, int B, int T, int H, void *stream);
int glowtts_gru_bwd(const float *dhs, const float *hs, const float *keep, const float *w_hh, float *dgi, float *dgh,
                    int B, int T, int H, void *stream);
/* ------------------------------------------------------------------------------------------
 * Style-token tail of the GST prosody encoder (Modules.py:345-355, 371-385; ABI 6, csrc/gst_ops.hip): the GRU state at each utterance's last valid step
 * (index ceil(length / stride_prod) - 1, :373) attends over tanh(gst_Tokens) with `H` heads (RPR_MHA.py:69-128 without relative positions / masks, one query):
 *   hs [B][Tp][G] GRU states, lengths [B] i64 (mel frames), tokens [I][NT] = gst_Tokens, Wq [C][G], Wk / Wv [C][I], Wp [C][C] (Conv1d k = 1 weights) + biases [C]
 *   (may be NULL) -> out [B][C].  K, V [C][NT] (batch independent) and keep (glowtts_gst_keep_floats floats) are written for the backward; fp32 arithmetic.
 * _bwd: dout [B][C] -> dhs [B][Tp][G] (fully written: zeros but the gathered step) and every parameter gradient (overwritten; deterministic sums over the batch);
 * scratch: B (2 C + H NT) + 2 C NT floats.  C a multiple of 64, <= 1024; NT <= 256; H <= 8 (glowtts_gst_supported). */
int glowtts_gst_supported(int B, int Tp, int G, int C, int H, int NT, int I);
int64_t glowtts_gst_keep_floats(int B, int G, int C, int H, int NT, int I);
int glowtts_gst_fwd(const float *hs, const int64_t *lengths, int stride_prod, const float *tokens, const float *Wq, const float *bq, const float *Wk,
                    const float *bk, const float *Wv, const float *bv, const float *Wp, const float *bp, float *K, float *V, float *out, float *keep,
                    int B, int Tp, int G, int C, int H, int NT, int I, void *stream);
int glowtts_gst_bwd(const float *dout, const float *keep, const int64_t *lengths, int stride_prod, const float *tokens, const float *Wq, const float *Wk,
                    const float *Wv, const float *Wp, const float *K, const float *V, float *dhs, float *scratch,
                    float *dWq, float *dbq, float *dWk, float *dbk, float *dWv, float *dbv, float *dWp, float *dbp, float *dtokens,
                    int B, int Tp, int G, int C, int H, int NT, int I, void *stream);

/* ------------------------------------------------------------------------------------------
 * Direct Conv2d(3x3, stride 2, padding 1, no bias) (+ ReLU) on channels-last activations x [B][H][W][Ci] -> y [B][Ho][Wo][Co], Ho = ceil(H / 2), Wo =
 * ceil(W / 2): the six layers of the GST reference encoder (Modules.py:320-333, 366-368; ABI 6, csrc/conv2d_ops.hip).  w is the torch Conv2d weight
 * [Co][Ci][3][3] fp32.  No patch matrix, no layout change: the forward and the data gradient are implicit GEMMs on MFMA whose A rows are gathered while
 * they are staged, the weight gradient reads row-major tiles of both operands (exact-fp32 MFMA, or bf16 MFMA on fragments rounded in registers; layer 0: fp32 VALU).  Supported (glowtts_conv3x3s2_supported): Ci = 1 with
 * Co % 4 == 0, Co <= 128 (VALU kernels), or Ci, Co in {32, 64, 128}; B H W max(Ci, Co) < 2^31.
 *
 * Weight images (MFMA tile order, like glowtts_pack_weight): one forward image per layer with Ci > 1 and four data-gradient images, one per parity class
 * cls = 2 (h & 1) + (w & 1) of the INPUT pixel (a pixel of class (1, 1) is read by four taps, (0, 0) by one).  glowtts_conv3x3s2_image_bytes reports the
 * sizes; all images of a stack are written by ONE launch over a device job table (fill the jobs on the host with glowtts_conv3x3s2_pack_job_init - cls
 * = -1: forward image -, block0 = running sum of *blocks_out, copy the table to the device once: it stays valid while the pointers do). */
typedef struct glowtts_c2d_pack_job {
    const float *w; void *img;
    int Ci, Co, cls, N, K, npad, kchunks, block0;
} glowtts_c2d_pack_job;
int glowtts_conv3x3s2_supported(int B, int H, int W, int Ci, int Co);
int glowtts_conv3x3s2_image_bytes(int Ci, int Co, int precision, int64_t *fwd_bytes /* host */, int64_t *dgrad_bytes /* host [4] */);
int glowtts_conv3x3s2_pack_job_init(glowtts_c2d_pack_job *job /* host */, const float *w, int Ci, int Co, int cls, int precision, void *img,
                                    int block0, int *blocks_out /* host */);
int glowtts_conv3x3s2_pack(const glowtts_c2d_pack_job *dev_jobs, int njobs, int total_blocks, int precision, void *stream);
/* y = relu?(conv(x)).  Ci = 1: reads w; else reads img_fwd (w may be NULL). */
int glowtts_conv3x3s2_fwd(const float *x, const float *w, const void *img_fwd, float *y, int B, int H, int W, int Ci, int Co, int relu,
                          int precision, void *stream);
/* dx [B][H][W][Ci] from dpre [B][Ho][Wo][Co] (the gradient of the conv's output BEFORE its ReLU); gate (optional, shaped like dx: the layer's input = the
 * previous layer's ReLU output): dx = gate > 0 ? dx : 0, i.e. dx leaves as the previous layer's dpre.  img_dgrad: HOST array of the four class images. */
int glowtts_conv3x3s2_dgrad(const float *dpre, const void *const *img_dgrad, const float *gate, float *dx, int B, int H, int W, int Ci, int Co,
                            int precision, void *stream);
/* Weight gradient in two steps: _wgrad writes *splits_out partial images [splits][Co][(kh, kw, ci)] into `partial`
 * (glowtts_conv3x3s2_wgrad_scratch_floats(...) floats), one glowtts_conv3x3s2_wgrad_reduce over up to GLOWTTS_C2D_MAX_LAYERS layers sums them in a fixed
 * order into dw [Co][Ci][3][3] (overwritten).  Deterministic, no atomics. */
#define GLOWTTS_C2D_MAX_LAYERS 8
typedef struct glowtts_c2d_reduce_job { const float *partial; float *dw; int splits, Ci, Co, block0 /* set by the call */; } glowtts_c2d_reduce_job;
int64_t glowtts_conv3x3s2_wgrad_scratch_floats(int B, int H, int W, int Ci, int Co);
int glowtts_conv3x3s2_wgrad(const float *x, const float *dpre, float *partial, int B, int H, int W, int Ci, int Co, int precision,
                            int *splits_out /* host */, void *stream);
int glowtts_conv3x3s2_wgrad_reduce(const glowtts_c2d_reduce_job *jobs /* host */, int njobs, void *stream);

/* ------------------------------------------------------------------------------------------
 * Text-encoder kernels that are not convolutions (rows layout).
 */
/* y = rowmask * dropout( relu?( LayerNorm_C(a + b) * gamma + beta ) )   (Modules.py:485-487, 561-562, 569-571; eps 1e-4).
 * b may be NULL; when given, s_out receives a + b (the LayerNorm input the backward needs).  stats [rows][2] = (mean, rstd). */
int glowtts_layernorm_fwd(const float *a, const float *b, float *s_out, const float *gamma, const float *beta, const float *rowmask,
                          float *y, float *stats, int64_t rows, int C, float eps, int relu, float drop_p, uint32_t seed,
                          const uint32_t *seed_ptr, void *stream);
/* same, and y_bf16 (may be NULL) additionally receives y rounded to bf16: the A operand of the LDS-DMA convs that consume y */
int glowtts_layernorm_fwd_io(const float *a, const float *b, float *s_out, const float *gamma, const float *beta, const float *rowmask,
                             float *y, float *stats, int64_t rows, int C, float eps, int relu, float drop_p, uint32_t seed,
                             const uint32_t *seed_ptr, uint16_t *y_bf16, void *stream);
/* Round 4: the attention block's output projection and the LayerNorm behind it in one launch (Modules.py:560-562; replaces glowtts_conv_cl on the
 * fp32 attention rows + glowtts_layernorm_fwd_io):  proj = Dropout(a W^T + bias) (kept in proj_kept when drop_p > 0: the backward's dropout gate),
 * s = proj + x, stats = (mean, rstd) of s over C = 192 channels, y = (LayerNorm(s) gamma + beta) rowmask, y_bf16 = y rounded.  w: the packed bf16
 * image of the [192][192][1] weight (glowtts_pack_weight*, npad columns).  bf16 MFMA operands, fp32 everything else. */
int glowtts_proj_layernorm(const float *a, int64_t lda, const void *w, int npad, const float *bias, const float *x, const float *gamma,
                           const float *beta, const float *rowmask, float *proj_kept, float *s, float *stats, float *y, uint16_t *y_bf16,
                           int64_t rows, int C, float eps, float drop_p, uint32_t seed, const uint32_t *seed_ptr, void *stream);
/* Round 4: the LayerNorm that closes a transformer block and the fused Q / K / V 1x1 conv of the next block in one launch (Modules.py:571 ->
 * RPR_MHA.py:82-84; replaces glowtts_layernorm_fwd_io + glowtts_conv_cl on the bf16 rows):  s = a + b, stats, y, y_bf16 as glowtts_layernorm_fwd_io
 * (no relu, no dropout); qkv [rows][576] = y_bf16 Wqkv^T + bias, wqkv the packed bf16 image of the [576][192][1] weight (npad columns). */
int glowtts_layernorm_qkv(const float *a, const float *b, const float *gamma, const float *beta, const float *rowmask, float *s, float *stats,
                          float *y, uint16_t *y_bf16, const void *wqkv, int npad, const float *bias, float *qkv, int64_t rows, int C, float eps,
                          void *stream);
int64_t glowtts_layernorm_scratch_floats(int64_t rows, int C);
/* ds = dL/d(a + b); dgamma_dbeta [2C].  gated != 0: the forward applied relu and/or dropout, y is its output (zero where cut). */
int glowtts_layernorm_bwd(const float *dy, const float *y, const float *s, const float *stats, const float *gamma, const float *rowmask,
                          float *ds, float *dgamma_dbeta, float *scratch, int64_t rows, int C, int gated, float drop_p, void *stream);
/* same, and: ds_bf16 (may be NULL) additionally receives ds rounded to bf16 - with gate_out ([rows][C] fp32, the forward output of the conv
 * that produced the LayerNorm input) as d(pre-activation) of that conv, ds * (gate_out != 0 ? gate_scale : 0), i.e. through its relu /
 * dropout gate; dgamma_dbeta == NULL leaves the per-workgroup partials in `scratch` ([glowtts_layernorm_scratch_floats / (2C)][2C]) for one
 * glowtts_colsum_batched over several calls. */
int glowtts_layernorm_bwd_io(const float *dy, const float *y, const float *s, const float *stats, const float *gamma, const float *rowmask,
                             float *ds, float *dgamma_dbeta, float *scratch, int64_t rows, int C, int gated, float drop_p,
                             uint16_t *ds_bf16, const float *gate_out, float gate_scale, void *stream);
/* dz = dy * (out != 0 ? scale : 0) * rowmask : backward gate of relu / dropout given the forward output */
int glowtts_gate_bwd(const float *dy, const float *out, const float *rowmask, float *dz, int64_t rows, int C, float scale, void *stream);
/* io_flags: 1 = dy, 2 = out, 4 = dz stored as bf16 instead of fp32 (C a multiple of 4).  ABI 7: out == NULL (with a rowmask) = no gate, dz = dy * scale * rowmask. */
int glowtts_gate_bwd_io(const void *dy, const void *out, const float *rowmask, void *dz, int64_t rows, int C, float scale, int io_flags, void *stream);
/* rows[b][PAD+t][:] = table[tokens[b][t]][:] * scale * mask (Modules.py:267), and its gradient (deterministic) */
/* mask [B][T] = (t < lengths[b]) and the rows layout's row mask [B][T + 2 GLOWTTS_ROW_PAD] (zero pad rows) in one launch (Modules.py:206-211; round 5) */
int glowtts_token_masks(const int64_t *lengths, float *mask, float *rowmask, int B, int T, void *stream);
int glowtts_embedding_fwd(const int64_t *tokens, const float *table, const float *rowmask, float *rows, int B, int T, int C, float scale, void *stream);
int glowtts_embedding_bwd(const int64_t *tokens, const float *drows, const float *rowmask, float *dtable, int V, int B, int T, int C, float scale, void *stream);
/* Relative-position multi-head self-attention core (RPR_MHA.py:95-128; window `win`, embeddings shared over heads).
 * qkv rows [B][Tp][3*H*D] (Q | K | V); out rows [B][Tp][H*D]; P [B][H][Tp][Tp] is kept for the backward (opaque to the caller:
 * the MFMA paths - D in {64, 96}, win <= 15; one workgroup per (utterance, head) for Tp <= 128, query / key blocks above - store the
 * probabilities before dropout, the general path after). Tp <= 256.
 * The backward takes the forward's (seed, seed_ptr): it regenerates the dropout keep mask. */
int glowtts_rpr_attention_fwd(const float *qkv, const float *relk, const float *relv, const float *rowmask, float *out, float *P,
                              int B, int Tp, int H, int D, int win, float drop_p, uint32_t seed, const uint32_t *seed_ptr, void *stream);
int64_t glowtts_rpr_attention_scratch_floats(int B, int Tp, int H, int D, int win);
/* scratch: glowtts_rpr_attention_scratch_floats(...) + 2*(2*win+1)*D floats; dS: [B][H][Tp][Tp] floats (general path only);
 * drelk / drelv [2*win+1][D] each; passing them adjacent (one [2][2*win+1][D] tensor) saves two copies */
int glowtts_rpr_attention_bwd(const float *qkv, const float *relk, const float *relv, const float *rowmask, const float *P, const float *dout,
                              float *dS, float *dqkv, float *drelk, float *drelv, float *scratch,
                              int B, int Tp, int H, int D, int win, float drop_p, uint32_t seed, const uint32_t *seed_ptr, void *stream);
/* The same with an arithmetic mode (GLOWTTS_F32 = the two functions above; GLOWTTS_BF16: for Tp <= 128 the five contractions of the core run on
 * bf16 MFMAs - operands rounded to bf16 in registers, fp32 accumulate, fp32 softmax - the other paths are fp32 in either mode). */
int glowtts_rpr_attention_fwd_prec(const float *qkv, const float *relk, const float *relv, const float *rowmask, float *out, float *P,
                                   int B, int Tp, int H, int D, int win, float drop_p, uint32_t seed, const uint32_t *seed_ptr, int precision, void *stream);
/* rows of per-workgroup partial sums of (d relK | d relV) [rows][2 (2 win + 1) D] that glowtts_rpr_attention_bwd* leaves at the head of `scratch`; with
 * drelk == drelv == NULL (round 5) the call stops there and the caller sums them itself (glowtts_colsum_batched over several layers at once). */
int64_t glowtts_rpr_attention_bwd_partial_rows(int B, int Tp, int H, int D, int win);
/* Eval-mode attention core (RPR_MHA.py:95-128) for any Tp >= 1 (long-text inference): what glowtts_rpr_attention_fwd_prec computes on valid
 * rows, without dropout and without the probability matrix - keys stream through LDS in blocks with an online softmax, so neither LDS nor
 * device memory grows with Tp^2 and no scratch is needed.  Same qkv / out / rowmask layouts; rows of padded queries are finite.
 * D <= 128.  D in {64, 96} with win <= 15: MFMA path (GLOWTTS_F32: v_mfma_f32_32x32x2_f32, exact fp32; GLOWTTS_BF16: bf16 operands on
 * v_mfma_f32_32x32x16_bf16, fp32 softmax and accumulate); any other D or window: fp32 VALU path in either mode. */
int glowtts_rpr_attention_fwd_eval(const float *qkv, const float *relk, const float *relv, const float *rowmask, float *out,
                                   int B, int Tp, int H, int D, int win, int precision, void *stream);
int glowtts_rpr_attention_bwd_prec(const float *qkv, const float *relk, const float *relv, const float *rowmask, const float *P, const float *dout,
                                   float *dS, float *dqkv, float *drelk, float *drelv, float *scratch,
                                   int B, int Tp, int H, int D, int win, float drop_p, uint32_t seed, const uint32_t *seed_ptr, int precision, void *stream);

/* ------------------------------------------------------------------------------------------
 * Alignment expansion and likelihood loss.
 */
/* out[b][c][y] = idx[b][y] >= 0 ? src[b][c][idx[b][y]] : 0   ==  src @ attentions (Modules.py:120-121), attentions one-hot per frame */
/* Operands of the log-prior GEMM (Modules.py:108-114) in one launch: the fp32 MFMA weight image of (sigma^-2 | mu sigma^-2)
 * [B][kchunks][npad][16] (what glowtts_pack_weight_batched(F32) would produce from [B][Tx][2 Cm]), the per-token constant cb [B][Tx], the
 * frame mask [B][Ty] and the lengths as int32; mel lengths are first rounded down to a multiple of `mel_multiple` (Decoder.Num_Squeeze,
 * Modules.py:897-898).  packed == NULL: size query (npad_out, kchunks_out). */
int glowtts_logprior_prep(const float *mean, const float *log_std, const int64_t *token_lengths, const int64_t *mel_lengths, float *packed,
                          float *cb, float *fmask, int32_t *tx32, int32_t *ty32, int B, int Cm, int Tx, int Ty, int mel_multiple,
                          int *npad_out, int *kchunks_out, void *stream);
int glowtts_expand_fwd(const float *src, const int32_t *idx, float *out, int B, int C, int Tx, int Ty, void *stream);
/* its gradient w.r.t. src: a segment sum over the (contiguous) frames of each token */
int glowtts_expand_bwd(const float *dout, const int32_t *idx, float *dsrc, int B, int C, int Tx, int Ty, void *stream);
/* log_Duration_Targets = log(frames per token + 1e-7) * token_mask   (Modules.py:122); out [B][Tx] */
int glowtts_duration_targets(const int32_t *idx, const int64_t *token_lengths, float *out, int B, int Tx, int Ty, void *stream);
/* MLE_Loss (Modules.py:1020-1029) over n = B*mel_dim*T_mel elements; loss and inv_denom are device scalars; scratch 1024 floats */
int glowtts_mle_loss_fwd(const float *z, const float *mean, const float *log_std, const float *log_dets, const int64_t *lengths,
                         float *loss, float *inv_denom, float *scratch, int64_t n, int B, int n_squeeze, int mel_dim, void *stream);
/* dlogdet (optional, [B]): also writes d loss / d log_dets[b] = -dloss * inv_denom */
int glowtts_mle_loss_bwd(const float *z, const float *mean, const float *log_std, const float *dloss, const float *inv_denom,
                         float *dz, float *dmean, float *dlog_std, int64_t n, float *dlogdet, int B, void *stream);
/* ABI 6.  Both expansions and the duration targets of Modules.py:120-122 in one launch (Ty % 4 == 0, 16-byte aligned idx / outputs): mel_mean, mel_log_std
 * [B][C][Ty] as glowtts_expand_fwd, targets [B][Tx] as glowtts_duration_targets.  ABI 7: path (optional, fp32 [B][Tx][Ty], 16-byte aligned): the dense 0/1
 * attentions of Modules.py:116 as glowtts_mas_path_from_idx writes them, in the same launch. */
int glowtts_expand_pair_targets(const float *mean, const float *log_std, const int32_t *idx, const int64_t *token_lengths, float *mel_mean,
                                float *mel_log_std, float *targets, float *path, int B, int C, int Tx, int Ty, void *stream);
/* ABI 6.  glowtts_mle_loss_bwd THROUGH the expansion, in one launch: z [B][C][Ty], the TOKEN-space mean / log_std [B][C][Tx] the expansion gathered from and idx
 * [B][Ty] -> dz [B][C][Ty] and the token-space gradients dmean / dlog_std [B][C][Tx] (each token's frames are one contiguous run: segment sums, no atomics;
 * the same bits as glowtts_mle_loss_bwd followed by two glowtts_expand_bwd); dlogdet optional as above.  Tx <= 1024. */
int glowtts_prior_loss_bwd(const float *z, const float *mean, const float *log_std, const int32_t *idx, const float *dloss, const float *inv_denom,
                           float *dz, float *dmean, float *dlog_std, float *dlogdet, int B, int C, int Tx, int Ty, void *stream);
/* ABI 6.  loss = s * sum (a - target)^2 and da = 2 s dloss (a - target), one launch per direction; loss / dloss are device scalars.  s = `scale` (Train.py:203-211:
 * MSELoss on the log durations, scale = 1 / n), or - lengths [B] i64 given - 1 / (B max(lengths)): the mean over the batch's own longest text when the token axis is
 * padded to a shape bucket, or - extent (device scalar) given - 1 / (B extent[0]): data parallel, the global batch's longest text. */
int glowtts_mse_loss_fwd(const float *a, const float *target, float *loss, int64_t n, float scale, const int64_t *lengths, int B, const float *extent,
                         float *da_unit, void *stream);
int glowtts_mse_loss_bwd(const float *a, const float *target, const float *dloss, float *da, int64_t n, float scale, const int64_t *lengths, int B,
                         const float *extent, void *stream);
/* ABI 7.  glowtts_mse_loss_fwd's da_unit (optional, [n]): the gradient for d loss = 1, written by the forward launch (glowtts_mse_loss_bwd's value for that seed). */
/* ABI 7.  MLE_Loss (Modules.py:1020-1029) on the expanded prior - value AND gradients for the seed dloss[0] - in ONE launch: glowtts_mle_loss_fwd on
 * (z, mel_mean, mel_log_std) [B][C][Ty] and glowtts_prior_loss_bwd on the token-space (mean, log_std) [B][C][Tx] + idx [B][Ty], the same bits as those calls.
 * scratch: 1024 floats; counter: one uint32 zeroed once by the caller (the kernel leaves it zero).  dlogdet optional.  Tx <= 1024. */
int glowtts_prior_loss(const float *z, const float *mel_mean, const float *mel_log_std, const float *mean, const float *log_std, const int32_t *idx,
                       const float *log_dets, const int64_t *lengths, const float *dloss, float *scratch, uint32_t *counter, float *loss, float *inv_denom,
                       float *dz, float *dmean, float *dlog_std, float *dlogdet, int B, int C, int Tx, int Ty, int n_squeeze, int mel_dim, void *stream);
/* ABI 7.  Duration_Predictor's Projection (Modules.py:596-618: Conv1d(C -> 1, k = 1) on masked features, times the mask) on rows: d [B][T + 2 pad][C] fp32
 * (16-byte aligned, C % 4 == 0, C <= 1024), w [C], bias [1], mask [B][T] -> out [B][T].  Backward: g [B][T] -> dd rows (pad rows zero), dw [C], dbias [1];
 * scratch B * (C + 1) floats, counter one uint32 zeroed once (left zero).  Fixed summation order. */
int glowtts_dur_proj_supported(int C);
int glowtts_dur_proj_fwd(const float *d, const float *w, const float *bias, const float *mask, float *out, int B, int T, int pad, int C, void *stream);
int glowtts_dur_proj_bwd(const float *g, const float *mask, const float *d, const float *w, float *dd, float *dw, float *dbias, float *scratch,
                         uint32_t *counter, int B, int T, int pad, int C, void *stream);
/* ABI 7.  The encoder's projected rows [B][T + 2 pad][2 M] -> mean, log_std [B][M][T] (Modules.py:283-286) and back (dmean / dlog_std may be NULL = zero;
 * pad rows of drows are zeroed). */
int glowtts_prior_split_fwd(const float *rows, float *mean, float *log_std, int B, int T, int pad, int M, void *stream);
int glowtts_prior_split_bwd(const float *dmean, const float *dlog_std, float *drows, int B, int T, int pad, int M, void *stream);

/* ------------------------------------------------------------------------------------------
 * Old-style weight normalisation of the WaveNet convolutions (Modules.py:766,818,825,838,845: torch.nn.utils.weight_norm,
 * norm over (in, k) per output channel) for a whole stack of convs per launch.
 *   v [rows][cols], g [rows]  ->  w = g * v / ||v||  [rows][cols],  inv_norm [rows] = 1 / ||v||   (kept for the backward)
 *   backward: dg = <dw, v> / ||v||,  dv = g / ||v|| * (dw - v <dw, v> / ||v||^2)
 * rows = stacked convs x output channels, cols = in * k.  All pointers fp32 device tensors. */
int glowtts_weightnorm_fwd(const float *v, const float *g, float *w, float *inv_norm, int64_t rows, int cols, void *stream);
int glowtts_weightnorm_bwd(const float *dw, const float *v, const float *g, const float *inv_norm, float *dv, float *dg,
                           int64_t rows, int cols, void *stream);
/* ABI 7.  Up to GLOWTTS_WN_BWD_MAX_JOBS glowtts_weightnorm_bwd problems in one launch (`jobs` is a HOST array; same arithmetic, same bits). */
#define GLOWTTS_WN_BWD_MAX_JOBS 8
typedef struct glowtts_wn_bwd_job {
    const float *dw, *v, *g, *inv_norm; float *dv, *dg;
    int64_t rows; int cols, reserved;
} glowtts_wn_bwd_job;
int glowtts_weightnorm_bwd_multi(const glowtts_wn_bwd_job *jobs, int njobs, void *stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer side of the training step: multi-tensor launches over a DEVICE job table.
 * A job = one contiguous run of fp32 elements (a stacked weight class is one job); block0 = running sum of ceil(n / glowtts_opt_chunk())
 * over the preceding jobs, total_blocks = that sum over all jobs.
 *   glowtts_multi_grad_norm : norm_and_coef[0] = ||all gradients||_2, [1] = min(1, max_norm / (norm + 1e-6))   (torch.nn.utils.clip_grad_norm_,
 *                             Train.py:228-231); partial: total_blocks floats of scratch; deterministic two-stage reduction
 *   glowtts_multi_grad_scale: g *= coef[0] in place (clip_grad_norm_'s second half)
 *   glowtts_radam_step      : Rectified Adam exactly as Radam.py:45-90.  hyper (device, 8 floats): lr, beta1, beta2, eps, weight_decay,
 *                             step_size, rectified (N_sma >= 5), unused - computed on the host per step like Radam.py:63-79 and uploaded, so a
 *                             captured hipGraph of the step stays valid while the learning rate changes; grad_scale (device, optional): the
 *                             clip coefficient applied on the fly instead of a separate scale pass. */
typedef struct glowtts_opt_job {
    float *p; const float *g; float *m; float *v;     /* parameter, gradient, exp_avg, exp_avg_sq */
    int64_t n;
    int64_t block0;
} glowtts_opt_job;
int glowtts_opt_chunk(void);
int glowtts_multi_grad_norm(const glowtts_opt_job *dev_jobs, int njobs, int total_blocks, float max_norm, float *partial,
                            float *norm_and_coef, void *stream);
/* out[i] = sum over s < S of partial[s][i], i < n, in a fixed order (round 5; n % 4 == 0, both pointers 16-byte aligned): the row splits of the text
 * encoder's weight gradients summed into the gradients (no reference counterpart: autograd of Modules.py:438-573 accumulates in one pass). */
int glowtts_sum_slices(const float *partial, float *out, int S, int64_t n, void *stream);
/* ... into up to GLOWTTS_SUM_MAX_SEGS destination tensors: partial [S][stride]; segment k = elements [off, off + n) of a slice -> dst[0 .. n); the segments tile
 * [0, sum n) in ascending order, every n a multiple of 4, every dst 16-byte aligned (the decoder's one-tap weight gradients in row splits). */
#define GLOWTTS_SUM_MAX_SEGS 12
typedef struct glowtts_sum_seg { float *dst; int64_t off, n; } glowtts_sum_seg;
int glowtts_sum_slices_seg(const float *partial, int S, int64_t stride, const glowtts_sum_seg *segs /* host */, int nseg, void *stream);
int glowtts_multi_grad_scale(const glowtts_opt_job *dev_jobs, int njobs, int total_blocks, const float *coef, void *stream);
int glowtts_radam_step(const glowtts_opt_job *dev_jobs, int njobs, int total_blocks, const float *hyper, const float *grad_scale, void *stream);

/* ------------------------------------------------------------------------------------------
 * Griffin-Lim vocoder (waveform output; no reference counterpart: the reference's Inference.py stops at the mel).  New symbols only, the ABI version stays 7.
 * It inverts the front end of Audio.py:14-47 as glow_tts_amd/audio.py restates it: STFT with center = True, reflect padding by n_fft / 2, a periodic Hann
 * window of win_length centred in n_fft, hop `hop`.  Supported geometry (glowtts_vocoder_supported, else GLOWTTS_E_ARG): n_fft a power of two in
 * [256, 4096], win_length <= n_fft, win_length % hop == 0.  F = n_fft / 2 + 1 everywhere.
 *   window  [win_length] f32, twiddle [n_fft / 2][2] f32 = (cos, -sin)(2 pi k / n_fft): tables the host computes in float64 and rounds.
 *   A T-frame spectrogram corresponds to hop * (T - 1) samples; signals are [B][ldx] with ldx >= hop * (T - 1).
 *   Lengths are device data and cannot be checked on the host without a synchronisation: they are the caller's to get right.  Lengths beyond T frames
 *   are clamped to T.  An utterance longer than its signal row (wav_lengths[b] > ldx, or hop * (frame_lengths[b] - 1) > ldx) is never read or written
 *   beyond ldx; it is a caller error, and the result for that utterance is then all zeros (glowtts_stft_f32) or frames left unwritten (the others).
 *
 * glowtts_mel_to_linear_f32: mels [B][Mel][T] normalised to +- max_abs (Audio.py:44-47) -> mag [B][T][F] = max(basis . amp, 1e-10) with
 *   amp = max(10^(((clip(mel, +-max_abs) + max_abs) / (2 max_abs) * 100 - 100) / 20) - 1e-7, 0), basis [F][Mel]; frames t >= frame_lengths[b] are zeros.
 * glowtts_stft_f32: wav [B][ldx], wav_lengths [B] i32 (samples; utterance b has 1 + len / hop frames) -> spec [B][T][F][2] (re, im); frames beyond: zeros.
 * glowtts_istft_f32: spec [B][T][F][2], frame_lengths [B] i32 -> wav [B][ldx]: per frame the inverse real FFT, windowed again (into `frames`
 *   [B][T][win_length], scratch), then glowtts_overlap_add_f32.  The imaginary parts of bins 0 and n_fft / 2 are ignored.
 * glowtts_overlap_add_f32: every sample GATHERS its win_length / hop contributing frames in ascending frame order and is divided by the summed squared
 *   window floored at 1e-8 (no atomics: bit-identical from run to run); samples at or beyond hop * (frame_lengths[b] - 1) are written as zeros.
 * glowtts_griffin_lim_step_f32: one fused iteration.  Per frame: y = x + alpha (x - x_prev) gathered and windowed, forward FFT, P = Y / max(|Y|, 1e-8),
 *   times mag [B][T][F], inverse FFT, windowed -> frames [B][T][win_length]; the spectrum stays in LDS.  glowtts_overlap_add_f32 turns `frames`
 *   into the next signal.  Frames at or beyond frame_lengths[b] are left untouched. */
int glowtts_vocoder_supported(int n_fft, int win_length, int hop);
int glowtts_mel_to_linear_f32(const float *mels, const int32_t *frame_lengths, const float *basis, float *mag, int B, int Mel, int T, int F, float max_abs,
                              void *stream);
int glowtts_stft_f32(const float *wav, const int32_t *wav_lengths, const float *window, const float *twiddle, float *spec, int B, int ldx, int T, int n_fft,
                     int win_length, int hop, void *stream);
int glowtts_istft_f32(const float *spec, const int32_t *frame_lengths, const float *window, const float *twiddle, float *frames, float *wav, int B, int T,
                      int ldx, int n_fft, int win_length, int hop, void *stream);
int glowtts_overlap_add_f32(const float *frames, const int32_t *frame_lengths, const float *window, float *wav, int B, int T, int ldx, int n_fft,
                            int win_length, int hop, void *stream);
int glowtts_griffin_lim_step_f32(const float *x, const float *x_prev, const float *mag, const int32_t *frame_lengths, const float *window,
                                 const float *twiddle, float alpha, float *frames, int B, int T, int ldx, int n_fft, int win_length, int hop, void *stream);

/* ------------------------------------------------------------------------------------------
 * Analysis front end (csrc/frontend_ops.hip): what Pattern_Generator.py computes per utterance - the mel of Audio.py:14-47 and the YIN pitch track of
 * yin.py - as glow_tts_amd/audio.py restates them (`mel_generate`, `yin_pitch`), in fp32.  New symbols only, the ABI version stays 7.
 * Signals are [B][ldx] f32 with wav_lengths [B] i32 on the device; an utterance with wav_lengths[b] > ldx is a caller error that is never read beyond
 * ldx and comes out as padding.  1 <= B <= 65535, T >= 1, ldx >= 1 and B * T <= 2^30, else GLOWTTS_E_ARG.  Both are bit-identical from run to run and independent of the batch around an utterance (fixed reduction orders, no atomics).
 *
 * glowtts_mel_analysis_f32: -> mel [B][T][Mel], utterance b has T_b = 1 + len / hop frames (clamped to T); frames beyond are -max_abs.  Per frame:
 *   pre-emphasis y[s] = x[s] - pre_emphasis x[s-1] (y[0] = x[0]) applied while gathering, reflect padding of y by n_fft / 2, the window / twiddle tables of
 *   the vocoder, FFT, |Y|, the mel filterbank in SPARSE form - fb_index [Mel][3] i32 = (first bin, bin count, offset into fb_weight), fb_weight [n_weights]
 *   f32: row j of the dense filterbank is fb_weight[offset_j .. offset_j + count_j) at bins first_j .. - then 20 log10(m + 1e-7) and
 *   clip(2 max_abs (db - min_db) / (-min_db) - max_abs, +- max_abs).  Geometry: n_fft a power of two in [256, 4096], 1 <= win_length <= n_fft, hop >= 1
 *   (no win_length % hop condition: nothing is overlap-added), Mel <= 1024; else GLOWTTS_E_ARG.
 * glowtts_yin_f32: -> pitch [B][T] in Hz, 0 where unvoiced or beyond the utterance; when cmnd is not NULL also the cumulative-mean-normalised difference
 *   cmnd [B][T][tau_max].  The signal is reflect-padded by (w_step + w_len - len % w_step) / 2 samples each side (index arithmetic), frames start every
 *   w_step samples, ceil((padded length - w_len) / w_step) of them (clamped to T).  d(tau) = sum_{j < w_len - tau} (x_j - x_{j+tau})^2 summed directly,
 *   cm[0] = 1, cm[tau] = d(tau) tau / (sum_{1..tau} d + 1e-8); the first tau in [tau_min, tau_max) with cm < thresh, walked forward while
 *   cm[tau + 1] < cm[tau], gives pitch = sample_rate / tau.  Supported: w_len <= 2048, 1 <= tau_min < tau_max <= w_len; else GLOWTTS_E_ARG. */
int glowtts_mel_analysis_f32(const float *wav, const int32_t *wav_lengths, const float *window, const float *twiddle, const int32_t *fb_index,
                             const float *fb_weight, float *mel, int B, int ldx, int T, int Mel, int n_weights, int n_fft, int win_length, int hop,
                             float pre_emphasis, float min_db, float max_abs, void *stream);
int glowtts_yin_f32(const float *wav, const int32_t *wav_lengths, float *pitch, float *cmnd, int B, int ldx, int T, int w_len, int w_step, int tau_min,
                    int tau_max, float thresh, float sample_rate, void *stream);

/* ---- seeded prior sample of GlowTTS.inference (csrc/sample_ops.hip; an addition, the ABI version stays) ----
 * Modules.py:175-191 in ONE launch, logged as `prior_sample`: mean / log_std [B][C][Tx] (the text encoder's), dur [B][Tx] (integer-valued, >= 0),
 * mel_lengths [B] -> with cum the running sum of dur (int32):
 *   idx  [B][Tmax]      idx[y] = #{x : cum[x] <= y} where y < mel_lengths[b] and that count is < Tx, else -1
 *   attn [B][Tx][Tmax]  attn[x][y] = (idx[y] == x), every element written; NULL: not written
 *   z    [B][C][Tmax]   mean[idx] + exp(log_std[idx]) * gauss(seeds[b][0], seeds[b][1], c, y, C) * noise_scales[b] where idx >= 0, exactly 0 elsewhere
 * gauss is the counter hash of csrc/gauss_hash.h (a frozen contract, DESIGN.md "Seeded sampling"): a function of the utterance's two seed words, the
 * channel and the frame only - not of B, Tx, Tmax or the utterance's place in the batch.  seeds [B][2] and noise_scales [B] are DEVICE buffers read by the
 * kernel (a captured graph reads them at every replay).  Tx of any length: the durations are scanned through LDS in chunks of GLOWTTS_SAMPLE_SCAN_CHUNK
 * tokens; grid (ceil(Tmax / GLOWTTS_SAMPLE_TILE), B).  16-byte stores when Tmax % 4 == 0 and z / attn are 16-byte aligned, the same values otherwise. */
#define GLOWTTS_SAMPLE_SCAN_CHUNK 1024
#define GLOWTTS_SAMPLE_TILE 64
int glowtts_prior_sample(const float *mean, const float *log_std, const float *dur, const int64_t *mel_lengths, const uint32_t *seeds,
                         const float *noise_scales, float *z, int32_t *idx, float *attn, int B, int C, int Tx, int Tmax, void *stream);
/* The teacher-forced counterpart (an addition, the ABI version stays): the sample of the prior ALONG a given index, the index's run lengths and the
 * alignment score, logged as `prior_sample_aligned` (+ `prior_score_final` when score is asked for; the durations are a token-indexed block of the
 * first launch's grid, not a launch of their own).
 *   idx   [B][Tmax]     the per-frame token index as glowtts_mas_dp_f32_t and glowtts_prior_sample write it: values in [0, Tx), -1 past the utterance.
 *                       ANY value outside [0, Tx) is treated as -1; nothing is read out of bounds.
 *   z_rec [B][C][Tmax]  the recording's latent; may be NULL (then score must be NULL)
 * Outputs, each may be NULL independently (not all three), except that score needs score_partials and z_rec:
 *   z     [B][C][Tmax]  mean[idx] + exp(log_std[idx]) * gauss(seeds[b][0], seeds[b][1], c, y, C) * noise_scales[b] where idx >= 0, exactly 0 elsewhere: the
 *                       bits glowtts_prior_sample writes for the same idx (one device function serves both).  seeds / noise_scales: device buffers as
 *                       above, required with z.
 *   dur   [B][Tx]       the number of frames y with idx[y] == x; every element is written
 *   score [B]           the mean over the utterance's valid (c, y) of  -0.5 log(2 pi) - ls - 0.5 (z_rec - m)^2 exp(-2 ls),  m / ls gathered by idx: the
 *                       log-prior density per element along the alignment (what MAS maximised), NOT a likelihood (no log-determinants); 0 for an
 *                       utterance without a valid frame.  Per-tile partials go to score_partials [B][ceil(Tmax / GLOWTTS_SAMPLE_TILE)] by one fixed
 *                       summation tree (the same in both store forms, invalid frames add +0.0); the second launch adds the tiles in ascending order and
 *                       divides.  No float atomics: an utterance's score has the same bits alone, in any batch, at any Tmax.
 * GLOWTTS_E_ARG as for glowtts_prior_sample (NULL required pointer, B outside 1..65535, counters out of range). */
int glowtts_prior_sample_aligned(const float *mean, const float *log_std, const int32_t *idx, const float *z_rec, const uint32_t *seeds,
                                 const float *noise_scales, float *z, int32_t *dur, float *score, float *score_partials, int B, int C, int Tx, int Tmax,
                                 void *stream);

/* ---- neural vocoder: Parallel WaveGAN generator (csrc/pwg_ops.hip; inference, f32; additions, the ABI version stays) ----
 * Rows are samples, channels-last: x [B][Lmax hop][R], c [B][Lmax hop][A], skips [B][Lmax hop][S]; frame_lengths [B] i32 (device) are the utterances'
 * frame counts L <= Lmax, an utterance owns rows [0, L hop) of its slab and only those are read or written (the waveform is zero beyond them).  Every
 * value depends on its own utterance and a fixed summation order only.  All matrix products: v_mfma_f32_16x16x4_f32.
 * Supported (glowtts_pwg_supported, else GLOWTTS_E_ARG): R, S multiples of 16 and A a multiple of 4, all <= 256; G == 2 R; dilation in [1, 1024]; the
 * layer's LDS tile within 160 KB; 1 <= B <= 65535, 1 <= hop <= 65536, Lmax hop <= 2^30; at most 8 scales, each in [1, 16]; 0 <= ctx <= 16.
 * glowtts_pwg_condition: mel [B][A][Lmax] -> c.  w_in [(2 ctx + 1) A][A] (row = tap * A + input channel) is conv_in, whose replicate padding uses the
 *   utterance's own first / last frame; then per scale s: nearest-neighbour repeat and the (2 s + 1)-tap FIR (firs: the scales' taps one after another),
 *   zero beyond the utterance's own ends.  scales is a HOST array.  work: 2 * B * Lmax * A * (hop / last scale) floats.  Logged as `pwg_cond_in` and one
 *   `pwg_upsample` per scale.
 * glowtts_pwg_first: x = first_conv(z), w / bias [R]; z[t] = noises [B][Lmax hop] or, noises NULL, gauss(seeds[b][0], seeds[b][1], 0, t, 1) of
 *   csrc/gauss_hash.h evaluated in the kernel (seeds [B][2] u32 on the device); exactly one of the two is given.
 * glowtts_pwg_layer: one WaveNet layer in one launch.  w1 [3 R + A][2 R]: rows x(t - d) | x(t) | x(t + d) | aux channels, columns tanh half | sigmoid
 *   half, b1 [2 R];  w2 [R][R + S]: columns conv1x1_out | conv1x1_skip, b2 [R + S].  x_out = (out + x) sqrt(0.5) (x_out != x: neighbours read x);
 *   skips = skip (accumulate == 0) or skips + skip.
 * glowtts_pwg_head: wav [B][Lmax hop] = w2 . relu(w1^T relu(skips * scale) + b1) + b2;  w1 [S][S] (row = input channel), w2 [S], b2 [1]. */
int glowtts_pwg_supported(int R, int G, int S, int A, int max_dilation);
int glowtts_pwg_condition(const float *mel, const int32_t *frame_lengths, const float *w_in, const float *firs, const int *scales, int n_scales,
                          float *work, float *c, int B, int A, int Lmax, int ctx, void *stream);
int glowtts_pwg_first(const float *noises, const uint32_t *seeds, const int32_t *frame_lengths, const float *w, const float *bias, float *x, int B,
                      int Lmax, int hop, int R, void *stream);
int glowtts_pwg_layer(const float *x, const float *c, const float *w1, const float *b1, const float *w2, const float *b2, float *x_out, float *skips,
                      const int32_t *frame_lengths, int B, int Lmax, int hop, int R, int S, int A, int dilation, int accumulate, void *stream);
int glowtts_pwg_head(const float *skips, const int32_t *frame_lengths, const float *w1, const float *b1, const float *w2, const float *b2, float *wav,
                     int B, int Lmax, int hop, int S, float scale, void *stream);

/* ---- neural vocoder, bf16 inference mode (csrc/pwg_bf16_ops.hip; additions, the ABI version stays) ----
 * glowtts_pwg_layer_bf16 is glowtts_pwg_layer with bf16 operands on v_mfma_f32_16x16x32_bf16, logged as `pwg_layer_bf16`: the gathered rows
 * x(t - d) | x(t) | x(t + d) | c(t), the weights and the gate tanh * sigmoid are rounded to bf16 (nearest even); the accumulators, the biases, tanh / sigmoid,
 * the residual (which adds the unrounded x), the skip sum and x, x_out, skips in memory stay f32.  Rows, lengths, ownership and bit-identity as for
 * glowtts_pwg_layer.  The weights come as packed bf16 images [Kp / 8][N][8] - element (k, n) at ((k / 8) N + n) 8 + k % 8, Kp = K rounded up to a multiple of
 * 32, zero rows beyond K:  w1p packs w1 (K = 3 R + A, N = 2 R), w2p packs w2 (K = R, N = R + S); b1, b2 as for glowtts_pwg_layer.
 * Supported (glowtts_pwg_supported_bf16, else GLOWTTS_E_ARG): glowtts_pwg_supported, and the bf16 LDS tile 128 (Kp(3 R + A) + Kp(R) + 16) bytes within 160 KB. */
int glowtts_pwg_supported_bf16(int R, int G, int S, int A, int max_dilation);
int glowtts_pwg_layer_bf16(const float *x, const float *c, const uint16_t *w1p, const float *b1, const uint16_t *w2p, const float *b2, float *x_out,
                           float *skips, const int32_t *frame_lengths, int B, int Lmax, int hop, int R, int S, int A, int dilation, int accumulate,
                           void *stream);

/* ---- neural vocoder: HiFi-GAN generator (csrc/hifigan_ops.hip; inference, f32; additions, the ABI version stays) ----
 * Rows are samples, channels-last: a tensor of a stage with `mult` rows per mel frame is [B][Lmax mult][C]; frame_lengths [B] i32 (device) are the
 * utterances' frame counts L <= Lmax, an utterance owns rows [0, L mult) of its slab and only those are read or written (the waveform is zero beyond them):
 * a tap outside them reads zero, padded rows are never written.  Every value depends on its own utterance and a fixed summation order only (no atomics, no
 * workgroup waits on another).  All matrix products: v_mfma_f32_16x16x4_f32, against K-major weight images w [taps Cin][Cout], row = tap * Cin + input
 * channel (a Conv1d weight [Cout][Cin][taps] permuted (2, 1, 0); a ConvTranspose1d weight [Cin][Cout][taps] permuted (2, 0, 1)); bias [Cout].
 * slope is the LeakyReLU applied to the input rows as they are gathered (x > 0 ? x : x slope; 1.0f: none).
 * Supported (glowtts_hifigan_supported(Cin, Cout, taps, dilation, rate), else GLOWTTS_E_ARG before any launch): Cin a multiple of 4 and Cout a multiple of 16,
 * both <= 512; rate == 0, a convolution: taps odd <= 11, dilation in [1, 16] (Cout == 1: the conv_post form, dilation 1); rate >= 1, a transposed
 * convolution: rate <= 16, rate <= taps <= 64, taps - rate even, at most 8 taps per phase, dilation 1.  1 <= B <= 65535, output rows Lmax mult (rate) <= 2^30.
 * glowtts_hifigan_conv: y = conv(lrelu(in)) + bias, zero padding (taps - 1) / 2 * dilation, then + residual (NULL: none; may be `out`), then
 *   out = y (accumulate 0), out = out + y (1: the MRF sum) or out = (out + y) / divisor (2: the last block of a stage).  in != out.  channels_first != 0:
 *   `in` is [B][Cin][Lmax mult] (the mel as the caller holds it).  One launch, logged as `hifigan_conv`.
 * glowtts_hifigan_upsample: the transposed convolution of stride `rate` and padding (taps - rate) / 2 in polyphase form: in [B][Lmax mult][Cin] ->
 *   out [B][Lmax mult rate][Cout], exactly `rate` rows per input row; output row t sums the taps j with (t + p - j) % rate == 0 of input row
 *   (t + p - j) / rate.  One launch, logged as `hifigan_upsample`.
 * glowtts_hifigan_post: wav [B][Lmax mult] = tanh(conv(lrelu(in)) + bias[0]) with w [taps Cin], a fixed-order sum per row.  Logged as `hifigan_conv,post`. */
int glowtts_hifigan_supported(int Cin, int Cout, int taps, int dilation, int rate);
int glowtts_hifigan_conv(const float *in, const float *w, const float *bias, const float *residual, float *out, const int32_t *frame_lengths, int B,
                         int Lmax, int mult, int Cin, int Cout, int taps, int dilation, float slope, int accumulate, float divisor, int channels_first,
                         void *stream);
int glowtts_hifigan_upsample(const float *in, const float *w, const float *bias, float *out, const int32_t *frame_lengths, int B, int Lmax, int mult,
                             int Cin, int Cout, int taps, int rate, float slope, void *stream);
int glowtts_hifigan_post(const float *in, const float *w, const float *bias, float *wav, const int32_t *frame_lengths, int B, int Lmax, int mult, int Cin,
                         int taps, float slope, void *stream);

/* ---- neural vocoder: HiFi-GAN generator, fp16 inference mode (csrc/hifigan_f16_ops.hip; additions, the ABI version stays) ----
 * glowtts_hifigan_conv_f16 / glowtts_hifigan_upsample_f16 are glowtts_hifigan_conv / glowtts_hifigan_upsample with fp16 operands on
 * v_mfma_f32_16x16x32_f16, logged as `hifigan_conv_f16` / `hifigan_upsample_f16`: the staged rows after the LeakyReLU and the weights are clamped to +-65504
 * and rounded to fp16 (nearest even); the sums (which start at the fp32 bias), the residual (which adds the unrounded row), the accumulate epilogues and
 * every tensor in memory stay f32.  Arguments, rows, lengths, ownership and bit-identity as for the f32 entries; conv_post stays glowtts_hifigan_post.
 * The weights come as packed fp16 images [taps][Cp / 8][Cout][8] - element (tap, k, n) at ((tap Cp / 8 + k / 8) Cout + n) 8 + k % 8, Cp = Cin rounded up to
 * a multiple of 32, zero rows from Cin to Cp; tap and k as the rows tap * Cin + k of the f32 image.
 * Supported (glowtts_hifigan_supported_f16, else GLOWTTS_E_ARG before any launch): glowtts_hifigan_supported with the fp16 tile
 * (64 + reach) (min(Cp, 64) + 8) 2 bytes of LDS in place of the f32 tile (Cout == 1: the f32 answer, conv_post has no fp16 form). */
int glowtts_hifigan_supported_f16(int Cin, int Cout, int taps, int dilation, int rate);
int glowtts_hifigan_conv_f16(const float *in, const uint16_t *w, const float *bias, const float *residual, float *out, const int32_t *frame_lengths, int B,
                             int Lmax, int mult, int Cin, int Cout, int taps, int dilation, float slope, int accumulate, float divisor, int channels_first,
                             void *stream);
int glowtts_hifigan_upsample_f16(const float *in, const uint16_t *w, const float *bias, float *out, const int32_t *frame_lengths, int B, int Lmax, int mult,
                                 int Cin, int Cout, int taps, int rate, float slope, void *stream);

/* ---- training the HiFi-GAN generator (csrc/hifigan_train_ops.hip; f32; additions, the ABI version stays) ----
 * Layouts, lengths and ownership as above: nothing is read beyond an utterance's rows [0, L mult) and nothing is written there.  Every product runs on
 * v_mfma_f32_16x16x4_f32, every sum has a fixed order that depends on the sizes alone (no float atomics): every gradient is bit-identical from run to run.
 * Cin, Cout, taps, dilation, rate always name the FORWARD convolution.  Supported: glowtts_hifigan_train_supported(Cin, Cout, taps, dilation, rate) -
 * glowtts_hifigan_supported, and for rate >= 1 Cin a multiple of 16, rate Cout <= 4096 and at most 11 row offsets; else GLOWTTS_E_ARG before any launch.
 * glowtts_hifigan_conv_bwd: the data gradient of glowtts_hifigan_conv, one launch logged as `hifigan_conv_bwd`: dy [B][Lmax mult][Cout] against the
 *   tap-reversed, channel-transposed image wt [taps Cout][Cin] (row = (taps - 1 - tap) Cout + output channel), then
 *   y = sum * (x > 0 ? 1 : mask_slope) * scale + residual * res_scale with x [B][Lmax mult][Cin] the forward's input before its LeakyReLU and residual
 *   (NULL: none; may be `out`) laid out as out [B][Lmax mult][Cin]; out = y (accumulate 0) or out = out + y (1).  Cin a multiple of 16; dy != out.
 * glowtts_hifigan_upsample_bwd: the data gradient of glowtts_hifigan_upsample, one launch logged as `hifigan_upsample_bwd`: dy [B][Lmax mult rate][Cout] read
 *   as [B][Lmax mult][rate Cout], an (hi - lo + 1)-tap convolution over rows against wt [(hi - lo + 1) rate Cout][Cin]: row (e - lo) rate Cout + ph Cout + co
 *   holds W[ci][co][j0 + (e + o0) rate] (j0 = (ph + p) % rate, o0 = (ph + p) / rate, p = (taps - rate) / 2) where that tap exists, else zero; [lo, hi] is the
 *   range of e = m - o0 over the phases' taps m.  out [B][Lmax mult][Cin] = sum * (x > 0 ? 1 : mask_slope).
 * glowtts_hifigan_post_bwd: dpre [B][Lmax mult] = dwav (1 - wav^2) and dx [B][Lmax mult][Cin] = (x > 0 ? 1 : slope) * sum over the taps of w dpre (w [taps Cin]
 *   as glowtts_hifigan_post takes it), a fixed-order sum per element.  Logged as `hifigan_post_bwd`.
 * glowtts_hifigan_wgrad: dw and dbias of one convolution (rate 0: x [B][Lmax mult][Cin], channels_first [B][Cin][Lmax mult]; dy [B][Lmax mult][Cout];
 *   dw [Cout][Cin][taps]; Cout == 1: the conv_post form) or transposed convolution (rate >= 1: dy [B][Lmax mult rate][Cout]; dw [Cin][Cout][taps]) in torch's
 *   layouts, both times `scale`: the sum over the utterances' rows of lrelu(x, slope) dy.  Partition: per utterance chunks of 1024 rows, consecutive
 *   (utterance, chunk) units grouped by 1024 / (Lmax mult) when that exceeds 1, partial sums added in ascending order.  work: at least
 *   glowtts_hifigan_wgrad_work_floats(...) floats.  Two launches, logged as `hifigan_wgrad` and `hifigan_wgrad_sum`. */
int glowtts_hifigan_train_supported(int Cin, int Cout, int taps, int dilation, int rate);
int64_t glowtts_hifigan_wgrad_work_floats(int B, int Lmax, int mult, int Cin, int Cout, int taps, int rate);
int glowtts_hifigan_conv_bwd(const float *dy, const float *wt, const float *x, const float *residual, float *out, const int32_t *frame_lengths, int B,
                             int Lmax, int mult, int Cin, int Cout, int taps, int dilation, float mask_slope, float scale, float res_scale, int accumulate,
                             void *stream);
int glowtts_hifigan_upsample_bwd(const float *dy, const float *wt, const float *x, float *out, const int32_t *frame_lengths, int B, int Lmax, int mult,
                                 int Cin, int Cout, int taps, int rate, float mask_slope, void *stream);
int glowtts_hifigan_post_bwd(const float *dwav, const float *wav, const float *x, const float *w, float *dpre, float *dx, const int32_t *frame_lengths,
                             int B, int Lmax, int mult, int Cin, int taps, float slope, void *stream);
int glowtts_hifigan_wgrad(const float *x, const float *dy, const int32_t *frame_lengths, float *work, float *dw, float *dbias, int B, int Lmax, int mult,
                          int Cin, int Cout, int taps, int dilation, int rate, float slope, float scale, int channels_first, void *stream);

/* ---- training the HiFi-GAN generator in mixed precision (csrc/hifigan_mixed_ops.hip; additions, the ABI version stays) ----
 * The forward of the mode is the fp16 inference forward (glowtts_hifigan_conv_f16 / _upsample_f16 / glowtts_hifigan_post); these are the backward's matrix
 * products on v_mfma_f32_16x16x32_bf16 with fp32 sums.  Every tensor in memory stays f32; arguments, rows, lengths, ownership, epilogues, the partition of the
 * weight gradient and its work buffer (glowtts_hifigan_wgrad_work_floats) are those of the f32 entries above.  Operands are rounded to bf16, nearest even, no
 * clamp; run-to-run and batch-independent bit-identity as for the f32 entries.
 * Supported (glowtts_hifigan_train_supported_mixed, else GLOWTTS_E_ARG before any launch): glowtts_hifigan_train_supported and glowtts_hifigan_supported_f16
 * with the 16-bit tiles' LDS terms; Cout == 1 (conv_post) answers for the f32 launches that serve it.
 * glowtts_hifigan_conv_bwd_bf16: glowtts_hifigan_conv_bwd, logged as `hifigan_conv_bwd_bf16`; dy is rounded as it lies in memory (before `scale`); wt is the
 *   bf16 image [taps][pad32(Cout) / 8][Cin][8] of the tap-reversed, channel-transposed weights (element (tap, k, n) at ((tap Kp / 8 + k / 8) Cin + n) 8 + k % 8).
 * glowtts_hifigan_upsample_bwd_bf16: glowtts_hifigan_upsample_bwd, logged as `hifigan_upsample_bwd_bf16`; wt is the bf16 image
 *   [offsets][pad32(rate Cout) / 8][Cin][8] of the view's image with its zero rows.
 * glowtts_hifigan_wgrad_bf16: glowtts_hifigan_wgrad with lrelu(x) and dy rounded to bf16, logged as `hifigan_wgrad_bf16` and `hifigan_wgrad_sum`; the bias
 *   gradient is the column sum of the unrounded dy, in double.  Cout == 1 runs glowtts_hifigan_wgrad itself (logged as `hifigan_wgrad`).
 * glowtts_hifigan_pack_images: ONE launch, logged as `hifigan_pack_images`, builds weight images from fp32 master weights through a DEVICE job table of
 *   njobs x 8 int64: source, destination, kind, Cin, Cout, taps, rate (of the forward convolution), first block; total_blocks = the jobs' blocks of 256
 *   16-byte groups (kind 4: floats), first blocks ascending from 0.  Kinds: 0 / 1 the fp16 forward image of a Conv1d / ConvTranspose1d weight
 *   ([taps][pad32(Cin) / 8][Cout][8], clamped to +-65504), 2 / 3 the bf16 data-gradient images above, 4 conv_post's f32 [taps][Cin] rows. */
int glowtts_hifigan_train_supported_mixed(int Cin, int Cout, int taps, int dilation, int rate);
int glowtts_hifigan_conv_bwd_bf16(const float *dy, const uint16_t *wt, const float *x, const float *residual, float *out, const int32_t *frame_lengths, int B,
                                  int Lmax, int mult, int Cin, int Cout, int taps, int dilation, float mask_slope, float scale, float res_scale, int accumulate,
                                  void *stream);
int glowtts_hifigan_upsample_bwd_bf16(const float *dy, const uint16_t *wt, const float *x, float *out, const int32_t *frame_lengths, int B, int Lmax, int mult,
                                      int Cin, int Cout, int taps, int rate, float mask_slope, void *stream);
int glowtts_hifigan_wgrad_bf16(const float *x, const float *dy, const int32_t *frame_lengths, float *work, float *dw, float *dbias, int B, int Lmax, int mult,
                               int Cin, int Cout, int taps, int dilation, int rate, float slope, float scale, int channels_first, void *stream);
int glowtts_hifigan_pack_images(const int64_t *jobs, int njobs, int total_blocks, void *stream);

/* ---- GE2E speaker encoder: stacked LSTM -> linear -> d-vector (csrc/ge2e_ops.hip; inference, f32; additions, the ABI version stays) ----
 * torch.nn.LSTM's definition (gates i, f, g, o; bias b_ih + b_hh; h0 = c0 = 0), then e = W h_{T-1}^{top} + b per slice, w = e / max(|e|, 1e-12),
 * d = normalize(mean over an utterance's Samples consecutive slices of w).  Every product runs on v_mfma_f32_16x16x4_f32; a sequence's values depend on
 * that sequence and a fixed summation order only (bit-identical alone and in any batch).  No kernel waits on another workgroup.
 * Supported (glowtts_ge2e_supported, else GLOWTTS_E_ARG): Mel a multiple of 4, <= GLOWTTS_GE2E_MAX_MEL; H a multiple of 16, <= GLOWTTS_GE2E_MAX_H;
 * 1 <= Stacks <= GLOWTTS_GE2E_MAX_STACKS; 1 <= E <= GLOWTTS_GE2E_MAX_E; T >= 1 (<= 2^20); N >= 1 a multiple of Samples, N <= 16 * 65535.
 * Layouts (all f32, device):
 *   x       [N][Mel][T]                 the slice stack, channels first (read in place)
 *   images  glowtts_ge2e_image_floats() floats: layer 0 [Mel + H][4 H], then layers 1.. [2 H][4 H] each; K-major: rows are the layer's input channels
 *           followed by its own hidden units (W_ih | W_hh as one K range); column 64 s + 4 u + g holds gate g (i, f, g, o) of hidden unit 16 s + u
 *   biases  [Stacks][4 H], b_ih + b_hh in the images' column order
 *   head_w  [E][H], head_b [E]          torch.nn.Linear's own tensors
 *   work    glowtts_ge2e_work_floats(N, T, H, Stacks) = Stacks N H (T + 1) floats: c [Stacks][N][H] (updated in place), then the hidden states; with hs
 *           given they go there instead and the first Stacks N H floats suffice
 *   hs      [Stacks][N][T][H] or NULL   all hidden states (tests); e [N][E] or NULL: the raw embeddings; d [N / Samples][E]: unit-norm d-vectors
 * glowtts_ge2e_pack packs ONE layer's torch tensors (w_ih [4 H][in], w_hh [4 H][H], b_ih, b_hh [4 H]) into its place in images / biases: call it once
 * per layer at load and again only when the parameters change.  Logged as `ge2e_pack`.
 * glowtts_ge2e_forward allocates nothing and takes only pointers and a stream: T + Stacks - 1 launches `ge2e_cell` (launch d: every cell
 * (layer k, step d - k), which reads only what launch d - 1 wrote; grid (H / 16, ceil(N / 16), cells on the diagonal)) and one `ge2e_head`. */
#define GLOWTTS_GE2E_MAX_MEL 512
#define GLOWTTS_GE2E_MAX_H 768
#define GLOWTTS_GE2E_MAX_STACKS 8
#define GLOWTTS_GE2E_MAX_E 1024
int glowtts_ge2e_supported(int Mel, int H, int Stacks, int E);
int64_t glowtts_ge2e_image_floats(int Mel, int H, int Stacks);
int64_t glowtts_ge2e_work_floats(int64_t N, int T, int H, int Stacks);
int glowtts_ge2e_pack(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, float *images, float *biases, int layer, int Mel, int H,
                      int Stacks, void *stream);
int glowtts_ge2e_forward(const float *x, const float *images, const float *biases, const float *head_w, const float *head_b, float *work, float *hs,
                         float *e, float *d, int N, int Samples, int Mel, int T, int H, int Stacks, int E, void *stream);

/* ---- Training the GE2E speaker encoder (csrc/ge2e_train_ops.hip; f32; additions, the ABI version stays) ----
 * The forward's rules hold: launch order on the stream is the only synchronisation, no float atomics, every sum has a fixed partition and order (every
 * result is bit-identical from run to run), the stack's products run on v_mfma_f32_16x16x4_f32.  None of these functions allocates.
 * Layouts (all f32, device; N, Mel, T, H, Stacks, E, x, images, biases, head_w, head_b as for glowtts_ge2e_forward; N T < 2^31):
 *   keep      glowtts_ge2e_train_keep_floats() = 6 Stacks N T H floats: hs [Stacks][N][T][H] | c [Stacks][N][T][H] | the activated gates
 *             [Stacks][N][T][4 H] in the images' column order (column 64 s + 4 u + g: gate g (i, f, g, o) of hidden unit 16 s + u)
 *   images_t  glowtts_ge2e_train_image_floats() = (8 Stacks - 4) H H floats: layer k at 8 k H H: W_hh^k as [4 H][H] with the rows in that column order,
 *             then (all layers but the top one) W_ih^{k+1} likewise
 *   da        [Stacks][N][T][4 H]: the gradients of the pre-activations, in the same column order
 *   work      glowtts_ge2e_train_work_floats(): scratch shared by glowtts_ge2e_train_backward and glowtts_ge2e_train_wgrad
 *   loss work glowtts_ge2e_train_loss_work_floats(N, S, E)
 * glowtts_ge2e_train_pack    `ge2e_pack_bwd`: one layer's part of images_t from w_hh [4 H][H] of that layer and w_ih [4 H][H] of the layer above (NULL for
 *                            the top layer, and only for it); call it whenever glowtts_ge2e_pack is called.
 * glowtts_ge2e_train_forward T + Stacks - 1 `ge2e_cell` (the inference forward's arithmetic in its order: hs and e are bit-identical to
 *                            glowtts_ge2e_forward's) and one `ge2e_head_fwd`: e [N][E].
 * glowtts_ge2e_train_loss    the GE2E softmax loss over e [S M][E], row j M + i = speaker j's utterance i (S >= 2, M >= 2): u = e / max(|e|, 1e-12),
 *                            s_{ji,k} = w cos(u_ji, c_k) with c_k the mean of speaker k's u and, for k = j, the mean without u_ji,
 *                            L = mean_ji [logsumexp_k s_{ji,k} - s_{ji,j}].  w: one device float.  Writes loss [1], de [N][E], dw [1].
 *                            `ge2e_loss_norm`, `_centroid`, `_scores`, `_dcent`, `_du`, `_final`.
 * glowtts_ge2e_train_backward `ge2e_head_bwd` (dhead_w [E][H], dhead_b [E], the top layer's dh) and T + Stacks - 1 `ge2e_cell_bwd` (launch d, descending: every
 *                            cell (layer k, step d - k)); fills da.  The gradient of x is not computed.
 * glowtts_ge2e_train_wgrad   two `ge2e_wgrad` launches for ONE layer, after glowtts_ge2e_train_backward: dw_ih [4 H][in], dw_hh [4 H][H],
 *                            db_ih = db_hh [4 H] in torch's row order (overwritten, not accumulated). */
int64_t glowtts_ge2e_train_image_floats(int H, int Stacks);
int64_t glowtts_ge2e_train_keep_floats(int64_t N, int T, int H, int Stacks);
int64_t glowtts_ge2e_train_loss_work_floats(int64_t N, int S, int E);
int64_t glowtts_ge2e_train_work_floats(int64_t N, int T, int Mel, int H, int Stacks);
int glowtts_ge2e_train_pack(const float *w_hh, const float *w_ih_next, float *images_t, int layer, int H, int Stacks, void *stream);
int glowtts_ge2e_train_forward(const float *x, const float *images, const float *biases, const float *head_w, const float *head_b, float *keep, float *e,
                               int N, int Mel, int T, int H, int Stacks, int E, void *stream);
int glowtts_ge2e_train_loss(const float *e, const float *w, float *work, float *loss, float *de, float *dw, int S, int M, int E, void *stream);
int glowtts_ge2e_train_backward(const float *images_t, const float *keep, const float *head_w, const float *de, float *da, float *work, float *dhead_w,
                                float *dhead_b, int N, int T, int H, int Stacks, int E, void *stream);
int glowtts_ge2e_train_wgrad(const float *x, const float *keep, const float *da, float *work, float *dw_ih, float *dw_hh, float *db_ih, float *db_hh,
                             int layer, int N, int Mel, int T, int H, int Stacks, void *stream);

/* ---- Training the Parallel WaveGAN generator (csrc/pwg_train_ops.hip; f32; additions, the ABI version stays) ----
 * The training forward is the inference forward: the glowtts_pwg_* entry points above, with every layer's input x kept in its own slab (layer i reads
 * slab i and writes slab i + 1), so the waveform is bit-identical.  The gate is recomputed here.  Rows, lengths and layouts as for glowtts_pwg_layer; nothing
 * beyond an utterance's own rows is read or written.  No float atomics, no kernel waits on another workgroup, fixed partitions and orders: every gradient
 * is bit-identical from run to run.  All matrix products: v_mfma_f32_16x16x4_f32.  None of these functions allocates.  The gradient of the mel is not computed.
 * Supported (glowtts_pwg_train_supported, else GLOWTTS_E_ARG): glowtts_pwg_supported, and the backward's LDS tiles within 160 KB:
 * 64 (stride(3 R + A) + R + S + 4) floats (gate launch) and 64 (6 R + 4) floats (data launch); B * ceil(Lmax hop / 1024) <= 65535.
 *   work   glowtts_pwg_train_work_floats() floats, 8-byte aligned: the weight gradients' splits (one per utterance and 1024 rows), the FIR gradient's block sums
 * glowtts_pwg_train_head_bwd    `pwg_head_bwd`: skips, dwav [B][Lmax hop] -> dskips [B][Lmax hop][S] (the same tensor for every layer) and, for the weight
 *                               gradients, y = relu(scale skips), h = relu(W1 y + b1), dh, all [B][Lmax hop][S].  w1 [S][S] row = input channel (the forward's
 *                               image), w1t [S][S] row = output channel (torch's tensor).
 * glowtts_pwg_train_head_wgrad  `pwg_wgrad` + `pwg_wgrad_sum`: dw1 [S][S] (torch's [out][in]), db1 [S], dw2 [S], db2 [1]; overwritten.
 * glowtts_pwg_train_layer_bwd   `pwg_layer_bwd_gate` (recomputes the gate from x, c, w1, b1; dgate = [sqrt(1/2) dxp | dskips] w2t^T-wise, w2t [R + S][R] =
 *                               the forward's w2 transposed; writes gate [B][Lmax hop][R] and dpre [B][Lmax hop][2 R]) and `pwg_layer_bwd_data`
 *                               (dx = sqrt(1/2) dxp + sum over the taps of dpre(t -+ d) W1_tap^T, w1t [3 * 2 R][R]: row = tap * 2 R + gate column;
 *                               dc (+)= dpre wauxt, wauxt [2 R][A]; first != 0 overwrites dc).  dxp: the gradient of the layer's output x', dx: of its input.
 * glowtts_pwg_train_layer_wgrad `pwg_wgrad` + `pwg_wgrad_sum` for ONE layer, after glowtts_pwg_train_layer_bwd: conv.weight [2 R][R][3], conv.bias [2 R],
 *                               conv1x1_aux.weight [2 R][A], conv1x1_out.weight [R][R], .bias [R], conv1x1_skip.weight [S][R], .bias [S] in torch's layouts;
 *                               overwritten.
 * glowtts_pwg_train_first_bwd   `pwg_first_bwd` + `pwg_wgrad_sum`: first_conv's dw [R], db [R] from dx0 and z (noises or seeds as for glowtts_pwg_first).
 * glowtts_pwg_train_upsample_bwd `pwg_upsample_bwd`, `pwg_upsample_bwd_fir` and `pwg_upsample_bwd_sum` for ONE scale s: dout [B][Lmax mult s][A], the stage's input in
 *                               [B][Lmax mult][A], fir [2 s + 1] -> din [B][Lmax mult][A], dfir [2 s + 1].
 * glowtts_pwg_train_cond_in_bwd `pwg_cond_in_bwd`: mel [B][A][Lmax], dcond [B][Lmax][A] -> dw [A][A][2 ctx + 1] (torch's layout). */
int glowtts_pwg_train_supported(int R, int S, int A, int max_dilation);
int64_t glowtts_pwg_train_work_floats(int B, int Lmax, int hop, int R, int S, int A);
int glowtts_pwg_train_head_bwd(const float *skips, const int32_t *frame_lengths, const float *w1, const float *w1t, const float *b1, const float *w2,
                               const float *dwav, float *y, float *h, float *dh, float *dskips, int B, int Lmax, int hop, int S, float scale, void *stream);
int glowtts_pwg_train_head_wgrad(const float *y, const float *h, const float *dh, const float *dwav, const int32_t *frame_lengths, float *work, float *dw1,
                                 float *db1, float *dw2, float *db2, int B, int Lmax, int hop, int S, void *stream);
int glowtts_pwg_train_layer_bwd(const float *x, const float *c, const float *w1, const float *b1, const float *w2t, const float *w1t, const float *wauxt,
                                const float *dxp, const float *dskips, float *gate, float *dpre, float *dx, float *dc, const int32_t *frame_lengths, int B,
                                int Lmax, int hop, int R, int S, int A, int dilation, int first, void *stream);
int glowtts_pwg_train_layer_wgrad(const float *x, const float *c, const float *gate, const float *dpre, const float *dxp, const float *dskips,
                                  const int32_t *frame_lengths, float *work, float *dconv_w, float *dconv_b, float *daux_w, float *dout_w, float *dout_b,
                                  float *dskip_w, float *dskip_b, int B, int Lmax, int hop, int R, int S, int A, int dilation, void *stream);
int glowtts_pwg_train_first_bwd(const float *noises, const uint32_t *seeds, const float *dx0, const int32_t *frame_lengths, float *work, float *dw, float *db,
                                int B, int Lmax, int hop, int R, void *stream);
int glowtts_pwg_train_upsample_bwd(const float *dout, const float *in, const float *fir, const int32_t *frame_lengths, float *work, float *din, float *dfir,
                                   int B, int A, int Lmax, int mult, int s, void *stream);
int glowtts_pwg_train_cond_in_bwd(const float *mel, const float *dcond, const int32_t *frame_lengths, float *dw, int B, int A, int Lmax, int ctx, void *stream);

/* ---- Multi-resolution STFT loss of vocoder training (csrc/stft_loss_ops.hip; f32 signals, float64 sums; additions, the ABI version stays) ----
 * ONE resolution (n_fft, hop, win_length) per call; vocoder.MultiResolutionSTFTLoss calls once per resolution.  pred, target [B][T], every row of the full
 * length T.  X = STFT with center = True, reflect padding by n_fft / 2, the periodic Hann window of win_length centred in n_fft (the tables of
 * glowtts_stft_f32), NF = 1 + T / hop frames, F = n_fft / 2 + 1 bins;  |X| = sqrt(max(re^2 + im^2, 1e-7));  L_sc = ||Y| - |X||_F / ||Y||_F over the whole
 * batch, L_mag = mean |log |Y| - log |X||  (Y: target, X: pred).  No atomics, fixed summation orders: bit-identical from run to run.
 * Supported (glowtts_stft_loss_supported, else GLOWTTS_E_ARG): n_fft a power of two in [256, 4096], 1 <= hop <= win_length <= n_fft,
 * n_fft / 2 < T <= 2^29; also 1 <= B <= 65535, B T < 2^31, B NF <= 2^24.  None of these functions allocates.
 *   keep   glowtts_stft_loss_keep_floats() = 4 B NF F floats (8-byte aligned): pred's spectrum [B NF][F][2] | |X| [B NF][F] | |Y| [B NF][F]
 *   work   glowtts_stft_loss_work_floats() = B NF (6 + win_length) floats (8-byte aligned): per-frame sums [B NF][3] f64 | the backward's windowed
 *          frame gradients [B NF][win_length]
 *   terms  [3]: L_sc, L_mag and the backward's coefficient 1 / (||Y| - |X||_F ||Y||_F) (0 when the magnitudes are equal)
 * glowtts_stft_loss_forward   `stft_loss_fwd` (per frame: both signals through the LDS FFT, magnitudes and pred's spectrum into keep, the frame's sums)
 *                             and `stft_loss_reduce` (one workgroup): fills terms and loss[0] = weight (L_sc + L_mag), added to loss[0] when accumulate.
 * glowtts_stft_loss_backward  `stft_loss_bwd_frames` (per frame: dL/d|X| in closed form times X / |X|, zero where the clamp is active, the transposed real
 *                             DFT in LDS, the window) and `stft_loss_bwd_fold` (per sample: gather of the ceil(win_length / hop) covering frames in ascending
 *                             order at the sample's own padded position and the at most two that reflect onto it):
 *                             dpred [B][T] = grad_out[0] weight dL/dpred (grad_out: one device float), added to dpred when accumulate. */
int glowtts_stft_loss_supported(int n_fft, int win_length, int hop, int T);
int64_t glowtts_stft_loss_keep_floats(int B, int T, int n_fft, int hop);
int64_t glowtts_stft_loss_work_floats(int B, int T, int win_length, int hop);
int glowtts_stft_loss_forward(const float *pred, const float *target, const float *window, const float *twiddle, float *keep, float *work, float *terms,
                              float *loss, int B, int T, int n_fft, int win_length, int hop, float weight, int accumulate, void *stream);
int glowtts_stft_loss_backward(const float *keep, const float *terms, const float *grad_out, const float *window, const float *twiddle, float *work,
                               float *dpred, int B, int T, int n_fft, int win_length, int hop, float weight, int accumulate, void *stream);

/* ---- Mel-spectrogram L1 loss of vocoder training (csrc/mel_loss_ops.hip; f32 signals, float64 sums; additions, the ABI version stays) ----
 * ONE analysis geometry per call.  pred, target [B][T], every row of the full length T, framed exactly as the STFT loss above frames them (NF = 1 + T / hop
 * frames, F = n_fft / 2 + 1 bins, the same window and twiddle tables).  Per frame and filter j:  |X|[k] = sqrt(re^2 + im^2 + 1e-9);
 * mel[j] = sum_k fb[j, k] |X|[k] in ascending bin order;  m[j] = ln(max(mel[j], floor));  L_mel = mean over (B, NF, n_mel) of |m_target - m_pred|.
 * No atomics, fixed summation orders: bit-identical from run to run.
 * The filterbank is sparse, one run of bins per filter: fb_index [n_mel][3] = (first bin, bin count, offset into fb_weights), fb_weights [n_weights]
 * (frontend.sparse_filterbank); the backward reads its transpose in CSR form, bin k's entries fbt_start[k] .. fbt_start[k + 1] (fbt_start [F + 1]) with
 * their filters fbt_filter [n_weights] in ascending order and weights fbt_weights [n_weights].  The kernels hold every table index to the tables' sizes; a
 * filter without bins contributes ln(floor) on both sides, the callers refuse it.
 * Supported (glowtts_mel_loss_supported, else GLOWTTS_E_ARG): what glowtts_stft_loss_supported takes and 4 <= n_mel <= 256; also 1 <= B <= 65535,
 * B T < 2^31, B NF <= 2^24, 1 <= n_weights <= n_mel F, floor > 0.  None of these functions allocates.
 *   keep   glowtts_mel_loss_keep_floats() = B NF n_mel floats: c[j] = sign(m_pred - m_target) / mel_pred, 0 at equality and where mel_pred <= floor
 *   work   glowtts_mel_loss_work_floats() = B NF (2 + win_length) floats (8-byte aligned): per-frame sums [B NF] f64 | the backward's windowed frame
 *          gradients [B NF][win_length]
 *   terms  [1]: L_mel
 * glowtts_mel_loss_forward   `mel_loss_fwd` (per frame: both signals through the LDS FFT, magnitudes and filter sums in LDS, c into keep, the frame's sum)
 *                            and `mel_loss_reduce` (one workgroup): fills terms and loss[0] = weight L_mel, added to loss[0] when accumulate.
 * glowtts_mel_loss_backward  `mel_loss_bwd_frames` (per frame: pred's spectrum again, G[k] = grad_out[0] weight / (B NF n_mel) (sum_j fb[j, k] c[j])
 *                            X[k] / |X|[k], the transposed real DFT in LDS, the window) and `mel_loss_bwd_fold` (the STFT loss's fold):
 *                            dpred [B][T] = grad_out[0] weight dL_mel/dpred (grad_out: one device float), added to dpred when accumulate.  pred is the
 *                            forward's, unchanged. */
int glowtts_mel_loss_supported(int n_fft, int win_length, int hop, int T, int n_mel);
int64_t glowtts_mel_loss_keep_floats(int B, int T, int hop, int n_mel);
int64_t glowtts_mel_loss_work_floats(int B, int T, int win_length, int hop);
int glowtts_mel_loss_forward(const float *pred, const float *target, const float *window, const float *twiddle, const int32_t *fb_index,
                             const float *fb_weights, float *keep, float *work, float *terms, float *loss, int B, int T, int n_fft, int win_length,
                             int hop, int n_mel, int n_weights, float floor, float weight, int accumulate, void *stream);
int glowtts_mel_loss_backward(const float *pred, const float *keep, const float *grad_out, const float *window, const float *twiddle,
                              const int32_t *fbt_start, const int32_t *fbt_filter, const float *fbt_weights, float *work, float *dpred, int B, int T,
                              int n_fft, int win_length, int hop, int n_mel, int n_weights, float weight, int accumulate, void *stream);

/* ---- The Parallel WaveGAN discriminator and the adversarial loss (csrc/pwg_disc_ops.hip; f32; additions, the ABI version stays) ----
 * `layers` 1-D convolutions of kernel size 3 over wav [B][T], "same" zero padding, bias, LeakyReLU(slope) after all but the last: 1 -> C (dilation 1),
 * C -> C with dilation i for i = 1 .. layers - 2, C -> 1 (dilation 1).  Activations are rows [B][T][C]; EVERY batch row is of the full length T, tiles are
 * counted from a row's own sample 0 and every tap is masked by the row's own [0, T): a row's result does not depend on the batch around it, and nothing
 * beyond the B T rows is read or written.  Matrix products: v_mfma_f32_16x16x4_f32.  No float atomics, fixed partitions and orders: bit-identical from run
 * to run.  None of these functions allocates.
 * Supported (glowtts_pwg_disc_supported, else GLOWTTS_E_ARG): C a multiple of 16 in [16, 256] whose tile of 64 stride(3 C) floats fits 160 KB (C <= 208),
 * 3 <= layers <= 16, dilation in [1, 1024]; 1 <= B <= 65535, 1 <= T <= 2^30, B T < 2^31, B ceil(T / 1024) <= 65535.
 *   work   glowtts_pwg_disc_work_floats() floats, 8-byte aligned: the weight gradients' splits (one per batch row and 1024 samples), the loss's block sums
 * glowtts_pwg_disc_first      `pwg_disc_first`: wav -> out [B][T][C]; w [3][C] (row = tap), bias [C].
 * glowtts_pwg_disc_layer      `pwg_disc_layer`: x -> out (out != x), both [B][T][C]; w [3 C][C]: row = tap * C + input channel, column = output channel.
 * glowtts_pwg_disc_last       `pwg_disc_last`: x [B][T][C] -> scores [B][T]; w [3][C] (row = tap), bias [1].
 * glowtts_pwg_disc_mse        `pwg_disc_mse` + `pwg_disc_mse_sum`: p, dp [N]; the scores before `split` (1 <= split <= N) are held against v0, the others
 *                             against v1: m0 = mean (p - v0)^2 over the first part, m1 = mean (p - v1)^2 over the second (0 when split == N), float64 block
 *                             sums added in ascending order; loss [3] = factor (m0 + m1), m0, m1; dp = factor 2 (p - v) / (the size of its part).
 * glowtts_pwg_disc_last_bwd   `pwg_disc_last_bwd`: dp [B][T] -> dh [B][T][C], the gradient of the last hidden layer's output; w as for glowtts_pwg_disc_last.
 * glowtts_pwg_disc_layer_bwd  `pwg_disc_layer_bwd`: dout, out [B][T][C] (the gradient of a middle layer's output, and that output: it carries the LeakyReLU
 *                             mask) -> dx [B][T][C], the gradient of the layer's input (dx != dout); wt [3 C][C]: row = tap * C + output channel, column =
 *                             input channel.  dpre [B][T][C] (or NULL: not wanted) receives dout (out > 0 ? 1 : slope) for the weight gradient (dpre != dout).
 * glowtts_pwg_disc_first_bwd  `pwg_disc_first_bwd`: dout, out of layer 0 -> dwav [B][T]; dpre as above; w as for glowtts_pwg_disc_first.
 * glowtts_pwg_disc_wgrad      `pwg_disc_wgrad` + `pwg_disc_wgrad_sum` (the kernels of glowtts_pwg_train_layer_wgrad) for ONE layer: a [B][T][Cin] its input,
 *                             dpre [B][T][Cout], lengths [B] int32 all equal to T -> dw [Cout][Cin][3], db [Cout] in torch's layouts; overwritten.
 *                             Cin == 1 (the first layer, a = wav) or Cout == 1 (the last, dpre = d scores) or both supported widths. */
int glowtts_pwg_disc_supported(int C, int layers, int max_dilation);
int64_t glowtts_pwg_disc_work_floats(int B, int T, int C);
int glowtts_pwg_disc_first(const float *wav, const float *w, const float *bias, float *out, int B, int T, int C, float slope, void *stream);
int glowtts_pwg_disc_layer(const float *x, const float *w, const float *bias, float *out, int B, int T, int C, int dilation, float slope, void *stream);
int glowtts_pwg_disc_last(const float *x, const float *w, const float *bias, float *scores, int B, int T, int C, void *stream);
int glowtts_pwg_disc_mse(const float *p, float *dp, float *work, float *loss, int64_t N, int64_t split, float v0, float v1, float factor, void *stream);
int glowtts_pwg_disc_last_bwd(const float *dp, const float *w, float *dh, int B, int T, int C, void *stream);
int glowtts_pwg_disc_layer_bwd(const float *dout, const float *out, const float *wt, float *dx, float *dpre, int B, int T, int C, int dilation, float slope,
                               void *stream);
int glowtts_pwg_disc_first_bwd(const float *dout, const float *out, const float *w, float *dwav, float *dpre, int B, int T, int C, float slope, void *stream);
int glowtts_pwg_disc_wgrad(const float *a, const float *dpre, const int32_t *lengths, float *work, float *dw, float *db, int B, int T, int Cin, int Cout,
                           int dilation, void *stream);

/* ---- The HiFi-GAN multi-period discriminator and the feature-matching loss (csrc/hifigan_disc_ops.hip; f32; additions, the ABI version stays) ----
 * One sub-network per period p: wav [B][T] is reflect-padded on the right to H0 p samples, H0 = ceil(T / p) (sample T + j is sample T - 2 - j), and folded to
 * rows (h, c) = (n / p, n % p); convolutions run over h alone: `widths` layers of 5 taps, zero padding 2 and stride 3 (the last: 1), then conv_post with 3
 * taps, width -> 1.  H' = (H - 1) / stride + 1.  Activations are channels-last [B][H p][C] with the flat row n = h p + c and hold PRE-activations: the
 * LeakyReLU is the consumer's prologue and the backward recomputes its mask (1 where pre > 0, the slope elsewhere).  Every batch row is of the full length;
 * a row's result does not depend on the batch around it and nothing beyond the B H p rows is read or written.  Matrix products: v_mfma_f32_16x16x4_f32.
 * No float atomics, fixed partitions and orders: bit-identical from run to run.  None of these functions allocates.
 * Supported (glowtts_hifigan_disc_supported, else GLOWTTS_E_ARG): period in [2, 16]; widths multiples of 16 in [16, 1024] (Cin = 1: the first layer,
 * Cout = 1: conv_post); stride 1 or 3; T >= 2 period; 1 <= B <= 65535, B H p <= 2^30.
 *   work   glowtts_hifigan_disc_work_floats(B, rows_out, Cin, Cout, taps) floats, 8-byte aligned: the weight gradient's splits of a layer with rows_out flat
 *          output rows per batch row (one split per batch row and 1024 rows), and at least the block sums of glowtts_hifigan_disc_fm on that layer's output.
 * glowtts_hifigan_disc_first      `hifigan_disc_first`: wav -> out [B][H1 p][C]; w [5][C] (row = tap), bias [C].
 * glowtts_hifigan_disc_conv       `hifigan_disc_conv`: x [B][H p][Cin] -> out [B][H' p][Cout] = bias + conv(lrelu(x, slope)); w [5 Cin][Cout]: row = tap Cin +
 *                                 input channel.
 * glowtts_hifigan_disc_post       `hifigan_disc_post`: x [B][H p][C] -> scores [B][H p] = bias + conv(lrelu(x, slope)); w [3][C] (row = tap), bias [1].
 * glowtts_hifigan_disc_fm         `hifigan_disc_fm` + `hifigan_disc_fm_sum`: f holds 2 count floats, a feature map of the real rows then of the fake rows;
 *                                 term [1] = mean |lrelu(fake) - lrelu(real)| (slope 1: raw), float64 block sums of 4096 elements added in ascending order;
 *                                 inj [count] = sign(lrelu(fake) - lrelu(real)) lrelu'(fake) / count, sign(0) = 0.  count < 2^30.  total [1] (or NULL):
 *                                 receives the term (accumulate 0) or total + term (accumulate 1): L_fm as the sum of the terms in launch order.
 * glowtts_hifigan_disc_post_bwd   `hifigan_disc_post_bwd`: d = dscores + dscores2 *inj_scale ([B][H p]; dscores2 may be NULL) -> dx [B][H p][C] = lrelu'(x) times
 *                                 the transposed conv_post of d, + inj *inj_scale (inj [B][H p][C] or NULL).  inj_scale: ONE float on the device.
 * glowtts_hifigan_disc_conv_bwd   `hifigan_disc_conv_bwd`: dy [B][H' p][Cout] (d pre of the layer's output), x [B][H p][Cin] (the kept pre-activation of its
 *                                 input) -> dx [B][H p][Cin] = lrelu'(x) times the transposed convolution of dy, + inj *inj_scale; wt [5 Cout][Cin]: row = tap
 *                                 Cout + output channel.
 * glowtts_hifigan_disc_first_bwd  `hifigan_disc_first_bwd`: dpre [B][H1 p][C] of the first layer -> dwav [B][T]: d(padded wav) gathered at t and, where that
 *                                 lies in [T, H0 p), at 2 T - 2 - t; accumulate 1: added to what dwav holds (the periods, in period order).
 * glowtts_hifigan_disc_wgrad      `hifigan_disc_wgrad` + `hifigan_disc_wgrad_sum` (the kernels of glowtts_hifigan_wgrad under the discriminator's row map)
 *                                 for ONE layer with H input rows: x its input (lrelu(x, slope) is formed on the way in), dy [B][H' p][Cout] -> dw
 *                                 [Cout][Cin][taps], dbias [Cout] in torch's layouts; overwritten.  taps 5, or 3 with stride 1 (conv_post).  Cin == 1: x is
 *                                 the waveform [B][wav_samples] itself (slope 1), H = ceil(wav_samples / period); else wav_samples = 0. */
int glowtts_hifigan_disc_supported(int period, int Cin, int Cout);
int64_t glowtts_hifigan_disc_work_floats(int B, int rows_out, int Cin, int Cout, int taps);
int glowtts_hifigan_disc_first(const float *wav, const float *w, const float *bias, float *out, int B, int T, int period, int stride, int C, void *stream);
int glowtts_hifigan_disc_conv(const float *x, const float *w, const float *bias, float *out, int B, int H, int period, int stride, int Cin, int Cout, float slope,
                              void *stream);
int glowtts_hifigan_disc_post(const float *x, const float *w, const float *bias, float *scores, int B, int H, int period, int C, float slope, void *stream);
int glowtts_hifigan_disc_fm(const float *f, float *inj, float *work, float *term, float *total, int64_t count, float slope, int accumulate, void *stream);
int glowtts_hifigan_disc_post_bwd(const float *dscores, const float *dscores2, const float *x, const float *w, const float *inj, const float *inj_scale, float *dx,
                                  int B, int H, int period, int C, float slope, void *stream);
int glowtts_hifigan_disc_conv_bwd(const float *dy, const float *wt, const float *x, const float *inj, const float *inj_scale, float *dx, int B, int H, int period,
                                  int stride, int Cin, int Cout, float slope, void *stream);
int glowtts_hifigan_disc_first_bwd(const float *dpre, const float *w, float *dwav, int B, int T, int period, int stride, int C, int accumulate,
                                   void *stream);
int glowtts_hifigan_disc_wgrad(const float *x, const float *dy, float *work, float *dw, float *dbias, int B, int H, int period, int stride, int Cin, int Cout,
                               int taps, int wav_samples, float slope, void *stream);

/* ---- The bf16 mode of the HiFi-GAN multi-period discriminator (csrc/hifigan_disc_bf16_ops.hip; additions, the ABI version stays) ----
 * The middle convolutions (5 taps, Cin and Cout multiples of 16) with bf16 operands (nearest even, no clamp) on v_mfma_f32_16x16x32_bf16 and fp32 sums, biases
 * and epilogues; the arguments are the f32 entries' with 16-bit images.  Every tensor in memory stays fp32; the first layer, conv_post and the
 * feature-matching loss keep the f32 entries above.  Deterministic; a batch row's results do not depend on the batch.  Bad arguments return GLOWTTS_E_ARG
 * before any launch.
 * Supported (glowtts_hifigan_disc_supported_bf16): glowtts_hifigan_disc_supported with the 16-bit tiles' LDS terms; Cin == 1 and Cout == 1 answer for the f32
 * launches that serve them (the three launches below refuse them).
 * glowtts_hifigan_disc_conv_bf16      glowtts_hifigan_disc_conv, logged as `hifigan_disc_conv_bf16`; w is the bf16 image [5][pad32(Cin) / 8][Cout][8] of the
 *                                     weights [Cout][Cin][5] (element (tap, k, n) at ((tap Kp / 8 + k / 8) Cout + n) 8 + k % 8, zero for k from Cin to Kp):
 *                                     glowtts_hifigan_pack_images kind 5.
 * glowtts_hifigan_disc_conv_bwd_bf16  glowtts_hifigan_disc_conv_bwd, logged as `hifigan_disc_conv_bwd_bf16`; dy is rounded as it lies in memory; wt is the bf16
 *                                     image [5][pad32(Cout) / 8][Cin][8] of the channel-transposed weights, taps NOT reversed: kind 6.
 * glowtts_hifigan_disc_wgrad_bf16     glowtts_hifigan_disc_wgrad with lrelu(x) and dy rounded to bf16, logged as `hifigan_disc_wgrad_bf16` and
 *                                     `hifigan_disc_wgrad_sum`; the bias gradient is the column sum of the unrounded dy, in double.  taps 5 and
 *                                     wav_samples 0 alone; work as glowtts_hifigan_disc_wgrad.
 * glowtts_hifigan_pack_images kinds 5 / 6: the two images above from a Conv weight [Cout][Cin][taps]. */
int glowtts_hifigan_disc_supported_bf16(int period, int Cin, int Cout);
int glowtts_hifigan_disc_conv_bf16(const float *x, const uint16_t *w, const float *bias, float *out, int B, int H, int period, int stride, int Cin, int Cout,
                                   float slope, void *stream);
int glowtts_hifigan_disc_conv_bwd_bf16(const float *dy, const uint16_t *wt, const float *x, const float *inj, const float *inj_scale, float *dx, int B, int H,
                                       int period, int stride, int Cin, int Cout, float slope, void *stream);
int glowtts_hifigan_disc_wgrad_bf16(const float *x, const float *dy, float *work, float *dw, float *dbias, int B, int H, int period, int stride, int Cin, int Cout,
                                    int taps, int wav_samples, float slope, void *stream);

/* ---- The HiFi-GAN multi-scale discriminator (csrc/hifigan_msd_ops.hip, the dense layers in csrc/hifigan_disc_ops.hip; f32; additions, the ABI version stays) ----
 * One sub-network per scale: scale 0 sees wav [B][T], scale i the waveform after i average pools (4 taps, stride 2, zero padding 2, always divided by 4:
 * T' = T / 2 + 1).  A sub-network is a stack of Conv1d over time with zero padding taps / 2 and L' = (L - 1) / stride + 1: a first layer 1 -> C0 (stride 1), grouped
 * strided middle layers, a dense last layer (5 taps, stride 1) and conv_post (3 taps, width -> 1).  Activations are channels-last [B][L][C] and hold
 * PRE-activations: the LeakyReLU is the consumer's prologue and the backward recomputes its mask (1 where pre > 0, the slope elsewhere).  Every batch row is of
 * the full length; a row's result does not depend on the batch around it and nothing beyond the B L rows is read or written.  Matrix products:
 * v_mfma_f32_16x16x4_f32.  No float atomics, fixed partitions and orders: bit-identical from run to run.  None of these functions allocates.  The feature-matching
 * loss of a map is glowtts_hifigan_disc_fm, which knows no layout.
 * Supported (glowtts_hifigan_msd_supported(Cin, Cout, taps, stride, groups), else GLOWTTS_E_ARG): widths multiples of 16 in [16, 1024]; Cin = 1 (the first
 * layer): odd taps <= 15, stride 1, groups 1; Cout = 1 (conv_post): 3 taps, stride 1, groups 1; the dense layer: 5 taps, stride 1, groups 1; a grouped layer: odd
 * taps <= 41, stride 1, 2 or 4, Cout / groups a multiple of 16, Cin / groups a multiple of 4 and at most 64.  1 <= B <= 65535, B L <= 2^30.
 *   work   glowtts_hifigan_msd_work_floats(B, rows_out, Cin, Cout, taps, groups) floats, 8-byte aligned: the weight gradient's splits of a first or grouped
 *          layer with rows_out output rows per batch row, and at least the block sums of glowtts_hifigan_disc_fm on that layer's output (the dense layers:
 *          glowtts_hifigan_disc_work_floats).
 * glowtts_hifigan_msd_pool         `hifigan_msd_pool`: x [B][T] -> y [B][T / 2 + 1], y[j] = (x[2 j - 2] + .. + x[2 j + 1]) / 4, zero outside [0, T).
 * glowtts_hifigan_msd_pool_bwd     `hifigan_msd_pool_bwd`: dy [B][T / 2 + 1] -> dx [B][T], a gather over the at most 2 outputs that read a sample; accumulate 1:
 *                                  added to what dx holds.
 * glowtts_hifigan_msd_first        `hifigan_msd_first`: wav [B][T] -> out [B][T][C]; w [taps][C] (row = tap), bias [C].
 * glowtts_hifigan_msd_conv         `hifigan_msd_conv`: x [B][L][Cin] -> out [B][L'][Cout] = bias + grouped conv(lrelu(x, slope)); w [groups][taps Cin_g][Cout_g]:
 *                                  row = tap Cin_g + input channel of the group.
 * glowtts_hifigan_msd_dense        `hifigan_msd_dense`: x [B][L][Cin] -> out [B][L][Cout], 5 taps; w [5 Cin][Cout] (glowtts_hifigan_disc_conv at period 1).
 * glowtts_hifigan_msd_post         `hifigan_msd_post`: x [B][L][C] -> scores [B][L] = bias + conv(lrelu(x, slope)); w [3][C] (row = tap), bias [1].
 * glowtts_hifigan_msd_post_bwd     `hifigan_msd_post_bwd`: glowtts_hifigan_disc_post_bwd at period 1.
 * glowtts_hifigan_msd_dense_bwd    `hifigan_msd_dense_bwd`: dy [B][L][Cout], x [B][L][Cin] (kept) -> dx [B][L][Cin] = lrelu'(x) times the transposed convolution of
 *                                  dy, + inj *inj_scale; wt [5 Cout][Cin]: row = tap Cout + output channel.
 * glowtts_hifigan_msd_conv_bwd     `hifigan_msd_conv_bwd`: dy [B][L'][Cout], x [B][L][Cin] (kept) -> dx [B][L][Cin], the transposed convolution in polyphase form
 *                                  (input row n takes only the taps m with (n + taps / 2 - m) % stride == 0), times lrelu'(x), + inj *inj_scale (inj [B][L][Cin]
 *                                  or NULL; inj_scale: ONE float on the device); wt [groups][taps][Cout_g][Cin_g rounded up to 16]: the columns from Cin_g on zero.
 * glowtts_hifigan_msd_first_bwd    `hifigan_msd_first_bwd`: dpre [B][T][C] of the first layer -> dwav [B][T]; accumulate 1: added to what dwav holds.
 * glowtts_hifigan_msd_wgrad        `hifigan_msd_wgrad` + `hifigan_msd_wgrad_sum` for ONE grouped layer with L input rows: x its input (lrelu(x, slope) is formed
 *                                  on the way in), dy [B][L'][Cout] -> dw [Cout][Cin_g][taps], dbias [Cout] in torch's layouts; overwritten.  One split per batch
 *                                  row and 1024 output rows, added in ascending order.
 * glowtts_hifigan_msd_first_wgrad  `hifigan_msd_first_wgrad` + `hifigan_msd_first_wgrad_sum`: wav [B][T], dy [B][T][C] -> dw [C][1][taps], dbias [C].
 * glowtts_hifigan_msd_dense_wgrad  `hifigan_msd_dense_wgrad` + `hifigan_msd_dense_wgrad_sum` (glowtts_hifigan_disc_wgrad at period 1): the dense layer (taps 5) or
 *                                  conv_post (taps 3, Cout 1, dy = d scores [B][L]); work: glowtts_hifigan_disc_work_floats. */
int glowtts_hifigan_msd_supported(int Cin, int Cout, int taps, int stride, int groups);
int64_t glowtts_hifigan_msd_work_floats(int B, int rows_out, int Cin, int Cout, int taps, int groups);
int glowtts_hifigan_msd_pool(const float *x, float *y, int B, int T, void *stream);
int glowtts_hifigan_msd_pool_bwd(const float *dy, float *dx, int B, int T, int accumulate, void *stream);
int glowtts_hifigan_msd_first(const float *wav, const float *w, const float *bias, float *out, int B, int T, int taps, int C, void *stream);
int glowtts_hifigan_msd_conv(const float *x, const float *w, const float *bias, float *out, int B, int L, int taps, int stride, int groups, int Cin, int Cout,
                             float slope, void *stream);
int glowtts_hifigan_msd_dense(const float *x, const float *w, const float *bias, float *out, int B, int L, int Cin, int Cout, float slope, void *stream);
int glowtts_hifigan_msd_post(const float *x, const float *w, const float *bias, float *scores, int B, int L, int C, float slope, void *stream);
int glowtts_hifigan_msd_post_bwd(const float *dscores, const float *dscores2, const float *x, const float *w, const float *inj, const float *inj_scale, float *dx,
                                 int B, int L, int C, float slope, void *stream);
int glowtts_hifigan_msd_dense_bwd(const float *dy, const float *wt, const float *x, const float *inj, const float *inj_scale, float *dx, int B, int L, int Cin,
                                  int Cout, float slope, void *stream);
int glowtts_hifigan_msd_conv_bwd(const float *dy, const float *wt, const float *x, const float *inj, const float *inj_scale, float *dx, int B, int L, int taps,
                                 int stride, int groups, int Cin, int Cout, float slope, void *stream);
int glowtts_hifigan_msd_first_bwd(const float *dpre, const float *w, float *dwav, int B, int T, int taps, int C, int accumulate, void *stream);
int glowtts_hifigan_msd_wgrad(const float *x, const float *dy, float *work, float *dw, float *dbias, int B, int L, int taps, int stride, int groups, int Cin,
                              int Cout, float slope, void *stream);
int glowtts_hifigan_msd_first_wgrad(const float *wav, const float *dy, float *work, float *dw, float *dbias, int B, int T, int taps, int C, void *stream);
int glowtts_hifigan_msd_dense_wgrad(const float *x, const float *dy, float *work, float *dw, float *dbias, int B, int L, int Cin, int Cout, int taps, float slope,
                                    void *stream);

/* ---- Objective evaluation: mel cepstra and dynamic time warping (csrc/eval_ops.hip; f32; additions, the ABI version stays) ----
 * glowtts_mel_cepstrum   `eval_mel_cepstrum`: mels in this project's normalisation m = 2A (db + 100) / 100 - A (A = max_abs; values at the clip +- A taken
 *   as they are), read through the element strides (stride_b, stride_t, stride_m) - [B][T][Mel] or the models' [B][Mel][T] - with lengths [B] int64 (device)
 *   -> cep [B][T][K] f32.  L = ln(amplitude) = (ln 10 / 20) ((m + A) 100 / (2A) - 100); c_k = sqrt(2 / Mel) sum_m L_m cos(pi k (m + 1/2) / Mel), k = 1 .. K:
 *   the orthonormal DCT-II without its 0th coefficient, so a constant offset of the mel drops out.  basis [K][Mel] f32 (device) holds
 *   sqrt(2 / Mel) cos(pi (k + 1) (m + 1/2) / Mel) for row k = 0 .. K - 1; the sum runs over m ascending, one fused multiply-add per term.  Rows t >= lengths[b]
 *   are zeros.  Supported (glowtts_mel_cepstrum_supported, else GLOWTTS_E_ARG): 1 <= K <= 64, K < Mel <= 512, Mel K <= 4096; 1 <= B <= 65535, B T <= 2^30.
 * glowtts_dtw            `eval_dtw`: B pairs X_b [x_lengths[b]][K], Y_b [y_lengths[b]][K] of the padded batches x [B][tx_max][K], y [B][ty_max][K] (lengths
 *   int32, device, each in [1, its max]).  Local cost d(i, j) = sqrt(sum_k (x_ik - y_jk)^2) in f32, k ascending, one fused multiply-add per term, correctly
 *   rounded square root.  D(0, 0) = d(0, 0); the first row and column accumulate along themselves; else D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j),
 *   D(i, j-1)), the predecessor being the diagonal if it is <= both others, else (i-1, j) if it is <= (i, j-1), else (i, j-1).  No band or slope constraint.
 *   Backtrack from (Tx-1, Ty-1).  Outputs per pair: cost [B] = D(Tx-1, Ty-1); steps [B] = N; ix, iy [B][tx_max + ty_max - 1] int32 = the path in forward
 *   order, -1 beyond N; moves [B][3] int32 = the number of diagonal, (i-1, j) and (i, j-1) steps.  A pair whose length is out of range gets cost NaN,
 *   steps 0 and no path.  work: B * glowtts_dtw_work_bytes(tx_max, ty_max) bytes (2-bit back-pointers); nothing is allocated.  One workgroup per pair, no
 *   atomics: a pair's result is bit-identical alone, in any batch, at any padding and from run to run.
 *   Supported (glowtts_dtw_supported, else GLOWTTS_E_ARG): tx_max, ty_max in [1, GLOWTTS_DTW_MAX_FRAMES], k in [1, GLOWTTS_DTW_MAX_K]; 1 <= B <= 65535. */
#define GLOWTTS_DTW_MAX_FRAMES 4096
#define GLOWTTS_DTW_MAX_K 64
int glowtts_mel_cepstrum_supported(int Mel, int K);
int glowtts_mel_cepstrum(const float *mel, const int64_t *lengths, const float *basis, float *cep, int B, int T, int Mel, int K, int64_t stride_b,
                         int64_t stride_t, int64_t stride_m, float max_abs, void *stream);
int glowtts_dtw_supported(int tx_max, int ty_max, int k);
int64_t glowtts_dtw_work_bytes(int tx_max, int ty_max);
int glowtts_dtw(const float *x, const int32_t *x_lengths, const float *y, const int32_t *y_lengths, void *work, float *cost, int32_t *steps, int32_t *ix,
                int32_t *iy, int32_t *moves, int B, int tx_max, int ty_max, int K, void *stream);

/* ---- Embedding maps: exact t-SNE into two dimensions (csrc/tsne_ops.hip; f32; additions, the ABI version stays) ----
 * The matrix of the fit is N rows of pitch ld = (N + 3) & ~3 floats (rows 16-byte aligned; the pad columns hold 0 once it is P) at the start of the workspace:
 * squared distances, then conditional affinities, then the joint affinities P, in place.  work: glowtts_tsne_work_bytes(N) bytes = that matrix, then the per-row
 * partials sums [N][4] f32 and shares [N][4] float64 of the last `tsne_forces` launch; 16-byte aligned; nothing is allocated.
 * glowtts_tsne_sqdist      `tsne_sqdist`: x [N][D] -> d2 [N][ld], ld >= N: d2[i][j] = sum_k (x_ik - x_jk)^2 by direct differences, k ascending, one fused
 *   multiply-add per term (never the Gram form: identical rows give exactly 0).  Columns j >= N are not written.
 * glowtts_tsne_affinities  `tsne_sqdist`, `tsne_affinity` and, with joint != 0, `tsne_symmetrize`: x -> the matrix of the workspace.  Row i works on
 *   d_j = d2[i][j] - min_{j != i} d2[i][j], j != i, and bisects beta in exactly 64 steps from beta = 1, lo = 0, hi = inf: each step evaluates e_j = exp(-beta d_j),
 *   s = sum e_j, H = ln s + beta sum d_j e_j / s (the two sums in float64 over the f32 terms, rounded to f32; H in f32); H > ln(perplexity): lo = beta and beta
 *   doubles while hi is inf, else beta = (beta + hi) / 2; otherwise hi = beta, beta = (beta + lo) / 2.  p_{j|i} = e_j / s of the last beta evaluated, p_{i|i} = 0
 *   (joint == 0 stops here: the conditional rows, for tests).  P_ij = max((p_{j|i} + p_{i|j}) / (2N), 1e-12) off the diagonal, 0 on it: symmetric bit for bit.
 * glowtts_tsne_forces      `tsne_forces` (kl != 0: `tsne_forces,kl`), one evaluation: p (the matrix P), y [N][2] -> sums [N][4] f32 = sum_j P_ij w_ij (y_i - y_j)
 *   (x, y) and sum_j w_ij^2 (y_i - y_j) (x, y), w_ij = 1 / (1 + |y_i - y_j|^2), j != i; shares [N][4] float64 = sum_j w_ij, and with kl != 0
 *   sum_j P_ij (ln P_ij - ln w_ij) and sum_j P_ij (else 0, 0), and 0.  w and the force terms are f32.  kl == 0: the Z share adds the f32 w in float64
 *   (within 3 * 2^-24 Z of the exact sum).  kl != 0, the launch whose figures are reported: the Z share and the KL share's terms are float64 arithmetic on
 *   the exact differences of the f32 y, -ln w_ij taken as ln(1 + |y_i - y_j|^2).  Every sum runs in a fixed order.
 * glowtts_tsne_iterate     iterations t = t0 .. t1 - 1 on the state y, u, gain [N][2] (f32, in place), two launches each: `tsne_forces` (`tsne_forces,kl` when
 *   kl_every > 0 and t % kl_every == 0) and `tsne_step` (one workgroup): Z = sum_i shares; a = 12, mu = 0.5 while t < exaggeration_iterations, then a = 1,
 *   mu = 0.8; g = 4 (a attractive - repulsive / Z); gain += 0.2 where sign(g) != sign(u) (sign(0) = 0), else gain *= 0.8, floor 0.01; u = mu u - lr gain g; y += u;
 *   y -= mean(y).  A measuring iteration writes KL = sum_ij P_ij (ln P_ij - ln w_ij) + ln Z sum_ij P_ij (float64) of the y it STARTS from into kl[t / kl_every];
 *   kl_final != 0 adds one `tsne_forces,kl` and one `tsne_step,finish` launch that write the KL of the final y into kl[ceil(t1 / kl_every)] (kl[0] when
 *   kl_every <= 0) and change no state.  No host synchronisation; no atomics; every reduction order is fixed: the state is bit-identical from run to run.
 *   Supported (glowtts_tsne_supported, else GLOWTTS_E_ARG): N in [8, GLOWTTS_TSNE_MAX_N], D in [1, GLOWTTS_TSNE_MAX_D], 1 <= perplexity <= (N - 1) / 3. */
#define GLOWTTS_TSNE_MAX_N 8192
#define GLOWTTS_TSNE_MAX_D 1024
int glowtts_tsne_supported(int N, int D);
int64_t glowtts_tsne_work_bytes(int N);
int glowtts_tsne_sqdist(const float *x, float *d2, int N, int D, int ld, void *stream);
int glowtts_tsne_affinities(const float *x, void *work, int N, int D, float perplexity, int joint, void *stream);
int glowtts_tsne_forces(const float *p, const float *y, float *sums, double *shares, int N, int kl, void *stream);
int glowtts_tsne_iterate(void *work, float *y, float *u, float *gain, double *kl, int N, int t0, int t1, int exaggeration_iterations, float learning_rate,
                         int kl_every, int kl_final, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOWTTS_HIP_H */
