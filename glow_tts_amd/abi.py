"""The Python restatement of the C ABI (include/glowtts_hip.h) - the only one: every constant, struct mirror and function signature the package,
the tests, the tools and the benchmark use.  Nothing here loads a library (`_lib.lib()` does, and binds SIGNATURES onto it once);
tests/test_abi.py compares all three parts with the header on the CPU: names, parameter kinds, struct layouts (through the C compiler), values."""
import ctypes
from ctypes import POINTER, c_char_p

# ---- constants: GLOWTTS_<NAME> of the header is <NAME> here --------------------------------------------------------------------------
ABI_VERSION = 7
OK, E_ARG, E_LAUNCH = 0, -1, -2
F32, BF16 = 0, 1
PERM_NONE, PERM_PAIR = 0, 1
APRO_NONE, APRO_PAIRMUL, APRO_SQNEG = 0, 1, 2
EPI_LINEAR, EPI_GATE, EPI_RESSKIP, EPI_COUPLE, EPI_DGATE = 0, 1, 2, 3, 4
F_BIAS, F_RELU, F_ADD_IN0, F_MASK, F_ACCUM, F_FIRST, F_LAST, F_REVERSE, F_COLMASK, F_DROPOUT = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
F_COND_ROWS, F_GATE_IN0, F_COND_FX = 1024, 2048, 4096
IO_A_BF16, IO_IN0_BF16, IO_OUT0_BF16 = 1, 2, 4      # glowtts_conv_args.io_flags
WIO_DY_BF16, WIO_X_BF16, WIO_WIDE, WIO_DMA = 1, 2, 4, 8           # glowtts_wgrad_args.io_flags (DMA: grouped launches only)
ROW_PAD = 2
MAX_WN_LAYERS = 8
WN_SLAB_BYTES = 24576
WN_FUSED_MAX_LAYERS = 4
PREP_MAX_JOBS = 22
WN_BWD_MAX_JOBS = 8
SUM_MAX_SEGS = 12
C2D_MAX_LAYERS = 8
SAMPLE_SCAN_CHUNK = 1024
SAMPLE_TILE = 64
GE2E_MAX_MEL, GE2E_MAX_H, GE2E_MAX_STACKS, GE2E_MAX_E = 512, 768, 8, 1024
DTW_MAX_FRAMES, DTW_MAX_K = 4096, 64
TSNE_MAX_N, TSNE_MAX_D = 8192, 1024

# ---- struct mirrors: `c_name` is the C struct whose layout the class restates ------------------------------------------------------------
I, L, F, U, P = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint32, ctypes.c_void_p
PI, PL = POINTER(I), POINTER(L)


def _fields(*groups):
    """("a b c", T), ... -> [("a", T), ("b", T), ("c", T), ...]"""
    return [(name, t) for names, t in groups for name in names.split()]


class Packed(ctypes.Structure):
    c_name = "glowtts_packed"
    _fields_ = _fields(("w", P), ("npad kchunks", I))


class FlowDims(ctypes.Structure):
    c_name = "glowtts_flow_dims"
    _fields_ = _fields(("B T C H L ksize precision", I), ("drop_p", F), ("seed", U), ("seed_ptr", P), ("act_bf16", I))


class FlowParams(ctypes.Structure):
    c_name = "glowtts_flow_params"
    _fields_ = _fields(("an_logs an_bias winfo", P),
                       ("start", Packed), ("in_ rs", Packed * MAX_WN_LAYERS), ("end", Packed),
                       ("start_t", Packed), ("in_t rs_t", Packed * MAX_WN_LAYERS), ("end_t", Packed),
                       ("b_start", P), ("b_in b_rs", P * MAX_WN_LAYERS), ("b_end", P),
                       ("cond", P), ("ldcond", L), ("cond_rows", I), ("wn_img wn_img_t", P))


class FlowActs(ctypes.Structure):
    c_name = "glowtts_flow_acts"
    _fields_ = _fields(("xin xmid xout", P), ("hs gates", P * MAX_WN_LAYERS), ("skip outs rowmask", P), ("acts", P * MAX_WN_LAYERS),
                       ("skip_bf xa_bf next_an_logs next_an_bias next_winfo next_xmid next_xout next_xa_bf", P), ("actnorm_done", I))


class FlowGrads(ctypes.Structure):
    c_name = "glowtts_flow_grads"
    _fields_ = _fields(("dx dlogdet douts dskip", P), ("dh dins", P * MAX_WN_LAYERS), ("defer_wgrad", I),
                       ("scratch d_an dw_start db_start", P), ("dw_in db_in dw_rs db_rs", P * MAX_WN_LAYERS),
                       ("dw_end db_end dcond douts_bf", P), ("coupling_done", I), ("prev_xmid prev_outs prev_douts prev_douts_bf pitch_rows", P),
                       ("pitch_ns dh0_bf16", I))


class WnBwdJob(ctypes.Structure):
    c_name = "glowtts_wn_bwd_job"
    _fields_ = _fields(("dw v g inv_norm dv dg", P), ("rows", L), ("cols reserved", I))


class SumSeg(ctypes.Structure):
    c_name = "glowtts_sum_seg"
    _fields_ = _fields(("dst", P), ("off n", L))


class WgradJob(ctypes.Structure):
    """One weight-gradient problem of the grouped launch."""
    c_name = "glowtts_wgrad_job"
    _fields_ = _fields(("dy x xmask dw dbias", P), ("lddy ldx", L), ("m ca xpro perm perm_h tile0 mt nt rows reserved", I))


class PrepJob(ctypes.Structure):
    """Weight norm + packing of one conv class into one image (csrc/prep_ops.hip)."""
    c_name = "glowtts_prep_job"
    _fields_ = _fields(("v g inv_out packed", P), ("outer_stride inner_stride w_stride g_stride", L),
                       ("batch inner O I taps transpose perm perm_h o_ext npad kchunks tiles block0 reserved", I),
                       ("twin", P), ("twin_outer twin_inner twin_half", L), ("twin_batch twin_npad", I))


class ConvArgs(ctypes.Structure):
    c_name = "glowtts_conv_args"
    _fields_ = _fields(("a", P), ("lda", L), ("a2", P), ("lda2", L), ("ca1 ca apro rows", I), ("w", P),
                       ("n npad kchunks taps pad precision epi flags h rows_per_utt", I), ("bias rowmask cond", P), ("ldcond", L),
                       ("out0", P), ("ld0", L), ("out1", P), ("ld1", L), ("in0", P), ("ldi0", L), ("batch", I),
                       ("a_bstride w_bstride bias_bstride out_bstride mask_bstride", L), ("ncols_valid", P),
                       ("seed", U), ("drop_p", F), ("seed_ptr", P), ("io_flags", I))


class WgradArgs(ctypes.Structure):
    c_name = "glowtts_wgrad_args"
    _fields_ = _fields(("dy", P), ("lddy", L), ("x", P), ("ldx", L), ("xpro", I), ("xmask", P),
                       ("rows m ca taps pad perm perm_h precision splits accumulate", I), ("dw dbias", P), ("io_flags", I))


class PackJob(ctypes.Structure):
    c_name = "glowtts_pack_job"
    _fields_ = _fields(("w packed", P), ("O I taps transpose perm perm_h N K npad kchunks block0 reserved", I))


class OptJob(ctypes.Structure):
    c_name = "glowtts_opt_job"
    _fields_ = _fields(("p g m v", P), ("n block0", L))


class C2dPackJob(ctypes.Structure):
    c_name = "glowtts_c2d_pack_job"
    _fields_ = _fields(("w img", P), ("Ci Co cls N K npad kchunks block0", I))


class C2dReduceJob(ctypes.Structure):
    c_name = "glowtts_c2d_reduce_job"
    _fields_ = _fields(("partial dw", P), ("splits Ci Co block0", I))


# ---- signatures: name -> (restype, argtypes), one entry per prototype of the header, in its order.  I = int, L = int64_t, F = float, U = uint32_t,
# P = any pointer (callers pass device addresses as integers, None or byref(...)); typed pointers where callers pass byref() of that type ----
SIGNATURES = {
    "glowtts_abi_version": (I, []),
    "glowtts_device_arch": (I, [c_char_p, I]),
    "glowtts_launch_count": (L, [c_char_p]),
    "glowtts_launch_log_reset": (None, []),
    "glowtts_launch_log_dump": (I, [c_char_p, I]),
    "glowtts_mfma_clock_probe": (I, [P, I, I, PI, P]),
    "glowtts_debug_stamp": (I, [P, P]),
    "glowtts_step_seed": (I, [P] * 3),
    "glowtts_mas_dp_f32": (I, [P] * 5 + [I] * 3 + [F, P]),
    "glowtts_mas_dp_f32_t": (I, [P] * 5 + [I] * 3 + [F, P]),
    "glowtts_mas_path_from_idx": (I, [P, P] + [I] * 4 + [P]),
    "glowtts_mas_f32": (I, [P] * 5 + [I] * 3 + [F, P]),
    "glowtts_mas_f32_host": (I, [P] * 4 + [I] * 3 + [F, I]),
    "glowtts_pack_weight": (I, [P] + [I] * 7 + [P, PI, PI, P]),
    "glowtts_pack_job_init": (I, [POINTER(PackJob), P] + [I] * 7 + [P, I, PI, PL]),
    "glowtts_pack_weight_multi": (I, [P] + [I] * 3 + [P]),
    "glowtts_pack_weight_batched": (I, [P] + [I] * 8 + [P, PI, PI, P]),
    "glowtts_pack_weight_strided": (I, [P] + [I] * 9 + [P] + [L] * 3 + [P]),
    "glowtts_prep_jobs_twin_in": (I, [P, PI, PI]),
    "glowtts_prep_job_init": (I, [P] * 4 + [I] * 8 + [P] + [L] * 4 + [I, PI]),
    "glowtts_prep_launch": (I, [P] + [I] * 3 + [P]),
    "glowtts_prep_launch_dev": (I, [P] + [I] * 3 + [P]),
    "glowtts_conv_chain": (I, [P] * 3),
    "glowtts_conv_cl": (I, [P, P]),
    "glowtts_squeeze_rows": (I, [P] * 4 + [I] * 4 + [P]),
    "glowtts_unsqueeze_rows": (I, [P] * 3 + [I] * 5 + [F, P]),
    "glowtts_inv1x1_prepare": (I, [P, P, I, P]),
    "glowtts_actnorm_inv1x1": (I, [P] * 6 + [L, I, I, P]),
    "glowtts_actnorm_inv1x1_pass_bf": (I, [P] * 8 + [L, I, P]),
    "glowtts_actnorm_inv1x1_pass": (I, [P] * 7 + [L, I, P]),
    "glowtts_actnorm_stats": (I, [P] * 4 + [L, I, P]),
    "glowtts_actnorm_stats_scratch_floats": (L, [L, I]),
    "glowtts_actnorm_from_stats": (I, [P] * 3 + [I, P]),
    "glowtts_coupling_bwd": (I, [P] * 6 + [L] + [I] * 3 + [P]),
    "glowtts_coupling_bwd_bf16": (I, [P] * 7 + [L] + [I] * 3 + [P]),
    "glowtts_fill_zero": (I, [P, L, P]),
    "glowtts_actnorm_inv1x1_bwd": (I, [P] * 9 + [L, I, P]),
    "glowtts_actnorm_bwd_blocks": (L, [L]),
    "glowtts_actnorm_inv1x1_bwd_coupling": (I, [P] * 8 + [L, I] + [P] * 5 + [I, I, P]),
    "glowtts_colsum_batched": (I, [P, P] + [I] * 3 + [L, L, P]),
    "glowtts_decoder_param_grads": (I, [P] * 7 + [I] * 4 + [P]),
    "glowtts_decoder_logdet": (I, [P, L] + [P] * 5 + [I] * 5 + [P]),
    "glowtts_wgrad_cl": (I, [P, P]),
    "glowtts_wgrad_grouped": (I, [P] + [I] * 9 + [P]),
    "glowtts_wgrad_grouped_io": (I, [P] + [I] * 10 + [P]),
    "glowtts_wgrad_grouped_phased": (I, [P] + [I] * 5 + [P]),
    "glowtts_flow_forward": (I, [P] * 4),
    "glowtts_flow_inverse": (I, [P] * 4),
    "glowtts_flow_encode": (I, [P] * 4),
    "glowtts_flow_backward": (I, [P] * 5),
    "glowtts_wavenet_image_bytes": (I, [I, I, PL]),
    "glowtts_wavenet_pack_images": (I, [P] * 5 + [I] * 3 + [P] * 3),
    "glowtts_wavenet_prep_jobs": (I, [P, I, PI, PI] + [P] * 13 + [I] * 3 + [P, I, P]),
    "glowtts_wavenet_fwd": (I, [P] * 5 + [I, I, P]),
    "glowtts_wavenet_bwd": (I, [P] * 5),
    "glowtts_wavenet_debug_safe_waits": (None, [I]),
    "glowtts_utt_colsum": (I, [P, L, P, L] + [I] * 5 + [P]),
    "glowtts_cond_linear_fwd": (I, [P] * 6 + [I] * 4 + [P]),
    "glowtts_cond_linear_bwd_scratch_floats": (L, [I] * 3),
    "glowtts_cond_linear_supported": (I, [I] * 3),
    "glowtts_fx_to_float": (I, [P, P, L, P]),
    "glowtts_cond_linear_bwd": (I, [P, L] + [P] * 9 + [I] * 3 + [P]),
    "glowtts_gru_fwd": (I, [P] * 5 + [I] * 3 + [P]),
    "glowtts_gru_bwd": (I, [P] * 6 + [I] * 3 + [P]),
    "glowtts_gst_supported": (I, [I] * 7),
    "glowtts_gst_keep_floats": (L, [I] * 6),
    "glowtts_gst_fwd": (I, [P, P, I] + [P] * 13 + [I] * 7 + [P]),
    "glowtts_gst_bwd": (I, [P] * 3 + [I] + [P] * 18 + [I] * 7 + [P]),
    "glowtts_conv3x3s2_supported": (I, [I] * 5),
    "glowtts_conv3x3s2_image_bytes": (I, [I] * 3 + [PL, PL]),
    "glowtts_conv3x3s2_pack_job_init": (I, [POINTER(C2dPackJob), P] + [I] * 4 + [P, I, PI]),
    "glowtts_conv3x3s2_pack": (I, [P] + [I] * 3 + [P]),
    "glowtts_conv3x3s2_fwd": (I, [P] * 4 + [I] * 7 + [P]),
    "glowtts_conv3x3s2_dgrad": (I, [P, POINTER(P), P, P] + [I] * 6 + [P]),
    "glowtts_conv3x3s2_wgrad_scratch_floats": (L, [I] * 5),
    "glowtts_conv3x3s2_wgrad": (I, [P] * 3 + [I] * 6 + [PI, P]),
    "glowtts_conv3x3s2_wgrad_reduce": (I, [POINTER(C2dReduceJob), I, P]),
    "glowtts_layernorm_fwd": (I, [P] * 8 + [L, I, F, I, F, U, P, P]),
    "glowtts_layernorm_fwd_io": (I, [P] * 8 + [L, I, F, I, F, U] + [P] * 3),
    "glowtts_proj_layernorm": (I, [P, L, P, I] + [P] * 10 + [L, I, F, F, U, P, P]),
    "glowtts_layernorm_qkv": (I, [P] * 10 + [I, P, P, L, I, F, P]),
    "glowtts_layernorm_scratch_floats": (L, [L, I]),
    "glowtts_layernorm_bwd": (I, [P] * 9 + [L, I, I, F, P]),
    "glowtts_layernorm_bwd_io": (I, [P] * 9 + [L, I, I, F, P, P, F, P]),
    "glowtts_gate_bwd": (I, [P] * 4 + [L, I, F, P]),
    "glowtts_gate_bwd_io": (I, [P] * 4 + [L, I, F, I, P]),
    "glowtts_token_masks": (I, [P] * 3 + [I, I, P]),
    "glowtts_embedding_fwd": (I, [P] * 4 + [I] * 3 + [F, P]),
    "glowtts_embedding_bwd": (I, [P] * 4 + [I] * 4 + [F, P]),
    "glowtts_rpr_attention_fwd": (I, [P] * 6 + [I] * 5 + [F, U, P, P]),
    "glowtts_rpr_attention_scratch_floats": (L, [I] * 5),
    "glowtts_rpr_attention_bwd": (I, [P] * 11 + [I] * 5 + [F, U, P, P]),
    "glowtts_rpr_attention_fwd_prec": (I, [P] * 6 + [I] * 5 + [F, U, P, I, P]),
    "glowtts_rpr_attention_bwd_partial_rows": (L, [I] * 5),
    "glowtts_rpr_attention_fwd_eval": (I, [P] * 5 + [I] * 6 + [P]),
    "glowtts_rpr_attention_bwd_prec": (I, [P] * 11 + [I] * 5 + [F, U, P, I, P]),
    "glowtts_logprior_prep": (I, [P] * 9 + [I] * 5 + [PI, PI, P]),
    "glowtts_expand_fwd": (I, [P] * 3 + [I] * 4 + [P]),
    "glowtts_expand_bwd": (I, [P] * 3 + [I] * 4 + [P]),
    "glowtts_duration_targets": (I, [P] * 3 + [I] * 3 + [P]),
    "glowtts_mle_loss_fwd": (I, [P] * 8 + [L] + [I] * 3 + [P]),
    "glowtts_mle_loss_bwd": (I, [P] * 8 + [L, P, I, P]),
    "glowtts_expand_pair_targets": (I, [P] * 8 + [I] * 4 + [P]),
    "glowtts_prior_loss_bwd": (I, [P] * 10 + [I] * 4 + [P]),
    "glowtts_mse_loss_fwd": (I, [P] * 3 + [L, F, P, I] + [P] * 3),
    "glowtts_mse_loss_bwd": (I, [P] * 4 + [L, F, P, I, P, P]),
    "glowtts_prior_loss": (I, [P] * 17 + [I] * 6 + [P]),
    "glowtts_dur_proj_supported": (I, [I]),
    "glowtts_dur_proj_fwd": (I, [P] * 5 + [I] * 4 + [P]),
    "glowtts_dur_proj_bwd": (I, [P] * 9 + [I] * 4 + [P]),
    "glowtts_prior_split_fwd": (I, [P] * 3 + [I] * 4 + [P]),
    "glowtts_prior_split_bwd": (I, [P] * 3 + [I] * 4 + [P]),
    "glowtts_weightnorm_fwd": (I, [P] * 4 + [L, I, P]),
    "glowtts_weightnorm_bwd": (I, [P] * 6 + [L, I, P]),
    "glowtts_weightnorm_bwd_multi": (I, [P, I, P]),
    "glowtts_opt_chunk": (I, []),
    "glowtts_multi_grad_norm": (I, [P, I, I, F] + [P] * 3),
    "glowtts_sum_slices": (I, [P, P, I, L, P]),
    "glowtts_sum_slices_seg": (I, [P, I, L, P, I, P]),
    "glowtts_multi_grad_scale": (I, [P, I, I, P, P]),
    "glowtts_radam_step": (I, [P, I, I] + [P] * 3),
    "glowtts_vocoder_supported": (I, [I] * 3),
    "glowtts_mel_to_linear_f32": (I, [P] * 4 + [I] * 4 + [F, P]),
    "glowtts_stft_f32": (I, [P] * 5 + [I] * 6 + [P]),
    "glowtts_istft_f32": (I, [P] * 6 + [I] * 6 + [P]),
    "glowtts_overlap_add_f32": (I, [P] * 4 + [I] * 6 + [P]),
    "glowtts_griffin_lim_step_f32": (I, [P] * 6 + [F, P] + [I] * 6 + [P]),
    "glowtts_mel_analysis_f32": (I, [P] * 7 + [I] * 8 + [F] * 3 + [P]),
    "glowtts_yin_f32": (I, [P] * 4 + [I] * 7 + [F, F, P]),
    "glowtts_prior_sample": (I, [P] * 9 + [I] * 4 + [P]),
    "glowtts_prior_sample_aligned": (I, [P] * 10 + [I] * 4 + [P]),
    "glowtts_pwg_supported": (I, [I] * 5),
    "glowtts_pwg_condition": (I, [P] * 5 + [I] + [P] * 2 + [I] * 4 + [P]),
    "glowtts_pwg_first": (I, [P] * 6 + [I] * 4 + [P]),
    "glowtts_pwg_layer": (I, [P] * 9 + [I] * 8 + [P]),
    "glowtts_pwg_head": (I, [P] * 7 + [I] * 4 + [F, P]),
    "glowtts_pwg_supported_bf16": (I, [I] * 5),
    "glowtts_pwg_layer_bf16": (I, [P] * 9 + [I] * 8 + [P]),
    "glowtts_hifigan_supported": (I, [I] * 5),
    "glowtts_hifigan_conv": (I, [P] * 6 + [I] * 7 + [F, I, F, I, P]),
    "glowtts_hifigan_upsample": (I, [P] * 5 + [I] * 7 + [F, P]),
    "glowtts_hifigan_post": (I, [P] * 5 + [I] * 5 + [F, P]),
    "glowtts_hifigan_supported_f16": (I, [I] * 5),
    "glowtts_hifigan_conv_f16": (I, [P] * 6 + [I] * 7 + [F, I, F, I, P]),
    "glowtts_hifigan_upsample_f16": (I, [P] * 5 + [I] * 7 + [F, P]),
    "glowtts_hifigan_train_supported": (I, [I] * 5),
    "glowtts_hifigan_wgrad_work_floats": (L, [I] * 7),
    "glowtts_hifigan_conv_bwd": (I, [P] * 6 + [I] * 7 + [F, F, F, I, P]),
    "glowtts_hifigan_upsample_bwd": (I, [P] * 5 + [I] * 7 + [F, P]),
    "glowtts_hifigan_post_bwd": (I, [P] * 7 + [I] * 5 + [F, P]),
    "glowtts_hifigan_wgrad": (I, [P] * 6 + [I] * 8 + [F, F, I, P]),
    "glowtts_hifigan_train_supported_mixed": (I, [I] * 5),
    "glowtts_hifigan_conv_bwd_bf16": (I, [P] * 6 + [I] * 7 + [F, F, F, I, P]),
    "glowtts_hifigan_upsample_bwd_bf16": (I, [P] * 5 + [I] * 7 + [F, P]),
    "glowtts_hifigan_wgrad_bf16": (I, [P] * 6 + [I] * 8 + [F, F, I, P]),
    "glowtts_hifigan_pack_images": (I, [P, I, I, P]),
    "glowtts_ge2e_supported": (I, [I] * 4),
    "glowtts_ge2e_image_floats": (L, [I] * 3),
    "glowtts_ge2e_work_floats": (L, [L] + [I] * 3),
    "glowtts_ge2e_pack": (I, [P] * 6 + [I] * 4 + [P]),
    "glowtts_ge2e_forward": (I, [P] * 9 + [I] * 7 + [P]),
    "glowtts_ge2e_train_image_floats": (L, [I] * 2),
    "glowtts_ge2e_train_keep_floats": (L, [L] + [I] * 3),
    "glowtts_ge2e_train_loss_work_floats": (L, [L] + [I] * 2),
    "glowtts_ge2e_train_work_floats": (L, [L] + [I] * 4),
    "glowtts_ge2e_train_pack": (I, [P] * 3 + [I] * 3 + [P]),
    "glowtts_ge2e_train_forward": (I, [P] * 7 + [I] * 6 + [P]),
    "glowtts_ge2e_train_loss": (I, [P] * 6 + [I] * 3 + [P]),
    "glowtts_ge2e_train_backward": (I, [P] * 8 + [I] * 5 + [P]),
    "glowtts_ge2e_train_wgrad": (I, [P] * 8 + [I] * 6 + [P]),
    "glowtts_pwg_train_supported": (I, [I] * 4),
    "glowtts_pwg_train_work_floats": (L, [I] * 6),
    "glowtts_pwg_train_head_bwd": (I, [P] * 11 + [I] * 4 + [F, P]),
    "glowtts_pwg_train_head_wgrad": (I, [P] * 10 + [I] * 4 + [P]),
    "glowtts_pwg_train_layer_bwd": (I, [P] * 14 + [I] * 8 + [P]),
    "glowtts_pwg_train_layer_wgrad": (I, [P] * 15 + [I] * 7 + [P]),
    "glowtts_pwg_train_first_bwd": (I, [P] * 7 + [I] * 4 + [P]),
    "glowtts_pwg_train_upsample_bwd": (I, [P] * 7 + [I] * 5 + [P]),
    "glowtts_pwg_train_cond_in_bwd": (I, [P] * 4 + [I] * 4 + [P]),
    "glowtts_stft_loss_supported": (I, [I] * 4),
    "glowtts_stft_loss_keep_floats": (L, [I] * 4),
    "glowtts_stft_loss_work_floats": (L, [I] * 4),
    "glowtts_stft_loss_forward": (I, [P] * 8 + [I] * 5 + [F, I, P]),
    "glowtts_stft_loss_backward": (I, [P] * 7 + [I] * 5 + [F, I, P]),
    "glowtts_mel_loss_supported": (I, [I] * 5),
    "glowtts_mel_loss_keep_floats": (L, [I] * 4),
    "glowtts_mel_loss_work_floats": (L, [I] * 4),
    "glowtts_mel_loss_forward": (I, [P] * 10 + [I] * 7 + [F, F, I, P]),
    "glowtts_mel_loss_backward": (I, [P] * 10 + [I] * 7 + [F, I, P]),
    "glowtts_pwg_disc_supported": (I, [I] * 3),
    "glowtts_pwg_disc_work_floats": (L, [I] * 3),
    "glowtts_pwg_disc_first": (I, [P] * 4 + [I] * 3 + [F, P]),
    "glowtts_pwg_disc_layer": (I, [P] * 4 + [I] * 4 + [F, P]),
    "glowtts_pwg_disc_last": (I, [P] * 4 + [I] * 3 + [P]),
    "glowtts_pwg_disc_mse": (I, [P] * 4 + [L] * 2 + [F] * 3 + [P]),
    "glowtts_pwg_disc_last_bwd": (I, [P] * 3 + [I] * 3 + [P]),
    "glowtts_pwg_disc_layer_bwd": (I, [P] * 5 + [I] * 4 + [F, P]),
    "glowtts_pwg_disc_first_bwd": (I, [P] * 5 + [I] * 3 + [F, P]),
    "glowtts_pwg_disc_wgrad": (I, [P] * 6 + [I] * 5 + [P]),
    "glowtts_hifigan_disc_supported": (I, [I] * 3),
    "glowtts_hifigan_disc_work_floats": (L, [I] * 5),
    "glowtts_hifigan_disc_first": (I, [P] * 4 + [I] * 5 + [P]),
    "glowtts_hifigan_disc_conv": (I, [P] * 4 + [I] * 6 + [F, P]),
    "glowtts_hifigan_disc_post": (I, [P] * 4 + [I] * 4 + [F, P]),
    "glowtts_hifigan_disc_fm": (I, [P] * 5 + [L, F, I, P]),
    "glowtts_hifigan_disc_post_bwd": (I, [P] * 7 + [I] * 4 + [F, P]),
    "glowtts_hifigan_disc_conv_bwd": (I, [P] * 6 + [I] * 6 + [F, P]),
    "glowtts_hifigan_disc_first_bwd": (I, [P] * 3 + [I] * 6 + [P]),
    "glowtts_hifigan_disc_wgrad": (I, [P] * 5 + [I] * 8 + [F, P]),
    "glowtts_hifigan_disc_supported_bf16": (I, [I] * 3),
    "glowtts_hifigan_disc_conv_bf16": (I, [P] * 4 + [I] * 6 + [F, P]),
    "glowtts_hifigan_disc_conv_bwd_bf16": (I, [P] * 6 + [I] * 6 + [F, P]),
    "glowtts_hifigan_disc_wgrad_bf16": (I, [P] * 5 + [I] * 8 + [F, P]),
    "glowtts_hifigan_msd_supported": (I, [I] * 5),
    "glowtts_hifigan_msd_work_floats": (L, [I] * 6),
    "glowtts_hifigan_msd_pool": (I, [P] * 2 + [I] * 2 + [P]),
    "glowtts_hifigan_msd_pool_bwd": (I, [P] * 2 + [I] * 3 + [P]),
    "glowtts_hifigan_msd_first": (I, [P] * 4 + [I] * 4 + [P]),
    "glowtts_hifigan_msd_conv": (I, [P] * 4 + [I] * 7 + [F, P]),
    "glowtts_hifigan_msd_dense": (I, [P] * 4 + [I] * 4 + [F, P]),
    "glowtts_hifigan_msd_post": (I, [P] * 4 + [I] * 3 + [F, P]),
    "glowtts_hifigan_msd_post_bwd": (I, [P] * 7 + [I] * 3 + [F, P]),
    "glowtts_hifigan_msd_dense_bwd": (I, [P] * 6 + [I] * 4 + [F, P]),
    "glowtts_hifigan_msd_conv_bwd": (I, [P] * 6 + [I] * 7 + [F, P]),
    "glowtts_hifigan_msd_first_bwd": (I, [P] * 3 + [I] * 5 + [P]),
    "glowtts_hifigan_msd_wgrad": (I, [P] * 5 + [I] * 7 + [F, P]),
    "glowtts_hifigan_msd_first_wgrad": (I, [P] * 5 + [I] * 4 + [P]),
    "glowtts_hifigan_msd_dense_wgrad": (I, [P] * 5 + [I] * 5 + [F, P]),
    "glowtts_mel_cepstrum_supported": (I, [I] * 2),
    "glowtts_mel_cepstrum": (I, [P] * 4 + [I] * 4 + [L] * 3 + [F, P]),
    "glowtts_dtw_supported": (I, [I] * 3),
    "glowtts_dtw_work_bytes": (L, [I] * 2),
    "glowtts_dtw": (I, [P] * 10 + [I] * 4 + [P]),
    "glowtts_tsne_supported": (I, [I] * 2),
    "glowtts_tsne_work_bytes": (L, [I]),
    "glowtts_tsne_sqdist": (I, [P] * 2 + [I] * 3 + [P]),
    "glowtts_tsne_affinities": (I, [P] * 2 + [I] * 2 + [F, I, P]),
    "glowtts_tsne_forces": (I, [P] * 4 + [I] * 2 + [P]),
    "glowtts_tsne_iterate": (I, [P] * 5 + [I] * 4 + [F, I, I, P]),
}

# ---- the entry points above whose `int` result is a VALUE (a version, a chunk size, a yes / no), not a GLOWTTS_OK / _E_ARG / _E_LAUNCH status: `_lib.api()`
# raises on a non-zero result of every other `int` entry point (int64_t results - *_floats, *_blocks, *_rows, glowtts_launch_count - are never statuses) ----
VALUE_RETURNING = frozenset({
    "glowtts_abi_version", "glowtts_opt_chunk",
    "glowtts_cond_linear_supported", "glowtts_gst_supported", "glowtts_conv3x3s2_supported", "glowtts_dur_proj_supported", "glowtts_vocoder_supported",
    "glowtts_pwg_supported", "glowtts_pwg_supported_bf16", "glowtts_hifigan_supported", "glowtts_hifigan_supported_f16", "glowtts_hifigan_train_supported", "glowtts_hifigan_train_supported_mixed", "glowtts_ge2e_supported", "glowtts_pwg_train_supported", "glowtts_stft_loss_supported",
    "glowtts_mel_loss_supported",
    "glowtts_pwg_disc_supported", "glowtts_hifigan_disc_supported", "glowtts_hifigan_disc_supported_bf16", "glowtts_hifigan_msd_supported", "glowtts_mel_cepstrum_supported", "glowtts_dtw_supported", "glowtts_tsne_supported",
})
