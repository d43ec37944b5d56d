"""The teacher-forced pass on the GPU.  Operator level: glowtts_prior_sample_aligned (csrc/sample_ops.hip) against glowtts_prior_sample on the same index
(z bit for bit), against bincount (durations, exactly) and against tests/teacher_forced_ref.py (the score, within 4 x the error of the same restatement
evaluated in float32), at the smallest shapes where it can go wrong; batch independence and the NULL-output variants bit for bit.  Model level:
`GlowTTS.teacher_forced` on the tiny golden models of all four modes against the eval `forward`, `encode_mels` and the oracle, and its launch anatomy."""
import numpy as np
import pytest
import torch

import prior_sample_ref as PS
import teacher_forced_ref as R
from helpers import launch_counts, launch_reset, load_case, tiny_cfg
from test_gpu_prior_sample import TINY, build_tiny

pytestmark = pytest.mark.gpu
B = 6
SENTINEL = 1234.5


def composition(rng, total, parts):
    """`total` frames over `parts` tokens (zeros wherever parts > total, and elsewhere by chance)"""
    return np.bincount(rng.integers(0, parts, total), minlength=parts).astype(np.float32)


def make_case(C, Tx, Tmax, seed=0):
    """Six utterances: the full frame count, ragged ones, and row 2 without durations (the model clamps its mel length to 1; its idx is all -1)."""
    rng = np.random.default_rng(1000 * C + 10 * Tx + Tmax + seed)
    lengths = [Tmax, max(1, 2 * Tmax // 3), 0, max(1, Tmax // 3), max(1, Tmax // 2), max(1, Tmax - 1)]
    dur = np.stack([composition(rng, n, Tx) for n in lengths])
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    mean = torch.rand(B, C, Tx, generator=g) * 4 - 2
    log_std = torch.rand(B, C, Tx, generator=g) * 1.5 - 1
    z_rec = torch.randn(B, C, Tmax, generator=g) * 1.5
    seeds = torch.tensor([[1, 2], [0xFFFFFFFF, 7], [3, 4], [2499690753, 1716153205], [5, 6], [7, 8]], dtype=torch.int64)
    scales = torch.tensor([1.5, 0.7, 1.0, 0.0, 1.0, 0.667])
    return mean, log_std, torch.from_numpy(dur), torch.tensor(lengths).clamp_min(1), z_rec, seeds, scales


def raw(mean, log_std, idx, z_rec, seeds, scales, z, dur, score, partials, checked=True, dims=None):
    """The entry point itself; every argument a device tensor, an address or None.  dims: (B, C, Tx, Tmax) where mean or idx is None"""
    from glow_tts_amd import _lib
    p = lambda t: t if (t is None or isinstance(t, int)) else _lib.ptr(t)
    Bn, C, Tx, Tmax = dims if dims is not None else tuple(mean.shape) + (idx.shape[1],)
    handle = _lib.api() if checked else _lib.lib()
    return handle.glowtts_prior_sample_aligned(p(mean), p(log_std), p(idx), p(z_rec), p(seeds), p(scales), p(z), p(dur), p(score), p(partials), Bn, C, Tx,
                                               Tmax, _lib.stream())


@pytest.mark.parametrize("Tmax", [1, 63, 64, 65, 130, 256])
@pytest.mark.parametrize("Tx", [1, 7, 300])
@pytest.mark.parametrize("C", [5, 8])
def test_aligned_sample_operator(C, Tx, Tmax):
    from glow_tts_amd import abi, alignment
    assert abi.SAMPLE_TILE == 64                          # (the frame counts above sit on both sides of one tile; 130: scalar stores, 256: 16-byte stores)
    mean, log_std, dur, lengths, z_rec, seeds, scales = make_case(C, Tx, Tmax)
    c = lambda t: t.cuda()
    mean_d, ls_d, zr_d, sc_d = c(mean), c(log_std), c(z_rec), c(scales)
    want_z, idx, _ = alignment.prior_sample(mean_d, ls_d, c(dur), c(lengths), seeds, sc_d, Tmax, want_attn=False)
    z, d, score = alignment.aligned_sample(mean_d, ls_d, idx, zr_d, seeds, sc_d)
    torch.cuda.synchronize()
    idx_h = idx.cpu().numpy()
    assert (idx_h[2] == -1).all() and (idx_h[0] >= 0).all() and d.dtype == torch.int32 and d.shape == (B, Tx)
    assert torch.equal(z, want_z)                                                              # the bits glowtts_prior_sample writes for this index
    assert np.array_equal(d.cpu().numpy(), R.durations(idx_h, Tx)) and np.array_equal(d.cpu().numpy(), dur.numpy().astype(np.int32))
    if Tx > Tmax:
        assert (d[0] == 0).any()                                                               # tokens without a frame
    # the score: float64 restatement, the bar from the same restatement in float32
    args = (mean.numpy(), log_std.numpy(), idx_h, z_rec.numpy())
    s64, s32 = R.score(*args), R.score(*args, dtype=np.float32)
    scale = np.abs(s64).max()
    err, e32 = np.abs(score.cpu().numpy().astype(np.float64) - s64).max() / scale, np.abs(s32.astype(np.float64) - s64).max() / scale
    print(f"C {C} Tx {Tx} Tmax {Tmax}: score err {err:.3e}  e32 {e32:.3e}  ratio {err / (4 * e32 + 1e-300):.3f}")
    assert score[2].item() == 0.0 and s64[2] == 0.0                                            # no valid frame
    assert err <= 4 * e32, (err, e32)
    # an index beyond the token axis (and one below -1) is -1: nothing of that frame is read, its z is 0, it has no duration and no part in the score
    bad = idx.clone()
    y = min(Tmax - 1, 5)
    bad[0, y], bad[4, 0] = Tx + 5, -9
    zb, db, sb = alignment.aligned_sample(mean_d, ls_d, bad, zr_d, seeds, sc_d)
    torch.cuda.synchronize()
    want_b = want_z.clone()
    want_b[0, :, y], want_b[4, :, 0] = 0, 0
    assert torch.equal(zb, want_b) and np.array_equal(db.cpu().numpy(), R.durations(bad.cpu().numpy(), Tx))
    bad_args = (mean.numpy(), log_std.numpy(), bad.cpu().numpy(), z_rec.numpy())
    sb64, sb32 = R.score(*bad_args), R.score(*bad_args, dtype=np.float32)
    assert np.abs(sb.cpu().numpy() - sb64).max() <= 4 * np.abs(sb32 - sb64).max()
    for b in (1, 2, 3, 5):
        assert sb[b].item() == score[b].item()
    # two runs: the same bits
    z2, d2, s2 = alignment.aligned_sample(mean_d, ls_d, idx, zr_d, seeds, sc_d)
    assert torch.equal(z2, z) and torch.equal(d2, d) and torch.equal(s2, score)


@pytest.mark.parametrize("C", [5, 8])
def test_scalar_store_form_at_an_offset_view(C):
    """Tmax % 4 == 0 with z one float off a 16-byte boundary takes the one-frame-per-lane stores: the same z, and the same score bits (one summation tree)."""
    from glow_tts_amd import alignment
    Tx, Tmax = 7, 256
    mean, log_std, dur, lengths, z_rec, seeds, scales = make_case(C, Tx, Tmax)
    c = lambda t: t.cuda()
    mean_d, ls_d, zr_d, sc_d = c(mean), c(log_std), c(z_rec), c(scales)
    _, idx, _ = alignment.prior_sample(mean_d, ls_d, c(dur), c(lengths), seeds, sc_d, Tmax, want_attn=False)
    z, d, score = alignment.aligned_sample(mean_d, ls_d, idx, zr_d, seeds, sc_d)
    words = alignment.seed_words(seeds, B, mean_d.device)
    buf = torch.full((B * C * Tmax + 1,), SENTINEL, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d2, s2 = torch.empty_like(d), torch.empty_like(score)
    partials = torch.empty(B, Tmax // 64, device="cuda")
    raw(mean_d, ls_d, idx, zr_d, words, sc_d, buf.data_ptr() + 4, d2, s2, partials)
    torch.cuda.synchronize()
    assert buf[0].item() == SENTINEL and torch.equal(buf[1:].view(B, C, Tmax), z) and torch.equal(d2, d) and torch.equal(s2, score)


@pytest.mark.parametrize("C", [5, 8])
def test_batch_independence_bit_for_bit(C):
    """One utterance alone at Tmax = its own length (130: not a multiple of 4) and as row 2 of three at Tmax = 256 (a multiple of 4, a longer token axis,
    other seeds around it): its frames of z, its durations and its score have the same bits."""
    from glow_tts_amd import alignment
    Tx, n = 7, 130
    rng = np.random.default_rng(C)
    g = torch.Generator().manual_seed(C)
    dur = torch.from_numpy(composition(rng, n, Tx))[None]
    mean, log_std, z_rec = torch.randn(1, C, Tx, generator=g), torch.rand(1, C, Tx, generator=g) - 1, torch.randn(1, C, n, generator=g)
    seed, scale = torch.tensor([[123456789, 987654321]], dtype=torch.int64), torch.tensor([0.8])
    c = lambda t: t.cuda()
    _, i1, _ = alignment.prior_sample(c(mean), c(log_std), c(dur), torch.tensor([n]).cuda(), seed, c(scale), n, want_attn=False)
    z1, d1, s1 = alignment.aligned_sample(c(mean), c(log_std), i1, c(z_rec), seed, c(scale))
    Tx3, T3 = 300, 256
    mean3, ls3, zr3 = torch.randn(3, C, Tx3, generator=g), torch.rand(3, C, Tx3, generator=g) - 1, torch.randn(3, C, T3, generator=g)
    dur3 = torch.stack([torch.from_numpy(composition(rng, 256, Tx3)), torch.from_numpy(composition(rng, 77, Tx3)), torch.zeros(Tx3)])
    mean3[2, :, :Tx], ls3[2, :, :Tx], zr3[2, :, :n], dur3[2, :Tx] = mean[0], log_std[0], z_rec[0], dur[0]
    seeds3 = torch.tensor([[5, 6], [7, 8], [123456789, 987654321]], dtype=torch.int64)
    sc3 = torch.tensor([1.0, 0.3, 0.8]).cuda()
    _, i3, _ = alignment.prior_sample(c(mean3), c(ls3), c(dur3), dur3.sum(1).long().cuda(), seeds3, sc3, T3, want_attn=False)
    z3, d3, s3 = alignment.aligned_sample(c(mean3), c(ls3), i3, c(zr3), seeds3, sc3)
    torch.cuda.synchronize()
    assert torch.equal(i3[2, :n], i1[0]) and (i3[2, n:] == -1).all()
    assert torch.equal(z3[2, :, :n], z1[0]) and (z3[2, :, n:] == 0).all()
    assert torch.equal(d3[2, :Tx], d1[0]) and (d3[2, Tx:] == 0).all() and int(d1.sum()) == n
    assert s3[2].item() == s1[0].item() and s1[0].item() != 0.0


def test_null_outputs_and_argument_errors():
    from glow_tts_amd import _lib, abi, alignment
    C, Tx, Tmax = 5, 7, 65
    mean, log_std, dur, lengths, z_rec, seeds, scales = make_case(C, Tx, Tmax)
    c = lambda t: t.cuda()
    mean_d, ls_d, zr_d, sc_d = c(mean), c(log_std), c(z_rec), c(scales)
    _, idx, _ = alignment.prior_sample(mean_d, ls_d, c(dur), c(lengths), seeds, sc_d, Tmax, want_attn=False)
    z, d, score = alignment.aligned_sample(mean_d, ls_d, idx, zr_d, seeds, sc_d)
    words = alignment.seed_words(seeds, B, mean_d.device)
    # the wrapper's variants
    z_none, d1, s1 = alignment.aligned_sample(mean_d, ls_d, idx, zr_d, None, None, want_z=False)
    z2, d2, s_none = alignment.aligned_sample(mean_d, ls_d, idx, None, seeds, sc_d)
    assert z_none is None and torch.equal(d1, d) and torch.equal(s1, score) and s_none is None and torch.equal(z2, z) and torch.equal(d2, d)
    # the entry point: a NULL output is not written, whatever else is given
    fresh = lambda like: torch.full_like(like, 77)
    partials = torch.full((B, 2), SENTINEL, device="cuda")
    zz, dd = fresh(z), fresh(d)
    raw(mean_d, ls_d, idx, zr_d, words, sc_d, zz, dd, None, partials)                           # no score: the partials stay as they are
    torch.cuda.synchronize()
    assert torch.equal(zz, z) and torch.equal(dd, d) and (partials == SENTINEL).all()
    ss = fresh(score)
    raw(mean_d, ls_d, idx, zr_d, None, None, None, None, ss, partials)                          # the score alone (no seeds needed without z)
    torch.cuda.synchronize()
    assert torch.equal(ss, score) and not (partials == SENTINEL).any()
    dd = fresh(d)
    raw(mean_d, ls_d, idx, None, None, None, None, dd, None, None)                              # the durations alone
    torch.cuda.synchronize()
    assert torch.equal(dd, d)
    # argument errors: a NULL required pointer, a score without its partials or without z_rec, no output at all, B out of range
    good = [mean_d, ls_d, idx, zr_d, words, sc_d, fresh(z), fresh(d), fresh(score), partials]
    for hole in (0, 1, 2, 3, 4, 5, 9):
        row = list(good)
        row[hole] = None
        assert raw(*row, checked=False, dims=(B, C, Tx, Tmax)) == abi.E_ARG, hole
        with pytest.raises(_lib.GlowTTSHipError, match=r"glowtts_prior_sample_aligned failed with code -1"):
            raw(*row, dims=(B, C, Tx, Tmax))
    assert raw(*good[:6], None, None, None, None, checked=False) == abi.E_ARG
    many = (torch.zeros(65536, C, Tx, device="cuda"), torch.zeros(65536, C, Tx, device="cuda"), torch.zeros(65536, Tmax, dtype=torch.int32, device="cuda"))
    assert raw(*many, None, None, None, None, good[7], None, None, checked=False) == abi.E_ARG   # (B > 65535: refused before any launch)
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in good[6:9])                                              # nothing was launched


# ------------------------------------------------------------------------------------------------ whole models
def case_inputs(mode, r, n=None):
    t = lambda k: torch.from_numpy(r[k][:n]).cuda()
    spk = t("speakers") if mode in ("SE", "GR") and "speakers" in r else None
    pit = t("pitches") if mode == "GR" else None
    return t("tokens"), t("token_lengths"), t("mels"), t("mel_lengths"), spk, pit


def index_of(attn):
    """dense 0/1 attentions [B, Tx, Ty] -> the per-frame token index, -1 where a frame has no token"""
    return torch.where(attn.sum(1) > 0, attn.argmax(1), torch.full_like(attn.argmax(1), -1)).to(torch.int32)


@pytest.mark.parametrize("mode,fname", TINY)
def test_teacher_forced_f32_against_forward_and_oracle(mode, fname):
    from oracle import glowtts_ref as O
    sd, _, r = load_case(fname)
    model = build_tiny(mode, "f32", sd)
    tokens, tl, mels, ml, spk, pit = case_inputs(mode, r)
    Bn = tokens.shape[0]
    seeds = torch.tensor([PS.seed_words(7, f"U{b}", 0) for b in range(Bn)], dtype=torch.int64)
    scale = 0.667
    with torch.no_grad():
        fwd = model(tokens, tl, mels, ml, spk, None, pit)
        z_enc, z_len = model.encode_mels(mels, ml, spk, None, pit)
        tf = model.teacher_forced(tokens, tl, mels, ml, speakers=spk, pitches=pit, noise_scale=scale, seeds=seeds)
        torch.cuda.synchronize()
    attn = fwd[6]
    assert tf.idx.dtype == torch.int32 and torch.equal(tf.idx, index_of(attn))
    assert tf.durations.dtype == torch.int32 and torch.equal(tf.durations, attn.sum(2).to(torch.int32))
    assert torch.equal(tf.z, z_enc) and torch.equal(tf.mel_lengths, z_len) and tf.mels.shape == tf.z.shape
    # the oracle's composition on the host: alignment, the sample along it with the contract's noise, the inverse flows under the same conditioning
    cfg = tiny_cfg(mode)
    h = lambda x: None if x is None else x.cpu()
    o = O.forward_train(sd, cfg, h(tokens), h(tl), h(mels), h(ml), h(spk), None, h(pit))
    assert torch.equal(attn.cpu(), o["attn"])
    idx_o = index_of(o["attn"]).numpy()
    s64 = R.score(o["mean"].detach().numpy(), o["log_std"].detach().numpy(), idx_o, o["z"].detach().numpy())
    err_s = np.abs(tf.score.cpu().numpy() - s64).max()
    Ty = o["z"].shape[2]
    mask = O.mask_from_lengths((h(ml) // cfg.n_squeeze) * cfg.n_squeeze, Ty)
    noise = torch.from_numpy(np.stack([PS.noise(int(s0), int(s1), cfg.mel_dim, Ty) for s0, s1 in seeds.tolist()])).float()
    z_s = ((o["mean"] @ o["attn"]) + torch.exp(o["log_std"] @ o["attn"]) * noise * scale) * mask
    spk_o = None if spk is None else torch.nn.functional.embedding(h(spk), sd["layer_Dict.LUT.weight"])
    want, _, m2 = O.decoder(sd, z_s.detach(), mask, cfg, True, spk_o, o["prosodies"], None if pit is None or mode != "GR" else h(pit)[:, :Ty])
    want = want.masked_fill(m2 == 0.0, -cfg.max_abs_mel).detach()
    err_m = (tf.mels.cpu() - want).abs().max().item()
    print(f"{mode}: score err {err_s:.3e}, mel err {err_m:.3e}")
    assert err_s <= 1e-3, err_s
    assert tf.mels.shape == want.shape and err_m <= 2e-4, err_m
    # without reconstruction: the same alignment, no mel; uninitialised ActNorm is refused as encode_mels refuses it
    with torch.no_grad():
        lean = model.teacher_forced(tokens, tl, mels, ml, speakers=spk, pitches=pit, noise_scale=0.0, reconstruct=False)
    assert lean.mels is None and torch.equal(lean.idx, tf.idx) and torch.equal(lean.durations, tf.durations) and torch.equal(lean.score, tf.score)
    flow0 = model.layer_Dict["Decoder"].layer_Dict["Flows"][0].layers[0]
    flow0.initialized = False
    with pytest.raises(RuntimeError, match="ActNorm is not initialised"):
        model.teacher_forced(tokens, tl, mels, ml, speakers=spk, pitches=pit, noise_scale=0.0)
    flow0.initialized = True


@pytest.mark.parametrize("mode,fname", TINY)
def test_teacher_forced_bf16(mode, fname):
    """bf16: the index is the bf16 eval forward's (z bit-identical to encode_mels, the log-prior the same fp32 launch); noise_scale = 0 without seeds returns
    the inverse of the expanded mean; train mode changes nothing (eval arithmetic whatever `self.training` is)."""
    from glow_tts_amd import decoder
    sd, _, r = load_case(fname)
    model = build_tiny(mode, "bf16", sd)
    tokens, tl, mels, ml, spk, pit = case_inputs(mode, r)
    with torch.no_grad():
        fwd = model(tokens, tl, mels, ml, spk, None, pit)
        z_enc, z_len = model.encode_mels(mels, ml, spk, None, pit)
        tf = model.teacher_forced(tokens, tl, mels, ml, speakers=spk, pitches=pit, noise_scale=0.0)
        P = model._params()
        s, p = model._conditioning(P, spk, None, mels, ml)
        mean = fwd[1]                                                                          # the eval forward's expanded mean: mean[idx]
        pw, pb = model._stacks(P).pitch_weights()
        want = decoder.decoder_inverse(model.dec_cfg, dict(zip(decoder.WEIGHT_KEYS, [w.contiguous() for w in model._stacks(P).weights()])),
                                       (mean * model.Mask_Generate(z_len, mean.shape[2])).contiguous(), z_len, cond=model._stacks(P).conditioning(s, p),
                                       fill=-float(model.hp.Sound.Max_Abs_Mel), pitch=None if pw is None else (pit, pw, pb))
        model.train()
        again = model.teacher_forced(tokens, tl, mels, ml, speakers=spk, pitches=pit, noise_scale=0.0)
        model.eval()
        torch.cuda.synchronize()
    assert torch.equal(tf.idx, index_of(fwd[6])) and torch.equal(tf.z, z_enc)
    assert torch.equal(tf.mels, want)
    assert all(torch.equal(a, b) for a, b in zip(tf, again))


def add(*counts):
    out = {}
    for c in counts:
        for k, v in c.items():
            if v:
                out[k] = out.get(k, 0) + v
    return out


@pytest.mark.parametrize("mode,fname", TINY)
def test_launch_anatomy(mode, fname):
    """One teacher_forced call launches what its parts launch - encode_mels, the text encoder in eval mode, the log-prior and the alignment search (the two
    launches of `alignment.align`, without its dense path), the inverse flows - plus exactly one `prior_sample_aligned` and one `prior_score_final`;
    no `prior_sample`, no expansion, no dense path."""
    from glow_tts_amd import alignment, decoder, encoder
    sd, _, r = load_case(fname)
    model = build_tiny(mode, "f32", sd)
    tokens, tl, mels, ml, spk, pit = case_inputs(mode, r)
    seeds = torch.tensor([PS.seed_words(7, f"U{b}", 0) for b in range(tokens.shape[0])], dtype=torch.int64)
    hp = model.hp

    def counted(fn):
        torch.cuda.synchronize()
        launch_reset()
        out = fn()
        torch.cuda.synchronize()
        return out, {k: v for k, v in launch_counts().items() if v}

    with torch.no_grad():
        run = lambda: model.teacher_forced(tokens, tl, mels, ml, speakers=spk, pitches=pit, noise_scale=0.667, seeds=seeds)
        first = run()                                                                          # (the caches of the model are warm from here on)
        tf, total = counted(run)
        (z, z_len), c_encode = counted(lambda: model.encode_mels(mels, ml, spk, None, pit))
        P, stacks, prep, pitch = model._decoder_pass_inputs(mels, ml, pit)
        s, p = model._conditioning(P, spk, None, mels, ml)
        cond = stacks.conditioning(s, p)
        mask = model.Mask_Generate(tl, tokens.shape[1])
        (mean, log_std, _), c_text = counted(lambda: encoder.encoder_forward(P, hp, tokens, mask, s, p, False, precision=model.dec_cfg.precision,
                                                                             cache=model._enc_cache))

        def search():
            value_t, tx, ty = alignment.log_prior_t(mean, log_std, z, tl, ml, int(hp.Decoder.Num_Squeeze), return_lengths=True)
            return alignment.maximum_path_t(value_t, tx, ty)
        idx, c_search = counted(search)
        _, c_align = counted(lambda: alignment.align(mean, log_std, z, tl, ml, int(hp.Decoder.Num_Squeeze)))
        sample, _, _ = alignment.aligned_sample(mean, log_std, idx, z, seeds, torch.full((tokens.shape[0],), 0.667, device="cuda"))
        _, c_inverse = counted(lambda: decoder.decoder_inverse(model.dec_cfg, None, sample, z_len, cond=cond, fill=-float(hp.Sound.Max_Abs_Mel), prep=prep,
                                                               pitch=pitch))
    assert all(torch.equal(a, b) for a, b in zip(first, tf)) and torch.equal(idx, tf.idx)
    assert add(c_search, {"mas_path_from_idx": 1}) == c_align, (c_search, c_align)              # `align` = these two launches + its dense path
    want = add(c_encode, c_text, c_search, c_inverse, {"prior_sample_aligned": 1, "prior_score_final": 1})
    assert total == want, (total, want)
    assert total["prior_sample_aligned"] == 1 and total["prior_score_final"] == 1 and "prior_dur" not in total
    assert not any(k == "prior_sample" or k.startswith("expand_") or k.startswith("mas_path") for k in total), total
