"""CPU tests of tests/flow_ops_ref.py: (1) the layout converters round-trip and the rows-layout references agree with the oracle functions they wrap
to 1e-12; (2) mutation checks - a deliberately wrong result, cast to fp32 like a kernel's output, must be REJECTED by the comparison helper that
tests/test_gpu_flow_ops.py will hold the kernels to.  The bars themselves are derived in flow_ops_ref.py, not measured."""
import pytest
import torch

import flow_ops_ref as R
from oracle import glowtts_ref as O

F64 = torch.float64
SHAPES = {"small": (1, 33, 12), "medium": (4, 400, 160)}          # (B, T, C): 37 rows / 1616 rows, the shapes of the GPU file


def _case(shape, **kw):
    B, T, C = SHAPES[shape]
    return R.make_case(B, T, C, seed=7 + C, **kw)


def to32(t):
    return t.to(torch.float32)


# ------------------------------------------------------------------------------------------------------ reference agreement
@pytest.mark.parametrize("B,C,T", [(1, 4, 1), (3, 12, 7), (2, 20, 16)])
def test_rows_layout_roundtrip(B, C, T):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, T, generator=g, dtype=F64)
    rows = R.to_rows(x, fill=9.0)
    assert rows.shape == (B, T + 4, C)
    assert bool((rows[:, :2] == 9).all()) and bool((rows[:, T + 2:] == 9).all())
    assert torch.equal(R.from_rows(rows), x)
    assert torch.equal(rows[:, 2:T + 2, :], x.transpose(1, 2))
    mask = O.mask_from_lengths(torch.tensor([T] + [max(T - 2, 0)] * (B - 1)), T).to(F64)
    rm = R.mask_to_rows(mask)
    assert rm.shape == (B, T + 4) and float(rm.sum()) == float(mask.sum()) and bool((rm[:, :2] == 0).all())


@pytest.mark.parametrize("C,pad_slots", [(8, 28), (24, 20), (56, 4), (160, 16), (20, 22), (164, 14), (264, 28), (1024, 0)])
def test_pair_packing_roundtrip_and_pad_columns(C, pad_slots):
    C2, ldo = C // 2, R.pair_ldo(C)
    assert ldo % 64 == 0 and ldo >= C and ldo - C < 64
    g = torch.Generator().manual_seed(C)
    m, lg = torch.randn(5, C2, generator=g, dtype=F64), torch.randn(5, C2, generator=g, dtype=F64)
    p = R.pair_pack(m, lg, ldo + 64, fill=3.0)
    m2, lg2 = R.pair_unpack(p, C2)
    assert torch.equal(m, m2) and torch.equal(lg, lg2)
    for j in (0, min(31, C2 - 1), C2 - 1):
        assert float(p[2, (j >> 5) * 64 + (j & 31)]) == float(m[2, j]) and float(p[2, (j >> 5) * 64 + (j & 31) + 32]) == float(lg[2, j])
    assert R.pair_pad_cols(C2, ldo).numel() == 2 * pad_slots
    pads = R.pair_pad_cols(C2, ldo + 64)
    assert pads.numel() == 2 * pad_slots + 64 and bool((p[:, pads] == 3.0).all())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_actnorm_inv1x1_rows_reference_is_the_oracle(shape):
    """The flat-rows wrapper against O.actnorm / O.inv1x1 on the [B, C, T] tensors they were pinned on, forward and reverse; and the explicit
    channel grouping against the oracle's view / permute form."""
    c = _case(shape, garbage=0.0)
    x3 = R.from_rows(c.x.view(c.B, c.Tp, c.C))
    mask = R.from_rows(c.rowmask2.unsqueeze(-1))
    sd = {"a.logs": c.logs.view(1, -1, 1), "a.bias": c.bias.view(1, -1, 1), "w.weight": c.W}
    cfg = O.Cfg()
    y, _ = O.actnorm(sd, "a", x3, mask, False)
    z, _ = O.inv1x1(sd, "w", y, mask, cfg, False)
    got = R.actnorm_inv1x1(c.x, c.logs, c.bias, c.W, c.rowmask)
    assert (R.from_rows(got.view(c.B, c.Tp, c.C)) - z).abs().max() <= 1e-12
    assert bool((got[c.rowmask == 0] == 0).all())
    u, _ = O.inv1x1(sd, "w", z, mask, cfg, True)
    back, _ = O.actnorm(sd, "a", u, mask, True)
    got_back = R.actnorm_inv1x1(got, c.logs, c.bias, c.W, c.rowmask, reverse=True)
    assert (R.from_rows(got_back.view(c.B, c.Tp, c.C)) - back).abs().max() <= 1e-12
    assert ((got_back - c.x) * c.rowmask[:, None]).abs().max() <= 1e-12
    with_inv = R.actnorm_inv1x1(got, c.logs, c.bias, c.W, c.rowmask, reverse=True, Winv=torch.linalg.inv(c.W))
    assert (with_inv - got_back).abs().max() <= 1e-12
    yv = (c.bias + torch.exp(c.logs) * c.x) * c.rowmask[:, None]
    assert (R.mix_by_groups(yv, c.W) - got).abs().max() <= 1e-12


def _tiny_coupling_sd(C, H, g, flows=1):
    """Decoder weights whose End conv has a zero weight: (m, logs) of every coupling are then the End bias, whatever the WaveNet computes."""
    sd = {}
    for f in range(flows):
        q = f"layer_Dict.Decoder.layer_Dict.Flows.{f}.layers"
        sd[q + ".0.logs"] = torch.randn(1, C, 1, generator=g, dtype=F64) * 0.1
        sd[q + ".0.bias"] = torch.randn(1, C, 1, generator=g, dtype=F64) * 0.1
        sd[q + ".1.weight"] = R.well_conditioned_4x4(g)[0]
        for name, o, i in (("Start", H, C // 2), ("WaveNet.layer_Dict.In_0", 2 * H, H), ("WaveNet.layer_Dict.Res_Skip_0", H, H)):
            sd[f"{q}.2.layer_Dict.{name}.weight_v"] = torch.randn(o, i, 1, generator=g, dtype=F64)
            sd[f"{q}.2.layer_Dict.{name}.weight_g"] = torch.rand(o, 1, 1, generator=g, dtype=F64) + 0.5
            sd[f"{q}.2.layer_Dict.{name}.bias"] = torch.randn(o, generator=g, dtype=F64) * 0.1
        sd[f"{q}.2.layer_Dict.End.weight"] = torch.zeros(C, H, 1, dtype=F64)
        sd[f"{q}.2.layer_Dict.End.bias"] = torch.randn(C, generator=g, dtype=F64) * 0.3
    return sd


def test_coupling_affine_and_decoder_logdet_are_the_oracle():
    """coupling_affine against O.coupling, decoder_logdet against O.decoder's log-determinant (2 flows), with constant (m, logs)."""
    g = torch.Generator().manual_seed(5)
    C, H, B, T = 12, 4, 3, 9
    cfg = O.Cfg(mel_dim=C // 2, n_flows=2, wn_channels=H, wn_layers=1, wn_kernel=1)
    sd = _tiny_coupling_sd(C, H, g, flows=2)
    lens_sq = torch.tensor([9, 4, 0])
    mask = O.mask_from_lengths(lens_sq, T).to(F64)
    x = torch.randn(B, C, T, generator=g, dtype=F64)
    q = "layer_Dict.Decoder.layer_Dict.Flows.0.layers.2"
    z, ld = O.coupling(sd, q, x, mask, cfg, False)
    eb = sd[q + ".layer_Dict.End.bias"]
    xr, rm = R.to_rows(x).reshape(-1, C), R.mask_to_rows(mask).reshape(-1)
    zb, ldr = R.coupling_affine(xr[:, C // 2:], eb[:C // 2].expand(len(rm), -1), eb[C // 2:].expand(len(rm), -1), rm)
    assert (R.from_rows(zb.view(B, T + 4, C // 2)) - z[:, C // 2:]).abs().max() <= 1e-12
    assert (ldr.view(B, T + 4).sum(1) - ld).abs().max() <= 1e-12
    mel = torch.randn(B, C // 2, 2 * T, generator=g, dtype=F64)
    _, want, _ = O.decoder(sd, mel, O.mask_from_lengths(2 * lens_sq, 2 * T).to(F64), cfg)
    logs_all = torch.stack([sd[f"layer_Dict.Decoder.layer_Dict.Flows.{f}.layers.0.logs"].flatten() for f in range(2)])
    W_all = torch.stack([sd[f"layer_Dict.Decoder.layer_Dict.Flows.{f}.layers.1.weight"] for f in range(2)])
    outs_logs = torch.stack([sd[f"layer_Dict.Decoder.layer_Dict.Flows.{f}.layers.2.layer_Dict.End.bias"][C // 2:].expand(B, T + 4, -1) for f in range(2)])
    got, sumabs = R.decoder_logdet(outs_logs, logs_all, W_all, R.mask_to_rows(mask), C)
    assert (got - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max()))
    assert bool((sumabs >= got.abs() - 1e-12).all())


@pytest.mark.parametrize("ns,Tm,Cm", [(1, 7, 5), (2, 9, 3), (2, 8, 1), (3, 10, 4)])
def test_squeeze_rows_reference_is_the_oracle(ns, Tm, Cm):
    g = torch.Generator().manual_seed(ns * 100 + Tm)
    B = 3
    mel = torch.randn(B, Cm, Tm, generator=g, dtype=F64)
    lens = torch.tensor([Tm, max(Tm - 3, 1), ns - 1 if ns > 1 else 1])
    rows, rm = R.squeeze_rows(mel, lens, ns)
    T = Tm // ns
    assert rows.shape == (B, T + 4, ns * Cm) and rm.shape == (B, T + 4)
    for b in range(B):
        for t in range(T):
            valid = ns * t + ns - 1 < int(lens[b])
            assert float(rm[b, 2 + t]) == float(valid)
            for s in range(ns):
                want = mel[b, :, ns * t + s] * float(valid)
                assert torch.equal(rows[b, 2 + t, s * Cm:(s + 1) * Cm], want)
    back = R.unsqueeze_rows(rows, lens, Tm, ns)
    maskf = O.mask_from_lengths(lens, Tm).to(F64)
    sq, sm = O.squeeze(mel, maskf, ns)
    want_back, _ = O.unsqueeze(sq, sm, ns)
    assert torch.equal(back, want_back)
    filled = R.unsqueeze_rows(R.to_rows(R.from_rows(rows), fill=5.0) + (1 - rm)[..., None] * 77.0, lens, Tm, ns, fill=-4.0)
    m_un = sm.unsqueeze(-1).repeat(1, 1, 1, ns).view(B, 1, T * ns).bool()
    assert torch.equal(filled, torch.where(m_un, want_back, torch.full_like(want_back, -4.0)))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_actnorm_init_and_param_grad_references(shape):
    c = _case(shape, garbage=0.0)
    x3, mask = R.from_rows(c.x.view(c.B, c.Tp, c.C)), R.from_rows(c.rowmask2.unsqueeze(-1))
    wl, wb = O.actnorm_init(x3, mask)
    gl, gb = R.actnorm_init(c.x, c.rowmask)
    assert (gl - wl.flatten()).abs().max() <= 1e-12 and (gb - wb.flatten()).abs().max() <= 1e-12
    st, sa = R.colstats(c.x, c.rowmask)
    den = st[-1]
    assert float(den) == float(c.rowmask.sum()) and bool((sa >= st.abs()).all())
    var = (st[c.C:2 * c.C] / den - (st[:c.C] / den) ** 2).clamp_min(1e-7)
    assert (-0.5 * torch.log(var) - gl).abs().max() <= 1e-12
    # closed form of the log-determinant terms of the parameter gradients
    g = torch.Generator().manual_seed(3)
    F_ = 2
    logs_all, W_all = torch.randn(F_, c.C, generator=g, dtype=F64) * 0.2, R.well_conditioned_4x4(g, F_)
    d_an = torch.randn(F_, 2 * c.C + 16, generator=g, dtype=F64)
    dlogs, dbias, dW, s, sabs = R.decoder_param_grads(d_an, c.dld, logs_all, W_all, c.lens_sq, c.C)
    assert abs(float(s) - float((c.dld * c.lens_sq).sum())) <= 1e-12 * float(sabs) + 1e-300
    assert (dlogs - (d_an[:, :c.C] + s)).abs().max() <= 1e-10 and torch.equal(dbias, d_an[:, c.C:2 * c.C])
    want_w = d_an[:, 2 * c.C:].view(F_, 4, 4) + s * (c.C / 4) * torch.linalg.inv(W_all).transpose(1, 2)
    assert (dW - want_w).abs().max() <= 1e-9 * max(1.0, float(want_w.abs().max()))


@pytest.mark.parametrize("F_", [1, 12, 65])
def test_pivot_matrices_do_what_their_names_say(F_):
    """The weights the GPU test hands glowtts_inv1x1_prepare: cond < 100, and the pivoting kinds really need a row exchange in column 0."""
    W = R.pivot_matrices(F_, seed=F_)
    assert float(torch.linalg.cond(W).max()) < 100
    for f in range(F_):
        kind, w = R.PIVOT_KINDS[f % len(R.PIVOT_KINDS)], W[f]
        if kind in ("zero_corner", "largest_last"):
            assert float(w[0, 0].abs()) < float(w[:, 0].abs().max())
        if kind == "largest_last":
            assert int(w[:, 0].abs().argmax()) == 3
        if kind == "permutation":
            assert sorted(w.sum(0).tolist()) == [1.0] * 4 and float(w.abs().sum()) == 4.0
        if kind == "negative_diagonal":
            assert float(torch.linalg.slogdet(w)[0]) == -1.0
    assert torch.equal(W, R.f32(W))


def test_backward_references_match_their_closed_forms():
    """The autograd references against the formulas in the kernels' comments (dx = W^T dz e m, ...), so that a wrong sign or transpose in the
    wrapper cannot pass as `the reference`."""
    c = _case("small")
    dx, dlogs, dbias, dW = R.actnorm_inv1x1_bwd(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    m = c.rowmask[:, None]
    d = torch.where(m.bool(), c.dz, torch.zeros_like(c.dz))
    xv = torch.where(m.bool(), c.x, torch.zeros_like(c.x))
    dy = R.mix_by_groups(d, c.W.t())
    e = torch.exp(c.logs)
    assert (dx - dy * e).abs().max() <= 1e-12 and bool((dx[c.rowmask == 0] == 0).all())
    assert (dlogs - (dy * e * xv).sum(0)).abs().max() <= 1e-11 and (dbias - dy.sum(0)).abs().max() <= 1e-11
    y = (c.bias + e * xv) * m
    ch = R.group_channels(c.C)
    assert (dW - torch.einsum("rag,rkg->ak", d[:, ch], y[:, ch])).abs().max() <= 1e-11
    sc = R.actnorm_inv1x1_bwd_scale(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    for got, bound in zip((dx, dlogs, dbias, dW), sc):
        assert bool((bound >= got.abs() - 1e-12).all())
    xb = c.xmid[:, c.C2:]
    dxb, dm, dlg = R.coupling_bwd(c.dz[:, c.C2:], xb, c.m, c.lg, c.rowmask, c.dld_rows)
    dzb = d[:, c.C2:]
    el = torch.exp(c.lg)
    assert (dxb - dzb * el * m).abs().max() <= 1e-9 and (dm - dzb).abs().max() <= 1e-12
    want_l = torch.where(m.bool(), dzb * el * xb + c.dld_rows[:, None], torch.zeros_like(dzb))
    assert (dlg - want_l).abs().max() <= 1e-9 * max(1.0, float(want_l.abs().max()))


# ------------------------------------------------------------------------------------------------------------- mutations
def _drop_one_valid_row(rowmask):
    m = rowmask.clone()
    valid = torch.nonzero(m > 0).flatten()
    m[valid[len(valid) // 2]] = 0
    return m


def _reduction_rejects(mut, want, sumabs, min_fraction=0.9):
    """The helper raises, and at least 90 % of the elements are outside the bar (a fault in a sum over rows may hide under tol in a few channels)."""
    with pytest.raises(AssertionError):
        R.assert_reduction(to32(mut), want, sumabs)
    assert R.rejected_fraction(to32(mut), want, sumabs) >= min_fraction


def _mut_row_dropped(c):
    want = R.actnorm_inv1x1_bwd(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    sc = R.actnorm_inv1x1_bwd_scale(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    mut = R.actnorm_inv1x1_bwd(c.dz, c.x, c.logs, c.bias, c.W, _drop_one_valid_row(c.rowmask))
    for k in (1, 2, 3):                                            # dlogs, dbias, dW
        R.assert_reduction(to32(want[k]), want[k], sc[k])
        _reduction_rejects(mut[k], want[k], sc[k])
    st, sa = R.colstats(c.x, c.rowmask)
    R.assert_reduction(to32(st), st, sa)
    _reduction_rejects(R.colstats(c.x, _drop_one_valid_row(c.rowmask))[0], st, sa)
    outs_logs = c.lg.view(1, c.B, c.Tp, c.C2)
    ld, la = R.decoder_logdet(outs_logs, c.logs[None], c.W[None], c.rowmask2, c.C)
    R.assert_reduction(to32(ld), ld, la)
    # (one row dropped from the coupling's sum of ONE utterance: that utterance must be rejected)
    m2 = _drop_one_valid_row(c.rowmask).view(c.B, c.Tp)
    mut_ld = R.decoder_logdet(outs_logs, c.logs[None], c.W[None], c.rowmask2, c.C)[0] - (outs_logs[0] * (c.rowmask2 - m2)[..., None]).sum((1, 2))
    with pytest.raises(AssertionError):
        R.assert_reduction(to32(mut_ld), ld, la)


def _mut_rowmask_shifted(c):
    shifted = torch.roll(c.rowmask, 1)
    want, scale = R.actnorm_inv1x1(c.x, c.logs, c.bias, c.W, c.rowmask), R.actnorm_inv1x1_scale(c.x, c.logs, c.bias, c.W, c.rowmask)
    R.assert_elementwise(to32(want), want, scale)
    with pytest.raises(AssertionError):
        R.assert_elementwise(to32(R.actnorm_inv1x1(c.x, c.logs, c.bias, c.W, shifted)), want, scale)
    xb, dzb = c.xmid[:, c.C2:], c.dz[:, c.C2:]
    wantc, sc = R.coupling_bwd(dzb, xb, c.m, c.lg, c.rowmask, c.dld_rows), R.coupling_bwd_scale(dzb, xb, c.m, c.lg, c.rowmask, c.dld_rows)
    mutc = R.coupling_bwd(dzb, xb, c.m, c.lg, shifted, c.dld_rows)
    for k in range(3):
        R.assert_elementwise(to32(wantc[k]), wantc[k], sc[k])
        with pytest.raises(AssertionError):
            R.assert_elementwise(to32(mutc[k]), wantc[k], sc[k])
    wantb, sb = R.actnorm_inv1x1_bwd(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask), R.actnorm_inv1x1_bwd_scale(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    mutb = R.actnorm_inv1x1_bwd(c.dz, c.x, c.logs, c.bias, c.W, shifted)
    R.assert_elementwise(to32(wantb[0]), wantb[0], sb[0])
    with pytest.raises(AssertionError):
        R.assert_elementwise(to32(mutb[0]), wantb[0], sb[0])
    st, sa = R.colstats(c.x, c.rowmask)
    with pytest.raises(AssertionError):
        R.assert_reduction(to32(R.colstats(c.x, shifted)[0]), st, sa)


def _mut_grouping(c):
    want, scale = R.actnorm_inv1x1(c.x, c.logs, c.bias, c.W, c.rowmask), R.actnorm_inv1x1_scale(c.x, c.logs, c.bias, c.W, c.rowmask)
    m = c.rowmask[:, None]
    y = torch.where(m.bool(), c.bias + torch.exp(c.logs) * c.x, torch.zeros_like(c.x))
    R.assert_elementwise(to32(R.mix_by_groups(y, c.W)), want, scale)
    with pytest.raises(AssertionError):
        R.assert_elementwise(to32(R.mix_by_groups(y, c.W, wrong=True)), want, scale)
    wantb, sb = R.actnorm_inv1x1_bwd(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask), R.actnorm_inv1x1_bwd_scale(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    d = torch.where(m.bool(), c.dz, torch.zeros_like(c.dz))
    with pytest.raises(AssertionError):
        R.assert_elementwise(to32(R.mix_by_groups(d, c.W.t(), wrong=True) * torch.exp(c.logs)), wantb[0], sb[0])
    ch = R.group_channels(c.C, wrong=True)
    _reduction_rejects(torch.einsum("rag,rkg->ak", d[:, ch], y[:, ch]), wantb[3], sb[3], min_fraction=0.75)       # dW: 16 entries


def _mut_w_transposed(c):
    wantb, sb = R.actnorm_inv1x1_bwd(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask), R.actnorm_inv1x1_bwd_scale(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    m = c.rowmask[:, None]
    d = torch.where(m.bool(), c.dz, torch.zeros_like(c.dz))
    e = torch.exp(c.logs)
    R.assert_elementwise(to32(R.mix_by_groups(d, c.W.t()) * e), wantb[0], sb[0])
    bad_dy = R.mix_by_groups(d, c.W)                                   # W used where W^T belongs
    with pytest.raises(AssertionError):
        R.assert_elementwise(to32(bad_dy * e), wantb[0], sb[0])
    _reduction_rejects(bad_dy.sum(0), wantb[2], sb[2])                  # dbias
    _reduction_rejects(wantb[3].t().contiguous(), wantb[3], sb[3], min_fraction=0.5)      # dW transposed (its diagonal stays)
    # ... and in the parameter gradient's log-determinant term: s (C/4) W^-1 instead of its transpose
    d_an = torch.zeros(1, 2 * c.C + 16, dtype=F64)
    _, _, dW, s, sabs = R.decoder_param_grads(d_an, c.dld, c.logs[None], c.W[None], c.lens_sq, c.C)
    winv = torch.linalg.inv(c.W)
    sc = sabs * (c.C / 4) * winv.t().abs()[None]
    R.assert_reduction(to32(dW), dW, sc)
    with pytest.raises(AssertionError):
        R.assert_reduction(to32(s * (c.C / 4) * winv[None]), dW, sc)


def _mut_winv_row_exchange(c):
    g = torch.Generator().manual_seed(11)
    W = R.well_conditioned_4x4(g, 3)
    W[0, 0, 0] = 0.0                                                   # column 0 needs a pivot from below
    W[1] = W[1][[1, 2, 3, 0]]                                          # ... the largest entry of column 0 moves
    winv, logabs, sign = R.inv1x1_prepare(W)
    R.assert_inverse(to32(winv), to32(logabs), to32(sign), W)
    # a Gauss-Jordan that exchanged rows of the left half only: the inverse of P W = W^-1 P^T, two columns of W^-1 exchanged
    for f in range(3):
        piv = int(W[f, :, 0].abs().argmax()) or 1
        bad = winv.clone()
        bad[f][:, [0, piv]] = winv[f][:, [piv, 0]]
        with pytest.raises(AssertionError):
            R.assert_inverse(to32(bad), to32(logabs), to32(sign), W)
    Wn = W.clone()
    Wn[2, 1] = -Wn[2, 1]
    wi, la, sg = R.inv1x1_prepare(Wn)
    assert float(sg[2]) == -1.0
    R.assert_inverse(to32(wi), to32(la), to32(sg), Wn)
    with pytest.raises(AssertionError):                                # the sign word: a negative determinant reported as positive
        R.assert_inverse(to32(wi), to32(la), to32(sg.abs()), Wn)


def _mut_logdet_len(c):
    outs_logs = c.lg.view(1, c.B, c.Tp, c.C2)
    ld, la = R.decoder_logdet(outs_logs, c.logs[None], c.W[None], c.rowmask2, c.C)
    R.assert_reduction(to32(ld), ld, la)
    assert int(c.lens[0]) // c.ns != int(c.lens[0])
    mut, _ = R.decoder_logdet(outs_logs, c.logs[None], c.W[None], c.rowmask2, c.C, lens_from=c.lens)       # len, not len // ns
    with pytest.raises(AssertionError):
        R.assert_reduction(to32(mut), ld, la)
    d_an = torch.zeros(1, 2 * c.C + 16, dtype=F64)
    dlogs, _, _, s, sabs = R.decoder_param_grads(d_an, c.dld, c.logs[None], c.W[None], c.lens_sq, c.C)
    bad = R.decoder_param_grads(d_an, c.dld, c.logs[None], c.W[None], c.lens, c.C)[0]
    with pytest.raises(AssertionError):
        R.assert_reduction(to32(bad), dlogs, sabs.expand_as(dlogs))


def _mut_douts_pad(c):
    xb, dzb = c.xmid[:, c.C2:], c.dz[:, c.C2:]
    _, dm, dlg = R.coupling_bwd(dzb, xb, c.m, c.lg, c.rowmask, c.dld_rows)
    for extra in (0, 64):
        packed = to32(R.pair_pack(dm, dlg, c.ldo + extra))
        R.assert_pair_pads_zero(packed, c.C2)
        pads = R.pair_pad_cols(c.C2, c.ldo + extra)
        for col in (int(pads[0]), int(pads[-1])):
            bad = packed.clone()
            bad[c.R // 2, col] = 1e-30
            with pytest.raises(AssertionError):
                R.assert_pair_pads_zero(bad, c.C2)
        bad16 = packed.to(torch.bfloat16)
        bad16[0, int(pads[len(pads) // 2])] = 1.0
        with pytest.raises(AssertionError):
            R.assert_pair_pads_zero(bad16, c.C2)


MUTATIONS = {
    "valid_row_dropped_from_reduction": _mut_row_dropped,
    "rowmask_shifted_by_one_frame": _mut_rowmask_shifted,
    "channel_grouping_4g_instead_of_split_halves": _mut_grouping,
    "W_used_where_W_transposed_belongs": _mut_w_transposed,
    "W_inverse_with_row_exchange_undone": _mut_winv_row_exchange,
    "logdet_len_not_divided_by_squeeze": _mut_logdet_len,
    "douts_pad_column_left_nonzero": _mut_douts_pad,
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_mutation_is_rejected(mutation, shape):
    MUTATIONS[mutation](_case(shape))


def test_helpers_reject_nan_and_unwritten_outputs():
    want = torch.ones(4, 3, dtype=F64)
    got = torch.ones(4, 3)
    assert R.assert_elementwise(got, want, want) == 0.0 and R.assert_reduction(got, want, want) == 0.0
    got[2, 1] = float("nan")
    with pytest.raises(AssertionError):
        R.assert_elementwise(got, want, want)
    with pytest.raises(AssertionError):
        R.assert_reduction(got, want, want)
    with pytest.raises(AssertionError):                                # zero scale (a masked row): exactly zero or nothing
        R.assert_elementwise(torch.full((2,), 1e-30), torch.zeros(2, dtype=F64), torch.zeros(2, dtype=F64))
    with pytest.raises(AssertionError):
        R.assert_bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    R.assert_bits_equal(torch.tensor([1.5, 2.0]), torch.tensor([1.5, 2.0]))


def test_decoder_config_names_the_channel_constraint():
    """Mel_Dim * Num_Squeeze must be a multiple of 8: the Start conv and its weight gradient read the C/2 pass-through channels in 4-channel granules
    (glowtts_conv_cl / glowtts_wgrad_cl return an argument error for ca % 4 != 0).  The constructor says so instead of the first launch."""
    from glow_tts_amd.decoder import DecoderConfig
    for mel_dim in (10, 14, 50):
        with pytest.raises(ValueError, match="multiple of 8"):
            DecoderConfig(mel_dim, 3, 2, 4, 32, 2, 5)
    assert DecoderConfig(12, 3, 2, 4, 32, 2, 5).C == 24 and DecoderConfig(80, 12, 2, 4, 192, 4, 5).C == 160
