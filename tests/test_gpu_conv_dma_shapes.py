"""conv_dma_kernel (csrc/gemm_cl.hip: the LDS-DMA conv on 16x16x32 bf16 MFMAs) over every instantiation glowtts_conv_cl dispatches to, at the
smallest shapes where it can go wrong (the kernel takes rows >= 128 and npad % 64 == 0):

  rows     R = 3 * (61 + 4) = 195 and R = 2 * (126 + 4) = 260: a partial last 32-row fragment, a partial last workgroup, utterance seams inside
           a tile, a masked tail (rowmask);
  columns  npad 64 (one strip), 192 (three strips; at k = 3 the 32-column strips of dma_prefers_32), 384;
  K        32 (one chunk: the rotated stage order degenerates), 64, 192, 384, 768 (the FFN's 768 -> 192 at k = 3); one tap: even chunk
           counts, and the dual-source gate derivative (ca1 = 192 of 384).

LINEAR is held to float64.  Inputs are bf16 values, so every product is exact in fp32 and only the fp32 summation rounds: for ANY summation order
|err| <= (K * taps) * 2^-23 * sum |a| |w| per output, plus half a bf16 ulp (2^-8 |ref|, itself widened by the fp32 bound) where the output is stored
as bf16.  GATE / RESSKIP / DGATE / COUPLE are compared with the same call on fp32-stored operands, which runs conv_cl_kernel, with the tolerances of
test_gpu_conv.py::test_bf16_activation_storage_matches_fp32_storage: 2^-7 on gates; allclose(1e-5, 1e-5) on fp32 outputs, that test's allowance for
the two kernels' different summation order; on bf16 outputs that same allowance on the fp32 value in front of the rounding plus one bf16 rounding
(2^-7 |x|: a value next to a rounding boundary may land on either neighbour).  The launch log proves which kernel served each call."""
import pytest
import torch

from helpers import launch_counts, launch_reset

pytestmark = pytest.mark.gpu

SHAPES = {195: (3, 61), 260: (2, 126)}        # rows -> (utterances, frames); rows = B * (T + 4)
bf = lambda t: t.to(torch.bfloat16)


def _rowmask(R):
    B, T = SHAPES[R]
    m = torch.zeros(B, T + 4)
    m[:, 2:T + 2] = 1
    m[1, T - 9:] = 0                          # a masked tail inside the second utterance
    return m.reshape(-1)


def _served_by(name, fn):
    launch_reset()
    fn()
    torch.cuda.synchronize()
    counts = launch_counts()
    assert counts.get(name, 0) == 1 and not any(k.startswith(("conv_cl<", "conv_skinny")) for k in counts), (name, counts)


def _only_conv_cl(fn):
    launch_reset()
    fn()
    torch.cuda.synchronize()
    counts = launch_counts()
    assert not any(k.startswith("conv_dma<") for k in counts) and any(k.startswith("conv_cl<") for k in counts), counts


def _one_bf16_rounding(got16, want32):
    want = bf(want32).float()
    d, tol = (got16.float() - want).abs(), 2.0 ** -7 * want.abs() + 1e-5 * (1 + want32.abs())
    print(f"bf16 output: worst |d| - tol = {(d - tol).max().item():.3e}")
    return bool((d <= tol).all())


def _linear_f64(a, w, mask, pad):
    """rows are one long sequence for the kernel (a seam is just a row): y[r, n] = mask[r] * sum_t sum_c a[r + t - pad, c] w[n, c, t], and the
    same sum over |a| |w|.  Rows before 0 / after R - 1 are taken as zero; the kernel clamps them instead, which only reaches the outermost
    pad rows of the first / last utterance - masked here as in every consumer."""
    R, C = a.shape
    a64, w64 = a.double().cpu(), w.double().cpu()
    taps = w.shape[2]
    y = torch.zeros(R, w.shape[0], dtype=torch.float64)
    s = torch.zeros_like(y)
    for t in range(taps):
        sh = torch.zeros_like(a64)
        lo, hi = max(0, pad - t), min(R, R + pad - t)
        sh[lo:hi] = a64[lo + t - pad:hi + t - pad]
        y += sh @ w64[:, :, t].T
        s += sh.abs() @ w64[:, :, t].abs().T
    m = mask.double().cpu()[:, None]
    return y * m, s * m


@pytest.mark.parametrize("R,K,N,taps,out_bf", [
    (195, 32, 64, 5, False),          # one chunk, one strip
    (260, 192, 192, 5, False),        # the In_l data gradient's shape: 64-column strips, three of them
    (195, 64, 384, 5, True),
    (195, 768, 192, 3, False),        # the encoder FFN's 768 -> 192: 32-column strips (NI = 1)
    (260, 32, 64, 3, True),
    (2808, 32, 384, 3, False),        # enough tiles that k = 3 keeps its 64-column strips (NI = 2); 2808 = 2 * (1400 + 4)
    (195, 64, 192, 1, False),         # one stage of two chunks
    (260, 384, 64, 1, True),
    (195, 192, 384, 1, False),
])
def test_linear_against_float64(R, K, N, taps, out_bf):
    from glow_tts_amd import ops
    g = torch.Generator().manual_seed(R + K + N + taps)
    if R in SHAPES:
        mask = _rowmask(R)
    else:
        mask = torch.zeros(2, R // 2); mask[:, 2:-2] = 1; mask = mask.reshape(-1)
    a = bf(torch.randn(R, K, generator=g))
    w = bf(torch.randn(N, K, taps, generator=g) / (K * taps) ** 0.5).float()
    pw = ops.pack_weight(w.cuda(), precision=ops.BF16)
    assert pw.npad == N
    out = torch.full((R, N), float("nan"), device="cuda", dtype=torch.bfloat16 if out_bf else torch.float32)
    pad = (taps - 1) // 2
    ad, md = a.cuda(), mask.cuda()
    _served_by(f"conv_dma<LINEAR,{taps}>", lambda: ops.conv_cl(ad, pw, K, R, pad=pad, epi=ops.EPI_LINEAR, flags=ops.F_MASK, n=N, rowmask=md, out0=out,
                                                              ld0=N, io_flags=ops.IO_A_BF16 | (ops.IO_OUT0_BF16 if out_bf else 0)))
    ref, sabs = _linear_f64(a, w, mask, pad)
    bound = (K * taps) * 2.0 ** -23 * sabs
    if out_bf:
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)
    err = (out.cpu().double() - ref).abs()
    worst = (err - bound).max().item()
    print(f"R={R} K={K} N={N} taps={taps}: max err {err.max().item():.3e}, max bound {bound.max().item():.3e}, worst margin {worst:.3e}")
    assert bool((err <= bound).all()), worst


@pytest.mark.parametrize("R,C,H,taps", [(195, 32, 32, 5), (260, 192, 96, 5), (195, 64, 192, 5), (260, 384, 32, 3), (195, 64, 96, 3)])
def test_gate_matches_fp32_storage(R, C, H, taps):
    from glow_tts_amd import ops
    B, T = SHAPES[R]
    g = torch.Generator().manual_seed(R + C + H + taps)
    rm = _rowmask(R).cuda()
    hs = bf(torch.randn(R, C, generator=g).cuda() * rm[:, None])
    w = (torch.randn(2 * H, C, taps, generator=g) / (C * taps) ** 0.5).cuda()
    b = (torch.randn(2 * H, generator=g) * 0.1).cuda()
    cond = (torch.randn(B, 2 * H, generator=g) * 0.3).cuda()
    pw = ops.pack_weight(w, perm=ops.PERM_PAIR, perm_h=H, precision=ops.BF16)
    assert pw.npad == 2 * H
    G32 = torch.zeros(R, 2 * H, device="cuda")
    G16 = torch.zeros(R, 2 * H, device="cuda", dtype=torch.bfloat16)
    acts = torch.zeros(R, H, device="cuda", dtype=torch.bfloat16)
    kw = dict(pad=(taps - 1) // 2, epi=ops.EPI_GATE, h=H, n=2 * H, rows_per_utt=T + 4, bias=b, cond=cond, ldcond=2 * H, ld0=2 * H)
    _only_conv_cl(lambda: ops.conv_cl(hs.float(), pw, C, R, out0=G32, **kw))
    _served_by(f"conv_dma<GATE,{taps}>", lambda: ops.conv_cl(hs, pw, C, R, out0=G16, out1=acts, ld1=H, io_flags=ops.IO_A_BF16 | ops.IO_OUT0_BF16, **kw))
    d = (bf(G32).float() - G16.float()).abs().max().item()
    print(f"gates: max |d| {d:.3e}")
    assert d <= 2 ** -7
    # tanh * sigmoid for the Res_Skip conv: the product of the fp32 gates, rounded once; against the product of the bf16-stored gates that is
    # two input roundings (2^-9 each on values in (-1, 1)) and one output rounding (2^-9): within 2^-7
    da = (acts.float() - G16[:, 0::2].float() * G16[:, 1::2].float()).abs().max().item()
    print(f"acts: max |d| {da:.3e}")
    assert da <= 2 ** -7


@pytest.mark.parametrize("R,H,first", [(195, 64, True), (260, 128, False), (195, 192, False)])       # K = H: 2, 4, 6 chunks (whole stages of two)
def test_resskip_matches_fp32_storage(R, H, first):
    from glow_tts_amd import ops
    B, T = SHAPES[R]
    g = torch.Generator().manual_seed(R + H)
    rm = _rowmask(R).cuda()
    acts = bf(torch.rand(R, H, generator=g).cuda() * 2 - 1)
    hin = bf(torch.randn(R, H, generator=g).cuda() * rm[:, None])
    w = (torch.randn(2 * H, H, 1, generator=g) / H ** 0.5).cuda()
    b = (torch.randn(2 * H, generator=g) * 0.1).cuda()
    pw = ops.pack_weight(w, precision=ops.BF16)
    skip0 = torch.zeros(R, H) if first else torch.randn(R, H, generator=g)
    x32, s32 = torch.zeros(R, H, device="cuda"), skip0.clone().cuda()
    x16, s16 = torch.zeros(R, H, device="cuda", dtype=torch.bfloat16), skip0.clone().cuda()
    kw = dict(epi=ops.EPI_RESSKIP, flags=ops.F_FIRST if first else 0, h=H, n=2 * H, rows_per_utt=T + 4, bias=b, rowmask=rm, ld0=H, ld1=H, ldi0=H)
    # fp32 storage has no plain-operand RESSKIP: the comparator multiplies the pair (acts, 1) in its PAIRMUL prologue - the same bf16 operand
    pairs = torch.stack([acts.float(), torch.ones_like(acts, dtype=torch.float32)], 2).reshape(R, 2 * H).contiguous()
    _only_conv_cl(lambda: ops.conv_cl(pairs, pw, H, R, lda=2 * H, apro=ops.APRO_PAIRMUL, out0=x32, out1=s32, in0=hin.float(), **kw))
    _served_by("conv_dma<RESSKIP,1>", lambda: ops.conv_cl(acts, pw, H, R, out0=x16, out1=s16, in0=hin,
                                                          io_flags=ops.IO_A_BF16 | ops.IO_IN0_BF16 | ops.IO_OUT0_BF16, **kw))
    print(f"res: max |d| {(bf(x32).float() - x16.float()).abs().max().item():.3e}; skip: max |d| {(s32 - s16).abs().max().item():.3e}")
    assert _one_bf16_rounding(x16, x32)
    assert torch.allclose(s32, s16, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("R,H", [(195, 64), (260, 192)])          # K = 2 H from two sources: ca1 = 64 of 128, 192 of 384
def test_dgate_matches_fp32_storage(R, H):
    from glow_tts_amd import ops
    B, T = SHAPES[R]
    g = torch.Generator().manual_seed(R * 3 + H)
    rm = _rowmask(R).cuda()
    w = (torch.randn(2 * H, H, 1, generator=g) / H ** 0.5).cuda()
    pwt = ops.pack_weight(w, transpose=True, precision=ops.BF16)
    dres, dskip = bf(torch.randn(R, H, generator=g).cuda()), bf(torch.randn(R, H, generator=g).cuda())
    gates = bf(torch.rand(R, 2 * H, generator=g).cuda())
    d32 = torch.zeros(R, 2 * H, device="cuda")
    d16 = torch.zeros(R, 2 * H, device="cuda", dtype=torch.bfloat16)
    kw = dict(lda2=H, ca1=H, epi=ops.EPI_DGATE, n=H, h=H, rows_per_utt=T + 4, rowmask=rm, ldi0=2 * H, ld0=2 * H)
    _only_conv_cl(lambda: ops.conv_cl(dres.float(), pwt, 2 * H, R, a2=dskip.float(), out0=d32, in0=gates.float(), **kw))
    _served_by("conv_dma<DGATE,1>", lambda: ops.conv_cl(dres, pwt, 2 * H, R, a2=dskip, out0=d16, in0=gates,
                                                        io_flags=ops.IO_A_BF16 | ops.IO_IN0_BF16 | ops.IO_OUT0_BF16, **kw))
    print(f"dgate: max |d| {(bf(d32).float() - d16.float()).abs().max().item():.3e}")
    assert _one_bf16_rounding(d16, d32)


@pytest.mark.parametrize("R,H,reverse", [(195, 64, False), (260, 192, False), (195, 192, True)])
def test_couple_matches_fp32_storage(R, H, reverse):
    """End conv + affine coupling: 160 mel channels, (m, logs) of the 80 x_b channels PAIR-packed into npad = 192."""
    from glow_tts_amd import ops
    B, T = SHAPES[R]
    C, C2 = 160, 80
    g = torch.Generator().manual_seed(R + H + int(reverse))
    rm = _rowmask(R).cuda()
    skip = bf(torch.randn(R, H, generator=g).cuda())
    w = (torch.randn(C, H, 1, generator=g) * 0.3 / H ** 0.5).cuda()
    b = (torch.randn(C, generator=g) * 0.1).cuda()
    pw = ops.pack_weight(w, perm=ops.PERM_PAIR, perm_h=C2, precision=ops.BF16)
    assert pw.npad == 192
    x = torch.randn(R, C, generator=g).cuda()
    z32, z16 = torch.zeros(R, C, device="cuda"), torch.zeros(R, C, device="cuda")
    k32, k16 = torch.zeros(R, pw.npad, device="cuda"), torch.zeros(R, pw.npad, device="cuda")
    kw = dict(epi=ops.EPI_COUPLE, flags=ops.F_REVERSE if reverse else 0, n=C, h=C2, rows_per_utt=T + 4, bias=b, rowmask=rm, in0=x[:, C2:], ldi0=C,
              ld0=C, ld1=pw.npad)
    _only_conv_cl(lambda: ops.conv_cl(skip.float(), pw, H, R, out0=z32[:, C2:], out1=k32, **kw))
    _served_by("conv_dma<COUPLE,1>", lambda: ops.conv_cl(skip, pw, H, R, out0=z16[:, C2:], out1=k16, io_flags=ops.IO_A_BF16, **kw))
    print(f"couple: x_b' max |d| {(z32 - z16).abs().max().item():.3e}; (m, logs) max |d| {(k32 - k16).abs().max().item():.3e}")
    assert torch.all(z16[:, :C2] == 0)
    assert torch.allclose(z32, z16, rtol=1e-5, atol=1e-5) and torch.allclose(k32, k16, rtol=1e-5, atol=1e-5)


def test_dma_epilogue_stores_stay_inside_rows():
    """test_gpu_conv.py::test_epilogue_stores_stay_inside_rows on the LDS-DMA path: the last workgroup's rows past `rows` are computed from clamped
    loads and must be dropped by the epilogue - canary rows behind `rows` stay untouched (LINEAR fp32 / bf16, GATE, RESSKIP, DGATE)."""
    from glow_tts_amd import ops
    g = torch.Generator().manual_seed(5)
    H, K, Rbuf, R = 64, 3, 400, 301                      # 301 rows: the last tile is partial, and so is its last 32-row fragment
    S = 7.0
    io = ops.IO_A_BF16 | ops.IO_IN0_BF16 | ops.IO_OUT0_BF16
    a = bf(torch.randn(Rbuf, H, generator=g).cuda())
    w = (torch.randn(2 * H, H, K, generator=g) / (H * K) ** 0.5).cuda()
    b = torch.randn(2 * H, generator=g).cuda()
    rm = torch.ones(Rbuf, device="cuda")
    pw = ops.pack_weight(w, perm=ops.PERM_PAIR, perm_h=H, precision=ops.BF16)
    G = torch.full((Rbuf, 2 * H), S, device="cuda", dtype=torch.bfloat16)
    acts = torch.full((Rbuf, H), S, device="cuda", dtype=torch.bfloat16)
    _served_by("conv_dma<GATE,3>", lambda: ops.conv_cl(a, pw, H, R, pad=1, epi=ops.EPI_GATE, h=H, n=2 * H, rows_per_utt=R, bias=b, out0=G, ld0=2 * H,
                                                       out1=acts, ld1=H, io_flags=ops.IO_A_BF16 | ops.IO_OUT0_BF16))
    assert torch.all(G[R:] == S) and not torch.any(G[:R] == S) and torch.all(acts[R:] == S) and not torch.any(acts[:R] == S)
    pwl = ops.pack_weight(w, precision=ops.BF16)
    for dt, fl in ((torch.float32, ops.IO_A_BF16), (torch.bfloat16, ops.IO_A_BF16 | ops.IO_OUT0_BF16)):
        Y = torch.full((Rbuf, 2 * H), S, device="cuda", dtype=dt)
        _served_by("conv_dma<LINEAR,3>", lambda: ops.conv_cl(a, pwl, H, R, pad=1, flags=ops.F_BIAS | ops.F_MASK, bias=b, rowmask=rm, out0=Y, ld0=2 * H, io_flags=fl))
        assert torch.all(Y[R:] == S) and not torch.any(Y[:R] == S)
    w2 = (torch.randn(2 * H, H, 1, generator=g) / H ** 0.5).cuda()
    pw2 = ops.pack_weight(w2, precision=ops.BF16)
    xo, sk = torch.full((Rbuf, H), S, device="cuda", dtype=torch.bfloat16), torch.full((Rbuf, H), S, device="cuda")
    _served_by("conv_dma<RESSKIP,1>", lambda: ops.conv_cl(acts, pw2, H, R, epi=ops.EPI_RESSKIP, flags=ops.F_FIRST, h=H, n=2 * H, bias=b, rowmask=rm,
                                                          out0=xo, ld0=H, out1=sk, ld1=H, in0=a, ldi0=H, io_flags=io))
    assert torch.all(xo[R:] == S) and torch.all(sk[R:] == S) and not torch.any(xo[:R] == S) and not torch.any(sk[:R] == S)
    pw3 = ops.pack_weight(w2, transpose=True, precision=ops.BF16)
    d = torch.full((Rbuf, 2 * H), S, device="cuda", dtype=torch.bfloat16)
    _served_by("conv_dma<DGATE,1>", lambda: ops.conv_cl(a, pw3, 2 * H, R, a2=a, lda2=H, ca1=H, epi=ops.EPI_DGATE, n=H, h=H, in0=G, ldi0=2 * H, out0=d,
                                                        ld0=2 * H, io_flags=io))
    assert torch.all(d[R:] == S) and not torch.any(d[:R] == S)
