"""float64 references of the flow decoder's bandwidth-bound kernels (glow_tts_amd/csrc/flow_ops.hip) and the comparison helpers of their
operator tests.  Plain torch on the CPU, no GPU import: tests/test_flow_ops_ref_cpu.py checks this file on any machine,
tests/test_gpu_flow_ops.py compares the kernels with it.

The references are the oracle's own pinned functions (oracle/glowtts_ref.py: squeeze, unsqueeze, actnorm_init, actnorm, inv1x1 and the
affine lines of coupling) applied to the library's layouts, with torch.autograd supplying every backward reference.

Layouts
  rows     [B][T + 4][C]: channels contiguous, two zero pad rows either side of every utterance (GLOWTTS_ROW_PAD); flat: [R][C], R = B (T + 4)
  rowmask  [R]: 1 on valid squeezed frames, 0 on padding and pad rows
  PAIR     (m, logs) of the coupling [R][ldo]: slot j < C/2 sits at column (j >> 5) * 64 + (j & 31), its log-scale 32 columns further;
           ldo = C rounded up to a multiple of 64, the columns no slot uses are the pad columns
"""
import types

import torch

from oracle import glowtts_ref as O

ROW_PAD = 2
EPS32 = 2.0 ** -24                       # half an fp32 ulp of 1: the relative error of one rounding to nearest
F64 = torch.float64
_CFG = types.SimpleNamespace(n_split=4)


# ----------------------------------------------------------------------------------------------------------------- layouts
def to_rows(x, fill=0.0):
    """[B, C, T] -> rows [B, T + 4, C]; the pad rows hold `fill` (0: the library's contract; a test passes garbage)."""
    B, C, T = x.shape
    r = x.new_full((B, T + 2 * ROW_PAD, C), fill)
    r[:, ROW_PAD:ROW_PAD + T] = x.transpose(1, 2)
    return r


def from_rows(rows):
    """rows [B, T + 4, C] -> [B, C, T]."""
    return rows[:, ROW_PAD:rows.shape[1] - ROW_PAD].transpose(1, 2).contiguous()


def mask_to_rows(mask):
    """oracle mask [B, 1, T] -> rowmask [B, T + 4]."""
    return to_rows(mask)[..., 0].contiguous()


def pair_ldo(C):
    return (C + 63) // 64 * 64


def pair_cols(C2):
    """-> (columns of m, columns of logs) of the C2 pair slots."""
    j = torch.arange(C2)
    cm = (j >> 5) * 64 + (j & 31)
    return cm, cm + 32


def pair_pad_cols(C2, ldo):
    used = torch.zeros(ldo, dtype=torch.bool)
    cm, cl = pair_cols(C2)
    used[cm] = True
    used[cl] = True
    return torch.nonzero(~used).flatten()


def pair_pack(m, logs, ldo, fill=0.0):
    """m, logs [R, C2] -> PAIR-packed [R, ldo] (pad columns = fill)."""
    out = m.new_full((m.shape[0], ldo), fill)
    cm, cl = pair_cols(m.shape[1])
    out[:, cm] = m
    out[:, cl] = logs
    return out


def pair_unpack(packed, C2):
    cm, cl = pair_cols(C2)
    return packed[:, cm], packed[:, cl]


def _bct(x2):
    """flat rows [R, C] -> the oracle's [1, C, R]."""
    return x2.t().unsqueeze(0)


def _flat(x3):
    return x3[0].t().contiguous()


def group_channels(C, wrong=False):
    """[4, C/4]: channel of split index s in mixing group g - {2g, 2g+1, C/2+2g, C/2+2g+1} (Modules.py:738-740).  wrong: {4g .. 4g+3}, the
    grouping a kernel author would write first (a mutation of the CPU tests; identical only at C = 4)."""
    g = torch.arange(C // 4)
    if wrong:
        return torch.stack([4 * g, 4 * g + 1, 4 * g + 2, 4 * g + 3])
    return torch.stack([2 * g, 2 * g + 1, C // 2 + 2 * g, C // 2 + 2 * g + 1])


def mix_by_groups(x2, M, wrong=False):
    """out[r, ch[o, g]] = sum_i M[o, i] x[r, ch[i, g]]: the 4x4 mixing by explicit indices (checked against the oracle's view / permute form)."""
    ch = group_channels(x2.shape[1], wrong)
    out = torch.empty_like(x2)
    out[:, ch] = torch.einsum("oi,rig->rog", M, x2[:, ch])
    return out


# -------------------------------------------------------------------------------------------------------------- squeeze
def squeeze_rows(mel, lengths, ns):
    """mel [B, Cm, Tm], lengths [B] -> (rows [B, T+4, ns Cm], rowmask [B, T+4]) through O.squeeze (an odd tail is dropped, Modules.py:897-898)."""
    mask = O.mask_from_lengths(lengths, mel.shape[2]).to(mel.dtype)
    x, m = O.squeeze(mel, mask, ns)
    T = mel.shape[2] // ns
    return to_rows(x), mask_to_rows(m[:, :, :T])


def unsqueeze_rows(rows, lengths, Tm, ns, fill=None):
    """rows [B, T+4, C] -> mel [B, C/ns, ns T] through O.unsqueeze; fill: value of the masked frames (GlowTTS.inference's masked_fill_)."""
    T = Tm // ns
    sm = O.mask_from_lengths(lengths, Tm).to(rows.dtype)[:, :, ns - 1::ns][:, :, :T]
    x = from_rows(rows)
    x = torch.where(sm.bool(), x, torch.zeros_like(x))          # the kernel selects: what an invalid row holds never reaches the output
    mel, m = O.unsqueeze(x, sm, ns)
    if fill is not None:
        mel = torch.where(m.bool(), mel, torch.full_like(mel, fill))
    return mel


# -------------------------------------------------------------------------------------------------- 4x4 inverse / logdet
def inv1x1_prepare(W):
    """W [F, 4, 4] -> (W^-1, log|det|, sign) in float64 (torch.inverse / torch.logdet, Modules.py:743, 747)."""
    W = W.to(F64)
    sign, logabs = torch.linalg.slogdet(W)
    return torch.linalg.inv(W), logabs, sign


def assert_inverse(got_inv, got_logdet, got_sign, W, what="inv1x1_prepare"):
    """W^-1 within 4 * 2**-24 * max|W^-1| per entry (the kernel eliminates in double and rounds once: 1 rounding = 2**-24 relative, x 4 for the
    double-precision elimination error at cond(W) < 100 and margin); log|det| within 1e-6 max(1, |log|det||) (one fp32 rounding of a double
    result, 6e-8 relative, plus the same margin); sign exact.  -> worst error / bar."""
    winv, logabs, sign = inv1x1_prepare(W)
    bar = 4 * EPS32 * winv.abs().amax(dim=(1, 2), keepdim=True)
    err = (got_inv.to(F64) - winv).abs()
    if not bool((err <= bar).all()):
        f = int(torch.nonzero(~(err <= bar))[0, 0])
        raise AssertionError(f"{what}: W^-1 of matrix {f} is off by {float(err[f].max()):.3e}, bar {float(bar[f].max()):.3e}")
    lbar = 1e-6 * logabs.abs().clamp_min(1.0)
    lerr = (got_logdet.to(F64) - logabs).abs()
    if not bool((lerr <= lbar).all()):
        raise AssertionError(f"{what}: log|det| off by {float(lerr.max()):.3e}")
    if not torch.equal(got_sign.to(F64), sign):
        raise AssertionError(f"{what}: sign of the determinant differs")
    return max(float((err / bar).max()), float((lerr / lbar).max()))


# ------------------------------------------------------------------------------------------------ ActNorm + invertible 1x1
def actnorm_inv1x1(x2, logs, bias, W, rowmask, reverse=False, Winv=None):
    """Forward: z = W (bias + exp(logs) x) per mixing group, masked (O.actnorm then O.inv1x1).  Reverse: (W^-1 z - bias) exp(-logs), masked;
    Winv given: that matrix is used as W^-1 (the kernel reads the fp32 inverse glowtts_inv1x1_prepare stored)."""
    sd = {"a.logs": logs.view(1, -1, 1), "a.bias": bias.view(1, -1, 1)}
    m = rowmask.view(1, 1, -1)
    if not reverse:
        sd["w.weight"] = W
        y, _ = O.actnorm(sd, "a", _bct(x2), m, False)
        z, _ = O.inv1x1(sd, "w", y, m, _CFG, False)
    else:
        sd["w.weight"] = W if Winv is None else Winv
        u, _ = O.inv1x1(sd, "w", _bct(x2), m, _CFG, Winv is None)
        z, _ = O.actnorm(sd, "a", u, m, True)
    return _flat(z)


def actnorm_inv1x1_scale(x2, logs, bias, W, rowmask):
    """sum_k |W_ik| (|e_k x_k| + |b_k|) on valid rows, 0 on masked ones (where the result must be exactly 0)."""
    return actnorm_inv1x1(x2.abs(), logs, bias.abs(), W.abs(), rowmask)


def actnorm_inv1x1_reverse_scale(z2, logs, bias, Winv, rowmask):
    """(sum_k |W^-1_ik| |z_k| + |b_i|) exp(-logs_i) on valid rows."""
    return actnorm_inv1x1(z2.abs(), logs, -bias.abs(), None, rowmask, reverse=True, Winv=Winv.abs())


def actnorm_inv1x1_bwd(dz2, x2, logs, bias, W, rowmask):
    """autograd of the forward reference for the loss sum(dz * z) -> (dx [R, C], dlogs [C], dbias [C], dW [4, 4])."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x2, logs, bias, W)]
    z = actnorm_inv1x1(leaves[0], leaves[1], leaves[2], leaves[3], rowmask)
    return torch.autograd.grad((z * dz2).sum(), leaves)


def actnorm_inv1x1_bwd_scale(dz2, x2, logs, bias, W, rowmask):
    """The same sums over absolute values: every term of dx / dlogs / dbias / dW is a product of entries of dz, W, exp(logs), x, bias, so the
    backward of the reference at (|dz|, |x|, logs, |bias|, |W|) is the sum of the absolute values of the terms of each result."""
    return actnorm_inv1x1_bwd(dz2.abs(), x2.abs(), logs, bias.abs(), W.abs(), rowmask)


# ------------------------------------------------------------------------------------------------------ ActNorm statistics
def colstats(x2, rowmask):
    """-> (stats [2C + 1] = sum x m, sum x^2 m, sum m; sumabs of the same terms)."""
    m = rowmask[:, None]
    s = torch.cat([(x2 * m).sum(0), (x2 * x2 * m).sum(0), rowmask.sum().view(1)])
    a = torch.cat([(x2.abs() * m).sum(0), (x2 * x2 * m).sum(0), rowmask.sum().view(1)])
    return s, a


def actnorm_init(x2, rowmask):
    """O.actnorm_init (Modules.py:698-711) on flat rows -> (logs [C], bias [C])."""
    logs, bias = O.actnorm_init(_bct(x2), rowmask.view(1, 1, -1))
    return logs.flatten(), bias.flatten()


def actnorm_init_bars(x2, rowmask, rel=128 * EPS32):
    """Propagated bars of (logs, bias) for column sums that carry a relative error rel (128 additions of 2**-24 each, assert_reduction's chain):
    var = E[x^2] - mean^2 then moves by rel (E[x^2] + mean^2) to first order, and logs = -0.5 log(var) by
        logs_bar = 0.5 * rel * (E[x^2] + mean^2) / var        (>= 64 * 2**-24: the roundings of the division, logf and expf hide under it);
    bias = -mean exp(logs) by  bias_bar = exp(logs) (rel E|x| + |mean| logs_bar).  All in float64 from the data."""
    m = rowmask[:, None]
    den = rowmask.sum()
    mean = (x2 * m).sum(0) / den
    sq = (x2 * x2 * m).sum(0) / den
    eabs = (x2.abs() * m).sum(0) / den
    var = (sq - mean ** 2).clamp_min(1e-7)
    logs_bar = 0.5 * rel * (sq + mean ** 2) / var
    bias_bar = torch.exp(-0.5 * torch.log(var)) * (rel * eabs + mean.abs() * logs_bar)
    return logs_bar, bias_bar


# ------------------------------------------------------------------------------------------------------- affine coupling
def coupling_affine(xb, m, logs, rowmask):
    """Modules.py:805-806 (the forward lines of O.coupling): z_b = (m + exp(logs) x_b) mask; per-row log-determinant terms sum_j logs mask."""
    mask = rowmask[:, None]
    return (m + torch.exp(logs) * xb) * mask, (logs * mask).sum(1)


def coupling_bwd(dzb, xb, m, logs, rowmask, dld_rows):
    """autograd of coupling_affine for sum(dz_b z_b) + sum_r dld[r] logdet_r -> (d x_b, d m, d logs), each [R, C/2]."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (xb, m, logs)]
    zb, ld = coupling_affine(leaves[0], leaves[1], leaves[2], rowmask)
    return torch.autograd.grad((zb * dzb).sum() + (ld * dld_rows).sum(), leaves)


def coupling_bwd_scale(dzb, xb, m, logs, rowmask, dld_rows):
    """|dz| e, |dz|, |dz| e |x_b| + |dld| on valid rows."""
    return coupling_bwd(dzb.abs(), xb.abs(), m, logs, rowmask, dld_rows.abs())


# ------------------------------------------------------------------------------------------- log-determinant bookkeeping
def _lens_mask(lens_sq, T):
    return O.mask_from_lengths(lens_sq, T).to(F64) if int(lens_sq.max()) > 0 else torch.zeros(len(lens_sq), 1, T, dtype=F64)


def param_logdet_terms(logs_all, W_all, lens_sq, C):
    """[F, B]: (sum_c logs_f[c] + logdet(W_f) C/4) * len'_b, from the log-determinants O.actnorm and O.inv1x1 return (Modules.py:694, 747)."""
    T = max(int(lens_sq.max()), 1)
    mask = _lens_mask(lens_sq, T)
    x = torch.zeros(len(lens_sq), C, T, dtype=F64)
    out = []
    for f in range(logs_all.shape[0]):
        sd = {"a.logs": logs_all[f].view(1, -1, 1), "a.bias": torch.zeros(1, C, 1, dtype=F64), "w.weight": W_all[f]}
        _, l0 = O.actnorm(sd, "a", x, mask, False)
        _, l1 = O.inv1x1(sd, "w", x, mask, _CFG, False)
        out.append(l0 + l1)
    return torch.stack(out)


def decoder_param_grads(d_an, dlogdet, logs_all, W_all, lens_sq, C):
    """d_an [F, 2C + 16] data terms + autograd of sum_b dlogdet[b] * param_logdet_terms -> (dlogs [F, C], dbias [F, C], dW [F, 4, 4], s, sum|terms of s|):
    s = sum_b dlogdet[b] len'_b, dlogs = d_an + s, dW = d_an + s (C/4) W^-T."""
    logs_ = logs_all.detach().clone().requires_grad_(True)
    W_ = W_all.detach().clone().requires_grad_(True)
    terms = param_logdet_terms(logs_, W_, lens_sq, C)
    gl, gw = torch.autograd.grad((terms * dlogdet[None, :]).sum(), [logs_, W_])
    F_ = logs_all.shape[0]
    s = (dlogdet * lens_sq.to(F64)).sum()
    sabs = (dlogdet.abs() * lens_sq.to(F64)).sum()
    return d_an[:, :C] + gl, d_an[:, C:2 * C].clone(), d_an[:, 2 * C:].view(F_, 4, 4) + gw, s, sabs


def decoder_logdet(outs_logs, logs_all, W_all, rowmask2, C, lens_from=None):
    """outs_logs [F, B, Tp, C/2] coupling log-scales (rows layout), rowmask2 [B, Tp] -> (logdet [B], sum|terms| [B]).
    logdet[b] = sum_f [(sum logs_f + logdet(W_f) C/4) len'_b + sum over valid rows sum_j logs^coupling]   (Modules.py:309).
    lens_from: lengths to use instead of the mask's row count (the `len' from len` mutation of the CPU tests)."""
    lens = rowmask2.sum(1).round().long() if lens_from is None else lens_from
    pt = param_logdet_terms(logs_all, W_all, lens, C)                                        # [F, B]
    cp = (outs_logs * rowmask2[None, :, :, None]).sum((2, 3))                                # [F, B]
    cabs = (outs_logs.abs() * rowmask2[None, :, :, None]).sum((2, 3))
    return (pt + cp).sum(0), (pt.abs() + cabs).sum(0)          # the parameter term enters as ONE product |sum logs + logdet(W) C/4| * len'


# ---------------------------------------------------------------------------------------------------------- seeded inputs
def f32(t):
    """float64 values that fp32 holds exactly (what the kernels are given)."""
    return t.to(torch.float32).to(F64)


def ragged_lengths(B, T, ns, g):
    """Mel lengths for B utterances of T squeezed frames: Tm = ns T + 1 (odd for ns = 2: the tail frame is dropped); utterance 0 has len == Tm,
    the others odd lengths, the last of three or more has len < ns (no valid frame)."""
    Tm = ns * T + 1
    lens = [Tm] + [int(torch.randint(ns, Tm + 1, (1,), generator=g)) | 1 for _ in range(B - 1)]
    if B >= 3:
        lens[-1] = ns - 1
    return torch.tensor([min(l, Tm) for l in lens]), Tm


def well_conditioned_4x4(g, n=1):
    """Perturbed orthogonal matrices with det > 0 (the reference keeps det > 0, Modules.py:722-723), cond < 2."""
    out = []
    for _ in range(n):
        w = torch.linalg.qr(torch.randn(4, 4, generator=g))[0] + 0.05 * torch.randn(4, 4, generator=g)
        if torch.det(w) < 0:
            w[:, 0] = -w[:, 0]
        out.append(w)
    return f32(torch.stack(out))


PIVOT_KINDS = ("random", "zero_corner", "largest_last", "permutation", "negative_diagonal")


def pivot_matrix(kind, g):
    """4x4 weights for glowtts_inv1x1_prepare, cond < 100 (the double-precision elimination error then stays far below one fp32 ulp):
    zero_corner: W[0][0] = 0; largest_last: the largest entry of column 0 sits in the last row (both force a row exchange);
    permutation: a permutation matrix (det +1 or -1); negative_diagonal: det < 0 (sign word -1)."""
    w = well_conditioned_4x4(g)[0]
    if kind == "zero_corner":
        w[0, 0] = 0.0
    elif kind == "largest_last":
        w = w[torch.argsort(w[:, 0].abs())]               # rows ordered by |column 0|: every elimination step of column 0 pivots from below
    elif kind == "permutation":
        w = torch.eye(4, dtype=F64)[torch.randperm(4, generator=g)]
    elif kind == "negative_diagonal":
        w = torch.diag(f32(torch.rand(4, generator=g) + 0.5))
        w[2, 2] = -w[2, 2]
    return w


def pivot_matrices(F_, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([pivot_matrix(PIVOT_KINDS[f % len(PIVOT_KINDS)], g) for f in range(F_)])


def make_case(B, T, C, seed, garbage=1e3, ldo_extra=0):
    """Seeded inputs of every operator test at (B, T, C), float64 holding fp32 values, flat rows.  Masked rows (padding and pad rows) hold large finite
    garbage (+-garbage) instead of zeros: a kernel that relies on zeros there instead of on rowmask then shows it, while reference and contract mask.
    Only the coupling's log-scales get +-20 there: exp(1e3) is inf in float64 too and 0 * inf is NaN in the reference itself."""
    g = torch.Generator().manual_seed(seed)
    ns, C2 = 2, C // 2
    lens, Tm = ragged_lengths(B, T, ns, g)
    _, rowmask2 = squeeze_rows(torch.zeros(B, 1, Tm, dtype=F64), lens, ns)
    rowmask = rowmask2.reshape(-1)
    R = rowmask.numel()
    bad = (rowmask == 0)[:, None]

    def rows(width, std=1.0, junk=garbage):
        v = torch.randn(R, width, generator=g) * std
        sign = 1.0 - 2.0 * ((torch.arange(R)[:, None] + torch.arange(width)[None, :]) % 2)
        return f32(torch.where(bad, sign * junk, v.to(F64)))
    c = types.SimpleNamespace(B=B, T=T, C=C, C2=C2, Tp=T + 2 * ROW_PAD, R=R, ns=ns, Tm=Tm, lens=lens, lens_sq=rowmask2.sum(1).round().long(),
                              rowmask2=rowmask2, rowmask=rowmask, ldo=pair_ldo(C) + ldo_extra)
    c.x, c.dz, c.xmid = rows(C, 1.5), rows(C), rows(C, 1.5)
    c.m, c.lg = rows(C2), rows(C2, 0.3, 20.0)
    c.outs = pair_pack(c.m, c.lg, c.ldo, fill=garbage)
    c.dld = f32(torch.randn(B, generator=g) + torch.arange(B) * 0.25)               # different for every utterance
    c.dld_rows = c.dld.repeat_interleave(c.Tp)
    c.logs, c.bias = f32(torch.randn(C, generator=g) * 0.3), f32(torch.randn(C, generator=g) * 0.5)
    c.W = well_conditioned_4x4(g)[0]
    return c


# -------------------------------------------------------------------------------------------------------------- helpers
WORST = {}           # what -> worst observed error / bar (a report, never asserted)


def _note(what, ratio):
    if what:
        WORST[what] = max(WORST.get(what, 0.0), float(ratio))


def _check(got, want64, bar, what, kind):
    got64 = got.detach().to("cpu").to(F64)
    assert got64.shape == want64.shape, (what, tuple(got64.shape), tuple(want64.shape))
    err = (got64 - want64).abs()
    ok = err <= bar                                   # (a NaN in `got` compares false)
    ratio = float(torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.zeros_like(err)).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    if not bool(ok.all()):
        idx = torch.nonzero(~ok)[0].tolist()
        i = tuple(idx)
        raise AssertionError(f"{what or kind}: {int((~ok).sum())} of {ok.numel()} elements miss the {kind} bar; first at {i}: got {float(got64[i])!r}, "
                             f"want {float(want64[i])!r}, bar {float(bar[i]):.3e}; worst error / bar = {ratio:.3g}")
    _note(what, ratio)
    return ratio


def assert_elementwise(got, want64, scale64, k=16, what=""):
    """|got - want| <= k * 2**-24 * scale per element; scale = float64 sum of the absolute values of the terms that make up the element.
    k = 16 is derived: at most 8 roundings in the longest fp32 chain of these kernels (each at most 2**-24 of a partial result that the
    absolute sum bounds) plus device expf at up to 2 ulp, all doubled.  Where scale is 0 (masked rows) the result must be exactly 0.  -> worst error / bar."""
    return _check(got, want64, k * EPS32 * scale64, what, "elementwise")


def assert_reduction(got, want64, sumabs64, tol=1e-5, what=""):
    """|got - want| <= tol * sum|terms| per element, for the sums over rows.  tol = 1e-5 is derived: the deepest fp32 summation chain of these kernels is
    64 serial rows + at most 8 serial partials per lane + 6 shuffle levels < 128 additions for rows <= 32768, and 128 * 2**-24 = 7.6e-6.  -> worst error / bar."""
    return _check(got, want64, tol * sumabs64, what, "reduction")


def rejected_fraction(got, want64, sumabs64, tol=1e-5):
    """Fraction of the elements assert_reduction would reject (the mutation checks: a fault may hide under tol in a few channels)."""
    err = (got.detach().to("cpu").to(F64) - want64).abs()
    return float((~(err <= tol * sumabs64)).double().mean())


def assert_pair_pads_zero(packed, C2, what="pad columns"):
    """Every pad column of a PAIR-packed buffer is exactly zero (the End conv's data / weight gradients read them)."""
    pads = pair_pad_cols(C2, packed.shape[1])
    p = packed.detach().to("cpu")[:, pads].float()
    if pads.numel() and not bool((p == 0).all()):
        r, c = torch.nonzero(p != 0)[0].tolist()
        raise AssertionError(f"{what}: pad column {int(pads[c])} of row {r} holds {float(p[r, c])!r}")


def assert_bits_equal(a, b, what="bit equality"):
    a, b = a.detach().to("cpu").contiguous(), b.detach().to("cpu").contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    it = {4: torch.int32, 2: torch.int16, 8: torch.int64}[a.element_size()]
    if not torch.equal(a.view(it), b.view(it)):
        n = int((a.view(it) != b.view(it)).sum())
        raise AssertionError(f"{what}: {n} of {a.numel()} elements differ in their bits")
