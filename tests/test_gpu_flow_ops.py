"""Operator-level tests of the flow decoder's bandwidth-bound kernels (glow_tts_amd/csrc/flow_ops.hip) through the C ABI, against the float64
references of tests/flow_ops_ref.py (themselves checked on the CPU by tests/test_flow_ops_ref_cpu.py).

Technique common to every case: inputs hold large finite garbage on every padding and pad row (a kernel that relies on zeros there instead of on
rowmask shows it); outputs are pre-filled with NaN and every element must be written; every output and scratch buffer sits between sentinel
guard bands that must come back untouched; rowmask is what glowtts_squeeze_rows writes for ragged lengths (full, odd, no valid frame, odd Tm).

No tolerance below was set from a kernel's output.  Each is one of: exact; assert_elementwise (16 * 2**-24 * sum|terms|); assert_reduction
(1e-5 * sum|terms|); the propagated statistics bar - all derived in flow_ops_ref.py.  The worst error / bar per entry point is printed at the end of
the module (a report of how much room the derived bars leave, not an assertion)."""
import json
import math
import os
import types

import pytest
import torch

import flow_ops_ref as R
from helpers import launch_counts, launch_reset

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
GUARD = 64                     # elements of sentinel either side of every device buffer (256 bytes of fp32: the body stays 16-byte aligned)
SENT = -7.0                    # exact in fp32 and bf16
E_ARG = -1

CHANNELS = [4, 12, 20, 24, 36, 160, 164, 264, 1024]
SMALL_ROWS = [(1, 1), (4, 5), (1, 33), (5, 9)]          # B (T + 4) = 5 rows, exactly one block of 36, 37, 64 + 1


def _shapes():
    out = []
    for C in CHANNELS:
        out += [(C, B, T) for B, T in SMALL_ROWS]
        if C in (20, 24, 160, 164, 264):
            out.append((C, 4, 400))                      # 1616 rows
        if C in (20, 160, 164):
            out.append((C, 32, 400))                     # 12928 rows (the 1024-channel cases stay small)
    return out


SHAPES = _shapes()


def L():
    from glow_tts_amd import _lib
    return _lib.lib()


def stream():
    from glow_tts_amd import _lib
    return _lib.stream()


class Buf:
    """A device buffer between two guard bands.  init None: pre-filled with NaN (an output: every element must be written); else a CPU tensor.
    misalign: elements by which the body is moved off its 16-byte alignment."""
    all = []

    def __init__(self, shape, init=None, dtype=torch.float32, misalign=0):
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        n = math.prod(shape)
        self.raw = torch.full((n + 2 * GUARD + misalign,), SENT, dtype=dtype, device="cuda")
        self.lo, self.n = GUARD + misalign, n
        self.t = self.raw[self.lo:self.lo + n].view(shape)
        if init is None:
            self.t.fill_(NAN)
        else:
            self.t.copy_(init.to(dtype).reshape(shape))
        Buf.all.append(self)

    @property
    def p(self):
        return self.t.data_ptr()

    def cpu(self):
        return self.t.cpu()

    def check(self, what=""):
        g = torch.cat([self.raw[:self.lo], self.raw[self.lo + self.n:]]).float().cpu()
        assert bool((g == SENT).all()), f"{what}: guard band overwritten at offsets {torch.nonzero(g != SENT).flatten()[:8].tolist()}"


def check_guards():
    torch.cuda.synchronize()
    for i, b in enumerate(Buf.all):
        b.check(f"buffer {i} {tuple(b.t.shape)}")


@pytest.fixture(autouse=True)
def _fresh_buffers():
    Buf.all = []
    yield
    Buf.all = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    R.WORST.clear()
    yield
    if R.WORST:
        print("\nworst error / bar per entry point (derived bars; a report, not an assertion):")
        for k in sorted(R.WORST):
            print(f"  {k:56s} {R.WORST[k]:.3f}")
        path = os.environ.get("GLOWTTS_FLOW_OPS_REPORT")
        if path:
            with open(path, "w") as f:
                json.dump(R.WORST, f, indent=1, sort_keys=True)


def ok(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def device_rowmask(lens, Tm, ns=2):
    """rowmask [B, T + 4] as glowtts_squeeze_rows writes it (Cm = 1: the mask does not depend on the channel count), checked against the reference."""
    B = len(lens)
    T = Tm // ns
    mel = Buf((B, 1, Tm), torch.zeros(B, 1, Tm))
    rows, rm = Buf((B, T + 4, ns)), Buf((B, T + 4))
    ln = torch.as_tensor(lens, dtype=torch.int64).cuda()
    ok(L().glowtts_squeeze_rows(mel.p, rows.p, rm.p, ln.data_ptr(), B, 1, Tm, ns, stream()), "glowtts_squeeze_rows")
    _, want = R.squeeze_rows(torch.zeros(B, 1, Tm, dtype=F64), torch.as_tensor(lens), ns)
    R.assert_bits_equal(rm.cpu(), want.float(), "rowmask")
    assert bool((rows.cpu() == 0).all())
    return rm


def case(C, B, T, **kw):
    c = R.make_case(B, T, C, seed=1000 * C + 10 * T + B, **kw)
    c.d_rowmask = device_rowmask(c.lens.tolist(), c.Tm)
    return c


def prepare(W):
    """W [F, 4, 4] (float64 holding fp32) -> winfo Buf [F, 36] by glowtts_inv1x1_prepare; W^-1 as the kernel stored it (float64)."""
    F_ = W.shape[0]
    w = Buf((F_, 16), W.reshape(F_, 16))
    winfo = Buf((F_, 36))
    ok(L().glowtts_inv1x1_prepare(w.p, winfo.p, F_, stream()), "glowtts_inv1x1_prepare")
    return winfo, winfo.cpu()[:, 16:32].reshape(F_, 4, 4).to(F64)


# ------------------------------------------------------------------------------------------------------- squeeze / unsqueeze
@pytest.mark.parametrize("T", [7, 16, 37])                # below, at and above the 16-frame tile
@pytest.mark.parametrize("Cm", [1, 5, 12, 80])
@pytest.mark.parametrize("ns", [1, 2, 3])
def test_squeeze_unsqueeze_rows_are_exact(ns, Cm, T):
    """Selection times {0, 1}: bit-equal to the float64 reference cast to fp32; pad rows and rowmask exactly 0 / 1."""
    from glow_tts_amd import decoder as D
    g = torch.Generator().manual_seed(ns * 1000 + Cm * 10 + T)
    B = 4
    for Tm in ([ns * T] if ns == 1 else [ns * T, ns * T + 1]):          # a multiple of ns and not
        lens = torch.tensor([Tm, (Tm // 2) | 1, max(ns - 1, 1), int(torch.randint(1, Tm + 1, (1,), generator=g))])
        mel = R.f32(torch.randn(B, Cm, Tm, generator=g, dtype=F64))
        beyond = torch.arange(Tm)[None, None, :] >= lens[:, None, None]
        mel = torch.where(beyond, torch.full_like(mel, -1e3), mel)      # garbage past every length
        want_rows, want_mask = R.squeeze_rows(mel, lens, ns)
        ln = lens.cuda()
        for with_mask in (True, False):
            d_mel, rows, rm = Buf((B, Cm, Tm), mel), Buf((B, T + 4, ns * Cm)), Buf((B, T + 4))
            ok(L().glowtts_squeeze_rows(d_mel.p, rows.p, rm.p if with_mask else None, ln.data_ptr(), B, Cm, Tm, ns, stream()), "glowtts_squeeze_rows")
            R.assert_bits_equal(rows.cpu(), want_rows.float(), "squeeze rows")
            assert bool((rows.cpu()[:, :2] == 0).all()) and bool((rows.cpu()[:, T + 2:] == 0).all())
            if with_mask:
                R.assert_bits_equal(rm.cpu(), want_mask.float(), "rowmask")
            else:
                assert bool(torch.isnan(rm.cpu()).all())
        # unsqueeze: whatever the invalid rows hold never reaches the output
        junk = R.f32(torch.where(want_mask[..., None] > 0, want_rows, torch.full_like(want_rows, 1e3)))
        d_rows = Buf((B, T + 4, ns * Cm), junk)
        for fill in (None, -4.0):
            want = R.unsqueeze_rows(junk, lens, Tm, ns, fill)
            out = Buf((B, Cm, Tm))
            ok(L().glowtts_unsqueeze_rows(d_rows.p, out.p, ln.data_ptr(), B, Cm, Tm, ns, 0 if fill is None else 1, 0.0 if fill is None else fill, stream()),
               "glowtts_unsqueeze_rows")
            got = out.cpu()
            R.assert_bits_equal(got[:, :, :ns * T], want.float(), "unsqueeze")
            assert bool(torch.isnan(got[:, :, ns * T:]).all())          # the kernel does not write an odd tail ...
            wrapped = D.unsqueeze_rows(types.SimpleNamespace(Cm=Cm, ns=ns), d_rows.t.view(-1, ns * Cm), ln, B, Tm, fill).cpu()
            R.assert_bits_equal(wrapped[:, :, :ns * T], want.float(), "unsqueeze (wrapper)")
            assert bool((wrapped[:, :, ns * T:] == 0).all())             # ... the Python wrapper zeroes it
        check_guards()
    assert L().glowtts_squeeze_rows(d_mel.p, rows.p, None, ln.data_ptr(), B, Cm, ns - 1, ns, stream()) == E_ARG      # Tm < ns


# ------------------------------------------------------------------------------------------------------- 4x4 inverse / logdet
@pytest.mark.parametrize("F_", [1, 12, 65])               # crosses the 64-thread block
def test_inv1x1_prepare_pivots_and_signs(F_):
    """Against torch.linalg.inv / slogdet in float64 of the same fp32 weights (R.assert_inverse: 4 * 2**-24 * max|W^-1| per entry, 1e-6 on log|det|)."""
    sets = [R.pivot_matrices(F_, seed=F_)] if F_ > 1 else [R.pivot_matrix(k, torch.Generator().manual_seed(i))[None] for i, k in enumerate(R.PIVOT_KINDS)]
    for W in sets:
        assert float(torch.linalg.cond(W).max()) < 100
        winfo, _ = prepare(W)
        got = winfo.cpu()
        R.assert_bits_equal(got[:, :16], W.reshape(-1, 16).float(), "copied W")
        ratio = R.assert_inverse(got[:, 16:32].reshape(-1, 4, 4), got[:, 32], got[:, 33], W)
        R._note("inv1x1_prepare", ratio)
        sign = torch.linalg.slogdet(W)[0]
        assert torch.equal(got[:, 33].to(F64), sign)
        if F_ > 1:
            assert float(sign.min()) == -1.0 and float(sign.max()) == 1.0
        check_guards()


# ---------------------------------------------------------------------------------------------- ActNorm + 1x1, forward / reverse
@pytest.mark.parametrize("C,B,T", SHAPES)
def test_actnorm_inv1x1_forward_reverse_pass(C, B, T):
    c = case(C, B, T)
    lib, s = L(), stream()
    winfo, winv = prepare(c.W[None])
    logs, bias = Buf(C, c.logs), Buf(C, c.bias)
    want = R.actnorm_inv1x1(c.x, c.logs, c.bias, c.W, c.rowmask)
    scale = R.actnorm_inv1x1_scale(c.x, c.logs, c.bias, c.W, c.rowmask)
    masked = c.rowmask == 0

    def check_fwd(got, what):
        R.assert_elementwise(got, want, scale, what=what)
        assert bool((got[masked] == 0).all()), what + ": masked rows are not exactly zero"
    x = Buf((c.R, C), c.x)
    out = Buf((c.R, C))
    ok(lib.glowtts_actnorm_inv1x1(x.p, out.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, c.R, C, 0, s), "actnorm_inv1x1")
    fwd = out.cpu()
    check_fwd(fwd, "actnorm_inv1x1 forward")
    xi = Buf((c.R, C), c.x)
    ok(lib.glowtts_actnorm_inv1x1(xi.p, xi.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, c.R, C, 0, s), "actnorm_inv1x1 in place")
    R.assert_bits_equal(xi.cpu(), fwd, "forward in place vs out of place")
    # _pass: the first C/2 output channels also go to xpass, whose second half stays as it was
    out2, xpass = Buf((c.R, C)), Buf((c.R, C), torch.full((c.R, C), 3.25))
    ok(lib.glowtts_actnorm_inv1x1_pass(x.p, out2.p, xpass.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, c.R, C, s), "actnorm_inv1x1_pass")
    R.assert_bits_equal(out2.cpu(), fwd, "_pass xout")
    R.assert_bits_equal(xpass.cpu()[:, :C // 2], fwd[:, :C // 2], "_pass xpass first half")
    assert bool((xpass.cpu()[:, C // 2:] == 3.25).all()), "_pass wrote the second half of xpass"
    out3 = Buf((c.R, C))
    ok(lib.glowtts_actnorm_inv1x1_pass(x.p, out3.p, out3.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, c.R, C, s), "actnorm_inv1x1_pass xpass == xout")
    R.assert_bits_equal(out3.cpu(), fwd, "_pass with xpass == xout")
    # _pass_bf: + a bf16 copy of x_a [rows][C/2], with xpass, with xpass == NULL and with xpass == xout
    for mode in ("xpass", "null", "same"):
        out4, xp4 = Buf((c.R, C)), Buf((c.R, C), torch.full((c.R, C), 3.25))
        xa = Buf((c.R, C // 2), dtype=torch.bfloat16)
        pp = {"xpass": xp4.p, "null": None, "same": out4.p}[mode]
        launch_reset()
        ok(lib.glowtts_actnorm_inv1x1_pass_bf(x.p, out4.p, pp, xa.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, c.R, C, s), "actnorm_inv1x1_pass_bf")
        assert launch_counts().get("actnorm_inv1x1_pass", 0) == 1
        R.assert_bits_equal(out4.cpu(), fwd, "_pass_bf xout")
        R.assert_bits_equal(xa.cpu(), fwd[:, :C // 2].to(torch.bfloat16), "xa_bf vs nearest-even bf16 of the kernel's own fp32 output")
        if mode == "xpass":
            R.assert_bits_equal(xp4.cpu()[:, :C // 2], fwd[:, :C // 2], "_pass_bf xpass")
            assert bool((xp4.cpu()[:, C // 2:] == 3.25).all())
        else:
            assert bool((xp4.cpu() == 3.25).all())
    ok(lib.glowtts_actnorm_inv1x1_pass_bf(x.p, out4.p, None, None, logs.p, bias.p, winfo.p, c.d_rowmask.p, c.R, C, s), "actnorm_inv1x1_pass_bf without xa_bf")
    R.assert_bits_equal(out4.cpu(), fwd, "_pass_bf without a bf16 copy")
    # reverse, on garbage-padded rows of its own
    z = c.xmid
    wantr = R.actnorm_inv1x1(z, c.logs, c.bias, c.W, c.rowmask, reverse=True, Winv=winv[0])
    scaler = R.actnorm_inv1x1_reverse_scale(z, c.logs, c.bias, winv[0], c.rowmask)
    zin, rout = Buf((c.R, C), z), Buf((c.R, C))
    ok(lib.glowtts_actnorm_inv1x1(zin.p, rout.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, c.R, C, 1, s), "actnorm_inv1x1 reverse")
    rev = rout.cpu()
    R.assert_elementwise(rev, wantr, scaler, what="actnorm_inv1x1 reverse")
    assert bool((rev[masked] == 0).all())
    ok(lib.glowtts_actnorm_inv1x1(zin.p, zin.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, c.R, C, 1, s), "actnorm_inv1x1 reverse in place")
    R.assert_bits_equal(zin.cpu(), rev, "reverse in place vs out of place")
    # reverse of forward returns the input: the forward's error (<= 16 eps scale) carried through |W^-1| exp(-logs), plus the reverse pass's own bar at z.
    # (W^-1 is the fp32 inverse: W^-1 W differs from 1 by 4 eps max|W^-1| per entry of W^-1 - R.assert_inverse - which the third term carries)
    back = Buf((c.R, C))
    ok(lib.glowtts_actnorm_inv1x1(out.p, back.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, c.R, C, 1, s), "reverse of forward")
    zero_b = torch.zeros_like(c.bias)
    carried = R.actnorm_inv1x1_reverse_scale(scale, c.logs, zero_b, winv[0], c.rowmask)
    own = R.actnorm_inv1x1_reverse_scale(want, c.logs, c.bias, winv[0], c.rowmask)
    inv_err = R.actnorm_inv1x1_reverse_scale(want, c.logs, zero_b, torch.full((4, 4), 0.25 * float(winv.abs().max()), dtype=F64), c.rowmask)
    R.assert_elementwise(back.cpu(), c.x * c.rowmask[:, None], carried + own + inv_err, what="actnorm_inv1x1 reverse(forward)")
    check_guards()


@pytest.mark.parametrize("C", [6, 2])
def test_actnorm_inv1x1_rejects_channel_counts_off_the_group_size(C):
    b = Buf((8, 8), torch.zeros(8, 8))
    for rev in (0, 1):
        assert L().glowtts_actnorm_inv1x1(b.p, b.p, b.p, b.p, b.p, b.p, 8, C, rev, stream()) == E_ARG
    assert L().glowtts_actnorm_inv1x1_pass(b.p, b.p, b.p, b.p, b.p, b.p, b.p, 8, C, stream()) == E_ARG


# ------------------------------------------------------------------------------------------------------- ActNorm statistics
@pytest.mark.parametrize("offset,std", [(-2.0, 1.0), (-4.0, 0.3)])          # mel-like inputs
@pytest.mark.parametrize("C,B,T", SHAPES)
def test_actnorm_stats_and_from_stats(C, B, T, offset, std):
    c = case(C, B, T)
    lib, s = L(), stream()
    x = c.x / 1.5 * std + offset
    const = C // 2                                                   # one constant channel
    x[:, const] = -2.5
    x = R.f32(torch.where((c.rowmask == 0)[:, None], c.x, x))       # (masked rows keep their garbage)
    d_x, stats = Buf((c.R, C), x), Buf(2 * C + 1)
    scratch = Buf(int(lib.glowtts_actnorm_stats_scratch_floats(c.R, C)))
    ok(lib.glowtts_actnorm_stats(d_x.p, c.d_rowmask.p, stats.p, scratch.p, c.R, C, s), "actnorm_stats")
    want, sumabs = R.colstats(x, c.rowmask)
    R.assert_reduction(stats.cpu(), want, sumabs, what="actnorm_stats")
    assert float(stats.cpu()[-1]) == float(c.rowmask.sum())          # a count: exact
    logs, bias = Buf(C), Buf(C)
    ok(lib.glowtts_actnorm_from_stats(stats.p, logs.p, bias.p, C, s), "actnorm_from_stats")
    wl, wb = R.actnorm_init(x, c.rowmask)
    lbar, bbar = R.actnorm_init_bars(x, c.rowmask)
    gl, gb = logs.cpu().to(F64), bias.cpu().to(F64)
    assert bool(torch.isfinite(gl).all()) and bool(torch.isfinite(gb).all())
    # The propagated bar is first order in (error of var) / var.  Where the variance is no larger than four times the error the sums may carry - the constant
    # channel, and every channel when one frame is valid - the fp32 cancellation E[x^2] - mean^2 may land either side of the 1e-7 clamp: there only
    # `finite and at most -0.5 log(1e-7) plus the bar` is asserted, not equality with the float64 clamp.
    m = c.rowmask[:, None]
    den = c.rowmask.sum()
    mean, sq = (x * m).sum(0) / den, (x * x * m).sum(0) / den
    degenerate = (sq - mean ** 2) <= 4 * 128 * R.EPS32 * (sq + mean ** 2)
    assert bool(degenerate[const])
    good = ~degenerate
    assert bool((gl[degenerate] <= -0.5 * math.log(1e-7) + lbar[degenerate]).all())
    if bool(good.any()):
        R._note("actnorm_from_stats logs", float(((gl - wl).abs() / lbar)[good].max()))
        R._note("actnorm_from_stats bias", float(((gb - wb).abs() / bbar)[good].max()))
        assert bool(((gl - wl).abs() <= lbar)[good].all()), float(((gl - wl).abs() / lbar)[good].max())
        assert bool(((gb - wb).abs() <= bbar)[good].all()), float(((gb - wb).abs() / bbar)[good].max())
    check_guards()


# ------------------------------------------------------------------------------------------------------- coupling backward
@pytest.mark.parametrize("C,B,T", SHAPES)
def test_coupling_bwd(C, B, T):
    lib, s = L(), stream()
    for extra in (0, 64):                                            # ldo at its minimum and one step wider
        c = case(C, B, T, ldo_extra=extra)
        C2, ldo = c.C2, c.ldo
        xb, dzb = c.xmid[:, C2:], c.dz[:, C2:]
        want = R.coupling_bwd(dzb, xb, c.m, c.lg, c.rowmask, c.dld_rows)              # d x_b, d m, d logs
        scale = R.coupling_bwd_scale(dzb, xb, c.m, c.lg, c.rowmask, c.dld_rows)
        xmid, outs, dld = Buf((c.R, C), c.xmid), Buf((c.R, ldo), c.outs), Buf(B, c.dld)
        results = {}
        for form in ("f32", "both", "bf16"):
            dz = Buf((c.R, C), c.dz)
            douts = Buf((c.R, ldo)) if form != "bf16" else None
            d16 = Buf((c.R, ldo), dtype=torch.bfloat16) if form != "f32" else None
            if form == "f32":
                ok(lib.glowtts_coupling_bwd(dz.p, xmid.p, outs.p, douts.p, c.d_rowmask.p, dld.p, c.R, C, ldo, c.Tp, s), "coupling_bwd")
            else:
                ok(lib.glowtts_coupling_bwd_bf16(dz.p, xmid.p, outs.p, douts.p if douts else None, d16.p, c.d_rowmask.p, dld.p, c.R, C, ldo, c.Tp, s), "coupling_bwd_bf16")
            got_dz = dz.cpu()
            R.assert_bits_equal(got_dz[:, :C2], c.dz[:, :C2].float(), "first C/2 channels of dz")
            R.assert_elementwise(got_dz[:, C2:], want[0], scale[0], what="coupling_bwd d x_b")
            if douts is not None:
                g = douts.cpu()
                gm, gl = R.pair_unpack(g, C2)
                R.assert_elementwise(gm, want[1], scale[1], what="coupling_bwd d m")
                R.assert_elementwise(gl, want[2], scale[2], what="coupling_bwd d logs")
                R.assert_pair_pads_zero(g, C2, "douts")
            if d16 is not None:
                R.assert_pair_pads_zero(d16.cpu(), C2, "douts_bf16")
            if form == "both":
                R.assert_bits_equal(d16.cpu(), douts.cpu().to(torch.bfloat16), "bf16 copy vs nearest-even of the fp32 copy")
            results[form] = (got_dz, douts.cpu() if douts else None, d16.cpu() if d16 else None)
        # the douts == NULL form: the same kernel on the same inputs - its outputs are the bits of the form that keeps both copies
        R.assert_bits_equal(results["bf16"][0], results["both"][0], "dz, bf16-only form")
        R.assert_bits_equal(results["bf16"][2], results["both"][2], "douts_bf16, bf16-only form")
        R.assert_bits_equal(results["f32"][1], results["both"][1], "douts, fp32-only form")
        check_guards()
        Buf.all = []
    b = Buf((4, 64), torch.zeros(4, 64))
    assert lib.glowtts_coupling_bwd(b.p, b.p, b.p, b.p, b.p, b.p, 4, 8, 32, 4, s) == E_ARG               # ldo not a multiple of 64
    assert lib.glowtts_coupling_bwd(b.p, b.p, b.p, b.p, b.p, b.p, 4, 128, 64, 4, s) == E_ARG             # ldo < C
    assert lib.glowtts_coupling_bwd_bf16(b.p, b.p, b.p, b.p, None, b.p, b.p, 4, 8, 64, 4, s) == E_ARG    # no bf16 copy to write


# ----------------------------------------------------------------------------------------------- ActNorm + 1x1 backward
def _bwd_inputs(c, misalign):
    return Buf((c.R, c.C), c.dz, misalign=misalign), Buf((c.R, c.C), c.x, misalign=misalign)


def _expect_kernel(C, misalign, coupling=False):
    wide = C % 8 == 0 and misalign == 0                             # the float4 kernel needs C % 8 == 0 and 16-byte aligned rows
    return "actnorm_inv_bwd<%s%s>" % ("16B" if wide else "8B", ",coupling" if coupling else "")


def _bwd_kernels_taken():
    return {k: n for k, n in launch_counts().items() if k.startswith("actnorm_inv_bwd<") and n}


BWD_CASES = [(C, B, T, 0) for C, B, T in SHAPES] + [(C, B, T, 2) for C in (24, 160) for B, T in SMALL_ROWS + [(4, 400)]]      # 2 floats = 8 bytes off


@pytest.mark.parametrize("C,B,T,misalign", BWD_CASES)
def test_actnorm_inv1x1_bwd(C, B, T, misalign):
    """Both kernels: C % 8 == 4 takes the 8-byte kernel, C % 8 == 0 the float4 kernel, and C = 24 / 160 with all three row pointers 8 bytes inside a larger
    allocation the 8-byte kernel at the shapes production runs.  In place (dz == dx, what flow.hip does) and out of place."""
    c = case(C, B, T)
    lib, s = L(), stream()
    winfo, _ = prepare(c.W[None])
    logs, bias = Buf(C, c.logs), Buf(C, c.bias)
    want = R.actnorm_inv1x1_bwd(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    scale = R.actnorm_inv1x1_bwd_scale(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    want_pg, scale_pg = torch.cat([want[1], want[2], want[3].flatten()]), torch.cat([scale[1], scale[2], scale[3].flatten()])
    name = _expect_kernel(C, misalign)
    n = 2 * C + 16
    nfl = int(lib.glowtts_actnorm_stats_scratch_floats(c.R, C))
    direct = None
    for inplace in (True, False):
        dz, x = _bwd_inputs(c, misalign)
        dx = dz if inplace else Buf((c.R, C), misalign=misalign)
        pg, scratch = Buf(n), Buf(nfl)
        launch_reset()
        ok(lib.glowtts_actnorm_inv1x1_bwd(dz.p, dx.p, x.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, pg.p, scratch.p, c.R, C, s), "actnorm_inv1x1_bwd")
        assert _bwd_kernels_taken() == {name: 1}, _bwd_kernels_taken()
        R.assert_elementwise(dx.cpu(), want[0], scale[0], what=name + " dx")
        R.assert_reduction(pg.cpu(), want_pg, scale_pg, what=name + " param_grads")
        if direct is None:
            direct = (dx.cpu(), pg.cpu())
        else:
            R.assert_bits_equal(dx.cpu(), direct[0], "dx out of place vs in place")
            R.assert_bits_equal(pg.cpu(), direct[1], "param_grads out of place vs in place")
        if not inplace:
            R.assert_bits_equal(dz.cpu(), c.dz.float(), "dz (read only out of place)")
    # param_grads == NULL, then glowtts_colsum_batched over the per-block partials: same partials, same reduction kernel - the same bits
    dz, x = _bwd_inputs(c, misalign)
    scratch, pg2 = Buf(nfl), Buf(n)
    nblk = int(lib.glowtts_actnorm_bwd_blocks(c.R))
    assert nblk == -(-c.R // 36) and nblk * n <= nfl
    ok(lib.glowtts_actnorm_inv1x1_bwd(dz.p, dz.p, x.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, None, scratch.p, c.R, C, s), "actnorm_inv1x1_bwd (partials)")
    ok(lib.glowtts_colsum_batched(scratch.p, pg2.p, nblk, n, 1, 0, 0, s), "colsum_batched")
    R.assert_bits_equal(dz.cpu(), direct[0], "dx, partials form")
    R.assert_bits_equal(pg2.cpu(), direct[1], "param_grads through colsum_batched")
    part = scratch.cpu()
    assert bool(torch.isfinite(part[:nblk * n]).all()) and bool(torch.isnan(part[nblk * n:]).all())       # every partial written, nothing behind them
    check_guards()


@pytest.mark.parametrize("C", [1028, 6])
def test_actnorm_inv1x1_bwd_rejects_unsupported_channel_counts(C):
    """C / 4 > 256 and C % 4 != 0: GLOWTTS_E_ARG without a launch (the outputs keep their NaN pre-fill)."""
    lib, s = L(), stream()
    rows = 8
    a = Buf((rows, 1028), torch.zeros(rows, 1028))
    out, pg, scratch = Buf((rows, 1028)), Buf(2 * 1028 + 16), Buf(int(lib.glowtts_actnorm_stats_scratch_floats(rows, 1028)))
    launch_reset()
    assert lib.glowtts_actnorm_inv1x1_bwd(a.p, out.p, a.p, a.p, a.p, a.p, a.p, pg.p, scratch.p, rows, C, s) == E_ARG
    ldo = R.pair_ldo(C)
    assert lib.glowtts_actnorm_inv1x1_bwd_coupling(a.p, out.p, a.p, a.p, a.p, a.p, a.p, scratch.p, rows, C, a.p, a.p, out.p, None, a.p, ldo, 4, s) == E_ARG
    torch.cuda.synchronize()
    assert _bwd_kernels_taken() == {}
    assert bool(torch.isnan(out.cpu()).all()) and bool(torch.isnan(pg.cpu()).all()) and bool(torch.isnan(scratch.cpu()).all())
    check_guards()


# (C, pad slots of the PAIR packing at the minimum ldo); the last two entries take the 8-byte kernel
FUSED_C = [(8, 28), (24, 20), (56, 4), (160, 16), (20, 22), (164, 14)]
FUSED_CASES = [(C, B, T, 0) for C, _ in FUSED_C for B, T in [(1, 33), (5, 9), (4, 400)]] + [(C, B, T, 2) for C in (24, 160) for B, T in [(5, 9), (4, 400)]]


@pytest.mark.parametrize("C,B,T,misalign", FUSED_CASES)
def test_actnorm_inv1x1_bwd_coupling_fused(C, B, T, misalign):
    """The fused launch against (a) the float64 reference of the composition and (b) the two separate launches; fp32 copy only, bf16 copy only, both.
    The pad columns of the PAIR packing are zeroed by a different loop in each kernel: exactly zero on both, at several pad widths."""
    c = case(C, B, T)
    lib, s = L(), stream()
    C2, ldo = c.C2, c.ldo
    assert dict(FUSED_C)[C] * 2 == R.pair_pad_cols(C2, ldo).numel()
    winfo, _ = prepare(c.W[None])
    logs, bias = Buf(C, c.logs), Buf(C, c.bias)
    w1 = R.actnorm_inv1x1_bwd(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    s1 = R.actnorm_inv1x1_bwd_scale(c.dz, c.x, c.logs, c.bias, c.W, c.rowmask)
    xb = c.xmid[:, C2:]
    w2 = R.coupling_bwd(w1[0][:, C2:], xb, c.m, c.lg, c.rowmask, c.dld_rows)
    s2 = R.coupling_bwd_scale(s1[0][:, C2:], xb, c.m, c.lg, c.rowmask, c.dld_rows)       # the first stage's error travels through the same products
    want_dx, scale_dx = torch.cat([w1[0][:, :C2], w2[0]], 1), torch.cat([s1[0][:, :C2], s2[0]], 1)
    want_pg, scale_pg = torch.cat([w1[1], w1[2], w1[3].flatten()]), torch.cat([s1[1], s1[2], s1[3].flatten()])
    name = _expect_kernel(C, misalign, coupling=True)
    n, nfl, nblk = 2 * C + 16, int(lib.glowtts_actnorm_stats_scratch_floats(c.R, C)), int(lib.glowtts_actnorm_bwd_blocks(c.R))
    xmid, outs, dld = Buf((c.R, C), c.xmid, misalign=misalign), Buf((c.R, ldo), c.outs), Buf(B, c.dld)

    def check(dx, pg, douts, d16, what):
        R.assert_elementwise(dx, want_dx, scale_dx, what=what + " dx")
        R.assert_reduction(pg, want_pg, scale_pg, what=what + " param_grads")
        if douts is not None:
            gm, gl = R.pair_unpack(douts, C2)
            R.assert_elementwise(gm, w2[1], s2[1], what=what + " d m")
            R.assert_elementwise(gl, w2[2], s2[2], what=what + " d logs")
            R.assert_pair_pads_zero(douts, C2, what + " douts")
        if d16 is not None:
            R.assert_pair_pads_zero(d16, C2, what + " douts_bf16")
            if douts is not None:
                R.assert_bits_equal(d16, douts.to(torch.bfloat16), what + ": bf16 copy vs nearest-even of the fp32 copy")

    fused = {}
    for form in ("f32", "bf16", "both"):
        dz, x = _bwd_inputs(c, misalign)
        douts = Buf((c.R, ldo)) if form != "bf16" else None
        d16 = Buf((c.R, ldo), dtype=torch.bfloat16) if form != "f32" else None
        scratch, pg = Buf(nfl), Buf(n)
        launch_reset()
        ok(lib.glowtts_actnorm_inv1x1_bwd_coupling(dz.p, dz.p, x.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, scratch.p, c.R, C, xmid.p, outs.p,
                                                   douts.p if douts else None, d16.p if d16 else None, dld.p, ldo, c.Tp, s), "actnorm_inv1x1_bwd_coupling")
        assert _bwd_kernels_taken() == {name: 1}, _bwd_kernels_taken()
        ok(lib.glowtts_colsum_batched(scratch.p, pg.p, nblk, n, 1, 0, 0, s), "colsum_batched")
        fused[form] = (dz.cpu(), pg.cpu(), douts.cpu() if douts else None, d16.cpu() if d16 else None)
        check(*fused[form], what=name)
    R.assert_bits_equal(fused["f32"][0], fused["both"][0], "dx, fp32-only vs both")
    R.assert_bits_equal(fused["bf16"][0], fused["both"][0], "dx, bf16-only vs both")
    R.assert_bits_equal(fused["bf16"][3], fused["both"][3], "douts_bf16, bf16-only vs both")
    # (b) the separate launches: ActNorm / 1x1 backward (partials form), then the coupling backward on its dx
    dz, x = _bwd_inputs(c, misalign)
    douts, d16, scratch, pg = Buf((c.R, ldo)), Buf((c.R, ldo), dtype=torch.bfloat16), Buf(nfl), Buf(n)
    ok(lib.glowtts_actnorm_inv1x1_bwd(dz.p, dz.p, x.p, logs.p, bias.p, winfo.p, c.d_rowmask.p, None, scratch.p, c.R, C, s), "actnorm_inv1x1_bwd")
    ok(lib.glowtts_colsum_batched(scratch.p, pg.p, nblk, n, 1, 0, 0, s), "colsum_batched")
    ok(lib.glowtts_coupling_bwd_bf16(dz.p, xmid.p, outs.p, douts.p, d16.p, c.d_rowmask.p, dld.p, c.R, C, ldo, c.Tp, s), "coupling_bwd_bf16")
    sep = (dz.cpu(), pg.cpu(), douts.cpu(), d16.cpu())
    check(*sep, what="separate launches")
    same = all(torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))
               for a, b in zip(fused["both"], sep))
    print(f"{name} C={C} rows={c.R}: fused launch {'bit-equal to' if same else 'differs in the last bits from'} the separate launches (not asserted: contraction may differ)")
    check_guards()


# ------------------------------------------------------------------------------------------------------- colsum_batched
@pytest.mark.parametrize("batch", [1, 12])
@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 513])          # 513: the 8 x 64 unrolled stride runs a second trip
def test_colsum_batched(nrows, batch):
    g = torch.Generator().manual_seed(nrows * 100 + batch)
    for n in (5, 56):
        ps, os_ = nrows * n + 24, n + 8                             # strides larger than the extent: the gaps hold NaN / stay as they are
        part = torch.full((batch, ps), NAN, dtype=F64)
        vals = R.f32(torch.randn(batch, nrows, n, generator=g, dtype=F64) * torch.logspace(-2, 2, n, dtype=F64))
        part[:, :nrows * n] = vals.reshape(batch, -1)
        d_part, out = Buf((batch, ps), part), Buf((batch, os_), torch.full((batch, os_), 3.25))
        ok(L().glowtts_colsum_batched(d_part.p, out.p, nrows, n, batch, ps, os_, stream()), "colsum_batched")
        got = out.cpu()
        R.assert_reduction(got[:, :n], vals.sum(1), vals.abs().sum(1), what="colsum_batched")
        assert bool((got[:, n:] == 3.25).all())
        check_guards()


# ------------------------------------------------------------------------------------------------------- parameter gradients
@pytest.mark.parametrize("B", [1, 7, 8, 9, 33])
@pytest.mark.parametrize("Tp", [5, 256, 1024, 1025, 1500])         # 1025, 1500: the branch of its own for Tp > 1024
def test_decoder_param_grads(Tp, B):
    """dlogs = d_an + s, dbias = d_an, dW = d_an + s (C/4) W^-T with s = sum_b dlogdet[b] len'_b, against float64."""
    C, T = 20, Tp - 4
    g = torch.Generator().manual_seed(Tp * 100 + B)
    lens, Tm = R.ragged_lengths(B, T, 2, g)
    rm = device_rowmask(lens.tolist(), Tm)
    lens_sq = R.squeeze_rows(torch.zeros(B, 1, Tm, dtype=F64), lens, 2)[1].sum(1).round().long()
    dld = R.f32(torch.randn(B, generator=g, dtype=F64) + 0.25 * torch.arange(B))
    d_dld = Buf(B, dld)
    for F_ in (1, 12):
        W = R.well_conditioned_4x4(g, F_)
        winfo, winv = prepare(W)
        logs_all = R.f32(torch.randn(F_, C, generator=g, dtype=F64) * 0.3)
        d_an = R.f32(torch.randn(F_, 2 * C + 16, generator=g, dtype=F64))
        dlogs, dbias, dW, s_, sabs = R.decoder_param_grads(d_an, dld, logs_all, W, lens_sq, C)
        o_logs, o_bias, o_w = Buf((F_, C)), Buf((F_, C)), Buf((F_, 16))
        ok(L().glowtts_decoder_param_grads(Buf((F_, 2 * C + 16), d_an).p, d_dld.p, rm.p, winfo.p, o_logs.p, o_bias.p, o_w.p, F_, B, Tp, C, stream()),
           "decoder_param_grads")
        # s itself is not an output: it shows in dlogs - d_an.  sum|terms| of d_an + s is |d_an| + sum_b |dlogdet[b]| len'_b (the last addition's rounding,
        # 2**-24 of that, hides under 1e-5 of it)
        R.assert_reduction(o_logs.cpu(), dlogs, d_an[:, :C].abs() + sabs, what="decoder_param_grads dlogs")
        R.assert_bits_equal(o_bias.cpu(), d_an[:, C:2 * C].float(), "dbias")
        # dW: the kernel multiplies by W^-1 as glowtts_inv1x1_prepare stored it, within 4 * 2**-24 * max|W^-1| per entry of the float64 inverse
        # (R.assert_inverse); in units of the 1e-5 bar that is (4 * 2**-24 / 1e-5) max|W^-1| more per entry
        winv_abs = winv.transpose(1, 2).abs() + (4 * R.EPS32 / 1e-5) * winv.abs().amax(dim=(1, 2), keepdim=True)
        R.assert_reduction(o_w.cpu().view(F_, 4, 4), dW, d_an[:, 2 * C:].view(F_, 4, 4).abs() + sabs * (C / 4) * winv_abs, what="decoder_param_grads dW")
    check_guards()


# ------------------------------------------------------------------------------------------------------- log-determinant
@pytest.mark.parametrize("B,T", [(3, 33), (4, 400)])               # Tp = 37, 404: not multiples of 64
@pytest.mark.parametrize("C2", [2, 12, 64, 80, 128, 132])          # one load, both loads of the two-load scheme (64 < C/2 <= 128), the loop for C/2 > 128
def test_decoder_logdet(C2, B, T):
    C = 2 * C2
    g = torch.Generator().manual_seed(C2 * 1000 + T)
    for F_ in (1, 12):
        c = R.make_case(B, T, C, seed=C * 100 + T)
        rm = device_rowmask(c.lens.tolist(), c.Tm)
        ldo = c.ldo
        stride = c.R * ldo + 128                                      # a flow stride larger than one buffer: the gap holds NaN
        outs_all = torch.full((F_, stride), NAN, dtype=F64)
        bad = (c.rowmask == 0)[:, None]
        junk = 1e3 * (1.0 - 2.0 * ((torch.arange(c.R)[:, None] + torch.arange(C2)[None, :]) % 2))
        lg_all = []
        for f in range(F_):
            lg = R.f32(torch.where(bad, junk, torch.randn(c.R, C2, generator=g, dtype=F64) * 0.3))       # (no exp in this kernel: 1e3 on the masked rows)
            outs_all[f, :c.R * ldo] = R.pair_pack(R.f32(torch.randn(c.R, C2, generator=g, dtype=F64)), lg, ldo, fill=1e3).flatten()
            lg_all.append(lg.view(B, c.Tp, C2))
        W = R.well_conditioned_4x4(g, F_)
        winfo, _ = prepare(W)
        logs_all = R.f32(torch.randn(F_, C, generator=g, dtype=F64) * 0.3)
        want, sumabs = R.decoder_logdet(torch.stack(lg_all), logs_all, W, c.rowmask2, C)
        # the kernel reads log|det W| as glowtts_inv1x1_prepare stored it, within 1e-6 max(1, |logdet|) of the float64 value (R.assert_inverse): that is
        # 1e-6 max(1, |logdet|) (C/4) len' of the result, 0.1 of it in units of the 1e-5 bar
        sumabs = sumabs + 0.1 * (torch.linalg.slogdet(W)[1].abs().clamp_min(1.0).sum() * (C / 4)) * c.lens_sq.to(F64)
        part, out = Buf(F_ * B), Buf(B)
        ok(L().glowtts_decoder_logdet(Buf((F_, stride), outs_all).p, stride, Buf((F_, C), logs_all).p, winfo.p, rm.p, part.p, out.p, F_, B, c.Tp, C, ldo, stream()),
           "decoder_logdet")
        R.assert_reduction(out.cpu(), want, sumabs, what="decoder_logdet")
        assert float(out.cpu()[-1]) == 0.0 and float(c.lens_sq[-1]) == 0            # an utterance with no valid frame
        check_guards()
        Buf.all = []
