"""The fused coupling kernels (csrc/wavenet_fused.hip wn_fwd_kernel, csrc/wavenet_fused_bwd.hip wn_bwd_kernel) over their whole shape contract - 1 <= L <= 4 layers,
Sound.Mel_Dim 68 .. 96 - in two tiers, on the cases of tests/wavenet_fused_cases.py (their docstring states shapes, bars and what was measured):

  (a) CONTRACT: every kept tensor of the training forward, the rows after each flow, z, the log-determinants, the inverse and EVERY gradient of a 2-flow decoder
      against the independent float64 restatement of the rounding contract (tests/wavenet_fused_ref.py, emu64) under bars that are twice what the restatement's own
      float32 runs reach (tests/test_wavenet_fused_ref_cpu.py holds those runs to half the bars); the error next to the workgroups' window seams against the error
      elsewhere; exact zeros on pad rows and masked frames.
  (b) ENVELOPE: the fused launches against the per-conv launches with the assertions tests/test_gpu_wavenet_fused.py makes at (L, Mel_Dim) = (4, 80).

Every test asserts the launch log first - exactly F `wn_fwd<..>` (and, in training, F `wn_bwd<..>`) launches and no per-conv coupling launch - so that a silent
fallback cannot pass for coverage."""
import pytest
import torch

import wavenet_fused_cases as C
from wavenet_fused_gpu import close_rows, forward, grads, outs_columns, seam_rows

pytestmark = pytest.mark.gpu
IDS = [C.case_id(c) for c in C.CASES]
F_ = C.N_FLOWS


def _count(counts, prefix):
    return sum(n for k, n in counts.items() if k.startswith(prefix))


def _fused_only(counts, K, bwd):
    tag = ("drop" if K["drop_p"] else "nodrop") + (",cond" if K["cond"] is not None else "")
    assert counts.get(f"wn_fwd<{tag}>", 0) == F_ and _count(counts, "wn_fwd<") == F_, counts
    assert not any(k.startswith(("conv_dma<GATE", "conv_dma<RESSKIP", "conv_dma<LINEAR", "conv_dma<DGATE", "conv_chain", "conv_cl<GATE", "conv_cl<RESSKIP", "conv_cl<DGATE")) for k in counts), counts
    if bwd:
        assert counts.get(f"wn_bwd<{tag}>", 0) == F_ and _count(counts, "wn_bwd<") == F_, counts


def _per_conv_only(counts):
    assert not any(k.startswith(("wn_fwd", "wn_bwd")) for k in counts), counts


def _device(c):
    from glow_tts_amd import decoder as D
    K = C.build(c)
    cfg = K["cfg"]
    dc = D.DecoderConfig(cfg.mel_dim, cfg.n_flows, cfg.n_squeeze, cfg.n_split, cfg.wn_channels, cfg.wn_layers, cfg.wn_kernel, 1)
    assert D.fused_wn_supported(dc)
    P = {k: v.cuda() for k, v in K["sd"].items()}
    W = dict(zip(D.WEIGHT_KEYS, [w.contiguous() for w in D.stack_decoder_weights(P, dc)]))
    cond = K["cond"].cuda() if K["cond"] is not None else None
    seed = torch.tensor([K["word"]], device="cuda", dtype=torch.int32) if K["drop_p"] else None
    return D, K, dc, P, W, K["mels"].cuda(), K["ml"].cuda(), cond, seed


def _bct(rows, K):
    """[B * (T + 4), ch] on the device -> [B, ch, T] float64 on the host"""
    return rows.float().view(K["B"], K["T"] + 4, -1)[:, 2:2 + K["T"]].transpose(1, 2).double().cpu()


def _flat(t, K):
    """[B, ch, T] -> the rows layout [B * (T + 4), ch] (pad rows zero)"""
    return torch.nn.functional.pad(t.transpose(1, 2), (0, 0, 2, 2)).reshape(K["B"] * (K["T"] + 4), -1)


def _train_forward(c, fused=True):
    D, K, dc, P, W, mels, ml, cond, seed = _device(c)
    D.TUNE["drop_skip32"] = False                               # the fp32 skip rows are compared
    try:
        z, ld, buf, rm, counts = forward(D, dc, W, mels, ml, cond, fused, K["drop_p"], seed)
    finally:
        D.TUNE["drop_skip32"] = True
    return K, z, ld, buf, rm, counts


def _kept(K, z, ld, buf, rm):
    """name -> [B, ch, T] float64 tensors named as wavenet_fused_cases.run names them (masked frames zero)"""
    sm = _bct(rm[:, None], K)
    cm, cl = outs_columns(K["C2"])
    out = {"z": z.double().cpu()}
    if K["B"] > 1:
        out["logdet"] = ld.double().cpu()
    for f in range(F_):
        for l in range(K["L"]):
            out[f"hs{f}.{l}"] = _bct(buf.hs[f, l], K) * sm
            g = buf.gates[f, l].view(-1, C.H, 2)
            out[f"gates{f}.{l}"] = _bct(torch.cat([g[:, :, 0], g[:, :, 1]], 1), K) * sm
            out[f"acts{f}.{l}"] = _bct(buf.actp[f, l], K) * sm
        out[f"skip{f}"] = _bct(buf.skip[f], K) * sm
        out[f"m{f}"], out[f"logs{f}"] = _bct(buf.outs[f][:, cm], K) * sm, _bct(buf.outs[f][:, cl], K) * sm
        out[f"x{f + 1}"] = _bct(buf.x[f + 1], K) * sm
    return out


# ------------------------------------------------------------------------------------------------------------------ (a) contract tier
@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_contract_forward(c):
    K, z, ld, buf, rm, counts = _train_forward(c)
    _fused_only(counts, K, bwd=False)
    R = C.refs(c)
    got = _kept(K, z, ld, buf, rm)
    assert set(got) == {n for n in R["emu64"] if n not in ("mel_inv", "dmel", "dcond") and not n.startswith("grad/")}
    failed = []
    for name, t in got.items():
        try:
            C.check(C.case_id(c), name, t, R)
        except AssertionError as e:                            # (every tensor is measured and printed before the test fails)
            failed.append(str(e)[:300])
    # pad rows and masked frames: exact zeros in the rows of every flow and in z
    for f in range(F_ + 1):
        assert (buf.x[f] * (1 - rm).unsqueeze(1)).abs().max() == 0, f
    valid = (torch.arange(K["tm"], device="cuda")[None, :] < (K["ml"].cuda() // 2 * 2)[:, None]).unsqueeze(1)
    assert (z * (~valid)).abs().max() == 0
    # window seams: the error of the rows within 2 L rows of a multiple of nvalid(L) against the error elsewhere
    Rr = buf.x.shape[1]
    seam = seam_rows(Rr, C.nvalid(K["L"]), 2 * K["L"])
    for f in range(F_):
        err = ((buf.x[f + 1].double().cpu() - _flat(R["emu64"][f"x{f + 1}"], K)).abs().max(dim=1).values * rm.double().cpu())
        s_, o_ = err[seam.cpu()].max().item(), err[~seam.cpu()].max().item()
        print(f"{C.case_id(c)} flow {f}: row error next to the seams {s_:.3e}, elsewhere {o_:.3e}")
        assert (rm.cpu()[seam.cpu()] > 0).any() and o_ > 0
        if s_ > 4 * o_ + 1e-3:
            failed.append(f"seam rows of flow {f}: {s_} against {o_} elsewhere")
    assert not failed, failed


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_contract_inverse(c):
    from helpers import launch_counts, launch_reset
    D, K, dc, P, W, mels, ml, cond, seed = _device(c)
    with torch.no_grad():
        launch_reset()
        mel = D.decoder_inverse(dc, W, K["zin"].cuda(), ml, cond=cond)
        torch.cuda.synchronize()
        counts = launch_counts()
    assert _count(counts, "wn_fwd<nodrop") == F_ and _count(counts, "wn_fwd<") == F_ and not any(k.startswith(("conv_dma", "conv_chain")) for k in counts), counts
    C.check(C.case_id(c), "mel_inv", mel, C.refs(c))


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_contract_backward(c):
    D, K, dc, P, W, mels, ml, cond, seed = _device(c)
    g, dx, counts = grads(D, dc, P, mels, ml, K["wz"].cuda(), K["wl"].cuda(), True, K["drop_p"], cond, seed)
    _fused_only(counts, K, bwd=True)
    R = C.refs(c)
    assert set(K["sd"]) <= set(g)
    failed = []
    got = {"grad/" + k: g[k] for k in K["sd"]}
    got["dmel"] = dx
    if cond is not None:
        got["dcond"] = g["<conditioning>"]
    for name, t in got.items():
        try:
            C.check(C.case_id(c), name, t, R)
        except AssertionError as e:
            failed.append(str(e)[:300])
    if cond is not None:                                        # per utterance as well: a run credited to the wrong utterance keeps the total
        for b in range(K["B"]):
            a, w = got["dcond"][b].flatten().double().cpu(), R["emu64"]["dcond"][b].flatten()
            assert w.norm() > 0 and (a @ w / (a.norm() * w.norm())).item() >= 0.999, b
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------ (b) envelope tier
ENVELOPE = [c for c in C.CASES if c[2] != "span"]


@pytest.mark.parametrize("c", ENVELOPE, ids=[C.case_id(c) for c in ENVELOPE])
def test_envelope_forward_matches_per_conv_launches(c):
    """tests/test_gpu_wavenet_fused.py test_fused_forward_matches_per_conv_launches' assertions at this (L, Mel_Dim)"""
    K, zf, ldf, bf, rm, cf = _train_forward(c, True)
    _, zu, ldu, bu, _, cu = _train_forward(c, False)
    _fused_only(cf, K, bwd=False)
    _per_conv_only(cu)
    assert any(k.startswith("conv_chain<RESSKIP,COUPLE>") for k in cu), cu
    L = K["L"]
    close_rows(bf.hs[0, 0], bu.hs[0, 0], "h0", rm, atol=0.0, frac=2e-3, big=0.05)
    for l in range(L):
        close_rows(bf.gates[0, l], bu.gates[0, l], f"gates{l}", rm, atol=1e-6, frac=2e-2 * (l + 1), big=0.05)
        close_rows(bf.actp[0, l], bu.actp[0, l], f"acts{l}", rm, atol=1e-6, frac=2e-2 * (l + 1), big=0.05)
        close_rows(bf.hs[0, l], bu.hs[0, l], f"hs{l}", rm, atol=1e-6, frac=2e-2 * (l + 1), big=0.1)
    close_rows(bf.skip[0], bu.skip[0], "skip", rm, atol=2e-2, frac=1e-3, big=0.2)
    cm, cl = outs_columns(K["C2"])
    close_rows(bf.outs[0][:, cm], bu.outs[0][:, cm], "m", rm, atol=5e-3, frac=2e-3, big=0.05)
    close_rows(bf.outs[0][:, cl], bu.outs[0][:, cl], "logs", rm, atol=5e-3, frac=2e-3, big=0.05)
    assert (bf.x[1] * (1 - rm).unsqueeze(1)).abs().max() == 0
    valid = (torch.arange(K["tm"], device="cuda")[None, :] < (K["ml"].cuda() // 2 * 2)[:, None]).unsqueeze(1)
    assert ((zf - zu) * valid).abs().max() <= 0.2, ((zf - zu) * valid).abs().max()
    assert (((zf - zu) * valid) ** 2).mean().sqrt() <= 5e-3 * ((zu * valid) ** 2).mean().sqrt()
    assert ((ldf - ldu).abs() <= 2e-3 * ldu.abs() + 0.05).all(), (ldf, ldu)
    err = ((bf.x[1] - bu.x[1]).abs().max(dim=1).values * rm)
    seam = seam_rows(bf.x.shape[1], C.nvalid(L), 2 * L)
    if seam.any() and (~seam).any() and err[~seam].max() > 0:
        assert err[seam].max() <= 4 * err[~seam].max() + 1e-3, (err[seam].max().item(), err[~seam].max().item())


@pytest.mark.parametrize("c", ENVELOPE, ids=[C.case_id(c) for c in ENVELOPE])
def test_envelope_inverse_matches_per_conv_launches(c):
    from helpers import launch_counts, launch_reset
    D, K, dc, P, W, mels, ml, cond, seed = _device(c)
    z = K["zin"].cuda()
    outs = []
    for fused in (True, False):
        D.TUNE["fused_wn"] = fused
        try:
            with torch.no_grad():
                launch_reset()
                outs.append(D.decoder_inverse(dc, W, z, ml, cond=cond))
                torch.cuda.synchronize()
                n = _count(launch_counts(), "wn_fwd<")
                assert n == (F_ if fused else 0), launch_counts()
        finally:
            D.TUNE["fused_wn"] = True
    valid = (torch.arange(outs[0].shape[2], device="cuda")[None, :] < (ml // 2 * 2)[:, None]).unsqueeze(1)
    d = ((outs[0] - outs[1]) * valid).abs()
    assert d.max() <= 0.2 and (d ** 2).mean().sqrt() <= 5e-3 * ((outs[1] * valid) ** 2).mean().sqrt(), d.max()
    with torch.no_grad():                                       # and the round trip through the fused forward returns the input
        prep = D._Prepared(dc, W, need_bwd=False, cond=cond)
        back = D._run_forward(dc, prep, outs[0], ml)[0]
    assert ((back - z) * valid[:, :, :back.shape[2]]).abs().max() <= 0.1


@pytest.mark.parametrize("c", ENVELOPE, ids=[C.case_id(c) for c in ENVELOPE])
def test_envelope_backward_matches_per_conv_backward(c):
    D, K, dc, P, W, mels, ml, cond, seed = _device(c)
    wz, wl = K["wz"].cuda(), K["wl"].cuda()
    gf, dxf, cf = grads(D, dc, P, mels, ml, wz, wl, True, K["drop_p"], cond, seed)
    gu, dxu, cu = grads(D, dc, P, mels, ml, wz, wl, False, K["drop_p"], cond, seed)
    _fused_only(cf, K, bwd=True)
    assert _count(cu, "wn_bwd") == 0 and any("<LINEAR,5" in k for k in cu), cu
    worst = (2.0, "")
    for k, want in gu.items():
        a, b = gf[k].flatten().double(), want.flatten().double()
        cos, ratio = (a @ b / (a.norm() * b.norm() + 1e-30)).item(), (a.norm() / (b.norm() + 1e-30)).item()
        worst = min(worst, (cos, k))
        assert cos >= 0.9995 and 0.99 <= ratio <= 1.01, (k, cos, ratio)
    valid = (torch.arange(K["tm"], device="cuda")[None, :] < (ml // 2 * 2)[:, None]).unsqueeze(1)
    a, b = (dxf * valid).flatten().double(), (dxu * valid).flatten().double()
    assert (a @ b / (a.norm() * b.norm())).item() >= 0.9995 and 0.99 <= (a.norm() / b.norm()).item() <= 1.01
    if cond is not None:
        for b_ in range(K["B"]):
            a, b = gf["<conditioning>"][b_].flatten().double(), gu["<conditioning>"][b_].flatten().double()
            assert b.norm() > 0 and (a @ b / (a.norm() * b.norm() + 1e-30)).item() >= 0.999, b_
    print(f"{C.case_id(c)}: fused vs per-conv backward, worst gradient cosine", worst)
