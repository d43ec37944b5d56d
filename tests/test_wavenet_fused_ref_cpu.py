"""The restatement of the fused coupling kernels' rounding contract (tests/wavenet_fused_ref.py), host side (no GPU): with the rounding switched off it IS
the oracle's coupling - forward, inverse and, for the hand-written backward, torch.autograd of the oracle -, and the reference runs emu32 / emu32b satisfy,
on every case, the bars tests/test_gpu_wavenet_fused_contract.py sets for the kernels (tests/wavenet_fused_cases.py: the bars are twice what is measured here)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wavenet_fused_cases as C  # noqa: E402
import wavenet_fused_ref as E  # noqa: E402
from oracle import glowtts_ref as O  # noqa: E402

IDS = [C.case_id(c) for c in C.CASES]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _oracle_hook(K):
    """The oracle's `drop` hook carrying the case's keep multipliers and conditioning rows: ins * keep + cond (Modules.py:861-866)."""
    keep = {k: v.double() for k, v in K["keep"].items()} if K["keep"] is not None else None
    cond = K["cond"].double().requires_grad_(True) if K["cond"] is not None else None

    def hook(pfx, layer, ins):
        f = int(pfx.split(".Flows.")[1].split(".")[0])
        if keep is not None:
            ins = ins * keep[(f, layer)]
        if cond is not None:
            ins = ins + cond[:, f, layer, :, None]
        return ins
    return (hook if (keep is not None or cond is not None) else None), cond


def test_rb_is_round_to_nearest_even():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8)], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0], dtype=torch.float64)
    assert torch.equal(E.rb(t), want) and E.rb(t).dtype == torch.float64 and E.rb(t.float()).dtype == torch.float32


def test_cases_are_the_ragged_batches_the_docstring_states():
    assert len(C.CASES) == 22 and {c[:2] for c in C.CASES if c[2] == "plain"} == set(C.CONFIGS) and (4, 80) in C.CONFIGS
    for L in (1, 2, 3, 4):
        lengths, tm = C.lengths_of(L)
        nv, Tp = C.nvalid(L), tm // 2 + 4
        assert nv == 64 - 4 * (L - 1) and Tp == nv + 1 and lengths == [tm, tm - 9, 36, 2] and lengths[1] % 2 == 1
        assert [(b * Tp) % nv for b in range(1, 4)] == [1, 2, 3]                     # utterance boundaries 1, 2, 3 rows behind a seam
        assert 212 <= 4 * Tp <= 260 and 4 <= -(-4 * Tp // nv) <= 5
        (n,), _ = C.lengths_of(L, "span")                                           # ... and fall on pad rows; the "span" case has mask 1 on both sides of the seam at nv
        assert n % 2 == 1 and 2 + 2 * L <= nv - 2 * L and nv + 2 * L <= 2 + n // 2 and (L, "span") in {(c[0], c[2]) for c in C.CASES}


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_unrounded_restatement_is_the_oracle_forward_inverse_and_autograd(c):
    K = C.build(c)
    cfg = K["cfg"]
    sd = {k: v.double().requires_grad_(True) for k, v in K["sd"].items()}
    x = K["mels"].double().requires_grad_(True)
    mask = O.mask_from_lengths(K["ml"], K["tm"]).double()
    hook, cond = _oracle_hook(K)
    zo, ldo, _ = O.decoder(sd, x, mask, cfg, drop=hook)
    ((zo * K["wz"].double()).sum() + (ldo * K["wl"].double()).sum()).backward()
    R = C.run(c, "ref64")
    assert _rel(R["z"], zo.detach()) <= 1e-12 and ("logdet" not in R or _rel(R["logdet"], ldo.detach()) <= 1e-12)
    worst = max((_rel(R["grad/" + k], v.grad), k) for k, v in sd.items())
    print(C.case_id(c), "ref64 against autograd of the oracle: worst gradient", worst, "d mel", _rel(R["dmel"], x.grad))
    assert worst[0] <= 1e-10 and _rel(R["dmel"], x.grad) <= 1e-10
    if cond is not None:
        assert _rel(R["dcond"], cond.grad) <= 1e-10
    # one coupling alone, forward and inverse, against oracle.coupling on the first flow's input
    q = "layer_Dict.Decoder.layer_Dict.Flows.0.layers.2"
    with torch.no_grad():
        sdd = {k: v.detach() for k, v in sd.items()}
        xs, sm = O.squeeze(x.detach(), mask, cfg.n_squeeze)
        P = E.flow_params(sdd, q, K["L"])
        cf = cond.detach()[:, 0] if cond is not None else None
        kf = [K["keep"][(0, l)].double() for l in range(K["L"])] if K["keep"] is not None else None
        for reverse in (False, True):
            want, ldw = O.coupling(sdd, q, xs, sm, cfg, reverse, drop=hook)
            got, ldg, _ = E.coupling_forward(P, xs, sm, "ref64", reverse, cf, kf)
            assert _rel(got, want) <= 1e-12 and (reverse or _rel(ldg, ldw) <= 1e-12)
        if hook is None:                                                             # (the oracle's inverse takes no hook: the whole decoder where nothing is injected)
            assert _rel(R["mel_inv"], O.decoder(sdd, K["zin"].double(), mask, cfg, reverse=True)[0]) <= 1e-12


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_reference_runs_meet_the_gpu_bars_with_a_quarter_to_spare(c):
    """emu32 / emu32b against emu64 on every compared tensor: within THREE QUARTERS of every bar (the bars are twice the worst of these ratios on the host the
    tables were made on; which elements float32 flips depends on the host's summation order), every ratio printed; the guards (e_bf > 100 e32, scale > 1e-3) are
    asserted inside `check`."""
    R = C.refs(c)
    part = {k: (0.75 * a, 0.75 * b) for k, (a, b) in C.BARS.items()}
    part_f = {k: 0.75 * f for k, f in C.FRACS.items()}
    assert all(C.key_of(n) in C.BARS for n in R["ref64"] if n != "logdet"), sorted(C.key_of(n) for n in R["ref64"] if C.key_of(n) not in C.BARS)
    for v in ("emu32", "emu32b"):
        assert all(t.dtype == torch.float64 for t in R[v].values())
        for name in R["ref64"]:
            C.check(f"{v} {C.case_id(c)}", name, R[v][name], R, bars=part, fracs=part_f)


def test_the_first_stages_bars_discriminate_and_the_table_is_complete():
    worst = C.measure()
    assert set(worst) == set(C.BARS) and {k for k in C.BARS if not k.startswith("grad/") and C.kind_of(k) in C.STORED_BF16} == set(C.FRACS)
    for k, (rm, rr, bad) in worst.items():
        print(f"{k}: measured max {rm:.3f} rms {rr:.3f} (bars {C.BARS[k]})" + (f" fraction off {bad:.4f} (bar {C.FRACS[k]})" if k in C.FRACS else ""))
        assert rm <= 0.75 * C.BARS[k][0] and rr <= 0.75 * C.BARS[k][1], (k, C.BARS[k], rm, rr)
    print("bars that separate the contracted rounding points from another scheme (a <= 0.75, b <= 0.35):", C.DISCRIMINATING)
    # the tensors a wrong Start operand tile, K padding, column predicate or first-layer halo shows in first
    assert {"hs0.0", "gates0.0", "acts0.0", "gates0.1", "acts0.1"} <= set(C.DISCRIMINATING)
