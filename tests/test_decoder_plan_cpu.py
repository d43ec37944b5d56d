"""CPU suite: decoder.fused_flow_plan - how many forward flows of a training step stay on the per-conv launches (nskip) and how many backward
flows take the fused data-gradient kernel (nfb).  The policy is pure arithmetic over the batch's row count and the CU count; these are the
cases its comments and DESIGN.md section 5 name."""
import pytest

from glow_tts_amd import decoder as D

ROWS_B32, ROWS_B16 = 32 * 404, 16 * 404          # B x (800 frames / 2 + 4 pad rows)


def _cfg(n_flows=12, n_layers=4):
    return D.DecoderConfig(80, n_flows, 2, 4, 192, n_layers, 5)


def _plan(rows=ROWS_B32, cus=256, need_bwd=True, conditioned=False, fused_bwd_ok=True, have_image=True, cfg=None, **tune):
    saved = dict(D.TUNE)
    try:
        D.TUNE.update(tune)
        return D.fused_flow_plan(cfg or _cfg(), rows, cus, need_bwd, conditioned, fused_bwd_ok, have_image)
    finally:
        D.TUNE.clear()
        D.TUNE.update(saved)


def test_fused_workgroups_of_the_benchmarked_batches():
    # one fused workgroup per 64 - 4 (L - 1) = 52-row window
    assert -(-ROWS_B32 // 52) == 249 and -(-ROWS_B16 // 52) == 125
    assert 4 * 249 > 3 * 256 and 4 * 125 <= 3 * 256


@pytest.mark.parametrize("kw, want", [
    (dict(), (3, 9)),                                         # default decoder, chip-filling batch: skip 3 forward flows, 9 of 12 fused backward
    (dict(conditioned=True), (3, 8)),                         # conditioned modes: 8 of 12
    (dict(rows=ROWS_B16), (0, 12)),                           # a quarter of the CUs stays free: everything fused
    (dict(rows=None), (0, 9)),                                # batch unknown: no forward skip, the chip-filling share backward
    (dict(need_bwd=False), (0, 0)),
    (dict(have_image=False), (0, 0)),
])
def test_automatic_plan(kw, want):
    assert _plan(**kw) == want
    assert D.TUNE["fused_wn_fwd_skip"] == -1 and D.TUNE["fused_wn_bwd"] == -1      # (the defaults these cases are stated for)


def test_fused_backward_not_available():
    assert _plan(fused_bwd_ok=False) == (3, 0)
    assert _plan(fused_bwd_ok=False, fused_wn_bwd=True)[1] == 0


def test_explicit_settings():
    assert _plan(fused_wn_bwd=True)[1] == 12
    assert _plan(fused_wn_bwd=5)[1] == 5
    assert _plan(fused_wn_bwd=40)[1] == 12
    assert _plan(fused_wn_bwd=0)[1] == 0
    assert _plan(fused_wn_fwd_skip=1)[0] == 1
    assert _plan(fused_wn_fwd_skip=40)[0] == 12
    assert _plan(fused_wn_fwd_skip=1, need_bwd=False)[0] == 0


def test_plan_scales_with_the_chip_and_the_flow_count():
    assert _plan(cus=512) == (0, 12)                          # 249 workgroups leave half of a 512-CU chip free
    assert _plan(cfg=_cfg(n_flows=4)) == (3, 3)
    assert _plan(cfg=_cfg(n_flows=4), conditioned=True) == (3, 2)
    assert _plan(cfg=_cfg(n_flows=1)) == (1, 1)               # never fewer than one fused backward flow, never more skipped flows than there are


def test_tune_is_restored():
    before = dict(D.TUNE)
    _plan(fused_wn_bwd=5, fused_wn_fwd_skip=2)
    assert D.TUNE == before
