"""CPU: the bf16 mode of the multi-period discriminator - the restatement against the unrounded reference, the settings key, the host pack's layout, the bars
against a fresh measurement, and the argument checks of the new entry points (which return before any launch)."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hifigan_disc_bf16_cases as C  # noqa: E402
import hifigan_disc_bf16_ref as BR  # noqa: E402
import hifigan_disc_ref as HR  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402

KEY = "Vocoder.Train.Adversarial.Precision"


def hp_of(adversarial, train=None):
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Vocoder"] = {"Type": "HiFiGAN", "Train": dict(train or {}, Adversarial=adversarial)}
    return Recursive_Parse(copy.deepcopy(d))


@pytest.mark.parametrize("case", ["narrow_b3", "k48_80"])
def test_without_the_rounding_the_restatement_is_the_reference(case):
    periods, channels, _, _ = C.CASES[case]
    sd, wav = C.case_inputs(case, 1234)
    want = C.tensors(HR.score_grads(sd, wav, periods, len(channels), C.SLOPE, 1.0))
    got = C.tensors(BR.score_grads(sd, wav, periods, len(channels), C.SLOPE, 1.0, rounding=False))
    rounded = C.tensors(BR.score_grads(sd, wav, periods, len(channels), C.SLOPE, 1.0))
    assert set(got) == set(want)
    for k in want:
        assert C.dist(got[k], want[k]) <= 1e-12 * float(want[k].abs().max()), k
        assert C.dist(rounded[k], want[k]) > 1e-6 * float(want[k].abs().max()), k      # and the rounding is not a no-op on any of them


def test_bf16_rounds_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 3.0e38, -1.0e-30], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 0.0, 0.0], dtype=torch.float64)
    got = BR.bf16(x)
    assert torch.equal(got[:3], want[:3])                   # ties to even, above a tie up
    assert torch.isfinite(got[3]) and abs(float(got[3]) / 3.0e38 - 1) < 2.0 ** -8 and got[4] != 0      # fp32's range: no clamp, no flush of 1e-30


def test_the_key_is_parsed_and_appears_only_when_present():
    from glow_tts_amd.hifigan_trainer import train_settings
    from glow_tts_amd.vocoder import MPD_DEFAULTS, hifigan_disc_precision, hifigan_disc_settings
    block = {"Periods": [2, 3], "Channels": C.NARROW}
    plain, keyed = hifigan_disc_settings(hp_of(block)), hifigan_disc_settings(hp_of(dict(block, Precision="bf16")))
    assert "Precision" not in MPD_DEFAULTS and "Precision" not in plain
    assert keyed == dict(plain, Precision="bf16")
    assert hifigan_disc_settings(hp_of(dict(block, Precision="f32")))["Precision"] == "f32"
    assert hifigan_disc_precision(hp_of(block)) == "f32" and hifigan_disc_precision(hp_of(dict(block, Precision="bf16"))) == "bf16"
    assert hifigan_disc_precision(hp_of(dict(block, Precision="bf16")), "f32") == "f32"        # the argument wins
    assert train_settings(hp_of(dict(block, Precision="bf16")))["Adversarial"]["Precision"] == "bf16"
    assert "Precision" not in train_settings(hp_of(block))["Adversarial"]
    # the generator's key is another key: both may be set
    s = train_settings(hp_of(dict(block, Precision="bf16"), {"Precision": "mixed"}))
    assert s["Precision"] == "mixed" and s["Adversarial"]["Precision"] == "bf16"


@pytest.mark.parametrize("bad", ["fp16", "mixed", "BF16", 16, None])
def test_a_bad_value_is_named_before_the_device_is_touched(bad):
    from glow_tts_amd.vocoder import HiFiGANDiscriminators, HiFiGANPeriodDiscriminator, hifigan_disc_settings
    block = {"Periods": [2, 3], "Channels": C.NARROW}
    if bad is not None:
        with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
            hifigan_disc_settings(hp_of(dict(block, Precision=bad)))
        with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
            HiFiGANPeriodDiscriminator(hp_of(dict(block, Precision=bad)), "cuda:0")
    for cls, blk in ((HiFiGANPeriodDiscriminator, block), (HiFiGANDiscriminators, dict(block, Multi_Scale={}))):
        with pytest.raises(ValueError, match="precision = ") as err:
            cls(hp_of(blk), "cuda:0", precision=bad if bad is not None else "f64")
        assert "multi-scale discriminator is f32" in str(err.value)


def test_the_host_pack_layout():
    from glow_tts_amd.vocoder import hifigan_disc_pack_bf16, hifigan_disc_pack_plan, hifigan_disc_geometry, HIFIGAN_PACK_KINDS
    g = torch.Generator().manual_seed(3)
    for co, ci in ((32, 16), (80, 48), (16, 80)):
        w = torch.randn(co, ci, 5, 1, generator=g)
        fwd, kt = hifigan_disc_pack_bf16(w)
        cip, cop = (ci + 31) // 32 * 32, (co + 31) // 32 * 32
        assert fwd.dtype == kt.dtype == torch.bfloat16 and fwd.shape == (5, cip // 8, co, 8) and kt.shape == (5, cop // 8, ci, 8)
        assert fwd.is_contiguous() and kt.is_contiguous()
        r = w[..., 0].to(torch.bfloat16)
        for tap, k, n in ((0, 0, 0), (4, ci - 1, co - 1), (2, 9, 5), (1, 8, 15)):
            assert fwd[tap, k // 8, n, k % 8] == r[n, k, tap]                  # (tap, input channel, output channel)
        for tap, k, n in ((0, 0, 0), (4, co - 1, ci - 1), (2, 9, 5), (3, 15, 8)):
            assert kt[tap, k // 8, n, k % 8] == r[k, n, tap]                   # (tap, output channel, input channel): the tap is NOT reversed
        full, full_t = fwd.permute(0, 1, 3, 2).reshape(5, cip, co), kt.permute(0, 1, 3, 2).reshape(5, cop, ci)      # [tap][k][n]
        assert torch.equal(full[:, :ci], r.permute(2, 1, 0)) and not full[:, ci:].any()
        assert torch.equal(full_t[:, :co], r.permute(2, 0, 1)) and not full_t[:, co:].any()
    geo = hifigan_disc_geometry(hp_of({"Periods": [2, 3], "Channels": [16, 48, 80]}))
    plan = hifigan_disc_pack_plan(geo)
    assert [(key, kind) for key, kind, *_ in plan] == [(f"discriminators.{i}.convs.{j}.weight", kind) for i in range(2) for j in (1, 2)
                                                       for kind in ("conv_bf16", "conv_kt_bf16")]
    assert [shape for *_, shape, _ in plan][:4] == [(5, 4, 48, 8), (5, 8, 16, 8), (5, 8, 80, 8), (5, 12, 48, 8)]
    assert HIFIGAN_PACK_KINDS["conv_bf16"] == 5 and HIFIGAN_PACK_KINDS["conv_kt_bf16"] == 6
    assert {k: v for k, v in HIFIGAN_PACK_KINDS.items() if v < 5} == {"conv_f16": 0, "up_f16": 1, "conv_t_bf16": 2, "up_t_bf16": 3, "post_f32": 4}


def test_the_bars_follow_from_the_reference_arithmetic():
    """A fresh measurement of the cases that set the bars: the constants are this arithmetic's, no pair misses the guard, and a float32 realisation of the
    contract - which is what the kernels are - holds both bars with the margins the bars were given."""
    m = C.measure(cases=("narrow_b3", "rows65", "k48_80", "default_p11"))
    assert [d for d in m["dropped"]] == list(C.DROPPED) and len(C.DROPPED) <= C.MAX_DROPPED * m["pairs"]
    assert abs(m["worst_a"] / C.WORST_A - 1) < 0.05, m["worst_a"]
    assert m["worst_b"] <= 1.5 * C.WORST_B, m["worst_b"]
    assert C.BAR_A == 1.5 * C.WORST_A and C.BAR_B == 2.0 * C.WORST_B
    assert set(C.NARROW_CASES) == {c for c, v in C.CASES.items() if v[1] == C.NARROW} and "default_p11" not in C.NARROW_CASES
    assert list(C.CASES)[:7] == ["narrow_b3", "p7_pad6", "t2p", "rows63", "rows64", "rows65", "splits"] and C.CASES["p16"][0] == [16]


def test_the_entry_points_check_their_arguments_before_any_launch():
    from glow_tts_amd import _lib, abi
    lib = _lib.api()
    assert lib.glowtts_hifigan_disc_supported_bf16(11, 1024, 1024) == 1 and lib.glowtts_hifigan_disc_supported_bf16(16, 16, 48) == 1
    assert lib.glowtts_hifigan_disc_supported_bf16(3, 1, 32) == 1 and lib.glowtts_hifigan_disc_supported_bf16(3, 32, 1) == 1      # the f32 launches' layers
    assert lib.glowtts_hifigan_disc_supported_bf16(1, 32, 32) == 0 and lib.glowtts_hifigan_disc_supported_bf16(17, 32, 32) == 0
    assert lib.glowtts_hifigan_disc_supported_bf16(3, 24, 32) == 0 and lib.glowtts_hifigan_disc_supported_bf16(3, 32, 2048) == 0
    for name in ("glowtts_hifigan_disc_supported_bf16", "glowtts_hifigan_disc_conv_bf16", "glowtts_hifigan_disc_conv_bwd_bf16", "glowtts_hifigan_disc_wgrad_bf16"):
        assert name in abi.SIGNATURES
    raw = _lib.lib()
    assert raw.glowtts_abi_version() == 7
    with pytest.raises(_lib.GlowTTSHipError):
        lib.glowtts_hifigan_disc_conv_bf16(None, None, None, None, 1, 4, 3, 3, 16, 32, 0.1, None)
    with pytest.raises(_lib.GlowTTSHipError):
        lib.glowtts_hifigan_disc_conv_bwd_bf16(None, None, None, None, None, None, 1, 4, 3, 3, 16, 32, 0.1, None)
    with pytest.raises(_lib.GlowTTSHipError):
        lib.glowtts_hifigan_disc_wgrad_bf16(None, None, None, None, None, 1, 4, 3, 3, 16, 32, 5, 0, 0.1, None)
