"""GPU: the HiFi-GAN multi-period discriminator and the feature-matching loss (csrc/hifigan_disc_ops.hip through `vocoder.HiFiGANPeriodDiscriminator`)
against tests/hifigan_disc_ref.py.  The bar is the project's own, unchanged (`pwg_train_ref.check`): max |hip - ref64| / max |ref64| <= 4 e32 + 1e-6 with e32
from the float32 run of the reference on the CPU and the guards 0 < e32 < 1e-3, max |ref64| > 1e-3 - separately for every period's scores, every feature
map, L_fm, the losses, d wav and every parameter gradient.  Weights: the init rule times 3, signals: white noise of amplitude 0.3.  With these two the
float64 / float32 reference alone holds every guard at every case used here (tests/test_hifigan_disc_cpu.py::test_the_gpu_cases_hold_the_guards asserts
exactly that on the CPU, from this file's own CASES)."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hifigan_disc_ref as HR  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
from helpers import launch_counts, launch_reset, tiny_hp_dict  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
SLOPE, WEIGHT_SCALE, AMPLITUDE = 0.1, 3.0, 0.3
NARROW = [16, 32, 16]
DEFAULT = [32, 128, 512, 1024, 1024]
CASES = {
    # name: (Periods, Channels, B, T)
    "narrow_b3": ([2, 3], NARROW, 3, 50),          # no pad for 2, pad 1 for 3; every layer far below one tile: a tile would straddle batch rows
    "p7_pad6": ([7], NARROW, 2, 50),               # 50 = 7 * 7 + 1: the largest pad, p - 1
    "t2p": ([5], NARROW, 2, 10),                   # T = 2 p: H0 = 2, nearly every tap outside
    "rows63": ([3], NARROW, 2, 542),               # the second layer writes 21 * 3 = 63 flat rows (pad 1)
    "rows64": ([2], NARROW, 2, 559),               # 32 * 2 = 64 (pad 1)
    "rows65": ([5], NARROW, 2, 541),               # 13 * 5 = 65 (pad 4)
    "splits": ([3], NARROW, 1, 3300),              # the first layer writes 367 * 3 = 1101 rows: two chunks of the weight-gradient partition
    "default_p11": ([11], DEFAULT, 1, 600),        # 16 K chunks, 8 column groups, a 1024-wide conv_post
    "c64_80": ([3], [64, 64, 80], 2, 200),         # the (4, 1) layout in both directions; 80 source channels: a K walk of 64 + 16
}
_cache = {}


def hp_of(periods, channels):
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Vocoder"] = {"Type": "HiFiGAN", "Train": {"Adversarial": {"Periods": periods, "Channels": channels, "Negative_Slope": SLOPE}}}
    return Recursive_Parse(copy.deepcopy(d))


def case_inputs(case):
    periods, channels, B, T = CASES[case]
    g = torch.Generator().manual_seed(7)
    return HR.random_state_dict(periods, channels, 1234, WEIGHT_SCALE), (torch.randn(B, T, generator=g) * AMPLITUDE).float()


def case_reference(case):
    """Computed once per case, shared and left unchanged"""
    if case not in _cache:
        periods, channels, _, _ = CASES[case]
        sd, wav = case_inputs(case)
        _cache[case] = tuple(HR.score_grads(sd, wav, periods, len(channels), SLOPE, 1.0, dtype=dt) for dt in (torch.float64, torch.float32))
    return _cache[case]


def build(case):
    from glow_tts_amd.vocoder import HiFiGANPeriodDiscriminator
    periods, channels, _, _ = CASES[case]
    sd, wav = case_inputs(case)
    return HiFiGANPeriodDiscriminator(hp_of(periods, channels), "cuda:0", state_dict={"discriminator": sd}), wav.cuda()


def step(disc, wav, value=1.0, freeze=False):
    """score + sum of the periods' least-squares losses + backward through autograd -> dict(scores, loss, dwav, grads)"""
    from glow_tts_amd.vocoder import adversarial_mse
    for p in disc.params.values():
        p.grad = None
    x = wav.clone().requires_grad_(True)
    scores = disc.score(x, freeze=freeze)
    loss = sum(adversarial_mse(s, value)[0] for s in scores)
    loss.backward()
    torch.cuda.synchronize()
    return {"scores": [s.detach() for s in scores], "loss": loss.detach().reshape(1), "dwav": x.grad, "grads": {k: p.grad for k, p in disc.params.items()}}


def collect(failed, name, got, r64, r32):
    assert tuple(got.shape) == tuple(r64.shape), (name, got.shape, r64.shape)
    try:
        TR.check(name, got, r64, r32)
    except AssertionError as err:
        failed.append(str(err))


@pytest.mark.parametrize("case", list(CASES))
def test_operators_match_the_float64_reference(case):
    from glow_tts_amd.vocoder import hifigan_disc_feature_maps, hifigan_disc_forward
    r64, r32 = case_reference(case)
    disc, wav = build(case)
    got = step(disc, wav)
    fwd = hifigan_disc_forward(disc, wav)
    failed = []
    for i, per in enumerate(fwd["periods"]):
        assert torch.equal(per["scores"], got["scores"][i])
        collect(failed, f"{case} scores[{i}]", got["scores"][i], r64["scores"][i], r32["scores"][i])
        maps = hifigan_disc_feature_maps(disc, per)
        assert len(maps) == len(r64["maps"][i])
        for j, m in enumerate(maps):
            collect(failed, f"{case} map[{i}][{j}]", m, r64["maps"][i][j], r32["maps"][i][j])
    for name in ("loss", "dwav"):
        collect(failed, f"{case} {name}", got[name], r64[name], r32[name])
    assert set(got["grads"]) == set(r64["grads"])
    for name in r64["grads"]:
        collect(failed, f"{case} {name}", got["grads"][name], r64["grads"][name], r32["grads"][name])
    assert not failed, failed


def test_guard_rows_are_neither_read_nor_written():
    """Inputs carry 1e3 and every output NaN in a spare row after the last batch row: the spare row stays NaN and no result changes."""
    from glow_tts_amd.vocoder import hifigan_disc_backward, hifigan_disc_forward
    case = "narrow_b3"
    _, _, B, T = CASES[case]
    disc, wav = build(case)
    plain_f = hifigan_disc_forward(disc, wav)
    g = torch.Generator().manual_seed(9)
    ds = [torch.randn(per["scores"].shape, generator=g).cuda() for per in plain_f["periods"]]
    plain_dwav, plain_grads = hifigan_disc_backward(disc, plain_f, ds)
    spare = []

    def alloc(*shape):
        if len(shape) >= 2 and shape[0] == B:
            buf = torch.full((B + 1,) + tuple(shape[1:]), NAN, device="cuda")
            spare.append(buf)
            return buf[:B]
        return torch.full(shape, NAN, device="cuda")
    padded = torch.full((B + 1, T), 1e3, device="cuda")
    padded[:B] = wav
    dsp = []
    for d in ds:
        buf = torch.full((B + 1, d.shape[1]), 1e3, device="cuda")
        buf[:B] = d
        dsp.append(buf[:B])
    f = hifigan_disc_forward(disc, padded[:B], alloc=alloc)
    dwav, grads = hifigan_disc_backward(disc, f, dsp, alloc=alloc)
    torch.cuda.synchronize()
    assert len(spare) == 2 * (3 + 1) + 2 * 3 + 1                             # per period: kept outputs and scores; a d pre per width; d wav
    assert all(torch.isnan(b[B]).all() and torch.isfinite(b[:B]).all() for b in spare)
    assert torch.equal(dwav, plain_dwav) and all(torch.equal(grads[k], plain_grads[k]) for k in plain_grads)
    for a, b in zip(f["periods"], plain_f["periods"]):
        assert torch.equal(a["scores"], b["scores"]) and all(torch.equal(x, y) for x, y in zip(a["keep"], b["keep"]))


@pytest.mark.parametrize("case", ["narrow_b3", "rows65"])
def test_a_row_is_the_same_alone_and_in_a_batch(case):
    from glow_tts_amd.vocoder import hifigan_disc_forward
    _, _, B, T = CASES[case]
    disc, wav = build(case)
    g = torch.Generator().manual_seed(9)

    def run(w, ds):
        x = w.clone().requires_grad_(True)
        scores = disc.score(x)
        sum((s * d).sum() for s, d in zip(scores, ds)).backward()
        keep = [k for per in hifigan_disc_forward(disc, w.contiguous())["periods"] for k in per["keep"]]
        return [s.detach() for s in scores], x.grad, keep
    ds = [torch.randn(s.shape, generator=g).cuda() for s in disc.score(wav)]
    scores, dwav, keep = run(wav, ds)
    for b in range(B):
        s1, d1, k1 = run(wav[b:b + 1], [d[b:b + 1] for d in ds])
        assert all(torch.equal(a[0], s[b]) for a, s in zip(s1, scores)) and torch.equal(d1[0], dwav[b]), b
        assert all(torch.equal(a[0], k[b]) for a, k in zip(k1, keep)), b


def test_two_runs_are_bit_identical():
    for case in ("narrow_b3", "splits"):
        disc, wav = build(case)
        a, b = step(disc, wav), step(disc, wav)
        assert all(torch.equal(x, y) for x, y in zip(a["scores"], b["scores"])) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["dwav"], b["dwav"])
        assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])


def test_freeze_runs_the_data_chain_alone():
    disc, wav = build("narrow_b3")
    full = step(disc, wav)
    launch_reset()
    frozen = step(disc, wav, freeze=True)
    counts = launch_counts()
    assert torch.equal(frozen["dwav"], full["dwav"]) and all(torch.equal(a, b) for a, b in zip(frozen["scores"], full["scores"]))
    assert all(g is None for g in frozen["grads"].values())
    assert not any("wgrad" in k and n for k, n in counts.items()), counts
    assert counts.get("hifigan_disc_first") == 2 and counts.get("hifigan_disc_conv") == 4 and counts.get("hifigan_disc_post") == 2
    assert counts.get("hifigan_disc_post_bwd") == 2 and counts.get("hifigan_disc_conv_bwd") == 4 and counts.get("hifigan_disc_first_bwd") == 2
    launch_reset()
    step(disc, wav)
    counts = launch_counts()
    assert counts.get("hifigan_disc_wgrad") == 8 and counts.get("hifigan_disc_wgrad_sum") == 8 and not counts.get("hifigan_wgrad")


def test_real_and_fake_as_one_batch_of_2b_rows():
    """`score_pair`: ONE forward per period over [real; fake]; L_D's gradients equal the float64 reference under the bar and do not reach the fake; the
    generator term (adversarial + feature matching, both Lambdas other than 1) gives d fake under the bar from ONE frozen data chain per period, with no
    weight-gradient launch and no parameter gradient."""
    from glow_tts_amd.vocoder import adversarial_mse
    case = "narrow_b3"
    periods, channels, B, T = CASES[case]
    n, lam_adv, lam_fm = len(channels), 1.5, 2.5
    disc, real = build(case)
    sd, _ = case_inputs(case)
    fake = (torch.randn(B, T, generator=torch.Generator().manual_seed(21)) * AMPLITUDE).float().cuda()
    p64, p32 = (HR.pair_grads(sd, real.cpu(), fake.cpu(), periods, n, SLOPE, dtype=dt) for dt in (torch.float64, torch.float32))
    g64, g32 = (HR.generator_term_grads(sd, real.cpu(), fake.cpu(), periods, n, SLOPE, lam_adv, lam_fm, dtype=dt) for dt in (torch.float64, torch.float32))
    x = fake.clone().requires_grad_(True)
    launch_reset()
    both, p_fake, l_fm, fm_terms = disc.score_pair(real, x)
    counts = launch_counts()
    assert counts.get("hifigan_disc_first") == 2 and counts.get("hifigan_disc_conv") == 2 * (n - 1) and counts.get("hifigan_disc_post") == 2
    assert counts.get("hifigan_disc_fm") == 2 * (n + 1) and counts.get("hifigan_disc_fm_sum") == 2 * (n + 1)
    assert all(b.shape == (2 * B, p.shape[1]) and torch.equal(b[B:], p) for b, p in zip(both, p_fake))
    adv = [adversarial_mse(p, 1.0)[0] for p in p_fake]
    loss = lam_adv * sum(adv) + lam_fm * l_fm
    launch_reset()
    loss.backward()
    torch.cuda.synchronize()
    counts = launch_counts()
    assert not any("wgrad" in k and c for k, c in counts.items()), counts
    assert counts.get("hifigan_disc_post_bwd") == 2 and counts.get("hifigan_disc_conv_bwd") == 2 * (n - 1) and counts.get("hifigan_disc_first_bwd") == 2, counts
    assert all(p.grad is None for p in disc.params.values())
    failed = []
    collect(failed, "L_fm", l_fm.detach().reshape(1), g64["l_fm"], g32["l_fm"])
    collect(failed, "fm terms", fm_terms, g64["fm_terms"], g32["fm_terms"])
    collect(failed, "adversarial terms", torch.stack([a.detach() for a in adv]), g64["adv_terms"], g32["adv_terms"])
    collect(failed, "generator loss", loss.detach().reshape(1), g64["loss"], g32["loss"])
    collect(failed, "generator term d fake", x.grad, g64["dfake"], g32["dfake"])
    x.grad = None
    d_loss = sum(adversarial_mse(b, (1.0, 0.0))[0] for b in both)
    d_loss.backward()
    torch.cuda.synchronize()
    assert x.grad is None
    collect(failed, "L_D", d_loss.detach().reshape(1), p64["loss"], p32["loss"])
    for name, p in disc.params.items():
        collect(failed, "L_D " + name, p.grad, p64["grads"][name], p32["grads"][name])
    assert not failed, failed
