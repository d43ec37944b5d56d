"""GPU: the HiFi-GAN multi-scale discriminator (csrc/hifigan_msd_ops.hip and the period-1 entries of csrc/hifigan_disc_ops.hip through
`vocoder.HiFiGANScaleDiscriminator`) against tests/hifigan_msd_ref.py.  The bar is the project's own, unchanged (`pwg_train_ref.check`):
max |hip - ref64| / max |ref64| <= 4 e32 + 1e-6 with e32 from the float32 run of the reference on the CPU and the guards 0 < e32 < 1e-3, max |ref64| > 1e-3 -
separately for every scale's scores, every feature map, the loss, d wav and every parameter gradient.  Weights: the init rule times 3, signals: white noise of
amplitude 0.3.  With these two the float64 / float32 reference alone holds every guard at every case used here
(tests/test_hifigan_msd_cpu.py::test_the_gpu_cases_hold_the_guards asserts exactly that on the CPU, from this file's own CASES)."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hifigan_msd_ref as MR  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
from helpers import launch_counts, launch_reset, tiny_hp_dict  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
SLOPE, WEIGHT_SCALE, AMPLITUDE = 0.1, 3.0, 0.3
NARROW, DEFAULT = MR.NARROW, MR.DEFAULT
CASES = {
    # name: (net, Scales, B, T); the narrow net's layers: stride 1, 2, 4, 1, 1
    "b3": (NARROW, 2, 3, 200),              # every layer far below two tiles for three rows: a tile would straddle batch rows; 100 rows enter the stride-4 layer
    "t24": (NARROW, 2, 2, 24),              # nearly every tap is outside the signal
    "rows65": (NARROW, 1, 2, 513),          # the stride-4 layer reads 257 rows and writes 65
    "rows64": (NARROW, 1, 2, 512),          # 256 -> 64
    "rows63": (NARROW, 1, 2, 500),          # 250 -> 63
    "splits": (NARROW, 1, 1, 2300),         # 2300 and 1150 output rows: three and two chunks of the weight-gradient partition
    "s3": (NARROW, 3, 2, 333),              # three scales (333, 167, 84 samples); 167 rows enter the stride-4 layer
    "t203": (NARROW, 1, 2, 203),            # 102 rows enter the stride-4 layer: with 100, 257 and 167 every residue mod 4
    "default": (DEFAULT, 1, 1, 600),        # the default widths: 16 groups, Cin_g 8 .. 64, 16 K chunks of the dense layer, a 1024-wide conv_post
}
_cache = {}


def block_of(net, scales):
    return {"Scales": scales, "Channels": net["channels"], "Groups": net["groups"], "Strides": net["strides"], "Kernel_Sizes": net["kernels"]}


def hp_of(net, scales):
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Vocoder"] = {"Type": "HiFiGAN", "Train": {"Adversarial": {"Negative_Slope": SLOPE, "Multi_Scale": block_of(net, scales)}}}
    return Recursive_Parse(copy.deepcopy(d))


def case_inputs(case):
    net, scales, B, T = CASES[case]
    g = torch.Generator().manual_seed(7)
    return MR.random_state_dict(scales, net, 1234, WEIGHT_SCALE), (torch.randn(B, T, generator=g) * AMPLITUDE).float()


def case_reference(case):
    """Computed once per case, shared and left unchanged"""
    if case not in _cache:
        net, scales, _, _ = CASES[case]
        sd, wav = case_inputs(case)
        _cache[case] = tuple(MR.score_grads(sd, wav, scales, net, SLOPE, 1.0, dtype=dt) for dt in (torch.float64, torch.float32))
    return _cache[case]


def build(case):
    from glow_tts_amd.vocoder import HiFiGANScaleDiscriminator
    net, scales, _, _ = CASES[case]
    sd, wav = case_inputs(case)
    return HiFiGANScaleDiscriminator(hp_of(net, scales), "cuda:0", state_dict={"msd": sd}), wav.cuda()


def step(disc, wav, value=1.0, freeze=False):
    """score + sum of the scales' least-squares losses + backward through autograd -> dict(scores, loss, dwav, grads)"""
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
    from glow_tts_amd.vocoder import hifigan_msd_feature_maps, hifigan_msd_forward
    r64, r32 = case_reference(case)
    disc, wav = build(case)
    got = step(disc, wav)
    fwd = hifigan_msd_forward(disc, wav)
    failed = []
    assert len(fwd["scales"]) == len(r64["scores"])
    for i, sc in enumerate(fwd["scales"]):
        assert torch.equal(sc["scores"], got["scores"][i])
        collect(failed, f"{case} scores[{i}]", got["scores"][i], r64["scores"][i], r32["scores"][i])
        maps = hifigan_msd_feature_maps(disc, sc)
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
    from glow_tts_amd.vocoder import hifigan_msd_backward, hifigan_msd_forward
    case = "b3"
    net, scales, B, T = CASES[case]
    n = len(net["channels"])
    disc, wav = build(case)
    plain_f = hifigan_msd_forward(disc, wav)
    g = torch.Generator().manual_seed(9)
    ds = [torch.randn(sc["scores"].shape, generator=g).cuda() for sc in plain_f["scales"]]
    plain_dwav, plain_grads = hifigan_msd_backward(disc, plain_f, ds)
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
    f = hifigan_msd_forward(disc, padded[:B], alloc=alloc)
    dwav, grads = hifigan_msd_backward(disc, f, dsp, alloc=alloc)
    torch.cuda.synchronize()
    assert len(spare) == scales * (n + 1) + (scales - 1) + scales * n + scales     # kept outputs and scores; the pooled waveforms; a d pre per layer; d wav per scale
    assert all(torch.isnan(b[B]).all() and torch.isfinite(b[:B]).all() for b in spare)
    assert torch.equal(dwav, plain_dwav) and all(torch.equal(grads[k], plain_grads[k]) for k in plain_grads)
    for a, b in zip(f["scales"], plain_f["scales"]):
        assert torch.equal(a["scores"], b["scores"]) and all(torch.equal(x, y) for x, y in zip(a["keep"], b["keep"]))


@pytest.mark.parametrize("case", ["b3", "rows65"])
def test_a_row_is_the_same_alone_and_in_a_batch(case):
    from glow_tts_amd.vocoder import hifigan_msd_forward
    _, _, B, T = CASES[case]
    disc, wav = build(case)
    g = torch.Generator().manual_seed(9)

    def run(w, ds):
        x = w.clone().requires_grad_(True)
        scores = disc.score(x)
        sum((s * d).sum() for s, d in zip(scores, ds)).backward()
        keep = [k for sc in hifigan_msd_forward(disc, w.contiguous())["scales"] for k in sc["keep"]]
        return [s.detach() for s in scores], x.grad, keep
    ds = [torch.randn(s.shape, generator=g).cuda() for s in disc.score(wav)]
    scores, dwav, keep = run(wav, ds)
    for b in range(B):
        s1, d1, k1 = run(wav[b:b + 1], [d[b:b + 1] for d in ds])
        assert all(torch.equal(a[0], s[b]) for a, s in zip(s1, scores)) and torch.equal(d1[0], dwav[b]), b
        assert all(torch.equal(a[0], k[b]) for a, k in zip(k1, keep)), b


def test_two_runs_are_bit_identical():
    for case in ("b3", "splits"):
        disc, wav = build(case)
        a, b = step(disc, wav), step(disc, wav)
        assert all(torch.equal(x, y) for x, y in zip(a["scores"], b["scores"])) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["dwav"], b["dwav"])
        assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])


def test_launches_of_one_forward_and_one_backward():
    net, scales, _, _ = CASES["b3"]
    mid = len(net["channels"]) - 2
    disc, wav = build("b3")
    full = step(disc, wav)
    launch_reset()
    frozen = step(disc, wav, freeze=True)
    counts = launch_counts()
    assert torch.equal(frozen["dwav"], full["dwav"]) and all(torch.equal(a, b) for a, b in zip(frozen["scores"], full["scores"]))
    assert all(g is None for g in frozen["grads"].values())
    assert not any("wgrad" in k and n for k, n in counts.items()), counts
    assert not any(k.startswith("hifigan_disc") and n for k, n in counts.items()), counts
    want = {"hifigan_msd_pool": scales - 1, "hifigan_msd_first": scales, "hifigan_msd_conv": scales * mid, "hifigan_msd_dense": scales, "hifigan_msd_post": scales,
            "hifigan_msd_post_bwd": scales, "hifigan_msd_dense_bwd": scales, "hifigan_msd_conv_bwd": scales * mid, "hifigan_msd_first_bwd": scales,
            "hifigan_msd_pool_bwd": scales - 1}
    assert {k: n for k, n in counts.items() if k.startswith("hifigan_msd") and n} == want, counts
    launch_reset()
    step(disc, wav)
    counts = launch_counts()
    want.update({"hifigan_msd_wgrad": scales * mid, "hifigan_msd_wgrad_sum": scales * mid, "hifigan_msd_dense_wgrad": 2 * scales, "hifigan_msd_dense_wgrad_sum": 2 * scales,
                 "hifigan_msd_first_wgrad": scales, "hifigan_msd_first_wgrad_sum": scales})
    assert {k: n for k, n in counts.items() if k.startswith("hifigan_msd") and n} == want, counts
    assert not counts.get("hifigan_wgrad") and not counts.get("hifigan_disc_wgrad")


def test_real_and_fake_as_one_batch_of_2b_rows():
    """`score_pair`: ONE forward per scale over [real; fake]; `both`, p_fake and L_fm equal the float64 reference under the bar; L_D's gradients come from
    `both` alone and do not reach the fake; the generator term (adversarial + feature matching, both Lambdas other than 1) gives d fake under the bar from ONE
    frozen data chain per scale, with no weight-gradient launch and no parameter gradient."""
    from glow_tts_amd.vocoder import adversarial_mse
    case = "b3"
    net, scales, B, T = CASES[case]
    n, lam_adv, lam_fm = len(net["channels"]), 1.5, 2.5
    disc, real = build(case)
    sd, _ = case_inputs(case)
    fake = (torch.randn(B, T, generator=torch.Generator().manual_seed(21)) * AMPLITUDE).float().cuda()
    p64, p32 = (MR.pair_grads(sd, real.cpu(), fake.cpu(), scales, net, SLOPE, dtype=dt) for dt in (torch.float64, torch.float32))
    g64, g32 = (MR.generator_term_grads(sd, real.cpu(), fake.cpu(), scales, net, SLOPE, lam_adv, lam_fm, dtype=dt) for dt in (torch.float64, torch.float32))
    x = fake.clone().requires_grad_(True)
    launch_reset()
    both, p_fake, l_fm, fm_terms = disc.score_pair(real, x)
    counts = launch_counts()
    assert counts.get("hifigan_msd_first") == scales and counts.get("hifigan_msd_conv") == scales * (n - 2) and counts.get("hifigan_msd_post") == scales
    assert counts.get("hifigan_disc_fm") == scales * (n + 1) and counts.get("hifigan_disc_fm_sum") == scales * (n + 1)
    assert all(b.shape == (2 * B, p.shape[1]) and torch.equal(b[B:], p) for b, p in zip(both, p_fake))
    adv = [adversarial_mse(p, 1.0)[0] for p in p_fake]
    loss = lam_adv * sum(adv) + lam_fm * l_fm
    launch_reset()
    loss.backward()
    torch.cuda.synchronize()
    counts = launch_counts()
    assert not any("wgrad" in k and c for k, c in counts.items()), counts
    assert counts.get("hifigan_msd_post_bwd") == scales and counts.get("hifigan_msd_conv_bwd") == scales * (n - 2) and counts.get("hifigan_msd_first_bwd") == scales
    assert all(p.grad is None for p in disc.params.values())
    failed = []
    for i in range(scales):
        collect(failed, f"both[{i}]", both[i].detach(), p64["both"][i], p32["both"][i])
        collect(failed, f"p_fake[{i}]", p_fake[i].detach(), g64["p_fake"][i], g32["p_fake"][i])
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


def test_refusals():
    """What the kernels do not support is refused by the entry points (GLOWTTS_E_ARG through the binding) and by the class before any launch."""
    from glow_tts_amd import _lib
    from glow_tts_amd.vocoder import MSD_MIN_SAMPLES
    lib = _lib.api()
    good = [(1, 128, 15, 1, 1), (128, 128, 41, 2, 4), (128, 256, 41, 2, 16), (1024, 1024, 41, 1, 16), (1024, 1024, 5, 1, 1), (1024, 1, 3, 1, 1), (16, 32, 41, 2, 2)]
    bad = [(1, 128, 17, 1, 1), (1, 128, 15, 2, 1), (128, 128, 43, 2, 4), (128, 128, 40, 2, 4), (128, 128, 41, 3, 4), (128, 128, 41, 2, 1), (128, 256, 41, 2, 32),
           (128, 120, 41, 2, 4), (1040, 1040, 41, 1, 65), (1, 1, 3, 1, 1), (1024, 1, 5, 1, 1), (24, 32, 41, 2, 8)]
    assert all(lib.glowtts_hifigan_msd_supported(*a) for a in good) and not any(lib.glowtts_hifigan_msd_supported(*a) for a in bad)
    assert not lib.glowtts_hifigan_disc_supported(1, 16, 16)                                             # period 1 stays refused by the multi-period entry points
    disc, wav = build("t24")
    x, y = torch.zeros(2, 24, 16, device="cuda"), torch.zeros(2, 12, 32, device="cuda")
    w, b = torch.zeros(2, 41 * 8, 16, device="cuda"), torch.zeros(32, device="cuda")
    P = _lib.ptr
    with pytest.raises(_lib.GlowTTSHipError):
        lib.glowtts_hifigan_msd_conv(P(x), P(w), P(b), P(y), 2, 24, 41, 3, 2, 16, 32, 0.1, _lib.stream())      # stride 3
    with pytest.raises(_lib.GlowTTSHipError):
        lib.glowtts_hifigan_msd_conv(P(x), P(w), P(b), P(x), 2, 24, 41, 2, 2, 16, 32, 0.1, _lib.stream())      # in place
    with pytest.raises(_lib.GlowTTSHipError):
        lib.glowtts_hifigan_disc_conv(P(x), P(w), P(b), P(y), 2, 24, 1, 1, 16, 32, 0.1, _lib.stream())         # period 1 through the multi-period entry
    with pytest.raises(ValueError, match=r"Vocoder\.Train\.Adversarial\.Multi_Scale"):
        disc.score(torch.zeros(2, MSD_MIN_SAMPLES - 1, device="cuda"))
    with pytest.raises(_lib.GlowTTSHipError):
        disc.score(wav.cpu())
    with pytest.raises(ValueError, match="differ in shape"):
        disc.score_pair(wav, wav[:1])
