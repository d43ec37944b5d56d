"""GPU: the bf16 mode of the HiFi-GAN multi-period discriminator (csrc/hifigan_disc_bf16_ops.hip through `ops.*` and `vocoder.HiFiGANPeriodDiscriminator(...,
precision='bf16')`) against tests/hifigan_disc_bf16_ref.py, the contract of DESIGN.md "The multi-period discriminator in bf16".  Shapes and bars:
tests/hifigan_disc_bf16_cases.py, whose bars come from reference arithmetic on the CPU alone.  Every figure is printed before it is asserted."""
import copy
import hashlib
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hifigan_disc_bf16_cases as C  # noqa: E402
import hifigan_disc_bf16_ref as BR  # noqa: E402
import hifigan_disc_ref as HR  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
from helpers import launch_counts, launch_reset, tiny_hp_dict  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
NEW = ("hifigan_disc_conv_bf16", "hifigan_disc_conv_bwd_bf16", "hifigan_disc_wgrad_bf16")


def hp_of(periods, channels, precision=None, multi_scale=None):
    from glow_tts_amd.hparams import Recursive_Parse
    adv = {"Periods": periods, "Channels": channels, "Negative_Slope": C.SLOPE}
    if precision is not None:
        adv["Precision"] = precision
    if multi_scale is not None:
        adv["Multi_Scale"] = multi_scale
    d = tiny_hp_dict("Vanilla")
    d["Vocoder"] = {"Type": "HiFiGAN", "Train": {"Adversarial": adv}}
    return Recursive_Parse(copy.deepcopy(d))


def build(case, seed=1234, precision="bf16", by_key=False):
    from glow_tts_amd.vocoder import HiFiGANPeriodDiscriminator
    periods, channels, _, _ = C.CASES[case]
    sd, wav = C.case_inputs(case, seed)
    if by_key:
        disc = HiFiGANPeriodDiscriminator(hp_of(periods, channels, precision), "cuda:0", state_dict={"discriminator": sd})
    else:
        disc = HiFiGANPeriodDiscriminator(hp_of(periods, channels), "cuda:0", state_dict={"discriminator": sd}, precision=precision)
    return disc, wav.cuda()


def step(disc, wav, value=1.0, freeze=False):
    """score + sum of the periods' least-squares losses + backward through autograd -> score_grads' dict (maps: the feature maps of a second forward)"""
    from glow_tts_amd.vocoder import adversarial_mse, hifigan_disc_feature_maps, hifigan_disc_forward
    for p in disc.params.values():
        p.grad = None
    x = wav.clone().requires_grad_(True)
    scores = disc.score(x, freeze=freeze)
    loss = sum(adversarial_mse(s, value)[0] for s in scores)
    loss.backward()
    fwd = hifigan_disc_forward(disc, wav)
    torch.cuda.synchronize()
    assert all(torch.equal(per["scores"], s) for per, s in zip(fwd["periods"], scores))
    return {"scores": [s.detach() for s in scores], "maps": [hifigan_disc_feature_maps(disc, per) for per in fwd["periods"]], "loss": loss.detach().reshape(1),
            "dwav": x.grad, "grads": {k: p.grad for k, p in disc.params.items()}, "keep": [k for per in fwd["periods"] for k in per["keep"]]}


def digest(result):
    h = hashlib.sha256()
    for k, t in sorted(C.tensors(result).items()):
        h.update(k.encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# ---- operators ------------------------------------------------------------------------------------------------------------------------------------
OPERATOR_CASES = {
    # name: (period, stride, Cin, Cout, B, H)
    "narrow": (3, 3, 16, 32, 2, 67),               # (1, 2) layout; 23 * 3 = 69 output rows: two tiles, the second nearly empty
    "stride1": (2, 1, 32, 16, 3, 25),              # the last width's stride; (1, 1) layout; one tile would straddle batch rows
    "k48_80": (5, 3, 48, 80, 2, 40),               # K padded 48 -> 64; 80 columns in five (1, 1) groups
    "k80_64": (3, 3, 80, 64, 2, 50),               # a K walk of 64 + (16 -> 32); (4, 1) layout
    "wide": (16, 1, 64, 128, 1, 9),                # (4, 2) layout, the largest period
    "chunks": (3, 3, 16, 16, 1, 1101),             # 367 * 3 = 1101 output rows: two chunks of the weight-gradient partition
    "k1024": (11, 1, 1024, 128, 1, 3),             # 16 K chunks
}


def operator_inputs(name):
    p, s, ci, co, B, H = OPERATOR_CASES[name]
    g = torch.Generator().manual_seed(1234)
    Ho = (H - 1) // s + 1
    W = (torch.rand(co, ci, 5, 1, generator=g) * 2 - 1) * C.WEIGHT_SCALE / (5 * ci) ** 0.5
    b = (torch.rand(co, generator=g) * 2 - 1) * C.WEIGHT_SCALE / (5 * ci) ** 0.5
    x, dy, inj = torch.randn(B, H * p, ci, generator=g), torch.randn(B, Ho * p, co, generator=g), torch.randn(B, H * p, ci, generator=g)
    return W, b, x, dy, inj


@pytest.mark.parametrize("name", list(OPERATOR_CASES))
def test_the_three_launches_round_exactly(name):
    """ops.* on float32 inputs: max |got - emu64| / max |emu64| <= 4 e32' + 1e-6, e32' the float32 realisation's error on the same call"""
    from glow_tts_amd import _lib, ops
    from glow_tts_amd.vocoder import hifigan_disc_pack_bf16
    p, s, ci, co, B, H = OPERATOR_CASES[name]
    Ho = (H - 1) // s + 1
    W, b, x, dy, inj = operator_inputs(name)
    fwd_im, kt_im = (t.cuda() for t in hifigan_disc_pack_bf16(W))
    xc, dyc, injc, bc = x.cuda(), dy.cuda(), inj.cuda(), b.cuda()
    launch_reset()
    out = torch.full((B, Ho * p, co), NAN, device="cuda")
    ops.hifigan_disc_conv_bf16(xc, fwd_im, bc, out, H, p, s, C.SLOPE)
    dx = torch.full((B, H * p, ci), NAN, device="cuda")
    scale = torch.tensor([0.7], device="cuda")
    ops.hifigan_disc_conv_bwd_bf16(dyc, kt_im, xc, dx, H, p, s, C.SLOPE, inj=injc, inj_scale=scale)
    dx0 = torch.full((B, H * p, ci), NAN, device="cuda")
    ops.hifigan_disc_conv_bwd_bf16(dyc, kt_im, xc, dx0, H, p, s, C.SLOPE)
    work = torch.empty(_lib.api().glowtts_hifigan_disc_work_floats(B, Ho * p, ci, co, 5), device="cuda")
    dw, db = torch.full((co, ci, 5, 1), NAN, device="cuda"), torch.full((co,), NAN, device="cuda")
    ops.hifigan_disc_wgrad_bf16(xc, dyc, work, dw, db, H, p, s, C.SLOPE)
    torch.cuda.synchronize()
    counts = launch_counts()
    assert {k: counts.get(k) for k in NEW} == {NEW[0]: 1, NEW[1]: 2, NEW[2]: 1} and counts.get("hifigan_disc_wgrad_sum") == 1, counts
    want = {}
    for dt in (torch.float64, torch.float32):
        w_, db_ = BR.op_wgrad(x, dy, W.shape, p, s, C.SLOPE, dtype=dt)
        want[dt] = {"conv": BR.op_conv(x, W, b, p, s, C.SLOPE, dtype=dt), "conv_bwd": BR.op_conv_bwd(dy, W, x, p, s, C.SLOPE, inj, 0.7, dtype=dt),
                    "conv_bwd, nothing injected": BR.op_conv_bwd(dy, W, x, p, s, C.SLOPE, dtype=dt), "wgrad": w_, "wgrad bias": db_}
    got = {"conv": out, "conv_bwd": dx, "conv_bwd, nothing injected": dx0, "wgrad": dw, "wgrad bias": db}
    failed = []
    for k, t in got.items():
        assert tuple(t.shape) == tuple(want[torch.float64][k].shape), k
        try:
            TR.check(f"{name} {k}", t, want[torch.float64][k], want[torch.float32][k])
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, failed


def test_the_ops_refuse_a_wrong_image_and_bad_sizes():
    from glow_tts_amd import _lib, ops
    from glow_tts_amd.vocoder import hifigan_disc_pack_bf16
    W, b, x, dy, _ = operator_inputs("narrow")
    p, s, ci, co, B, H = OPERATOR_CASES["narrow"]
    fwd_im, kt_im = (t.cuda() for t in hifigan_disc_pack_bf16(W))
    out = torch.zeros(B, dy.shape[1], co, device="cuda")
    launch_reset()
    for bad in (kt_im, fwd_im.to(torch.float16), fwd_im.float(), fwd_im[:4].contiguous()):
        with pytest.raises(_lib.GlowTTSHipError, match="hifigan_disc_pack_bf16"):
            ops.hifigan_disc_conv_bf16(x.cuda(), bad, b.cuda(), out, H, p, s, C.SLOPE)
    with pytest.raises(_lib.GlowTTSHipError, match="hifigan_disc_pack_bf16"):
        ops.hifigan_disc_conv_bwd_bf16(dy.cuda(), fwd_im, x.cuda(), torch.zeros_like(x).cuda(), H, p, s, C.SLOPE)
    with pytest.raises(_lib.GlowTTSHipError):                       # stride 2 is no stride of the architecture
        ops.hifigan_disc_conv_bf16(x.cuda(), fwd_im, b.cuda(), out, H, p, 2, C.SLOPE)
    with pytest.raises(_lib.GlowTTSHipError):                       # period 1 is the multi-scale discriminator's
        ops.hifigan_disc_conv_bf16(x.cuda(), fwd_im, b.cuda(), out, H * p, 1, s, C.SLOPE)
    # every buffer's dtype, device, contiguity and size is checked against H, period and stride before the launch: a short `out` would be written past its end
    xc, dyc, bc, good = x.cuda(), dy.cuda(), b.cuda(), fwd_im
    work = torch.empty(_lib.api().glowtts_hifigan_disc_work_floats(B, dy.shape[1], ci, co, 5), device="cuda")
    dw, db, dx = torch.zeros(co, ci, 5, 1, device="cuda"), torch.zeros(co, device="cuda"), torch.zeros_like(xc)
    bad_calls = [lambda: ops.hifigan_disc_conv_bf16(xc, good, bc, out[:, :-1].contiguous(), H, p, s, C.SLOPE),           # a row short
                 lambda: ops.hifigan_disc_conv_bf16(xc, good, bc, out[:1], H, p, s, C.SLOPE),                            # a batch row short
                 lambda: ops.hifigan_disc_conv_bf16(xc, good, bc, out, H + 1, p, s, C.SLOPE),                            # H disagrees with x
                 lambda: ops.hifigan_disc_conv_bf16(xc.double(), good, bc, out, H, p, s, C.SLOPE),
                 lambda: ops.hifigan_disc_conv_bf16(x, good, bc, out, H, p, s, C.SLOPE),                                 # x on the host
                 lambda: ops.hifigan_disc_conv_bf16(xc, good.cpu(), bc, out, H, p, s, C.SLOPE),                          # the image on the host
                 lambda: ops.hifigan_disc_conv_bf16(xc, good, bc[:-1], out, H, p, s, C.SLOPE),
                 lambda: ops.hifigan_disc_conv_bf16(xc.transpose(1, 2).contiguous().transpose(1, 2), good, bc, out, H, p, s, C.SLOPE),
                 lambda: ops.hifigan_disc_conv_bwd_bf16(dyc, kt_im, xc, dx[:, :-1].contiguous(), H, p, s, C.SLOPE),
                 lambda: ops.hifigan_disc_conv_bwd_bf16(dyc[:, :-1].contiguous(), kt_im, xc, dx, H, p, s, C.SLOPE),
                 lambda: ops.hifigan_disc_conv_bwd_bf16(dyc, kt_im, xc, dx, H, p, s, C.SLOPE, inj=dx[:1], inj_scale=torch.ones(1, device="cuda")),
                 lambda: ops.hifigan_disc_conv_bwd_bf16(dyc, kt_im, xc, dx, H, p, s, C.SLOPE, inj=dx),                  # no scale
                 lambda: ops.hifigan_disc_wgrad_bf16(xc, dyc, work[:-1], dw, db, H, p, s, C.SLOPE),
                 lambda: ops.hifigan_disc_wgrad_bf16(xc, dyc, work, dw[:-1], db, H, p, s, C.SLOPE),
                 lambda: ops.hifigan_disc_wgrad_bf16(xc, dyc, work, dw, db[:-1], H, p, s, C.SLOPE),
                 lambda: ops.hifigan_disc_wgrad_bf16(xc, dyc[:, :-1].contiguous(), work, dw, db, H, p, s, C.SLOPE)]
    for i, call in enumerate(bad_calls):
        with pytest.raises(_lib.GlowTTSHipError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    torch.cuda.synchronize()
    assert not any(launch_counts().get(k) for k in NEW)


# ---- the whole discriminator ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", C.SEEDS)
@pytest.mark.parametrize("case", list(C.CASES))
def test_the_discriminator_holds_both_bars(case, seed):
    """score + adversarial_mse + backward: per period scores, every feature map the mode reaches, d wav and every parameter gradient.
    (a) |got - ref64| <= BAR_A e_mix on every case; (b) |got - emu64| <= BAR_B e_mix on the narrow cases; pairs with e_mix <= 100 e32 are dropped by name."""
    ref = C.references(case, seed)
    figs = C.pair_figures(case, seed)
    disc, wav = build(case, seed)
    assert disc.precision == "bf16"
    whole = step(disc, wav)
    got = C.tensors(whole)
    # the first layer's map is no pair of the bars (f32 launches in both modes, e_mix = 0): it is the f32 mode's, bit for bit, on every case
    from glow_tts_amd.vocoder import hifigan_disc_feature_maps, hifigan_disc_forward
    f32 = hifigan_disc_forward(build(case, seed, precision="f32")[0], wav)
    for i, per in enumerate(f32["periods"]):
        assert torch.equal(hifigan_disc_feature_maps(disc, per)[0], whole["maps"][i][0]), (case, seed, i)
    r64, e64 = C.tensors(ref["ref64"]), C.tensors(ref["emu64"])
    assert set(got) == set(r64)
    failed, dropped = [], []
    for k, t in got.items():
        assert tuple(t.shape) == tuple(r64[k].shape), k
        f = figs[k]
        if not C.compared(f):
            dropped.append(f"{case}/{seed}/{k}")
            continue
        a, b = C.dist(t.cpu(), r64[k]) / f["e_mix"], C.dist(t.cpu(), e64[k]) / f["e_mix"]
        print(f"{case}/{seed} {k}: e_mix {f['e_mix']:.3e}  |got - ref64| / e_mix {a:.4f} (bar {C.BAR_A:.4f})  |got - emu64| / e_mix {b:.5f}"
              + (f" (bar {C.BAR_B:.5f})" if case in C.NARROW_CASES else " (no bar: a wide case)"))
        if not a <= C.BAR_A:
            failed.append((k, "a", a))
        if case in C.NARROW_CASES and not b <= C.BAR_B:
            failed.append((k, "b", b))
    assert set(dropped) <= set(C.DROPPED), dropped
    assert not failed, failed


@pytest.mark.parametrize("case", ["narrow_b3", "rows65"])
def test_score_pair_holds_the_restatement(case):
    """`score_pair` keeps its contract - ONE forward over 2 B rows, one frozen data chain per period for p_fake and l_fm - and both, p_fake, l_fm, fm_terms,
    d fake and L_D's parameter gradients hold the bf16 restatement of pair_grads / generator_term_grads under bar (b)."""
    from glow_tts_amd.vocoder import adversarial_mse
    periods, channels, B, T = C.CASES[case]
    n, lam_adv, lam_fm = len(channels), 1.5, 2.5
    disc, real = build(case)
    sd, _ = C.case_inputs(case, 1234)
    fake = (torch.randn(B, T, generator=torch.Generator().manual_seed(21)) * C.AMPLITUDE).float().cuda()
    rc, fc = real.cpu(), fake.cpu()
    p64, p32 = (HR.pair_grads(sd, rc, fc, periods, n, C.SLOPE, dtype=dt) for dt in (torch.float64, torch.float32))
    g64, g32 = (HR.generator_term_grads(sd, rc, fc, periods, n, C.SLOPE, lam_adv, lam_fm, dtype=dt) for dt in (torch.float64, torch.float32))
    pe, ge = BR.pair_grads(sd, rc, fc, periods, n, C.SLOPE), BR.generator_term_grads(sd, rc, fc, periods, n, C.SLOPE, lam_adv, lam_fm)
    x = fake.clone().requires_grad_(True)
    launch_reset()
    both, p_fake, l_fm, fm_terms = disc.score_pair(real, x)
    counts = launch_counts()
    assert counts.get("hifigan_disc_first") == len(periods) and counts.get(NEW[0]) == len(periods) * (n - 1) and counts.get("hifigan_disc_post") == len(periods)
    assert counts.get("hifigan_pack_images") == 1 and not counts.get("hifigan_disc_conv"), counts
    assert all(b.shape == (2 * B, p.shape[1]) and torch.equal(b[B:], p) for b, p in zip(both, p_fake))
    adv = [adversarial_mse(p, 1.0)[0] for p in p_fake]
    loss = lam_adv * sum(adv) + lam_fm * l_fm
    launch_reset()
    loss.backward()
    torch.cuda.synchronize()
    counts = launch_counts()
    assert not any("wgrad" in k and c for k, c in counts.items()), counts
    assert counts.get("hifigan_disc_post_bwd") == len(periods) and counts.get(NEW[1]) == len(periods) * (n - 1) and not counts.get("hifigan_disc_conv_bwd"), counts
    assert counts.get("hifigan_disc_first_bwd") == len(periods) and all(p.grad is None for p in disc.params.values())
    dfake = x.grad
    x.grad = None
    d_loss = sum(adversarial_mse(b, (1.0, 0.0))[0] for b in both)
    d_loss.backward()
    torch.cuda.synchronize()
    assert x.grad is None
    # (name, got, the contract in float64, the unrounded network in float64 and float32)
    rows = [("l_fm", l_fm.detach().reshape(1), ge["l_fm"], g64["l_fm"], g32["l_fm"]), ("fm_terms", fm_terms, ge["fm_terms"], g64["fm_terms"], g32["fm_terms"]),
            ("d fake", dfake, ge["dfake"], g64["dfake"], g32["dfake"]), ("generator loss", loss.detach().reshape(1), ge["loss"], g64["loss"], g32["loss"]),
            ("L_D", d_loss.detach().reshape(1), pe["loss"], p64["loss"], p32["loss"])]
    for i in range(len(periods)):
        rows.append((f"p_fake[{i}]", p_fake[i].detach(), ge["p_fake"][i], None, None))
        rows.append((f"both[{i}]", both[i].detach(), pe["both"][i], None, None))
    rows += [("L_D " + k, p.grad, pe["grads"][k], p64["grads"][k], p32["grads"][k]) for k, p in disc.params.items()]
    failed, dropped = [], []
    for name, got, emu, r64, r32 in rows:
        assert tuple(got.shape) == tuple(emu.shape), name
        if r64 is None:                                     # the scores: the unrounded network's are those of the whole-discriminator test; e_mix from both halves
            r64 = torch.cat([HR.forward({k: v.double() for k, v in sd.items()}, t.double(), periods, n, C.SLOPE)[int(name[-2])][0] for t in (rc, fc)])
            r32 = torch.cat([HR.forward(sd, t, periods, n, C.SLOPE)[int(name[-2])][0] for t in (rc, fc)])
            if name.startswith("p_fake"):
                r64, r32 = r64[B:], r32[B:]
        e_mix, e32 = C.dist(emu, r64), C.dist(r32, r64)
        if not e_mix > C.GUARD * e32:
            dropped.append(name)
            continue
        b = C.dist(got.cpu(), emu) / e_mix
        print(f"{case} {name}: e_mix {e_mix:.3e}  e32 {e32:.3e}  |got - emu64| / e_mix {b:.5f} (bar {C.BAR_B:.5f})")
        if not b <= C.BAR_B:
            failed.append((name, b))
    print("dropped (e_mix <= 100 e32):", dropped)
    assert len(dropped) <= C.MAX_DROPPED * len(rows), dropped
    assert not failed, failed


# ---- contract checks ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["narrow_b3", "k48_80"])
def test_the_pack_launch_writes_the_host_restatements_bytes(case):
    from glow_tts_amd.vocoder import hifigan_disc_pack_bf16
    launch_reset()
    disc, _ = build(case)
    torch.cuda.synchronize()
    assert launch_counts().get("hifigan_pack_images") == 1          # ONE launch over every period
    n = len(disc.geo["channels"])
    for i, im in enumerate(disc.images):
        assert len(im["convs"]) == n - 1
        for j, (w, b, wt) in enumerate(im["convs"], start=1):
            fwd, kt = hifigan_disc_pack_bf16(disc.params[f"discriminators.{i}.convs.{j}.weight"].detach().cpu())
            assert w.dtype == wt.dtype == torch.bfloat16 and w.shape == fwd.shape and wt.shape == kt.shape
            assert torch.equal(w.cpu().view(torch.int16), fwd.view(torch.int16)) and torch.equal(wt.cpu().view(torch.int16), kt.view(torch.int16)), (i, j)
            assert torch.equal(b, disc.params[f"discriminators.{i}.convs.{j}.bias"])
    # a forward hands ITS images to its backward: a rebuild after an update does not reach them
    old = disc.images
    kept = [[(w.clone(), wt.clone()) for w, _, wt in im["convs"]] for im in old]
    with torch.no_grad():
        for p in disc.params.values():
            p.mul_(1.25)
    launch_reset()
    disc._build_images({k: t.detach() for k, t in disc.params.items()})
    torch.cuda.synchronize()
    assert launch_counts().get("hifigan_pack_images") == 1 and disc.images is not old
    assert all(torch.equal(w, kw) and torch.equal(wt, kwt) for im, ks in zip(old, kept) for (w, _, wt), (kw, kwt) in zip(im["convs"], ks))
    fwd, _ = hifigan_disc_pack_bf16(disc.params["discriminators.0.convs.1.weight"].detach().cpu())
    assert torch.equal(disc.images[0]["convs"][0][0].cpu().view(torch.int16), fwd.view(torch.int16))


def test_guard_rows_are_neither_read_nor_written():
    """Inputs carry 1e3 and every output NaN in a spare row after the last batch row: the spare row stays NaN and no result changes."""
    from glow_tts_amd.vocoder import hifigan_disc_backward, hifigan_disc_forward
    case = "narrow_b3"
    _, _, B, T = C.CASES[case]
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
    _, _, B, T = C.CASES[case]
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
    for case in ("narrow_b3", "splits", "k48_80"):
        disc, wav = build(case)
        a, b = step(disc, wav), step(disc, wav)
        assert digest(a) == digest(b) and torch.equal(a["loss"], b["loss"]) and all(torch.equal(x, y) for x, y in zip(a["keep"], b["keep"]))


def test_the_launch_log_of_a_step_and_of_a_frozen_step():
    """A bf16 step: the three new classes, no f32 middle launch, the f32 weight gradient exactly for layer 0 and conv_post; freeze: no weight gradient."""
    disc, wav = build("narrow_b3")
    n, periods = 3, 2
    full = step(disc, wav)
    launch_reset()
    frozen = step(disc, wav, freeze=True)
    counts = launch_counts()
    assert torch.equal(frozen["dwav"], full["dwav"]) and all(torch.equal(a, b) for a, b in zip(frozen["scores"], full["scores"]))
    assert all(g is None for g in frozen["grads"].values())
    assert not any("wgrad" in k and c for k, c in counts.items()), counts
    assert counts.get("hifigan_disc_first") == 2 * periods and counts.get(NEW[0]) == 2 * periods * (n - 1) and counts.get("hifigan_disc_post") == 2 * periods
    assert counts.get("hifigan_disc_post_bwd") == periods and counts.get(NEW[1]) == periods * (n - 1) and counts.get("hifigan_disc_first_bwd") == periods
    launch_reset()
    x = wav.clone().requires_grad_(True)
    sum(s.square().mean() for s in disc.score(x)).backward()
    torch.cuda.synchronize()
    counts = launch_counts()
    assert not counts.get("hifigan_disc_conv") and not counts.get("hifigan_disc_conv_bwd"), counts
    assert counts.get(NEW[0]) == periods * (n - 1) and counts.get(NEW[1]) == periods * (n - 1) and counts.get(NEW[2]) == periods * (n - 1), counts
    assert counts.get("hifigan_disc_wgrad") == 2 * periods and counts.get("hifigan_disc_wgrad_sum") == periods * (n + 1), counts       # layer 0 and conv_post
    assert counts.get("hifigan_pack_images") == 1 and not counts.get("hifigan_wgrad") and not counts.get("hifigan_wgrad_bf16"), counts


def test_the_f32_mode_is_what_it_was():
    """No key and no argument, the key 'f32', the argument 'f32' (over a yaml that says 'bf16'): the parent's launch classes and one set of bits, before and
    after a bf16 discriminator has run; the first layer's map has those bits in the bf16 mode too."""
    from glow_tts_amd.vocoder import HiFiGANPeriodDiscriminator
    case = "rows65"
    periods, channels, _, _ = C.CASES[case]
    sd, wav = C.case_inputs(case, 1234)
    wav = wav.cuda()
    mk = lambda hp, **kw: HiFiGANPeriodDiscriminator(hp, "cuda:0", state_dict={"discriminator": sd}, **kw)
    plain = mk(hp_of(periods, channels))
    assert plain.precision == "f32"
    launch_reset()
    base = step(plain, wav)
    counts = launch_counts()
    n = len(channels)
    assert not any(counts.get(k) for k in NEW + ("hifigan_pack_images",)), counts
    assert counts.get("hifigan_disc_conv") == 2 * (n - 1) and counts.get("hifigan_disc_conv_bwd") == n - 1 and counts.get("hifigan_disc_wgrad") == n + 1, counts
    mixed, _ = build(case, by_key=True)
    assert mixed.precision == "bf16"
    other = step(mixed, wav)
    assert digest(other) != digest(base)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(other["maps"], base["maps"]))          # layer 0: f32 launches in both modes
    for disc in (mk(hp_of(periods, channels, "f32")), mk(hp_of(periods, channels), precision="f32"), mk(hp_of(periods, channels, "bf16"), precision="f32"), plain):
        assert disc.precision == "f32"
        again = step(disc, wav)
        assert digest(again) == digest(base) and all(torch.equal(a, b) for a, b in zip(again["keep"], base["keep"]))
        assert all(w.dtype == torch.float32 and wt.dtype == torch.float32 for im in disc.images for w, _, wt in im["convs"])


def test_checkpoints_are_the_same_in_both_modes():
    from glow_tts_amd.vocoder import HiFiGANPeriodDiscriminator, hifigan_disc_expected_shapes
    f32, wav = build("narrow_b3", precision="f32")
    bf16, _ = build("narrow_b3")
    assert list(f32.params) == list(bf16.params) == list(hifigan_disc_expected_shapes(f32.geo))
    assert all(p.dtype == torch.float32 and torch.equal(p, f32.params[k]) for k, p in bf16.params.items())
    periods, channels, _, _ = C.CASES["narrow_b3"]
    with torch.no_grad():
        for p in bf16.params.values():
            p.add_(0.01)
    saved = {k: p.detach().cpu().clone() for k, p in bf16.params.items()}
    for src, precision in ((saved, "f32"), (saved, "bf16")):
        disc = HiFiGANPeriodDiscriminator(hp_of(periods, channels), "cuda:0", state_dict={"discriminator": src}, precision=precision)
        assert all(torch.equal(p.detach().cpu(), saved[k]) for k, p in disc.params.items())
        assert all(torch.isfinite(s).all() for s in disc.score(wav))
    a = step(HiFiGANPeriodDiscriminator(hp_of(periods, channels), "cuda:0", state_dict={"discriminator": saved}, precision="bf16"), wav)
    assert digest(a) == digest(step(bf16, wav))                     # a resumed run continues on the same bits
