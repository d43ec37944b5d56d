"""GPU suite of the HiFi-GAN generator's mixed-precision training mode (glow_tts_amd/vocoder.py: HiFiGAN(trainable=True, train_precision='mixed') on
csrc/hifigan_f16_ops.hip and csrc/hifigan_mixed_ops.hip) against the contract restated in tests/hifigan_mixed_ref.py.  The cases and the bars are
tests/hifigan_mixed_cases.py's: they come from reference arithmetic on the CPU, never from the kernels, and every figure is printed before it is asserted
(pytest -s).  Every test constructs the mixed mode or calls one of its operators."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hifigan_mixed_cases as C  # noqa: E402
import hifigan_mixed_ref as M  # noqa: E402
import hifigan_ref as H  # noqa: E402
import hifigan_train_ref as TR  # noqa: E402
import test_gpu_hifigan as G  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402
from test_gpu_hifigan_train import beyond_is_nan, lengths_of, pad  # noqa: E402

gpu = pytest.mark.gpu
NAN = float("nan")
_VOC = {}
E64, E32, _ = M.emus(C.FC.FLUSH_SUBNORMALS)


def logged():
    return {k: c for k, c in launch_counts().items() if c}


def mvoc(name, seed):
    """(the mixed-mode trainable generator, the frozen f16 generator) of a config under a weight seed, from one state dict"""
    from glow_tts_amd.vocoder import HiFiGAN
    if (name, seed) not in _VOC:
        hp, sd = G._hp(C.CFGS[name]), {"generator": C.FC.sd_of(name, seed)}
        _VOC[(name, seed)] = (HiFiGAN(hp, "cuda:0", state_dict=sd, trainable=True, train_precision="mixed"), HiFiGAN(hp, "cuda:0", state_dict=sd, precision="f16"))
    return _VOC[(name, seed)]


def image_t(w):
    from glow_tts_amd.vocoder import hifigan_conv_image_t, hifigan_pack_bf16
    return hifigan_pack_bf16(hifigan_conv_image_t(w), w.shape[2]).cuda()


def up_image_t(w, u):
    from glow_tts_amd.vocoder import hifigan_pack_bf16, hifigan_up_image_t, hifigan_up_reach
    lo, hi = hifigan_up_reach(u, w.shape[2])
    return hifigan_pack_bf16(hifigan_up_image_t(w, u), hi - lo + 1).cuda()


# ---------------------------------------------------------------------------------------------------------------- 1. the data gradient
@gpu
@pytest.mark.parametrize("taps, d", C.CONV_TAPS)
@pytest.mark.parametrize("cdy, cdx", C.DGRAD_CHANNELS)
def test_conv_bwd_bf16_against_the_contract_every_epilogue(cdy, cdx, taps, d):
    from glow_tts_amd import ops
    rows = C.CONV_ROWS
    w, b, xs, dys, rs, os_ = C.conv_case(cdy, cdx, taps, d, rows)
    assert any(bool((x == 0).any()) for x in xs)                              # the slope at x == 0
    lengths, Tmax = lengths_of(xs), max(rows)
    x, dy, wt = pad(xs, 1e3), pad(dys, 1e3), image_t(w)
    s = C.SCALE
    for tag, res, scale, rscale, acc in (("plain", False, s, 1.0, False), ("residual", True, 1.0, s, False), ("accumulate", True, s, s, True)):
        ref = {e: M.conv_grads(e, xs, w, b, dys, d, H.SLOPE, scale)[0] for e in (E64, E32)}
        out = pad(os_, NAN) if acc else torch.full((len(xs), Tmax, cdx), NAN, device="cuda")
        launch_reset()
        ops.hifigan_conv_bwd_bf16(dy, wt, x, out, lengths, Tmax, 1, taps, d, H.SLOPE, residual=pad(rs, 1e3) if res else None, scale=scale, res_scale=rscale,
                                  accumulate=acc)
        assert logged() == {"hifigan_conv_bwd_bf16": 1}
        for i, T in enumerate(rows):
            want = [ref[e][i] + (rs[i].to(e.dtype) * rscale if res else 0) + (os_[i].to(e.dtype) if acc else 0) for e in (E64, E32)]
            C.check_operator(f"conv_bwd_bf16 {cdx}<-{cdy} k={taps} d={d} {tag} T={T}", out[i, :T].cpu(), *want)
        assert beyond_is_nan(out, rows)                                       # rows beyond an utterance are untouched
        if not acc:
            again = torch.full_like(out, NAN)
            ops.hifigan_conv_bwd_bf16(dy, wt, x, again, lengths, Tmax, 1, taps, d, H.SLOPE, residual=pad(rs, 1e3) if res else None, scale=scale, res_scale=rscale)
            assert torch.equal(torch.nan_to_num(again), torch.nan_to_num(out))        # run to run


@gpu
@pytest.mark.parametrize("cdy, cdx, taps, d", [(256, 256, 11, 5), (48, 32, 3, 5)])
def test_conv_bwd_bf16_rows_are_the_same_alone_in_any_batch_at_any_padding(cdy, cdx, taps, d):
    from glow_tts_amd import ops
    rows = C.RAGGED_ROWS
    w, _, xs, dys, _, _ = C.conv_case(cdy, cdx, taps, d, rows, seed=1)
    wt, single = image_t(w), []
    for x, dy in zip(xs, dys):
        out = torch.full((1, x.shape[0], cdx), NAN, device="cuda")
        ops.hifigan_conv_bwd_bf16(pad([dy], 1e3), wt, pad([x], 1e3), out, lengths_of([x]), x.shape[0], 1, taps, d, H.SLOPE)
        single.append(out[0])
    for Tmax in (200, 263):
        out = torch.full((len(rows), Tmax, cdx), NAN, device="cuda")
        ops.hifigan_conv_bwd_bf16(pad(dys, 1e3, Tmax), wt, pad(xs, -1e3, Tmax), out, lengths_of(xs), Tmax, 1, taps, d, H.SLOPE)
        assert all(torch.equal(out[i, :T], single[i]) for i, T in enumerate(rows)) and beyond_is_nan(out, rows)


# ---------------------------------------------------------------------------------------------------------------- 2. the upsample data gradient
@gpu
@pytest.mark.parametrize("u, k", C.UP_KERNELS)
@pytest.mark.parametrize("cin, cout", C.UP_CHANNELS)
def test_upsample_bwd_bf16_against_the_contract(cin, cout, u, k):
    from glow_tts_amd import ops
    rows = C.UP_ROWS
    w, b, xs, dys = C.up_case(cin, cout, u, k, rows)
    assert any(bool((x == 0).any()) for x in xs)
    ref = {e: M.upsample_grads(e, xs, w, b, dys, u)[0] for e in (E64, E32)}
    lengths, Tmax, wt = lengths_of(xs), max(rows), up_image_t(w, u)
    x, dy = pad(xs, 1e3), pad(dys, 1e3)
    out = torch.full((len(xs), Tmax, cin), NAN, device="cuda")
    launch_reset()
    ops.hifigan_upsample_bwd_bf16(dy, wt, x, out, lengths, Tmax, 1, k, u, H.SLOPE)
    assert logged() == {"hifigan_upsample_bwd_bf16": 1}
    for i, T in enumerate(rows):
        C.check_operator(f"upsample_bwd_bf16 {cin}->{cout} u={u} k={k} T={T}", out[i, :T].cpu(), ref[E64][i], ref[E32][i])
    assert beyond_is_nan(out, rows)
    again = torch.full_like(out, NAN)
    ops.hifigan_upsample_bwd_bf16(dy, wt, x, again, lengths, Tmax, 1, k, u, H.SLOPE)
    assert torch.equal(torch.nan_to_num(again), torch.nan_to_num(out))
    for Tmax2 in (Tmax, Tmax + 7):                                            # a row has the same bits alone, in the batch and at another padding
        o2 = torch.full((len(xs), Tmax2, cin), NAN, device="cuda")
        ops.hifigan_upsample_bwd_bf16(pad(dys, -1e3, Tmax2 * u), wt, pad(xs, 1e3, Tmax2), o2, lengths, Tmax2, 1, k, u, H.SLOPE)
        assert all(torch.equal(o2[i, :T], out[i, :T]) for i, T in enumerate(rows))
    i = rows.index(33)
    o1 = torch.full((1, 33, cin), NAN, device="cuda")
    ops.hifigan_upsample_bwd_bf16(pad([dys[i]], 1e3), wt, pad([xs[i]], 1e3), o1, lengths_of([xs[i]]), 33, 1, k, u, H.SLOPE)
    assert torch.equal(o1[0], out[i, :33])


# ---------------------------------------------------------------------------------------------------------------- 3. the weight gradient
def check_wgrad(tag, dw, db, ref, dys, scale=1.0):
    """dw against the contract's (emu64, emu32); db to the f32 kernel's bar against float64 of the unrounded dy"""
    C.check_operator(tag + " dw", dw.cpu(), ref[E64][1] * scale, ref[E32][1] * scale)
    b64, b32 = sum(dy.double().sum(0) for dy in dys) * scale, sum(dy.sum(0) for dy in dys) * scale
    TR.check(tag + " db", db, b64, b32)


@gpu
@pytest.mark.parametrize("taps, d", C.CONV_TAPS)
@pytest.mark.parametrize("ca, cd, cf", C.WGRAD_CHANNELS)
def test_wgrad_bf16_against_the_contract_at_every_boundary_of_the_partition(ca, cd, cf, taps, d):
    from glow_tts_amd import ops
    slope = None if cf else H.SLOPE                                           # channels-first: the mel of conv_pre, no LeakyReLU
    dw, db = torch.full((cd, ca, taps), NAN, device="cuda"), torch.full((cd,), NAN, device="cuda")
    for T in C.WGRAD_ROWS:
        w, b, xs, dys, _, _ = C.conv_case(cd, ca, taps, d, [T], seed=T)
        ref = {e: M.conv_grads(e, xs, w, b, dys, d, slope) for e in (E64, E32)}
        x, dy = pad(xs, 1e3), pad(dys, 1e3)
        work = torch.empty(ops.hifigan_wgrad_work_floats(1, T, 1, ca, cd, taps), device="cuda")
        launch_reset()
        ops.hifigan_wgrad_bf16(x.transpose(1, 2).contiguous() if cf else x, dy, lengths_of(xs), work, dw, db, T, 1, taps, dilation=d,
                               slope=1.0 if cf else H.SLOPE, scale=C.SCALE, channels_first=cf)
        assert logged() == {"hifigan_wgrad_bf16": 1, "hifigan_wgrad_sum": 1}
        check_wgrad(f"wgrad_bf16 {ca}->{cd} k={taps} d={d} T={T}", dw, db, ref, dys, C.SCALE)     # (one row is one exact product: the scale makes e32' > 0)


@gpu
@pytest.mark.parametrize("rows", [[200, 64, 1, 200, 33, 150, 7], [40, 0, 2100, 0, 1025]], ids=["short utterances, group 5", "ragged with empty utterances"])
def test_wgrad_bf16_batches_scale_and_run_to_run(rows):
    from glow_tts_amd import ops
    ca, cd, taps, d = 32, 48, 7, 3
    w, b, xs, dys, _, _ = C.conv_case(cd, ca, taps, d, rows, seed=3)
    live = [i for i, T in enumerate(rows) if T]                               # an empty utterance contributes nothing (and torch refuses to convolve it)
    ref = {e: M.conv_grads(e, [xs[i] for i in live], w, b, [dys[i] for i in live], d, H.SLOPE) for e in (E64, E32)}
    Tmax = max(rows)
    x, dy, lengths = pad(xs, 1e3), pad(dys, 1e3), lengths_of(xs)
    dw, db = torch.full((cd, ca, taps), NAN, device="cuda"), torch.full((cd,), NAN, device="cuda")
    work = torch.empty(ops.hifigan_wgrad_work_floats(len(rows), Tmax, 1, ca, cd, taps), device="cuda")
    for scale in (1.0, C.SCALE):
        ops.hifigan_wgrad_bf16(x, dy, lengths, work, dw, db, Tmax, 1, taps, dilation=d, slope=H.SLOPE, scale=scale)
        check_wgrad(f"wgrad_bf16 batch {rows} scale={scale:.2f}", dw, db, ref, dys, scale)
    first = (dw.clone(), db.clone())
    work.fill_(NAN)
    ops.hifigan_wgrad_bf16(x, dy, lengths, work, dw, db, Tmax, 1, taps, dilation=d, slope=H.SLOPE, scale=C.SCALE)
    assert torch.equal(first[0], dw) and torch.equal(first[1], db)


@gpu
@pytest.mark.parametrize("u, k", C.WGRAD_UP)
def test_wgrad_bf16_of_the_transposed_convolutions_view(u, k):
    from glow_tts_amd import ops
    cin, cout, rows = 64, 32, [1, 9, 33, 65, 140]
    w, b, xs, dys = C.up_case(cin, cout, u, k, rows)
    ref = {e: M.upsample_grads(e, xs, w, b, dys, u) for e in (E64, E32)}
    Tmax = max(rows)
    dw, db = torch.full((cin, cout, k), NAN, device="cuda"), torch.full((cout,), NAN, device="cuda")
    work = torch.empty(ops.hifigan_wgrad_work_floats(len(rows), Tmax, 1, cin, cout, k, u), device="cuda")
    launch_reset()
    ops.hifigan_wgrad_bf16(pad(xs, 1e3), pad(dys, 1e3), lengths_of(xs), work, dw, db, Tmax, 1, k, rate=u, slope=H.SLOPE)
    assert logged() == {"hifigan_wgrad_bf16": 1, "hifigan_wgrad_sum": 1}
    check_wgrad(f"wgrad_bf16 view {cin}->{cout} u={u} k={k}", dw, db, ref, dys)


@gpu
def test_wgrad_bf16_of_one_output_column_runs_the_f32_launches():
    from glow_tts_amd import ops
    g = torch.Generator().manual_seed(5)
    C_, T = 32, 70
    x, dpre = torch.randn(1, T, C_, generator=g).cuda(), torch.randn(1, T, generator=g).cuda()
    lengths = torch.tensor([T], dtype=torch.int32, device="cuda")
    work = torch.empty(ops.hifigan_wgrad_work_floats(1, T, 1, C_, 1, 7), device="cuda")
    got, want = [(torch.full((1, C_, 7), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")) for _ in range(2)]
    launch_reset()
    ops.hifigan_wgrad_bf16(x, dpre, lengths, work, *got, T, 1, 7, slope=H.LAST_SLOPE)
    assert logged() == {"hifigan_wgrad": 1, "hifigan_wgrad_sum": 1}
    ops.hifigan_wgrad(x, dpre, lengths, work, *want, T, 1, 7, slope=H.LAST_SLOPE)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---------------------------------------------------------------------------------------------------------------- 4. hifigan_pack_images
@gpu
@pytest.mark.parametrize("name", ["narrow", "odd", "default"])
def test_pack_images_builds_every_image_in_one_launch(name):
    from glow_tts_amd.vocoder import (hifigan_conv_image, hifigan_conv_image_t, hifigan_pack_bf16, hifigan_pack_f16, hifigan_up_image, hifigan_up_image_t,
                                      hifigan_up_reach)
    v, _ = mvoc(name, 1234)
    same = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16), b.view(torch.int16))

    def check():
        w = {k: p.detach() for k, p in v.params.items()}
        launch_reset()
        v._build_images(w)
        assert logged() == {"hifigan_pack_images": 1}
        conv = lambda q: hifigan_pack_f16(hifigan_conv_image(w[q + ".weight"]), w[q + ".weight"].shape[2])
        conv_t = lambda q: hifigan_pack_bf16(hifigan_conv_image_t(w[q + ".weight"]), w[q + ".weight"].shape[2])
        assert same(v.pre[0], conv("conv_pre")) and v.pre[1].data_ptr() == w["conv_pre.bias"].data_ptr()
        for i, (u, k) in enumerate(zip(v.geo["rates"], v.geo["kernels"])):
            wu = w[f"ups.{i}.weight"]
            lo, hi = hifigan_up_reach(u, k)
            assert same(v.ups[i][0], hifigan_pack_f16(hifigan_up_image(wu), k)), i
            assert same(v.ups_t[i], hifigan_pack_bf16(hifigan_up_image_t(wu, u), hi - lo + 1)), i
        for n, steps in enumerate(v.blocks):
            for m, (_, c1, c2) in enumerate(steps):
                for which, pair, t in (("convs1", c1, v.blocks_t[n][m][0]), ("convs2", c2, v.blocks_t[n][m][1])):
                    if pair is not None:
                        q = f"resblocks.{n}.{which}.{m}"
                        assert same(pair[0], conv(q)) and same(t, conv_t(q)), q
        assert torch.equal(v.post[0], w["conv_post.weight"].permute(2, 1, 0).reshape(-1))

    check()
    keys = ["conv_pre.weight", "ups.0.weight", "resblocks.1.convs1.0.weight", "conv_post.weight"]
    kept = {k: v.params[k].detach().clone() for k in keys}
    with torch.no_grad():
        for k in keys:                                                        # an optimizer step writes the leaves in place
            v.params[k].mul_(1.5).add_(0.01)
    try:
        check()                                                               # the next pack reflects it
    finally:
        with torch.no_grad():
            for k in keys:
                v.params[k].copy_(kept[k])
        v._build_images({k: p.detach() for k, p in v.params.items()})


# ---------------------------------------------------------------------------------------------------------------- 5. the whole generator
@gpu
@pytest.mark.parametrize("name, seed, lengths", C.GENERATOR_CASES)
def test_generator_forward_is_the_f16_inference_forward_and_gradients_meet_the_bars(name, seed, lengths):
    from glow_tts_amd.vocoder import hifigan_train_launches
    cfg, (v, frozen) = C.CFGS[name], mvoc(name, seed)
    assert v.train_precision == "mixed" and v.precision == "f32" and v.geo["precision"] == "f32"
    hop, Lmax = H.hop(cfg), max(lengths)
    ref = C.reference(name, seed, lengths)
    mel = torch.full((len(lengths), cfg["A"], Lmax), 1e3)
    for b, m in enumerate(ref["mels"]):
        mel[b, :, :m.shape[1]] = m
    mel, dwav = mel.cuda(), pad(ref["fs"], 1e3, Lmax * hop)

    def run():
        for p in v.params.values():
            p.grad = None
        wav, n = v.generate(mel, lengths)
        wav.backward(dwav)
        return wav.detach(), n, {k: p.grad.clone() for k, p in v.params.items()}

    launch_reset()
    wav, n, grads = run()
    assert logged() == hifigan_train_launches(v.geo, "mixed")
    assert n.tolist() == [L * hop for L in lengths]
    assert torch.equal(wav, frozen(mel, lengths)[0])                          # the same launches, the same bits
    assert list(grads) == list(ref["ref64"]) == list(v.params)
    worst = [0.0, 0.0]
    for k in C.pairs((name, seed, lengths)):
        assert grads[k].shape == ref["ref64"][k].shape, k
        a, b = C.check_generator(f"{name} {seed} {lengths} d {k}", grads[k].cpu(), ref, k, name != "default")
        worst = [max(worst[0], a / C.BAR_A), max(worst[1], b / C.BAR_B if name != "default" else 0.0)]
    print(f"{name} {seed} {lengths}: worst ratio to bar (a) {worst[0]:.3f}, to bar (b) {worst[1]:.3f}")
    _, _, again = run()
    assert all(torch.equal(again[k], grads[k]) for k in grads)                # bit-identical from run to run


# ---------------------------------------------------------------------------------------------------------------- 6. the f32 mode is untouched
@gpu
def test_the_f32_training_mode_logs_exactly_its_own_launches():
    from glow_tts_amd.vocoder import HiFiGAN, hifigan_train_launches
    v = HiFiGAN(G._hp(H.NARROW), "cuda:0", state_dict={"generator": C.FC.sd_of("narrow", 1234)}, trainable=True)
    assert v.train_precision == "f32"
    mel = H.uniform_mel(H.NARROW["A"], 3, 1)[None].cuda()
    launch_reset()
    wav, _ = v.generate(mel, [3])
    wav.backward(torch.ones_like(wav))
    counts = logged()
    assert counts == hifigan_train_launches(v.geo) == hifigan_train_launches(v.geo, "f32")
    assert not [k for k in counts if "_f16" in k or "_bf16" in k or "pack" in k]


@gpu
def test_unsupported_sizes_return_before_any_launch():
    from glow_tts_amd import _lib, ops
    z = torch.zeros(1, 8, 24, device="cuda")
    launch_reset()
    with pytest.raises(_lib.GlowTTSHipError):                                  # 24 input channels: the data gradient writes tiles of 16
        ops.hifigan_conv_bwd_bf16(torch.zeros(1, 8, 16, device="cuda"), torch.zeros(3, 4, 24, 8, dtype=torch.bfloat16, device="cuda"), z, torch.zeros_like(z),
                                  torch.tensor([8], dtype=torch.int32, device="cuda"), 8, 1, 3, 1, 0.1)
    with pytest.raises(_lib.GlowTTSHipError):                                  # an f32 image is refused by the wrapper
        ops.hifigan_conv_bwd_bf16(torch.zeros(1, 8, 16, device="cuda"), torch.zeros(3 * 16, 16, device="cuda"), torch.zeros(1, 8, 16, device="cuda"),
                                  torch.zeros(1, 8, 16, device="cuda"), torch.tensor([8], dtype=torch.int32, device="cuda"), 8, 1, 3, 1, 0.1)
    assert not sum(launch_counts().values())
    api = _lib.api()
    assert api.glowtts_hifigan_train_supported_mixed(512, 256, 16, 1, 8) == 1 and api.glowtts_hifigan_train_supported_mixed(24, 16, 4, 1, 2) == 0
    assert api.glowtts_hifigan_train_supported_mixed(32, 1, 7, 1, 0) == 1     # conv_post: the f32 launches serve it
