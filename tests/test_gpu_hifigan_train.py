"""GPU suite of the HiFi-GAN generator's backward (glow_tts_amd/vocoder.py: HiFiGAN(trainable=True) on csrc/hifigan_train_ops.hip) against float64 autograd of
the restatement (tests/hifigan_train_ref.py).

THE BAR is the project's own (tests/test_gpu_hifigan.py): max |hip - ref64| / max |ref64| <= 4 e32 + 1e-6 with e32 from the float32 run of the restatement on
the CPU, never from the code under test; guards 0 < e32 < 1e-3 and max |ref64| > 1e-3; separately for the waveform and for every gradient tensor; every figure
is printed before it is asserted (pytest -s).  On the CPU the restatement alone stays inside the guards for all six whole-generator cases: the worst e32 over
the gradients is 3.4e-7, 2.2e-7, 7.9e-7, 3.5e-6, 1.9e-6 and 7.6e-7, the smallest max |g64| 2.5e-3."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hifigan_ref as H  # noqa: E402
import hifigan_train_ref as R  # noqa: E402
import test_gpu_hifigan as G  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402

gpu = pytest.mark.gpu
NAN = float("nan")
_TRAIN, _REF = {}, {}


def tvoc(name):
    from glow_tts_amd.vocoder import HiFiGAN
    if name not in _TRAIN:
        _TRAIN[name] = HiFiGAN(G._hp(G.CFGS[name]), "cuda:0", state_dict={"generator": G.sd_of(name)}, trainable=True)
    return _TRAIN[name]


def reference(name, lengths):
    """(mels, functionals, (wavs64, grads64), (wavs32, grads32)): computed once, shared, never changed"""
    key = (name, tuple(lengths))
    if key not in _REF:
        cfg = G.CFGS[name]
        g = torch.Generator().manual_seed(7)
        mels = [H.uniform_mel(cfg["A"], L, 20 + L) for L in lengths]
        fs = [torch.randn(L * H.hop(cfg), generator=g) for L in lengths]
        _REF[key] = (mels, fs, R.generator_grads(G.sd_of(name), cfg, mels, fs), R.generator_grads(G.sd_of(name), cfg, mels, fs, torch.float32))
    return _REF[key]


def pad(rows, fill, Tmax=None):
    """[T_b, ...] -> [B, Tmax, ...] on the device holding `fill` beyond each utterance"""
    Tmax = Tmax or max(r.shape[0] for r in rows)
    out = torch.full((len(rows), Tmax) + tuple(rows[0].shape[1:]), fill, dtype=torch.float32)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out.cuda()


def lengths_of(rows):
    return torch.tensor([r.shape[0] for r in rows], dtype=torch.int32, device="cuda")


def beyond_is_nan(out, lengths, mult=1):
    return all(bool(torch.isnan(out[b, T * mult:]).all()) for b, T in enumerate(lengths))


# ---------------------------------------------------------------------------------------------------------------- 1. whole generator
CASES = [("narrow", [5, 2, 7]), ("narrow", [1]), ("odd", [5, 2, 7]), ("default", [3]), ("default", [5, 2]), ("narrow", [300, 300])]
# the last: 1200 rows at the last stage, more than one 1024-row chunk of the weight gradient's partition


@gpu
@pytest.mark.parametrize("name, lengths", CASES)
def test_generator_gradients_against_float64_autograd(name, lengths):
    from glow_tts_amd.vocoder import hifigan_launches, hifigan_train_launches
    cfg, v = G.CFGS[name], tvoc(name)
    hop, Lmax = H.hop(cfg), max(lengths)
    mels, fs, (w64, g64), (w32, g32) = reference(name, lengths)
    mel = torch.full((len(lengths), cfg["A"], Lmax), 1e3)                      # padded input rows hold 1e3 and reach nothing
    for b, m in enumerate(mels):
        mel[b, :, :m.shape[1]] = m
    mel, dwav = mel.cuda(), pad(fs, 1e3, Lmax * hop)

    def run():
        for p in v.params.values():
            p.grad = None
        wav, n = v.generate(mel, lengths)
        wav.backward(dwav)
        return wav.detach(), n, {k: p.grad.clone() for k, p in v.params.items()}

    launch_reset()
    wav, n, grads = run()
    counts = {k: c for k, c in launch_counts().items() if c}
    assert counts == hifigan_train_launches(v.geo), counts
    assert counts["hifigan_wgrad"] == hifigan_launches(v.geo) and not [k for k in counts if not k.startswith("hifigan")]
    assert n.tolist() == [L * hop for L in lengths]
    plain, _ = G.voc(name)(mel, lengths)
    assert torch.equal(wav, plain)                                            # the training forward is the inference launches
    for b, L in enumerate(lengths):
        R.check(f"{name} {lengths} wav {b}", wav[b, :L * hop], w64[b], w32[b])
    assert list(grads) == list(g64) == list(v.params)
    for k in g64:
        assert grads[k].shape == g64[k].shape, k
        R.check(f"{name} {lengths} d {k}", grads[k], g64[k], g32[k])
    _, _, again = run()
    assert all(torch.equal(again[k], grads[k]) for k in grads)                # bit-identical from run to run


@gpu
def test_a_frozen_generator_is_unchanged():
    v = G.voc("default")
    assert not hasattr(v, "params") and v.trainable is False
    mel = H.uniform_mel(80, 3, 1)[None].cuda()
    v(mel, [3])
    launch_reset()
    v(mel, [3])
    assert sum(launch_counts().values()) == 78
    from glow_tts_amd import _lib
    with pytest.raises(_lib.GlowTTSHipError, match="trainable=True"):
        v.generate(mel, [3])


def test_trainable_refuses_bf16_before_the_device():
    from glow_tts_amd.vocoder import HiFiGAN
    with pytest.raises(ValueError, match="f32"):
        HiFiGAN(G._hp(H.NARROW), "cuda:0", trainable=True, precision="bf16")


# ---------------------------------------------------------------------------------------------------------------- 2. hifigan_conv_bwd + weight gradient
CONV_LENGTHS = [1, 5, 63, 64, 65, 200]


@gpu
@pytest.mark.parametrize("taps, d", [(3, 1), (3, 5), (7, 3), (11, 5)])
@pytest.mark.parametrize("cin, cout", [(16, 16), (32, 16), (256, 256), (80, 512)])
def test_conv_bwd_and_weight_gradient_against_float64_every_epilogue(cin, cout, taps, d):
    from glow_tts_amd import ops
    from glow_tts_amd.vocoder import hifigan_conv_image_t
    g = torch.Generator().manual_seed(1000 * cin + 10 * taps + d)
    w = (torch.rand(cout, cin, taps, generator=g) * 2 - 1) / (cin * taps) ** 0.5
    b = torch.rand(cout, generator=g) * 2 - 1
    xs = [torch.randn(T, cin, generator=g) for T in CONV_LENGTHS]
    dys = [torch.randn(T, cout, generator=g) for T in CONV_LENGTHS]
    rs = [torch.randn(T, cin, generator=g) for T in CONV_LENGTHS]              # the skip branch's gradient
    os_ = [torch.randn(T, cin, generator=g) for T in CONV_LENGTHS]             # what dU holds so far
    ref = {dt: R.conv_grads(xs, w, b, dys, d, H.SLOPE, dt) for dt in (torch.float64, torch.float32)}
    lengths, Tmax = lengths_of(xs), max(CONV_LENGTHS)
    x, dy, wt = pad(xs, 1e3), pad(dys, 1e3), hifigan_conv_image_t(w).cuda()
    s = 1.0 / 3
    for tag, res, scale, rscale, acc in (("mask", None, 1.0, 1.0, False), ("mask+res", "r", s, s, False), ("mask+res+acc", "r", 1.0, s, True),
                                         ("res is out", "out", 1.0, 1.0, False)):
        out = pad(os_ if acc else rs, NAN) if (acc or res == "out") else torch.full((len(xs), Tmax, cin), NAN, device="cuda")
        r = None if res is None else (out if res == "out" else pad(rs, 1e3))
        ops.hifigan_conv_bwd(dy, wt, x, out, lengths, Tmax, 1, taps, d, H.SLOPE, residual=r, scale=scale, res_scale=rscale, accumulate=acc)
        for i, T in enumerate(CONV_LENGTHS):
            want = [ref[dt][0][i] * scale + (rs[i].to(dt) * rscale if res else 0) + (os_[i].to(dt) if acc else 0) for dt in (torch.float64, torch.float32)]
            R.check(f"conv_bwd {cin}->{cout} k={taps} d={d} {tag} T={T}", out[i, :T], *want)
        assert beyond_is_nan(out, CONV_LENGTHS)
    dw, db = torch.full((cout, cin, taps), NAN, device="cuda"), torch.full((cout,), NAN, device="cuda")
    work = torch.empty(ops.hifigan_wgrad_work_floats(len(xs), Tmax, 1, cin, cout, taps), device="cuda")
    for scale in (1.0, s):
        ops.hifigan_wgrad(x, dy, lengths, work, dw, db, Tmax, 1, taps, dilation=d, slope=H.SLOPE, scale=scale)
        R.check(f"conv wgrad {cin}->{cout} k={taps} d={d} scale={scale:.2f} dw", dw, ref[torch.float64][1] * scale, ref[torch.float32][1] * scale)
        R.check(f"conv wgrad {cin}->{cout} k={taps} d={d} scale={scale:.2f} db", db, ref[torch.float64][2] * scale, ref[torch.float32][2] * scale)
    first = dw.clone()
    ops.hifigan_wgrad(x, dy, lengths, work, dw, db, Tmax, 1, taps, dilation=d, slope=H.SLOPE, scale=s)
    assert torch.equal(first, dw)


@gpu
def test_conv_pre_weight_gradient_reads_the_mel_channels_first():
    from glow_tts_amd import ops
    g = torch.Generator().manual_seed(3)
    A, C, lens = 12, 64, [9, 70, 2]
    w, b = (torch.rand(C, A, 7, generator=g) * 2 - 1) / (A * 7) ** 0.5, torch.rand(C, generator=g)
    xs, dys = [torch.randn(T, A, generator=g) for T in lens], [torch.randn(T, C, generator=g) for T in lens]
    ref = {dt: R.conv_grads(xs, w, b, dys, 1, None, dt) for dt in (torch.float64, torch.float32)}
    mel = pad(xs, 1e3).transpose(1, 2).contiguous()                           # [B, A, Tmax]
    dw, db = torch.full((C, A, 7), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
    work = torch.empty(ops.hifigan_wgrad_work_floats(3, 70, 1, A, C, 7), device="cuda")
    ops.hifigan_wgrad(mel, pad(dys, 1e3), lengths_of(xs), work, dw, db, 70, 1, 7, channels_first=True)
    R.check("conv_pre dw", dw, ref[torch.float64][1], ref[torch.float32][1])
    R.check("conv_pre db", db, ref[torch.float64][2], ref[torch.float32][2])


# ---------------------------------------------------------------------------------------------------------------- 3. hifigan_upsample_bwd + weight gradient
UP_LENGTHS = [1, 2, 9, 33, 65]


@gpu
@pytest.mark.parametrize("u, k", [(2, 4), (8, 16), (3, 7), (5, 11)])
@pytest.mark.parametrize("cin", [32, 512])
def test_upsample_bwd_and_weight_gradient_against_float64(u, k, cin):
    from glow_tts_amd import ops
    from glow_tts_amd.vocoder import hifigan_up_image_t
    cout = cin // 2
    g = torch.Generator().manual_seed(100 * u + k + cin)
    w = (torch.rand(cin, cout, k, generator=g) * 2 - 1) / (cout * k) ** 0.5
    b = torch.rand(cout, generator=g) * 2 - 1
    xs = [torch.randn(T, cin, generator=g) for T in UP_LENGTHS]
    dys = [torch.randn(u * T, cout, generator=g) for T in UP_LENGTHS]
    ref = {dt: R.upsample_grads(xs, w, b, dys, u, dt) for dt in (torch.float64, torch.float32)}
    lengths, Tmax = lengths_of(xs), max(UP_LENGTHS)
    x, dy = pad(xs, 1e3), pad(dys, 1e3)
    out = torch.full((len(xs), Tmax, cin), NAN, device="cuda")
    ops.hifigan_upsample_bwd(dy, hifigan_up_image_t(w, u).cuda(), x, out, lengths, Tmax, 1, k, u, H.SLOPE)
    for i, T in enumerate(UP_LENGTHS):
        R.check(f"upsample_bwd {cin}->{cout} u={u} k={k} T={T}", out[i, :T], ref[torch.float64][0][i], ref[torch.float32][0][i])
    assert beyond_is_nan(out, UP_LENGTHS)
    dw, db = torch.full((cin, cout, k), NAN, device="cuda"), torch.full((cout,), NAN, device="cuda")
    work = torch.empty(ops.hifigan_wgrad_work_floats(len(xs), Tmax, 1, cin, cout, k, u), device="cuda")
    ops.hifigan_wgrad(x, dy, lengths, work, dw, db, Tmax, 1, k, rate=u, slope=H.SLOPE)
    R.check(f"upsample wgrad {cin}->{cout} u={u} k={k} dw", dw, ref[torch.float64][1], ref[torch.float32][1])
    R.check(f"upsample wgrad {cin}->{cout} u={u} k={k} db", db, ref[torch.float64][2], ref[torch.float32][2])


# ---------------------------------------------------------------------------------------------------------------- 4. hifigan_post_bwd
@gpu
def test_post_bwd_and_its_weight_gradient_against_float64():
    from glow_tts_amd import ops
    g = torch.Generator().manual_seed(11)
    C, lens = 32, [1, 5, 300, 1100]                                           # 1100: a second chunk of the weight gradient's partition
    w, b = (torch.rand(1, C, 7, generator=g) * 2 - 1) / (C * 7) ** 0.5, torch.rand(1, generator=g) - 0.5
    xs, fs = [torch.randn(T, C, generator=g) for T in lens], [torch.randn(T, generator=g) for T in lens]
    ref = {}
    for dt in (torch.float64, torch.float32):
        wl, bl = w.to(dt).requires_grad_(True), b.to(dt).requires_grad_(True)
        xl = [x.to(dt).requires_grad_(True) for x in xs]
        loss = sum((f.to(dt) * torch.tanh(H.conv(x.T, wl, bl, 1, H.LAST_SLOPE))[0]).sum() for x, f in zip(xl, fs))
        gr = torch.autograd.grad(loss, xl + [wl, bl])
        ref[dt] = (gr[:len(xs)], gr[-2], gr[-1])
    lengths, Tmax = lengths_of(xs), max(lens)
    x, dwav, wimg, bias = pad(xs, 1e3), pad(fs, 1e3), w.permute(2, 1, 0).reshape(-1).contiguous().cuda(), b.cuda()
    wav = torch.empty(len(xs), Tmax, device="cuda")
    ops.hifigan_post(x, wimg, bias, wav, lengths, Tmax, 1, 7, H.LAST_SLOPE)
    dpre, dx = torch.full((len(xs), Tmax), NAN, device="cuda"), torch.full((len(xs), Tmax, C), NAN, device="cuda")
    ops.hifigan_post_bwd(dwav, wav, x, wimg, dpre, dx, lengths, Tmax, 1, 7, H.LAST_SLOPE)
    for i, T in enumerate(lens):
        R.check(f"post_bwd T={T}", dx[i, :T], ref[torch.float64][0][i], ref[torch.float32][0][i])
    assert beyond_is_nan(dx, lens) and beyond_is_nan(dpre, lens)
    dw, db = torch.full((1, C, 7), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    work = torch.empty(ops.hifigan_wgrad_work_floats(len(xs), Tmax, 1, C, 1, 7), device="cuda")
    ops.hifigan_wgrad(x, dpre, lengths, work, dw, db, Tmax, 1, 7, slope=H.LAST_SLOPE)
    R.check("conv_post dw", dw, ref[torch.float64][1], ref[torch.float32][1])
    R.check("conv_post db", db, ref[torch.float64][2], ref[torch.float32][2])


@gpu
def test_unsupported_sizes_return_before_any_launch():
    from glow_tts_amd import _lib, ops
    z = torch.zeros(1, 8, 24, device="cuda")
    launch_reset()
    with pytest.raises(_lib.GlowTTSHipError):                                  # 24 input channels: the data gradient writes tiles of 16
        ops.hifigan_conv_bwd(torch.zeros(1, 8, 16, device="cuda"), torch.zeros(3 * 16, 24, device="cuda"), z, torch.zeros_like(z),
                             torch.tensor([8], dtype=torch.int32, device="cuda"), 8, 1, 3, 1, 0.1)
    assert not sum(launch_counts().values())
    assert _lib.api().glowtts_hifigan_train_supported(512, 256, 16, 1, 8) == 1 and _lib.api().glowtts_hifigan_train_supported(24, 16, 4, 1, 2) == 0
