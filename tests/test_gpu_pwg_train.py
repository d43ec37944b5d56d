"""GPU: the training path of the Parallel WaveGAN generator (csrc/pwg_train_ops.hip through `vocoder.ParallelWaveGAN(..., trainable=True)`) against
tests/pwg_train_ref.py (tests/pwg_ref.py's generator under autograd).  The bar is the project's own, unchanged (`pwg_train_ref.check`):
max |hip - ref64| / max |ref64| <= 4 e32 + 1e-6 with e32 from the float32 run of the reference on the CPU, separately for the wav and every parameter gradient
(and, for a layer alone, dx and dc).  Weights: torch's default Conv initialisation under a fixed seed, the conv weights times 1 or 3 (at scale 1 the
30-layer default sits on a ReLU edge of the head in float32 and leaves the guards; scale 3 does not)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pwg_ref as P  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402
from test_gpu_pwg import _hp, pad_mels, pad_rows  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
ODD = dict(P.DEFAULT, layers=10, stacks=1, scales=[3, 5])                    # default widths, hop 15, dilations 1 .. 512
CASES = {
    # name: (config, frames per utterance, weight scale)
    "narrow_ragged": (P.NARROW, [5, 2, 7], 1.0),
    "narrow_short": (P.NARROW, [1, 2], 1.0),                                 # fewer frames than the context window reaches
    "default_l3": (P.DEFAULT, [3], 3.0),                                     # 30 layers
    "default_short": (dict(P.DEFAULT, layers=3, stacks=1), [1, 2, 5], 1.0),  # scales [4, 4, 4, 4] at fewer frames than the context window reaches
    "splits": (dict(P.DEFAULT, layers=6, stacks=2), [7, 7, 7], 1.0),         # 1792 rows per utterance: two splits each of the weight-gradient partition
}
_cache = {}


def state_dict(cfg, scale):
    return {k: v * (scale if k.endswith("weight") and "up_layers" not in k else 1.0) for k, v in P.random_state_dict(cfg, 1234).items()}


def case_inputs(case):
    cfg, Ls, scale = CASES[case]
    hop, g = P.hop(cfg), torch.Generator().manual_seed(7)
    mels = [P.uniform_mel(cfg["A"], L, 20 + L) for L in Ls]
    zs = [torch.randn(L * hop, generator=g) for L in Ls]
    fs = [torch.randn(L * hop, generator=g) for L in Ls]
    return cfg, state_dict(cfg, scale), mels, zs, fs


def case_reference(case):
    if case not in _cache:
        cfg, sd, mels, zs, fs = case_inputs(case)
        _cache[case] = TR.generator_grads(sd, cfg, mels, zs, fs), TR.generator_grads(sd, cfg, mels, zs, fs, torch.float32)
    return _cache[case]


def build(case, trainable=True):
    from glow_tts_amd.vocoder import ParallelWaveGAN
    cfg, sd, mels, zs, fs = case_inputs(case)
    v = ParallelWaveGAN(_hp(cfg), "cuda:0", state_dict={"generator": sd}, trainable=trainable)
    m, lengths = pad_mels(mels)
    return v, m, lengths, pad_rows(zs, fill=1e3), pad_rows(fs, fill=1e3)


def step(v, m, lengths, z, f):
    """generate + backward of <f, wav> through autograd -> (wav, {name: .grad})"""
    for p in v.params.values():
        p.grad = None
    wav, _ = v.generate(m, lengths, noises=z)
    (wav * f).sum().backward()
    torch.cuda.synchronize()
    return wav.detach(), {k: p.grad for k, p in v.params.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_whole_generator_matches_the_float64_reference(case):
    cfg, Ls, _ = CASES[case]
    hop = P.hop(cfg)
    (w64, g64), (w32, g32) = case_reference(case)
    v, m, lengths, z, f = build(case)
    wav, grads = step(v, m, lengths, z, f)
    assert set(grads) == set(g64)
    failed = []
    for b, L in enumerate(Ls):
        assert not wav[b, L * hop:].any()
        try:
            TR.check(f"{case} wav {b}", wav[b, :L * hop], w64[b], w32[b])
        except AssertionError as err:
            failed.append(str(err))
    for name in g64:
        assert grads[name].shape == g64[name].shape, name
        if not g64[name].any():                                              # nothing reads the last layer's x': exactly zero, on both sides
            assert name.startswith(f"conv_layers.{cfg['layers'] - 1}.conv1x1_out") and not grads[name].any()
            continue
        try:
            TR.check(f"{case} {name}", grads[name], g64[name], g32[name])
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, failed


LAYER_CASES = [(n, ls, i) for n, ls in (("default", [3, 1, 2]), ("odd", [7, 2, 5])) for i in (0, 1, 6, 9)] + [("narrow", [7, 2, 5], 1)]


@pytest.mark.parametrize("name, lengths, layer", LAYER_CASES)       # dilations 1, 2, 64, 512 at T = 768 / 256 / 512 and T = 105 / 30 / 75; the narrow widths once
def test_one_layer_backward_alone(name, lengths, layer):
    """dx, dc and the layer's six parameter gradients from given dx' and d skips, on a ragged batch whose rows beyond every utterance hold 1e3 in every input
    and NaN in every output: they reach no gradient and nothing beyond an utterance's rows is written."""
    from glow_tts_amd import _lib
    from glow_tts_amd.vocoder import ParallelWaveGAN, pwg_expected_shapes
    cfg = {"default": P.DEFAULT, "odd": ODD, "narrow": P.NARROW}[name]
    sd = state_dict(cfg, 1.0)
    v = ParallelWaveGAN(_hp(cfg), "cuda:0", state_dict={"generator": sd}, trainable=True)
    hop, R, S, A, G, d = P.hop(cfg), cfg["R"], cfg["S"], cfg["A"], cfg["G"], P.dilation(cfg, layer)
    g = torch.Generator().manual_seed(500 + layer)
    rows = lambda C: [torch.randn(L * hop, C, generator=g) for L in lengths]
    xs, cs, dxps, dsks = rows(R), rows(A), rows(R), rows(S)
    Lmax = max(lengths) + 1
    Tmax = Lmax * hop
    x, c, dxp, dsk = (pad_rows(t, Tmax, 1e3) for t in (xs, cs, dxps, dsks))
    nan = lambda *shape: torch.full(shape, NAN, device="cuda")
    B = len(lengths)
    gate, dpre, dx, dc = nan(B, Tmax, R), nan(B, Tmax, G), nan(B, Tmax, R), nan(B, Tmax, A)
    q = f"conv_layers.{layer}."
    names = ["conv.weight", "conv.bias", "conv1x1_aux.weight", "conv1x1_out.weight", "conv1x1_out.bias", "conv1x1_skip.weight", "conv1x1_skip.bias"]
    grads = {k: nan(*pwg_expected_shapes(v.geo)[q + k]) for k in names}
    lib, Pt, st = _lib.lib(), _lib.ptr, _lib.stream()
    n = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    work = torch.empty(lib.glowtts_pwg_train_work_floats(B, Lmax, hop, R, S, A), device="cuda")
    (w1, b1, _, _), (w2t, w1t, wauxt) = v.layer_weights[layer], v.layer_weights_t[layer]
    assert lib.glowtts_pwg_train_layer_bwd(Pt(x), Pt(c), Pt(w1), Pt(b1), Pt(w2t), Pt(w1t), Pt(wauxt), Pt(dxp), Pt(dsk), Pt(gate), Pt(dpre), Pt(dx), Pt(dc), Pt(n), B,
                                           Lmax, hop, R, S, A, d, 1, st) == 0
    assert lib.glowtts_pwg_train_layer_wgrad(Pt(x), Pt(c), Pt(gate), Pt(dpre), Pt(dxp), Pt(dsk), Pt(n), Pt(work), *[Pt(grads[k]) for k in names], B, Lmax, hop, R, S,
                                             A, d, st) == 0
    torch.cuda.synchronize()
    for b, L in enumerate(lengths):
        for t in (gate, dpre, dx, dc):
            assert torch.isnan(t[b, L * hop:]).all() and torch.isfinite(t[b, :L * hop]).all()
    cat = lambda ts: torch.cat([t.T for t in ts], dim=1)
    # the reference runs the utterances one by one and adds the parameter gradients
    refs = []
    for dt in (torch.float64, torch.float32):
        per = [TR.layer_grads(sd, cfg, layer, xs[b].T, cs[b].T, dxps[b].T, dsks[b].T, dt) for b in range(B)]
        r = {k: sum(p[k] for p in per) for k in names}
        r["dx"], r["dc"] = torch.cat([p["dx"] for p in per], dim=1), torch.cat([p["dc"] for p in per], dim=1)
        refs.append(r)
    got = dict(grads, dx=cat([dx[b, :L * hop] for b, L in enumerate(lengths)]), dc=cat([dc[b, :L * hop] for b, L in enumerate(lengths)]))
    failed = []
    for k in refs[0]:
        try:
            TR.check(f"layer {name} d={d} {k}", got[k], refs[0][k], refs[1][k])
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, failed


@pytest.mark.parametrize("case", ["narrow_ragged", "default_l3"])
def test_training_forward_is_the_inference_forward_bit_for_bit(case):
    v, m, lengths, z, f = build(case)
    wav, n = v.generate(m, lengths, noises=z)
    ref, n_ref = v(m, lengths, noises=z)
    assert torch.equal(wav.detach(), ref) and torch.equal(n, n_ref)
    seeds = torch.tensor([[11 + b, 12345] for b in range(m.shape[0])])
    assert torch.equal(v.generate(m, lengths, seeds=seeds)[0].detach(), v(m, lengths, seeds=seeds)[0])


def test_two_runs_give_identical_gradients_and_seeded_noise_reaches_first_conv():
    for case in ("narrow_ragged", "splits"):
        v, m, lengths, z, f = build(case)
        w1, g1 = step(v, m, lengths, z, f)
        w2, g2 = step(v, m, lengths, z, f)
        assert torch.equal(w1, w2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    # the same noise drawn in the kernel from seed words: first_conv's gradient equals the one from the materialised z
    from glow_tts_amd import ops
    seeds = torch.tensor([[3, 4], [5, 6], [7, 8]])
    for p in v.params.values():
        p.grad = None
    wav, _ = v.generate(m, lengths, seeds=seeds)
    (wav * f).sum().backward()
    seeded = {k: p.grad.clone() for k, p in v.params.items()}
    ident_w, ident_b = torch.ones(v.geo["R"], device="cuda"), torch.zeros(v.geo["R"], device="cuda")
    x0 = torch.zeros(m.shape[0], m.shape[2] * v.hop, v.geo["R"], device="cuda")
    from glow_tts_amd.alignment import seed_words
    ops.pwg_first(None, seed_words(seeds, 3, "cuda:0"), v._lengths(lengths, 3, m.shape[2]), ident_w, ident_b, x0, m.shape[2], v.hop)
    _, mat = step(v, m, lengths, x0[:, :, 0].contiguous(), f)
    assert all(torch.equal(seeded[k], mat[k]) for k in mat)


def test_an_utterance_reaches_dx0_alone_as_inside_a_ragged_batch():
    from glow_tts_amd import vocoder
    v, m, lengths, z, f = build("narrow_ragged")
    hop = v.hop

    def dx0(idx, Lmax):
        mm = torch.full((len(idx), m.shape[1], Lmax), 1e3, device="cuda")
        zz, ff = torch.full((len(idx), Lmax * hop), 1e3, device="cuda"), torch.full((len(idx), Lmax * hop), 1e3, device="cuda")
        ls = []
        for j, b in enumerate(idx):
            L = int(lengths[b])
            mm[j, :, :L], zz[j, :L * hop], ff[j, :L * hop] = m[b, :, :L], z[b, :L * hop], f[b, :L * hop]
            ls.append(L)
        n = v._lengths(ls, len(idx), Lmax)
        v._build_images({k: p.detach() for k, p in v.params.items()})
        fwd = vocoder.pwg_train_forward(v, mm, n, None, zz)
        return vocoder.pwg_train_backward(v, mm, n, None, zz, fwd, ff)["dx0"], ls

    batch, ls = dx0([0, 1, 2], 9)
    for b, L in enumerate(ls):
        alone, _ = dx0([b], L)
        assert torch.equal(alone[0, :L * hop], batch[b, :L * hop]), b


def test_launch_log_of_a_step():
    v, m, lengths, z, f = build("narrow_ragged")
    step(v, m, lengths, z, f)
    launch_reset()
    step(v, m, lengths, z, f)
    counts = {k: n for k, n in launch_counts().items() if n}
    layers, scales = v.geo["layers"], len(v.geo["scales"])
    want = {"pwg_cond_in": scales + 1, "pwg_upsample": 1 + scales * (scales + 1) // 2, "pwg_first": 1, "pwg_layer": layers, "pwg_head": 1,
            "pwg_head_bwd": 1, "pwg_layer_bwd_gate": layers, "pwg_layer_bwd_data": layers, "pwg_wgrad": layers + 1, "pwg_first_bwd": 1,
            "pwg_wgrad_sum": layers + 2, "pwg_upsample_bwd": scales, "pwg_upsample_bwd_fir": scales, "pwg_upsample_bwd_sum": scales, "pwg_cond_in_bwd": 1}
    assert counts == want, counts


def test_no_torch_conv_matrix_or_fft_op_runs_in_a_step():
    from torch.utils._python_dispatch import TorchDispatchMode
    v, m, lengths, z, f = build("narrow_ragged")
    step(v, m, lengths, z, f)
    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    with Record():
        step(v, m, lengths, z, f)
    assert seen
    heavy = ("conv", "mm", "matmul", "linear", "einsum", "fft", "baddbmm", "addmv", "dot")
    assert not [s for s in seen if any(h in s for h in heavy)], seen


def test_autograd_leaves_in_grad_what_the_entry_points_return():
    from glow_tts_amd import vocoder
    v, m, lengths, z, f = build("narrow_ragged")
    wav, grads = step(v, m, lengths, z, f)
    n = v._lengths(lengths, m.shape[0], m.shape[2])
    fwd = vocoder.pwg_train_forward(v, m, n, None, z)
    want = vocoder.pwg_train_backward(v, m, n, None, z, fwd, f)
    assert torch.equal(fwd["wav"], wav) and all(torch.equal(grads[k], want[k]) for k in grads)


def test_the_frozen_vocoder_and_bad_arguments():
    from glow_tts_amd import _lib, vocoder
    v, m, lengths, z, f = build("narrow_ragged", trainable=False)
    assert not hasattr(v, "params")
    with pytest.raises(_lib.GlowTTSHipError):
        v.generate(m, lengths, noises=z)
    cfg = dict(P.DEFAULT, R=128, G=256, S=128)                               # inference supports it, the backward's LDS plan does not
    vocoder.ParallelWaveGAN(_hp(cfg), "cuda:0", state_dict={"generator": P.random_state_dict(cfg, 1)})
    with pytest.raises(ValueError) as e:
        vocoder.ParallelWaveGAN(_hp(cfg), "cuda:0", trainable=True)
    assert "Vocoder.Residual_Channels" in str(e.value)
    L, p = _lib.lib(), _lib.ptr(z)
    assert not L.glowtts_pwg_train_supported(128, 128, 80, 1) and L.glowtts_pwg_train_supported(64, 64, 80, 512)
    assert L.glowtts_pwg_train_head_bwd(*[None] * 11, 1, 3, 256, 64, 1.0, None) == -1
    assert L.glowtts_pwg_train_head_bwd(*[p] * 11, 1, 3, 256, 60, 1.0, None) == -1
    assert L.glowtts_pwg_train_head_wgrad(*[p] * 10, 0, 3, 256, 64, None) == -1
    assert L.glowtts_pwg_train_layer_bwd(*[p] * 14, 1, 3, 256, 128, 128, 80, 1, 1, None) == -1
    assert L.glowtts_pwg_train_layer_bwd(*[p] * 14, 1, 3, 256, 64, 64, 80, 2048, 1, None) == -1
    assert L.glowtts_pwg_train_layer_wgrad(*[p] * 15, 1, 3, 256, 64, 64, 82, 1, None) == -1
    assert L.glowtts_pwg_train_first_bwd(p, p, p, p, p, p, p, 1, 3, 256, 64, None) == -1      # noises and seeds both
    assert L.glowtts_pwg_train_upsample_bwd(*[p] * 7, 1, 80, 3, 1, 17, None) == -1
    assert L.glowtts_pwg_train_cond_in_bwd(*[p] * 4, 1, 80, 3, 17, None) == -1


@pytest.mark.parametrize("name", ["default", "narrow"])                       # S = 64 at hop 256 and S = 32 at hop 15; L = 1, 2, 5, 7
def test_head_backward_alone(name):
    """d skips and the head's four parameter gradients from given d wav through the entry points, on a ragged batch whose rows beyond every utterance hold
    1e3 in every input and NaN in every output."""
    import math
    import torch.nn.functional as F
    from glow_tts_amd import _lib
    from glow_tts_amd.vocoder import ParallelWaveGAN
    cfg, lengths = {"default": P.DEFAULT, "narrow": P.NARROW}[name], [1, 2, 5, 7]
    sd = state_dict(cfg, 1.0)
    v = ParallelWaveGAN(_hp(cfg), "cuda:0", state_dict={"generator": sd}, trainable=True)
    hop, S, scale, B, Lmax = P.hop(cfg), cfg["S"], math.sqrt(1.0 / cfg["layers"]), len(lengths), max(lengths) + 1
    Tmax, g = Lmax * hop, torch.Generator().manual_seed(41)
    sks = [torch.randn(L * hop, S, generator=g) * 3.0 for L in lengths]
    dws = [torch.randn(L * hop, generator=g) for L in lengths]
    skips, dwav = pad_rows(sks, Tmax, 1e3), pad_rows(dws, Tmax, 1e3)
    nan = lambda *shape: torch.full(shape, NAN, device="cuda")
    y, h, dh, dsk = nan(B, Tmax, S), nan(B, Tmax, S), nan(B, Tmax, S), nan(B, Tmax, S)
    names = ["last_conv_layers.1.weight", "last_conv_layers.1.bias", "last_conv_layers.3.weight", "last_conv_layers.3.bias"]
    grads = {k: nan(*sd[k].shape) for k in names}
    lib, Pt, st = _lib.lib(), _lib.ptr, _lib.stream()
    n = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    work = torch.empty(lib.glowtts_pwg_train_work_floats(B, Lmax, hop, cfg["R"], S, cfg["A"]), device="cuda")
    w1, b1, w2, _ = v.head
    assert lib.glowtts_pwg_train_head_bwd(Pt(skips), Pt(n), Pt(w1), Pt(v.head_w1t), Pt(b1), Pt(w2), Pt(dwav), Pt(y), Pt(h), Pt(dh), Pt(dsk), B, Lmax, hop, S, scale, st) == 0
    assert lib.glowtts_pwg_train_head_wgrad(Pt(y), Pt(h), Pt(dh), Pt(dwav), Pt(n), Pt(work), *[Pt(grads[k]) for k in names], B, Lmax, hop, S, st) == 0
    torch.cuda.synchronize()
    for b, L in enumerate(lengths):
        for t in (y, h, dh, dsk):
            assert torch.isnan(t[b, L * hop:]).all() and torch.isfinite(t[b, :L * hop]).all()
    refs = []
    for dt in (torch.float64, torch.float32):
        p = {k: sd[k].to(dt).clone().requires_grad_(True) for k in names}
        xs = [s.T.to(dt).clone().requires_grad_(True) for s in sks]
        total = 0.0
        for x, dw in zip(xs, dws):
            hh = torch.relu(F.conv1d(torch.relu(x * scale)[None], p[names[0]], p[names[1]]))
            total = total + (F.conv1d(hh, p[names[2]], p[names[3]])[0, 0] * dw.to(dt)).sum()
        total.backward()
        r = {k: t.grad for k, t in p.items()}
        r["dskips"] = torch.cat([x.grad for x in xs], dim=1)
        refs.append(r)
    got = dict(grads, dskips=torch.cat([dsk[b, :L * hop].T for b, L in enumerate(lengths)], dim=1))
    failed = []
    for k in refs[0]:
        try:
            TR.check(f"head {name} {k}", got[k], refs[0][k], refs[1][k])
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, failed


@pytest.mark.parametrize("name", ["default", "narrow"])                       # scales [4, 4, 4, 4] and [3, 5]; L = 1, 2, 5, 7
def test_conditioning_backward_alone(name):
    """The FIRs' and conv_in's gradients from given d c, the mel and d c holding 1e3 beyond every utterance and NaN in the gradients beforehand."""
    from glow_tts_amd import _lib, vocoder
    cfg, lengths = {"default": P.DEFAULT, "narrow": P.NARROW}[name], [1, 2, 5, 7]
    sd = state_dict(cfg, 1.0)
    v = vocoder.ParallelWaveGAN(_hp(cfg), "cuda:0", state_dict={"generator": sd}, trainable=True)
    hop, A, B, Lmax = P.hop(cfg), cfg["A"], len(lengths), max(lengths) + 1
    g = torch.Generator().manual_seed(43)
    mels = [P.uniform_mel(A, L, 60 + L) for L in lengths]
    dcs = [torch.randn(L * hop, A, generator=g) for L in lengths]
    m = torch.full((B, A, Lmax), 1e3)
    for b, x in enumerate(mels):
        m[b, :, :x.shape[1]] = x
    m, dc = m.cuda(), pad_rows(dcs, Lmax * hop, 1e3)
    n = v._lengths(lengths, B, Lmax)
    c = torch.full((B, Lmax * hop, A), NAN, device="cuda")
    stages = vocoder.pwg_condition_stages(v, m, n, c)
    names = ["upsample_net.conv_in.weight"] + [f"upsample_net.upsample.up_layers.{2 * i + 1}.weight" for i in range(len(cfg["scales"]))]
    grads = {k: torch.full(tuple(sd[k].shape), NAN, device="cuda") for k in names}
    work = torch.empty(_lib.lib().glowtts_pwg_train_work_floats(B, Lmax, hop, cfg["R"], cfg["S"], A), device="cuda")
    vocoder.pwg_condition_backward(v, m, n, stages, dc, work, grads)
    torch.cuda.synchronize()
    for b, L in enumerate(lengths):
        assert torch.isnan(c[b, L * hop:]).all() and torch.isfinite(c[b, :L * hop]).all()
    refs = []
    for dt in (torch.float64, torch.float32):
        p = {k: sd[k].to(dt).clone().requires_grad_(True) for k in names}
        sum((P.condition(p, cfg, x, dt) * d.T.to(dt)).sum() for x, d in zip(mels, dcs)).backward()
        refs.append({k: t.grad for k, t in p.items()})
    failed = []
    for k in names:
        try:
            TR.check(f"conditioning {name} {k}", grads[k], refs[0][k], refs[1][k])
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, failed
