"""GPU: the Parallel WaveGAN discriminator and the adversarial loss (csrc/pwg_disc_ops.hip through `vocoder.PWGDiscriminator` and `vocoder.adversarial_mse`)
against tests/pwg_disc_ref.py.  The bar is the project's own, unchanged (`pwg_train_ref.check`): max |hip - ref64| / max |ref64| <= 4 e32 + 1e-6 with e32 from
the float32 run of the reference on the CPU and the guards 0 < e32 < 1e-3, max |ref64| > 1e-3 - separately for the scores, the loss, d wav and every
parameter gradient, for the target values 1 and 0.  Weights: the init rule times 3, signals: white noise of amplitude 0.3 (at scale 1 the early layers'
gradients fall below the guard; at 3 every guard holds in the reference alone at every shape used here, for both values)."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pwg_disc_ref as DR  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
from helpers import launch_counts, launch_reset, tiny_hp_dict  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
CASES = {
    # name: (Layers, Channels, B, T)
    "default_105": (10, 64, 2, 105),         # dilations up to 8, two tiles, the second partly filled
    "narrow_b3": (4, 16, 3, 105),            # a tile and the dilated taps straddle batch rows
    "short5": (10, 64, 2, 5),                # shorter than the dilation 8: every outer tap outside
    "t1": (3, 16, 2, 1),
    "t63": (3, 16, 2, 63),
    "t64": (4, 64, 1, 64),
    "t65": (4, 16, 2, 65),
    "splits": (4, 16, 1, 1100),              # two row chunks of the weight-gradient partition
}
_cache = {}


def hp_of(layers, C):
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Vocoder"] = {"Type": "PWG", "Train": {"Discriminator": {"Layers": layers, "Channels": C}}}
    return Recursive_Parse(copy.deepcopy(d))


def case_inputs(case):
    layers, C, B, T = CASES[case]
    g = torch.Generator().manual_seed(7)
    return DR.random_state_dict(layers, C, 1234, 3.0), (torch.randn(B, T, generator=g) * 0.3).float()


def case_reference(case, value):
    """Computed once per (case, value), shared and left unchanged"""
    if (case, value) not in _cache:
        sd, wav = case_inputs(case)
        _cache[case, value] = DR.score_grads(sd, wav, value), DR.score_grads(sd, wav, value, dtype=torch.float32)
    return _cache[case, value]


def build(case):
    from glow_tts_amd.vocoder import PWGDiscriminator
    layers, C, _, _ = CASES[case]
    sd, wav = case_inputs(case)
    return PWGDiscriminator(hp_of(layers, C), "cuda:0", state_dict={"discriminator": sd}), wav.cuda()


def step(disc, wav, value, freeze=False):
    """score + loss + backward through autograd -> dict(scores, loss, dwav, grads)"""
    from glow_tts_amd.vocoder import adversarial_mse
    for p in disc.params.values():
        p.grad = None
    x = wav.clone().requires_grad_(True)
    scores = disc.score(x, freeze=freeze)
    loss, terms = adversarial_mse(scores, value)
    loss.backward()
    torch.cuda.synchronize()
    return {"scores": scores.detach(), "loss": loss.detach().reshape(1), "terms": terms, "dwav": x.grad, "grads": {k: p.grad for k, p in disc.params.items()}}


@pytest.mark.parametrize("value", [1.0, 0.0])
@pytest.mark.parametrize("case", list(CASES))
def test_operators_match_the_float64_reference(case, value):
    r64, r32 = case_reference(case, value)
    disc, wav = build(case)
    got = step(disc, wav, value)
    assert torch.equal(got["terms"][:1], got["loss"]) and float(got["terms"][1]) == 0.0
    failed = []
    for name in ("scores", "loss", "dwav"):
        assert got[name].shape == r64[name].shape, name
        try:
            TR.check(f"{case} v={value} {name}", got[name], r64[name], r32[name])
        except AssertionError as err:
            failed.append(str(err))
    assert set(got["grads"]) == set(r64["grads"])
    for name in r64["grads"]:
        assert got["grads"][name].shape == r64["grads"][name].shape, name
        try:
            TR.check(f"{case} v={value} {name}", got["grads"][name], r64["grads"][name], r32["grads"][name])
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, failed


def test_factor_scales_the_loss_and_its_gradient():
    from glow_tts_amd.vocoder import adversarial_mse
    g = torch.Generator().manual_seed(3)
    p = torch.randn(3, 1500, generator=g).cuda()                            # 4500 scores: two blocks of the loss
    ref = ((p.double().cpu() - 1.0) ** 2).mean()
    x = p.clone().requires_grad_(True)
    loss, terms = adversarial_mse(x, 1.0, factor=4.0)
    loss.backward()
    assert abs(float(terms[0]) - float(ref)) <= 1e-6 * float(ref) and abs(float(loss.detach()) - 4.0 * float(ref)) <= 1e-6 * 4.0 * float(ref)
    want = 4.0 * 2.0 * (p.double().cpu() - 1.0) / p.numel()
    assert float((x.grad.double().cpu() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    y = p.clone().requires_grad_(True)
    both, t2 = adversarial_mse(torch.cat([y, y]), (1.0, 0.0))               # [real; fake]: the sum of the halves' means
    ref2 = ref + (p.double().cpu() ** 2).mean()
    assert abs(float(both.detach()) - float(ref2)) <= 1e-6 * float(ref2) and abs(float(t2[0]) - float(ref)) <= 1e-6 * float(ref)


def test_guard_rows_are_neither_read_nor_written():
    """Inputs carry 1e3 and every output NaN in a spare row after the last batch row: the spare row stays NaN and no result changes."""
    from glow_tts_amd.vocoder import pwg_disc_backward, pwg_disc_forward
    case = "narrow_b3"
    layers, C, B, T = CASES[case]
    disc, wav = build(case)
    g = torch.Generator().manual_seed(9)
    ds = torch.randn(B, T, generator=g).cuda()
    plain_f = pwg_disc_forward(disc, wav)
    plain_dwav, plain_grads = pwg_disc_backward(disc, plain_f, ds)
    spare = []

    def alloc(*shape):
        if len(shape) >= 2 and shape[:2] == (B, T):
            buf = torch.full((B + 1,) + tuple(shape[1:]), NAN, device="cuda")
            spare.append(buf)
            return buf[:B]
        return torch.full(shape, NAN, device="cuda")
    padded = torch.full((B + 1, T), 1e3, device="cuda")
    padded[:B] = wav
    dsp = torch.full((B + 1, T), 1e3, device="cuda")
    dsp[:B] = ds
    f = pwg_disc_forward(disc, padded[:B], alloc=alloc)
    dwav, grads = pwg_disc_backward(disc, f, dsp[:B], alloc=alloc)
    torch.cuda.synchronize()
    assert len(spare) == (layers - 1) + 1 + 1 + 2 + 1                       # hidden outputs, scores, dpre, dout and dx, d wav
    assert all(torch.isnan(b[B]).all() and torch.isfinite(b[:B]).all() for b in spare)
    assert torch.equal(f["scores"], plain_f["scores"]) and torch.equal(dwav, plain_dwav)
    assert all(torch.equal(a, b) for a, b in zip(f["keep"], plain_f["keep"]))
    assert all(torch.equal(grads[k], plain_grads[k]) for k in plain_grads)


@pytest.mark.parametrize("case", ["narrow_b3", "default_105"])
def test_a_row_is_the_same_alone_and_in_a_batch(case):
    _, _, B, T = CASES[case]
    disc, wav = build(case)
    ds = torch.randn(B, T, generator=torch.Generator().manual_seed(9)).cuda()

    def run(w, d):
        x = w.clone().requires_grad_(True)
        scores = disc.score(x)
        (scores * d).sum().backward()
        return scores.detach(), x.grad
    scores, dwav = run(wav, ds)
    for b in range(B):
        s1, d1 = run(wav[b:b + 1], ds[b:b + 1])
        assert torch.equal(s1[0], scores[b]) and torch.equal(d1[0], dwav[b]), b


def test_two_runs_are_bit_identical():
    for case in ("default_105", "splits"):
        disc, wav = build(case)
        a, b = step(disc, wav, 1.0), step(disc, wav, 1.0)
        assert all(torch.equal(a[k], b[k]) for k in ("scores", "loss", "dwav")) and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])


def test_freeze_runs_the_data_chain_alone():
    disc, wav = build("default_105")
    full = step(disc, wav, 1.0)
    launch_reset()
    frozen = step(disc, wav, 1.0, freeze=True)
    counts = launch_counts()
    assert torch.equal(frozen["dwav"], full["dwav"]) and torch.equal(frozen["scores"], full["scores"])
    assert all(g is None for g in frozen["grads"].values())
    assert not any("wgrad" in k and n for k, n in counts.items()), counts
    assert counts.get("pwg_disc_layer_bwd") == 8 and counts.get("pwg_disc_first_bwd") == 1 and counts.get("pwg_disc_last_bwd") == 1
    launch_reset()
    step(disc, wav, 1.0)
    counts = launch_counts()
    assert counts.get("pwg_disc_wgrad") == 10 and counts.get("pwg_disc_wgrad_sum") == 10 and not counts.get("pwg_wgrad") and not counts.get("pwg_wgrad_sum")


def test_real_and_fake_as_one_batch_of_2b_rows():
    """`score_pair`: ONE forward over [real; fake]; L_D's gradients from the 2 B call equal the float64 reference of the sum of both terms under the bar and do
    not reach the fake waveform; the generator term's backward is the frozen data chain over the fake rows: no weight-gradient launch, no parameter gradient,
    d fake bit-identical to a frozen score of the fake rows alone."""
    from glow_tts_amd.vocoder import adversarial_mse
    layers, C, B, T = CASES["narrow_b3"]
    disc, real = build("narrow_b3")
    sd, _ = case_inputs("narrow_b3")
    fake = (torch.randn(B, T, generator=torch.Generator().manual_seed(21)) * 0.3).float().cuda()
    r64, r32 = DR.pair_grads(sd, real.cpu(), fake.cpu()), DR.pair_grads(sd, real.cpu(), fake.cpu(), dtype=torch.float32)
    x = fake.clone().requires_grad_(True)
    launch_reset()
    both, p_fake = disc.score_pair(real, x)
    counts = launch_counts()
    assert counts.get("pwg_disc_first") == 1 and counts.get("pwg_disc_layer") == layers - 2 and counts.get("pwg_disc_last") == 1
    assert both.shape == (2 * B, T) and torch.equal(both[B:], p_fake)
    adv, _ = adversarial_mse(p_fake, 1.0, 4.0)
    launch_reset()
    adv.backward()
    counts = launch_counts()
    assert not any("wgrad" in k and n for k, n in counts.items()), counts
    assert all(p.grad is None for p in disc.params.values())
    alone = step(disc, fake, 1.0, freeze=True)
    assert torch.equal(p_fake, alone["scores"])
    ref_d = DR.score_grads(sd, fake.cpu(), 1.0, factor=4.0), DR.score_grads(sd, fake.cpu(), 1.0, dtype=torch.float32, factor=4.0)
    TR.check("generator term d fake", x.grad, ref_d[0]["dwav"], ref_d[1]["dwav"])
    for p in disc.params.values():
        p.grad = None
    x.grad = None
    d_loss, terms = adversarial_mse(both, (1.0, 0.0))
    d_loss.backward()
    torch.cuda.synchronize()
    assert x.grad is None
    failed = []
    for name, got, k in [("L_D", d_loss.detach().reshape(1), "loss"), ("terms", terms, "terms")]:
        try:
            TR.check(name, got, r64[k], r32[k])
        except AssertionError as err:
            failed.append(str(err))
    for name, p in disc.params.items():
        try:
            TR.check("L_D " + name, p.grad, r64["grads"][name], r32["grads"][name])
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, failed
