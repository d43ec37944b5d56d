"""GPU: the multi-resolution STFT loss (csrc/stft_loss_ops.hip through `vocoder.MultiResolutionSTFTLoss`) against tests/pwg_train_ref.py.  The bar is the
project's own, unchanged (`pwg_train_ref.check`): max |hip - ref64| / max |ref64| <= 4 e32 + 1e-6 with e32 from the float32 run of the reference on the CPU,
separately for the loss, its per-resolution terms and d pred.

Parity inputs are white noise of amplitude 0.3 under seeds at which the smallest re^2 + im^2 of either signal stays above 10 x the 1e-7 clamp (asserted
in float64).  That is far enough: a bin's fp32 error is about eps |frame| = 6e-8 * 4.5 = 3e-7 in amplitude, so at re^2 + im^2 = 1e-6 (amplitude 1e-3) the
fp32 power is off by 6e-10, three orders below its distance to the clamp - no fp32 run decides the clamp differently from float64.  The silent-target cases
hold the PREDICTION to the same condition (its bins carry the 1 / |X| of the gradient; the target's clamped bins are constants)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pwg_train_ref as TR  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = [(256, 50, 240)]                                 # win / hop is not an integer: five frames cover most samples, four the rest
CASES = {
    # name: (resolutions, B, T, seed, silent target from this sample on or None)
    "default": (TR.RESOLUTIONS, 2, 2304, 4, None),       # T above the 1024 that the reflect padding of n_fft = 2048 needs
    "small": (SMALL, 2, 600, 2, None),
    "silent_half": (TR.RESOLUTIONS, 2, 2304, 4, 1152),   # the clamp is active on the target's frames inside the silence
    "silent_half_small": (SMALL, 3, 600, 2, 300),
}
_cache = {}


def case_inputs(case):
    res, B, T, seed, silent = CASES[case]
    pred, target = TR.signals(B, T, seed)
    if silent is not None:
        target = target.clone()
        target[:, silent:] = 0.0
    return res, pred, target


def case_reference(case):
    """(ref64, ref32) of a case, computed once"""
    if case not in _cache:
        res, pred, target = case_inputs(case)
        _cache[case] = TR.loss_and_grad(pred, target, res), TR.loss_and_grad(pred, target, res, torch.float32)
    return _cache[case]


def run(res, pred, target):
    """One forward and backward through autograd -> {'L', 'terms', 'dpred'}"""
    from glow_tts_amd.vocoder import MultiResolutionSTFTLoss
    crit = MultiResolutionSTFTLoss(res, "cuda:0")
    p = pred.cuda().requires_grad_(True)
    loss = crit(p, target.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return {"L": loss.detach().reshape(1), "terms": crit.terms.clone(), "dpred": p.grad}


@pytest.mark.parametrize("case", list(CASES))
def test_loss_terms_and_gradient_match_the_float64_reference(case):
    res, pred, target = case_inputs(case)
    r64, r32 = case_reference(case)
    if CASES[case][4] is None:
        assert r64["low"] > 10 * TR.CLAMP                # no bin near the clamp
    else:
        assert r64["low"] < TR.CLAMP < 10 * TR.CLAMP < r64["low_pred"]      # the clamp is active, on the target alone
    got = run(res, pred, target)
    assert all(torch.isfinite(t).all() for t in got.values())
    failed = []
    for name in ("L", "terms", "dpred"):
        assert got[name].shape == r64[name].shape, name
        try:
            TR.check(case + " " + name, got[name], r64[name], r32[name])
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, failed


def test_pred_equal_to_target():
    res, pred, _ = case_inputs("small")
    ref = TR.stft_loss(pred, pred, res)[0]
    got = run(res, pred, pred.clone())
    assert float(got["L"]) == float(ref) == 0.0
    assert torch.isfinite(got["dpred"]).all() and torch.isfinite(got["terms"]).all()


def test_two_runs_are_bit_identical():
    for case in ("default", "silent_half_small"):
        res, pred, target = case_inputs(case)
        a, b = run(res, pred, target), run(res, pred, target)
        assert all(torch.equal(a[k], b[k]) for k in a)


def test_autograd_scales_what_the_entry_points_return_and_logs_two_launches_each_way():
    from glow_tts_amd import vocoder
    res, pred, target = case_inputs("default")
    crit = vocoder.MultiResolutionSTFTLoss(res, "cuda:0")
    p, t = pred.cuda(), target.cuda()
    launch_reset()
    loss, terms, keeps = vocoder.stft_loss_forward(crit, p, t)
    d = vocoder.stft_loss_backward(crit, keeps, terms, torch.full((1,), 0.5, device="cuda"), *p.shape)
    torch.cuda.synchronize()
    counts = {k: n for k, n in launch_counts().items() if n}
    assert counts == {"stft_loss_fwd": 3, "stft_loss_reduce": 3, "stft_loss_bwd_frames": 3, "stft_loss_bwd_fold": 3}, counts
    q = p.clone().requires_grad_(True)
    out = crit(q, t)
    (out * 0.5).backward()
    assert torch.equal(out.reshape(1), loss) and torch.equal(q.grad, d)
    assert abs(float(loss) - float(terms[:, :2].sum()) / 3) < 1e-6


def test_no_torch_fft_or_matrix_op_runs():
    from torch.utils._python_dispatch import TorchDispatchMode
    from glow_tts_amd.vocoder import MultiResolutionSTFTLoss
    res, pred, target = case_inputs("small")
    crit = MultiResolutionSTFTLoss(res, "cuda:0")
    p, t = pred.cuda().requires_grad_(True), target.cuda()
    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    with Record():
        crit(p, t).backward()
    torch.cuda.synchronize()
    assert seen
    heavy = ("fft", "stft", "mm", "matmul", "conv", "einsum", "norm", "log", "sqrt")
    assert not [s for s in seen if any(h in s for h in heavy)], seen


def test_unsupported_input_raises_naming_the_keys():
    from glow_tts_amd import _lib
    from glow_tts_amd.vocoder import MultiResolutionSTFTLoss
    for res, word in (([(1000, 120, 600)], "n_fft"), ([(8192, 120, 600)], "n_fft"), ([(512, 50, 600)], "win"), ([(512, 300, 240)], "hop")):
        with pytest.raises(ValueError) as e:
            MultiResolutionSTFTLoss(res, "cuda:0")
        assert "Vocoder.Train.STFT_Resolutions" in str(e.value) and word in str(e.value)
    crit = MultiResolutionSTFTLoss(None, "cuda:0")
    x = torch.zeros(2, 1024, device="cuda")
    with pytest.raises(ValueError) as e:                 # T <= n_fft / 2 of (2048, 240, 1200)
        crit(x, x)
    assert "Vocoder.Train.STFT_Resolutions" in str(e.value) and "Segment_Frames" in str(e.value)
    x = torch.zeros(2, 2304, device="cuda")
    with pytest.raises(ValueError) as e:                 # ragged
        crit(x, x, lengths=[2304, 2000])
    assert "ragged" in str(e.value)
    with pytest.raises(ValueError):
        crit(x, x[:, :2000])
    with pytest.raises(_lib.GlowTTSHipError):
        crit(x.cpu(), x.cpu())
    L = _lib.lib()
    assert L.glowtts_stft_loss_forward(None, None, None, None, None, None, None, None, 2, 2304, 2048, 1200, 240, 1.0, 0, None) == -1
    assert L.glowtts_stft_loss_backward(None, None, None, None, None, None, None, 2, 2304, 2048, 1200, 240, 1.0, 0, None) == -1
    ok = (_lib.ptr(x),) * 8
    for B, T, n_fft, win, hop in ((2, 1024, 2048, 1200, 240), (2, 2304, 1000, 600, 120), (2, 2304, 512, 600, 50), (2, 2304, 512, 240, 300), (0, 2304, 512, 240, 50)):
        assert L.glowtts_stft_loss_forward(*ok, B, T, n_fft, win, hop, 1.0, 0, None) == -1
        assert not L.glowtts_stft_loss_supported(n_fft, win, hop, T) or B == 0
    assert L.glowtts_stft_loss_supported(2048, 1200, 240, 1025) and L.glowtts_stft_loss_supported(256, 240, 50, 600)
