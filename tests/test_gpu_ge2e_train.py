"""GPU: the training path of the GE2E speaker encoder (csrc/ge2e_train_ops.hip through `speaker_encoder`) against tests/ge2e_train_ref.py.  The bar is the
project's GE2E bar unchanged (`ge2e_ref.check`): max |hip - ref64| / max |ref64| <= 4 e32 + 1e-6 with e32 from the float32 run of the reference, separately
for L, de, dw and every parameter gradient."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ge2e_ref as R  # noqa: E402
import ge2e_train_ref as TR  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402
from test_gpu_ge2e import make_hp  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


def build(case, trainable=True):
    from glow_tts_amd.speaker_encoder import GE2E
    S, M, T, Mel, H, Stacks, E, _ = TR.CASES[case]
    sizes, sd, x = TR.case_inputs(case)
    return GE2E(make_hp(Mel, H, Stacks, E, M, T), "cuda:0", state_dict=sd, trainable=trainable), sizes, x.cuda()


def entry_points(enc, x, S, M, w=TR.W0, da=None):
    """One step through the C entry points -> {'L', 'e', 'de', 'dw', 'grads'}"""
    from glow_tts_amd import speaker_encoder as SE
    keep, e = SE.train_forward(enc, x)
    loss, de, dw = SE.ge2e_loss_launch(e, torch.tensor(float(w), device=x.device), S, M)
    grads = SE.train_backward(enc, x, keep, de, da)
    torch.cuda.synchronize()
    return {"L": loss, "e": e, "de": de, "dw": dw, "grads": grads}


@pytest.mark.parametrize("case", list(TR.CASES))
def test_step_matches_the_float64_reference(case):
    S, M = TR.CASES[case][:2]
    enc, sizes, x = build(case)
    got = TR.tensors(entry_points(enc, x, S, M))
    r64, r32 = (TR.tensors(r) for r in TR.case_reference(case))
    assert set(got) == set(r64)
    failed = []
    for name in r64:
        assert got[name].shape == r64[name].shape, name
        if case == "one_cell" and name == "lstm.weight_hh_l0":          # h_{-1} = 0 and T = 1: exactly zero, on both sides
            assert torch.equal(got[name].cpu(), torch.zeros_like(got[name].cpu())) and not r64[name].any()
            continue
        try:
            R.check(case + " " + name, got[name], r64[name], r32[name])
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, failed


@pytest.mark.parametrize("case", ["two_layers", "second_tile", "wide"])
def test_training_forward_is_the_inference_forward_bit_for_bit(case):
    from glow_tts_amd import speaker_encoder as SE
    enc, sizes, x = build(case)
    keep, e = SE.train_forward(enc, x)
    hs, e_inf, _ = enc.forward_all(x, samples=1, hidden=True, raw=True)
    assert torch.equal(keep[:hs.numel()].view_as(hs), hs) and torch.equal(e, e_inf)


def test_two_runs_give_identical_gradients():
    for case in ("chunks", "odd"):
        S, M = TR.CASES[case][:2]
        enc, _, x = build(case)
        a, b = TR.tensors(entry_points(enc, x, S, M)), TR.tensors(entry_points(enc, x, S, M))
        for name in a:
            assert torch.equal(a[name], b[name]), (case, name)


def test_rows_beyond_n_in_the_last_tile_never_reach_a_gradient():
    """A speaker-major batch of N = 6 sequences, alone and as the first rows of a batch of 10 (pad sequences appended within the 16-row tile), every
    buffer the kernels write pre-filled with NaN: the per-sequence results (e, the gradients da of the pre-activations for a given de) are bit-identical,
    de of the loss is finite, and no NaN reaches a gradient."""
    from glow_tts_amd import _lib, speaker_encoder as SE
    case = "odd"
    S, M, T, Mel, H, Stacks, E, _ = TR.CASES[case]
    enc, sizes, x = build(case)
    N, pad = S * M, 4
    big = torch.cat([x, R.uniform_input(pad, Mel, T, 77).cuda()])
    L = _lib.lib()

    def run(inp, de_rows):
        n = inp.shape[0]
        enc._pack()
        keep = torch.full((L.glowtts_ge2e_train_keep_floats(n, T, H, Stacks),), NAN, device="cuda")
        e = torch.full((n, E), NAN, device="cuda")
        _lib.check(L.glowtts_ge2e_train_forward(inp.data_ptr(), enc._images.data_ptr(), enc._biases.data_ptr(), enc.linear.weight.data_ptr(),
                                                enc.linear.bias.data_ptr(), keep.data_ptr(), e.data_ptr(), n, Mel, T, H, Stacks, E, _lib.stream()), "forward")
        de = de_rows(e)
        da = torch.full((Stacks, n, T, 4 * H), NAN, device="cuda")
        work = torch.full((L.glowtts_ge2e_train_work_floats(n, T, Mel, H, Stacks),), NAN, device="cuda")
        gw, gb = torch.full((E, H), NAN, device="cuda"), torch.full((E,), NAN, device="cuda")
        _lib.check(L.glowtts_ge2e_train_backward(enc._images_t.data_ptr(), keep.data_ptr(), enc.linear.weight.data_ptr(), de.data_ptr(), da.data_ptr(),
                                                 work.data_ptr(), gw.data_ptr(), gb.data_ptr(), n, T, H, Stacks, E, _lib.stream()), "backward")
        grads = []
        for k in range(Stacks):
            g = [torch.full(s, NAN, device="cuda") for s in ((4 * H, Mel if k == 0 else H), (4 * H, H), (4 * H,), (4 * H,))]
            _lib.check(L.glowtts_ge2e_train_wgrad(inp.data_ptr(), keep.data_ptr(), da.data_ptr(), work.data_ptr(), *[t.data_ptr() for t in g], k, n, Mel, T, H,
                                                  Stacks, _lib.stream()), "wgrad")
            grads += g
        torch.cuda.synchronize()
        return e, de, da, grads + [gw, gb]

    def loss_de(e):
        out = SE.ge2e_loss_launch(e[:N].contiguous(), torch.tensor(TR.W0, device="cuda"), S, M)[1]
        return out

    e1, de1, da1, g1 = run(x, loss_de)
    assert torch.isfinite(de1).all() and all(torch.isfinite(t).all() for t in g1)
    e2, de2, da2, g2 = run(big, lambda e: torch.cat([loss_de(e), torch.randn(pad, E, device="cuda")]))
    assert torch.equal(e2[:N], e1) and torch.equal(de2[:N], de1)
    assert torch.equal(da2[:, :N], da1)
    assert all(torch.isfinite(t).all() for t in g2)


def test_launch_log_of_a_step():
    case = "two_layers"
    S, M, T, Mel, H, Stacks, E, _ = TR.CASES[case]
    enc, _, x = build(case)
    entry_points(enc, x, S, M)                               # packs
    launch_reset()
    entry_points(enc, x, S, M)
    counts = {k: n for k, n in launch_counts().items() if n}
    assert counts.pop("ge2e_cell_bwd") == T + Stacks - 1 and counts.pop("ge2e_cell") == T + Stacks - 1
    assert counts.pop("ge2e_wgrad") == 2 * Stacks and counts.pop("ge2e_head_bwd") == 1 and counts.pop("ge2e_head_fwd") == 1
    assert sorted(counts) == ["ge2e_loss_" + n for n in ("centroid", "dcent", "du", "final", "norm", "scores")] and set(counts.values()) == {1}, counts
    assert not [k for k in launch_counts() if "Cijk" in k or "miopen" in k.lower()]


def test_no_torch_matrix_or_rnn_op_runs_in_a_step():
    """Every torch op of embed + loss + backward, recorded at dispatch: allocations, views and the scaling of the saved gradients by the incoming one - nothing
    that could launch a `Cijk_*` (hipBLASLt / rocBLAS) or MIOpen kernel."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from glow_tts_amd.speaker_encoder import GE2ELoss
    case = "two_layers"
    S, M = TR.CASES[case][:2]
    enc, _, x = build(case)
    crit = GE2ELoss().cuda()
    crit(enc.embed(x), S, M).backward()                      # warm: packs
    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    with Record():
        crit(enc.embed(x), S, M).backward()
    torch.cuda.synchronize()
    assert seen
    heavy = ("mm", "matmul", "linear", "lstm", "rnn", "conv", "einsum", "dot", "baddbmm", "addmv", "softmax", "norm")
    assert not [s for s in seen if any(h in s for h in heavy)], seen


def test_autograd_leaves_in_grad_what_the_entry_points_return():
    from glow_tts_amd.speaker_encoder import GE2ELoss
    case = "odd"
    S, M = TR.CASES[case][:2]
    enc, _, x = build(case)
    want = entry_points(enc, x, S, M)
    crit = GE2ELoss(init_w=TR.W0).cuda()
    e = enc.embed(x)
    loss = crit(e, S, M)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(e, want["e"]) and torch.equal(loss.reshape(1), want["L"]) and torch.equal(crit.w.grad.reshape(1), want["dw"])
    params = dict(enc.named_parameters())
    assert set(params) == set(want["grads"])
    for name, g in want["grads"].items():
        assert torch.equal(params[name].grad, g), name


def test_the_frozen_encoder_and_bad_arguments():
    from glow_tts_amd import _lib
    from glow_tts_amd.speaker_encoder import GE2ELoss
    enc, _, x = build("two_layers", trainable=False)
    assert not any(p.requires_grad for p in enc.parameters()) and not enc.training
    with pytest.raises(_lib.GlowTTSHipError):
        enc.embed(x)
    crit = GE2ELoss().cuda()
    e = torch.randn(6, 16, device="cuda")
    for S, M in ((1, 6), (6, 1), (2, 2)):
        with pytest.raises(ValueError):
            crit(e, S, M)
    L = _lib.lib()
    assert L.glowtts_ge2e_train_loss(None, None, None, None, None, None, 2, 2, 8, None) == -1
    assert L.glowtts_ge2e_train_backward(None, None, None, None, None, None, None, None, 4, 5, 16, 2, 16, None) == -1
