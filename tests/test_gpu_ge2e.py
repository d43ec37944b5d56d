"""GPU: the GE2E speaker encoder (csrc/ge2e_ops.hip through `speaker_encoder.GE2E`) against tests/ge2e_ref.py.  The bar is the project's own, measured on
the reference arithmetic and never on the code under test: with e32 = max |ref32 - ref64| / max |ref64|, the HIP result must satisfy
max |hip - ref64| / max |ref64| <= 4 e32 + 1e-6, separately for the raw embeddings, the d-vectors and (small cases) all hidden states."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ge2e_ref as R  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, Samples, T, Mel, H, Stacks, E, scale)
CASES = {
    "one_cell": (1, 1, 1, 4, 16, 1, 8, 1),                 # one cell, no recurrence
    "tiny_hp": (2, 3, 5, 12, 16, 2, 16, 1),                # the tiny-hp shape
    "odd": (3, 2, 7, 20, 48, 3, 24, 3),                    # H not a power of two, three layers on the diagonal, odd T, saturating gates
    "second_tile": (17, 1, 3, 12, 80, 2, 16, 3),           # one row in a second 16-row tile
    "shipped": (2, 5, 64, 80, 256, 3, 256, 1),             # the shipped sizes
    "shipped_saturating": (2, 5, 64, 80, 256, 3, 256, 3),
}
HIDDEN = ("one_cell", "tiny_hp", "odd", "second_tile")
WEIGHT_SEED, INPUT_SEED = 4321, 99


def make_hp(Mel, H, Stacks, E, Samples=5, T=64):
    from glow_tts_amd.hparams import Recursive_Parse
    return Recursive_Parse({"Sound": {"Mel_Dim": Mel},
                            "Speaker_Embedding": {"Embedding_Size": E, "GE2E": {"LSTM": {"Sizes": H, "Stacks": Stacks}, "Checkpoint_Path": None,
                                                                                  "Inference": {"Samples": Samples, "Slice_Length": T, "Overlap_Length": T // 2}}}})


def build(case):
    from glow_tts_amd.speaker_encoder import GE2E
    B, S, T, Mel, H, Stacks, E, scale = CASES[case]
    sizes = R.sizes_of(Mel, H, Stacks, E)
    sd = R.random_state_dict(sizes, WEIGHT_SEED, scale)
    enc = GE2E(make_hp(Mel, H, Stacks, E, S, T), "cuda:0", state_dict=sd)
    return enc, sd, sizes, R.uniform_input(B * S, Mel, T, INPUT_SEED)


@pytest.mark.parametrize("case", list(CASES))
def test_matches_the_float64_reference(case):
    enc, sd, sizes, x = build(case)
    S = CASES[case][1]
    hs, e, d = enc.forward_all(x.cuda(), hidden=case in HIDDEN, raw=True)
    torch.cuda.synchronize()
    hs64, e64, d64 = R.forward(sd, sizes, x, S)
    hs32, e32, d32 = R.forward(sd, sizes, x, S, torch.float32)
    assert d.shape == (CASES[case][0], sizes["E"]) and e.shape == (x.shape[0], sizes["E"])
    assert torch.isfinite(d).all() and (d.norm(dim=1) - 1).abs().max() < 1e-5
    R.check(case + " e", e, e64, e32)
    R.check(case + " d", d, d64, d32)
    if case in HIDDEN:
        R.check(case + " hs", hs, hs64, hs32)
    assert torch.equal(enc(x.cuda()), d)                   # the plain call (no hs, no e: hidden states in the work buffer) gives the same d-vectors


def test_an_utterance_is_bit_identical_alone_in_any_batch_and_from_run_to_run():
    enc, _, _, _ = build("odd")
    _, S, T, Mel = CASES["odd"][:4]
    utt = R.uniform_input(S, Mel, T, 7).cuda()
    alone = enc(utt)
    for pos in (0, 3, 6):
        batch = R.uniform_input(7 * S, Mel, T, 8).cuda()
        batch[pos * S:(pos + 1) * S] = utt
        got = enc(batch)
        assert torch.equal(got[pos:pos + 1], alone), pos
        assert torch.equal(enc(batch), got)                # run to run
    assert torch.equal(enc(utt), alone)


def test_launch_log_and_no_torch_ops_on_the_path():
    from torch.utils._python_dispatch import TorchDispatchMode
    enc, _, _, _ = build("tiny_hp")
    _, S, T, Mel, H, Stacks, E, _ = CASES["tiny_hp"]
    enc(R.uniform_input(S, Mel, T, 1).cuda())              # packs the weight images: once, not per call

    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    totals = []
    for N, samples in ((1, 1), (33, 3)):                   # one sequence; 33: one row in a third 16-row tile
        x = R.uniform_input(N, Mel, T, 2).cuda()
        launch_reset()
        with Record():
            enc(x, samples=samples)
        counts = {k: n for k, n in launch_counts().items() if n}
        assert set(counts) == {"ge2e_cell", "ge2e_head"}, counts
        assert counts == {"ge2e_cell": T + Stacks - 1, "ge2e_head": 1}, counts
        totals.append(sum(counts.values()))
    assert totals[0] == totals[1] <= T * Stacks + 2
    assert not [s for s in seen if "empty" not in s], seen   # allocations only


def test_repacks_only_when_the_parameters_change():
    enc, sd, sizes, x = build("tiny_hp")
    S = CASES["tiny_hp"][1]
    x = x.cuda()
    launch_reset()
    a = enc(x)
    enc(x)
    assert launch_counts().get("ge2e_pack", 0) == sizes["Stacks"]
    with torch.no_grad():
        enc.lstm.weight_hh_l1.mul_(0.5)
    b = enc(x)
    assert launch_counts().get("ge2e_pack", 0) == 2 * sizes["Stacks"] and not torch.equal(a, b)
    sd2 = dict(sd, **{"lstm.weight_hh_l1": sd["lstm.weight_hh_l1"] * 0.5})
    _, _, d64 = R.forward(sd2, sizes, x.cpu(), S)
    _, _, d32 = R.forward(sd2, sizes, x.cpu(), S, torch.float32)
    R.check("repacked d", b, d64, d32)


def test_bad_arguments_are_refused():
    from glow_tts_amd import _lib
    enc, _, _, x = build("tiny_hp")
    with pytest.raises(ValueError):
        enc(x.cuda()[:5])                                  # not a multiple of Samples
    with pytest.raises(ValueError):
        enc(torch.zeros(3, 16, 5, device="cuda"))          # another Mel
    with pytest.raises(_lib.GlowTTSHipError):
        enc(x)                                             # a host tensor: no CPU fallback
    L = _lib.lib()
    assert L.glowtts_ge2e_forward(None, None, None, None, None, None, None, None, None, 3, 3, 12, 5, 16, 2, 16, None) == -1
    assert L.glowtts_ge2e_supported(80, 256, 3, 256) == 1 and L.glowtts_ge2e_supported(80, 768, 8, 256) == 1
    assert L.glowtts_ge2e_supported(80, 250, 3, 256) == 0 and L.glowtts_ge2e_supported(82, 256, 3, 256) == 0 and L.glowtts_ge2e_supported(80, 256, 9, 256) == 0
