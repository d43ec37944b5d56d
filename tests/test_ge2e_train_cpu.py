"""CPU suite of the GE2E speaker encoder's training: the reference loss (gradcheck, invariances, mutations rejected by the bar, the guards of the GPU cases for
the reference alone), the batch sampler, the equal error rate, the checkpoint layout, the yaml defaults and the C-ABI additions."""
import copy
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import ge2e_ref as R  # noqa: E402
import ge2e_train_ref as TR  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402


def test_gradcheck_of_the_float64_loss():
    g = torch.Generator().manual_seed(0)
    e = torch.randn(6, 5, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.tensor(3.0, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b: TR.ge2e_loss(a, b, 3, 2), (e, w))
    assert torch.autograd.gradcheck(lambda a, b: TR.ge2e_loss(a, b, 2, 3), (e, w))


def test_invariances_of_the_loss():
    g = torch.Generator().manual_seed(1)
    S, M, E = 3, 4, 7
    e = torch.randn(S * M, E, generator=g, dtype=torch.float64)
    w = torch.tensor(10.0, dtype=torch.float64)

    def grad(x, **kw):
        x = x.clone().requires_grad_(True)
        L = TR.ge2e_loss(x, w, S, M, **kw)
        L.backward()
        return L.detach(), x.grad

    L0, de0 = grad(e)
    perm = torch.cat([j * M + torch.randperm(M, generator=g) for j in range(S)])          # the utterances permuted within each speaker
    L1, de1 = grad(e[perm])
    assert abs(L1 - L0) < 1e-13 and (de1 - de0[perm]).abs().max() < 1e-13
    L2, de2 = grad(e, bias=-5.0)                                                          # a constant on every score changes nothing
    assert abs(L2 - L0) < 1e-13 and (de2 - de0).abs().max() < 1e-13
    L3, de3 = grad(e * 7.5)                                                               # the loss sees directions only
    assert abs(L3 - L0) < 1e-13 and (de3 * 7.5 - de0).abs().max() < 1e-12


def test_guards_of_the_gpu_cases_hold_for_the_reference_alone():
    """Every tensor the bar applies to, in all seven cases: 0 < e32 < 1e-3 and max |ref64| > 1e-3 from the float64 / float32 reference alone; the one exception
    is the no-recurrence case's weight_hh gradient, exactly zero in both precisions."""
    for case in TR.CASES:
        r64, r32 = (TR.tensors(r) for r in TR.case_reference(case))
        for name in r64:
            if case == "one_cell" and name == "lstm.weight_hh_l0":
                assert not r64[name].any() and not r32[name].any()
                continue
            _, e32, scale = R.errors(r32[name], r64[name], r32[name])
            assert 0 < e32 < 1e-3 and scale > 1e-3, (case, name, e32, scale)


@pytest.mark.parametrize("mutation", TR.MUTATIONS)
def test_mutations_are_rejected_by_the_bar(mutation):
    """A float32 run of a wrong formula stands in for a wrong kernel: the bar (4 e32 + 1e-6, e32 from the right formula) rejects it on L, de and dw.
    'mean': the own speaker's mean in place of sum / (M - 1) - as c_j - u_ji / (M - 1); merely dividing the exclusive sum by M is no error, the cosine
    does not see the centroid's length."""
    case = "odd"
    S, M = TR.CASES[case][:2]
    sizes, sd, x = TR.case_inputs(case)
    r64, r32 = (TR.tensors(r) for r in TR.case_reference(case))
    wrong = TR.tensors(TR.run(sd, sizes, x, S, M, dtype=torch.float32, mutate=mutation))
    for name in ("L", "de", "dw"):
        err, e32, _ = R.errors(wrong[name], r64[name], r32[name])
        assert err > 100 * (4 * e32 + 1e-6), (mutation, name, err, e32)
        with pytest.raises(AssertionError):
            R.check(mutation + " " + name, wrong[name], r64[name], r32[name])
    e = torch.randn(6, 5, dtype=torch.float64)
    U = torch.nn.functional.normalize(e, dim=1).reshape(3, 2, 5)
    a, b = (U.sum(1)[:, None] - U) / 1, (U.sum(1)[:, None] - U) / 2
    assert torch.allclose(torch.nn.functional.cosine_similarity(U, a, dim=-1), torch.nn.functional.cosine_similarity(U, b, dim=-1), atol=1e-15)


def _write_patterns(root, speakers=4, utterances=4, mel=12, seed=0, lengths=(9, 30)):
    """A synthetic pattern directory written with the project's own writers (`pattern_generator._write`, `data.write_metadata`)."""
    from glow_tts_amd import data, pattern_generator
    rng = np.random.default_rng(seed)
    for s in range(speakers):
        for u in range(utterances):
            T = int(rng.integers(*lengths))
            item = {"path": "/corpus/S{}/u{}.wav".format(s, u), "dataset": "SYN", "speaker": "SYN.S{}".format(s), "speaker_id": s}
            item["file"] = pattern_generator.pattern_file(item)
            m = (rng.normal(0, 1.0, (T, mel)) + s).clip(-4, 4).astype(np.float32)
            pattern_generator._write(root, item, np.zeros(T * 4, np.float32), m, rng.random(T).astype(np.float32), False)
    return data.write_metadata(root, "METADATA.PICKLE", use_text=False)


def test_sampler_draws_speaker_major_batches_and_repeats(tmp_path):
    from glow_tts_amd.ge2e_trainer import Sampler
    root = str(tmp_path)
    meta = _write_patterns(root)
    extra = {"path": "/corpus/S9/u0.wav", "dataset": "SYN", "speaker": "SYN.S9", "speaker_id": 9}      # a speaker with one utterance: never drawn
    from glow_tts_amd import data, pattern_generator
    extra["file"] = pattern_generator.pattern_file(extra)
    pattern_generator._write(root, extra, np.zeros(80, np.float32), np.zeros((20, 12), np.float32), np.zeros(20, np.float32), False)
    meta = data.write_metadata(root, "METADATA.PICKLE", use_text=False)
    assert len(meta["File_List_by_Speaker_Dict"]) == 5
    a, b = Sampler(root, "METADATA.PICKLE", 3, 2, 5, 7, seed=4), Sampler(root, "METADATA.PICKLE", 3, 2, 5, 7, seed=4)
    other = Sampler(root, "METADATA.PICKLE", 3, 2, 5, 7, seed=5)
    seen_T = set()
    for step in range(12):
        T, rows = a.plan(step)
        seen_T.add(T)
        assert 5 <= T <= 7 and len(rows) == 6
        spk = [r[0] for r in rows]
        assert spk[0::2] == spk[1::2] and len(set(spk)) == 3 and "SYN.S9" not in spk          # speaker-major, distinct speakers, enough material
        for s, f, o in rows:
            assert f in meta["File_List_by_Speaker_Dict"][s] and 0 <= o <= meta["Mel_Length_Dict"][f] - T
        assert len({f for _, f, _ in rows}) == 6                                               # distinct utterances
        x = a.batch(step)
        assert x.shape == (6, 12, T) and x.dtype == torch.float32 and torch.equal(x, b.batch(step))
        with open(os.path.join(root, rows[3][1]), "rb") as fh:
            assert np.array_equal(x[3].numpy(), pickle.load(fh)["Mel"][rows[3][2]:rows[3][2] + T].T)
    assert seen_T == {5, 6, 7}
    assert any(a.plan(s) != other.plan(s) for s in range(4))
    with pytest.raises(ValueError, match="Speaker_Embedding.GE2E.Train.Speakers"):
        Sampler(root, "METADATA.PICKLE", 5, 2, 5, 7)                                           # only four speakers have two utterances


def test_equal_error_rate_on_hand_made_scores():
    from glow_tts_amd.ge2e_trainer import equal_error_rate
    assert equal_error_rate([0.9, 0.8, 0.2, 0.1], [True, True, False, False]) == 0.0           # separable
    assert equal_error_rate([0.1, 0.2, 0.8, 0.9], [True, True, False, False]) == 1.0           # inverted
    # targets 0.9 0.8 0.6, non-targets 0.7 0.3 0.2: at the threshold 0.7 one of three non-targets passes and one of three targets fails
    assert abs(equal_error_rate([0.9, 0.8, 0.7, 0.3, 0.2, 0.6], [1, 1, 0, 0, 0, 1]) - 1 / 3) < 1e-12
    assert abs(equal_error_rate([4, 3, 2, 1], [True, False, True, False]) - 0.5) < 1e-12
    with pytest.raises(ValueError):
        equal_error_rate([0.5, 0.6], [True, True])


def test_checkpoint_layout_round_trips_through_ge2e_load(tmp_path):
    from glow_tts_amd.speaker_encoder import ge2e_load
    sizes = R.sizes_of(12, 16, 2, 16)
    sd = R.random_state_dict(sizes, 3)
    path = str(tmp_path / "GE2E_3.pt")
    torch.save({"Model": sd, "Loss": {"w": torch.tensor(9.5)}, "Optimizer": {"state": {}, "param_groups": []}, "Steps": 3}, path)
    got = ge2e_load(torch.load(path, map_location="cpu"), sizes)
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="surplus key 'w'"):                                    # the loss's scale lives outside 'Model'
        ge2e_load({"Model": dict(sd, w=torch.tensor(9.5))}, sizes)


def test_yaml_defaults_apply_when_the_block_is_absent():
    from glow_tts_amd.ge2e_trainer import DEFAULTS, train_settings
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("SE")
    assert "Train" not in d["Speaker_Embedding"]["GE2E"]                                        # the shipped yaml: the block is a comment
    assert train_settings(Recursive_Parse(copy.deepcopy(d))) == DEFAULTS
    assert DEFAULTS == {"Speakers": 64, "Utterances": 10, "Slice_Length": {"Min": 140, "Max": 180}, "Learning_Rate": 1.0e-3, "Gradient_Norm": 3.0,
                        "Projection_Grad_Scale": 0.5, "Similarity_Grad_Scale": 0.01, "Max_Step": 1000000, "Checkpoint_Save_Interval": 5000,
                        "Evaluation_Interval": 1000, "Checkpoint_Path": "./ge2e_results"}
    d["Speaker_Embedding"]["GE2E"]["Train"] = {"Speakers": 3, "Slice_Length": {"Min": 5}}
    s = train_settings(Recursive_Parse(copy.deepcopy(d)))
    assert s["Speakers"] == 3 and s["Utterances"] == 10 and s["Slice_Length"] == {"Min": 5, "Max": 180}
    text = open(os.path.join(REPO, "glow_tts_amd", "Hyper_Parameters.default.yaml")).read()
    for k, v in DEFAULTS.items():
        assert "#     {}:".format(k) in text, k
    for bad, key in (({"Speakers": 1}, "Train.Speakers"), ({"Utterances": 1}, "Train.Utterances"), ({"Slice_Length": {"Min": 9, "Max": 3}}, "Train.Slice_Length"),
                     ({"Learning_Rate": 0}, "Train.Learning_Rate"), ({"Speaker": 3}, "Train.Speaker"),
                     ({"Learning_Rate": "fast"}, r"Speaker_Embedding\.GE2E\.Train\.Learning_Rate = fast"),             # a wrongly typed value is a bad value
                     ({"Slice_Length": {"Bogus": 1}}, r"unknown key Speaker_Embedding\.GE2E\.Train\.Slice_Length\.Bogus")):
        d["Speaker_Embedding"]["GE2E"]["Train"] = bad
        with pytest.raises(ValueError, match=key):
            train_settings(Recursive_Parse(copy.deepcopy(d)))


def test_abi_additions_and_host_side_queries():
    from glow_tts_amd import _lib, abi
    names = [n for n in abi.SIGNATURES if n.startswith("glowtts_ge2e_train_")]
    assert len(names) == 9 and abi.ABI_VERSION == 7
    header = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    assert all(n + "(" in header for n in names)
    L = _lib.lib()
    assert L.glowtts_ge2e_train_image_floats(256, 3) == (8 * 3 - 4) * 256 * 256 and L.glowtts_ge2e_train_image_floats(250, 3) == -1
    assert L.glowtts_ge2e_train_keep_floats(640, 160, 256, 3) == 6 * 3 * 640 * 160 * 256
    assert L.glowtts_ge2e_train_loss_work_floats(640, 64, 256) == 640 * 256 + 2 * 64 * 256 + 2 * 640 * 64 + 3 * 640 + 64
    assert L.glowtts_ge2e_train_work_floats(640, 160, 80, 256, 3) == 8 * 1024 * 513 and L.glowtts_ge2e_train_work_floats(4, 1, 4, 16, 1) == 64 * 33
    assert L.glowtts_ge2e_train_work_floats(1 << 20, 1 << 12, 80, 256, 3) == -1                  # N T >= 2^31
