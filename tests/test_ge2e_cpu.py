"""CPU suite of the GE2E speaker encoder: the checkpoint loader (three places, every bad key named), the size checks (yaml keys named), the C-ABI additions
(header and table, version 7), seeded slice selection, the --convert list's speaker column and GlowTTS checkpoints that carry `layer_Dict.GE2E.*`."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import ge2e_ref as R  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402

SIZES = R.sizes_of(12, 16, 2, 16)


def test_reference_guards_hold_for_the_reference_alone():
    """The bar's guards (0 < e32 < 1e-3, max |ref64| > 1e-3) on the smallest and on a saturating case, hidden states included; unit-norm d-vectors."""
    for (B, S, T, Mel, H, Stacks, E, scale) in [(1, 1, 1, 4, 16, 1, 8, 1), (3, 2, 7, 20, 48, 3, 24, 3)]:
        sizes = R.sizes_of(Mel, H, Stacks, E)
        sd = R.random_state_dict(sizes, 4321, scale)
        x = R.uniform_input(B * S, Mel, T, 99)
        r64, r32 = R.forward(sd, sizes, x, S), R.forward(sd, sizes, x, S, torch.float32)
        assert r64[0].shape == (Stacks, B * S, T, H) and r64[1].shape == (B * S, E) and r64[2].shape == (B, E)
        for a, b in zip(r64, r32):
            _, e32, scale_ = R.errors(b, a, b)
            assert 0 < e32 < 1e-3 and scale_ > 1e-3
        assert (r64[2].norm(dim=1) - 1).abs().max() < 1e-12
    before = torch.random.get_rng_state()
    R.random_state_dict(SIZES, 1)
    assert torch.equal(before, torch.random.get_rng_state())                 # the global generator is left alone


def test_loader_finds_the_dict_at_all_three_places():
    from glow_tts_amd.speaker_encoder import GLOWTTS_PREFIX, ge2e_find_state_dict, ge2e_load, ge2e_shapes
    sd = R.random_state_dict(SIZES, 3)
    assert set(sd) == set(ge2e_shapes(SIZES)) and all(tuple(sd[k].shape) == s for k, s in ge2e_shapes(SIZES).items())
    glow = {"layer_Dict.Encoder.x": torch.zeros(2)}
    glow.update({GLOWTTS_PREFIX + k: v for k, v in sd.items()})
    for obj in (sd, {"Model": sd, "Steps": 7}, {"Model": glow, "Steps": 7, "Optimizer": {}}, glow):
        got = ge2e_load(obj, SIZES)
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert ge2e_find_state_dict({"Model": {"layer_Dict.Encoder.x": torch.zeros(2)}}) is None and ge2e_find_state_dict(3) is None
    with pytest.raises(ValueError, match="no GE2E speaker encoder"):
        ge2e_load({"Model": {"layer_Dict.Encoder.x": torch.zeros(2)}}, SIZES)


def test_every_missing_surplus_or_misshaped_key_is_named():
    from glow_tts_amd.speaker_encoder import GLOWTTS_PREFIX, ge2e_load
    sd = R.random_state_dict(SIZES, 3)
    for k in sd:
        with pytest.raises(ValueError, match="missing key '{}'".format(re.escape(k))):
            ge2e_load({q: v for q, v in sd.items() if q != k}, SIZES)
        bad = dict(sd)
        bad[k] = torch.zeros(*[n + 1 for n in sd[k].shape])
        with pytest.raises(ValueError, match="key '{}' has shape".format(re.escape(k))):
            ge2e_load({"Model": bad}, SIZES)
    for extra in ("lstm.weight_ih_l2", "linear.scale", "similarity.w"):
        with pytest.raises(ValueError, match="surplus key '{}'".format(re.escape(extra))):
            ge2e_load(dict(sd, **{extra: torch.zeros(1)}), SIZES)
    pre = {GLOWTTS_PREFIX + k: v for k, v in sd.items()}
    with pytest.raises(ValueError, match="surplus key 'similarity.w'"):
        ge2e_load({"Model": dict(pre, **{GLOWTTS_PREFIX + "similarity.w": torch.zeros(1)})}, SIZES)
    with pytest.raises(ValueError, match="Speaker_Embedding.GE2E.LSTM.Sizes = 32"):      # another width: the first mis-shaped key, with the sizes asked for
        ge2e_load(sd, dict(SIZES, H=32))


def test_every_unsupported_size_names_its_yaml_keys():
    from glow_tts_amd import abi
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.speaker_encoder import GE2E, ge2e_check_sizes, ge2e_sizes
    ge2e_check_sizes(R.sizes_of(80, 256, 3, 256))
    ge2e_check_sizes(R.sizes_of(4, 16, 1, 1))
    ge2e_check_sizes(R.sizes_of(80, 768, 8, 256))
    assert abi.GE2E_MAX_H >= 768 and abi.GE2E_MAX_E >= 256 and abi.GE2E_MAX_STACKS == 8
    for change, key in ((dict(Mel=82), "Sound.Mel_Dim"), (dict(Mel=0), "Sound.Mel_Dim"), (dict(H=250), "Speaker_Embedding.GE2E.LSTM.Sizes"),
                        (dict(H=abi.GE2E_MAX_H + 16), "Speaker_Embedding.GE2E.LSTM.Sizes"), (dict(Stacks=0), "Speaker_Embedding.GE2E.LSTM.Stacks"),
                        (dict(Stacks=9), "Speaker_Embedding.GE2E.LSTM.Stacks"), (dict(E=0), "Speaker_Embedding.Embedding_Size"),
                        (dict(E=abi.GE2E_MAX_E + 1), "Speaker_Embedding.Embedding_Size")):
        with pytest.raises(ValueError, match=re.escape(key)):
            ge2e_check_sizes(dict(R.sizes_of(80, 256, 3, 256), **change))
    hp = tiny_hp_dict("SE")
    hp["Speaker_Embedding"]["GE2E"]["LSTM"] = {"Sizes": 250, "Stacks": 9}
    assert ge2e_sizes(Recursive_Parse(hp)) == {"Mel": 12, "H": 250, "Stacks": 9, "E": 16}
    with pytest.raises(ValueError, match=r"LSTM\.Sizes.*LSTM\.Stacks"):      # at construction, before any device is touched
        GE2E(Recursive_Parse(hp), "cuda:0")


def test_the_library_agrees_with_the_python_size_check():
    from glow_tts_amd import _lib
    from glow_tts_amd.speaker_encoder import ge2e_check_sizes
    L = _lib.lib()                                                            # host-side queries: no GPU needed
    for Mel, H, Stacks, E in [(80, 256, 3, 256), (4, 16, 1, 1), (80, 768, 8, 1024), (512, 768, 8, 256), (82, 256, 3, 256), (80, 250, 3, 256), (80, 784, 3, 256),
                              (80, 256, 0, 256), (80, 256, 9, 256), (80, 256, 3, 0), (80, 256, 3, 1025), (516, 256, 3, 256)]:
        try:
            ge2e_check_sizes(R.sizes_of(Mel, H, Stacks, E))
            ok = 1
        except ValueError:
            ok = 0
        assert L.glowtts_ge2e_supported(Mel, H, Stacks, E) == ok, (Mel, H, Stacks, E)
    assert L.glowtts_ge2e_image_floats(80, 256, 3) == (336 + 512 + 512) * 1024 and L.glowtts_ge2e_image_floats(80, 250, 3) == -1
    assert L.glowtts_ge2e_work_floats(160, 64, 256, 3) == 3 * 160 * 256 * 65


def test_abi_additions_are_in_the_header_and_the_table_at_version_7():
    from glow_tts_amd import abi
    text = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    for name in ("glowtts_ge2e_supported", "glowtts_ge2e_image_floats", "glowtts_ge2e_work_floats", "glowtts_ge2e_pack", "glowtts_ge2e_forward"):
        assert name in abi.SIGNATURES and re.search(r"\b{}\s*\(".format(name), text), name
    assert abi.ABI_VERSION == 7 and re.search(r"#define\s+GLOWTTS_ABI_VERSION\s+7\b", text)
    restype, argtypes = abi.SIGNATURES["glowtts_ge2e_forward"]
    assert restype is abi.I and argtypes == [abi.P] * 9 + [abi.I] * 7 + [abi.P]


def test_seeded_slice_selection_repeats():
    from glow_tts_amd import data
    from glow_tts_amd.inferencer import utterance_seed_words
    mel = np.random.default_rng(0).normal(size=(500, 12)).astype(np.float32)
    word = utterance_seed_words(11, "Alpha")[0]
    a = data.mels_for_ge2e([mel], 3, 16, 8, rng=np.random.RandomState(word))
    b = data.mels_for_ge2e([mel], 3, 16, 8, rng=np.random.RandomState(word))
    c = data.mels_for_ge2e([mel], 3, 16, 8, rng=np.random.RandomState(utterance_seed_words(12, "Alpha")[0]))
    assert a.shape == (3, 16, 12) and np.array_equal(a, b) and not np.array_equal(a, c)
    exact = mel[:3 * 8 + 8]                                                   # Slice-exact: no offset to draw
    assert np.array_equal(data.mels_for_ge2e([exact], 3, 16, 8, rng=None)[1], exact[8:24])


def test_read_convert_list_keeps_integers_and_returns_strings_for_paths(tmp_path):
    from glow_tts_amd.inferencer import read_convert_list
    p = tmp_path / "list.tsv"
    p.write_text("Label\tSource\tSource_Speaker\tTarget_Speaker\tReference\n"
                 "a\tsrc.npy\t3\t-1\n"
                 "b\tsrc.wav\tspk/one.wav\tspk/two.npy\tref.npy\n"
                 "c\tsrc.npy\t\t 07 \t\n")
    recs = read_convert_list(str(p))
    assert [(r["source_speaker"], r["target_speaker"]) for r in recs] == [(3, -1), ("spk/one.wav", "spk/two.npy"), (None, 7)]
    assert all(type(r["source_speaker"]) is int for r in recs[:1]) and recs[1]["target_reference"] == "ref.npy" and recs[2]["target_reference"] is None


def test_glowtts_checkpoint_with_ge2e_keys_still_loads():
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    from glow_tts_amd.speaker_encoder import GLOWTTS_PREFIX, ge2e_load, ge2e_sizes
    d = tiny_hp_dict("SE")
    d["Speaker_Embedding"]["Type"] = "GE2E"
    d["Speaker_Embedding"]["GE2E"]["LSTM"] = {"Sizes": 16, "Stacks": 2}
    hp = Recursive_Parse(d)
    m = GlowTTS(hp)
    sd = dict(m.state_dict())
    enc = R.random_state_dict(ge2e_sizes(hp), 5)
    sd.update({GLOWTTS_PREFIX + k: v for k, v in enc.items()})
    GlowTTS(hp).load_state_dict(sd, strict=True)                             # the encoder's keys do not fail the strict load
    assert any(k.startswith(GLOWTTS_PREFIX) for k in sd)                     # ... and the caller's dict is left whole for the Inferencer to read them
    got = ge2e_load({"Model": sd}, ge2e_sizes(hp))
    assert all(torch.equal(got[k], enc[k]) for k in enc)
