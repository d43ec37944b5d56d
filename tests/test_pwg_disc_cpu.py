"""CPU: the Parallel WaveGAN discriminator's host side - the yaml block `Vocoder.Train.Discriminator`, the state-dict contract (shapes, seeded init, weight-norm
fold, nesting, named errors), geometry errors before the device, and the kernels' form of the backward (tests/pwg_disc_ref.py) against autograd at 1e-10.
The signature-table entries of the new `glowtts_pwg_disc_*` entry points are compared with the header by tests/test_abi.py (it walks every prototype of the
header and every entry of the table), so nothing here repeats that."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pwg_disc_ref as DR  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402

KEY = "Vocoder.Train.Discriminator"


def hp_of(block=None, train=None):
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Sound"]["Frame_Shift"] = 256
    d["Vocoder"] = {"Type": "PWG", "Train": dict(train or {})}
    if block is not None:
        d["Vocoder"]["Train"]["Discriminator"] = block
    return Recursive_Parse(copy.deepcopy(d))


def test_block_defaults_and_absent_block():
    from glow_tts_amd.pwg_trainer import DEFAULTS, train_settings
    from glow_tts_amd.vocoder import DISC_DEFAULTS, pwg_disc_settings
    assert DISC_DEFAULTS == {"Start_Step": 100000, "Lambda_Adversarial": 4.0, "Learning_Rate": 5.0e-5, "Epsilon": 1.0e-6, "Gradient_Norm": 1.0,
                             "Learning_Rate_Decay": {"Step": 200000, "Gamma": 0.5}, "Layers": 10, "Channels": 64, "Negative_Slope": 0.2}
    s = train_settings(hp_of({}))
    assert s["Discriminator"] == DISC_DEFAULTS
    s = train_settings(hp_of({"Start_Step": 7, "Learning_Rate_Decay": {"Gamma": 0.25}}))
    assert s["Discriminator"]["Start_Step"] == 7 and s["Discriminator"]["Learning_Rate_Decay"] == {"Step": 200000, "Gamma": 0.25}
    assert s["Discriminator"]["Channels"] == 64
    # block absent: today's result, key for key
    absent = train_settings(hp_of(None))
    assert set(absent) == set(DEFAULTS) and "Discriminator" not in absent and pwg_disc_settings(hp_of(None)) is None
    for k, v in DEFAULTS.items():
        if k != "STFT_Resolutions":
            assert absent[k] == v, k
    assert absent["STFT_Resolutions"] == [tuple(r) for r in DEFAULTS["STFT_Resolutions"]]


BAD = [("Start_Step", -1), ("Start_Step", 1.5), ("Lambda_Adversarial", -0.5), ("Learning_Rate", 0), ("Epsilon", -1.0), ("Gradient_Norm", 0.0),
       ("Learning_Rate_Decay", {"Step": 0}), ("Learning_Rate_Decay", {"Gamma": 1.5}), ("Layers", 2), ("Layers", 17), ("Channels", 24), ("Channels", 0),
       ("Channels", 224), ("Negative_Slope", 1.0), ("Negative_Slope", -0.1), ("Learning_Rate", "fast")]


@pytest.mark.parametrize("key, value", BAD)
def test_every_bad_key_is_named(key, value):
    from glow_tts_amd.pwg_trainer import train_settings
    with pytest.raises(ValueError, match="{}.{}".format(KEY, key).replace(".", r"\.")):
        train_settings(hp_of({key: value}))


def test_unknown_keys_are_named():
    from glow_tts_amd.pwg_trainer import train_settings
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Discriminator\.Bogus"):
        train_settings(hp_of({"Bogus": 1}))
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Discriminator\.Learning_Rate_Decay\.Bogus"):
        train_settings(hp_of({"Learning_Rate_Decay": {"Bogus": 1}}))
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Bogus"):                       # the outer block's own check is as before
        train_settings(hp_of(None, train={"Bogus": 1}))


def test_geometry_and_the_largest_channels():
    from glow_tts_amd.vocoder import pwg_disc_geometry, pwg_disc_lds, pwg_disc_max_channels
    g = pwg_disc_geometry(hp_of(None))
    assert g == {"layers": 10, "C": 64, "slope": 0.2, "dilations": [1, 1, 2, 3, 4, 5, 6, 7, 8, 1]}
    assert pwg_disc_geometry(hp_of({"Layers": 3, "Channels": 16}))["dilations"] == [1, 1, 1]
    assert pwg_disc_lds(64) == 64 * (192 + 4) * 4                                                   # 49 KB at the defaults
    assert pwg_disc_max_channels() == 208 and pwg_disc_lds(208) <= 160 * 1024 < pwg_disc_lds(224)
    assert pwg_disc_geometry(hp_of({"Channels": 208}))["C"] == 208


def test_geometry_errors_come_before_the_device(monkeypatch):
    from glow_tts_amd import _lib
    from glow_tts_amd.vocoder import PWGDiscriminator

    def no_device(*a, **k):
        raise AssertionError("the library was loaded before the geometry was checked")
    monkeypatch.setattr(_lib, "lib", no_device)
    for block, key in (({"Channels": 24}, "Channels"), ({"Layers": 2}, "Layers"), ({"Negative_Slope": 2.0}, "Negative_Slope"), ({"Bogus": 0}, "Bogus")):
        with pytest.raises(ValueError, match=r"Vocoder\.Train\.Discriminator\." + key):
            PWGDiscriminator(hp_of(block), "cuda:0")


def test_shapes_init_and_reference_agree():
    from glow_tts_amd.vocoder import pwg_disc_expected_shapes, pwg_disc_geometry, pwg_disc_init
    for layers, C in ((10, 64), (4, 16), (3, 32)):
        geo = pwg_disc_geometry(hp_of({"Layers": layers, "Channels": C}))
        want = pwg_disc_expected_shapes(geo)
        assert want == DR.shapes(layers, C) and list(want) == list(DR.shapes(layers, C))
        assert want["conv_layers.0.weight"] == (C, 1, 3) and want["conv_layers.{}.weight".format(layers - 1)] == (1, C, 3)
        a, b, c = pwg_disc_init(geo, 3), pwg_disc_init(geo, 3), pwg_disc_init(geo, 4)
        assert all(torch.equal(a[k], b[k]) for k in want) and not torch.equal(a["conv_layers.1.weight"], c["conv_layers.1.weight"])
        ref = DR.random_state_dict(layers, C, 3)                                                   # the same rule, drawn in the same order
        assert all(torch.equal(a[k], ref[k]) and tuple(a[k].shape) == want[k] and a[k].dtype == torch.float32 for k in want)
        bound = 1.0 / np.sqrt(3 * C)
        assert float(a["conv_layers.1.weight"].abs().max()) <= bound and float(a["conv_layers.1.bias"].abs().max()) <= bound
        assert float(a["conv_layers.0.bias"].abs().max()) <= 1.0 / np.sqrt(3) and float(a["conv_layers.0.weight"].abs().max()) > bound


def test_load_folds_weight_norm_and_finds_nested_dicts():
    from glow_tts_amd.vocoder import pwg_disc_geometry, pwg_disc_init, pwg_disc_load
    geo = pwg_disc_geometry(hp_of({"Layers": 4, "Channels": 16}))
    sd = pwg_disc_init(geo, 0)
    for nest in (lambda d: d, lambda d: {"discriminator": d}, lambda d: {"Discriminator": d}, lambda d: {"model": {"discriminator": d}},
                 lambda d: {"generator": {"first_conv.weight": torch.zeros(1)}, "discriminator": d, "Steps": 3}):
        got = pwg_disc_load(nest(dict(sd)), geo)
        assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    wn = dict(sd)
    w = wn.pop("conv_layers.2.weight").double()
    v = w * 1.7
    wn["conv_layers.2.weight_v"], wn["conv_layers.2.weight_g"] = v.float(), w.reshape(16, -1).norm(dim=1).reshape(16, 1, 1).float()
    got = pwg_disc_load(wn, geo)
    assert (got["conv_layers.2.weight"].double() - w).abs().max() < 1e-6 * w.abs().max()
    with pytest.raises(ValueError, match=r"conv_layers\.2\.weight_g has no"):
        pwg_disc_load({k: t for k, t in wn.items() if not k.endswith("weight_v")}, geo)
    with pytest.raises(ValueError, match=r"conv_layers\.2\.weight is given both"):
        pwg_disc_load(dict(wn, **{"conv_layers.2.weight": sd["conv_layers.2.weight"]}), geo)
    with pytest.raises(ValueError, match=r"missing key conv_layers\.3\.bias"):
        pwg_disc_load({k: t for k, t in sd.items() if k != "conv_layers.3.bias"}, geo)
    with pytest.raises(ValueError, match=r"surplus key conv_layers\.4\.weight"):
        pwg_disc_load(dict(sd, **{"conv_layers.4.weight": torch.zeros(1, 16, 3)}), geo)
    with pytest.raises(ValueError, match=r"conv_layers\.1\.weight has shape \(16, 16, 5\)"):
        pwg_disc_load(dict(sd, **{"conv_layers.1.weight": torch.zeros(16, 16, 5)}), geo)
    with pytest.raises(ValueError, match="no Parallel WaveGAN discriminator"):
        pwg_disc_load({"generator": {"first_conv.weight": torch.zeros(1)}}, geo)


def test_generator_is_still_found_beside_a_discriminator():
    """A six-key checkpoint of the adversarial trainer loads into the frozen vocoder: `pwg_load` finds the generator, `pwg_disc_load` the discriminator."""
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.vocoder import pwg_disc_geometry, pwg_disc_init, pwg_disc_load, pwg_geometry, pwg_init, pwg_load
    d = tiny_hp_dict("Vanilla")
    d["Sound"]["Frame_Shift"] = 15
    d["Vocoder"] = {"Type": "PWG", "Layers": 4, "Stacks": 2, "Residual_Channels": 16, "Gate_Channels": 32, "Skip_Channels": 16, "Upsample_Scales": [3, 5],
                    "Train": {"Discriminator": {"Layers": 4, "Channels": 16}}}
    hp = Recursive_Parse(d)
    geo, dgeo = pwg_geometry(hp), pwg_disc_geometry(hp)
    gen, disc = pwg_init(geo, 1), pwg_disc_init(dgeo, 1)
    state = {"generator": gen, "Optimizer": {}, "Steps": 2, "discriminator": disc, "Discriminator_Optimizer": {}, "Discriminator_Steps": 1}
    got = pwg_load(state, geo)
    assert all(torch.equal(got[k], gen[k]) for k in gen)
    got = pwg_disc_load(state, dgeo)
    assert all(torch.equal(got[k], disc[k]) for k in disc)


# ---- the kernels' form of the backward against autograd ----------------------------------------------------------------------------------------
def form_case(layers, C, T, seed):
    sd = DR.random_state_dict(layers, C, seed, scale=3.0)
    g = torch.Generator().manual_seed(seed + 1)
    wav, dsc = (torch.randn(1, T, generator=g) * 0.3).double(), torch.randn(1, T, generator=g).double()
    ref = DR.functional_grads(sd, wav, dsc)
    sdn = {k: v.double().numpy() for k, v in sd.items()}
    return sdn, wav[0].numpy(), dsc[0].numpy(), ref


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("layers, C, T", [(10, 16, 105), (4, 16, 5), (3, 16, 1), (6, 32, 70)])
def test_kernel_form_matches_autograd(layers, C, T):
    sdn, wav, dsc, ref = form_case(layers, C, T, 11)
    scores, dwav, grads = DR.kernel_form_backward(sdn, wav, dsc)
    assert rel(scores, ref["scores"][0].numpy()) < 1e-10 and rel(dwav, ref["dwav"][0].numpy()) < 1e-10
    assert set(grads) == set(ref["grads"])
    for k, g in grads.items():
        assert g.shape == tuple(ref["grads"][k].shape) and rel(g, ref["grads"][k].numpy()) < 1e-10, k


@pytest.mark.parametrize("switch", ["mask_from_input", "same_side_gather"])
def test_each_broken_form_is_rejected(switch):
    sdn, wav, dsc, ref = form_case(6, 16, 70, 12)
    _, dwav, grads = DR.kernel_form_backward(sdn, wav, dsc, **{switch: True})
    assert rel(dwav, ref["dwav"][0].numpy()) > 1e-3
    assert max(rel(g, ref["grads"][k].numpy()) for k, g in grads.items()) > 1e-3


def test_losses_of_the_reference():
    p, q = torch.tensor([[0.5, 1.5], [1.0, 0.0]], dtype=torch.float64), torch.tensor([[0.5, -0.5], [0.0, 1.0]], dtype=torch.float64)
    assert float(DR.adversarial_loss(p)) == pytest.approx((0.25 + 0.25 + 0 + 1) / 4)
    assert float(DR.discriminator_loss(p, q)) == pytest.approx((0.25 + 0.25 + 0 + 1) / 4 + (0.25 + 0.25 + 0 + 1) / 4)
