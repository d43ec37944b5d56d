"""CPU: the HiFi-GAN multi-period discriminator's host side - the yaml block `Vocoder.Train.Adversarial`, the state-dict contract (shapes, seeded init,
weight-norm fold on 4-D tensors, nesting, named errors), geometry errors before the device, the kernels' form of the backward
(tests/hifigan_disc_ref.py) against autograd at 1e-10, hand-computed losses, and that the reference alone holds the guards of the GPU tests' bar at their
cases.  The signature-table entries of the `glowtts_hifigan_disc_*` entry points are compared with the header by tests/test_abi.py."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hifigan_disc_ref as HR  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402

KEY = "Vocoder.Train.Adversarial"


def hp_of(block=None, train=None, kind="HiFiGAN"):
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Vocoder"] = {"Type": kind, "Train": dict(train or {})}
    if block is not None:
        d["Vocoder"]["Train"]["Adversarial"] = block
    return Recursive_Parse(copy.deepcopy(d))


def test_block_defaults_and_absent_block():
    from glow_tts_amd.vocoder import MPD_DEFAULTS, hifigan_disc_geometry, hifigan_disc_settings
    assert MPD_DEFAULTS == {"Start_Step": 0, "Lambda_Adversarial": 1.0, "Lambda_Feature_Matching": 2.0, "Learning_Rate": 2.0e-4, "Epsilon": 1.0e-6,
                            "Gradient_Norm": 10.0, "Learning_Rate_Decay": {"Step": 200000, "Gamma": 0.5}, "Periods": [2, 3, 5, 7, 11],
                            "Channels": [32, 128, 512, 1024, 1024], "Negative_Slope": 0.1}
    assert hifigan_disc_settings(hp_of(None)) is None
    assert hifigan_disc_settings(hp_of({})) == MPD_DEFAULTS
    s = hifigan_disc_settings(hp_of({"Start_Step": 7, "Learning_Rate_Decay": {"Gamma": 0.25}, "Periods": [3, 2]}))
    assert s["Start_Step"] == 7 and s["Learning_Rate_Decay"] == {"Step": 200000, "Gamma": 0.25} and s["Periods"] == [3, 2] and s["Channels"] == MPD_DEFAULTS["Channels"]
    assert hifigan_disc_geometry(hp_of(None)) == {"periods": [2, 3, 5, 7, 11], "channels": [32, 128, 512, 1024, 1024], "strides": [3, 3, 3, 3, 1], "slope": 0.1}
    assert hifigan_disc_geometry(hp_of({"Channels": [16, 1024]}))["strides"] == [3, 1]


def test_the_trainer_reads_the_block_and_an_absent_block_changes_nothing():
    from glow_tts_amd import hifigan_trainer as T
    from glow_tts_amd import pwg_trainer
    from glow_tts_amd.vocoder import MPD_DEFAULTS
    absent = T.train_settings(hp_of(None))
    assert set(absent) == set(T.DEFAULTS) and "Adversarial" not in absent and "Discriminator" not in absent       # today's result, key for key
    for k, v in T.DEFAULTS.items():
        if k != "STFT_Resolutions":
            assert absent[k] == v, k
    assert absent["STFT_Resolutions"] == [tuple(r) for r in T.DEFAULTS["STFT_Resolutions"]]
    assert T.DEFAULTS == dict(pwg_trainer.DEFAULTS, Batch_Size=16, Segment_Frames=32, Learning_Rate=2.0e-4, Checkpoint_Path="./hifigan_results")
    s = T.train_settings(hp_of({}))
    assert s["Adversarial"] == MPD_DEFAULTS and {k: v for k, v in s.items() if k != "Adversarial"} == absent
    s = T.train_settings(hp_of({"Start_Step": 7, "Periods": [3, 2]}, train={"Batch_Size": 4}))
    assert s["Adversarial"]["Start_Step"] == 7 and s["Adversarial"]["Periods"] == [3, 2] and s["Batch_Size"] == 4
    assert T.HiFiGAN_Trainer.DISC_BLOCK == "Adversarial" and pwg_trainer.PWG_Trainer.DISC_BLOCK == "Discriminator"
    assert [b[4] for b in T.BUNDLES] == [("generator", "Optimizer", "Steps"), ("discriminator", "Discriminator_Optimizer", "Discriminator_Steps")]


@pytest.mark.parametrize("key, value", [("Periods", [1, 2]), ("Channels", [16, 24]), ("Start_Step", -1), ("Bogus", 1)])
def test_the_trainer_names_bad_keys_of_the_block(key, value):
    from glow_tts_amd import hifigan_trainer as T
    with pytest.raises(ValueError, match="{}.{}".format(KEY, key).replace(".", r"\.")):
        T.train_settings(hp_of({key: value}))


BAD = [("Start_Step", -1), ("Start_Step", 1.5), ("Lambda_Adversarial", -0.5), ("Lambda_Feature_Matching", -1), ("Learning_Rate", 0), ("Epsilon", -1.0),
       ("Gradient_Norm", 0.0), ("Learning_Rate_Decay", {"Step": 0}), ("Learning_Rate_Decay", {"Gamma": 1.5}), ("Periods", []), ("Periods", [1, 2]),
       ("Periods", [2, 17]), ("Periods", [2, 2]), ("Periods", [2.5]), ("Periods", list(range(2, 11))), ("Periods", 3), ("Channels", [16]), ("Channels", [16, 24]),
       ("Channels", [16, 1040]), ("Channels", [16] * 7), ("Channels", [0, 16]), ("Channels", 64), ("Negative_Slope", 1.0), ("Negative_Slope", -0.1),
       ("Learning_Rate", "fast")]


@pytest.mark.parametrize("key, value", BAD)
def test_every_bad_key_is_named(key, value):
    from glow_tts_amd.vocoder import hifigan_disc_settings
    with pytest.raises(ValueError, match="{}.{}".format(KEY, key).replace(".", r"\.")):
        hifigan_disc_settings(hp_of({key: value}))


def test_unknown_keys_are_named():
    from glow_tts_amd.vocoder import hifigan_disc_settings
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Adversarial\.Bogus"):
        hifigan_disc_settings(hp_of({"Bogus": 1}))
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Adversarial\.Learning_Rate_Decay\.Bogus"):
        hifigan_disc_settings(hp_of({"Learning_Rate_Decay": {"Bogus": 1}}))
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Adversarial\.Layers"):       # the Parallel WaveGAN discriminator's key
        hifigan_disc_settings(hp_of({"Layers": 10}))


def test_the_trainers_keys_are_as_before():
    """The HiFi-GAN trainer still refuses `Vocoder.Train.Discriminator`, and the Parallel WaveGAN trainer does not know `Adversarial`."""
    from glow_tts_amd import hifigan_trainer, pwg_trainer
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Vocoder"] = {"Type": "HiFiGAN", "Train": {"Discriminator": {}}}
    with pytest.raises(ValueError, match=r"Vocoder\.Train\.Discriminator.*Vocoder\.Train\.Adversarial"):     # refused, and pointed at the new key
        hifigan_trainer.train_settings(Recursive_Parse(copy.deepcopy(d)))
    d["Vocoder"] = {"Type": "PWG", "Train": {"Adversarial": {}}}
    d["Sound"]["Frame_Shift"] = 256
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Adversarial"):
        pwg_trainer.train_settings(Recursive_Parse(copy.deepcopy(d)))


def test_geometry_errors_come_before_the_device(monkeypatch):
    from glow_tts_amd import _lib
    from glow_tts_amd.vocoder import HiFiGANPeriodDiscriminator, hifigan_disc_geometry, hifigan_disc_rows

    def no_device(*a, **k):
        raise AssertionError("the library was loaded before the geometry was checked")
    monkeypatch.setattr(_lib, "lib", no_device)
    for block, key in (({"Channels": [16, 24]}, "Channels"), ({"Periods": [1]}, "Periods"), ({"Negative_Slope": 2.0}, "Negative_Slope"), ({"Bogus": 0}, "Bogus")):
        with pytest.raises(ValueError, match=r"Vocoder\.Train\.Adversarial\." + key):
            HiFiGANPeriodDiscriminator(hp_of(block), "cuda:0")
    geo = hifigan_disc_geometry(hp_of({"Periods": [2, 11]}))
    with pytest.raises(ValueError, match=r"Vocoder\.Train\.Adversarial\.Periods"):                  # T below 2 max(Periods)
        hifigan_disc_rows(geo, 21, 2)
    assert hifigan_disc_rows(geo, 22, 11) == [2, 1, 1, 1, 1, 1] and hifigan_disc_rows(geo, 8192, 2) == [4096, 1366, 456, 152, 51, 51]


def test_shapes_init_and_reference_agree():
    from glow_tts_amd.vocoder import hifigan_disc_expected_shapes, hifigan_disc_geometry, hifigan_disc_init
    for periods, channels in (([2, 3, 5, 7, 11], [32, 128, 512, 1024, 1024]), ([2, 3], [16, 32, 16]), ([16], [16, 16])):
        geo = hifigan_disc_geometry(hp_of({"Periods": periods, "Channels": channels}))
        want = hifigan_disc_expected_shapes(geo)
        assert want == HR.shapes(periods, channels) and list(want) == list(HR.shapes(periods, channels))
        assert want["discriminators.0.convs.0.weight"] == (channels[0], 1, 5, 1) and want["discriminators.0.convs.1.weight"] == (channels[1], channels[0], 5, 1)
        assert want[f"discriminators.{len(periods) - 1}.conv_post.weight"] == (1, channels[-1], 3, 1) and want["discriminators.0.conv_post.bias"] == (1,)
        if len(channels) > 3:
            continue                                                                                # (the default widths: the shapes alone)
        a, b, c = hifigan_disc_init(geo, 3), hifigan_disc_init(geo, 3), hifigan_disc_init(geo, 4)
        assert all(torch.equal(a[k], b[k]) for k in want) and not torch.equal(a["discriminators.0.convs.1.weight"], c["discriminators.0.convs.1.weight"])
        ref = HR.random_state_dict(periods, channels, 3)                                            # the same rule, drawn in the same order
        assert all(torch.equal(a[k], ref[k]) and tuple(a[k].shape) == want[k] and a[k].dtype == torch.float32 for k in want)
        bound = 1.0 / np.sqrt(5 * channels[0])                                                      # fan-in = Cin * 5
        assert float(a["discriminators.0.convs.1.weight"].abs().max()) <= bound and float(a["discriminators.0.convs.1.bias"].abs().max()) <= bound
        assert float(a["discriminators.0.convs.0.weight"].abs().max()) > bound


def test_load_folds_weight_norm_and_names_errors():
    from glow_tts_amd.vocoder import hifigan_disc_geometry, hifigan_disc_load, hifigan_find_state_dict, hifigan_load, pwg_disc_find_state_dict
    periods, channels = [2, 3], [16, 32, 16]
    geo = hifigan_disc_geometry(hp_of({"Periods": periods, "Channels": channels}))
    sd = HR.random_state_dict(periods, channels, 5)
    for nest in (lambda d: d, lambda d: {"discriminator": d}, lambda d: {"Discriminator": d}, lambda d: {"mpd": d}, lambda d: {"model": d},
                 lambda d: {"model": {"discriminator": d}}, lambda d: {"generator": {"conv_pre.weight": torch.zeros(1)}, "discriminator": d}):
        got = hifigan_disc_load(nest(dict(sd)), geo)
        assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    # weight norm on 4-D tensors: g [Cout, 1, 1, 1], v [Cout, Cin, k, 1]
    wn = {}
    for k, v in sd.items():
        if k.endswith(".weight"):
            norm = v.double().reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1, 1)
            wn[k + "_g"], wn[k + "_v"] = norm, v.double() * 2.5                                    # any positive multiple of the direction
        else:
            wn[k] = v
    got = hifigan_disc_load({"discriminator": wn}, geo)
    assert all(float((got[k].double() - sd[k].double()).abs().max()) <= 1e-6 * float(sd[k].abs().max()) for k in sd)
    # named errors
    k0 = "discriminators.1.convs.2.weight"
    with pytest.raises(ValueError, match="missing key " + k0.replace(".", r"\.")):
        hifigan_disc_load({k: v for k, v in sd.items() if k != k0}, geo)
    with pytest.raises(ValueError, match=r"surplus key discriminators\.2\.convs\.0\.weight"):
        hifigan_disc_load(dict(sd, **{"discriminators.2.convs.0.weight": torch.zeros(16, 1, 5, 1)}), geo)
    with pytest.raises(ValueError, match=k0.replace(".", r"\.") + r" has shape \(16, 32, 5\)"):
        hifigan_disc_load(dict(sd, **{k0: sd[k0][..., 0]}), geo)
    # neither a Parallel WaveGAN discriminator nor a generator is taken for it, and it is taken for neither
    with pytest.raises(ValueError, match="no HiFi-GAN multi-period discriminator"):
        hifigan_disc_load({"discriminator": {"conv_layers.0.weight": torch.zeros(16, 1, 3)}}, geo)
    with pytest.raises(ValueError, match="no HiFi-GAN multi-period discriminator"):
        hifigan_disc_load({"generator": {"conv_pre.weight": torch.zeros(1)}}, geo)
    with pytest.raises(ValueError, match="no Parallel WaveGAN discriminator"):
        pwg_disc_find_state_dict({"discriminator": sd})
    # the generator is still found beside a discriminator
    gen = {"conv_pre.weight": torch.zeros(1)}
    assert hifigan_find_state_dict({"generator": gen, "discriminator": sd}) is gen
    assert hifigan_find_state_dict({"model": {"generator": gen, "discriminator": sd}}) is gen
    # ... and loaded: a real tiny generator's state dict beside the discriminator, at the top level and inside `model`
    from glow_tts_amd.vocoder import hifigan_expected_shapes, hifigan_geometry, hifigan_init
    ggeo = hifigan_geometry(hp_of(None))
    gsd = hifigan_init(ggeo, 2)
    for obj in ({"generator": gsd, "discriminator": sd, "Steps": 3}, {"model": {"generator": gsd, "discriminator": sd}}):
        got = hifigan_load(obj, ggeo)
        assert list(got) == list(hifigan_expected_shapes(ggeo)) and all(torch.equal(got[k], gsd[k]) for k in gsd)
        assert all(torch.equal(v, sd[k]) for k, v in hifigan_disc_load(obj, geo).items())


FORM_CASES = [([16, 32, 16], 2, 50), ([16, 32, 16], 3, 50), ([16, 16], 7, 50), ([16, 32, 16], 5, 10), ([16, 32, 16, 16], 4, 91), ([16, 32], 5, 64)]


@pytest.mark.parametrize("channels, p, T", FORM_CASES)
def test_kernel_form_backward_matches_autograd(channels, p, T):
    """T mod p covers 0 (50 / 2, 10 / 5), 1 (50 / 7), p - 1 (50 / 3, 91 / 4, 64 / 5) and one in between"""
    n, slope, B = len(channels), 0.1, 2
    sd = HR.random_state_dict([p], channels, 11, 3.0)
    g = torch.Generator().manual_seed(2)
    wav = torch.randn(B, T, generator=g, dtype=torch.float64)
    ref = HR.score_grads(sd, wav, [p], n, slope, 1.0)
    dscores = (2.0 * (ref["scores"][0] - 1.0) / ref["scores"][0].numel()).numpy()
    dwav, grads = HR.kernel_form_backward(sd, 0, wav, p, n, slope, dscores)
    rel = lambda a, b: float(np.abs(a - b.numpy()).max() / np.abs(b.numpy()).max())
    assert rel(dwav, ref["dwav"]) < 1e-10
    assert set(grads) == set(ref["grads"])
    for k in grads:
        assert grads[k].shape == tuple(ref["grads"][k].shape) and rel(grads[k], ref["grads"][k]) < 1e-10, k
    for broken in HR.BROKEN:
        if broken == "fold" and T % p == 0:
            continue                                                                                # (no pad: nothing to fold)
        if broken == "wgrad_stride" and -(-T // p) <= 3:
            continue                                                                                # (one output row per layer: no stride to see)
        bw, bg = HR.kernel_form_backward(sd, 0, wav, p, n, slope, dscores, broken=broken)
        worst = max([rel(bw, ref["dwav"])] + [rel(bg[k], ref["grads"][k]) for k in bg])
        assert worst > 1e-3, (broken, worst)


def test_hand_computed_losses():
    """L_fm and both least-squares losses on numbers small enough to add by hand"""
    real_maps = [torch.tensor([[1.0, -2.0], [0.5, 0.0]]).reshape(1, 1, 2, 2), torch.tensor([3.0, 1.0]).reshape(1, 1, 1, 2)]
    fake_maps = [torch.tensor([[0.0, -1.0], [0.5, 2.0]]).reshape(1, 1, 2, 2), torch.tensor([1.0, 1.5]).reshape(1, 1, 1, 2)]
    terms = HR.feature_matching(real_maps, fake_maps)
    assert torch.allclose(terms, torch.tensor([(1.0 + 1.0 + 0.0 + 2.0) / 4, (2.0 + 0.5) / 2]))
    # a "network" whose score is known: all weights zero, conv_post's bias 0.25 -> every score 0.25
    periods, channels = [2, 3], [16, 16]
    sd = {k: torch.zeros(s) for k, s in HR.shapes(periods, channels).items()}
    for i in range(2):
        sd[f"discriminators.{i}.conv_post.bias"] += 0.25
    wav = torch.randn(2, 12, generator=torch.Generator().manual_seed(0))
    r = HR.pair_grads(sd, wav, wav + 1, periods, 2, 0.1)
    assert abs(float(r["loss"]) - 2 * (0.75 ** 2 + 0.25 ** 2)) < 1e-12                              # per period (0.25 - 1)^2 + 0.25^2
    g = HR.generator_term_grads(sd, wav, wav + 1, periods, 2, 0.1, 1.5, 2.0)
    assert abs(float(g["loss"]) - 1.5 * 2 * 0.75 ** 2) < 1e-12 and float(g["l_fm"]) == 0.0          # equal maps: no feature-matching term


def test_the_gpu_cases_hold_the_guards():
    """The float64 / float32 reference alone, at the weight scale and amplitude of tests/test_gpu_hifigan_disc.py, holds the guards of the bar for every
    tensor that file checks at every one of its cases: 0 < e32 < 1e-3 and max |ref64| > 1e-3."""
    import pwg_train_ref as TR
    import test_gpu_hifigan_disc as G
    worst = {}
    for case in G.CASES:
        r64, r32 = G.case_reference(case)
        named = [("loss", r64["loss"], r32["loss"]), ("dwav", r64["dwav"], r32["dwav"])]
        named += [(f"scores[{i}]", a, b) for i, (a, b) in enumerate(zip(r64["scores"], r32["scores"]))]
        named += [(f"map[{i}][{j}]", a, b) for i, (ma, mb) in enumerate(zip(r64["maps"], r32["maps"])) for j, (a, b) in enumerate(zip(ma, mb))]
        named += [(k, r64["grads"][k], r32["grads"][k]) for k in r64["grads"]]
        for name, a, b in named:
            _, e32, scale = TR.errors(a, a, b)
            assert 0 < e32 < 1e-3 and scale > 1e-3, (case, name, e32, scale)
            worst[case] = (min(worst.get(case, (1e9, 0))[0], scale), max(worst.get(case, (1e9, 0))[1], e32))
    print(worst)
