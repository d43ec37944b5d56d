"""CPU: the HiFi-GAN multi-scale discriminator's host side - the yaml sub-block `Vocoder.Train.Adversarial.Multi_Scale`, the state-dict contract (shapes,
seeded init, weight-norm fold, spectral-norm refusal, not taking the multi-period discriminator's state dict for its own), row counts, the reference
(tests/hifigan_msd_ref.py) against a plain-module autograd at 1e-10, that the reference alone holds the guards of the GPU tests' bar at their cases, the
composite's parameter names and the checkpoint bundle.  The signature-table entries of the `glowtts_hifigan_msd_*` entry points are compared with the header
by tests/test_abi.py."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hifigan_disc_ref as HR  # noqa: E402
import hifigan_msd_ref as MR  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402

KEY = "Vocoder.Train.Adversarial.Multi_Scale"
NARROW = {"Scales": 2, "Channels": [16, 32, 64, 32, 64], "Groups": [1, 2, 4, 2, 1], "Strides": [1, 2, 4, 1, 1], "Kernel_Sizes": [15, 41, 41, 41, 5]}


def hp_of(msd=None, adv=None):
    """adv: the Adversarial block (None: absent); msd: the Multi_Scale sub-block put into it (None: absent)"""
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Vocoder"] = {"Type": "HiFiGAN", "Train": {}}
    if adv is not None or msd is not None:
        d["Vocoder"]["Train"]["Adversarial"] = dict(adv or {})
        if msd is not None:
            d["Vocoder"]["Train"]["Adversarial"]["Multi_Scale"] = msd
    return Recursive_Parse(copy.deepcopy(d))


def test_absent_block_gives_todays_result_key_for_key():
    from glow_tts_amd import hifigan_trainer as T
    from glow_tts_amd.vocoder import MPD_DEFAULTS, hifigan_disc_settings, hifigan_msd_settings
    assert "Multi_Scale" not in MPD_DEFAULTS and len(MPD_DEFAULTS) == 10
    assert hifigan_disc_settings(hp_of()) is None and hifigan_msd_settings(hp_of()) is None
    assert hifigan_disc_settings(hp_of(adv={})) == MPD_DEFAULTS and list(hifigan_disc_settings(hp_of(adv={}))) == list(MPD_DEFAULTS)
    assert hifigan_msd_settings(hp_of(adv={})) is None
    s = T.train_settings(hp_of(adv={"Start_Step": 7}))
    assert "Multi_Scale" not in s["Adversarial"] and s["Adversarial"] == dict(MPD_DEFAULTS, Start_Step=7)
    assert [b[4] for b in T.BUNDLES] == [("generator", "Optimizer", "Steps"), ("discriminator", "Discriminator_Optimizer", "Discriminator_Steps")]


def test_multi_scale_is_accepted_and_empty_means_the_defaults():
    """(On the code before this block existed, `Multi_Scale` is an unknown key of `Vocoder.Train.Adversarial`.)"""
    from glow_tts_amd import hifigan_trainer as T
    from glow_tts_amd.vocoder import MPD_DEFAULTS, MSD_DEFAULTS, hifigan_disc_settings, hifigan_msd_geometry, hifigan_msd_settings
    assert MSD_DEFAULTS == {"Scales": 3, "Channels": [128, 128, 256, 512, 1024, 1024, 1024], "Groups": [1, 4, 16, 16, 16, 16, 1],
                            "Strides": [1, 2, 2, 4, 4, 1, 1], "Kernel_Sizes": [15, 41, 41, 41, 41, 41, 5]}
    assert hifigan_msd_settings(hp_of({})) == MSD_DEFAULTS
    s = hifigan_disc_settings(hp_of({}))
    assert s == dict(MPD_DEFAULTS, Multi_Scale=MSD_DEFAULTS)
    s = T.train_settings(hp_of(NARROW, adv={"Negative_Slope": 0.2}))
    assert s["Adversarial"]["Multi_Scale"] == NARROW and s["Adversarial"]["Periods"] == MPD_DEFAULTS["Periods"]
    assert hifigan_msd_settings(hp_of({"Scales": 1}))["Channels"] == MSD_DEFAULTS["Channels"]
    geo = hifigan_msd_geometry(hp_of(NARROW, adv={"Negative_Slope": 0.2}))
    assert geo == {"scales": 2, "channels": NARROW["Channels"], "groups": NARROW["Groups"], "strides": NARROW["Strides"], "kernels": NARROW["Kernel_Sizes"], "slope": 0.2}
    assert hifigan_msd_geometry(hp_of())["channels"] == MSD_DEFAULTS["Channels"] and hifigan_msd_geometry(hp_of())["slope"] == 0.1


def narrow(**change):
    return dict(NARROW, **change)


BAD = [("Scales", {"Scales": 0}), ("Scales", {"Scales": 5}), ("Scales", {"Scales": 1.5}), ("Channels", {"Channels": [16, 32]}), ("Channels", {"Channels": [16] * 9}),
       ("Channels", narrow(Channels=[16, 32, 72, 32, 64])), ("Channels", narrow(Channels=[16, 32, 64, 32, 1040])), ("Channels", {"Channels": 64}),
       ("Kernel_Sizes", narrow(Kernel_Sizes=[17, 41, 41, 41, 5])), ("Kernel_Sizes", narrow(Kernel_Sizes=[14, 41, 41, 41, 5])),
       ("Kernel_Sizes", narrow(Kernel_Sizes=[15, 43, 41, 41, 5])), ("Kernel_Sizes", narrow(Kernel_Sizes=[15, 40, 41, 41, 5])),
       ("Kernel_Sizes", narrow(Kernel_Sizes=[15, 41, 41, 41, 3])), ("Kernel_Sizes", narrow(Kernel_Sizes=[15, 41, 41, 5])),
       ("Strides", narrow(Strides=[2, 2, 4, 1, 1])), ("Strides", narrow(Strides=[1, 3, 4, 1, 1])), ("Strides", narrow(Strides=[1, 2, 8, 1, 1])),
       ("Strides", narrow(Strides=[1, 2, 4, 1, 2])), ("Strides", narrow(Strides=[1, 2, 4, 1])),
       ("Groups", narrow(Groups=[2, 2, 4, 2, 1])), ("Groups", narrow(Groups=[1, 2, 4, 2, 2])), ("Groups", narrow(Groups=[1, 4, 4, 2, 1])),      # 32 / 4 = 8 outputs
       ("Groups", narrow(Groups=[1, 2, 16, 2, 1])),                                                                                            # 32 / 16 = 2 inputs
       ("Groups", narrow(Channels=[128, 128, 64, 32, 64], Groups=[1, 1, 4, 2, 1])),                                                            # 128 inputs in one group
       ("Groups", narrow(Groups=[1, 3, 4, 2, 1])), ("Groups", narrow(Groups=[1, 2, 4, 2])), ("Groups", narrow(Groups=[1, 2.5, 4, 2, 1]))]


@pytest.mark.parametrize("key, block", BAD)
def test_every_bad_key_is_named(key, block):
    from glow_tts_amd import hifigan_trainer as T
    from glow_tts_amd.vocoder import hifigan_msd_settings
    with pytest.raises(ValueError, match="{}.{}".format(KEY, key).replace(".", r"\.")):
        hifigan_msd_settings(hp_of(block))
    with pytest.raises(ValueError, match="{}.{}".format(KEY, key).replace(".", r"\.")):
        T.train_settings(hp_of(block))


def test_unknown_keys_are_named():
    from glow_tts_amd.vocoder import hifigan_disc_settings
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Adversarial\.Multi_Scale\.Bogus"):
        hifigan_disc_settings(hp_of({"Bogus": 1}))
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Adversarial\.Multi_Scale\.Periods"):
        hifigan_disc_settings(hp_of({"Periods": [2]}))
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Adversarial\.Multi_Scales"):
        hifigan_disc_settings(hp_of(adv={"Multi_Scales": {}}))


def test_errors_come_before_the_device(monkeypatch):
    from glow_tts_amd import _lib
    from glow_tts_amd.vocoder import MSD_MIN_SAMPLES, HiFiGANDiscriminators, HiFiGANScaleDiscriminator, hifigan_msd_geometry, hifigan_msd_rows

    def no_device(*a, **k):
        raise AssertionError("the library was loaded before the geometry was checked")
    monkeypatch.setattr(_lib, "lib", no_device)
    for cls in (HiFiGANScaleDiscriminator, HiFiGANDiscriminators):
        with pytest.raises(ValueError, match=r"Vocoder\.Train\.Adversarial\.Multi_Scale\.Groups"):
            cls(hp_of(narrow(Groups=[1, 3, 4, 2, 1])), "cuda:0")
    geo = hifigan_msd_geometry(hp_of(narrow(Scales=3)))
    assert MSD_MIN_SAMPLES <= 64
    with pytest.raises(ValueError, match=r"Vocoder\.Train\.Adversarial\.Multi_Scale.*15 samples"):
        hifigan_msd_rows(geo, MSD_MIN_SAMPLES - 1)
    assert hifigan_msd_rows(geo, 64) == [[64, 64, 32, 8, 8, 8], [33, 33, 17, 5, 5, 5], [17, 17, 9, 3, 3, 3]]


def test_row_counts_and_expected_shapes_at_the_defaults():
    from glow_tts_amd.vocoder import hifigan_msd_expected_shapes, hifigan_msd_geometry, hifigan_msd_rows
    geo = hifigan_msd_geometry(hp_of({}))
    assert hifigan_msd_rows(geo, 8192) == [[8192, 8192, 4096, 2048, 512, 128, 128, 128], [4097, 4097, 2049, 1025, 257, 65, 65, 65], [2049, 2049, 1025, 513, 129, 33, 33, 33]]
    assert hifigan_msd_rows(geo, 513)[0][:5] == [513, 513, 257, 129, 33]
    want = hifigan_msd_expected_shapes(geo)
    assert want == MR.shapes(3, MR.DEFAULT) and list(want) == list(MR.shapes(3, MR.DEFAULT)) and len(want) == 3 * 16
    q = "discriminators.2."
    assert [want[f"{q}convs.{j}.weight"] for j in range(7)] == [(128, 1, 15), (128, 32, 41), (256, 8, 41), (512, 16, 41), (1024, 32, 41), (1024, 64, 41), (1024, 1024, 5)]
    assert want[q + "conv_post.weight"] == (1, 1024, 3) and want[q + "conv_post.bias"] == (1,) and want[q + "convs.3.bias"] == (512,)
    # the pool and the layers' lengths are torch's
    x = torch.zeros(1, 1, 513)
    assert torch.nn.functional.avg_pool1d(x, 4, 2, padding=2).shape[-1] == 513 // 2 + 1
    sd = {k: torch.zeros(s) for k, s in MR.shapes(1, MR.NARROW).items()}
    _, maps = MR.scale_forward(sd, 0, torch.zeros(1, 203), MR.NARROW, 0.1)
    geo = hifigan_msd_geometry(hp_of(narrow(Scales=1)))
    assert [m.shape[-1] for m in maps] == hifigan_msd_rows(geo, 203)[0][1:] + [hifigan_msd_rows(geo, 203)[0][-1]]


def test_seeded_init():
    from glow_tts_amd.vocoder import hifigan_msd_expected_shapes, hifigan_msd_geometry, hifigan_msd_init
    geo = hifigan_msd_geometry(hp_of(NARROW))
    want = hifigan_msd_expected_shapes(geo)
    a, b, c = hifigan_msd_init(geo, 3), hifigan_msd_init(geo, 3), hifigan_msd_init(geo, 4)
    assert all(torch.equal(a[k], b[k]) for k in want) and not torch.equal(a["discriminators.0.convs.1.weight"], c["discriminators.0.convs.1.weight"])
    ref = MR.random_state_dict(2, MR.NARROW, 3)                                                     # the same rule, drawn in the same order
    assert all(torch.equal(a[k], ref[k]) and tuple(a[k].shape) == want[k] and a[k].dtype == torch.float32 for k in want)
    bound = 1.0 / np.sqrt(41 * 16 // 2)                                                             # fan-in = (Cin / groups) k = 8 * 41
    assert float(a["discriminators.0.convs.1.weight"].abs().max()) <= bound and float(a["discriminators.0.convs.1.bias"].abs().max()) <= bound
    assert float(a["discriminators.0.convs.1.weight"].abs().max()) > 1.0 / np.sqrt(41 * 16)         # a dense layer's bound would be smaller


def test_load_folds_weight_norm_refuses_spectral_norm_and_knows_the_periods_dict():
    from glow_tts_amd.vocoder import (MSD_PREFIX, hifigan_disc_geometry, hifigan_disc_load, hifigan_discs_load, hifigan_msd_geometry, hifigan_msd_load)
    hp = hp_of(NARROW, adv={"Periods": [2, 3], "Channels": [16, 32, 16]})
    geo, pgeo = hifigan_msd_geometry(hp), hifigan_disc_geometry(hp)
    sd, psd = MR.random_state_dict(2, MR.NARROW, 5), HR.random_state_dict([2, 3], [16, 32, 16], 6)
    for nest in (lambda d: d, lambda d: {"scale_discriminator": d}, lambda d: {"msd": d}, lambda d: {"model": d}, lambda d: {"model": {"msd": d}},
                 lambda d: {"discriminator": psd, "msd": d}, lambda d: {"mpd": psd, "scale_discriminator": d}):
        got = hifigan_msd_load(nest(dict(sd)), geo)
        assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    # the multi-period discriminator's dict has the same names with 4-d weights: not taken for this one, wherever it lies
    for obj in (psd, {"msd": psd}, {"model": psd}, {"discriminator": psd}):
        with pytest.raises(ValueError, match="no HiFi-GAN multi-scale discriminator"):
            hifigan_msd_load(obj, geo)
    assert all(torch.equal(v, psd[k]) for k, v in hifigan_disc_load({"discriminator": psd, "msd": sd}, pgeo).items())
    # weight norm: g [Cout, 1, 1], v [Cout, Cin / groups, k]
    wn = {}
    for k, v in sd.items():
        if k.endswith(".weight"):
            wn[k + "_g"], wn[k + "_v"] = v.double().reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1), v.double() * 2.5
        else:
            wn[k] = v
    got = hifigan_msd_load({"msd": wn}, geo)
    assert all(float((got[k].double() - sd[k].double()).abs().max()) <= 1e-6 * float(sd[k].abs().max()) for k in sd)
    # a spectral-norm triple is refused by name
    k0 = "discriminators.0.convs.1.weight"
    sn = {k: v for k, v in sd.items() if k != k0}
    sn.update({k0 + "_orig": sd[k0], k0 + "_u": torch.zeros(32), k0 + "_v": torch.zeros(8 * 41)})
    with pytest.raises(ValueError, match=(k0 + "_orig").replace(".", r"\.") + ".*spectral-norm"):
        hifigan_msd_load({"msd": sn}, geo)
    with pytest.raises(ValueError, match="missing key " + k0.replace(".", r"\.")):
        hifigan_msd_load({k: v for k, v in sd.items() if k != k0}, geo)
    with pytest.raises(ValueError, match=k0.replace(".", r"\.") + r" has shape \(32, 16, 41\)"):
        hifigan_msd_load(dict(sd, **{k0: torch.zeros(32, 16, 41)}), geo)
    # the union of both, as the trainer's checkpoint holds it
    union = dict(psd, **{MSD_PREFIX + k: v for k, v in sd.items()})
    got = hifigan_discs_load({"discriminator": union, "Steps": 3}, {"periods": pgeo, "scales": geo})
    assert list(got) == list(union) and all(torch.equal(got[k], union[k]) for k in union)
    with pytest.raises(ValueError, match=r"missing key scale_discriminators\.discriminators\.0\.convs\.0\.weight.*Multi_Scale"):
        hifigan_discs_load({"discriminator": psd}, {"periods": pgeo, "scales": geo})


class PlainScale(torch.nn.Module):
    """One scale as plain torch modules, for the reference to be held against"""

    def __init__(self, net):
        super().__init__()
        cin, convs = 1, []
        for c, g, s, k in zip(net["channels"], net["groups"], net["strides"], net["kernels"]):
            convs.append(torch.nn.Conv1d(cin, c, k, s, padding=k // 2, groups=g))
            cin = c
        self.convs, self.conv_post = torch.nn.ModuleList(convs), torch.nn.Conv1d(cin, 1, 3, 1, padding=1)

    def forward(self, x):
        for conv in self.convs:
            x = torch.nn.functional.leaky_relu(conv(x), 0.1)
        return self.conv_post(x).flatten(1)


@pytest.mark.parametrize("scales, T", [(1, 203), (3, 64), (2, 77)])
def test_the_reference_matches_plain_autograd(scales, T):
    net = MR.NARROW
    sd = MR.random_state_dict(scales, net, 11, 3.0)
    wav = torch.randn(2, T, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    ref = MR.score_grads(sd, wav, scales, net, 0.1, 1.0)
    mods = [PlainScale(net).double() for _ in range(scales)]
    for i, m in enumerate(mods):
        m.load_state_dict({k[len(f"discriminators.{i}."):]: v.double() for k, v in sd.items() if k.startswith(f"discriminators.{i}.")})
    x = wav.clone().requires_grad_(True)
    pool, h, loss, scores = torch.nn.AvgPool1d(4, 2, padding=2), x[:, None, :], 0.0, []
    for i, m in enumerate(mods):
        if i:
            h = pool(h)
        scores.append(m(h))
        loss = loss + ((scores[-1] - 1.0) ** 2).mean()
    loss.backward()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert all(rel(a.detach(), b) < 1e-10 for a, b in zip(scores, ref["scores"])) and rel(x.grad, ref["dwav"]) < 1e-10 and rel(loss.detach().reshape(1), ref["loss"]) < 1e-10
    for i, m in enumerate(mods):
        for k, p in m.named_parameters():
            assert rel(p.grad, ref["grads"][f"discriminators.{i}.{k}"]) < 1e-10, (i, k)
    # the pair terms: L_D is the sum of the two halves; the generator term's parts add up
    fake = wav.flip(1) * 0.5
    p = MR.pair_grads(sd, wav, fake, scales, net, 0.1)
    real_only, fake_only = MR.score_grads(sd, wav, scales, net, 0.1, 1.0), MR.score_grads(sd, fake, scales, net, 0.1, 0.0)
    assert rel(p["loss"], real_only["loss"] + fake_only["loss"]) < 1e-12
    assert all(rel(p["grads"][k], real_only["grads"][k] + fake_only["grads"][k]) < 1e-10 for k in p["grads"])
    g = MR.generator_term_grads(sd, wav, fake, scales, net, 0.1, 1.5, 2.5)
    assert g["fm_terms"].shape == (scales, len(net["channels"]) + 1) and rel(g["loss"], 1.5 * g["adv_terms"].sum() + 2.5 * g["l_fm"]) < 1e-12
    same = MR.generator_term_grads(sd, wav, wav, scales, net, 0.1, 1.5, 2.5)
    assert float(same["l_fm"]) == 0.0


def test_the_gpu_cases_hold_the_guards():
    """The float64 / float32 reference alone, at the weight scale and amplitude of tests/test_gpu_hifigan_msd.py, holds the guards of the bar for every
    tensor that file checks at every one of its cases: 0 < e32 < 1e-3 and max |ref64| > 1e-3."""
    import pwg_train_ref as TR
    import test_gpu_hifigan_msd as G
    assert {(s, b, t) for net, s, b, t in G.CASES.values() if net is MR.NARROW} == {(2, 3, 200), (2, 2, 24), (1, 2, 513), (1, 2, 512), (1, 2, 500), (1, 1, 2300),
                                                                                   (3, 2, 333), (1, 2, 203)}
    assert [(s, b, t) for net, s, b, t in G.CASES.values() if net is MR.DEFAULT] == [(1, 1, 600)]
    assert (G.WEIGHT_SCALE, G.AMPLITUDE) == (3.0, 0.3)
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


def test_the_composite_names_and_the_checkpoint_bundle():
    from glow_tts_amd import hifigan_trainer as T
    from glow_tts_amd.vocoder import (MSD_PREFIX, HiFiGANDiscriminators, hifigan_disc_expected_shapes, hifigan_disc_geometry, hifigan_discs_load, hifigan_discs_split,
                                      hifigan_msd_expected_shapes, hifigan_msd_geometry)
    assert MSD_PREFIX == "scale_discriminators."
    assert [b[4] for b in T.BUNDLES_MULTI_SCALE] == [b[4] for b in T.BUNDLES] and T.BUNDLES_MULTI_SCALE[0] == T.BUNDLES[0]
    assert T.BUNDLES_MULTI_SCALE[1][:3] == T.BUNDLES[1][:3] and T.BUNDLES_MULTI_SCALE[1][3] is hifigan_discs_load
    hp = hp_of(NARROW, adv={"Periods": [2, 3], "Channels": [16, 32, 16]})
    names = list(hifigan_disc_expected_shapes(hifigan_disc_geometry(hp))) + [MSD_PREFIX + k for k in hifigan_msd_expected_shapes(hifigan_msd_geometry(hp))]
    union = {k: i for i, k in enumerate(names)}
    mpd, msd = hifigan_discs_split(union)
    assert list(mpd) == names[:len(mpd)] and [MSD_PREFIX + k for k in msd] == names[len(mpd):] and len(msd) == 2 * 12
    assert hasattr(HiFiGANDiscriminators, "score_pair") and hasattr(HiFiGANDiscriminators, "score")
