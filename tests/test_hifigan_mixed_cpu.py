"""Mixed-precision training of the HiFi-GAN generator, host side (no GPU): the restatement (tests/hifigan_mixed_ref.py) against itself - its forward is the
fp16 mode's bit for bit, its float32 realisations meet the bars that tests/test_gpu_hifigan_mixed.py sets for the kernels, the operator cases stay inside their
guard - and the setting: the constructor's argument, the yaml key, the refusals (all before the device is touched), the launch plan and the job table."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan_f16_ref as R16  # noqa: E402
import hifigan_mixed_cases as C  # noqa: E402
import hifigan_mixed_ref as M  # noqa: E402
import hifigan_ref as H  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E64, E32, E32B = M.emus(C.FC.FLUSH_SUBNORMALS)


def _hp(vocoder=None, **sound):
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Sound"]["Mel_Dim"] = 80
    d["Sound"].update(sound)
    if vocoder is not None:
        d["Vocoder"] = vocoder
    return Recursive_Parse(d)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name, seed, lengths", [c for c in C.GENERATOR_CASES if c[2] == [3]])
def test_the_restatements_forward_is_the_f16_modes_bit_for_bit(name, seed, lengths):
    ref, f16 = C.reference(name, seed, lengths), C.FC.reference(name, seed, lengths[0])
    for tag in ("emu64", "emu32", "emu32b"):
        assert torch.equal(ref["wav_" + tag][0], f16[tag][0]), tag


@pytest.mark.parametrize("name, seed, lengths", C.GENERATOR_CASES)
def test_the_float32_realisations_meet_the_generator_bars(name, seed, lengths):
    ref = C.reference(name, seed, lengths)
    keys = C.pairs((name, seed, lengths))
    assert not [k for k in ref["ref64"] if k not in keys and not k.endswith(".bias")]              # no weight tensor is dropped
    for k in keys:
        for tag in ("emu32", "emu32b"):
            C.check_generator(f"{name} {seed} {lengths} {tag} d {k}", ref[tag][k], ref, k, name != "default")
    for k in ref["ref64"]:                                                    # what the mode costs a gradient (informational)
        cos, norm = C.cost(ref, k)
        print(f"{name} {seed} {lengths} d {k}: cosine {cos:.6f}  norm ratio {norm:.5f} (emu64 against ref64)")


def test_the_dropped_pairs_are_few_are_biases_and_do_miss_the_guard():
    total = sum(len(H.shapes(C.CFGS[name])) for name, _, _ in C.GENERATOR_CASES)
    assert len(C.DROPPED) <= 0.05 * total and all(k.endswith(".bias") for *_, k in C.DROPPED)
    cases = {(n, s, tuple(L)) for n, s, L in C.GENERATOR_CASES}
    for name, seed, lengths, k in sorted(C.DROPPED):
        assert (name, seed, lengths) in cases
        if name != "default":                                                 # (DEFAULT's reference is computed by the test above; its pair is conv_post.bias)
            assert not C.figures(C.reference(name, seed, list(lengths)), k)[3], (name, seed, lengths, k)


@pytest.mark.parametrize("taps, d", C.CONV_TAPS)
@pytest.mark.parametrize("cdy, cdx", [(16, 16), (48, 32), (256, 256)])
def test_conv_operator_cases_stay_inside_the_guard(cdy, cdx, taps, d):
    rows = [1, 5, 65, 200]
    w, b, xs, dys, _, _ = C.conv_case(cdy, cdx, taps, d, rows)
    got = {e: M.conv_grads(e, xs, w, b, dys, d, H.SLOPE, C.SCALE) for e in (E64, E32, E32B)}
    for i, T in enumerate(rows):
        C.check_operator(f"dx emu32b {cdx}<-{cdy} k={taps} d={d} T={T}", got[E32B][0][i], got[E64][0][i], got[E32][0][i])
    C.check_operator(f"dw emu32b {cdx}<-{cdy} k={taps} d={d}", got[E32B][1], got[E64][1], got[E32][1])


@pytest.mark.parametrize("u, k", C.UP_KERNELS)
def test_upsample_operator_cases_stay_inside_the_guard(u, k):
    w, b, xs, dys = C.up_case(64, 32, u, k, C.UP_ROWS)
    got = {e: M.upsample_grads(e, xs, w, b, dys, u) for e in (E64, E32, E32B)}
    for i, T in enumerate(C.UP_ROWS):
        C.check_operator(f"dx emu32b u={u} k={k} T={T}", got[E32B][0][i], got[E64][0][i], got[E32][0][i])
    C.check_operator(f"dw emu32b u={u} k={k}", got[E32B][1], got[E64][1], got[E32][1])


def test_the_contracts_backward_rounds_what_it_says_and_nothing_else():
    """On operands that bf16 holds exactly the contract's gradients are the unrounded network's; the bias gradient never sees a rounding; the slope at x == 0"""
    import hifigan_train_ref as TR
    g = torch.Generator().manual_seed(1)
    q = lambda *s: torch.randint(-8, 9, s, generator=g).double() / 8          # exact in bf16 and fp16; small sums stay exact too
    w, b, x = q(16, 16, 3), q(16), q(9, 16)
    dy = torch.randint(8, 17, (9, 16), generator=g).double() / 8             # in [1, 2]: bf16 resolves 2^-7 there
    x[2, 3] = 0.0
    ref = TR.conv_grads([x], w, b, [dy], 1, 0.5)                              # slope 0.5: exact
    got = M.conv_grads(E64, [x], w, b, [dy], 1, 0.5)
    assert torch.equal(got[0][0], ref[0][0]) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    fine = dy + 2.0 ** -12                                                    # below bf16's resolution at this size: the products lose it, the bias gradient keeps it
    got2 = M.conv_grads(E64, [x], w, b, [fine], 1, 0.5)
    assert torch.equal(got2[0][0], got[0][0]) and torch.equal(got2[1], got[1]) and torch.equal(got2[2], fine.sum(0))
    assert float(M.mask(torch.zeros(1, dtype=torch.float64), 0.5)) == 0.5


# ---------------------------------------------------------------------------------------------------------------- setting, constructor, refusals
def test_train_precision_is_validated_before_the_device_is_touched():
    from glow_tts_amd.vocoder import HIFIGAN_TRAIN_PRECISIONS, HiFiGAN, hifigan_train_precision
    assert HIFIGAN_TRAIN_PRECISIONS == ("f32", "mixed")
    hi = _hp({"Type": "HiFiGAN"})
    assert hifigan_train_precision(hi) == "f32" and hifigan_train_precision(_hp({"Type": "HiFiGAN", "Train": {"Precision": "mixed"}})) == "mixed"
    for bad in ("bf16", "f16", "Mixed", "", 16):
        with pytest.raises(ValueError, match="train_precision"):
            HiFiGAN(hi, "cuda:0", state_dict={}, trainable=True, train_precision=bad)
        with pytest.raises(ValueError, match=r"Vocoder\.Train\.Precision"):
            HiFiGAN(_hp({"Type": "HiFiGAN", "Train": {"Precision": bad}}), "cuda:0", state_dict={}, trainable=True)
    for tp in ("f32", "mixed"):                                               # on a frozen generator the argument is refused by name
        with pytest.raises(ValueError, match="train_precision.*frozen"):
            HiFiGAN(hi, "cuda:0", state_dict={}, train_precision=tp)
    with pytest.raises(ValueError, match="trainable.*f32"):                   # what held before still holds
        HiFiGAN(hi, "cuda:0", state_dict={}, trainable=True, precision="f16", train_precision="mixed")
    # a valid value gets as far as the state dict, by the argument and by the key; the yaml's key is not read by a frozen generator
    with pytest.raises(ValueError, match="no HiFi-GAN generator"):
        HiFiGAN(hi, "cuda:0", state_dict={"generator": {}}, trainable=True, train_precision="mixed")
    with pytest.raises(ValueError, match="no HiFi-GAN generator"):
        HiFiGAN(_hp({"Type": "HiFiGAN", "Train": {"Precision": "mixed"}}), "cuda:0", state_dict={"generator": {}}, trainable=True)
    with pytest.raises(ValueError, match="no HiFi-GAN generator"):
        HiFiGAN(_hp({"Type": "HiFiGAN", "Train": {"Precision": "bf16"}}), "cuda:0", state_dict={"generator": {}})
    # unsupported sizes name their yaml keys
    for block, sound, key in (({"Initial_Channels": 1024}, {}, "Vocoder.Initial_Channels"), ({"Resblock_Dilations": [[1, 3, 17]] * 3}, {}, "Vocoder.Resblock_Dilations"),
                              ({"Resblock_Kernel_Sizes": [3, 13, 11]}, {}, "Vocoder.Resblock_Kernel_Sizes"), ({}, {"Mel_Dim": 78}, "Sound.Mel_Dim"),
                              ({"Upsample_Rates": [32, 8], "Upsample_Kernel_Sizes": [64, 16]}, {}, "Vocoder.Upsample_Rates")):
        with pytest.raises(ValueError, match=re.escape(key)):
            HiFiGAN(_hp(dict({"Type": "HiFiGAN"}, **block), Frame_Shift=256, **sound), "cuda:0", state_dict={}, trainable=True, train_precision="mixed")
        with pytest.raises(ValueError, match=re.escape(key)):
            HiFiGAN(_hp(dict({"Type": "HiFiGAN", "Train": {"Precision": "mixed"}}, **block), Frame_Shift=256, **sound), "cuda:0", state_dict={}, trainable=True)
    text = open(os.path.join(REPO, "glow_tts_amd", "Hyper_Parameters.default.yaml")).read()
    assert re.search(r"(?m)^#\s+Precision: 'f32'\s+# 'f32' \| 'mixed'", text)   # documented in the commented Train block


def test_the_mixed_predicate_is_the_f32_one_with_the_16_bit_tiles():
    from glow_tts_amd import _lib
    from glow_tts_amd.vocoder import hifigan_convs, hifigan_geometry
    api = _lib.api()
    for cfg in (H.DEFAULT, H.NARROW, H.ODD):
        hp = _hp({"Type": "HiFiGAN", "Initial_Channels": cfg["C0"], "Upsample_Rates": cfg["rates"], "Upsample_Kernel_Sizes": cfg["kernels"], "Resblock": cfg["resblock"],
                  "Resblock_Kernel_Sizes": cfg["rk"], "Resblock_Dilations": cfg["rd"]}, Mel_Dim=cfg["A"], Frame_Shift=H.hop(cfg))
        for _, ci, co, taps, d, rate, _ in hifigan_convs(hifigan_geometry(hp)):
            assert api.glowtts_hifigan_train_supported_mixed(ci, co, taps, d, rate) == 1
    assert api.glowtts_hifigan_train_supported_mixed(32, 1, 7, 1, 0) == 1     # conv_post answers for its f32 launches
    for args in ((24, 16, 4, 1, 2), (16, 16, 13, 1, 0), (16, 16, 3, 17, 0), (16, 24, 3, 1, 0), (1024, 16, 3, 1, 0), (512, 512, 32, 1, 16)):
        assert api.glowtts_hifigan_train_supported_mixed(*args) == 0, args
        assert api.glowtts_hifigan_train_supported_mixed(*args) <= api.glowtts_hifigan_train_supported(*args)


def test_the_trainers_read_the_key_or_refuse_it_by_name():
    from glow_tts_amd import hifigan_trainer, pwg_trainer
    s = hifigan_trainer.train_settings(_hp({"Type": "HiFiGAN"}, Frame_Shift=256))
    assert "Precision" not in s and "Precision" not in hifigan_trainer.DEFAULTS and "Precision" not in pwg_trainer.DEFAULTS     # an absent key changes nothing
    assert hifigan_trainer.train_settings(_hp({"Type": "HiFiGAN", "Train": {"Precision": "mixed"}}, Frame_Shift=256))["Precision"] == "mixed"
    with pytest.raises(ValueError, match=r"Vocoder\.Train\.Precision"):
        hifigan_trainer.train_settings(_hp({"Type": "HiFiGAN", "Train": {"Precision": "bf16"}}, Frame_Shift=256))
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Precision"):             # Train_PWG.py: an unknown key, refused by name
        pwg_trainer.train_settings(_hp({"Train": {"Precision": "mixed"}}, Frame_Shift=256))
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Precision"):
        pwg_trainer.train_settings(_hp({"Train": {"Precision": "f32"}}, Frame_Shift=256))


# ---------------------------------------------------------------------------------------------------------------- the launch plan and the job table
def test_the_mixed_launch_plan():
    from glow_tts_amd.vocoder import hifigan_geometry, hifigan_launches, hifigan_train_launches
    geo = hifigan_geometry(_hp({"Type": "HiFiGAN"}, Frame_Shift=256))         # the V1 sizes
    f32, mixed = hifigan_train_launches(geo), hifigan_train_launches(geo, "mixed")
    assert hifigan_train_launches(geo, "f32") == f32 and not [k for k in f32 if "f16" in k or "pack" in k]
    n = hifigan_launches(geo)
    assert n == 78
    assert mixed == {"hifigan_pack_images": 1, "hifigan_conv_f16": 73, "hifigan_upsample_f16": 4, "hifigan_conv,post": 1, "hifigan_post_bwd": 1,
                     "hifigan_conv_bwd_bf16": 72, "hifigan_upsample_bwd_bf16": 4, "hifigan_wgrad_bf16": 77, "hifigan_wgrad": 1, "hifigan_wgrad_sum": 78}
    assert sum(mixed.values()) == sum(f32.values()) + 1
    with pytest.raises(ValueError, match="train_precision"):
        hifigan_train_launches(geo, "bf16")


def test_the_pack_plan_covers_every_image_of_a_step():
    from glow_tts_amd.vocoder import hifigan_convs, hifigan_geometry, hifigan_pack_plan, hifigan_up_reach, pad32
    geo = hifigan_geometry(_hp({"Type": "HiFiGAN"}, Frame_Shift=256))
    plan = hifigan_pack_plan(geo)
    kinds = [p[1] for p in plan]
    assert kinds.count("conv_f16") == 73 and kinds.count("up_f16") == 4 and kinds.count("conv_t_bf16") == 72 and kinds.count("up_t_bf16") == 4
    assert kinds.count("post_f32") == 1 and len(plan) == 154
    by = {(p[0], p[1]): p for p in plan}
    for name, ci, co, taps, _, rate, _ in hifigan_convs(geo):
        if co == 1:
            assert by[(name + ".weight", "post_f32")][6:] == ((taps * ci,), torch.float32)
        elif rate:
            lo, hi = hifigan_up_reach(rate, taps)
            assert by[(name + ".weight", "up_f16")][6:] == ((taps, pad32(ci) // 8, co, 8), torch.float16)
            assert by[(name + ".weight", "up_t_bf16")][6:] == ((hi - lo + 1, pad32(rate * co) // 8, ci, 8), torch.bfloat16)
        else:
            assert by[(name + ".weight", "conv_f16")][6:] == ((taps, pad32(ci) // 8, co, 8), torch.float16)
            assert ((name + ".weight", "conv_t_bf16") in by) == (name != "conv_pre")


def test_pack_bf16_is_pack_f16s_layout_without_the_clamp():
    from glow_tts_amd.vocoder import hifigan_pack_bf16, hifigan_pack_f16
    g = torch.Generator().manual_seed(2)
    image = torch.randn(3 * 48, 16, generator=g)
    image[0, 0], image[1, 1] = 1e30, -3e-30                                   # beyond fp16's range: bf16 keeps them
    p = hifigan_pack_bf16(image, 3)
    assert p.dtype == torch.bfloat16 and p.shape == (3, 8, 16, 8) == hifigan_pack_f16(image, 3).shape
    back = p.permute(0, 1, 3, 2).reshape(3, 64, 16).float()
    assert torch.equal(back[:, :48], image.to(torch.bfloat16).float().view(3, 48, 16)) and not back[:, 48:].any()
    assert float(back[0, 0, 0]) == float(torch.tensor(1e30).to(torch.bfloat16))


def test_abi_declares_the_mixed_entries():
    from glow_tts_amd import abi
    header = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    for name in ("glowtts_hifigan_train_supported_mixed", "glowtts_hifigan_conv_bwd_bf16", "glowtts_hifigan_upsample_bwd_bf16", "glowtts_hifigan_wgrad_bf16",
                 "glowtts_hifigan_pack_images"):
        assert name in abi.SIGNATURES and re.search(r"\b" + name + r"\(", header), name
    assert "glowtts_hifigan_train_supported_mixed" in abi.VALUE_RETURNING
    assert R16.Emu.conv is not M.Emu.conv and issubclass(M.Emu, R16.Emu)      # the forward is imported, not copied
