"""Neural vocoder, host side (no GPU): the float64 restatement's conditioning against torch.nn.functional, the checkpoint loader, the geometry errors, the
ABI additions and the seed words."""
import copy
import hashlib
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pwg_ref as P  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hp(vocoder=None, **sound):
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Sound"]["Mel_Dim"] = 80
    d["Sound"].update(sound)
    if vocoder is not None:
        d["Vocoder"] = vocoder
    return Recursive_Parse(d)


def _geo(cfg):
    from glow_tts_amd.vocoder import pwg_geometry
    return pwg_geometry(_hp({"Layers": cfg["layers"], "Stacks": cfg["stacks"], "Residual_Channels": cfg["R"], "Gate_Channels": cfg["G"], "Skip_Channels": cfg["S"],
                             "Aux_Context_Window": cfg["ctx"], "Upsample_Scales": cfg["scales"]}, Mel_Dim=cfg["A"], Frame_Shift=P.hop(cfg)))


@pytest.mark.parametrize("cfg, L", [(P.DEFAULT, 1), (P.DEFAULT, 2), (P.DEFAULT, 7), (P.NARROW, 1), (P.NARROW, 5)])
def test_restated_conditioning_is_repeat_and_convolve(cfg, L):
    """The index arithmetic of pwg_ref.condition against replicate-pad + conv1d, then per scale repeat_interleave + a zero-padded conv2d of one shared FIR."""
    sd = P.random_state_dict(cfg, 5)
    mel = P.uniform_mel(cfg["A"], L, 6).double()
    c = F.conv1d(F.pad(mel[None], (cfg["ctx"], cfg["ctx"]), mode="replicate"), sd["upsample_net.conv_in.weight"].double())
    for i, s in enumerate(cfg["scales"]):
        w = sd["upsample_net.upsample.up_layers.{}.weight".format(2 * i + 1)].double()
        c = F.conv2d(c.repeat_interleave(s, dim=2)[:, None], w, padding=(0, s))[:, 0]
    got = P.condition(sd, cfg, mel)
    assert got.shape == (cfg["A"], L * P.hop(cfg))
    assert float((got - c[0]).abs().max()) <= 1e-13 * float(c.abs().max())


def test_geometry_defaults_and_every_unsupported_case_names_its_keys():
    from glow_tts_amd.vocoder import pwg_geometry
    g = pwg_geometry(_hp({}))
    assert (g["layers"], g["stacks"], g["R"], g["G"], g["S"], g["A"], g["ctx"], g["scales"], g["hop"]) == (30, 3, 64, 128, 64, 80, 2, [4, 4, 4, 4], 256)
    assert g["dilations"] == [2 ** (i % 10) for i in range(30)]
    assert _geo(P.NARROW)["dilations"] == [1, 2, 1, 2]
    bad = [({"Type": "HiFiGAN"}, {}, ["Vocoder.Type"]),
           ({"Gate_Channels": 96}, {}, ["Vocoder.Gate_Channels", "Vocoder.Residual_Channels"]),
           ({"Residual_Channels": 40, "Gate_Channels": 80}, {}, ["Vocoder.Residual_Channels"]),
           ({"Skip_Channels": 24}, {}, ["Vocoder.Skip_Channels"]),
           ({}, {"Mel_Dim": 78}, ["Sound.Mel_Dim"]),
           ({"Layers": 30, "Stacks": 4}, {}, ["Vocoder.Layers", "Vocoder.Stacks"]),
           ({"Layers": 24, "Stacks": 2}, {}, ["Vocoder.Layers", "Vocoder.Stacks"]),                 # dilations up to 2048
           ({"Upsample_Scales": [4, 4, 4]}, {}, ["Vocoder.Upsample_Scales", "Sound.Frame_Shift"]),
           ({"Upsample_Scales": [32, 8]}, {}, ["Vocoder.Upsample_Scales"]),
           ({"Upsample_Scales": [0, 256]}, {}, ["Vocoder.Upsample_Scales"])]
    for voc, sound, keys in bad:
        with pytest.raises(ValueError) as e:
            pwg_geometry(_hp(voc, **sound))
        assert all(k in str(e.value) for k in keys), (voc, sound, str(e.value))
    assert pwg_geometry(_hp({"Layers": 22, "Stacks": 2}))["dilations"][10] == 1024                      # the largest supported dilation


def test_loader_folds_weight_norm_finds_nesting_and_names_bad_keys():
    from glow_tts_amd.vocoder import pwg_expected_shapes, pwg_load
    cfg = P.NARROW
    geo = _geo(cfg)
    assert pwg_expected_shapes(geo) == P.shapes(cfg)
    sd = P.random_state_dict(cfg, 9)
    plain = pwg_load(sd, geo)
    assert set(plain) == set(sd) and all(torch.equal(plain[k], sd[k]) for k in sd)
    wn = {}
    for k, t in sd.items():                                                  # v = 2 w, g = |w| per output channel: the fold gives w back exactly
        if k.endswith(".weight"):
            wn[k + "_v"] = 2.0 * t
            wn[k + "_g"] = t.double().reshape(t.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (t.dim() - 1))
        else:
            wn[k] = t
    folded = pwg_load(wn, geo)
    assert all(folded[k].dtype == torch.float32 and (folded[k] - sd[k]).abs().max() <= 1e-7 * sd[k].abs().max() for k in sd)
    half = {k: v for k, v in wn.items() if not k.startswith("first_conv.weight")}
    half["first_conv.weight"] = sd["first_conv.weight"]                     # mixed forms load too
    assert torch.equal(pwg_load(half, geo)["first_conv.weight"], sd["first_conv.weight"])
    for nest in (lambda d: {"generator": d}, lambda d: {"Generator": d}, lambda d: {"model": {"generator": d}}, lambda d: {"model": d},
                 lambda d: {"model": {"Generator": d}, "steps": 3}):
        got = pwg_load(nest(sd), geo)
        assert all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="no Parallel WaveGAN generator"):
        pwg_load({"discriminator": {}}, geo)
    missing = dict(sd)
    del missing["conv_layers.2.conv1x1_skip.bias"]
    with pytest.raises(ValueError, match=re.escape("conv_layers.2.conv1x1_skip.bias")):
        pwg_load(missing, geo)
    surplus = dict(sd, **{"conv_layers.4.conv.bias": torch.zeros(64)})
    with pytest.raises(ValueError, match=re.escape("conv_layers.4.conv.bias")):
        pwg_load(surplus, geo)
    shaped = dict(sd, **{"conv_layers.1.conv1x1_aux.weight": torch.zeros(64, 80, 1)})
    with pytest.raises(ValueError, match=re.escape("conv_layers.1.conv1x1_aux.weight")):
        pwg_load(shaped, geo)
    lone = dict(sd, **{"first_conv.weight_g": torch.ones(32, 1, 1)})
    with pytest.raises(ValueError, match="first_conv.weight"):
        pwg_load(lone, geo)


def test_constructor_checks_geometry_and_checkpoint_before_the_device():
    from glow_tts_amd.vocoder import ParallelWaveGAN
    with pytest.raises(ValueError, match="Vocoder.Gate_Channels"):
        ParallelWaveGAN(_hp({"Gate_Channels": 64}), "cuda:0", state_dict={})
    with pytest.raises(ValueError, match="Vocoder.Checkpoint_Path"):
        ParallelWaveGAN(_hp({}), "cuda:0")
    from glow_tts_amd.inferencer import build_parser
    a = build_parser().parse_args(["-c", "x.pt", "--wav", "--vocoder", "pwg", "--vocoder-checkpoint", "v.pt"])
    assert (a.vocoder, a.vocoder_checkpoint) == ("pwg", "v.pt") and build_parser().parse_args(["-c", "x.pt"]).vocoder is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-c", "x.pt", "--vocoder", "wavernn"])


def test_abi_additions_are_in_header_and_table_and_the_version_stays():
    from glow_tts_amd import abi
    text = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    for n in ("glowtts_pwg_supported", "glowtts_pwg_condition", "glowtts_pwg_first", "glowtts_pwg_layer", "glowtts_pwg_head"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert n in abi.SIGNATURES
    assert abi.ABI_VERSION == 7 and re.search(r"#define\s+GLOWTTS_ABI_VERSION\s+7\b", text)


def test_supported_and_argument_validation_on_the_host():
    """glowtts_pwg_supported, and the entry points refuse bad sizes with the argument error before anything is launched (no device is touched)."""
    from glow_tts_amd import _lib, abi
    L = _lib.lib()
    assert L.glowtts_pwg_supported(64, 128, 64, 80, 512) == 1 and L.glowtts_pwg_supported(32, 64, 32, 20, 2) == 1
    for args in ((64, 96, 64, 80, 512), (40, 80, 64, 80, 1), (64, 128, 24, 80, 1), (64, 128, 64, 78, 1), (64, 128, 64, 80, 2048), (64, 128, 64, 80, 0),
                 (512, 1024, 64, 80, 1)):
        assert L.glowtts_pwg_supported(*args) == 0, args
    p = 4096                                                                 # a non-null address that is never dereferenced: every call below is refused
    assert L.glowtts_pwg_layer(p, p, p, p, p, p, p + 4, p, p, 1, 4, 256, 64, 64, 80, 2048, 0, None) == abi.E_ARG      # dilation
    assert L.glowtts_pwg_layer(p, p, p, p, p, p, p, p, p, 1, 4, 256, 64, 64, 80, 1, 0, None) == abi.E_ARG             # in place
    assert L.glowtts_pwg_layer(p, p, p, p, p, p, p + 4, p, p, 1, 1 << 24, 256, 64, 64, 80, 1, 0, None) == abi.E_ARG   # Lmax * hop beyond 2^30
    assert L.glowtts_pwg_layer(p, p, p, p, p, p, p + 4, p, p, 0, 4, 256, 64, 64, 80, 1, 0, None) == abi.E_ARG         # B
    assert L.glowtts_pwg_first(p, p, p, p, p, p, 1, 4, 256, 64, None) == abi.E_ARG                                    # noises AND seeds
    assert L.glowtts_pwg_first(None, None, p, p, p, p, 1, 4, 256, 64, None) == abi.E_ARG
    assert L.glowtts_pwg_first(p, None, p, p, p, p, 1, 4, 256, 40, None) == abi.E_ARG
    assert L.glowtts_pwg_head(p, p, p, p, p, p, p, 1, 4, 256, 24, 1.0, None) == abi.E_ARG
    import ctypes
    scales = (ctypes.c_int * 2)(32, 8)
    assert L.glowtts_pwg_condition(p, p, p, p, scales, 2, p, p, 1, 80, 4, 2, None) == abi.E_ARG                       # a scale beyond 16
    assert L.glowtts_pwg_condition(p, p, p, p, scales, 0, p, p, 1, 80, 4, 2, None) == abi.E_ARG
    assert L.glowtts_pwg_condition(p, p, p, p, None, 2, p, p, 1, 80, 4, 2, None) == abi.E_ARG


def test_vocoder_seed_words_differ_from_the_mels():
    from glow_tts_amd.inferencer import utterance_seed_words
    from glow_tts_amd.vocoder import pwg_seed_words
    for seed, label, k in ((7, "A", 0), (7, "A", 1), (0, "Bravo", 0), (123456789, "x y", 3)):
        w = pwg_seed_words(seed, label, k)
        d = hashlib.blake2b("{}\0{}\0{}\0pwg".format(seed, label, k).encode()).digest()
        assert w == (int.from_bytes(d[:4], "little"), int.from_bytes(d[4:8], "little")) == P.pwg_seed_words(seed, label, k)
        assert w != utterance_seed_words(seed, label, k) and set(w).isdisjoint(utterance_seed_words(seed, label, k))
        assert all(0 <= x < 2 ** 32 for x in w)
    assert len({pwg_seed_words(7, "A", k) for k in range(4)}) == 4


def test_restatement_guards_hold_for_the_gpu_cases():
    """The seeds the GPU tests use give non-degenerate cases: 0 < e32 < 1e-3 and max |ref64| > 1e-3 (whole generator, narrow net: the cheap one here)."""
    cfg = P.NARROW
    sd = P.random_state_dict(cfg, 1234)
    mel = P.uniform_mel(cfg["A"], 5, 12)
    z = torch.randn(5 * P.hop(cfg), generator=torch.Generator().manual_seed(112))
    r64, r32 = P.generator(sd, cfg, mel, z), P.generator(sd, cfg, mel, z, torch.float32)
    _, e32 = P.errors(r32, r64, r32)
    assert r32.dtype == torch.float32 and 0 < e32 < 1e-3 and float(r64.abs().max()) > 1e-3
    assert copy.deepcopy(sd).keys() == P.shapes(cfg).keys()


def test_pwg_kernels_use_no_scratch_memory(tmp_path):
    """As test_gpu_griffin_lim.test_vocoder_kernels_use_no_scratch_memory, for the kernels of csrc/pwg_ops.hip (code-object metadata; nothing is executed)."""
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    assert os.path.exists(f"{llvm}/llvm-objdump") and os.path.exists(f"{llvm}/llvm-readelf"), "ROCm LLVM tools not found"
    shutil.copy(os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    found = {"pwg_cond_in_kernel": 0, "pwg_upsample_kernel": 0, "pwg_first_kernel": 0, "pwg_layer_kernel": 0, "pwg_head_kernel": 0}
    for f in [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        for name, scratch, vgpr in re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S):
            for h in found:
                if h in name:
                    found[h] += 1
                    print(f"{name}: {vgpr} VGPRs, {scratch} bytes of scratch")
                    assert int(scratch) == 0, f"{name} spills: {scratch} bytes of scratch per lane at {vgpr} VGPRs"
    assert all(n > 0 for n in found.values()), found
