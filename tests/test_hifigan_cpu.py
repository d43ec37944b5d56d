"""HiFi-GAN vocoder, host side (no GPU): the float64 restatement's transposed convolution against zero-stuffing + conv1d, per-utterance independence of
the restatement, the geometry errors, the checkpoint loader, the vocoder choice, the parser and the ABI additions."""
import copy
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan_ref as H  # noqa: E402
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


def block_of(cfg, **more):
    return dict({"Type": "HiFiGAN", "Initial_Channels": cfg["C0"], "Upsample_Rates": list(cfg["rates"]), "Upsample_Kernel_Sizes": list(cfg["kernels"]),
                 "Resblock": cfg["resblock"], "Resblock_Kernel_Sizes": list(cfg["rk"]), "Resblock_Dilations": [list(d) for d in cfg["rd"]]}, **more)


def _geo(cfg):
    from glow_tts_amd.vocoder import hifigan_geometry
    return hifigan_geometry(_hp(block_of(cfg), Mel_Dim=cfg["A"], Frame_Shift=H.hop(cfg)))


@pytest.mark.parametrize("u, k", [(2, 4), (8, 16), (3, 7), (5, 11), (4, 4), (1, 3)])
@pytest.mark.parametrize("T", [1, 2, 9])
def test_restated_transposed_convolution_is_zero_stuffing_and_convolve(u, k, T):
    """The index arithmetic of hifigan_ref.upsample against zero-stuffing + conv1d with the flipped kernel, and against torch's own conv_transpose1d."""
    g = torch.Generator().manual_seed(10 * u + k + T)
    cin, cout = 6, 4
    x = torch.randn(cin, T, generator=g, dtype=torch.float64)
    w, b = torch.randn(cin, cout, k, generator=g, dtype=torch.float64), torch.randn(cout, generator=g, dtype=torch.float64)
    got = H.upsample(x, w, b, u)
    assert got.shape == (cout, u * T)
    xl = F.leaky_relu(x, H.SLOPE)
    stuffed = torch.zeros(cin, (T - 1) * u + 1, dtype=torch.float64)
    stuffed[:, ::u] = xl
    p = (k - u) // 2
    want = F.conv1d(F.pad(stuffed[None], (k - 1 - p, k - 1 - p)), w.flip(2).transpose(0, 1), b)[0]
    assert want.shape == got.shape and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    lib = F.conv_transpose1d(xl[None], w, b, stride=u, padding=p)[0]
    assert float((got - lib).abs().max()) <= 1e-12 * float(lib.abs().max())


def test_restated_ragged_batch_equals_the_single_runs():
    """Every utterance is computed as if alone: the restatement run on the utterances of a ragged batch one by one is the single run (it has no batch axis),
    and a mel padded beyond its length and cut back gives other samples - which is why the product masks by length instead of trusting the padding."""
    cfg = H.NARROW
    sd = H.random_state_dict(cfg, 3)
    mels = [H.uniform_mel(cfg["A"], L, 50 + L) for L in (5, 2, 7)]
    for m in mels:
        w1, r1 = H.generator(sd, cfg, m)
        w2, r2 = H.generator(copy.deepcopy(sd), cfg, m.clone())
        assert torch.equal(w1, w2) and torch.equal(r1, r2) and w1.shape == (m.shape[1] * H.hop(cfg),) and r1.shape == (16, m.shape[1] * H.hop(cfg))
    padded = torch.full((cfg["A"], 7), -4.0)
    padded[:, :2] = mels[1]
    assert not torch.equal(H.generator(sd, cfg, padded)[0][:2 * H.hop(cfg)], H.generator(sd, cfg, mels[1])[0])


def test_geometry_defaults_and_every_unsupported_case_names_its_keys():
    from glow_tts_amd.vocoder import HIFIGAN_DEFAULTS, hifigan_geometry, hifigan_launches, hifigan_settings, pwg_geometry
    assert hifigan_settings(_hp())["Upsample_Rates"] == [8, 8, 2, 2] and hifigan_settings(_hp({"Initial_Channels": 256}))["Initial_Channels"] == 256
    g = hifigan_geometry(_hp({"Type": "HiFiGAN"}))
    assert (g["A"], g["hop"], g["C0"], g["rates"], g["kernels"], g["channels"]) == (80, 256, 512, [8, 8, 2, 2], [16, 16, 4, 4], [256, 128, 64, 32])
    assert (g["resblock"], g["rk"], g["rd"], g["nk"], g["precision"]) == ("1", [3, 7, 11], [[1, 3, 5]] * 3, 3, "f32")
    assert HIFIGAN_DEFAULTS["Type"] == "HiFiGAN" and hifigan_launches(g) == 78
    assert hifigan_launches(hifigan_geometry(_hp({"Type": "HiFiGAN", "Resblock": "2", "Resblock_Dilations": [[1, 3]] * 3}))) == 30
    assert _geo(H.NARROW)["channels"] == [32, 16] and _geo(H.ODD)["hop"] == 15
    bad = [({"Upsample_Rates": [8, 8, 2]}, {}, ["Vocoder.Upsample_Rates", "Vocoder.Upsample_Kernel_Sizes"]),                 # lengths differ
           ({"Upsample_Rates": [8, 8, 2], "Upsample_Kernel_Sizes": [16, 16, 4]}, {}, ["Vocoder.Upsample_Rates", "Sound.Frame_Shift"]),
           ({"Upsample_Kernel_Sizes": [16, 16, 4, 1]}, {}, ["Vocoder.Upsample_Kernel_Sizes", "Vocoder.Upsample_Rates"]),      # k < u
           ({"Upsample_Kernel_Sizes": [16, 16, 4, 5]}, {}, ["Vocoder.Upsample_Kernel_Sizes", "Vocoder.Upsample_Rates"]),      # k - u odd
           ({"Upsample_Rates": [32, 8], "Upsample_Kernel_Sizes": [64, 16]}, {}, ["Vocoder.Upsample_Rates"]),                  # rate beyond the kernel's bound
           ({"Upsample_Kernel_Sizes": [16, 16, 4, 20]}, {}, ["Vocoder.Upsample_Kernel_Sizes"]),                                # 10 taps per phase
           ({"Resblock_Kernel_Sizes": [3, 6, 11]}, {}, ["Vocoder.Resblock_Kernel_Sizes"]),                                     # even
           ({"Resblock_Kernel_Sizes": [3, 7, 13]}, {}, ["Vocoder.Resblock_Kernel_Sizes"]),                                     # taps beyond the bound
           ({"Resblock_Kernel_Sizes": [3, 7]}, {}, ["Vocoder.Resblock_Kernel_Sizes", "Vocoder.Resblock_Dilations"]),           # lengths differ
           ({"Resblock_Dilations": [[1, 3, 5], [1, 3, 5], []]}, {}, ["Vocoder.Resblock_Dilations"]),
           ({"Resblock_Dilations": [[1, 3, 5], [1, 3, 17], [1, 3, 5]]}, {}, ["Vocoder.Resblock_Dilations"]),                   # dilation beyond the bound
           ({"Resblock_Dilations": [[1, 3, 5], [0, 3, 5], [1, 3, 5]]}, {}, ["Vocoder.Resblock_Dilations"]),
           ({"Initial_Channels": 128}, {}, ["Vocoder.Initial_Channels"]),                                                      # 128 / 16 = 8 channels at the end
           ({"Initial_Channels": 1024}, {}, ["Vocoder.Initial_Channels"]),
           ({}, {"Mel_Dim": 78}, ["Sound.Mel_Dim"]),
           ({"Resblock": "3"}, {}, ["Vocoder.Resblock"]),
           ({"Precision": "bf16"}, {}, ["Vocoder.Precision"]),
           ({"Type": "PWG"}, {}, ["Vocoder.Type"])]
    for voc, sound, keys in bad:
        with pytest.raises(ValueError) as e:
            hifigan_geometry(_hp(dict({"Type": "HiFiGAN"}, **voc), **sound))
        assert all(k in str(e.value) for k in keys), (voc, sound, str(e.value))
    assert hifigan_geometry(_hp({"Type": "HiFiGAN", "Resblock": 2}))["resblock"] == "2"                   # a yaml integer is taken too
    with pytest.raises(ValueError, match="Vocoder.Type"):                                                # the Parallel WaveGAN side stays PWG-only
        pwg_geometry(_hp({"Type": "HiFiGAN"}))


def test_loader_folds_weight_norm_finds_nesting_and_names_bad_keys():
    from glow_tts_amd.vocoder import hifigan_expected_shapes, hifigan_init, hifigan_load
    for cfg in (H.NARROW, H.ODD, H.DEFAULT):
        assert hifigan_expected_shapes(_geo(cfg)) == H.shapes(cfg)
    cfg = H.NARROW
    geo = _geo(cfg)
    sd = H.random_state_dict(cfg, 9)
    mine = hifigan_init(geo, 9)                                              # the product's initialiser draws the same tensors in the same order
    assert list(mine) == list(sd) and all(torch.equal(mine[k], sd[k]) for k in sd)
    plain = hifigan_load(sd, geo)
    assert set(plain) == set(sd) and all(torch.equal(plain[k], sd[k]) for k in sd)
    wn = {}
    for k, t in sd.items():                                                  # v = 2 w, g = |w| over everything but dim 0: the fold gives w back
        if k.endswith(".weight"):
            wn[k + "_v"] = 2.0 * t
            wn[k + "_g"] = t.double().reshape(t.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (t.dim() - 1))
        else:
            wn[k] = t
    assert wn["ups.0.weight_g"].shape == (64, 1, 1)                          # a transposed convolution's g is per INPUT channel (dim 0), as torch has it
    folded = hifigan_load(wn, geo)
    assert all(folded[k].dtype == torch.float32 and (folded[k] - sd[k]).abs().max() <= 1e-7 * sd[k].abs().max() for k in sd)
    ups = torch.nn.utils.parametrizations.weight_norm(torch.nn.ConvTranspose1d(64, 32, 4, 2, padding=1))  # torch's own pair for a transposed convolution
    g0, v0 = ups.parametrizations.weight.original0, ups.parametrizations.weight.original1
    with torch.no_grad():
        g0.mul_(1.7)                                                         # (a fresh pair has g = |v|: make the fold do something)
        want = ups.weight.detach().clone()
    pair = dict(sd)
    del pair["ups.0.weight"]
    pair["ups.0.weight_g"], pair["ups.0.weight_v"] = g0.detach(), v0.detach()
    assert (hifigan_load(pair, geo)["ups.0.weight"] - want).abs().max() <= 1e-6 * want.abs().max()
    for nest in (lambda d: {"generator": d}, lambda d: {"Generator": d}, lambda d: {"model": {"generator": d}}, lambda d: {"model": d},
                 lambda d: {"model": {"Generator": d}, "steps": 3}):
        got = hifigan_load(nest(sd), geo)
        assert all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="no HiFi-GAN generator"):
        hifigan_load({"mpd": {}, "msd": {}}, geo)
    missing = dict(sd)
    del missing["resblocks.2.convs1.1.bias"]
    with pytest.raises(ValueError, match=re.escape("resblocks.2.convs1.1.bias")):
        hifigan_load(missing, geo)
    surplus = dict(sd, **{"resblocks.0.convs2.0.weight": torch.zeros(32, 32, 3)})                        # a type-'1' tensor in a type-'2' generator
    with pytest.raises(ValueError, match=re.escape("resblocks.0.convs2.0.weight")):
        hifigan_load(surplus, geo)
    shaped = dict(sd, **{"ups.1.weight": torch.zeros(16, 32, 4)})                                        # Conv1d's order where ConvTranspose1d's is due
    with pytest.raises(ValueError, match=re.escape("ups.1.weight")):
        hifigan_load(shaped, geo)
    lone = dict(sd, **{"conv_pre.weight_g": torch.ones(64, 1, 1)})
    with pytest.raises(ValueError, match="conv_pre.weight"):
        hifigan_load(lone, geo)


def test_constructor_checks_geometry_checkpoint_and_precision_before_the_device():
    from glow_tts_amd.vocoder import HiFiGAN, ParallelWaveGAN, make_vocoder, vocoder_kind
    with pytest.raises(ValueError, match="Vocoder.Resblock_Kernel_Sizes"):
        HiFiGAN(_hp({"Type": "HiFiGAN", "Resblock_Kernel_Sizes": [3, 8, 11]}), "cuda:0", state_dict={})
    with pytest.raises(ValueError, match="Vocoder.Checkpoint_Path"):
        HiFiGAN(_hp({"Type": "HiFiGAN"}), "cuda:0")
    with pytest.raises(ValueError, match="Vocoder.Precision"):
        HiFiGAN(_hp({"Type": "HiFiGAN"}), "cuda:0", state_dict={}, precision="bf16")
    with pytest.raises(ValueError, match="no HiFi-GAN generator"):
        HiFiGAN(_hp({"Type": "HiFiGAN"}), "cuda:0", state_dict={"generator": {}})
    with pytest.raises(ValueError, match="Vocoder.Type"):                    # Train_PWG.py's generator refuses a HiFi-GAN block
        ParallelWaveGAN(_hp({"Type": "HiFiGAN"}), "cuda:0", state_dict={}, trainable=True)
    # the choice of a vocoder
    hi, pwg, none = _hp({"Type": "HiFiGAN"}), _hp({"Type": "PWG"}), _hp()
    assert vocoder_kind(hi) == "hifigan" and vocoder_kind(pwg) == "pwg" and vocoder_kind(_hp({})) == "pwg" and vocoder_kind(none) == "griffin_lim"
    assert vocoder_kind(none, checkpoint="v.pt") == "pwg" and vocoder_kind(hi, checkpoint="v.pt") == "hifigan"
    assert vocoder_kind(hi, "griffin_lim") == "griffin_lim" and vocoder_kind(none, "hifigan") == "hifigan" and vocoder_kind(hi, "pwg") == "pwg"
    with pytest.raises(ValueError, match="wavernn"):
        vocoder_kind(none, "wavernn")
    with pytest.raises(ValueError, match="Vocoder.Checkpoint_Path"):         # chosen, then refused before the device: no checkpoint
        make_vocoder(hi, "cuda:0")
    with pytest.raises(ValueError, match="Vocoder.Type"):                    # the flag against the block
        make_vocoder(pwg, "cuda:0", "hifigan", checkpoint=os.path.join(REPO, "no_such_file.pt"))
    with pytest.raises(ValueError, match="Vocoder.Precision"):
        make_vocoder(hi, "cuda:0", precision="bf16")


def test_parser_takes_hifigan_and_still_rejects_others():
    from glow_tts_amd.inferencer import build_parser
    a = build_parser().parse_args(["-c", "x.pt", "--wav", "--vocoder", "hifigan", "--vocoder-checkpoint", "g.pt"])
    assert (a.vocoder, a.vocoder_checkpoint) == ("hifigan", "g.pt")
    assert build_parser().parse_args(["-c", "x.pt", "--vocoder", "pwg"]).vocoder == "pwg" and build_parser().parse_args(["-c", "x.pt"]).vocoder is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-c", "x.pt", "--vocoder", "wavernn"])


def test_abi_additions_are_in_header_and_table_and_the_version_stays():
    from glow_tts_amd import abi
    text = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    for n in ("glowtts_hifigan_supported", "glowtts_hifigan_conv", "glowtts_hifigan_upsample", "glowtts_hifigan_post"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert n in abi.SIGNATURES
    assert "glowtts_hifigan_supported" in abi.VALUE_RETURNING and not {"glowtts_hifigan_conv", "glowtts_hifigan_upsample", "glowtts_hifigan_post"} & abi.VALUE_RETURNING
    assert abi.ABI_VERSION == 7 and re.search(r"#define\s+GLOWTTS_ABI_VERSION\s+7\b", text)


def test_supported_and_argument_validation_on_the_host():
    """glowtts_hifigan_supported, and the entry points refuse bad sizes with the argument error before anything is launched (no device is touched)."""
    from glow_tts_amd import _lib, abi
    L = _lib.lib()
    S = L.glowtts_hifigan_supported
    for args in ((80, 512, 7, 1, 0), (8, 64, 7, 1, 0), (256, 256, 11, 5, 0), (32, 32, 11, 16, 0), (512, 512, 3, 1, 0), (32, 1, 7, 1, 0),
                 (512, 256, 16, 1, 8), (64, 32, 7, 1, 3), (32, 16, 11, 1, 5), (64, 32, 4, 1, 2), (16, 16, 1, 1, 1)):
        assert S(*args) == 1, args
    for args in ((78, 512, 7, 1, 0), (80, 520, 7, 1, 0), (80, 24, 7, 1, 0), (1024, 512, 7, 1, 0), (64, 64, 13, 1, 0), (64, 64, 6, 1, 0), (64, 64, 3, 17, 0),
                 (64, 64, 3, 0, 0), (32, 1, 7, 2, 0), (64, 32, 2, 1, 4), (64, 32, 5, 1, 2), (64, 32, 34, 1, 17), (64, 32, 20, 1, 2), (64, 32, 4, 2, 2),
                 (64, 32, 4, 1, -1)):
        assert S(*args) == 0, args
    p = 4096                                                                 # a non-null address that is never dereferenced: every call below is refused
    conv = lambda **k: L.glowtts_hifigan_conv(*[dict(dict(i=p, w=p, b=p, r=None, o=p + 4, n=p, B=1, L=4, m=8, ci=64, co=64, t=7, d=3, s=0.1, a=0, v=1.0, cf=0,
                                                          st=None), **k)[q] for q in "i w b r o n B L m ci co t d s a v cf st".split()])
    assert conv(t=13) == conv(t=4) == conv(d=17) == conv(ci=62) == conv(co=40) == conv(co=1) == abi.E_ARG
    assert conv(o=p) == conv(B=0) == conv(L=1 << 24, m=256) == conv(a=3) == conv(a=2, v=0.0) == conv(i=None) == conv(n=None) == abi.E_ARG
    up = lambda **k: L.glowtts_hifigan_upsample(*[dict(dict(i=p, w=p, b=p, o=p + 4, n=p, B=1, L=4, m=8, ci=64, co=32, t=16, u=8, s=0.1, st=None), **k)[q]
                                                  for q in "i w b o n B L m ci co t u s st".split()])
    assert up(t=4) == up(t=17) == up(u=0) == up(u=32, t=64) == up(co=8) == up(o=p) == up(L=1 << 24, m=16) == up(w=None) == abi.E_ARG
    post = lambda **k: L.glowtts_hifigan_post(*[dict(dict(i=p, w=p, b=p, o=p, n=p, B=1, L=4, m=256, ci=32, t=7, s=0.01, st=None), **k)[q]
                                                for q in "i w b o n B L m ci t s st".split()])
    assert post(ci=30) == post(t=6) == post(t=13) == post(B=70000) == post(o=None) == abi.E_ARG


def test_restatement_guards_hold_for_the_gpu_cases():
    """The seeds the GPU tests use give non-degenerate cases: 0 < e32 < 1e-3 and max |ref64| > 1e-3, for the waveform and for the rows entering conv_post
    (the narrow and the odd net: the cheap ones here)."""
    for cfg, L, seed in ((H.NARROW, 5, 15), (H.NARROW, 1, 11), (H.ODD, 2, 12)):
        sd = H.random_state_dict(cfg, 1234)
        mel = H.uniform_mel(cfg["A"], L, seed)
        (w64, r64), (w32, r32) = H.generator(sd, cfg, mel), H.generator(sd, cfg, mel, torch.float32)
        assert w32.dtype == r32.dtype == torch.float32 and w64.shape == (L * H.hop(cfg),)
        for a64, a32 in ((w64, w32), (r64, r32)):
            _, e32 = H.errors(a32, a64, a32)
            assert 0 < e32 < 1e-3 and float(a64.abs().max()) > 1e-3


def test_hifigan_kernels_use_no_scratch_memory(tmp_path):
    """As test_pwg_cpu.test_pwg_kernels_use_no_scratch_memory, for the kernels of csrc/hifigan_ops.hip (code-object metadata; nothing is executed)."""
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    assert os.path.exists(f"{llvm}/llvm-objdump") and os.path.exists(f"{llvm}/llvm-readelf"), "ROCm LLVM tools not found"
    shutil.copy(os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    found = {"hifigan_conv_kernel": 0, "hifigan_upsample_kernel": 0, "hifigan_post_kernel": 0}
    for f in [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        for name, scratch, vgpr in re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S):
            for h in found:
                if h in name:
                    found[h] += 1
                    print(f"{name}: {vgpr} VGPRs, {scratch} bytes of scratch")
                    assert int(scratch) == 0, f"{name} spills: {scratch} bytes of scratch per lane at {vgpr} VGPRs"
    assert found == {"hifigan_conv_kernel": 4, "hifigan_upsample_kernel": 4, "hifigan_post_kernel": 1}, found
