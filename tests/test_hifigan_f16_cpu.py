"""fp16 inference mode of the HiFi-GAN vocoder, host side (no GPU): the setting, the constructor's and the parser's handling of it, the refusals (all before
the device is touched), the ABI additions, the host-side argument checks, the kernels' register allocation, the weight packing, the restatement's rounding,
and the guard that the restatement itself (emu32, emu32b of tests/hifigan_f16_ref.py) satisfies the bars that tests/test_gpu_hifigan_f16.py sets for the
kernels."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hifigan_f16_cases as C  # noqa: E402
import hifigan_f16_ref as R  # noqa: E402
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


# ---------------------------------------------------------------------------------------------------------------- setting, constructor, parser
def test_precision_setting_is_validated_and_defaults_to_f32():
    from glow_tts_amd.vocoder import HIFIGAN_DEFAULTS, HIFIGAN_PRECISIONS, hifigan_geometry, hifigan_settings
    assert HIFIGAN_DEFAULTS["Precision"] == "f32" and HIFIGAN_PRECISIONS == ("f32", "f16")
    assert hifigan_geometry(_hp({"Type": "HiFiGAN"}))["precision"] == "f32"
    hp = _hp({"Type": "HiFiGAN", "Precision": "f16"})
    assert hifigan_geometry(hp)["precision"] == "f16" and hifigan_settings(hp)["Precision"] == "f16"
    for bad in ("bf16", "fp16", "F16", "", None, 16):
        with pytest.raises(ValueError, match=r"Vocoder\.Precision"):
            hifigan_geometry(_hp({"Type": "HiFiGAN", "Precision": bad}))
    text = open(os.path.join(REPO, "glow_tts_amd", "Hyper_Parameters.default.yaml")).read()
    assert re.search(r"(?m)^#.*'f16'", text)                                  # documented in the commented Vocoder block


def test_refusals_are_raised_before_the_device_is_touched():
    from glow_tts_amd.vocoder import HiFiGAN, ParallelWaveGAN, make_vocoder
    hi = _hp({"Type": "HiFiGAN"})
    with pytest.raises(ValueError, match="trainable.*f32"):                   # training stays f32
        HiFiGAN(hi, "cuda:0", state_dict={}, trainable=True, precision="f16")
    with pytest.raises(ValueError, match=r"Vocoder\.Precision"):              # bf16 stays refused
        HiFiGAN(hi, "cuda:0", state_dict={}, precision="bf16")
    with pytest.raises(ValueError, match=r"Vocoder\.Precision"):
        HiFiGAN(_hp({"Type": "HiFiGAN", "Precision": "bf16"}), "cuda:0", state_dict={})
    with pytest.raises(ValueError, match=r"Vocoder\.Precision"):
        make_vocoder(hi, "cuda:0", precision="bf16")
    with pytest.raises(ValueError, match=r"Vocoder\.Precision"):              # f16 is not the Parallel WaveGAN's mode
        ParallelWaveGAN(_hp({}), "cuda:0", state_dict={}, precision="f16")
    with pytest.raises(ValueError, match=r"Vocoder\.Precision"):
        ParallelWaveGAN(_hp({"Precision": "f16"}), "cuda:0", state_dict={})
    with pytest.raises(ValueError, match=r"Vocoder\.Precision"):
        make_vocoder(_hp({"Precision": "f32"}), "cuda:0", "pwg", precision="f16")
    # unsupported sizes name their yaml keys, by the key and by the argument
    for block, sound, key in (({"Initial_Channels": 1024}, {}, "Vocoder.Initial_Channels"), ({"Resblock_Kernel_Sizes": [3, 13, 11]}, {}, "Vocoder.Resblock_Kernel_Sizes"),
                              ({"Resblock_Dilations": [[1, 3, 17]] * 3}, {}, "Vocoder.Resblock_Dilations"), ({}, {"Mel_Dim": 78}, "Sound.Mel_Dim"),
                              ({"Upsample_Rates": [32, 8], "Upsample_Kernel_Sizes": [64, 16]}, {}, "Vocoder.Upsample_Rates")):
        with pytest.raises(ValueError, match=re.escape(key)):
            HiFiGAN(_hp(dict({"Type": "HiFiGAN", "Precision": "f16"}, **block), **sound), "cuda:0", state_dict={})
        with pytest.raises(ValueError, match=re.escape(key)):
            HiFiGAN(_hp(dict({"Type": "HiFiGAN"}, **block), **sound), "cuda:0", state_dict={}, precision="f16")
    # a valid precision gets as far as the checkpoint, by the argument and by the key
    with pytest.raises(ValueError, match=r"Vocoder\.Checkpoint_Path"):
        HiFiGAN(hi, "cuda:0", precision="f16")
    with pytest.raises(ValueError, match=r"Vocoder\.Checkpoint_Path"):
        make_vocoder(_hp({"Type": "HiFiGAN", "Precision": "f16"}), "cuda:0")
    with pytest.raises(ValueError, match="no HiFi-GAN generator"):
        HiFiGAN(hi, "cuda:0", state_dict={"generator": {}}, precision="f16")
    src = open(os.path.join(REPO, "glow_tts_amd", "vocoder.py")).read()
    assert "training stays f32" in src


def test_parser_and_inferencer_take_f16():
    from glow_tts_amd.inferencer import Inferencer, build_parser
    for mode in (["--wav"], ["--convert", "list.tsv", "--wav"], ["--vocode", "list.txt"]):
        a = build_parser().parse_args(["-c", "x.pt"] + mode + ["--vocoder", "hifigan", "--vocoder-precision", "f16"])
        assert (a.vocoder, a.vocoder_precision) == ("hifigan", "f16")
    assert build_parser().parse_args(["-c", "x.pt", "--vocoder-precision", "bf16"]).vocoder_precision == "bf16"
    assert build_parser().parse_args(["-c", "x.pt"]).vocoder_precision is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-c", "x.pt", "--vocoder-precision", "fp16"])
    import inspect
    assert inspect.signature(Inferencer.__init__).parameters["vocoder_precision"].default is None
    with pytest.raises(ValueError, match="vocoder_precision"):               # checked first, before the checkpoint is opened
        Inferencer("no_such_checkpoint.pt", hp=_hp({"Type": "HiFiGAN"}), vocoder_precision="half")


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_additions_are_in_header_and_table_and_the_version_stays():
    from glow_tts_amd import abi
    text = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    for n in ("glowtts_hifigan_supported_f16", "glowtts_hifigan_conv_f16", "glowtts_hifigan_upsample_f16"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert n in abi.SIGNATURES
    assert abi.SIGNATURES["glowtts_hifigan_conv_f16"] == abi.SIGNATURES["glowtts_hifigan_conv"]
    assert abi.SIGNATURES["glowtts_hifigan_upsample_f16"] == abi.SIGNATURES["glowtts_hifigan_upsample"]
    assert "glowtts_hifigan_supported_f16" in abi.VALUE_RETURNING and not {"glowtts_hifigan_conv_f16", "glowtts_hifigan_upsample_f16"} & abi.VALUE_RETURNING
    assert abi.ABI_VERSION == 7 and re.search(r"#define\s+GLOWTTS_ABI_VERSION\s+7\b", text)
    assert re.search(r"const uint16_t \*w", text[text.index("int glowtts_hifigan_conv_f16"):])


def test_supported_and_argument_validation_on_the_host():
    """glowtts_hifigan_supported_f16 is glowtts_hifigan_supported on every size tried (the fp16 tile is the smaller one), and the entry points refuse bad
    arguments with the argument error before anything is launched (no device is touched)."""
    from glow_tts_amd import _lib, abi
    L = _lib.lib()
    good = ((80, 512, 7, 1, 0), (8, 64, 7, 1, 0), (256, 256, 11, 5, 0), (32, 32, 11, 16, 0), (512, 512, 11, 16, 0), (32, 1, 7, 1, 0), (512, 256, 16, 1, 8),
            (64, 32, 7, 1, 3), (32, 16, 11, 1, 5), (64, 32, 4, 1, 2), (16, 16, 1, 1, 1))
    bad = ((78, 512, 7, 1, 0), (80, 520, 7, 1, 0), (80, 24, 7, 1, 0), (1024, 512, 7, 1, 0), (64, 64, 13, 1, 0), (64, 64, 6, 1, 0), (64, 64, 3, 17, 0),
           (64, 64, 3, 0, 0), (32, 1, 7, 2, 0), (64, 32, 2, 1, 4), (64, 32, 5, 1, 2), (64, 32, 34, 1, 17), (64, 32, 20, 1, 2), (64, 32, 4, 2, 2), (64, 32, 4, 1, -1))
    for args in good + bad:
        assert L.glowtts_hifigan_supported_f16(*args) == L.glowtts_hifigan_supported(*args) == int(args in good), args
    p = 4096                                                                 # a non-null address that is never dereferenced: every call below is refused
    conv = lambda **k: L.glowtts_hifigan_conv_f16(*[dict(dict(i=p, w=p, b=p, r=None, o=p + 4, n=p, B=1, L=4, m=8, ci=64, co=64, t=7, d=3, s=0.1, a=0, v=1.0, cf=0,
                                                              st=None), **k)[q] for q in "i w b r o n B L m ci co t d s a v cf st".split()])
    assert conv(t=13) == conv(t=4) == conv(d=17) == conv(ci=62) == conv(co=40) == conv(co=1) == abi.E_ARG
    assert conv(o=p) == conv(B=0) == conv(L=1 << 24, m=256) == conv(a=3) == conv(a=2, v=0.0) == conv(i=None) == conv(w=None) == conv(n=None) == abi.E_ARG
    up = lambda **k: L.glowtts_hifigan_upsample_f16(*[dict(dict(i=p, w=p, b=p, o=p + 4, n=p, B=1, L=4, m=8, ci=64, co=32, t=16, u=8, s=0.1, st=None), **k)[q]
                                                      for q in "i w b o n B L m ci co t u s st".split()])
    assert up(t=4) == up(t=17) == up(u=0) == up(u=32, t=64) == up(co=8) == up(o=p) == up(L=1 << 24, m=16) == up(w=None) == abi.E_ARG


def test_f16_kernels_use_no_scratch_memory(tmp_path):
    """As test_hifigan_cpu.test_hifigan_kernels_use_no_scratch_memory, for csrc/hifigan_f16_ops.hip (code-object metadata; nothing is executed).  The widest
    layout (4, 2) must keep three waves per SIMD: at most 168 VGPRs."""
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    assert os.path.exists(f"{llvm}/llvm-objdump") and os.path.exists(f"{llvm}/llvm-readelf"), "ROCm LLVM tools not found"
    shutil.copy(os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    found = {"hifigan_conv_f16_kernel": 0, "hifigan_upsample_f16_kernel": 0}
    for f in [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        for name, scratch, vgpr in re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S):
            for h in found:
                if h in name:
                    found[h] += 1
                    print(f"{name}: {vgpr} VGPRs, {scratch} bytes of scratch")
                    assert int(scratch) == 0, f"{name} spills: {scratch} bytes of scratch per lane at {vgpr} VGPRs"
                    assert int(vgpr) <= 168, f"{name}: {vgpr} VGPRs leave fewer than three waves per SIMD"
    assert found == {"hifigan_conv_f16_kernel": 4, "hifigan_upsample_f16_kernel": 4}, found


# ---------------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("cin, cout, taps, transposed", [(8, 64, 7, False), (80, 512, 7, False), (256, 256, 11, False), (12, 16, 3, False), (64, 32, 16, True),
                                                         (16, 16, 11, True)])
def test_packed_image_is_the_rounded_weights_with_zero_padding_rows(cin, cout, taps, transposed):
    from glow_tts_amd.vocoder import hifigan_conv_image, hifigan_pack_f16, hifigan_unpack_f16, hifigan_up_image, pad32
    g = torch.Generator().manual_seed(cin + cout + taps)
    w = torch.randn((cin, cout, taps) if transposed else (cout, cin, taps), generator=g) * 0.3
    w.view(-1)[:3] = torch.tensor([1.0e6, -7.0e4, 3.0e-6])                    # clamped, clamped, an fp16 subnormal
    image = hifigan_pack_f16((hifigan_up_image if transposed else hifigan_conv_image)(w), taps)
    Cp = pad32(cin)
    assert Cp % 32 == 0 and 0 <= Cp - cin < 32 and Cp == cin // 64 * 64 + pad32(cin % 64)           # 64-channel chunks, the last padded to the k step
    assert image.dtype == torch.float16 and image.is_contiguous() and tuple(image.shape) == (taps, Cp // 8, cout, 8)
    back = hifigan_unpack_f16(image)                                          # [taps, Cp, Cout]
    want = R.r16(w).permute(2, 0, 1) if transposed else R.r16(w).permute(2, 1, 0)                   # [taps, Cin, Cout]
    assert back.shape == (taps, Cp, cout) and torch.equal(back[:, :cin], want) and bool((back[:, cin:] == 0).all())
    assert float(back.abs().max()) == 65504.0 and bool(torch.isfinite(back).all())
    flat = image.reshape(-1).float()                                          # the address the kernel computes: ((tap Cp / 8 + k / 8) Cout + n) 8 + k % 8
    for j, k, n in ((0, 0, 0), (1, 7, 1), (taps - 1, 8 % cin, 0), (taps - 1, cin - 1, cout - 1), (taps // 2, cin // 2, cout // 3), (taps - 1, Cp - 1, cout - 1)):
        assert float(flat[((j * (Cp // 8) + k // 8) * cout + n) * 8 + k % 8]) == (float(want[j, k, n]) if k < cin else 0.0), (j, k, n)


# ---------------------------------------------------------------------------------------------------------------- the restatement alone
def test_r16_clamps_and_rounds_to_nearest_even_and_keeps_or_flushes_subnormals():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -30, -(1.0 + 2.0 ** -11), 1.0e6, -1.0e6, 65519.0, 65520.0, 3.0e-6,
                      2.0 ** -14, 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40], dtype=torch.float64)
    sub = round(3.0e-6 / 2.0 ** -24) * 2.0 ** -24
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10, -1.0, 65504.0, -65504.0, 65504.0, 65504.0, sub, 2.0 ** -14, 0.0, 2.0 ** -24], dtype=torch.float64)
    assert torch.equal(R.r16(t), want) and R.r16(t).dtype == torch.float64 and R.r16(t.float()).dtype == torch.float32
    flushed = want.clone()
    flushed[9] = flushed[12] = 0.0
    assert torch.equal(R.r16(t, flush=True), flushed)
    x = torch.tensor([[-1.0, 2.0, -1.0e6]])
    assert torch.equal(R.operand(x, 0.1), R.r16(torch.tensor([[-1.0 * torch.tensor(0.1).item(), 2.0, -65504.0]]))) and R.operand(x.double(), None).dtype == torch.float64


def test_restated_operators_agree_across_realisations_and_with_the_unrounded_ones_on_fp16_inputs():
    """On inputs that are fp16 numbers already the contract rounds nothing: emu64 is hifigan_ref's float64 operator; emu32b is emu32 to float32 accuracy."""
    g = torch.Generator().manual_seed(1)
    e64, e32, e32b = R.emus()
    x, w, b = R.r16(torch.randn(80, 30, generator=g)), R.r16(torch.randn(24, 80, 7, generator=g) * 0.1), torch.randn(24, generator=g)
    assert torch.equal(e64.conv(x, w, b, 3), H.conv(x.double(), w.double(), b.double(), 3))
    blocked = Rb = R.Emu(torch.float64, True).conv(x, w, b, 3)
    assert float((blocked - e64.conv(x, w, b, 3)).abs().max()) < 1e-12 and Rb.dtype == torch.float64
    assert float((e32b.conv(x, w, b, 3).double() - e64.conv(x, w, b, 3)).abs().max()) < 1e-5
    wt = R.r16(torch.randn(80, 16, 7, generator=g) * 0.1)
    xl = torch.where(x > 0, x, x * 0.5)                                       # slope 0.5 keeps fp16 numbers fp16 numbers
    assert float((e64.upsample(x, wt, b[:16], 3, 0.5) - H.upsample(xl.double(), wt.double(), b[:16].double(), 3, 1.0)).abs().max()) < 1e-12
    assert float((R.Emu(torch.float64, True).upsample(x, wt, b[:16], 3) - e64.upsample(x, wt, b[:16], 3)).abs().max()) < 1e-12
    assert float((e32.upsample(x, wt, b[:16], 3).double() - e64.upsample(x, wt, b[:16], 3)).abs().max()) < 1e-5


@pytest.mark.parametrize("name, seed, lengths", C.GENERATOR_CASES)
def test_generator_restatements_satisfy_the_gpu_bars(name, seed, lengths):
    """emu32 and emu32b themselves under bars (a) and (b), with the guards, for the waveform and for the rows entering conv_post of every GPU case."""
    for L in lengths:
        ref = C.reference(name, seed, L)
        for i, what in enumerate(("wav", "rows")):
            scale, e_f16, e32 = C.figures(ref, i)
            print(f"{name} seed {seed} L = {L} {what}: max|ref64| {scale:.3e}  e_f16 / scale {e_f16 / scale:.3e}  e_f16 / e32 {e_f16 / e32:.0f}")
            for v in ("emu32", "emu32b"):
                assert ref[v][i].dtype == torch.float32
                C.check_generator(f"{v} {name} seed {seed} L = {L} {what}", ref[v][i], ref, i, name != "default")
