"""bf16 inference mode of the neural vocoder, host side (no GPU): the setting, the constructor's and the parser's handling of it, the ABI additions, the
host-side argument checks, the kernel's register allocation, the weight packing, and the guard that the restatement itself (emu32, emu32b of
tests/pwg_bf16_ref.py) satisfies the bars that tests/test_gpu_pwg_bf16.py sets for the kernel."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pwg_bf16_cases as C  # noqa: E402
import pwg_bf16_ref as E  # noqa: E402
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


# ---------------------------------------------------------------------------------------------------------------- setting, constructor, parser
def test_precision_setting_is_validated_and_defaults_to_f32():
    from glow_tts_amd.vocoder import PWG_DEFAULTS, pwg_geometry, pwg_settings
    assert PWG_DEFAULTS["Precision"] == "f32"
    assert pwg_geometry(_hp({}))["precision"] == "f32" and pwg_geometry(_hp())["precision"] == "f32"           # an absent key, an absent block
    assert pwg_geometry(_hp({"Precision": "bf16"}))["precision"] == "bf16" and pwg_settings(_hp({"Precision": "bf16"}))["Precision"] == "bf16"
    for bad in ("fp16", "BF16", "", None, 16):
        with pytest.raises(ValueError, match=r"Vocoder\.Precision"):
            pwg_geometry(_hp({"Precision": bad}))
    from glow_tts_amd.vocoder import pwg_bf16_geometry
    pwg_bf16_geometry({"R": 128, "A": 80})                                    # 62 KB
    with pytest.raises(ValueError) as e:                                      # (no size that f32 takes reaches this: the bf16 tile is the smaller one)
        pwg_bf16_geometry({"R": 256, "A": 256})
    assert all(k in str(e.value) for k in ("Vocoder.Precision", "Vocoder.Residual_Channels", "Sound.Mel_Dim"))
    text = open(os.path.join(REPO, "glow_tts_amd", "Hyper_Parameters.default.yaml")).read()
    assert re.search(r"(?m)^#\s+Precision: 'f32'", text)                                                       # documented in the commented Vocoder block


def test_constructor_refuses_bf16_training_and_bad_precisions_before_the_device():
    from glow_tts_amd.vocoder import ParallelWaveGAN
    with pytest.raises(ValueError, match="trainable"):
        ParallelWaveGAN(_hp({}), "cuda:0", state_dict={}, trainable=True, precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        ParallelWaveGAN(_hp({}), "cuda:0", state_dict={}, precision="fp16")
    with pytest.raises(ValueError, match=r"Vocoder\.Precision"):
        ParallelWaveGAN(_hp({"Precision": "half"}), "cuda:0", state_dict={})
    with pytest.raises(ValueError, match=r"Vocoder\.Checkpoint_Path"):                                       # a valid precision gets as far as the checkpoint
        ParallelWaveGAN(_hp({}), "cuda:0", precision="bf16")
    src = open(os.path.join(REPO, "glow_tts_amd", "pwg_trainer.py")).read()
    assert re.search(r"ParallelWaveGAN\([^\n]*trainable=True[^\n]*precision=\"f32\"", src)                    # the trainer asks for f32 explicitly


def test_parser_and_inferencer_take_the_vocoder_precision():
    from glow_tts_amd.inferencer import Inferencer, build_parser
    a = build_parser().parse_args(["-c", "x.pt", "--wav", "--vocoder", "pwg", "--vocoder-precision", "bf16"])
    assert a.vocoder_precision == "bf16"
    assert build_parser().parse_args(["-c", "x.pt", "--vocoder-precision", "f32"]).vocoder_precision == "f32"
    assert build_parser().parse_args(["-c", "x.pt"]).vocoder_precision is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-c", "x.pt", "--vocoder-precision", "fp16"])
    import inspect
    assert inspect.signature(Inferencer.__init__).parameters["vocoder_precision"].default is None


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_additions_are_in_header_and_table_and_the_version_stays():
    from glow_tts_amd import abi
    text = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    for n in ("glowtts_pwg_supported_bf16", "glowtts_pwg_layer_bf16"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert n in abi.SIGNATURES
    assert abi.SIGNATURES["glowtts_pwg_layer_bf16"] == abi.SIGNATURES["glowtts_pwg_layer"]
    assert abi.ABI_VERSION == 7 and re.search(r"#define\s+GLOWTTS_ABI_VERSION\s+7\b", text)
    assert "glowtts_pwg_layer_bf16" in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_supported_and_argument_validation_on_the_host():
    """glowtts_pwg_supported_bf16, and glowtts_pwg_layer_bf16 refuses bad arguments with the argument error before anything is launched (no device is touched)."""
    from glow_tts_amd import _lib, abi
    L = _lib.lib()
    for cfg in C.CFGS.values():
        assert L.glowtts_pwg_supported_bf16(cfg["R"], cfg["G"], cfg["S"], cfg["A"], 2 ** (cfg["layers"] // cfg["stacks"] - 1)) == 1, cfg
    assert L.glowtts_pwg_supported_bf16(64, 128, 64, 80, 1024) == 1
    for args in ((64, 96, 64, 80, 512), (40, 80, 64, 80, 1), (64, 128, 24, 80, 1), (64, 128, 64, 78, 1), (64, 128, 64, 80, 2048), (64, 128, 64, 80, 0),
                 (512, 1024, 64, 80, 1), (256, 512, 64, 256, 1)):
        assert L.glowtts_pwg_supported_bf16(*args) == 0, args
    p = 4096                                                                 # a non-null address that is never dereferenced: every call below is refused
    ok = (1, 4, 256, 64, 64, 80, 1, 0, None)
    for i in range(9):                                                       # every pointer NULL in turn
        ptrs = [p, p, p, p, p, p, p + 4, p, p]
        ptrs[i] = None
        assert L.glowtts_pwg_layer_bf16(*ptrs, *ok) == abi.E_ARG, i
    assert L.glowtts_pwg_layer_bf16(p, p, p, p, p, p, p, p, p, *ok) == abi.E_ARG                                          # in place
    assert L.glowtts_pwg_layer_bf16(p, p, p, p, p, p, p + 4, p, p, 1, 4, 256, 64, 64, 80, 2048, 0, None) == abi.E_ARG     # dilation
    assert L.glowtts_pwg_layer_bf16(p, p, p, p, p, p, p + 4, p, p, 1, 1 << 24, 256, 64, 64, 80, 1, 0, None) == abi.E_ARG  # Lmax * hop beyond 2^30
    assert L.glowtts_pwg_layer_bf16(p, p, p, p, p, p, p + 4, p, p, 0, 4, 256, 64, 64, 80, 1, 0, None) == abi.E_ARG        # B
    assert L.glowtts_pwg_layer_bf16(p, p, p, p, p, p, p + 4, p, p, 1, 4, 256, 40, 64, 80, 1, 0, None) == abi.E_ARG        # R
    assert L.glowtts_pwg_layer_bf16(p, p, p, p, p, p, p + 4, p, p, 1, 4, 256, 64, 64, 78, 1, 0, None) == abi.E_ARG        # A


def test_bf16_layer_kernel_uses_no_scratch_memory(tmp_path):
    """As test_pwg_cpu.test_pwg_kernels_use_no_scratch_memory, for csrc/pwg_bf16_ops.hip (code-object metadata; nothing is executed)."""
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    assert os.path.exists(f"{llvm}/llvm-objdump") and os.path.exists(f"{llvm}/llvm-readelf"), "ROCm LLVM tools not found"
    shutil.copy(os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    found = 0
    for f in [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        for name, scratch, vgpr in re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S):
            if "pwg_layer_bf16_kernel" in name:
                found += 1
                print(f"{name}: {vgpr} VGPRs, {scratch} bytes of scratch")
                assert int(scratch) == 0, f"{name} spills: {scratch} bytes of scratch per lane at {vgpr} VGPRs"
                assert int(vgpr) <= 168, f"{name}: {vgpr} VGPRs leave fewer than the three waves per SIMD that its LDS tile allows"
    assert found == 1


# ---------------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("K, N", [(272, 128), (64, 128), (116, 64), (16, 32), (52, 32), (324, 192), (96, 144)])
def test_packed_image_is_the_rounded_weights_with_zero_padding_rows(K, N):
    from glow_tts_amd.vocoder import pad32, pwg_pack_bf16, pwg_unpack_bf16
    w = torch.randn(K, N, generator=torch.Generator().manual_seed(K + N)) * 0.3
    image = pwg_pack_bf16(w)
    Kp = pad32(K)
    assert Kp % 32 == 0 and 0 <= Kp - K < 32
    assert image.dtype == torch.bfloat16 and image.is_contiguous() and tuple(image.shape) == (Kp // 8, N, 8)
    back = pwg_unpack_bf16(image)
    assert torch.equal(back[:K], E.rb(w)) and bool((back[K:] == 0).all()) and back.shape == (Kp, N)
    flat = image.reshape(-1).float()                                         # the address the kernel computes: ((k / 8) N + n) 8 + k % 8
    for k, n in ((0, 0), (7, 1), (8, 0), (K - 1, N - 1), (K // 2, N // 3), (Kp - 1, N - 1)):
        assert float(flat[((k // 8) * N + n) * 8 + k % 8]) == (float(E.rb(w)[k, n]) if k < K else 0.0), (k, n)


# ---------------------------------------------------------------------------------------------------------------- the restatement alone
def test_rb_is_round_to_nearest_even():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8), 3.0e-5], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, float(torch.tensor(3.0e-5).bfloat16())], dtype=torch.float64)
    assert torch.equal(E.rb(t), want) and E.rb(t).dtype == torch.float64 and E.rb(t.float()).dtype == torch.float32


@pytest.mark.parametrize("name, lengths, layer", C.LAYER_CASES)
def test_layer_restatements_satisfy_the_gpu_bar(name, lengths, layer):
    """emu32 and emu32b against emu64 under the elementwise layer bar, for x' and for the skips, on every case of the GPU test."""
    case = C.layer_case(name, lengths, layer)
    for what in ("x", "skips"):
        for v in ("emu32", "emu32b"):
            assert case[what][v].dtype == torch.float32
            C.check_layer(f"{v} {name} layer {layer} {what}", case[what][v], case[what])


@pytest.mark.parametrize("name, lengths", C.GENERATOR_CASES)
def test_generator_restatements_satisfy_the_gpu_bars(name, lengths):
    mels, zs = C.generator_inputs(name, lengths)
    for b in range(len(lengths)):
        r = C.generator_refs(name, mels[b], zs[b])
        for v in ("emu32", "emu32b"):
            C.check_generator(f"{v} {name} {lengths} utterance {b}", r[v], r)


@pytest.mark.parametrize("name", C.SEEDED_CASES)
def test_seeded_restatements_satisfy_the_gpu_bars(name):
    mels, _, zs = C.seeded_inputs(name)
    for b in range(len(mels)):
        r = C.generator_refs(name, mels[b], zs[b])
        for v in ("emu32", "emu32b"):
            C.check_generator(f"{v} seeded {name} utterance {b}", r[v], r)
