"""No GPU: what the HiFi-GAN generator's training rests on besides the kernels - the reference gradients themselves (tests/hifigan_train_ref.py against central
finite differences in float64), the transposed weight images of the data gradients (against autograd in float64), the trainer's settings and refusals, and
the launch plan."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hifigan_ref as H  # noqa: E402
import hifigan_train_ref as R  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402


def test_reference_gradients_match_central_finite_differences():
    cfg, lengths = H.NARROW, [3, 2]
    sd = {k: v.double() for k, v in H.random_state_dict(cfg, 1234).items()}
    mels = [H.uniform_mel(cfg["A"], L, 20 + L) for L in lengths]
    g = torch.Generator().manual_seed(7)
    fs = [torch.randn(L * H.hop(cfg), generator=g, dtype=torch.float64) for L in lengths]
    _, grads = R.generator_grads(sd, cfg, mels, fs)
    loss = lambda s: float(sum((f * H.generator(s, cfg, m)[0]).sum() for f, m in zip(fs, mels)))
    pick = torch.Generator().manual_seed(1)
    for k, t in sd.items():
        for _ in range(2):
            i = int(torch.randint(t.numel(), (1,), generator=pick))
            h = 1e-6
            up, down = {**sd, k: t.clone()}, {**sd, k: t.clone()}
            up[k].view(-1)[i] += h
            down[k].view(-1)[i] -= h
            fd, an = (loss(up) - loss(down)) / (2 * h), float(grads[k].reshape(-1)[i])
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (k, i, fd, an)


@pytest.mark.parametrize("taps, d", [(3, 1), (7, 3), (11, 5)])
def test_conv_image_t_convolves_dy_into_dx(taps, d):
    from glow_tts_amd.vocoder import hifigan_conv_image_t
    g = torch.Generator().manual_seed(taps)
    cin, cout, T = 6, 4, 40
    w, x, dy = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((cout, cin, taps), (cin, T), (cout, T)))
    x.requires_grad_(True)
    (dy * F.conv1d(x[None], w, padding=(taps - 1) // 2 * d, dilation=d)[0]).sum().backward()
    image = hifigan_conv_image_t(w)                                           # [taps * Cout, Cin], row = tap' * Cout + co
    assert image.shape == (taps * cout, cin)
    wt = image.view(taps, cout, cin).permute(2, 1, 0)                         # a Conv1d weight [Cin, Cout, taps]: the same padding, the same dilation
    dx = F.conv1d(dy[None], wt, padding=(taps - 1) // 2 * d, dilation=d)[0]
    assert torch.allclose(dx, x.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("u, k", [(2, 4), (3, 7), (5, 11), (8, 16)])
def test_up_image_t_convolves_the_view_of_dy_into_dx(u, k):
    from glow_tts_amd.vocoder import hifigan_up_image_t, hifigan_up_reach, hifigan_up_taps
    g = torch.Generator().manual_seed(10 * u + k)
    cin, cout, T = 5, 3, 17
    w, x, dy = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((cin, cout, k), (cin, T), (cout, u * T)))
    x.requires_grad_(True)
    (dy * F.conv_transpose1d(x[None], w, stride=u, padding=(k - u) // 2)[0]).sum().backward()
    lo, hi = hifigan_up_reach(u, k)
    taps = hifigan_up_taps(u, k)
    assert taps.shape == (hi - lo + 1, u) and sorted(taps[taps < k].tolist()) == list(range(k))      # every tap exactly once
    image = hifigan_up_image_t(w, u)                                          # [(hi - lo + 1) * u * Cout, Cin]
    assert image.shape == ((hi - lo + 1) * u * cout, cin)
    view = dy.T.reshape(T, u * cout).T                                        # dy [T u][Cout] read as [T][u Cout], channels first for torch
    wt = image.view(hi - lo + 1, u * cout, cin).permute(2, 1, 0)              # a Conv1d weight over the view: offsets lo .. hi
    dx = F.conv1d(F.pad(view, (-lo, hi))[None], wt)[0]
    assert torch.allclose(dx, x.grad, rtol=1e-12, atol=1e-12)
    if (u, k) == (8, 16):
        assert (lo, hi) == (-1, 1) and int((taps < k).sum()) * 3 == 2 * taps.numel()                 # 1.5 x the arithmetic of the polyphase form


def _hp(block):
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    if block is not None:
        d["Vocoder"] = block
    return Recursive_Parse(d)


TINY_BLOCK = {"Type": "HiFiGAN", "Initial_Channels": 128, "Upsample_Rates": [8, 8, 4], "Upsample_Kernel_Sizes": [16, 16, 8], "Resblock": "2",
              "Resblock_Kernel_Sizes": [3, 5], "Resblock_Dilations": [[1, 3], [1, 3]]}


def test_trainer_settings_defaults_bad_keys_and_refusals():
    from glow_tts_amd import hifigan_trainer as T, pwg_trainer
    s = T.train_settings(_hp(dict(TINY_BLOCK)))
    assert (s["Batch_Size"], s["Segment_Frames"], s["Learning_Rate"], s["Checkpoint_Path"]) == (16, 32, 2.0e-4, "./hifigan_results")
    for k, v in pwg_trainer.DEFAULTS.items():
        if k not in ("Batch_Size", "Segment_Frames", "Learning_Rate", "Checkpoint_Path", "STFT_Resolutions"):
            assert s[k] == v, k
    assert "Discriminator" not in s and pwg_trainer.train_settings(_hp(None))["Batch_Size"] == 8             # the Parallel WaveGAN trainer's are untouched
    s = T.train_settings(_hp(dict(TINY_BLOCK, Train={"Batch_Size": 4, "Learning_Rate_Decay": {"Gamma": 0.9}})))
    assert s["Batch_Size"] == 4 and s["Learning_Rate_Decay"] == {"Step": 200000, "Gamma": 0.9}
    for train, named in (({"Batch_Size": 0}, "Vocoder.Train.Batch_Size"), ({"Segment_Frames": "x"}, "Vocoder.Train.Segment_Frames"),
                         ({"Learning_Rate": -1.0}, "Vocoder.Train.Learning_Rate"), ({"Epsilon": 0}, "Vocoder.Train.Epsilon"),
                         ({"Gradient_Norm": 0}, "Vocoder.Train.Gradient_Norm"), ({"Max_Step": 0}, "Vocoder.Train.Max_Step"),
                         ({"Checkpoint_Save_Interval": 0}, "Vocoder.Train.Checkpoint_Save_Interval"), ({"Evaluation_Interval": 0}, "Vocoder.Train.Evaluation_Interval"),
                         ({"Learning_Rate_Decay": {"Step": 0}}, "Vocoder.Train.Learning_Rate_Decay"), ({"Momentum": 1}, "Vocoder.Train.Momentum"),
                         ({"Learning_Rate_Decay": {"Rate": 1}}, "Vocoder.Train.Learning_Rate_Decay.Rate")):
        with pytest.raises(ValueError, match=named.replace(".", r"\.")):
            T.train_settings(_hp(dict(TINY_BLOCK, Train=train)))
    with pytest.raises(ValueError, match=r"Vocoder\.Train\.Discriminator"):
        T.train_settings(_hp(dict(TINY_BLOCK, Train={"Discriminator": {"Start_Step": 1}})))
    for block in ({"Type": "PWG"}, {"Checkpoint_Path": "x.pt"}, None):
        with pytest.raises(ValueError, match=r"Vocoder\.Type"):
            T.train_settings(_hp(block))


def test_trainer_refuses_in_its_constructor_head():
    """The refusals leave the constructor before the sampler, the model or the device exist (no pattern directory is configured here)."""
    from glow_tts_amd import hifigan_trainer as T
    with pytest.raises(ValueError, match=r"Vocoder\.Train\.Discriminator"):
        T.HiFiGAN_Trainer(hp=_hp(dict(TINY_BLOCK, Train={"Discriminator": {}})), device="cuda:0")
    with pytest.raises(ValueError, match=r"Vocoder\.Type"):
        T.HiFiGAN_Trainer(hp=_hp({"Type": "PWG"}), device="cuda:0")
    with pytest.raises(ValueError, match=r"Vocoder\.Type"):
        T.HiFiGAN_Trainer(hp=_hp(None), device="cuda:0")


def test_train_launches_geometry_and_kept_floats():
    from glow_tts_amd.vocoder import (HIFIGAN_DEFAULTS, hifigan_geometry, hifigan_launches, hifigan_train_geometry, hifigan_train_keep_floats,
                                      hifigan_train_launches)
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    d = load_yaml(DEFAULT_YAML)
    d["Vocoder"] = {"Type": "HiFiGAN"}
    geo = hifigan_geometry(Recursive_Parse(d))
    assert geo["rates"] == HIFIGAN_DEFAULTS["Upsample_Rates"]
    n = hifigan_train_launches(geo)
    assert n == {"hifigan_conv": 73, "hifigan_upsample": 4, "hifigan_conv,post": 1, "hifigan_post_bwd": 1, "hifigan_conv_bwd": 72, "hifigan_upsample_bwd": 4,
                 "hifigan_wgrad": 78, "hifigan_wgrad_sum": 78}
    assert sum(n[k] for k in ("hifigan_conv", "hifigan_upsample", "hifigan_conv,post")) == hifigan_launches(geo) == 78
    assert hifigan_train_keep_floats(geo) == 512 + 17 * (8 * 256 + 64 * 128 + 128 * 64 + 256 * 32) + 256
    for cfg in (H.DEFAULT, H.NARROW, H.ODD):                                  # all three must train
        dd = load_yaml(DEFAULT_YAML)
        dd["Sound"].update(Mel_Dim=cfg["A"], Frame_Shift=H.hop(cfg))
        dd["Vocoder"] = {"Type": "HiFiGAN", "Initial_Channels": cfg["C0"], "Upsample_Rates": cfg["rates"], "Upsample_Kernel_Sizes": cfg["kernels"],
                         "Resblock": cfg["resblock"], "Resblock_Kernel_Sizes": cfg["rk"], "Resblock_Dilations": cfg["rd"]}
        hifigan_train_geometry(hifigan_geometry(Recursive_Parse(dd)))
    wide = dict(geo, rates=[16, 16], kernels=[32, 32], channels=[512, 256], C0=1024)                 # 16 * 512 columns in the view of dy
    with pytest.raises(ValueError, match=r"Vocoder\.Upsample_Rates"):
        hifigan_train_geometry(wide)
