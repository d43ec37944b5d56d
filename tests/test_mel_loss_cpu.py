"""CPU: the mel loss's reference (tests/mel_loss_ref.py) against the project's own front end and against finite differences, and the settings code of the
block `Vocoder.Train.Mel_Loss` (`vocoder.mel_loss_settings`, `vocoder.mel_loss_geometry`, both trainers' `train_settings`).

Bounds.  (1) exp(m) against `audio.mel_filterbank @ audio.stft_magnitude`, both float64, to 1e-10 relative, per element.  The restatement is held to it
with the constant inside its root set to 0: what then differs is the rounding of two FFTs, 1e-14, so framing, window, filterbank and bin order are the front
end's.  With the contract's 1e-9 inside the root the two differ by sum_k fb[j, k] (sqrt(|X|^2 + 1e-9) - |X|) <= sum_k fb[j, k] 1e-9 / (2 |X|[k]), which is
asserted as that inequality; it is NOT below 1e-10 of the mel for amplitude-0.3 noise: the first frame of a reflect-padded signal is even about its centre, its
spectrum real, and a real Gaussian bin comes within 1e-3 of zero among a thousand (measured: 6.6e-9 per element, 1.4e-9 of the largest mel at the default
geometry under seed 4; over 1500 seeds never below 8e-10 per element); it is printed.  The inequality
is held to 1e-3 of itself: both sides are differences of order 1e-12 of float64 values of order 1, known to 1e-16.  (2) central differences with h = 1e-5 in float64: the rounding of the loss,
1e-16 * L / h = 1e-11, and the truncation h^2 f''' / 6 = 1e-11 sit four orders below the largest gradient (1e-4 .. 1e-3 per sample), so 1e-5 of the largest
gradient is a bound with a decade to spare; the loss is smooth between the kinks of |.|, and no kink lies within h of the inputs (measure zero)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import mel_loss_ref as MR  # noqa: E402
import pwg_train_ref as TR  # noqa: E402
from helpers import tiny_hp_dict  # noqa: E402

KEY = "Vocoder.Train.Mel_Loss"
GEOS = {"default": (MR.DEFAULT, 2304, 4), "small": (MR.SMALL, 600, 2)}          # (geometry, T, seed)


def hp_of(block=None, train=None, kind="HiFiGAN", sound=None):
    from glow_tts_amd.hparams import Recursive_Parse
    d = tiny_hp_dict("Vanilla")
    d["Sound"].update(sound or {})
    d["Vocoder"] = {"Type": kind, "Train": dict(train or {})}
    if block is not None:
        d["Vocoder"]["Train"]["Mel_Loss"] = block
    return Recursive_Parse(copy.deepcopy(d))


@pytest.mark.parametrize("name", list(GEOS))
def test_the_restatement_is_the_front_ends_mel(name):
    from glow_tts_amd import audio
    geo, T, seed = GEOS[name]
    x = TR.signals(1, T, seed)[0][0].double()
    m, lin = MR.log_mel(x[None], geo)
    assert float(lin.min()) > 10 * geo["floor"]                                # the floor is idle: exp(m) is the mel itself
    fb = audio.mel_filterbank(geo["sample_rate"], geo["n_fft"], geo["mel"], geo["f_min"], geo["f_max"]).astype(np.float64)
    mag = audio.stft_magnitude(x.numpy(), geo["n_fft"], geo["hop"], geo["win"])
    want = fb @ mag
    assert want.shape == (geo["mel"], 1 + T // geo["hop"]) == tuple(m.shape[1:])
    got, plain = torch.exp(m[0]).numpy(), torch.exp(MR.log_mel(x[None], geo, eps=0.0)[0][0]).numpy()
    literal = float((np.abs(got - want) / want).max())
    framing = float((np.abs(plain - want) / want).max())
    excess = float(((got - plain) / (fb @ (0.5 * MR.EPS / mag))).max())
    print("{}: exp(m) vs the front end {:.3e} per element with the 1e-9 in the root, {:.3e} without it; (got - plain) / its bound {:.6f}, smallest |X| {:.3e}"
          .format(name, literal, framing, excess, mag.min()))
    assert framing <= 1e-10                                                    # framing, window, filterbank: the front end's
    assert (got >= plain * (1 - 1e-13)).all() and excess <= 1 + 1e-3           # and the rest is the root's constant, within its own bound


@pytest.mark.parametrize("name", list(GEOS))
def test_the_gradient_matches_central_differences(name):
    geo, T, seed = GEOS[name]
    pred, target = TR.signals(2, T, seed)
    r = MR.loss_and_grad(pred, target, geo)
    M, h = geo["n_fft"] // 2, 1e-5
    scale = float(r["dpred"].abs().max())
    # the reflected samples at both ends (1 .. M and T - 1 - M .. T - 2 are read twice), the edges themselves and the interior
    worst = 0.0
    for b, s in ((0, 0), (0, 1), (1, M // 2), (0, M), (1, M + 1), (0, T // 2), (1, T - 1 - M), (0, T - 2 - M // 3), (1, T - 2), (0, T - 1)):
        p = pred.double().clone()
        p[b, s] += h
        up = MR.mel_loss(p, target, geo)[0]
        p[b, s] -= 2 * h
        fd = float(up - MR.mel_loss(p, target, geo)[0]) / (2 * h)
        worst = max(worst, abs(fd - float(r["dpred"][b, s])) / scale)
    print("{}: finite differences off by {:.3e} of the largest gradient {:.3e}".format(name, worst, scale))
    assert scale > 1e-5 and worst <= 1e-5


def test_settings_defaults_come_from_sound():
    from glow_tts_amd.vocoder import MEL_KEY, mel_loss_geometry, mel_loss_settings
    assert MEL_KEY == KEY
    want = {"Lambda": 45.0, "Floor": 1.0e-5, "Mel_F_Min": 125, "Mel_F_Max": 7600}
    assert mel_loss_settings(hp_of(None)) == want and mel_loss_settings(hp_of({})) == want
    s = mel_loss_settings(hp_of({"Lambda": 10, "Mel_F_Max": 12000}))
    assert s == dict(want, Lambda=10, Mel_F_Max=12000)
    hp = hp_of({}, sound={"Mel_Dim": 80})
    assert mel_loss_geometry(hp) == mel_loss_geometry(hp, mel_loss_settings(hp)) == MR.DEFAULT
    g = mel_loss_geometry(hp_of({"Floor": 1e-4, "Mel_F_Min": 0, "Mel_F_Max": 12000}, sound={"Mel_Dim": 80}))
    assert g == dict(MR.DEFAULT, floor=1e-4, f_min=0.0, f_max=12000.0)
    small = hp_of(None, sound={"Spectrogram_Dim": 129, "Frame_Length": 240, "Frame_Shift": 50, "Mel_Dim": 20})
    assert mel_loss_geometry(small, None, T=600) == MR.SMALL
    assert MR.hp_dict(tiny_hp_dict("Vanilla"), MR.SMALL)["Sound"]["Spectrogram_Dim"] == 129


BAD = [("Lambda", 0), ("Lambda", -45.0), ("Lambda", "big"), ("Lambda", float("inf")), ("Floor", 0.0), ("Floor", -1e-5), ("Floor", None), ("Mel_F_Min", -1),
       ("Mel_F_Max", 100), ("Mel_F_Max", "high"), ("Bogus", 1), ("Start_Step", 0)]


@pytest.mark.parametrize("key, value", BAD)
def test_every_bad_or_unknown_key_is_named(key, value):
    from glow_tts_amd import hifigan_trainer, pwg_trainer
    from glow_tts_amd.vocoder import mel_loss_settings
    match = "{}.{}".format(KEY, key).replace(".", r"\.")
    with pytest.raises(ValueError, match=match):
        mel_loss_settings(hp_of({key: value}))
    with pytest.raises(ValueError, match=match):
        hifigan_trainer.train_settings(hp_of({key: value}))
    with pytest.raises(ValueError, match=match):
        pwg_trainer.train_settings(hp_of({key: value}, kind="PWG"))


def test_the_block_must_be_a_mapping():
    from glow_tts_amd.vocoder import mel_loss_settings
    with pytest.raises(ValueError, match=r"Vocoder\.Train\.Mel_Loss must be a mapping"):
        mel_loss_settings(hp_of(45.0))


GEOMETRY = [({"Spectrogram_Dim": 501}, None, None, r"Sound\.Spectrogram_Dim"), ({"Spectrogram_Dim": 4097}, None, None, r"Sound\.Spectrogram_Dim"),
            ({"Frame_Length": 4096}, None, None, r"Sound\.Frame_Length"), ({"Frame_Shift": 2048}, None, None, r"Sound\.Frame_Shift"),
            ({"Frame_Shift": 0}, None, None, r"Sound\.Frame_Shift"), ({"Mel_Dim": 3}, None, None, r"Sound\.Mel_Dim"), ({"Mel_Dim": 257}, None, None, r"Sound\.Mel_Dim"),
            ({}, {"Mel_F_Max": 12001}, None, r"Vocoder\.Train\.Mel_Loss\.Mel_F_Max"), ({"Spectrogram_Dim": 129, "Frame_Length": 240, "Frame_Shift": 50, "Mel_Dim": 80}, None, None, r"Sound\.Mel_Dim.*without a bin"),
            ({}, None, 1024, r"Vocoder\.Train\.Mel_Loss.*Segment_Frames")]


@pytest.mark.parametrize("sound, block, T, match", GEOMETRY)
def test_every_unsupported_size_names_its_key(sound, block, T, match):
    from glow_tts_amd.vocoder import mel_loss_geometry
    with pytest.raises(ValueError, match=match):
        mel_loss_geometry(hp_of(block, sound=sound), None, T)


def test_both_trainers_take_the_block_and_an_absent_block_changes_nothing():
    from glow_tts_amd import hifigan_trainer, pwg_trainer
    from glow_tts_amd.vocoder import MPD_DEFAULTS
    want = {"Lambda": 45.0, "Floor": 1.0e-5, "Mel_F_Min": 125, "Mel_F_Max": 7600}
    for T, kind, stage_two in ((hifigan_trainer, "HiFiGAN", "Adversarial"), (pwg_trainer, "PWG", "Discriminator")):
        absent = T.train_settings(hp_of(None, kind=kind))
        assert set(absent) == set(T.DEFAULTS)                                  # no Mel_Loss key: the trainer builds no mel criterion
        s = T.train_settings(hp_of({}, kind=kind))
        assert s["Mel_Loss"] == want and {k: v for k, v in s.items() if k != "Mel_Loss"} == absent
        s = T.train_settings(hp_of({"Lambda": 2.5}, train={stage_two: {}, "Batch_Size": 4}, kind=kind))           # beside the stage-two block
        assert s["Mel_Loss"] == dict(want, Lambda=2.5) and stage_two in s and s["Batch_Size"] == 4
    assert hifigan_trainer.train_settings(hp_of({}, train={"Adversarial": {}}))["Adversarial"] == MPD_DEFAULTS
    # the segment must cover the reflect padding of the mel loss's n_fft
    with pytest.raises(ValueError, match=r"Vocoder\.Train\.Mel_Loss.*Segment_Frames"):
        hifigan_trainer.train_settings(hp_of({}, train={"Segment_Frames": 4, "STFT_Resolutions": [[256, 50, 240]]}))
    assert "Mel_Loss" not in hifigan_trainer.train_settings(hp_of(None, train={"Segment_Frames": 4, "STFT_Resolutions": [[256, 50, 240]]}))


def test_the_hifigan_trainer_still_refuses_the_other_discriminator():
    from glow_tts_amd import hifigan_trainer, pwg_trainer
    with pytest.raises(ValueError, match=r"Vocoder\.Train\.Discriminator.*Vocoder\.Train\.Adversarial"):
        hifigan_trainer.train_settings(hp_of({}, train={"Discriminator": {}}))
    with pytest.raises(ValueError, match=r"unknown key Vocoder\.Train\.Adversarial"):
        pwg_trainer.train_settings(hp_of({}, train={"Adversarial": {}}, kind="PWG"))


def test_the_transposed_filterbank_is_the_filterbank():
    from glow_tts_amd import audio
    from glow_tts_amd.frontend import dense_filterbank, sparse_filterbank
    from glow_tts_amd.vocoder import transposed_filterbank
    for geo in (MR.DEFAULT, MR.SMALL):
        F = geo["n_fft"] // 2 + 1
        fb = audio.mel_filterbank(geo["sample_rate"], geo["n_fft"], geo["mel"], geo["f_min"], geo["f_max"])
        index, weights = sparse_filterbank(fb)
        assert np.array_equal(dense_filterbank(index, weights, F), fb) and (index[:, 1] > 0).all()
        start, filt, wt = transposed_filterbank(index, weights, F)
        assert start.dtype == filt.dtype == np.int32 and start.shape == (F + 1,) and start[0] == 0 and start[-1] == len(filt) == len(wt) == len(weights)
        back = np.zeros_like(fb)
        for k in range(F):
            row = filt[start[k]:start[k + 1]]
            assert (np.diff(row) > 0).all()                                    # ascending filter order, each filter once
            back[row, k] = wt[start[k]:start[k + 1]]
        assert np.array_equal(back, fb)
