"""CPU: the multi-resolution STFT loss of vocoder training.  The float64 numpy restatement of the loss's closed-form gradient in the kernels' own form
(tests/pwg_train_ref.py `kernel_form_grad`: gather overlap-add over ceil(win / hop) frames plus the reflect fold) against autograd of the torch.stft
reference, three ways of getting that form wrong shown rejected by the same comparison, and the geometry checks of `vocoder.stft_loss_geometry`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pwg_train_ref as TR  # noqa: E402

SMALL = [(256, 50, 240), (512, 120, 400)]               # win / hop is not an integer in either
T_SMALL = 600


def compare(resolutions, B, T, seed, **broken):
    pred, target = (t.double() for t in TR.signals(B, T, seed))
    ref = TR.loss_and_grad(pred, target, resolutions)
    assert ref["low"] > 2 * TR.CLAMP                     # no bin on the clamp
    L, d = TR.kernel_form_grad(pred.numpy(), target.numpy(), resolutions, **broken)
    scale = float(ref["dpred"].abs().max())
    return abs(L - float(ref["L"])) / float(ref["L"]), float(np.abs(d - ref["dpred"].numpy()).max()) / scale


def test_kernel_form_gradient_matches_autograd_of_the_stft_reference():
    for res, B, T in ((SMALL, 2, T_SMALL), ([(256, 64, 256)], 1, 300), ([(256, 7, 100)], 1, 131)):
        eL, eD = compare(res, B, T, seed=5)
        print(res, eL, eD)
        assert eL <= 1e-10 and eD <= 1e-10


def test_kernel_form_gradient_with_the_clamp_active():
    """A prediction that is silent over its first half: the frames inside the silence sit on the clamp and get no gradient, on both sides."""
    pred, target = (t.double() for t in TR.signals(1, T_SMALL, 9))
    pred[:, :T_SMALL // 2] = 0.0
    ref = TR.loss_and_grad(pred, target, SMALL[:1])
    assert ref["low"] == 0.0
    L, d = TR.kernel_form_grad(pred.numpy(), target.numpy(), SMALL[:1])
    assert abs(L - float(ref["L"])) <= 1e-10 * float(ref["L"])
    assert float(np.abs(d - ref["dpred"].numpy()).max()) <= 1e-10 * float(ref["dpred"].abs().max())


@pytest.mark.parametrize("broken", ["drop_last_frame", "unfolded", "floor_cover"])
def test_a_wrong_gather_is_rejected(broken):
    eL, eD = compare(SMALL[:1], 1, T_SMALL, seed=5, **{broken: True})
    print(broken, eD)
    assert eL <= 1e-10 and eD > 1e-3


def test_pred_equal_to_target_gives_zero_loss_and_zero_gradient():
    x = TR.signals(1, T_SMALL, 3)[0].double().numpy()
    L, d = TR.kernel_form_grad(x, x.copy(), SMALL)
    assert L == 0.0 and not d.any()
    assert float(TR.stft_loss(torch.from_numpy(x), torch.from_numpy(x), SMALL)[0]) == 0.0


def test_default_resolutions_restate_the_contract():
    from glow_tts_amd import vocoder
    assert vocoder.stft_loss_geometry(None) == TR.RESOLUTIONS == [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)]
    assert vocoder.stft_loss_geometry([[256, 50, 240]], T=600) == [(256, 50, 240)]


@pytest.mark.parametrize("res, T, word", [([(1000, 120, 600)], None, "n_fft"), ([(128, 30, 100)], None, "n_fft"), ([(8192, 120, 600)], None, "n_fft"),
                                          ([(512, 50, 600)], None, "win"), ([(512, 300, 240)], None, "hop"), ([(512, 0, 240)], None, "hop"),
                                          ([(2048, 240, 1200)], 1024, "Segment_Frames"), ([], None, "triples"), ([(512, 50)], None, "triples")])
def test_unsupported_geometry_raises_naming_the_keys(res, T, word):
    from glow_tts_amd import vocoder
    with pytest.raises(ValueError) as e:
        vocoder.stft_loss_geometry(res, T)
    assert "Vocoder.Train.STFT_Resolutions" in str(e.value) and word in str(e.value)


# ---- the generator's backward: index arithmetic of csrc/pwg_train_ops.hip restated in float64 -----------------------------------------------------
def shifted(rows, s):
    """rows [T, C] -> rows(t + s), zero outside [0, T)"""
    T = rows.shape[0]
    out = torch.zeros_like(rows)
    if abs(s) < T:
        if s >= 0:
            out[:T - s] = rows[s:]
        else:
            out[-s:] = rows[:T + s]
    return out


@pytest.mark.parametrize("layer, T", [(0, 45), (1, 45), (3, 3)])          # dilations 1, 2, and 2 with every tap outside the utterance
def test_layer_backward_index_arithmetic_matches_autograd(layer, T):
    import math
    import pwg_ref as P
    cfg, dt = P.NARROW, torch.float64
    R, G, S, A, d = cfg["R"], cfg["G"], cfg["S"], cfg["A"], P.dilation(cfg, layer)
    sd = {k: v.double() for k, v in P.random_state_dict(cfg, 77).items()}
    g = torch.Generator().manual_seed(layer)
    x, c, dxp, dsk = (torch.randn(T, C, generator=g, dtype=dt) for C in (R, A, R, S))
    q = "conv_layers.{}.".format(layer)
    # the forward's images as vocoder.ParallelWaveGAN builds them, and the backward's transposes
    w1 = torch.cat([sd[q + "conv.weight"].permute(2, 1, 0).reshape(3 * R, G), sd[q + "conv1x1_aux.weight"][:, :, 0].t()], dim=0)
    w2 = torch.cat([sd[q + "conv1x1_out.weight"][:, :, 0].t(), sd[q + "conv1x1_skip.weight"][:, :, 0].t()], dim=1)
    w2t, w1t, wauxt = w2.t(), w1[:3 * R].view(3, R, G).permute(0, 2, 1).reshape(3 * G, R), w1[3 * R:].t()
    # pwg_layer_bwd_gate
    gathered = torch.cat([shifted(x, -d), x, shifted(x, d), c], dim=1)                   # tap j reads x(t + (j - 1) d)
    pre = gathered @ w1 + sd[q + "conv.bias"]
    ta, sg = torch.tanh(pre[:, :R]), torch.sigmoid(pre[:, R:])
    gate = ta * sg
    dgate = torch.cat([dxp * math.sqrt(0.5), dsk], dim=1) @ w2t
    dpre = torch.cat([dgate * sg * (1 - ta * ta), dgate * ta * sg * (1 - sg)], dim=1)
    # pwg_layer_bwd_data: x(u) is reached through tap j from t = u - (j - 1) d
    dx = math.sqrt(0.5) * dxp + torch.cat([shifted(dpre, d), dpre, shifted(dpre, -d)], dim=1) @ w1t
    dc = dpre @ wauxt
    # pwg_wgrad's jobs, in torch's layouts
    got = {"dx": dx.T, "dc": dc.T,
           "conv.weight": torch.stack([(shifted(x, (j - 1) * d).T @ dpre).T for j in range(3)], dim=2), "conv.bias": dpre.sum(0),
           "conv1x1_aux.weight": (c.T @ dpre).T[:, :, None],
           "conv1x1_out.weight": ((gate.T @ dxp) * math.sqrt(0.5)).T[:, :, None], "conv1x1_out.bias": dxp.sum(0) * math.sqrt(0.5),
           "conv1x1_skip.weight": (gate.T @ dsk).T[:, :, None], "conv1x1_skip.bias": dsk.sum(0)}
    ref = TR.layer_grads(sd, cfg, layer, x.T, c.T, dxp.T, dsk.T)
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape, k
        assert float((got[k] - ref[k]).abs().max()) <= 1e-10 * max(float(ref[k].abs().max()), 1.0), k
    # a flipped tap sign is rejected by the same comparison
    wrong = math.sqrt(0.5) * dxp + torch.cat([shifted(dpre, -d), dpre, shifted(dpre, d)], dim=1) @ w1t
    if T > d:
        assert float((wrong.T - ref["dx"]).abs().max()) > 1e-3


# ---- trainer pieces that need no device -------------------------------------------------------------------------------------------------------
def test_pwg_init_gives_what_pwg_load_accepts():
    import pwg_ref as P
    from glow_tts_amd import vocoder
    for cfg in (P.NARROW, P.DEFAULT):
        geo = dict(cfg, hop=P.hop(cfg), dilations=[P.dilation(cfg, i) for i in range(cfg["layers"])])
        sd = vocoder.pwg_init(geo, seed=3)
        assert {k: tuple(v.shape) for k, v in sd.items()} == vocoder.pwg_expected_shapes(geo) == P.shapes(cfg)
        out = vocoder.pwg_load({"generator": sd}, geo)
        assert all(torch.equal(out[k], sd[k]) and sd[k].dtype == torch.float32 for k in sd)
        for i, s in enumerate(cfg["scales"]):
            fir = sd["upsample_net.upsample.up_layers.{}.weight".format(2 * i + 1)]
            assert torch.equal(fir, torch.full((1, 1, 1, 2 * s + 1), 1.0 / (2 * s + 1)))
        w = sd["conv_layers.0.conv.weight"]
        assert float(w.abs().max()) <= 1.0 / (3 * cfg["R"]) ** 0.5 and float(w.abs().max()) > 0.9 / (3 * cfg["R"]) ** 0.5
        again, other = vocoder.pwg_init(geo, seed=3), vocoder.pwg_init(geo, seed=4)
        assert all(torch.equal(again[k], sd[k]) for k in sd) and not torch.equal(other["first_conv.weight"], sd["first_conv.weight"])


def _hp(train=None, shift=15):
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    d = load_yaml(DEFAULT_YAML)
    d["Sound"].update(Mel_Dim=20, Frame_Shift=shift)
    d["Vocoder"] = {"Type": "PWG", "Layers": 4, "Stacks": 2, "Residual_Channels": 32, "Gate_Channels": 64, "Skip_Channels": 32, "Upsample_Scales": [3, 5]}
    if train is not None:
        d["Vocoder"]["Train"] = train
    return Recursive_Parse(d)


def test_train_settings_defaults_and_bad_settings():
    from glow_tts_amd import pwg_trainer as T
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    s = T.train_settings(Recursive_Parse(load_yaml(DEFAULT_YAML)))                         # no Vocoder block at all: hop 256
    assert (s["Batch_Size"], s["Segment_Frames"], s["Learning_Rate"], s["Epsilon"], s["Gradient_Norm"]) == (8, 100, 1.0e-4, 1.0e-6, 10.0)
    assert s["Learning_Rate_Decay"] == {"Step": 200000, "Gamma": 0.5} and s["STFT_Resolutions"] == [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)]
    s = T.train_settings(_hp({"Batch_Size": 3, "Segment_Frames": 40, "STFT_Resolutions": [[256, 50, 240], [512, 120, 400]], "Learning_Rate_Decay": {"Step": 2}}))
    assert s["Batch_Size"] == 3 and s["Learning_Rate_Decay"] == {"Step": 2, "Gamma": 0.5} and s["STFT_Resolutions"] == [(256, 50, 240), (512, 120, 400)]
    for train, word in (({"Batch_Size": 0}, "Vocoder.Train.Batch_Size"), ({"Learning_Rate": -1.0}, "Vocoder.Train.Learning_Rate"),
                        ({"Learning_Rate_Decay": {"Gamma": 2.0}}, "Vocoder.Train.Learning_Rate_Decay"), ({"Bogus": 1}, "Vocoder.Train.Bogus"),
                        ({"Segment_Frames": 40}, "Vocoder.Train.STFT_Resolutions"),                     # 600 samples: too short for n_fft = 2048
                        ({"Segment_Frames": 40, "STFT_Resolutions": [[300, 50, 240]]}, "Vocoder.Train.STFT_Resolutions"),
                        ({"Learning_Rate": "fast"}, "Vocoder.Train.Learning_Rate = fast"),                  # a wrongly typed value is a bad value
                        ({"Learning_Rate_Decay": {"Bogus": 1}}, "unknown key Vocoder.Train.Learning_Rate_Decay.Bogus")):
        with pytest.raises(ValueError) as e:
            T.train_settings(_hp(train))
        assert word in str(e.value), (train, str(e.value))


def write_patterns(root, lengths, hop=15, mel_dim=20, seed=0):
    """A synthetic pattern directory: files of the given frame counts, the audio a ramp that names its own sample index"""
    import pickle
    rng = np.random.default_rng(seed)
    meta = {"File_List": [], "Mel_Length_Dict": {}, "Audio_Length_Dict": {}}
    os.makedirs(root, exist_ok=True)
    for i, n in enumerate(lengths):
        name = "F{}.PICKLE".format(i)
        audio = (np.arange(n * hop, dtype=np.float32) + 100000.0 * i)
        mel = rng.uniform(-4, 4, (n, mel_dim)).astype(np.float32)
        mel[:, 0] = np.arange(n)                                                        # channel 0 names the frame index
        with open(os.path.join(root, name), "wb") as f:
            pickle.dump({"Audio": audio, "Mel": mel}, f)
        meta["File_List"].append(name)
        meta["Mel_Length_Dict"][name], meta["Audio_Length_Dict"][name] = n, len(audio)
    with open(os.path.join(root, "METADATA.PICKLE"), "wb") as f:
        pickle.dump(meta, f)


def test_sampler_is_deterministic_aligned_and_excludes_short_files(tmp_path):
    from glow_tts_amd.pwg_trainer import Sampler, noise_seed_words
    write_patterns(str(tmp_path), [60, 39, 45, 12, 80])
    a, b = (Sampler(str(tmp_path), "METADATA.PICKLE", 6, 40, 15, seed=1) for _ in range(2))
    assert a.files == ["F0.PICKLE", "F2.PICKLE", "F4.PICKLE"]                            # 39 and 12 frames: too short
    seen = set()
    for step in range(8):
        assert a.plan(step) == b.plan(step)
        mel, wav = a.batch(step)
        assert mel.shape == (6, 20, 40) and wav.shape == (6, 600) and torch.equal(mel, b.batch(step)[0])
        for (f, f0), m, w in zip(a.plan(step), mel, wav):
            i = int(f[1:-len(".PICKLE")])
            assert 0 <= f0 <= [60, 39, 45, 12, 80][i] - 40
            assert torch.equal(m[0], torch.arange(f0, f0 + 40, dtype=torch.float32))                    # frames f0 .. f0 + 39
            assert torch.equal(w, torch.arange(f0 * 15, (f0 + 40) * 15, dtype=torch.float32) + 100000.0 * i)     # sample f0 * hop sits under frame f0
            seen.add((f, f0))
    assert len(seen) > 20 and a.plan(0) != a.plan(1) and a.plan(0) != Sampler(str(tmp_path), "METADATA.PICKLE", 6, 40, 15, seed=2).plan(0)
    with pytest.raises(ValueError) as e:
        Sampler(str(tmp_path), "METADATA.PICKLE", 6, 100, 15)
    assert "Vocoder.Train.Segment_Frames" in str(e.value)
    assert noise_seed_words(0, 5, 1) == noise_seed_words(0, 5, 1) != noise_seed_words(0, 5, 2) and noise_seed_words(0, 5, 1) != noise_seed_words(0, 6, 1)


def test_dc_accumulates_over_the_layers_and_the_first_processed_overwrites():
    """The backward walks the layers from the last to the first with ONE dc buffer: the first layer processed overwrites it (no memset), the others add,
    as the forward does with `skips`.  Two stacked layers sharing c, restated in float64 in that order, against autograd of `pwg_ref.layer`."""
    import math
    import pwg_ref as P
    cfg, dt, T = P.NARROW, torch.float64, 37
    R, G, S, A = cfg["R"], cfg["G"], cfg["S"], cfg["A"]
    sd = {k: v.double() for k, v in P.random_state_dict(cfg, 78).items()}
    g = torch.Generator().manual_seed(3)
    x0, c, dx2, dsk = (torch.randn(T, C, generator=g, dtype=dt) for C in (R, A, R, S))
    xa, ca = x0.T.clone().requires_grad_(True), c.T.clone().requires_grad_(True)
    x1, s0 = P.layer(sd, cfg, 0, xa, ca, dt)
    x2, s1 = P.layer(sd, cfg, 1, x1, ca, dt)
    ((x2 * dx2.T).sum() + ((s0 + s1) * dsk.T).sum()).backward()                      # d skips is the same tensor for both layers
    dc = torch.full((T, A), float("nan"), dtype=dt)                                   # never cleared: the first layer processed must overwrite
    dxp, xs = dx2, [x0, x1.detach().T]
    for i in (1, 0):
        d, q = P.dilation(cfg, i), "conv_layers.{}.".format(i)
        w1 = torch.cat([sd[q + "conv.weight"].permute(2, 1, 0).reshape(3 * R, G), sd[q + "conv1x1_aux.weight"][:, :, 0].t()], dim=0)
        w2 = torch.cat([sd[q + "conv1x1_out.weight"][:, :, 0].t(), sd[q + "conv1x1_skip.weight"][:, :, 0].t()], dim=1)
        pre = torch.cat([shifted(xs[i], -d), xs[i], shifted(xs[i], d), c], dim=1) @ w1 + sd[q + "conv.bias"]
        ta, sg = torch.tanh(pre[:, :R]), torch.sigmoid(pre[:, R:])
        dgate = torch.cat([dxp * math.sqrt(0.5), dsk], dim=1) @ w2.t()
        dpre = torch.cat([dgate * sg * (1 - ta * ta), dgate * ta * sg * (1 - sg)], dim=1)
        w1t = w1[:3 * R].view(3, R, G).permute(0, 2, 1).reshape(3 * G, R)
        dxp = math.sqrt(0.5) * dxp + torch.cat([shifted(dpre, d), dpre, shifted(dpre, -d)], dim=1) @ w1t
        contribution = dpre @ w1[3 * R:].t()
        dc = contribution if i == 1 else dc + contribution
    assert float((dc.T - ca.grad).abs().max()) <= 1e-10 * float(ca.grad.abs().max())
    assert float((dxp.T - xa.grad).abs().max()) <= 1e-10 * float(xa.grad.abs().max())
