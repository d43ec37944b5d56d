"""Seeded sampling on the GPU: glowtts_prior_sample (csrc/sample_ops.hip) against today's path (searchsorted + path_from_idx + ExpandPrior) and the
float64 restatement (tests/prior_sample_ref.py) at the operator level; `GlowTTS.inference(seeds=)` against `noises=` on the tiny golden models of all
four modes; `GraphedInference(seeds=)` and `Inference.py --seed` in child processes (they capture hipGraphs)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prior_sample_ref as R
from helpers import launch_counts, launch_reset, load_case, tiny_hp_dict

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
B = 3


def consts():
    from glow_tts_amd import abi
    return abi.SAMPLE_SCAN_CHUNK, abi.SAMPLE_TILE


def hand_durations(Tx):
    """[3, Tx] integer-valued durations.  Row 0: zeros in the middle, runs of 1s, one token spanning more than three frame tiles, a padded tail of zeros;
    row 1: all zero (the model clamps its mel length to 1); row 2: no padding and, beyond one scan chunk, long tokens on both sides of the chunk boundary
    (the frames of one tile look up tokens of two chunks)."""
    chunk, tile = consts()
    d = np.zeros((B, Tx), np.float32)
    valid = max(1, Tx - Tx // 4)
    for i in range(valid):
        d[0, i] = 0 if i % 7 in (2, 3) else (1 if i % 7 in (4, 5, 6) else 2)
    d[0, min(valid - 1, 3)] = 3 * tile + 5
    for i in range(Tx):
        d[2, i] = (3, 0, 1)[i % 3]
    if Tx > chunk:
        d[2, chunk - 2:chunk + 1] = (3, tile + 6, 5)
    return d


def make_case(C, Tx, vec, seed=0):
    chunk, tile = consts()
    g = torch.Generator().manual_seed(100 * C + Tx + seed)
    dur = torch.from_numpy(hand_durations(Tx))
    lengths = dur.sum(1).clamp_min(1.0).long()
    Tmax = int(lengths.max()) + 37                       # bucket padding: larger than every length
    Tmax = (Tmax + 3) // 4 * 4 if vec else Tmax | 1      # 16-byte rows / odd rows (the scalar stores)
    if Tmax % tile == 0:
        Tmax += 4
    assert Tmax % tile != 0 and (Tmax % 4 == 0) == vec and Tmax > int(lengths.max())
    mean = torch.rand(B, C, Tx, generator=g) * 4 - 2
    log_std = torch.rand(B, C, Tx, generator=g) * 1.5 - 1
    seeds = torch.tensor([[1, 2], [0xFFFFFFFF, 7], [2499690753, 1716153205]], dtype=torch.int64)
    scales = torch.tensor([1.5, 0.7, 1.0])
    return mean, log_std, dur, lengths, seeds, scales, Tmax


def todays_path(dur, mel_lengths, Tmax, Tx):
    """idx and the dense attentions as `GlowTTS.inference_back` computes them without seeds"""
    from glow_tts_amd.monotonic_align import path_from_idx
    cum = torch.cumsum(dur, dim=1).contiguous()
    frames = torch.arange(Tmax, device=cum.device, dtype=cum.dtype)
    idx = torch.searchsorted(cum, frames.unsqueeze(0).expand(cum.shape[0], -1).contiguous(), right=True)
    idx = torch.where((frames.unsqueeze(0) < mel_lengths.unsqueeze(1)) & (idx < Tx), idx, torch.full_like(idx, -1)).to(torch.int32).contiguous()
    return idx, path_from_idx(idx, Tx, torch.float32)


@pytest.mark.parametrize("vec", [True, False])
@pytest.mark.parametrize("Tx", [1, 5, 65, 1025])
@pytest.mark.parametrize("C", [12, 80])
def test_prior_sample_operator(C, Tx, vec):
    from glow_tts_amd import alignment
    chunk, _ = consts()
    assert chunk + 1 == 1025                             # (the parametrisation names CHUNK + 1 as a literal)
    mean, log_std, dur, lengths, seeds, scales, Tmax = make_case(C, Tx, vec)
    c = lambda t: t.cuda()
    mean_d, ls_d, dur_d, len_d, sc_d = c(mean), c(log_std), c(dur), c(lengths), c(scales)
    z, idx, attn = alignment.prior_sample(mean_d, ls_d, dur_d, len_d, seeds, sc_d, Tmax)
    torch.cuda.synchronize()
    assert z.shape == (B, C, Tmax) and idx.shape == (B, Tmax) and attn.shape == (B, Tx, Tmax)
    # alignment: today's path, bit for bit
    widx, wattn = todays_path(dur_d, len_d, Tmax, Tx)
    assert torch.equal(idx, widx) and torch.equal(attn, wattn)
    # beyond each length: idx -1, z exactly 0
    frames = torch.arange(Tmax, device="cuda")
    beyond = frames[None, :] >= len_d[:, None]
    assert (idx[beyond] == -1).all() and (z.transpose(1, 2)[beyond] == 0).all()
    assert int(lengths[1]) == 1 and (idx[1] == -1).all() and (z[1] == 0).all()            # the utterance without durations
    if Tx > 1:
        assert (idx[0] >= 0).any() and (idx[2] >= 0).sum() == int(lengths[2])
    # float64 restatement: alignment, noise alone, the full sample
    zr, ir, ar = R.prior_sample(mean.numpy(), log_std.numpy(), dur.numpy(), lengths.numpy(), seeds.numpy(), scales.numpy(), Tmax)
    assert np.array_equal(idx.cpu().numpy(), ir) and np.array_equal(attn.cpu().numpy(), ar)
    zero = torch.zeros_like(mean_d)
    one = torch.ones(B, device="cuda")
    noise, _, _ = alignment.prior_sample(zero, zero, dur_d, len_d, seeds, one, Tmax, want_attn=False)
    want = np.stack([R.noise(int(s0), int(s1), C, Tmax) for s0, s1 in seeds.tolist()]) * (ir >= 0)[:, None, :]
    err_noise = np.abs(noise.cpu().numpy().astype(np.float64) - want).max()
    err_z = np.abs(z.cpu().numpy().astype(np.float64) - zr).max()
    print(f"C {C} Tx {Tx} Tmax {Tmax}: noise err {err_noise:.3e}, z err {err_z:.3e}")
    assert err_noise <= 1e-5, err_noise
    assert err_z <= 4e-5, err_z
    # noise_scale = 0 rows: the expanded mean itself
    sc0 = torch.tensor([0.0, 1.0, 0.0], device="cuda")
    z0, idx0, none = alignment.prior_sample(mean_d, ls_d, dur_d, len_d, seeds, sc0, Tmax, want_attn=False)
    expanded = alignment.ExpandPrior.apply(mean_d, idx)
    assert none is None and torch.equal(idx0, idx)                                        # attn = NULL leaves idx ...
    assert torch.equal(z0[0], expanded[0]) and torch.equal(z0[2], expanded[2])
    # the scale of row b reaches row b only
    sc2 = scales.clone()
    sc2[2] = 0.25
    z2, _, _ = alignment.prior_sample(mean_d, ls_d, dur_d, len_d, seeds, c(sc2), Tmax, want_attn=False)
    assert torch.equal(z2[:2], z[:2])
    if Tx > 1:
        assert not torch.equal(z2[2], z[2])
    # two runs are equal (and attn = NULL leaves z unchanged); another seed differs, in its own row only
    z3, idx3, _ = alignment.prior_sample(mean_d, ls_d, dur_d, len_d, seeds, sc_d, Tmax, want_attn=False)
    assert torch.equal(z3, z) and torch.equal(idx3, idx)
    seeds4 = seeds.clone()
    seeds4[0, 1] += 1
    z4, _, _ = alignment.prior_sample(mean_d, ls_d, dur_d, len_d, seeds4, sc_d, Tmax, want_attn=False)
    assert torch.equal(z4[1:], z[1:]) and not torch.equal(z4[0], z[0])
    valid0 = idx[0] >= 0
    assert (z4[0][:, valid0] != z[0][:, valid0]).float().mean() > 0.99


@pytest.mark.parametrize("C", [12, 80])
def test_batch_independence_bit_for_bit(C):
    """The same (mean, log_std, dur, seed) rows as b = 0 of B = 1 with Tmax = its length (odd: scalar stores, one scan chunk) and as b = 2 of B = 3 with a
    larger Tmax (16-byte stores) and a token axis padded beyond one scan chunk: the same bits."""
    from glow_tts_amd import alignment
    chunk, tile = consts()
    Tx = 65
    g = torch.Generator().manual_seed(C)
    dur = torch.from_numpy(hand_durations(Tx)[0:1])
    dur[0, 0] += 1 - int(dur.sum()) % 2                                                   # an odd length
    n = int(dur.sum())
    assert n % 2 == 1 and n > 3 * tile
    mean, log_std = torch.randn(1, C, Tx, generator=g), torch.rand(1, C, Tx, generator=g) - 1
    seed = torch.tensor([[123456789, 987654321]], dtype=torch.int64)
    z1, i1, a1 = alignment.prior_sample(mean.cuda(), log_std.cuda(), dur.cuda(), torch.tensor([n]).cuda(), seed, torch.tensor([0.8]).cuda(), n)
    Tx3, T3 = chunk + 76, (n + 303) // 4 * 4
    mean3, ls3, dur3 = torch.randn(3, C, Tx3, generator=g), torch.rand(3, C, Tx3, generator=g) - 1, torch.randint(0, 3, (3, Tx3), generator=g).float()
    mean3[2, :, :Tx], ls3[2, :, :Tx] = mean[0], log_std[0]
    dur3[:2, 150:] = 0                                                                    # (the other utterances stay shorter than the padded frame count)
    dur3[2] = 0
    dur3[2, :Tx] = dur[0]
    len3 = dur3.sum(1).long()
    seeds3 = torch.tensor([[5, 6], [7, 8], [123456789, 987654321]], dtype=torch.int64)
    z3, i3, a3 = alignment.prior_sample(mean3.cuda(), ls3.cuda(), dur3.cuda(), len3.cuda(), seeds3, torch.tensor([1.0, 0.3, 0.8]).cuda(), T3)
    torch.cuda.synchronize()
    assert int(len3[2]) == n and T3 > int(len3.max())
    assert torch.equal(z3[2, :, :n], z1[0]) and torch.equal(i3[2, :n], i1[0]) and torch.equal(a3[2, :Tx, :n], a1[0])
    assert (z3[2, :, n:] == 0).all() and not a3[2, Tx:].any()


# ------------------------------------------------------------------------------------------------ whole models
TINY = [("Vanilla", "tiny_vanilla.npz"), ("SE", "tiny_se.npz"), ("PE", "tiny_pe.npz"), ("GR", "tiny_gr.npz")]


def build_tiny(mode, precision, sd):
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    hp = tiny_hp_dict(mode)
    hp["HIP_Precision"] = precision
    model = GlowTTS(Recursive_Parse(hp))
    model.load_state_dict(sd)
    for f in model.layer_Dict["Decoder"].layer_Dict["Flows"]:
        f.layers[0].initialized = True
    return model.cuda().eval()


@pytest.mark.parametrize("mode,fname", TINY)
def test_seeded_inference_matches_injected_device_noise(mode, fname):
    """model.inference(seeds=) against model.inference(noises=D), D the device's own noise (prior_sample on mean 0, log_std 0, scale 1): equal lengths and
    attentions, mels within the f32 bar; the launch log of the seeded back half shows the one fused launch instead of the two expansions and the path."""
    from glow_tts_amd import alignment
    sd, _, r = load_case(fname)
    model = build_tiny(mode, "f32", sd)
    vocab = sd["layer_Dict.Encoder.layer_Dict.Embedding.weight"].shape[0]
    g = torch.Generator().manual_seed(17)
    lengths = [23, 9]
    tokens = torch.randint(1, vocab, (2, max(lengths)), generator=g)
    tokens[1, lengths[1]:] = 0
    tl = torch.tensor(lengths)
    ls = torch.tensor([1.3, 0.9])
    c = lambda t: None if t is None else t.cuda()
    spk = torch.tensor([1, 3]) if mode in ("SE", "GR") and "speakers" in r else None
    pm = torch.from_numpy(r["mels"][:2]) if mode in ("PE", "GR") else None
    pl = torch.from_numpy(r["mel_lengths"][:2]) if mode in ("PE", "GR") else None
    pit = torch.from_numpy(r["pitches"][:2]) if mode == "GR" else None
    args = (tokens.cuda(), tl.cuda(), c(pm), c(pl), c(spk), None, c(pit), c(pl) if pit is not None else None)
    seeds = torch.tensor([R.seed_words(7, "Alpha", 0), R.seed_words(7, "Bravo", 0)], dtype=torch.int64)
    with torch.no_grad():
        front = model.inference_front(args[0], args[1], args[2], args[3], args[4], None, ls.cuda())
        mean, log_std, dur, mel_lengths = front[:4]
        Tmax = int(mel_lengths.max())
        zero = torch.zeros_like(mean)
        D, _, _ = alignment.prior_sample(zero, zero, dur, mel_lengths, seeds, torch.ones(2, device="cuda"), Tmax, want_attn=False)
        got, gl, ga = model.inference(*args, noise_scale=0.667, length_scale=ls.cuda(), seeds=seeds)
        want, wl, wa = model.inference(*args, noise_scale=0.667, length_scale=ls.cuda(), noises=D)
        torch.cuda.synchronize()
        assert Tmax > 8 and D.abs().max() > 1
        assert torch.equal(gl, wl) and torch.equal(ga, wa)
        err = (got - want).abs().max().item()
        assert got.shape == want.shape and err <= 2e-4, err
        # a [B] noise_scale: row 1 at temperature 0 is the mean's mel, row 0 is unchanged
        per, _, _ = model.inference(*args, noise_scale=torch.tensor([0.667, 0.0]), length_scale=ls.cuda(), seeds=seeds)
        cold, _, _ = model.inference(*args, noise_scale=0.0, length_scale=ls.cuda(), noises=D)
        n0, n1 = (int(gl[0]) // 2) * 2, (int(gl[1]) // 2) * 2
        assert (per[0, :, :n0] - got[0, :, :n0]).abs().max().item() <= 2e-4 and (per[1, :, :n1] - cold[1, :, :n1]).abs().max().item() <= 2e-4
        with pytest.raises(ValueError, match=r"seeds.*noises"):
            model.inference(*args, seeds=seeds, noises=D)
        with pytest.raises(ValueError, match=r"noise_scale.*seeds"):
            model.inference(*args, noise_scale=torch.tensor([0.667, 0.0]))
        pitch_kw = dict(pitches=args[6], pitch_lengths=args[7])
        launch_reset()
        model.inference_back(front, None, 0.667, None, seeds=seeds, **pitch_kw)
        torch.cuda.synchronize()
        counts = launch_counts()
        assert counts.get("prior_sample", 0) == 1 and counts.get("expand_fwd", 0) == 0 and counts.get("mas_path_from_idx", 0) == 0, counts
        launch_reset()
        model.inference_back(front, None, 0.667, None, **pitch_kw)
        torch.cuda.synchronize()
        counts = launch_counts()
        assert counts.get("prior_sample", 0) == 0 and counts.get("expand_fwd", 0) == 2 and counts.get("mas_path_from_idx", 0) == 1, counts


def test_graphed_inference_with_seeds():
    """tests/prior_sample_graph_check.py in a child process (it captures hipGraphs)."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "prior_sample_graph_check.py")], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0 and "SEEDED GRAPH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_inference_entry_point_with_seed(tmp_path):
    """`python Inference.py -c <tiny checkpoint> --seed 7 --samples 2 --wav`: <label>.S0 / .S1 exist and differ; a second run writes byte-identical .npy and
    .wav files; Inference_Batch_Size 1 against 4 gives mels within the f32 bar."""
    import yaml
    from glow_tts_amd import data
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    texts = ["Birds of a feather flock together.", "A creative artist works on his next composition because he was not satisfied with his previous one."]
    token_dict = data.make_token_dict([data.text_filtering(t) for t in texts])
    with open(tmp_path / "Token.yaml", "w") as f:
        yaml.dump(token_dict, f)
    hp = tiny_hp_dict("Vanilla")
    hp["Token_Path"] = str(tmp_path / "Token.yaml")
    hp["Encoder"]["Embedding_Tokens"] = len(token_dict)
    torch.manual_seed(0)
    sd = GlowTTS(Recursive_Parse(hp)).state_dict()
    torch.save({"Model": sd, "Steps": 0}, tmp_path / "ckpt.pt")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(name, batch_size, wav=True):
        d = tmp_path / name
        d.mkdir()
        hp["Inference_Batch_Size"] = batch_size
        with open(d / "Hyper_Parameters.yaml", "w") as f:
            yaml.dump(hp, f)
        out = subprocess.run([sys.executable, os.path.join(REPO, "Inference.py"), "-c", str(tmp_path / "ckpt.pt"), "-o", str(d / "out"), "--seed", "7",
                              "--samples", "2"] + (["--wav"] if wav else []), capture_output=True, text=True, timeout=600, cwd=str(d), env=env)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        files = {}
        for label in ("Alpha", "Bravo"):
            for k in (0, 1):
                for sub, ext in (("NPY", "npy"), ("WAV", "wav"))[:2 if wav else 1]:
                    p = d / "out" / sub / f"{label}.S{k}.{ext}"
                    assert p.exists(), p
                    files[(label, k, ext)] = p.read_bytes()
        assert sorted(os.listdir(d / "out" / "NPY")) == ["Alpha.S0.npy", "Alpha.S1.npy", "Bravo.S0.npy", "Bravo.S1.npy"]
        return d, files

    d1, f1 = run("a", 4)
    _, f2 = run("b", 4)
    d3, _ = run("c", 1, wav=False)
    for label in ("Alpha", "Bravo"):
        assert f1[(label, 0, "npy")] != f1[(label, 1, "npy")] and f1[(label, 0, "wav")] != f1[(label, 1, "wav")]
    assert f1 == f2                                                                         # byte-identical from run to run
    for label in ("Alpha", "Bravo"):
        for k in (0, 1):
            a, b = np.load(d1 / "out" / "NPY" / f"{label}.S{k}.npy"), np.load(d3 / "out" / "NPY" / f"{label}.S{k}.npy")
            assert a.shape == b.shape and a.shape[1] == 12 and np.abs(a - b).max() <= 2e-4, (label, k, a.shape, b.shape)
