"""GPU: the objective evaluation (csrc/eval_ops.hip, glow_tts_amd/evaluation.py, Evaluate.py) against the float64 restatement tests/eval_ref.py.
Every observed ratio is printed before it is asserted (`pytest -s`).

Figures of the MI355X run that accompanied the change (observed / bar, worst case of each test) are recorded in DESIGN.md "Objective evaluation"."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import eval_ref as R  # noqa: E402
from helpers import launch_counts, launch_reset  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _pad(arrays, fill=0.0, extra=0):
    n = max(a.shape[0] for a in arrays) + extra
    out = np.full((len(arrays), n) + arrays[0].shape[1:], fill, np.float32)
    for b, a in enumerate(arrays):
        out[b, :a.shape[0]] = a
    return out


def _dtw(xs, ys, extra=(0, 0), **kw):
    """lists of [T, K] arrays -> DTWResult; `extra`: frames of padding beyond the longest"""
    from glow_tts_amd.evaluation import dtw
    return dtw(_dev(_pad(xs, 7.0, extra[0])), [len(x) for x in xs], _dev(_pad(ys, -7.0, extra[1])), [len(y) for y in ys], **kw)


def _pair(res, b):
    """(cost bits, steps, ix, iy, moves) of pair b on the host"""
    n = int(res.steps[b])
    return (int(res.cost[b:b + 1].view(torch.int32)), n, res.ix[b, :n].cpu().numpy(), res.iy[b, :n].cpu().numpy(), res.moves[b].cpu().tolist(),
            res.ix[b, n:].cpu().numpy(), res.iy[b, n:].cpu().numpy())


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4]


# ---------------------------------------------------------------------------------------------------------------- 1. the cepstrum
@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("mel_dim,K", [(80, 13), (80, 1), (80, 32), (20, 13), (20, 1), (20, 19)])
def test_cepstrum_against_float64(mel_dim, K, T):
    """Ragged batch of 3 in both layouts: within 4 x the float32 restatement's own error of the float64 one; padded rows exactly zero."""
    from glow_tts_amd.evaluation import mel_cepstrum
    rng = np.random.default_rng(1000 * mel_dim + 10 * K + T)
    lengths = [T, max(1, T // 2), max(1, T - 1)]
    mels = [rng.uniform(-4, 4, (n, mel_dim)).astype(np.float32) for n in lengths]
    mels[0][0, :3] = (4.0, -4.0, 4.0)                                                          # values at the clip are taken as they are
    want = [R.cepstrum(m, K) for m in mels]
    bar = 4.0 * max(np.abs(R.cepstrum(m, K, dtype=np.float32) - w).max() for m, w in zip(mels, want))
    padded = _pad(mels, -4.0, extra=2)
    for time_major, batch in ((True, padded), (False, padded.transpose(0, 2, 1))):
        got = mel_cepstrum(_dev(batch), lengths, K, 4.0, time_major=time_major).cpu().numpy()
        assert got.shape == (3, T + 2, K) and got.dtype == np.float32
        err = max(np.abs(got[b, :n] - want[b]).max() for b, n in enumerate(lengths))
        print(f"cepstrum Mel {mel_dim} K {K} T {T} time_major {time_major}: error {err:.3e}, bar {bar:.3e}, ratio {err / bar:.3f}")
        assert err <= bar
        for b, n in enumerate(lengths):
            assert not got[b, n:].any()


def test_cepstrum_refuses_what_it_does_not_support():
    from glow_tts_amd import _lib
    from glow_tts_amd.evaluation import mel_cepstrum
    with pytest.raises(ValueError, match="coefficients = 12 at Mel = 12"):
        mel_cepstrum(torch.zeros(1, 12, 5, device=DEV), [5], 12)
    with pytest.raises(_lib.GlowTTSHipError):
        mel_cepstrum(torch.zeros(1, 80, 5), [5])


# ---------------------------------------------------------------------------------------------------------------- 2. DTW, exact cases
EXACT_SHAPES = [(1, 1), (1, 50), (50, 1), (70, 3), (3, 70), (63, 64), (64, 64), (65, 63), (257, 255)]


def _exact_case(content, tx, ty):
    rng = np.random.default_rng(100 * tx + ty)
    if content == "constant":
        return np.full((tx, 1), 3.0), np.full((ty, 1), -5.0)
    if content == "self":
        x = rng.integers(-64, 65, (tx, 1)).astype(np.float64)
        return x, x.copy()
    if content == "doubled":                                                                 # consecutive frames differ: the zero-cost path is forced
        x = ((np.arange(tx) * 37) % 129 - 64.0)[:, None]
        return x, np.repeat(x, 2, axis=0)
    return rng.integers(-64, 65, (tx, 1)).astype(np.float64), rng.integers(-64, 65, (ty, 1)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _exact_reference(content, tx, ty):
    x, y = _exact_case(content, tx, ty)
    return R.dtw(x, y)


@pytest.mark.parametrize("content", ["constant", "self", "doubled", "random"])
@pytest.mark.parametrize("tx,ty", EXACT_SHAPES)
def test_dtw_exact_cases(content, tx, ty):
    """K = 1, integers of magnitude <= 64: every float32 operation is exact, so cost, steps, path and move counts equal the float64 restatement's."""
    x, y = _exact_case(content, tx, ty)
    cost, ix, iy, moves = _exact_reference(content, tx, ty)
    got = _pair(_dtw([x], [y]), 0)
    got_cost = float(np.array([got[0]], np.int32).view(np.float32)[0])
    print(f"dtw exact {content} ({len(x)}, {len(y)}): cost {got_cost} / {cost}, steps {got[1]} / {len(ix)}, moves {got[4]} / {moves}")
    assert got_cost == cost and got[1] == len(ix) and np.array_equal(got[2], ix) and np.array_equal(got[3], iy) and got[4] == moves
    assert (got[5] == -1).all() and (got[6] == -1).all() and len(got[5]) == len(x) + len(y) - 1 - got[1]
    if content == "self":
        assert cost == 0 and np.array_equal(ix, np.arange(len(x))) and np.array_equal(iy, ix)
    if content == "doubled":
        assert cost == 0 and got[1] == 2 * len(x)


# ---------------------------------------------------------------------------------------------------------------- 3. DTW, real-valued cases
@pytest.mark.parametrize("tx,ty", [(37, 96), (200, 131), (1, 50), (513, 640)])
def test_dtw_real_valued_cases(tx, ty):
    """K = 13, seeded normal features.  Every float32 cumulative cost is a sum of at most Tx + Ty - 1 positive terms, each with a relative error of at most about
    (K + 2) 2^-24; rounded addition is monotone, so the rounded recurrence still minimises the computed cost: the chosen path's true cost exceeds the optimum
    by at most twice that relative error.  The bar (Tx + Ty + K + 2) 2^-22 carries a further factor of two."""
    K = 13
    rng = np.random.default_rng(tx * 1000 + ty)
    x, y = rng.standard_normal((tx, K)).astype(np.float32), rng.standard_normal((ty, K)).astype(np.float32)
    optimum = float(R.dtw(x, y)[0])
    cost_bits, n, ix, iy, moves, _, _ = _pair(_dtw([x], [y]), 0)
    cost = float(np.array([cost_bits], np.int32).view(np.float32)[0])
    assert (ix[0], iy[0]) == (0, 0) and (ix[-1], iy[-1]) == (tx - 1, ty - 1)
    di, dj = np.diff(ix), np.diff(iy)
    assert (((di == 1) & (dj == 1)) | ((di == 1) & (dj == 0)) | ((di == 0) & (dj == 1))).all()
    assert moves == [int(((di == 1) & (dj == 1)).sum()), int(((di == 1) & (dj == 0)).sum()), int(((di == 0) & (dj == 1)).sum())]
    true = R.path_cost(x, y, ix, iy)
    bar = (tx + ty + K + 2) * 2.0 ** -22
    print(f"dtw ({tx}, {ty}): path cost / optimum - 1 = {true / optimum - 1:.3e}, |device cost / path cost - 1| = {abs(cost / true - 1):.3e}, bar {bar:.3e}, "
          f"ratios {(true / optimum - 1) / bar:.3f}, {abs(cost / true - 1) / bar:.3f}")
    assert true >= optimum * (1 - 1e-12)                                                      # (two float64 sums of <= 1152 terms taken in different orders)
    assert true <= optimum * (1 + bar)
    assert abs(cost - true) <= bar * true


# ---------------------------------------------------------------------------------------------------------------- 4. bit-identity
def test_dtw_is_bit_identical_alone_in_a_batch_and_at_any_padding():
    rng = np.random.default_rng(4)
    shapes = [(37, 96), (200, 131), (1, 50), (64, 64), (90, 3)]
    xs = [rng.standard_normal((a, 13)).astype(np.float32) for a, _ in shapes]
    ys = [rng.standard_normal((b, 13)).astype(np.float32) for _, b in shapes]
    batch, wide, again = _dtw(xs, ys), _dtw(xs, ys, extra=(17, 40)), _dtw(xs, ys)
    split = _dtw(xs, ys, work_budget=2 * 200 * 33)                                            # two pairs per launch: 3 launches
    for b in range(5):
        want = _pair(batch, b)
        assert want[1] >= max(shapes[b])
        for name, other in (("alone", _pair(_dtw([xs[b]], [ys[b]]), 0)), ("wider padding", _pair(wide, b)), ("second run", _pair(again, b)),
                            ("split batch", _pair(split, b))):
            print(f"pair {b} {shapes[b]} {name}: cost bits {other[0]:#x} / {want[0]:#x}, steps {other[1]} / {want[1]}")
            assert _same(want, other), (b, name)
    for f in ("cost", "steps", "ix", "iy", "moves"):
        assert torch.equal(getattr(batch, f), getattr(again, f)), f


def test_dtw_more_workgroups_than_compute_units():
    rng = np.random.default_rng(5)
    shapes = [(int(a), int(b)) for a, b in rng.integers(1, 13, (300, 2))]
    xs = [rng.standard_normal((a, 4)).astype(np.float32) for a, _ in shapes]
    ys = [rng.standard_normal((b, 4)).astype(np.float32) for _, b in shapes]
    batch, again = _dtw(xs, ys), _dtw(xs, ys)
    assert torch.equal(batch.cost, again.cost) and torch.equal(batch.ix, again.ix) and torch.equal(batch.iy, again.iy) and torch.equal(batch.steps, again.steps)
    for b in rng.choice(300, 10, replace=False).tolist():
        assert _same(_pair(batch, b), _pair(_dtw([xs[b]], [ys[b]]), 0)), b
        cost, ix, iy, _ = R.dtw(xs[b], ys[b])
        assert int(batch.steps[b]) >= max(shapes[b]) and abs(float(batch.cost[b]) - cost) <= 1e-5 * max(cost, 1.0)


def test_dtw_refuses_what_it_does_not_support():
    from glow_tts_amd import _lib
    from glow_tts_amd.evaluation import dtw
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(ValueError, match=r"dtw: x has 4097 frames"):
        dtw(z(1, 4097, 2), [4097], z(1, 5, 2), [5])
    with pytest.raises(ValueError, match=r"dtw: y has 4097 frames"):
        dtw(z(1, 5, 2), [5], z(1, 4097, 2), [4097])
    with pytest.raises(ValueError, match=r"65 features"):
        dtw(z(1, 5, 65), [5], z(1, 5, 65), [5])
    with pytest.raises(ValueError, match=r"x_lengths"):
        dtw(z(1, 5, 2), [0], z(1, 5, 2), [5])
    with pytest.raises(ValueError, match=r"y_lengths"):
        dtw(z(1, 5, 2), [5], z(1, 5, 2), [6])
    with pytest.raises(_lib.GlowTTSHipError):
        dtw(torch.zeros(1, 5, 2), [5], z(1, 5, 2), [5])
    res = dtw(z(1, 4096, 1), [4096], z(1, 4096, 1), [4096])                                   # the largest supported pair: the diagonal
    assert int(res.steps[0]) == 4096 and float(res.cost[0]) == 0.0 and res.moves[0].cpu().tolist() == [4095, 0, 0]
    assert torch.equal(res.ix[0, :4096].cpu(), torch.arange(4096, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 5. the metric
def _cepstrum_bar(mels, K):
    """4 x the float32 restatement's error on these mels (item 1's bar)"""
    return 4.0 * max(np.abs(R.cepstrum(m, K, dtype=np.float32) - R.cepstrum(m, K)).max() for m in mels)


def test_mcd_of_a_mel_against_itself_and_against_itself_plus_a_constant():
    from glow_tts_amd.evaluation import MCD_FACTOR, mcd_dtw
    rng = np.random.default_rng(6)
    K, mel = 13, rng.uniform(-3, 3, (90, 80)).astype(np.float32)
    m = _dev(mel.T[None])
    res = mcd_dtw(m, [90], m, [90], K)
    assert float(res.mcd[0]) == 0.0 and int(res.steps[0]) == 90 and float(res.stretch[0]) == 0.0 and float(res.duration_ratio[0]) == 1.0
    shifted = (mel + np.float32(0.5)).astype(np.float32)
    res = mcd_dtw(m, [90], _dev(shifted.T[None]), [90], K)
    # both cepstra lie within e of the same true cepstrum (the offset cancels for k >= 1): every distance on the diagonal is at most 2 sqrt(K) e, the optimum
    # costs no more than the diagonal and has at least T steps
    bar = MCD_FACTOR * 2.0 * np.sqrt(K) * _cepstrum_bar([mel, shifted], K)
    print(f"mcd of mel + 0.5 against mel: {float(res.mcd[0]):.3e} dB, bar {bar:.3e}, ratio {float(res.mcd[0]) / bar:.3f}")
    assert 0.0 <= float(res.mcd[0]) <= bar


def test_mcd_against_the_float64_chain_and_its_launches():
    from glow_tts_amd.evaluation import MCD_FACTOR, mcd_dtw
    rng = np.random.default_rng(7)
    K, tx, ty = 13, 120, 150
    ref = rng.uniform(-3.5, 3.5, (tx, 80)).astype(np.float32)
    cand = (ref[np.minimum(np.arange(ty) * tx // ty, tx - 1)] + 0.3 * rng.standard_normal((ty, 80))).astype(np.float32)
    want, steps, ix, iy = R.mcd_dtw(ref, cand, K)
    launch_reset()
    res = mcd_dtw(_dev(ref.T[None]), [tx], _dev(cand.T[None]), [ty], K)
    torch.cuda.synchronize()
    counts = {k: n for k, n in launch_counts().items() if n}
    assert counts == {"eval_mel_cepstrum": 2, "eval_dtw": 1}, counts                          # the documented anatomy, and nothing else of the library
    got, n = float(res.mcd[0]), int(res.steps[0])
    # item 3's bar r on the device's optimum over ITS cepstra, and those within e (item 1's bar) of the float64 ones: any path's cost moves by at most
    # 2 sqrt(K) e per step, of which there are at most Tx + Ty - 1
    r, e = (tx + ty + K + 2) * 2.0 ** -22, _cepstrum_bar([ref, cand], K)
    shift = (tx + ty - 1) * 2.0 * np.sqrt(K) * e
    bar = MCD_FACTOR * (r * want * steps / MCD_FACTOR + (1 + r) * shift) / steps
    print(f"mcd (120, 150): device {got:.6f} dB over {n} steps, float64 {want:.6f} dB over {steps} steps, difference {abs(got - want):.3e}, bar {bar:.3e}, "
          f"ratio {abs(got - want) / bar:.3f}")
    assert n == steps and abs(got - want) <= bar
    assert float(res.stretch[0]) == (n - 150) / 150 and float(res.duration_ratio[0]) == 150 / 120


# ---------------------------------------------------------------------------------------------------------------- 6. the entry point
def _tiny_setup(root, mode):
    """The synthetic pattern directory of the other entry-point tests + a randomly initialised tiny checkpoint -> (hp dict, checkpoint path)"""
    import yaml
    from test_gpu_entrypoints import _make_dataset
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    hp = _make_dataset(root, mode)
    hp["Evaluation"] = {"Cepstral_Coefficients": 8}                                           # (12 mel bands)
    torch.manual_seed(0)
    ckpt = os.path.join(root, "ckpt.pt")
    torch.save({"Model": GlowTTS(Recursive_Parse(hp)).state_dict(), "Steps": 0}, ckpt)
    with open(os.path.join(root, "Hyper_Parameters.yaml"), "w") as f:
        yaml.dump(hp, f)
    return hp, ckpt


@pytest.fixture
def keep_hp():
    """The entry points' `main` installs the yaml it is given as the process's hyper-parameters: put back what was there."""
    from glow_tts_amd import hparams
    before = hparams._hp
    yield
    hparams._hp = before


@pytest.mark.late(1)
@pytest.mark.parametrize("mode", ["Vanilla", "SE"])
def test_evaluate_patterns_entry_point(mode, tmp_path, keep_hp):
    """`Evaluate.py -c <tiny checkpoint> --patterns 3 --seed 7` in a child process (it replays hipGraphs): the TSV / JSON numbers are those of `Evaluator` on the
    .npy files `Inference.py --seed 7` writes for the same prompts, and a second run repeats both files byte for byte."""
    from glow_tts_amd import evaluation, hparams, inferencer
    root = str(tmp_path)
    hp, ckpt = _tiny_setup(root, mode)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(REPO, "Evaluate.py"), "-c", ckpt, "--patterns", "3", "--seed", "7", "-o", os.path.join(root, "e1")],
                         capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    first = {n: open(os.path.join(root, "e1", n), "rb").read() for n in ("evaluation.tsv", "evaluation.json")}
    hp_path = os.path.join(root, "Hyper_Parameters.yaml")
    evaluation.main(["-hp", hp_path, "-c", ckpt, "--patterns", "3", "--seed", "7", "-o", os.path.join(root, "e2")])
    for n, want in first.items():
        assert open(os.path.join(root, "e2", n), "rb").read() == want, n
    # the same prompts through Inference.py's main
    pats = evaluation.eval_patterns(hparams.Recursive_Parse(hp), 3)
    assert [p[0] for p in pats] == ["LJ.000", "LJ.001", "LJ.002"]
    with open(os.path.join(root, "eval_prompts.txt"), "w") as f:
        f.write("Label\tText\tLength_Scale\tSpeaker\tGE2E\tProsody\tPitch\n")
        for label, text, speaker, _ in pats:
            f.write(f"{label}\t{text}\t1.0\t{speaker}\t-\t-\t-\n")
    hparams.set_hp(hparams.load_yaml(hp_path))
    inferencer.main(["-c", ckpt, "-t", os.path.join(root, "eval_prompts.txt"), "--seed", "7", "-o", os.path.join(root, "inf")])
    triples = [(p[0], p[3], os.path.join(root, "inf", "NPY", p[0] + ".npy")) for p in pats]
    rows = evaluation.Evaluator(hparams.Recursive_Parse(hp), DEV)(triples)
    tsv, js = evaluation.write_report(rows, os.path.join(root, "direct"), evaluation.evaluation_settings(hparams.Recursive_Parse(hp)))
    assert open(tsv, "rb").read() == first["evaluation.tsv"]
    lines = first["evaluation.tsv"].decode().splitlines()
    assert lines[0].split("\t") == ["label"] + list(evaluation.COLUMNS) and len(lines) == 4
    for line, p in zip(lines[1:], pats):
        cols = dict(zip(lines[0].split("\t"), line.split("\t")))
        print(mode, cols)
        assert cols["label"] == p[0] and int(cols["ref_frames"]) == len(p[3]) and int(cols["steps"]) >= max(len(p[3]), int(cols["cand_frames"]))
        assert float(cols["mcd_db"]) > 0 and cols["f0_rmse_cents"] == cols["vuv_error"] == cols["voiced_steps"] == cols["speaker_cosine"] == ""
    report, direct = json.loads(first["evaluation.json"]), json.load(open(js))
    assert report["summary"] == direct["summary"] and report["settings"] == {"Cepstral_Coefficients": 8} and report["seed"] == 7
    assert report["checkpoint"] == "ckpt.pt" and report["utterances"] == 3 and report["summary"]["mcd_db"]["count"] == 3
    assert report["summary"]["speaker_cosine"] == {"count": 0, "mean": None, "median": None}


def test_evaluate_patterns_refuses_pe_mode(tmp_path, keep_hp):
    import yaml
    from test_gpu_entrypoints import _make_dataset
    from glow_tts_amd import evaluation
    hp = _make_dataset(str(tmp_path), "PE")
    with open(tmp_path / "hp.yaml", "w") as f:
        yaml.dump(hp, f)
    with pytest.raises(ValueError, match=r"Inference\.py.*--pairs"):
        evaluation.main(["-hp", str(tmp_path / "hp.yaml"), "-c", str(tmp_path / "none.pt"), "--patterns", "3", "-o", str(tmp_path / "e")])


def _sweep(sr, seconds, slow=1.0):
    t = np.arange(int(sr * seconds * slow)) / sr / slow                                        # the same sweep, `slow` times as long
    return (0.5 * np.sin(2 * np.pi * (150.0 * t + 0.5 * 100.0 * t * t))).astype(np.float32)      # 150 Hz -> 150 + 100 * seconds Hz


@pytest.mark.late(1)
def test_evaluate_pairs_with_wavs_and_a_speaker_encoder(tmp_path, keep_hp):
    """--pairs on two synthetic wavs - a sine sweep and the same sweep 10 % slower - and on a wav against itself, with --device-frontend and a tiny random GE2E
    checkpoint: F0 columns filled, duration ratio about 1.1, vuv_error (and the F0 error) as the restatement gives them on the device's own pitch tracks and
    path, similarity 1 within 1e-6 for the utterance against itself; without the flag the similarity column stays empty."""
    import yaml
    import ge2e_ref
    from glow_tts_amd import audio, evaluation, hparams
    root = str(tmp_path)
    hp = hparams.load_yaml(hparams.DEFAULT_YAML)
    hp["Speaker_Embedding"].update(Embedding_Size=16)
    hp["Speaker_Embedding"]["GE2E"].update(LSTM={"Sizes": 16, "Stacks": 2}, Inference={"Samples": 3, "Slice_Length": 16, "Overlap_Length": 8})
    sr = hp["Sound"]["Sample_Rate"]
    a, b = os.path.join(root, "sweep.wav"), os.path.join(root, "slow.wav")
    audio.write_wav(a, _sweep(sr, 1.2), sr)
    audio.write_wav(b, _sweep(sr, 1.2, 1.1), sr)
    enc = os.path.join(root, "ge2e.pt")
    torch.save({"Model": ge2e_ref.random_state_dict(ge2e_ref.sizes_of(hp["Sound"]["Mel_Dim"], 16, 2, 16), 5), "Steps": 1}, enc)
    with open(os.path.join(root, "hp.yaml"), "w") as f:
        yaml.dump(hp, f)
    with open(os.path.join(root, "pairs.tsv"), "w") as f:
        f.write(f"slow\t{a}\t{b}\nself\t{a}\t{a}\n")
    argv = ["-hp", os.path.join(root, "hp.yaml"), "--pairs", os.path.join(root, "pairs.tsv"), "--device-frontend"]
    evaluation.main(argv + ["--speaker-encoder", enc, "-o", os.path.join(root, "e1")])
    evaluation.main(argv + ["--speaker-encoder", enc, "-o", os.path.join(root, "e2")])
    evaluation.main(argv + ["-o", os.path.join(root, "e3")])
    for n in ("evaluation.tsv", "evaluation.json"):
        assert open(os.path.join(root, "e1", n), "rb").read() == open(os.path.join(root, "e2", n), "rb").read(), n
    lines = open(os.path.join(root, "e1", "evaluation.tsv")).read().splitlines()
    slow, same = (dict(zip(lines[0].split("\t"), line.split("\t"))) for line in lines[1:])
    print(slow, same, sep="\n")
    assert abs(float(slow["duration_ratio"]) - 1.1) <= 0.03 and int(slow["voiced_steps"]) > 20 and float(slow["mcd_db"]) > 0
    assert float(same["mcd_db"]) == 0 and float(same["f0_rmse_cents"]) == 0 and float(same["vuv_error"]) == 0 and float(same["duration_ratio"]) == 1
    assert abs(float(same["speaker_cosine"]) - 1.0) <= 1e-6 and -1.0 <= float(slow["speaker_cosine"]) <= 1.0 + 1e-6
    # the restatement on the device's own pitch tracks and path
    ev = evaluation.Evaluator(hparams.Recursive_Parse(hp), DEV, device_frontend=True)
    (rm, rf), (cm, cf) = ev.load(a), ev.load(b)
    assert rf is not None and len(rf) == len(rm) and (rf > 0).sum() > 20
    res = evaluation.mcd_dtw(_dev(rm[None]), [len(rm)], _dev(cm[None]), [len(cm)], 13, time_major=True)
    n = int(res.steps[0])
    rmse, vuv, voiced = R.f0_metrics(res.path.ix[0, :n].cpu().numpy(), res.path.iy[0, :n].cpu().numpy(), rf, cf)
    print(f"restated on the device's tracks: rmse {rmse}, vuv {vuv}, voiced {voiced}")
    assert int(slow["voiced_steps"]) == voiced and slow["vuv_error"] == "{:.6f}".format(vuv) and abs(float(slow["f0_rmse_cents"]) - rmse) <= 1e-5
    assert rmse < 100.0                                                                        # the same sweep, time-aligned: well within a semitone
    lines = open(os.path.join(root, "e3", "evaluation.tsv")).read().splitlines()
    assert all(dict(zip(lines[0].split("\t"), line.split("\t")))["speaker_cosine"] == "" for line in lines[1:])
    assert json.load(open(os.path.join(root, "e3", "evaluation.json")))["summary"]["f0_rmse_cents"]["count"] == 2
