"""GPU: `Prosody_Visualization.py` end to end on a synthetic pattern directory of 3 speakers x 4 patterns and tiny checkpoints (PE, GR, SE with a GE2E speaker
encoder), `--vectors` / `--labels` without a model, the refusal of a mode with nothing to map, and `Trainer.Prosody_Check_Epoch`."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import tiny_hp_dict

pytestmark = [pytest.mark.gpu, pytest.mark.late(1)]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTS = ["HELLO WORLD.", "A FLOW IS A BIJECTION, IS IT NOT?", "SHORT ONE.", "MONOTONIC ALIGNMENT SEARCH."]
SPEAKERS = ("ANN", "BOB", "CY")
FRAMES = (48, 61, 48, 77)                                                          # per text: two patterns of a speaker share a length (one encoder batch)
PROJECTION = {"Perplexity": 2, "Iterations": 60, "Exaggeration_Iterations": 30}        # (8 vectors, the fewest, allow perplexity 7 / 3)
N = len(SPEAKERS) * len(TEXTS)


def make_corpus(root, mode, ge2e=False):
    """Train/ and Eval/ pattern trees (speaker k's mels are drawn around their own offset), Token.yaml, Hyper_Parameters.yaml and a checkpoint of seeded
    initial weights -> the hp dict"""
    import yaml
    from glow_tts_amd import data
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    rng = np.random.default_rng(11)
    token_dict = data.make_token_dict(TEXTS)
    with open(os.path.join(root, "Token.yaml"), "w") as f:
        yaml.dump(token_dict, f)
    for split in ("Train", "Eval"):
        for k, speaker in enumerate(SPEAKERS):
            d = os.path.join(root, split, "SYN", speaker)
            os.makedirs(d)
            for i, (text, T) in enumerate(zip(TEXTS, FRAMES)):
                T = T + 8 * k
                pat = {"Audio": np.zeros(T * 4, np.float32), "Mel": (rng.normal(0, 1.2, (T, 12)) + (k - 1)).clip(-4, 4).astype(np.float32),
                       "Pitch": rng.random(T).astype(np.float32), "Speaker_ID": k, "Speaker": speaker, "Dataset": "SYN", "Text": text}
                with open(os.path.join(d, f"{speaker}.{i:03d}.PICKLE"), "wb") as f:
                    pickle.dump(pat, f, protocol=4)
        data.write_metadata(os.path.join(root, split), "METADATA.PICKLE")
    hp = tiny_hp_dict(mode)
    hp["HIP_Precision"] = "f32"
    hp["Token_Path"] = os.path.join(root, "Token.yaml")
    hp["Encoder"]["Embedding_Tokens"] = len(token_dict)
    for split, key in (("Train", "Train_Pattern"), ("Eval", "Eval_Pattern")):
        hp["Train"][key].update(Path=os.path.join(root, split), Metadata_File="METADATA.PICKLE")
        hp["Train"][key]["Mel_Length"] = {"Min": 2, "Max": 400}
        hp["Train"][key]["Text_Length"] = {"Min": 1, "Max": 60}
    hp["Train"].update(Batch_Size=4, Max_Step=2, Checkpoint_Save_Interval=100, Logging_Interval=100, Evaluation_Interval=2, Inference_Interval=100,
                       Prosody_Check_Interval=2, Use_Pattern_Cache=True, Inference_Pattern_File_in_Train=None)
    hp["Checkpoint_Path"] = os.path.join(root, "Checkpoint")
    hp["Inference_Batch_Size"] = 3
    hp["Inference_Path"] = os.path.join(root, "Inference")
    hp["HIP_Buckets"] = {"Mel": [128, 256, 384], "Token": [32, 64]}
    hp["Projection"] = dict(PROJECTION)
    if ge2e:
        import ge2e_ref
        sizes = ge2e_ref.sizes_of(12, 16, 2, 16)
        hp["Speaker_Embedding"]["Type"] = "GE2E"
        hp["Speaker_Embedding"]["GE2E"]["LSTM"] = {"Sizes": sizes["H"], "Stacks": sizes["Stacks"]}
        hp["Speaker_Embedding"]["GE2E"]["Inference"] = {"Samples": 3, "Slice_Length": 16, "Overlap_Length": 8}
        hp["Speaker_Embedding"]["GE2E"]["Checkpoint_Path"] = os.path.join(root, "ge2e.pt")
        torch.save({"Model": ge2e_ref.random_state_dict(sizes, 5), "Steps": 1}, hp["Speaker_Embedding"]["GE2E"]["Checkpoint_Path"])
    with open(os.path.join(root, "Hyper_Parameters.yaml"), "w") as f:
        yaml.dump(hp, f)
    torch.manual_seed(0)
    torch.save({"Model": GlowTTS(Recursive_Parse(hp)).state_dict(), "Steps": 0}, os.path.join(root, "ckpt.pt"))
    return hp


def run_tool(root, *args, ok=True):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(REPO, "Prosody_Visualization.py")] + list(args), capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert (r.returncode == 0) == ok, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def read_tree(out):
    files = {}
    for base, _, names in os.walk(out):
        for n in names:
            with open(os.path.join(base, n), "rb") as f:
                files[os.path.relpath(os.path.join(base, n), out)] = f.read()
    return files


def have_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except ImportError:
        return False


def check_map(out, files, n, with_plot=True):
    """-> (rows of map.tsv, map.json)"""
    assert sorted(files) == sorted(["embeddings.npy", "map.tsv", "map.json"] + (["map.png"] if with_plot and have_matplotlib() else []))
    table = files["map.tsv"].decode().splitlines()
    assert table[0].split("\t") == ["label", "speaker", "dataset", "x", "y"] and len(table) == n + 1
    rows = [line.split("\t") for line in table[1:]]
    xy = np.array([[float(r[3]), float(r[4])] for r in rows])
    assert np.isfinite(xy).all() and np.abs(xy.mean(0)).max() <= 1e-5 * max(np.abs(xy).max(), 1e-30)
    info = json.loads(files["map.json"])
    emb = np.load(os.path.join(out, "embeddings.npy"))
    assert emb.dtype == np.float32 and emb.shape == (n, info["D"]) and info["N"] == n
    T = info["settings"]["Iterations"]
    assert info["kl_iterations"] == list(range(0, T, 50)) + [T] and len(info["kl"]) == len(info["kl_iterations"]) and np.isfinite(info["kl"]).all()
    assert set(info["nearest_neighbour_agreement"]) == {"embeddings", "map"} and all(0.0 <= v <= 1.0 for v in info["nearest_neighbour_agreement"].values())
    return rows, info


@pytest.mark.parametrize("mode", ["PE", "GR"])
def test_prosody_map_end_to_end_twice(mode, tmp_path):
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.inferencer import Inferencer
    root = str(tmp_path)
    hp = make_corpus(root, mode)
    args = ["-c", os.path.join(root, "ckpt.pt"), "--patterns", "train", "--seed", "1"]
    run_tool(root, *args, "-o", os.path.join(root, "a"))
    run_tool(root, *args, "-o", os.path.join(root, "b"))
    a, b = read_tree(os.path.join(root, "a")), read_tree(os.path.join(root, "b"))
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a), [k for k in a if a[k] != b.get(k)]
    rows, info = check_map(os.path.join(root, "a"), a, N)
    assert info["what"] == "prosody" and info["settings"]["Perplexity"] == 2 and info["D"] == hp["Prosody_Encoder"]["Size"]
    assert sorted(r[0] for r in rows) == sorted(f"{s}.{i:03d}" for s in SPEAKERS for i in range(len(TEXTS)))
    assert all(r[1] == r[0].split(".")[0] and r[2] == "SYN" for r in rows)
    # every row is the encoder's vector of that pattern alone
    inf = Inferencer(checkpoint_path=os.path.join(root, "ckpt.pt"), hp=Recursive_Parse(hp))
    encoder = inf.model_Dict["GlowTTS"].layer_Dict["Prosody_Encoder"]
    emb = np.load(os.path.join(root, "a", "embeddings.npy"))
    for row, got in zip(rows, emb):
        with open(os.path.join(root, "Train", "SYN", row[1], row[0] + ".PICKLE"), "rb") as f:
            mel = torch.from_numpy(pickle.load(f)["Mel"].T.copy())[None].cuda()
        with torch.no_grad():
            want = encoder(mel, torch.tensor([mel.shape[2]], device="cuda")).cpu().numpy()[0]
        assert np.abs(got - want).max() <= 1e-5, row[0]
    if mode != "PE":
        return
    # --speakers, --per-speaker, --no-plot on the evaluation patterns: 2 of the 3 speakers
    few = os.path.join(root, "few")
    run_tool(root, "-c", os.path.join(root, "ckpt.pt"), "--patterns", "eval", "--speakers", "2", "--per-speaker", "4", "--no-plot", "-o", few)
    rows2, _ = check_map(few, read_tree(few), 8, with_plot=False)
    assert len({r[1] for r in rows2}) == 2


def test_vectors_and_labels_without_a_model(tmp_path):
    root = str(tmp_path)
    rng = np.random.default_rng(2)
    x = (rng.normal(size=(3, 1, 5)) * 6 + rng.normal(size=(3, 10, 5))).reshape(30, 5).astype(np.float32)
    np.save(os.path.join(root, "x.npy"), x)
    with open(os.path.join(root, "l.tsv"), "w") as f:
        f.write("".join(f"p{i}\tg{i // 10}\n" for i in range(30)))
    with open(os.path.join(root, "hp.yaml"), "w") as f:
        f.write("Mode: Vanilla\nProjection: {Perplexity: 5, Iterations: 300, Exaggeration_Iterations: 100}\n")
    out = os.path.join(root, "o")
    run_tool(root, "-hp", os.path.join(root, "hp.yaml"), "--vectors", os.path.join(root, "x.npy"), "--labels", os.path.join(root, "l.tsv"), "-o", out)
    rows, info = check_map(out, read_tree(out), 30)
    assert [r[0] for r in rows] == [f"p{i}" for i in range(30)] and [r[1] for r in rows] == [f"g{i // 10}" for i in range(30)]
    assert np.array_equal(np.load(os.path.join(out, "embeddings.npy")), x) and info["what"] == "vectors"
    assert info["nearest_neighbour_agreement"] == {"embeddings": 1.0, "map": 1.0}                  # three clusters six noise widths apart stay apart in the map
    bad = run_tool(root, "-hp", os.path.join(root, "hp.yaml"), "--vectors", os.path.join(root, "x.npy"), "--labels", os.path.join(root, "l.tsv"), "-o", out,
                   "--patterns", "train", ok=False)
    assert "either --patterns" in bad.stderr


def test_speaker_map_with_a_ge2e_encoder(tmp_path):
    root = str(tmp_path)
    make_corpus(root, "SE", ge2e=True)
    out = os.path.join(root, "o")
    run_tool(root, "-c", os.path.join(root, "ckpt.pt"), "--patterns", "train", "--what", "speaker", "--no-plot", "-o", out)
    rows, info = check_map(out, read_tree(out), N, with_plot=False)
    assert info["what"] == "speaker" and info["D"] == 16
    emb = np.load(os.path.join(out, "embeddings.npy"))
    assert np.abs(np.linalg.norm(emb, axis=1) - 1).max() < 1e-4                                     # d-vectors are unit vectors
    again = os.path.join(root, "again")
    run_tool(root, "-c", os.path.join(root, "ckpt.pt"), "--patterns", "train", "--no-plot", "-o", again)      # SE with GE2E: `speaker` is the default
    assert read_tree(again) == read_tree(out)
    bad = run_tool(root, "-c", os.path.join(root, "ckpt.pt"), "--patterns", "train", "--what", "prosody", "-o", out, ok=False)
    assert "no Prosody_Encoder" in bad.stderr


def test_a_vanilla_checkpoint_is_refused(tmp_path):
    root = str(tmp_path)
    make_corpus(root, "Vanilla")
    r = run_tool(root, "-c", os.path.join(root, "ckpt.pt"), "--patterns", "train", "-o", os.path.join(root, "o"), ok=False)
    assert "Mode Vanilla" in r.stderr and "neither" in r.stderr and not os.path.exists(os.path.join(root, "o"))


def _train(root, with_block):
    import copy
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.trainer import Trainer
    hp = copy.deepcopy(make_corpus(root, "PE"))
    if with_block:
        hp["Train"]["Prosody_Check"] = {"Speakers": 3, "Samples_per_Speaker": 4}
    hp = Recursive_Parse(hp)
    torch.manual_seed(0)
    tr = Trainer(steps=0, hp=hp, workers=0)                                        # (patterns load in this process: no worker start-up in a 2-step run)
    tr.Train()
    assert tr.steps == 2
    return hp


def test_trainer_writes_the_prosody_check(tmp_path):
    hp = _train(str(tmp_path), True)
    out = os.path.join(hp.Inference_Path, "Step-2", "PROSODY")
    rows, info = check_map(out, read_tree(out), N)
    assert info["what"] == "prosody" and info["steps"] == 2 and len({r[1] for r in rows}) == 3


def test_trainer_without_the_block_writes_nothing(tmp_path):
    hp = _train(str(tmp_path), False)
    assert not any("PROSODY" in dirs or "PROSODY" in base for base, dirs, _ in os.walk(str(tmp_path)))
    assert not os.path.exists(hp.Inference_Path) or "PROSODY" not in os.listdir(hp.Inference_Path)
