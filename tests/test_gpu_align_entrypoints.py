"""GPU: `Align.py` end to end on the synthetic pattern directory of tests/test_gpu_entrypoints.py and a tiny checkpoint: durations, alignment tables and
ground-truth-aligned pattern trees, byte-identical from run to run; the vocoder trainer samples and steps on the GTA tree unchanged."""
import copy
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_entrypoints import TEXTS, _make_dataset
from test_gpu_pwg_trainer import FRAMES, HOP, hp_dict as pwg_hp_dict, trainer as pwg_trainer

pytestmark = [pytest.mark.gpu, pytest.mark.late(1)]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_corpus(root, mode, ge2e=False):
    """tests/test_gpu_entrypoints.py's corpus with HOP samples of audio under every frame; a checkpoint of seeded initial weights -> the hp dict"""
    import yaml
    from glow_tts_amd import data
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    hp = _make_dataset(root, mode)
    hp["Sound"]["Frame_Shift"] = HOP
    if ge2e:                                                                       # this package's own speaker encoder, seeded weights; a window of 32 frames
        import ge2e_ref
        sizes = ge2e_ref.sizes_of(12, 16, 2, 16)
        hp["Speaker_Embedding"]["Type"] = "GE2E"
        hp["Speaker_Embedding"]["GE2E"]["LSTM"] = {"Sizes": sizes["H"], "Stacks": sizes["Stacks"]}
        hp["Speaker_Embedding"]["GE2E"]["Inference"] = {"Samples": 3, "Slice_Length": 16, "Overlap_Length": 8}
        hp["Speaker_Embedding"]["GE2E"]["Checkpoint_Path"] = os.path.join(root, "ge2e.pt")
        torch.save({"Model": ge2e_ref.random_state_dict(sizes, 5), "Steps": 1}, hp["Speaker_Embedding"]["GE2E"]["Checkpoint_Path"])
    rng = np.random.default_rng(9)
    for split in ("Train", "Eval"):
        d = os.path.join(root, split, "LJ", "LJ")
        for name in sorted(os.listdir(d)):
            with open(os.path.join(d, name), "rb") as f:
                pat = pickle.load(f)
            pat["Audio"] = (rng.standard_normal(pat["Mel"].shape[0] * HOP) * 0.3).astype(np.float32)
            with open(os.path.join(d, name), "wb") as f:
                pickle.dump(pat, f, protocol=4)
        data.write_metadata(os.path.join(root, split), "METADATA.PICKLE")
    with open(os.path.join(root, "Hyper_Parameters.yaml"), "w") as f:
        yaml.dump(hp, f)
    torch.manual_seed(0)
    torch.save({"Model": GlowTTS(Recursive_Parse(hp)).state_dict(), "Steps": 0}, os.path.join(root, "ckpt.pt"))
    return hp


def run_align(root, out, *extra):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(REPO, "Align.py"), "-c", os.path.join(root, "ckpt.pt"), "--patterns", "train", "-o", out] + list(extra),
                       capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    files = {}
    for base, _, names in os.walk(out):
        for n in names:
            with open(os.path.join(base, n), "rb") as f:
                files[os.path.relpath(os.path.join(base, n), out)] = f.read()
    return files


def check_outputs(root, out, hp, files):
    from glow_tts_amd import data
    labels = [f"LJ.{i:03d}" for i in range(len(TEXTS))]
    ns, mel_dim = hp["Decoder"]["Num_Squeeze"], hp["Sound"]["Mel_Dim"]
    assert sorted(files) == sorted(["alignment.tsv", "GTA/METADATA.PICKLE"] + [f"DUR/{x}.npy" for x in labels] + [f"ALIGN/{x}.tsv" for x in labels] +
                                   [f"GTA/LJ/LJ/{x}.PICKLE" for x in labels])
    table = files["alignment.tsv"].decode().splitlines()
    assert table[0].split("\t") == ["label", "tokens", "frames", "score", "min_duration", "max_duration"] and [row.split("\t")[0] for row in table[1:]] == labels
    for label, text, row in zip(labels, TEXTS, table[1:]):
        with open(os.path.join(root, "Train", "LJ", "LJ", label + ".PICKLE"), "rb") as f:
            src = pickle.load(f)
        frames = (src["Mel"].shape[0] // ns) * ns
        dur = np.load(os.path.join(out, "DUR", label + ".npy"))
        assert dur.dtype == np.int32 and dur.shape == (len(text) + 2,) and int(dur.sum()) == frames and (dur >= 0).all()
        cols = row.split("\t")
        assert cols[1:3] == [str(len(text) + 2), str(frames)] and np.isfinite(float(cols[3])) and cols[4:] == [str(dur.min()), str(dur.max())]
        lines = files[f"ALIGN/{label}.tsv"].decode().splitlines()
        assert lines[0] == "symbol\tstart\tend" and [x.split("\t")[0] for x in lines[1:]] == ["<S>"] + list(text) + ["<E>"]
        assert float(lines[1].split("\t")[1]) == 0.0
        assert abs(float(lines[-1].split("\t")[2]) - frames * hp["Sound"]["Frame_Shift"] / hp["Sound"]["Sample_Rate"]) <= 1e-6
        with open(os.path.join(out, "GTA", "LJ", "LJ", label + ".PICKLE"), "rb") as f:
            gta = pickle.load(f)
        assert list(gta) == list(src) and set(gta) <= set(data.PATTERN_KEYS)
        assert gta["Mel"].dtype == np.float32 and gta["Mel"].shape == (frames, mel_dim) and np.isfinite(gta["Mel"]).all()
        assert gta["Audio"].tobytes() == src["Audio"].tobytes() and gta["Audio"].dtype == src["Audio"].dtype
        assert all(np.array_equal(gta[k], src[k]) for k in src if k not in ("Mel", "Audio"))
        assert not np.array_equal(gta["Mel"], src["Mel"][:frames])
    with open(os.path.join(out, "GTA", "METADATA.PICKLE"), "rb") as f:
        meta = pickle.load(f)
    assert sorted(meta["File_List"]) == [f"LJ/LJ/{x}.PICKLE" for x in labels]


def test_align_writes_reproducible_durations_and_gta_patterns(tmp_path):
    root = str(tmp_path)
    hp = make_corpus(root, "Vanilla")
    a = run_align(root, os.path.join(root, "a"), "--gta", "--seed", "0")
    b = run_align(root, os.path.join(root, "b"), "--gta", "--seed", "0")
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a), [k for k in a if a[k] != b.get(k)]
    check_outputs(root, os.path.join(root, "a"), hp, a)
    # the vocoder trainer on the GTA tree, unchanged: a batch from its sampler and one step at the tiny vocoder sizes
    d = pwg_hp_dict(root)
    d["Train"]["Train_Pattern"].update(Path=os.path.join(root, "a", "GTA"))
    tr = pwg_trainer(copy.deepcopy(d))
    mel, target = tr.sampler["Train"].batch(0)
    assert mel.shape[1:] == (hp["Sound"]["Mel_Dim"], FRAMES) and target.shape[1] == FRAMES * HOP and mel.shape[0] == target.shape[0]
    with open(os.path.join(root, "a", "GTA", tr.sampler["Train"].plan(0)[0][0]), "rb") as f:
        first = pickle.load(f)
    f0 = tr.sampler["Train"].plan(0)[0][1]
    assert np.array_equal(mel[0].numpy(), first["Mel"][f0:f0 + FRAMES].T)                      # the batch holds GTA mels
    before = {k: v.detach().clone() for k, v in tr.model.params.items()}
    tr.Train_Step(mel, target)
    torch.cuda.synchronize()
    assert tr.steps == 1 and all(torch.isfinite(v).all() for v in tr.model.params.values())
    assert any(not torch.equal(before[k], v) for k, v in tr.model.params.items())


def test_align_in_ge2e_mode_repeats_without_a_seed(tmp_path):
    """GE2E mode, no --seed: the pattern's own mel is the speaker reference, every mel is longer than the slices' window of 32 frames, so an offset is
    drawn for every utterance - from the label, not from `np.random`: plain alignment and `--gta --noise-scale 0` repeat byte for byte across processes."""
    root = str(tmp_path)
    hp = make_corpus(root, "SE", ge2e=True)
    a = run_align(root, os.path.join(root, "a"), "--gta", "--noise-scale", "0")
    b = run_align(root, os.path.join(root, "b"), "--gta", "--noise-scale", "0")
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a), [k for k in a if a[k] != b.get(k)]
    check_outputs(root, os.path.join(root, "a"), hp, a)
    for i in range(len(TEXTS)):
        assert int(np.load(os.path.join(root, "a", "DUR", f"LJ.{i:03d}.npy")).sum()) > 32
    plain = run_align(root, os.path.join(root, "p"))
    assert sorted(plain) == sorted(k for k in a if not k.startswith("GTA/")) and all(plain[k] == a[k] for k in plain)


def test_align_in_gr_mode_reads_speaker_and_pitch_from_the_patterns(tmp_path):
    root = str(tmp_path)
    hp = make_corpus(root, "GR")
    out = os.path.join(root, "o")
    files = run_align(root, out, "--gta", "--seed", "3", "--noise-scale", "0.667")
    check_outputs(root, out, hp, files)
    few = run_align(root, os.path.join(root, "few"), "--limit", "2")                           # no --gta: durations and tables only
    assert sorted(few) == sorted(["alignment.tsv"] + [f"{sub}/LJ.{i:03d}.{ext}" for i in range(2) for sub, ext in (("DUR", "npy"), ("ALIGN", "tsv"))])
    assert len(few["alignment.tsv"].decode().splitlines()) == 3
