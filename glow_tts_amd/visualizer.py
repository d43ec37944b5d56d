"""Maps of the conditioning vectors (the reference's Prosody_Visualization.py and Train.py:463-492, Datasets.py:168-214, without TensorBoard):
`python Prosody_Visualization.py -c <checkpoint> --patterns {train,eval} [--what prosody|speaker] [--speakers 50] [--per-speaker 100] [--seed 0] -o DIR
[--no-plot]` selects patterns the reference's way - speakers, then files per speaker, inside the pattern set's Mel_Length bounds - but with
`random.Random(seed)` over sorted lists, runs each one's own mel through the model's Prosody_Encoder (PE, GR) or the GE2E speaker encoder (`--what speaker`),
and maps the vectors into the plane by exact t-SNE on the device (`projection.tsne`).  `--vectors X.npy --labels L.tsv` (label<TAB>group) maps any vectors
without a model.  Outputs, byte-identical from run to run:
  DIR/embeddings.npy   float32 [N, D], the rows in map.tsv's order
  DIR/map.tsv          label, speaker, dataset, x, y
  DIR/map.json         N, D, the settings, the KL series and the nearest-neighbour agreement with the speakers - of the embeddings and of the map
  DIR/map.png          one colour per speaker; only when matplotlib imports and --no-plot is absent
TensorBoard export, UMAP and a PCA start are out of scope."""
import json
import logging
import os
import pickle
import random

import numpy as np
import torch

from . import data, projection
from .hparams import overlay_settings

CHECK_DEFAULTS = {"Speakers": 50, "Samples_per_Speaker": 100}


def prosody_check_settings(hp):
    """The optional yaml block `Train.Prosody_Check` over its defaults, or None when it is absent (then `Trainer.Prosody_Check_Epoch` does nothing)."""
    block = getattr(getattr(hp, "Train", None), "Prosody_Check", None)
    if block is None:
        return None

    def rules(s, need):
        for k in CHECK_DEFAULTS:
            need(k, lambda v: isinstance(v, int) and not isinstance(v, bool) and v >= 1, "an integer >= 1")
    return overlay_settings(block, CHECK_DEFAULTS, "Train.Prosody_Check", "prosody check", rules)


def build_parser():
    """The command line of Prosody_Visualization.py."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--checkpoint", default=None, help="GlowTTS checkpoint (--patterns)")
    ap.add_argument("-hp", "--hyper-parameters", default=None, metavar="YAML", help="default: ./Hyper_Parameters.yaml, else the packaged defaults")
    ap.add_argument("--patterns", default=None, choices=["train", "eval"], help="the pattern directory: Train.Train_Pattern or Train.Eval_Pattern")
    ap.add_argument("--what", default=None, choices=["prosody", "speaker"], help="default: prosody in PE / GR mode, speaker with a GE2E speaker encoder")
    ap.add_argument("--speakers", type=int, default=50, help="at most this many speakers")
    ap.add_argument("--per-speaker", type=int, default=100, help="at most this many patterns of each")
    ap.add_argument("--vectors", default=None, metavar="X.npy", help="map these vectors [N, D] instead of a model's (with --labels)")
    ap.add_argument("--labels", default=None, metavar="L.tsv", help="label<TAB>group, one line per row of --vectors")
    ap.add_argument("--seed", type=int, default=0, help="the selection of patterns, the speaker slices' offsets and the start of the map")
    ap.add_argument("-o", "--out", required=True, metavar="DIR")
    ap.add_argument("--no-plot", action="store_true")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if (args.vectors is None) != (args.labels is None):
        ap.error("--vectors and --labels go together")
    if (args.vectors is None) == (args.patterns is None):
        ap.error("give either --patterns (with -c) or --vectors and --labels")
    if args.patterns is not None and not args.checkpoint:
        ap.error("--patterns needs -c <checkpoint>")
    if args.speakers < 1 or args.per_speaker < 1:
        ap.error("--speakers and --per-speaker must be at least 1")
    return args


def select_patterns(files_by_speaker, speakers, per_speaker, seed, keep=None):
    """Datasets.py:191-202 made repeatable: min(speakers, all) speakers drawn from the sorted names, then min(per_speaker, all) of each one's sorted files, by one
    `random.Random(seed)`; of those, the files `keep(file)` accepts.  -> relative paths, speaker by speaker in the order drawn"""
    rng = random.Random(seed)
    names = sorted(files_by_speaker, key=str)
    out = []
    for name in rng.sample(names, min(int(speakers), len(names))):
        files = sorted(files_by_speaker[name])
        out += [f for f in rng.sample(files, min(int(per_speaker), len(files))) if keep is None or keep(f)]
    return out


def pattern_selection(hp, which, speakers, per_speaker, seed):
    """-> (pattern directory, the selected relative paths) of Train.Train_Pattern / Train.Eval_Pattern, inside its Mel_Length bounds"""
    p = hp.Train.Train_Pattern if which == "train" else hp.Train.Eval_Pattern
    with open(os.path.join(p.Path, p.Metadata_File).replace("\\", "/"), "rb") as f:
        meta = pickle.load(f)
    lo, hi, length = p.Mel_Length.Min, p.Mel_Length.Max, meta["Mel_Length_Dict"]
    return p.Path, select_patterns(meta["File_List_by_Speaker_Dict"], speakers, per_speaker, seed, lambda f: lo <= length[f] <= hi)


def load_patterns(root, files):
    """-> rows [(label, speaker, dataset)], mels [[T, Mel] float32]"""
    rows, mels = [], []
    for name in files:
        with open(os.path.join(root, name).replace("\\", "/"), "rb") as f:
            pat = pickle.load(f)
        rows.append((os.path.splitext(os.path.basename(name))[0], str(pat["Speaker"]), str(pat["Dataset"])))
        mels.append(np.asarray(pat["Mel"], np.float32))
    return rows, mels


@torch.no_grad()
def prosody_vectors(model, mels, batch_size, max_abs_mel, device):
    """Each mel [T, Mel] through `model.layer_Dict["Prosody_Encoder"]` (the model in eval mode) -> float32 [N, Size] on the device, in the order given.  Sorted by
    length and batched by up to `batch_size`, but a batch holds mels of ONE length only: the encoder's strided convolutions read a few frames beyond an
    utterance's end, so beside a longer neighbour a vector would depend on the padding - here it is the vector of the pattern alone, whatever else was selected."""
    encoder = model.layer_Dict["Prosody_Encoder"]
    order = sorted(range(len(mels)), key=lambda i: (mels[i].shape[0], i))
    out = [None] * len(mels)
    s = 0
    while s < len(order):
        e = s + 1
        while e < len(order) and e - s < batch_size and mels[order[e]].shape[0] == mels[order[s]].shape[0]:
            e += 1
        part, s = order[s:e], e
        lengths = torch.tensor([mels[i].shape[0] for i in part], dtype=torch.int64)
        batch = torch.full((len(part), mels[part[0]].shape[1], int(lengths.max())), -float(max_abs_mel))
        for b, i in enumerate(part):
            batch[b, :, :mels[i].shape[0]] = torch.from_numpy(mels[i].T)
        vectors = encoder(batch.to(device), lengths.to(device)).detach().float()
        for b, i in enumerate(part):
            out[i] = vectors[b]
    return torch.stack(out).contiguous()


@torch.no_grad()
def speaker_vectors(encoder, hp, mels, labels, seed, batch_size, device):
    """The d-vector of each mel through the GE2E speaker encoder; the slices' offset of an utterance comes from its label under the seed, as in Align.py."""
    from .inferencer import utterance_seed_words
    ge = hp.Speaker_Embedding.GE2E.Inference
    samples = int(ge.Samples)
    out = []
    for s in range(0, len(mels), batch_size):
        stacks = [data.mels_for_ge2e([m], samples, int(ge.Slice_Length), int(ge.Overlap_Length), rng=np.random.RandomState(utterance_seed_words(seed, label)[0]))
                  for m, label in zip(mels[s:s + batch_size], labels[s:s + batch_size])]
        x = torch.from_numpy(np.concatenate(stacks).astype(np.float32)).transpose(2, 1).contiguous().to(device)
        out.append(encoder(x, samples=samples).detach().float())
    return torch.cat(out).contiguous()


def read_labels(path, n):
    """--labels: label<TAB>group per line -> rows [(label, group, "")]; blank lines are skipped"""
    rows = []
    with open(path, "r", encoding="utf-8") as f:
        for i, line in enumerate(f.read().splitlines()):
            if not line.strip():
                continue
            cols = [c.strip() for c in line.split("\t")]
            if len(cols) != 2 or not all(cols):
                raise ValueError("{}:{}: expected label<TAB>group".format(path, i + 1))
            rows.append((cols[0], cols[1], ""))
    if len(rows) != n:
        raise ValueError("--labels has {} rows, --vectors {}".format(len(rows), n))
    return rows


def plot(path, xy, groups):
    """map.png, one colour per group; False when matplotlib does not import"""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    names = sorted(set(groups))
    cmap = plt.get_cmap("gist_ncar")
    fig = plt.figure(figsize=(10, 10))
    for k, name in enumerate(names):
        pick = np.array([g == name for g in groups])
        plt.scatter(xy[pick, 0], xy[pick, 1], s=9, color=cmap((k + 0.5) / len(names)), label=name)
    if len(names) <= 50:
        plt.legend(fontsize=6, markerscale=1.5)
    plt.tight_layout()
    fig.savefig(path, dpi=120, metadata={"Software": None})
    plt.close(fig)
    return True


def write_map(out_dir, vectors, rows, settings, seed=0, extra=None, with_plot=True):
    """Maps `vectors` [N, D] (float32, on the device; rows: (label, speaker, dataset) each) with `projection.tsne` under `settings` (the `Projection` block)
    and writes the files of the module's docstring.  -> the dict of map.json"""
    if vectors.shape[0] != len(rows):
        raise ValueError("{} vectors, {} labels".format(vectors.shape[0], len(rows)))
    N, D = int(vectors.shape[0]), int(vectors.shape[1])
    if not 1 <= settings["Perplexity"] <= (N - 1) / 3:
        raise ValueError("Projection.Perplexity = {} needs at least {} vectors, {} were selected (supported: 1 <= Perplexity <= (N - 1) / 3)"
                         .format(settings["Perplexity"], int(3 * settings["Perplexity"]) + 1, N))
    vectors = vectors.float().contiguous()
    res = projection.tsne(vectors, perplexity=float(settings["Perplexity"]), iterations=int(settings["Iterations"]),
                          exaggeration_iterations=int(settings["Exaggeration_Iterations"]), learning_rate=float(settings["Learning_Rate"]), seed=seed)
    speakers = [r[1] for r in rows]
    info = dict({"N": N, "D": D, "seed": int(seed), "settings": settings, "kl": res.kl, "kl_iterations": res.kl_iterations,
                 "nearest_neighbour_agreement": {"embeddings": projection.nearest_neighbour_agreement(vectors, speakers),
                                                 "map": projection.nearest_neighbour_agreement(res.y, speakers)}}, **(extra or {}))
    xy = res.y.cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "embeddings.npy"), vectors.cpu().numpy(), allow_pickle=False)
    with open(os.path.join(out_dir, "map.tsv"), "w", encoding="utf-8", newline="\n") as f:
        f.write("label\tspeaker\tdataset\tx\ty\n")
        for (label, speaker, dataset), (px, py) in zip(rows, xy.tolist()):
            f.write("{}\t{}\t{}\t{!r}\t{!r}\n".format(label, speaker, dataset, px, py))
    with open(os.path.join(out_dir, "map.json"), "w", encoding="utf-8", newline="\n") as f:
        json.dump(info, f, indent=2, sort_keys=True)
        f.write("\n")
    if with_plot:
        plot(os.path.join(out_dir, "map.png"), xy, speakers)
    return info


def what_to_map(hp, asked=None):
    """'prosody' or 'speaker', or a ValueError naming the mode that has neither."""
    mode = str(hp.Mode).upper()
    ge2e = mode in ("SE", "GR") and str(hp.Speaker_Embedding.Type).upper() == "GE2E"
    if asked == "prosody" or (asked is None and mode in ("PE", "GR")):
        if mode not in ("PE", "GR"):
            raise ValueError("Mode {}: the model has no Prosody_Encoder (PE and GR have one)".format(hp.Mode))
        return "prosody"
    if asked == "speaker" or (asked is None and ge2e):
        if not ge2e:
            raise ValueError("Mode {} with Speaker_Embedding.Type {}: there is no GE2E speaker encoder to map".format(hp.Mode, hp.Speaker_Embedding.Type))
        return "speaker"
    raise ValueError("Mode {}: the model has neither a Prosody_Encoder (PE, GR) nor a GE2E speaker encoder (SE, GR with Speaker_Embedding.Type GE2E): "
                     "nothing to map - use --vectors / --labels for vectors of your own".format(hp.Mode))


def main(argv=None):
    logging.basicConfig(level=logging.INFO)
    args = parse_args(argv)
    from . import hparams
    if args.hyper_parameters:
        hparams.set_hp(hparams.load_yaml(args.hyper_parameters))
    hp = hparams.get_hp()
    settings = projection.projection_settings(hp)                              # a bad block fails before anything is loaded
    device = torch.device("cuda:0")
    if args.vectors is not None:
        x = np.load(args.vectors, allow_pickle=False)
        if x.ndim != 2:
            raise ValueError("--vectors must hold an array [N, D], got {}".format(list(x.shape)))
        rows = read_labels(args.labels, x.shape[0])
        vectors, extra = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device), {"what": "vectors"}
    else:
        what = what_to_map(hp, args.what)                                      # (before the checkpoint is loaded)
        root, files = pattern_selection(hp, args.patterns, args.speakers, args.per_speaker, args.seed)
        rows, mels = load_patterns(root, files)
        batch = int(hp.Inference_Batch_Size or hp.Train.Batch_Size)
        if what == "prosody":
            from .inferencer import Inferencer
            inf = Inferencer(checkpoint_path=args.checkpoint, hp=hp, device=device)
            vectors = prosody_vectors(inf.model_Dict["GlowTTS"], mels, batch, hp.Sound.Max_Abs_Mel, device)
        else:
            from . import speaker_encoder
            path = getattr(hp.Speaker_Embedding.GE2E, "Checkpoint_Path", None)
            encoder = speaker_encoder.GE2E.from_checkpoint(hp, device, path) if path else \
                speaker_encoder.from_glowtts_checkpoint(hp, device, torch.load(args.checkpoint, map_location="cpu")["Model"])
            if encoder is None:
                raise ValueError("no GE2E speaker encoder: set Speaker_Embedding.GE2E.Checkpoint_Path or give a checkpoint that carries one")
            vectors = speaker_vectors(encoder, hp, mels, [r[0] for r in rows], args.seed, batch, device)
        extra = {"what": what, "checkpoint": os.path.basename(args.checkpoint), "patterns": args.patterns}
    info = write_map(args.out, vectors, rows, settings, args.seed, extra, with_plot=not args.no_plot)
    logging.info("final KL {:.4f}; nearest-neighbour agreement with the speakers: embeddings {:.3f}, map {:.3f}".format(
        info["kl"][-1], info["nearest_neighbour_agreement"]["embeddings"], info["nearest_neighbour_agreement"]["map"]))
    print(os.path.join(args.out, "map.tsv"))
