"""Teacher-forced alignment of a pattern directory (no counterpart in the reference): `python Align.py -c <checkpoint> --patterns {train,eval} [--limit N]
-o DIR [--gta] [--seed 0] [--noise-scale 1.0]` runs a trained GlowTTS over its own training recordings (`Inferencer.Align` -> `GlowTTS.teacher_forced`) and
writes
  DIR/alignment.tsv        one row per utterance: label, tokens, frames, score, shortest and longest duration
  DIR/DUR/<label>.npy      int32 [Tt]: frames per token, <S> and <E> included
  DIR/ALIGN/<label>.tsv    symbol, start s, end s (frames * Frame_Shift / Sample_Rate)
and, with --gta, a pattern tree DIR/GTA/<the source's relative path> with the source pattern's keys, `Mel` replaced by the model's own mel for the recording
(ground-truth aligned: sampled from the prior along the recording's alignment, through the inverse flows) and a metadata pickle - a directory
`Train.Train_Pattern.Path` can point at to fine-tune the vocoder on the mels it will see at inference time.  `score` is the mean log-prior density per
element along the alignment, the quantity the alignment search maximised; it is not a likelihood (no log-determinants).  Every output is a function of the
checkpoint, the patterns and the seed: byte-identical from run to run (GE2E mode: the offset of the speaker slices comes from the label under the seed,
seed 0 without one).  A label is the pattern's file name without its extension; two patterns that share one are refused before anything is written."""
import logging
import os
import pickle

import numpy as np

from . import data

CHUNK_BATCHES = 16                                                              # patterns held in memory at a time: this many batches


def build_parser():
    """The command line of Align.py."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--checkpoint", required=True, help="GlowTTS checkpoint")
    ap.add_argument("-hp", "--hyper-parameters", default=None, metavar="YAML", help="default: ./Hyper_Parameters.yaml, else the packaged defaults")
    ap.add_argument("--patterns", required=True, choices=["train", "eval"], help="the pattern directory: Train.Train_Pattern or Train.Eval_Pattern")
    ap.add_argument("--limit", type=int, default=None, metavar="N", help="only the first N patterns, in metadata order")
    ap.add_argument("-o", "--out", required=True, metavar="DIR")
    ap.add_argument("--gta", action="store_true", help="also write DIR/GTA: the patterns with `Mel` replaced by the model's own, frame-aligned mel")
    ap.add_argument("--seed", type=int, default=None, help="the noise of --gta: an utterance's mel depends on this seed and its label only")
    ap.add_argument("--noise-scale", type=float, default=1.0, help="sampling temperature of --gta (the default is Inference.py's: the mels the vocoder will see)")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.gta and args.seed is None and args.noise_scale != 0.0:
        ap.error("--gta draws its noise from --seed: give --seed, or --noise-scale 0 for the prior's mean")
    if args.limit is not None and args.limit < 1:
        ap.error("--limit must be at least 1")
    return args


def pattern_files(hp, which, limit=None):
    """-> (pattern directory, the first `limit` (None: all) relative paths of its metadata's File_List)"""
    p = hp.Train.Train_Pattern if which == "train" else hp.Train.Eval_Pattern
    with open(os.path.join(p.Path, p.Metadata_File).replace("\\", "/"), "rb") as f:
        files = pickle.load(f)["File_List"]
    return p.Path, list(files[:limit])


def label_of(name):
    """relative path of a pattern -> its label: the file name without the extension"""
    return os.path.splitext(os.path.basename(name))[0]


def check_labels(files):
    """DUR/ and ALIGN/ are flat: two patterns of one file name in different sub-directories would overwrite each other's files"""
    seen = {}
    for name in files:
        other = seen.setdefault(label_of(name), name)
        if other != name:
            raise ValueError("patterns {} and {} share the label {!r}: DIR/DUR and DIR/ALIGN are named by label - rename one, or align them in separate "
                             "runs".format(other, name, label_of(name)))


def _write_text(path, text):
    with open(path, "w", encoding="utf-8", newline="\n") as f:
        f.write(text)


def write_alignment(out_dir, label, text, result, seconds_per_frame):
    """DUR/<label>.npy and ALIGN/<label>.tsv of one `Inferencer.Align` result -> its row of alignment.tsv"""
    dur = np.asarray(result["durations"], np.int32)
    np.save(os.path.join(out_dir, "DUR", label + ".npy"), dur, allow_pickle=False)
    symbols = ["<S>"] + list(text) + ["<E>"]
    ends = np.cumsum(dur.astype(np.int64))
    lines = ["{}\t{:.6f}\t{:.6f}".format(s, (e - d) * seconds_per_frame, e * seconds_per_frame) for s, d, e in zip(symbols, dur.tolist(), ends.tolist())]
    _write_text(os.path.join(out_dir, "ALIGN", label + ".tsv"), "symbol\tstart\tend\n" + "\n".join(lines) + "\n")
    return "\t".join([label, str(len(dur)), str(result["frames"]), "{:.6f}".format(result["score"]), str(int(dur.min())), str(int(dur.max()))])


def main(argv=None):
    logging.basicConfig(level=logging.INFO)
    args = parse_args(argv)
    from . import hparams
    if args.hyper_parameters:
        hparams.set_hp(hparams.load_yaml(args.hyper_parameters))
    hp = hparams.get_hp()
    from .inferencer import Inferencer
    root, files = pattern_files(hp, args.patterns, args.limit)
    check_labels(files)                                                         # (before the checkpoint is loaded or anything is written)
    inf = Inferencer(checkpoint_path=args.checkpoint, hp=hp)
    mode = hp.Mode.upper()
    for sub in ("DUR", "ALIGN") + (("GTA",) if args.gta else ()):
        os.makedirs(os.path.join(args.out, sub), exist_ok=True)
    seconds_per_frame = float(hp.Sound.Frame_Shift) / float(hp.Sound.Sample_Rate)
    rows = []
    step = CHUNK_BATCHES * int(hp.Inference_Batch_Size or hp.Train.Batch_Size)
    for s in range(0, len(files), step):
        part = files[s:s + step]
        pats = []
        for name in part:
            with open(os.path.join(root, name).replace("\\", "/"), "rb") as f:
                pats.append(pickle.load(f))
        labels = [label_of(name) for name in part]
        mels = [np.asarray(p["Mel"], np.float32) for p in pats]
        results = inf.Align([data.text_to_token(p["Text"], inf.token_Dict) for p in pats],
                            [(m, np.asarray(p["Pitch"], np.float32)) for m, p in zip(mels, pats)] if mode == "GR" else mels,
                            speakers=[int(p["Speaker_ID"]) for p in pats] if mode in ("SE", "GR") and not inf.ge2e_mode else None,
                            speaker_references=mels if inf.ge2e_mode else None, labels=labels, seed=args.seed, noise_scale=args.noise_scale,
                            reconstruct=args.gta)
        for name, label, pat, r in zip(part, labels, pats, results):
            rows.append(write_alignment(args.out, label, pat["Text"], r, seconds_per_frame))
            if args.gta:
                path = os.path.join(args.out, "GTA", name).replace("\\", "/")
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with open(path, "wb") as f:
                    pickle.dump(dict(pat, Mel=r["mel"]), f, protocol=4)
    _write_text(os.path.join(args.out, "alignment.tsv"), "label\ttokens\tframes\tscore\tmin_duration\tmax_duration\n" + "\n".join(rows) + "\n")
    if args.gta:
        p = hp.Train.Train_Pattern if args.patterns == "train" else hp.Train.Eval_Pattern
        data.write_metadata(os.path.join(args.out, "GTA"), p.Metadata_File, hp)
    print(os.path.join(args.out, "alignment.tsv"))
