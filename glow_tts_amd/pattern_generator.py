"""wav corpus -> pattern directory (the reference's `Pattern_Generator.py` entry point): one pickle per utterance with the keys `data.py` reads, the
metadata pickles of both splits and `Token.yaml`.

    corpus walker -> text filter -> speaker ids, train / eval split -> audio_prep on host threads -> analysis -> <Path>/<DATASET>/<SPEAKER>/<NAME>.PICKLE

The analysis (mel and the YIN pitch track) runs on the device through `frontend.Analyzer`, in batches, while the host threads decode, resample, trim and
normalise the next files; `--host` runs it through `audio.pattern_from_audio` instead and needs no device.  The corpus walkers are written from the
corpora's published layouts and are driven by the `CORPORA` table; any other corpus goes through `--list`."""
import argparse
import os
import pickle
import random
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import audio, data
from .hparams import Recursive_Parse, get_hp, load_yaml

# Corpus layouts.  `index`: a text file with one utterance per line, `sep`-separated, the wav at `wav` formatted with the line's first column, the text in
# column `text_col` (falling back to `text_alt` when that column is missing or empty).  Without `index`: one directory per speaker under `speakers`, every
# wav in it an utterance, its text in the file `text` names; `no_text` lists speakers whose transcripts the corpus lacks; `keep_list` names an optional
# file in the corpus root that lists the utterances to keep (file names, with or without extension), all others are dropped.
CORPORA = {
    "LJ": {"top_db": 60, "index": "metadata.csv", "sep": "|", "wav": "wavs/{id}.wav", "text_col": 2, "text_alt": 1, "speaker": "LJ"},
    "VCTK": {"top_db": 15, "speakers": "wav48", "text": "txt/{speaker}/{id}.txt", "no_text": ("p315",), "keep_list": "VCTK.NonOutlier.txt",
             "speaker": "VCTK.{speaker}"},
}
LIST_TOP_DB = 60
FLUSH_FILES = 64                                                    # utterances handed to the analysis at a time
RUN_AHEAD = 4 * FLUSH_FILES                                        # prepared utterances the host threads may be ahead of their consumer


def walk_corpus(dataset, root, use_text):
    """-> [{'path', 'dataset', 'speaker', 'text' (raw, or None), 'top_db'}] of corpus `dataset` (a key of CORPORA) rooted at `root`."""
    spec, items = CORPORA[dataset], []
    if "index" in spec:
        with open(os.path.join(root, spec["index"]), encoding="utf-8") as f:
            for line in f.read().splitlines():
                cols = line.split(spec["sep"])
                if not cols or not cols[0].strip():
                    continue
                text = cols[spec["text_col"]] if len(cols) > spec["text_col"] and cols[spec["text_col"]].strip() else \
                    (cols[spec["text_alt"]] if len(cols) > spec["text_alt"] else None)
                items.append({"path": os.path.join(root, spec["wav"].format(id=cols[0].strip())), "dataset": dataset, "speaker": spec["speaker"],
                              "text": text, "top_db": spec["top_db"]})
        return items
    keep = None
    if spec.get("keep_list") and os.path.exists(os.path.join(root, spec["keep_list"])):
        with open(os.path.join(root, spec["keep_list"]), encoding="utf-8") as f:
            keep = {os.path.splitext(os.path.basename(x.strip()))[0].lower() for x in f if x.strip()}
    base = os.path.join(root, spec["speakers"])
    for speaker in sorted(os.listdir(base)):
        if not os.path.isdir(os.path.join(base, speaker)):
            continue
        for name in sorted(os.listdir(os.path.join(base, speaker))):
            stem, ext = os.path.splitext(name)
            if ext.lower() != ".wav" or (keep is not None and stem.lower() not in keep):
                continue
            text = None
            if use_text:
                if speaker.lower() in spec.get("no_text", ()):
                    continue
                path = os.path.join(root, spec["text"].format(speaker=speaker, id=stem))
                if not os.path.exists(path):
                    print("No transcript for {}: skipped".format(os.path.join(base, speaker, name)))
                    continue
                with open(path, encoding="utf-8") as f:
                    text = f.read().strip()
            items.append({"path": os.path.join(base, speaker, name), "dataset": dataset, "speaker": spec["speaker"].format(speaker=speaker.upper()),
                          "text": text, "top_db": spec["top_db"]})
    return items


def read_list(path):
    """The generic corpus list: `wav<TAB>dataset<TAB>speaker[<TAB>text[<TAB>top_db]]` per line; a relative wav path is relative to the list."""
    items, here = [], os.path.dirname(os.path.abspath(path))
    with open(path, encoding="utf-8") as f:
        for i, line in enumerate(f.read().splitlines()):
            if not line.strip():
                continue
            cols = [c.strip() for c in line.split("\t")]
            if len(cols) < 3 or not all(cols[:3]):
                raise ValueError("{}:{}: expected wav<TAB>dataset<TAB>speaker[<TAB>text[<TAB>top_db]]".format(path, i + 1))
            items.append({"path": cols[0] if os.path.isabs(cols[0]) else os.path.join(here, cols[0]), "dataset": cols[1], "speaker": cols[2],
                          "text": cols[3] if len(cols) > 3 and cols[3] else None, "top_db": float(cols[4]) if len(cols) > 4 and cols[4] else LIST_TOP_DB})
    return items


def pattern_file(item):
    """<DATASET>/<SPEAKER>/<NAME>.PICKLE; the upper-cased name carries the dataset, the speaker and the wav's base name."""
    stem = os.path.splitext(os.path.basename(item["path"]))[0]
    speaker = item["speaker"] if item["dataset"] in item["speaker"] else "{}.{}".format(item["dataset"], item["speaker"])
    return "/".join([item["dataset"], item["speaker"], "{}.{}.PICKLE".format(speaker, stem).upper()])


def split_eval(items, ratio, minimum, seed=0):
    """(train, eval): max(minimum, int(len * ratio)) utterances drawn with a seeded shuffle of the sorted paths, so a second run draws the same ones."""
    order = sorted(items, key=lambda x: x["path"])
    random.Random(seed).shuffle(order)
    n = min(len(order), max(int(minimum), int(len(order) * float(ratio))))
    return order[n:], order[:n]


def _write(root, item, audio_, mel, pitch, use_text):
    if mel.shape[0] == 0 or mel.shape[0] != pitch.shape[0]:
        raise ValueError("{} mel frames but {} pitch frames".format(mel.shape[0], pitch.shape[0]) if mel.shape[0] else "the clip is too short: no frames")
    pat = {"Audio": audio_.astype(np.float32), "Mel": mel.astype(np.float32), "Pitch": pitch.astype(np.float32), "Speaker_ID": item["speaker_id"],
           "Speaker": item["speaker"], "Dataset": item["dataset"]}
    if use_text:
        pat["Text"] = item["text"]
    target = os.path.join(root, item["file"])
    os.makedirs(os.path.dirname(target), exist_ok=True)
    with open(target + ".tmp", "wb") as f:
        pickle.dump(pat, f, protocol=4)
    os.replace(target + ".tmp", target)                            # an interrupted run leaves no half-written pattern behind


def _skipped(item, err):
    print("Skipped {}: {}".format(item["path"], err))


def _run_ahead(pool, job, items, window):
    """Results of job(item) in order, with at most `window` jobs submitted and not yet consumed: the host threads work ahead of the consumer, but what they
    have prepared and nobody has taken yet stays bounded (a corpus is tens of thousands of files, a prepared utterance about half a megabyte)."""
    queue, it = deque(), iter(items)
    for item in it:
        queue.append(pool.submit(job, item))
        if len(queue) >= window:
            yield queue.popleft().result()
    while queue:
        yield queue.popleft().result()


def generate(items, root, hp, use_text, analyzer=None, max_worker=10):
    """Writes the patterns of `items` that `root` lacks; returns (written, failed).  A FILE that fails - unreadable, too short - is reported and skipped.  An
    error of the device analysis is no file's fault: it ends the run (what is written stays, and the next run skips it)."""
    pending = [x for x in items if not os.path.exists(os.path.join(root, x["file"]))]
    written = failed = 0

    def store(item, a, mel, pitch):
        nonlocal written, failed
        try:
            _write(root, item, a, mel, pitch, use_text)
            written += 1
        except Exception as e:                                     # noqa: BLE001 - this file only; the run goes on
            _skipped(item, e)
            failed += 1

    def flush(batch):
        for (item, a), (mel, pitch) in zip(batch, analyzer([a for _, a in batch], with_pitch=True)):
            store(item, a, mel, pitch)

    def job(item):
        try:
            a = audio.audio_prep(item["path"], hp.Sound.Sample_Rate, item["top_db"]).astype(np.float32)
            if analyzer is not None:
                return item, (a,), None
            return item, (a,) + audio.pattern_from_audio(a, hp, with_pitch=True), None      # host: the whole pattern is made on the worker threads
        except Exception as e:                                     # noqa: BLE001
            return item, None, e

    with ThreadPoolExecutor(max_workers=max(1, int(max_worker))) as pool:
        batch = []
        for item, res, err in _run_ahead(pool, job, pending, RUN_AHEAD):
            if err is not None:
                _skipped(item, err)
                failed += 1
            elif analyzer is None:
                store(item, *res)
            else:
                batch.append((item, res[0]))
                if len(batch) >= FLUSH_FILES:
                    flush(batch)
                    batch = []
        if batch:
            flush(batch)
    return written, failed


def main(argv=None, hp=None):
    ap = argparse.ArgumentParser(description="wav corpus -> pattern pickles, METADATA.PICKLE and Token.yaml")
    ap.add_argument("-hp", "--hyper_parameters", default=None, help="yaml to read instead of ./Hyper_Parameters.yaml")
    ap.add_argument("-lj", "--lj_path", default=None)
    ap.add_argument("-vctk", "--vctk_path", default=None)
    ap.add_argument("--list", default=None, metavar="FILE", help="generic corpus: wav<TAB>dataset<TAB>speaker[<TAB>text[<TAB>top_db]] per line")
    ap.add_argument("-text", "--use_text", action="store_true")
    ap.add_argument("-evalr", "--eval_ratio", default=0.001, type=float)
    ap.add_argument("-evalm", "--eval_min", default=1, type=int)
    ap.add_argument("-mw", "--max_worker", default=10, type=int, help="host threads for decoding, resampling and trimming")
    ap.add_argument("--host", action="store_true", help="analyse on the host (numpy / scipy); no device needed")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if hp is None:
        hp = Recursive_Parse(load_yaml(args.hyper_parameters)) if args.hyper_parameters else get_hp()
    if not hp.Train.Train_Pattern.Path or not hp.Train.Eval_Pattern.Path:
        raise ValueError("Train.Train_Pattern.Path and Train.Eval_Pattern.Path must be set: the patterns are written there")
    analyzer = None
    if not args.host:
        from .frontend import Analyzer
        analyzer = Analyzer(hp, args.device, with_pitch=True)      # geometry errors before any file is read

    items = []
    for dataset, root in (("LJ", args.lj_path), ("VCTK", args.vctk_path)):
        if root is not None:
            found = walk_corpus(dataset, root, args.use_text)
            print("{}: {} utterances found".format(dataset, len(found)))
            items += found
    if args.list is not None:
        items += read_list(args.list)
    if args.use_text:
        kept = []
        for x in items:
            x["text"] = data.text_filtering(x["text"]) if x["text"] is not None else None
            if x["text"] is None:
                print("Text rejected: {}".format(x["path"]))
                continue
            kept.append(x)
        items = kept
    if not items:
        raise ValueError("no utterance to process: give -lj, -vctk or --list a corpus whose texts pass the filter")
    speaker_ids = {s: i for i, s in enumerate(sorted({x["speaker"] for x in items}))}
    for x in items:
        x["speaker_id"], x["file"] = speaker_ids[x["speaker"]], pattern_file(x)
    if args.use_text:
        import yaml
        if not hp.Token_Path:
            raise ValueError("Token_Path is not set: -text writes the token dictionary there")
        os.makedirs(os.path.dirname(os.path.abspath(hp.Token_Path)), exist_ok=True)
        with open(hp.Token_Path, "w", encoding="utf-8") as f:
            yaml.dump(data.make_token_dict([x["text"] for x in items]), f)

    train, evals = split_eval(items, args.eval_ratio, args.eval_min)
    t0, total = time.perf_counter(), [0, 0]
    for part, pattern in ((train, hp.Train.Train_Pattern), (evals, hp.Train.Eval_Pattern)):
        os.makedirs(pattern.Path, exist_ok=True)
        w, f = generate(part, pattern.Path, hp, args.use_text, analyzer, args.max_worker)
        total[0] += w
        total[1] += f
    dt = time.perf_counter() - t0
    print("Patterns written: {} (failed: {}, already there: {}) in {:.2f} s, {:.1f} files/s".format(total[0], total[1], len(items) - total[0] - total[1], dt,
                                                                                                    total[0] / max(dt, 1e-9)))
    for pattern in (hp.Train.Train_Pattern, hp.Train.Eval_Pattern):
        data.write_metadata(pattern.Path, pattern.Metadata_File, hp, use_text=args.use_text)
    return {"written": total[0], "failed": total[1], "seconds": dt, "train": len(train), "eval": len(evals)}
