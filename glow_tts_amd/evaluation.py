"""Objective evaluation of synthesised utterances against recordings (Evaluate.py): mel-cepstral distortion along a dynamic-time-warping (DTW) path, log-F0 and
voicing errors along the same path, and the cosine of the two GE2E d-vectors.

    mel [B, Mel, T] --eval_mel_cepstrum (one launch per side)--> cepstra [B, T, K] --eval_dtw (one launch, one workgroup per pair)--> cost, steps, path
    MCD = (10 sqrt 2 / ln 10) cost / steps  [dB]

The cepstrum is this project's own contract - the orthonormal DCT-II of the log mel amplitudes, coefficients 1 .. K (`mel_cepstrum`) - not SPTK's
mel-generalised cepstrum: figures compare checkpoints of this project with each other, not with numbers from papers.  The kernels are csrc/eval_ops.hip; the
F0 metrics are plain torch indexing over the path, on the device.  Band-constrained DTW, WORLD / SPTK cepstra, PESQ / STOI / MOS predictors and
evaluation inside the trainer are out of scope."""
import json
import logging
import math
import os
import pickle

import numpy as np
import torch

from . import _lib, abi, data
from .hparams import overlay_settings

MCD_FACTOR = 10.0 * math.sqrt(2.0) / math.log(10.0)
WORK_BUDGET = 256 << 20                                               # bytes of back-pointers per `dtw` launch (32 x 800 x 800 frames are 5 MiB)
PAIR_BATCH = 32                                                       # pairs per `Evaluator` batch
DEFAULTS = {"Cepstral_Coefficients": 13}
COLUMNS = ("ref_frames", "cand_frames", "mcd_db", "steps", "stretch_share", "duration_ratio", "f0_rmse_cents", "vuv_error", "voiced_steps", "speaker_cosine")
F0_HOP = 256                                                          # the pitch track is analysed every 256 samples whatever the yaml says (frontend.YIN_W_STEP)


def evaluation_settings(hp):
    """The optional yaml block `Evaluation` over its defaults; an unknown key raises a ValueError naming it."""
    s = overlay_settings(getattr(hp, "Evaluation", None), DEFAULTS, "Evaluation", "evaluation", lambda s, need: None)
    k = s["Cepstral_Coefficients"]
    if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k > abi.DTW_MAX_K:
        raise ValueError("Evaluation.Cepstral_Coefficients = {!r} (an integer in [1, {}])".format(k, abi.DTW_MAX_K))
    return s


# ---------------------------------------------------------------------------------------------------------------- kernels' wrappers
_BASIS = {}


def dct_basis(mel_dim, coefficients):
    """[K, Mel] float64: sqrt(2 / Mel) cos(pi k (m + 1/2) / Mel), k = 1 .. K - the orthonormal DCT-II without its 0th row."""
    k = np.arange(1, coefficients + 1, dtype=np.float64)[:, None]
    m = np.arange(mel_dim, dtype=np.float64)[None, :]
    return math.sqrt(2.0 / mel_dim) * np.cos(np.pi * k * (m + 0.5) / mel_dim)


def _lengths(lengths, n, device, dtype):
    return torch.as_tensor(lengths).to(device=device, dtype=dtype).reshape(n).contiguous()


def mel_cepstrum(mels, mel_lengths, coefficients=13, max_abs_mel=4.0, time_major=False):
    """mels [B, Mel, T] as the models emit them (time_major: [B, T, Mel]), fp32 on the device, in the normalisation of `audio.mel_generate` -> cepstra [B, T, K]
    fp32: c_k = sqrt(2 / Mel) sum_m L_m cos(pi k (m + 1/2) / Mel), k = 1 .. K, L the natural log of the mel amplitude; rows at or beyond an utterance's
    length are zeros.  The energy coefficient c_0 is left out, so a constant offset of the mel drops out."""
    if not torch.is_tensor(mels) or not mels.is_cuda:
        raise _lib.GlowTTSHipError("mel_cepstrum: expected a device tensor (the HIP path has no CPU fallback)")
    if mels.dim() != 3 or mels.dtype != torch.float32:
        raise ValueError("mel_cepstrum: expected fp32 mels [B, Mel, T], got {} {}".format(mels.dtype, list(mels.shape)))
    mels = mels.contiguous()
    B, Mel, T = (mels.shape[0], mels.shape[2], mels.shape[1]) if time_major else tuple(mels.shape)
    K = int(coefficients)
    L = _lib.api()
    if not L.glowtts_mel_cepstrum_supported(Mel, K):
        raise ValueError("mel_cepstrum: coefficients = {} at Mel = {} is not supported (1 <= coefficients <= 64, coefficients < Mel <= 512, "
                         "Mel * coefficients <= 4096)".format(K, Mel))
    key = (Mel, K, str(mels.device))
    if key not in _BASIS:
        _BASIS[key] = torch.from_numpy(dct_basis(Mel, K).astype(np.float32)).to(mels.device)
    lengths = _lengths(mel_lengths, B, mels.device, torch.int64)
    cep = torch.empty(B, T, K, dtype=torch.float32, device=mels.device)
    sb, st, sm = (T * Mel, Mel, 1) if time_major else (Mel * T, 1, T)
    L.glowtts_mel_cepstrum(_lib.ptr(mels), _lib.ptr(lengths), _lib.ptr(_BASIS[key]), _lib.ptr(cep), B, T, Mel, K, sb, st, sm, float(max_abs_mel), _lib.stream())
    return cep


class DTWResult:
    """cost [B] fp32, steps [B] int32, ix / iy [B, Tx_max + Ty_max - 1] int32 (the path in forward order, -1 beyond `steps`), moves [B, 3] int32 (the
    number of diagonal, (i-1, j) and (i, j-1) steps) - all on the device."""
    __slots__ = ("cost", "steps", "ix", "iy", "moves")

    def __init__(self, cost, steps, ix, iy, moves):
        self.cost, self.steps, self.ix, self.iy, self.moves = cost, steps, ix, iy, moves


def _host_lengths_check(name, lengths, limit):
    """Lengths that are already on the host are checked there; a device vector is not pulled back (the kernel answers a bad length with cost NaN, steps 0)."""
    if torch.is_tensor(lengths) and lengths.is_cuda:
        return
    v = np.asarray(lengths if not torch.is_tensor(lengths) else lengths.numpy()).reshape(-1)
    if v.size and (v.min() < 1 or v.max() > limit):
        raise ValueError("dtw: every element of {} must lie in [1, {}], got [{}, {}]".format(name, limit, v.min(), v.max()))


def dtw(x, x_lengths, y, y_lengths, work_budget=WORK_BUDGET):
    """Unconstrained DTW of B pairs of feature sequences x [B, Tx, K], y [B, Ty, K] (fp32, on the device; lengths at least 1) under the Euclidean local cost
    -> DTWResult.  Tie-break of the predecessor: the diagonal, then (i-1, j), then (i, j-1).  A pair's result is bit-identical alone, in any batch and at any
    padding.  A batch whose back-pointers exceed `work_budget` bytes goes through several launches."""
    for name, t in (("x", x), ("y", y)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.GlowTTSHipError("dtw: expected device tensors (the HIP path has no CPU fallback)")
        if t.dim() != 3 or t.dtype != torch.float32 or t.shape[0] < 1:
            raise ValueError("dtw: {} must be fp32 [B, T, K], got {} {}".format(name, t.dtype, list(t.shape)))
        if t.shape[1] < 1 or t.shape[1] > abi.DTW_MAX_FRAMES:
            raise ValueError("dtw: {} has {} frames, supported are 1 .. {}".format(name, t.shape[1], abi.DTW_MAX_FRAMES))
    if x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2]:
        raise ValueError("dtw: x {} and y {} differ in batch or feature size".format(list(x.shape), list(y.shape)))
    B, Tx, K = x.shape
    Ty = y.shape[1]
    if K < 1 or K > abi.DTW_MAX_K:
        raise ValueError("dtw: x, y have {} features per frame, supported are 1 .. {}".format(K, abi.DTW_MAX_K))
    _host_lengths_check("x_lengths", x_lengths, Tx)
    _host_lengths_check("y_lengths", y_lengths, Ty)
    L = _lib.api()
    if not L.glowtts_dtw_supported(Tx, Ty, K):
        raise ValueError("dtw: x {} / y {} is not supported".format(list(x.shape), list(y.shape)))
    dev = x.device
    x, y = x.contiguous(), y.contiguous()
    xl, yl = _lengths(x_lengths, B, dev, torch.int32), _lengths(y_lengths, B, dev, torch.int32)
    P = Tx + Ty - 1
    res = DTWResult(torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                    torch.empty(B, P, dtype=torch.int32, device=dev), torch.empty(B, P, dtype=torch.int32, device=dev),
                    torch.empty(B, 3, dtype=torch.int32, device=dev))
    per_pair = int(L.glowtts_dtw_work_bytes(Tx, Ty))
    chunk = max(1, min(B, int(work_budget) // per_pair, 65535))
    work = torch.empty(chunk * per_pair, dtype=torch.uint8, device=dev)
    for s in range(0, B, chunk):
        e = min(B, s + chunk)
        L.glowtts_dtw(_lib.ptr(x[s:e]), _lib.ptr(xl[s:e]), _lib.ptr(y[s:e]), _lib.ptr(yl[s:e]), _lib.ptr(work), _lib.ptr(res.cost[s:e]), _lib.ptr(res.steps[s:e]),
                      _lib.ptr(res.ix[s:e]), _lib.ptr(res.iy[s:e]), _lib.ptr(res.moves[s:e]), e - s, Tx, Ty, K, _lib.stream())
    return res


class MCDResult:
    """Per pair, on the device: mcd [B] float64 in dB, steps [B] int32, stretch [B] float64 = (steps - max(Tx, Ty)) / max(Tx, Ty), duration_ratio [B] float64
    = Ty / Tx, and path: the DTWResult."""
    __slots__ = ("mcd", "steps", "stretch", "duration_ratio", "path")

    def __init__(self, mcd, steps, stretch, duration_ratio, path):
        self.mcd, self.steps, self.stretch, self.duration_ratio, self.path = mcd, steps, stretch, duration_ratio, path


def mcd_dtw(ref_mels, ref_lengths, cand_mels, cand_lengths, coefficients=13, max_abs_mel=4.0, time_major=False, work_budget=WORK_BUDGET):
    """Mel-cepstral distortion of candidates against references (both [B, Mel, T], or [B, T, Mel] with time_major) along the DTW path of their cepstra:
    two `eval_mel_cepstrum` launches and one `eval_dtw` launch (more only beyond `work_budget`)."""
    cx = mel_cepstrum(ref_mels, ref_lengths, coefficients, max_abs_mel, time_major)
    cy = mel_cepstrum(cand_mels, cand_lengths, coefficients, max_abs_mel, time_major)
    B, dev = cx.shape[0], cx.device
    path = dtw(cx, ref_lengths, cy, cand_lengths, work_budget)
    tx, ty = _lengths(ref_lengths, B, dev, torch.float64), _lengths(cand_lengths, B, dev, torch.float64)
    steps = path.steps.double()
    longer = torch.maximum(tx, ty)
    return MCDResult(MCD_FACTOR * path.cost.double() / steps, path.steps, (steps - longer) / longer, ty / tx, path)


def f0_metrics(path, f0_ref, f0_cand):
    """F0 tracks in Hz ([B, Tx], [B, Ty]; 0 = unvoiced; moved to the path's device) compared along a DTW path (a DTWResult or an MCDResult) -> one dict per pair:
    f0_rmse_cents - the RMS of 1200 log2(f_cand / f_ref) over the path steps where both sides are voiced, None when there is no such step;
    vuv_error - the share of path steps whose voicing decisions differ; voiced_steps - the number of both-voiced steps."""
    path = getattr(path, "path", path)
    f0_ref, f0_cand = torch.as_tensor(f0_ref).to(path.ix.device), torch.as_tensor(f0_cand).to(path.ix.device)      # (no kernel of its own: wherever the path is)
    on = path.ix >= 0
    fr = torch.gather(f0_ref.double(), 1, path.ix.clamp(min=0, max=f0_ref.shape[1] - 1).long())
    fc = torch.gather(f0_cand.double(), 1, path.iy.clamp(min=0, max=f0_cand.shape[1] - 1).long())
    vr, vc = (fr > 0) & on, (fc > 0) & on
    both = vr & vc
    one = torch.ones_like(fr)
    cents = 1200.0 * torch.log2(torch.where(both, fc, one) / torch.where(both, fr, one))          # exactly 0 off the both-voiced steps: NaN-free
    n_both = both.sum(1)
    rmse = torch.sqrt((cents * cents).sum(1) / n_both.clamp(min=1).double())
    vuv = (vr != vc).sum(1).double() / on.sum(1).clamp(min=1).double()
    out = []
    for r, v, n in zip(rmse.cpu().tolist(), vuv.cpu().tolist(), n_both.cpu().tolist()):
        out.append({"f0_rmse_cents": r if n else None, "vuv_error": v, "voiced_steps": int(n)})
    return out


def _mel_list(mels, lengths):
    """Padded [B, Mel, T] (+ lengths) or a list of [T, Mel] arrays -> list of float32 host arrays [T, Mel]."""
    if torch.is_tensor(mels):
        host = mels.detach().float().cpu().numpy()
        n = torch.as_tensor(lengths).reshape(-1).cpu().tolist() if lengths is not None else [host.shape[2]] * host.shape[0]
        return [np.ascontiguousarray(host[b, :, :int(n[b])].T) for b in range(host.shape[0])]
    return [np.asarray(m, np.float32) for m in mels]


def speaker_similarity(encoder, ref_mels, ref_lengths, cand_mels, cand_lengths, labels=None, seed=0, slicing=None):
    """Cosine of the two d-vectors of `encoder` (a `speaker_encoder.GE2E`) per pair -> float64 [B] on the device.  Mels: padded [B, Mel, T] with lengths, or
    lists of [T, Mel] arrays (lengths None).  slicing: (Samples, Slice_Length, Overlap_Length) of `data.mels_for_ge2e`, default (the encoder's Samples, 64, 32).
    The slices' random offset is drawn per side from a generator seeded with the first word of `utterance_seed_words(seed, label)`: a run repeats, and an
    utterance against itself is cut the same way on both sides."""
    from .inferencer import utterance_seed_words
    ref, cand = _mel_list(ref_mels, ref_lengths), _mel_list(cand_mels, cand_lengths)
    if len(ref) != len(cand):
        raise ValueError("speaker_similarity: {} references, {} candidates".format(len(ref), len(cand)))
    labels = [str(i) for i in range(len(ref))] if labels is None else list(labels)
    samples, slice_length, overlap = slicing if slicing is not None else (encoder.samples, 64, 32)
    dev = next(encoder.parameters()).device
    vectors = []
    for side in (ref, cand):
        stacks = [data.mels_for_ge2e([m], int(samples), int(slice_length), int(overlap), rng=np.random.RandomState(utterance_seed_words(seed, label)[0]))
                  for m, label in zip(side, labels)]
        x = torch.from_numpy(np.concatenate(stacks).astype(np.float32)).transpose(2, 1).contiguous().to(dev)
        vectors.append(encoder(x, samples=int(samples)).double())
    a, b = vectors
    return (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1)).clamp(min=1e-30)


# ---------------------------------------------------------------------------------------------------------------- the tool
class Evaluator:
    """Evaluator(hp, device)(triples) -> one row (dict) per (label, reference, candidate) triple.  A side is a [T, Mel] array, a `.npy` path holding one, or a
    wav path, which goes through `audio.pattern_from_wav`'s analysis (device_frontend: `frontend.Analyzer`).  Pitch tracks, hence the F0 columns, exist only
    when both sides are wavs and Sound.Frame_Shift is 256; the similarity column only with a speaker encoder.  Columns without a value are None."""

    def __init__(self, hp, device="cuda:0", coefficients=None, speaker_encoder=None, device_frontend=False, seed=0):
        self.hp, self.device = hp, torch.device(device)
        self.settings = evaluation_settings(hp)
        if coefficients is not None:
            self.settings = dict(self.settings, Cepstral_Coefficients=int(coefficients))
        self.coefficients = int(self.settings["Cepstral_Coefficients"])
        self.max_abs, self.mel_dim = float(hp.Sound.Max_Abs_Mel), int(hp.Sound.Mel_Dim)
        self.with_f0 = int(hp.Sound.Frame_Shift) == F0_HOP
        self.speaker_encoder, self.device_frontend, self.seed = speaker_encoder, bool(device_frontend), int(seed)
        self._analyzer = None

    def _wav(self, path):
        """-> (mel [T, Mel], F0 in Hz [T] or None)"""
        from . import audio
        s = self.hp.Sound
        x = audio.audio_prep(path, s.Sample_Rate, 30)
        if self.device_frontend:
            if self._analyzer is None:
                from .frontend import Analyzer
                self._analyzer = Analyzer(self.hp, self.device, with_pitch=self.with_f0)
            mel = self._analyzer([x], with_pitch=False)[0][0]
            hz = None
            if self.with_f0:
                track, frames, _ = self._analyzer.yin(torch.from_numpy(np.ascontiguousarray(x, np.float32))[None])
                hz = track[0, :int(frames[0])].cpu().numpy()
        else:
            mel = audio.pattern_from_audio(x, self.hp)[0]
            hz = audio.yin_pitch(x, s.Sample_Rate, harmo_thresh=1.0 - float(s.Confidence_Threshold)) if self.with_f0 else None
        if hz is not None:                                                    # the track on the mel's frames: cut, or unvoiced beyond its end
            fit = np.zeros(mel.shape[0], np.float32)
            n = min(len(hz), mel.shape[0])
            fit[:n] = hz[:n]
            hz = fit
        return mel, hz

    def load(self, side):
        """-> (mel [T, Mel] float32, F0 in Hz [T] or None)"""
        if isinstance(side, np.ndarray) or torch.is_tensor(side):
            mel, hz = np.asarray(side.detach().cpu() if torch.is_tensor(side) else side, np.float32), None
        elif str(side).lower().endswith(".npy"):
            mel, hz = np.load(side).astype(np.float32), None
        else:
            mel, hz = self._wav(side)
        if mel.ndim != 2 or mel.shape[1] != self.mel_dim or mel.shape[0] < 1:
            raise ValueError("expected a mel [T >= 1, Sound.Mel_Dim = {}], got {}".format(self.mel_dim, list(mel.shape)))
        return np.ascontiguousarray(mel, np.float32), hz

    def _pad(self, arrays, fill, dims):
        n = max(a.shape[0] for a in arrays)
        out = np.full((len(arrays), n) + dims, fill, np.float32)
        for b, a in enumerate(arrays):
            out[b, :a.shape[0]] = a
        return torch.from_numpy(out).to(self.device)

    @torch.no_grad()
    def _batch(self, labels, refs, cands):
        (rm, rf), (cm, cf) = zip(*refs), zip(*cands)
        tx, ty = [m.shape[0] for m in rm], [m.shape[0] for m in cm]
        res = mcd_dtw(self._pad(rm, -self.max_abs, (self.mel_dim,)), tx, self._pad(cm, -self.max_abs, (self.mel_dim,)), ty, self.coefficients, self.max_abs,
                      time_major=True)
        rows = [{"label": label, "ref_frames": a, "cand_frames": b, "f0_rmse_cents": None, "vuv_error": None, "voiced_steps": None, "speaker_cosine": None}
                for label, a, b in zip(labels, tx, ty)]
        for row, m, n, s, d in zip(rows, res.mcd.cpu().tolist(), res.steps.cpu().tolist(), res.stretch.cpu().tolist(), res.duration_ratio.cpu().tolist()):
            row.update(mcd_db=m, steps=int(n), stretch_share=s, duration_ratio=d)
        zero = lambda n: np.zeros(n, np.float32)
        with_f0 = [r is not None and c is not None for r, c in zip(rf, cf)]
        if any(with_f0):                                                      # (a side without a track rides along as unvoiced; its columns stay empty)
            f0 = f0_metrics(res, self._pad([r if r is not None else zero(n) for r, n in zip(rf, tx)], 0.0, ()),
                            self._pad([c if c is not None else zero(n) for c, n in zip(cf, ty)], 0.0, ()))
            for row, has, m in zip(rows, with_f0, f0):
                if has:
                    row.update(m)
        if self.speaker_encoder is not None:
            ge = getattr(getattr(self.hp.Speaker_Embedding, "GE2E", None), "Inference", None)
            slicing = (int(ge.Samples), int(ge.Slice_Length), int(ge.Overlap_Length)) if ge is not None else None
            cos = speaker_similarity(self.speaker_encoder, list(rm), None, list(cm), None, labels, self.seed, slicing)
            for row, c in zip(rows, cos.cpu().tolist()):
                row["speaker_cosine"] = c
        return rows

    def __call__(self, triples):
        triples = list(triples)
        rows = []
        for s in range(0, len(triples), PAIR_BATCH):
            part = triples[s:s + PAIR_BATCH]
            rows += self._batch([str(t[0]) for t in part], [self.load(t[1]) for t in part], [self.load(t[2]) for t in part])
        return rows


def _cell(v):
    return "" if v is None else ("{:.6f}".format(v) if isinstance(v, float) else str(v))


def summarise(rows):
    """column -> {mean, median, count} over the rows that have it (None when none has)."""
    out = {}
    for c in COLUMNS:
        v = np.array([float(r[c]) for r in rows if r.get(c) is not None], np.float64)
        out[c] = {"count": int(v.size), "mean": float(v.mean()) if v.size else None, "median": float(np.median(v)) if v.size else None}
    return out


def write_report(rows, out_dir, settings, extra=None):
    """DIR/evaluation.tsv (one row per utterance) and DIR/evaluation.json (mean, median, count per column, the settings and `extra`); both are functions of
    the rows alone: byte-identical from run to run.  -> the two paths."""
    os.makedirs(out_dir, exist_ok=True)
    tsv, js = os.path.join(out_dir, "evaluation.tsv"), os.path.join(out_dir, "evaluation.json")
    with open(tsv, "w", encoding="utf-8", newline="\n") as f:
        f.write("\t".join(("label",) + COLUMNS) + "\n")
        for r in rows:
            f.write("\t".join([str(r["label"])] + [_cell(r.get(c)) for c in COLUMNS]) + "\n")
    with open(js, "w", encoding="utf-8", newline="\n") as f:
        json.dump(dict({"utterances": len(rows), "settings": settings, "summary": summarise(rows)}, **(extra or {})), f, indent=2, sort_keys=True)
        f.write("\n")
    return tsv, js


def read_pairs_list(path):
    """The --pairs list: one `label<TAB>reference<TAB>candidate` per line; blank lines are skipped.  -> [(label, reference, candidate)]"""
    out = []
    with open(path, "r", encoding="utf-8") as f:
        for i, line in enumerate(f.read().splitlines()):
            if not line.strip():
                continue
            cols = [x.strip() for x in line.split("\t")]
            if len(cols) != 3 or not all(cols):
                raise ValueError("{}:{}: expected label<TAB>reference<TAB>candidate".format(path, i + 1))
            out.append(tuple(cols))
    return out


def eval_patterns(hp, count=None):
    """The first `count` (None: all) patterns of Train.Eval_Pattern in metadata order -> [(label, text, speaker id, mel [T, Mel])]"""
    p = hp.Train.Eval_Pattern
    with open(os.path.join(p.Path, p.Metadata_File).replace("\\", "/"), "rb") as f:
        files = pickle.load(f)["File_List"]
    out = []
    for name in files[:count]:
        with open(os.path.join(p.Path, name).replace("\\", "/"), "rb") as f:
            pat = pickle.load(f)
        out.append((os.path.splitext(os.path.basename(name))[0], pat["Text"], int(pat["Speaker_ID"]), np.asarray(pat["Mel"], np.float32)))
    return out


def build_parser():
    """The command line of Evaluate.py."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("-hp", "--hyper-parameters", default=None, metavar="YAML", help="default: ./Hyper_Parameters.yaml, else the packaged defaults")
    ap.add_argument("-o", "--out", default="./evaluation")
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("--pairs", default=None, metavar="LIST.tsv", help="compare what exists: one label<TAB>reference<TAB>candidate per line (.npy mels [T, Mel] or wavs)")
    what.add_argument("--patterns", nargs="?", type=int, const=-1, default=None, metavar="N",
                      help="synthesise the text of the first N (default: all) patterns of Train.Eval_Pattern with -c and compare with their recorded mels")
    ap.add_argument("-c", "--checkpoint", default=None, help="GlowTTS checkpoint (--patterns)")
    ap.add_argument("--seed", type=int, default=0, help="sampling seed of --patterns and of the speaker encoder's slice offsets")
    ap.add_argument("--speaker-encoder", default=None, metavar="PATH", help="GE2E checkpoint: adds the speaker_cosine column (default: the yaml's "
                                                                            "Speaker_Embedding.GE2E.Checkpoint_Path when it has one)")
    ap.add_argument("--device-frontend", action="store_true", help="analyse wavs on the device instead of the host")
    return ap


def main(argv=None):
    logging.basicConfig(level=logging.INFO)
    args = build_parser().parse_args(argv)
    from . import hparams
    if args.hyper_parameters:
        hparams.set_hp(hparams.load_yaml(args.hyper_parameters))
    hp = hparams.get_hp()
    settings = evaluation_settings(hp)                                        # a bad block fails before anything is loaded
    device = "cuda:0"
    extra = {"seed": args.seed}
    if args.patterns is not None:
        if not args.checkpoint:
            raise ValueError("--patterns needs -c <checkpoint>")
        if hp.Mode.upper() in ("PE", "GR"):
            raise ValueError("Mode {}: --patterns does not choose prosody references or pitch tracks - synthesise with Inference.py and compare the "
                             "results with Evaluate.py --pairs".format(hp.Mode))
        from .inferencer import Inferencer
        pats = eval_patterns(hp, None if args.patterns < 0 else args.patterns)
        inf = Inferencer(checkpoint_path=args.checkpoint, hp=hp, device=device, device_frontend=args.device_frontend)
        labels = [p[0] for p in pats]
        files = inf.Inference(labels, [p[1] for p in pats], [1.0] * len(pats), [p[2] for p in pats] if hp.Mode.upper() == "SE" else None, None, args.out,
                              seed=args.seed, speaker_references=[p[3] for p in pats] if inf.ge2e_mode else None)
        triples = [(label, p[3], f) for label, p, f in zip(labels, pats, files)]
        extra["checkpoint"] = os.path.basename(args.checkpoint)
    else:
        triples = read_pairs_list(args.pairs)
    encoder = None
    path = args.speaker_encoder or getattr(getattr(getattr(hp, "Speaker_Embedding", None), "GE2E", None), "Checkpoint_Path", None)
    if path:
        from .speaker_encoder import GE2E
        encoder = GE2E.from_checkpoint(hp, device, path)
    rows = Evaluator(hp, device, speaker_encoder=encoder, device_frontend=args.device_frontend, seed=args.seed)(triples)
    print("\n".join(write_report(rows, args.out, settings, extra)))
