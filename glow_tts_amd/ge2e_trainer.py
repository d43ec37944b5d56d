"""Trainer of the GE2E speaker encoder (DESIGN.md "Training the GE2E speaker encoder"): `python Train_GE2E.py -hp <yaml> -s <steps>`.

Reads the pattern directories `Pattern_Generator.py` writes (through METADATA.PICKLE: `File_List_by_Speaker_Dict`, `Mel_Length_Dict`), draws seeded
speaker-major batches of mel slices, and steps `speaker_encoder.GE2E(trainable=True)` under `speaker_encoder.GE2ELoss` with the project's clipping and RAdam
kernels (`optim`).  The checkpoints `GE2E_<steps>.pt` load unchanged through `GE2E.from_checkpoint` / `Speaker_Embedding.GE2E.Checkpoint_Path`."""
import argparse
import logging
import os
import pickle

import numpy as np
import torch

from . import optim
from .hparams import Recursive_Parse, get_hp, load_yaml
from .speaker_encoder import GE2E, GE2ELoss

TRAIN_KEY = "Speaker_Embedding.GE2E.Train"
DEFAULTS = {"Speakers": 64, "Utterances": 10, "Slice_Length": {"Min": 140, "Max": 180}, "Learning_Rate": 1.0e-3, "Gradient_Norm": 3.0,
            "Projection_Grad_Scale": 0.5, "Similarity_Grad_Scale": 0.01, "Max_Step": 1000000, "Checkpoint_Save_Interval": 5000, "Evaluation_Interval": 1000,
            "Checkpoint_Path": "./ge2e_results"}


def _plain(v):
    return {k: _plain(x) for k, x in vars(v).items()} if isinstance(v, argparse.Namespace) else v


def train_settings(hp):
    """The optional yaml block `Speaker_Embedding.GE2E.Train` over DEFAULTS (absent block or key: the default), checked: a ValueError names every bad key."""
    given = _plain(getattr(hp.Speaker_Embedding.GE2E, "Train", None)) or {}
    unknown = sorted(set(given) - set(DEFAULTS))
    if unknown:
        raise ValueError("unknown key {}.{} (known: {})".format(TRAIN_KEY, unknown[0], ", ".join(DEFAULTS)))
    s = dict(DEFAULTS, **given)
    s["Slice_Length"] = dict(DEFAULTS["Slice_Length"], **(given.get("Slice_Length") or {}))
    bad = []
    if int(s["Speakers"]) < 2:
        bad.append("{}.Speakers = {} (at least 2)".format(TRAIN_KEY, s["Speakers"]))
    if int(s["Utterances"]) < 2:
        bad.append("{}.Utterances = {} (at least 2)".format(TRAIN_KEY, s["Utterances"]))
    lo, hi = int(s["Slice_Length"]["Min"]), int(s["Slice_Length"]["Max"])
    if lo < 1 or hi < lo:
        bad.append("{}.Slice_Length = {{Min: {}, Max: {}}} (1 <= Min <= Max)".format(TRAIN_KEY, lo, hi))
    for k in ("Learning_Rate", "Gradient_Norm", "Projection_Grad_Scale", "Similarity_Grad_Scale"):
        if not float(s[k]) > 0:
            bad.append("{}.{} = {} (positive)".format(TRAIN_KEY, k, s[k]))
    if bad:
        raise ValueError("the GE2E trainer does not support " + "; ".join(bad))
    return s


def equal_error_rate(scores, labels):
    """The equal error rate of a trial list on the host: `scores` (higher: more likely the same speaker), `labels` (True: a target trial).  The threshold runs
    over the scores; the rate is (FAR + FRR) / 2 at the threshold where the two are closest."""
    scores, labels = np.asarray(scores, np.float64).reshape(-1), np.asarray(labels, bool).reshape(-1)
    if scores.size == 0 or labels.all() or not labels.any():
        raise ValueError("the equal error rate needs target and non-target trials")
    best = None
    for th in np.concatenate([np.unique(scores), [scores.max() + 1.0]]):
        accept = scores >= th
        far, frr = (accept & ~labels).sum() / (~labels).sum(), (~accept & labels).sum() / labels.sum()
        if best is None or abs(far - frr) < best[0]:
            best = (abs(far - frr), (far + frr) / 2)
    return float(best[1])


class Sampler:
    """Speaker-major batches of mel slices from one pattern directory.  Batch `step` is a function of (seed, step) alone: one slice length T from [Min, Max],
    S speakers among those with at least M utterances of at least T frames, M of those utterances each, a random offset per utterance."""

    def __init__(self, pattern_path, metadata_file, speakers, utterances, slice_min, slice_max, seed=0, cache=True):
        self.path, self.S, self.M, self.lo, self.hi, self.seed = pattern_path, int(speakers), int(utterances), int(slice_min), int(slice_max), int(seed)
        with open(os.path.join(pattern_path, metadata_file.upper()), "rb") as f:
            meta = pickle.load(f)
        self.lengths = meta["Mel_Length_Dict"]
        self.by_speaker = {spk: sorted(files) for spk, files in sorted(meta["File_List_by_Speaker_Dict"].items())}
        self._cache = {} if cache else None
        if len(self.eligible(self.hi)) < self.S:
            raise ValueError("{}: {} speakers have {} utterances of {} frames ({}.Slice_Length.Max), {}.Speakers = {} are needed".format(
                pattern_path, len(self.eligible(self.hi)), self.M, self.hi, TRAIN_KEY, TRAIN_KEY, self.S))

    def eligible(self, T):
        """speaker -> its files of at least T frames, for the speakers that have at least M of them"""
        out = {}
        for spk, files in self.by_speaker.items():
            long = [f for f in files if self.lengths[f] >= T]
            if len(long) >= self.M:
                out[spk] = long
        return out

    def plan(self, step):
        """-> (T, [(speaker, file, offset)] * S M) of batch `step`"""
        rng = np.random.default_rng([self.seed, int(step)])
        T = int(rng.integers(self.lo, self.hi + 1))
        pool = self.eligible(T)
        names = sorted(pool)
        rows = []
        for si in rng.choice(len(names), self.S, replace=False):
            files = pool[names[si]]
            for fi in rng.choice(len(files), self.M, replace=False):
                rows.append((names[si], files[fi], int(rng.integers(0, self.lengths[files[fi]] - T + 1))))
        return T, rows

    def mel(self, file):
        if self._cache is not None and file in self._cache:
            return self._cache[file]
        with open(os.path.join(self.path, file), "rb") as f:
            m = np.asarray(pickle.load(f)["Mel"], np.float32)
        if self._cache is not None:
            self._cache[file] = m
        return m

    def batch(self, step):
        """-> float32 tensor [S M, Mel, T] (host)"""
        T, rows = self.plan(step)
        return torch.from_numpy(np.stack([self.mel(f)[o:o + T].T for _, f, o in rows]).astype(np.float32))


class GE2E_Trainer:
    def __init__(self, steps=0, hp=None, device="cuda:0", seed=0):
        self.hp = hp if hp is not None else get_hp()
        self.set = train_settings(self.hp)
        self.device, self.steps, self.seed = torch.device(device), int(steps), int(seed)
        s, tp, ep = self.set, self.hp.Train.Train_Pattern, self.hp.Train.Eval_Pattern
        cache = bool(getattr(self.hp.Train, "Use_Pattern_Cache", True))
        args = (s["Speakers"], s["Utterances"], s["Slice_Length"]["Min"], s["Slice_Length"]["Max"])
        self.sampler = {"Train": Sampler(tp.Path, tp.Metadata_File, *args, seed=self.seed, cache=cache)}
        if ep.Path and os.path.exists(os.path.join(ep.Path, ep.Metadata_File.upper())):
            try:
                self.sampler["Eval"] = Sampler(ep.Path, ep.Metadata_File, *args, seed=self.seed + 1, cache=cache)
            except ValueError as err:
                logging.warning("no evaluation: %s", err)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(self.seed)
            self.model = GE2E(self.hp, self.device, trainable=True)
        self.criterion = GE2ELoss().to(self.device)
        self.params = list(self.model.parameters()) + [self.criterion.w]
        self.optimizer = optim.RAdam(self.params, lr=float(s["Learning_Rate"]))
        self.last = {}
        if self.steps > 0:
            self.Load_Checkpoint()

    def checkpoint_file(self, steps):
        return os.path.join(self.set["Checkpoint_Path"], "GE2E_{}.pt".format(steps))

    def Train_Step(self, stack):
        """One step on a host or device batch [S M, Mel, T]; returns the loss (0-d device tensor)."""
        s = self.set
        loss = self.criterion(self.model.embed(stack.to(self.device, non_blocking=True)), s["Speakers"], s["Utterances"])
        for p in self.params:
            p.grad = None
        loss.backward()
        self.model.linear.weight.grad.mul_(float(s["Projection_Grad_Scale"]))             # the paper's gradient scales (Wan et al. 2018, section 3.1)
        self.model.linear.bias.grad.mul_(float(s["Projection_Grad_Scale"]))
        self.criterion.w.grad.mul_(float(s["Similarity_Grad_Scale"]))
        norm = optim.clip_grad_norm_(self.params, float(s["Gradient_Norm"]), _table_key=("ge2e", id(self)))
        self.optimizer.step()
        self.model.invalidate_images()                                                     # (the update kernel writes the parameters through raw pointers)
        with torch.no_grad():
            self.criterion.w.clamp_(min=1e-6)
        self.steps += 1
        self.last = {"Loss": loss.detach(), "Gradient_Norm": norm}
        return loss.detach()

    @torch.no_grad()
    def Evaluation(self, batches=4):
        """-> (mean loss, equal error rate) over `batches` batches of the evaluation set: the d-vector of every slice against every speaker centroid of its
        batch (its own speaker's without itself), the cosine scores pooled on the host."""
        if "Eval" not in self.sampler:
            return None
        S, M = self.set["Speakers"], self.set["Utterances"]
        losses, scores, labels = [], [], []
        for b in range(batches):
            e = self.model.embed(self.sampler["Eval"].batch(b).to(self.device))
            losses.append(float(self.criterion(e, S, M)))
            u = torch.nn.functional.normalize(e.double().cpu(), dim=1)
            U = u.reshape(S, M, -1)
            sums = U.sum(1)
            cent, excl = sums / M, (sums[:, None, :] - U) / (M - 1)
            cos = (u @ cent.t()) / cent.norm(dim=1).clamp_min(1e-12)[None, :]
            own = torch.arange(S * M) // M
            target = torch.zeros(S * M, S, dtype=torch.bool)
            target[torch.arange(S * M), own] = True
            cos[target] = ((U * excl).sum(-1) / excl.norm(dim=-1).clamp_min(1e-12)).reshape(-1)
            scores.append(cos.reshape(-1).numpy())
            labels.append(target.reshape(-1).numpy())
        scores, labels = np.concatenate(scores), np.concatenate(labels)
        return float(np.mean(losses)), equal_error_rate(scores, labels)

    def Save_Checkpoint(self):
        os.makedirs(self.set["Checkpoint_Path"], exist_ok=True)
        state = {"Model": {k: v.detach().cpu() for k, v in self.model.state_dict().items()}, "Loss": {"w": self.criterion.w.detach().cpu()},
                 "Optimizer": self.optimizer.state_dict(), "Steps": self.steps}
        torch.save(state, self.checkpoint_file(self.steps))
        logging.info("Checkpoint saved at %d steps.", self.steps)
        return self.checkpoint_file(self.steps)

    def Load_Checkpoint(self):
        state = torch.load(self.checkpoint_file(self.steps), map_location="cpu")
        from .speaker_encoder import ge2e_load
        with torch.no_grad():
            for k, v in ge2e_load(state, self.model.sizes).items():
                dict(self.model.named_parameters())[k].copy_(v)
            self.criterion.w.copy_(state["Loss"]["w"])
        self.model.invalidate_images()
        self.optimizer.load_state_dict(state["Optimizer"])
        self.steps = int(state["Steps"])

    def Train(self):
        s = self.set
        while self.steps < int(s["Max_Step"]):
            loss = self.Train_Step(self.sampler["Train"].batch(self.steps))
            if self.steps % int(s["Evaluation_Interval"]) == 0:
                ev = self.Evaluation()
                logging.info("Step %d: loss %.4f%s", self.steps, float(loss), "" if ev is None else ", evaluation loss {:.4f}, EER {:.4f}".format(*ev))
            if self.steps % int(s["Checkpoint_Save_Interval"]) == 0:
                self.Save_Checkpoint()
        if not os.path.exists(self.checkpoint_file(self.steps)):
            self.Save_Checkpoint()


def main(argv=None):
    ap = argparse.ArgumentParser(description="train the GE2E speaker encoder on the pattern directories of Train.Train_Pattern / Train.Eval_Pattern")
    ap.add_argument("-hp", "--hyper_parameters", default=None, help="yaml to read instead of ./Hyper_Parameters.yaml")
    ap.add_argument("-s", "--steps", default=0, type=int, help="resume from GE2E_<steps>.pt")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    hp = Recursive_Parse(load_yaml(args.hyper_parameters)) if args.hyper_parameters else get_hp()
    GE2E_Trainer(steps=args.steps, hp=hp, device=args.device, seed=args.seed).Train()
