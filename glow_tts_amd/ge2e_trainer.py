"""Trainer of the GE2E speaker encoder (DESIGN.md "Training the GE2E speaker encoder"): `python Train_GE2E.py -hp <yaml> -s <steps>`.

Reads the pattern directories `Pattern_Generator.py` writes (through METADATA.PICKLE: `File_List_by_Speaker_Dict`, `Mel_Length_Dict`), draws seeded
speaker-major batches of mel slices, and steps `speaker_encoder.GE2E(trainable=True)` under `speaker_encoder.GE2ELoss` with the project's clipping and RAdam
kernels (`optim`).  The checkpoints `GE2E_<steps>.pt` load unchanged through `GE2E.from_checkpoint` / `Speaker_Embedding.GE2E.Checkpoint_Path`."""
import logging

import numpy as np
import torch

from . import aux_trainer, optim
from .hparams import get_hp, overlay_settings
from .speaker_encoder import GE2E, GE2ELoss, ge2e_load

TRAIN_KEY = "Speaker_Embedding.GE2E.Train"
DEFAULTS = {"Speakers": 64, "Utterances": 10, "Slice_Length": {"Min": 140, "Max": 180}, "Learning_Rate": 1.0e-3, "Gradient_Norm": 3.0,
            "Projection_Grad_Scale": 0.5, "Similarity_Grad_Scale": 0.01, "Max_Step": 1000000, "Checkpoint_Save_Interval": 5000, "Evaluation_Interval": 1000,
            "Checkpoint_Path": "./ge2e_results"}


def train_settings(hp):
    """The optional yaml block `Speaker_Embedding.GE2E.Train` over DEFAULTS (`hparams.overlay_settings`), checked: a ValueError names every bad key."""
    def rules(s, need):
        need("Speakers", lambda v: int(v) >= 2, "at least 2")
        need("Utterances", lambda v: int(v) >= 2, "at least 2")
        need("Slice_Length", lambda v: 1 <= int(v["Min"]) <= int(v["Max"]), "1 <= Min <= Max")
        for k in ("Learning_Rate", "Gradient_Norm", "Projection_Grad_Scale", "Similarity_Grad_Scale"):
            need(k, lambda v: float(v) > 0, "positive")
    return overlay_settings(getattr(hp.Speaker_Embedding.GE2E, "Train", None), DEFAULTS, TRAIN_KEY, "GE2E", rules)


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


class Sampler(aux_trainer.PatternSampler):
    """Speaker-major batches of mel slices from one pattern directory.  Batch `step` is a function of (seed, step) alone: one slice length T from [Min, Max],
    S speakers among those with at least M utterances of at least T frames, M of those utterances each, a random offset per utterance."""

    def __init__(self, pattern_path, metadata_file, speakers, utterances, slice_min, slice_max, seed=0, cache=True):
        super().__init__(pattern_path, metadata_file, seed, cache)
        self.S, self.M, self.lo, self.hi = int(speakers), int(utterances), int(slice_min), int(slice_max)
        self.lengths = self.meta["Mel_Length_Dict"]
        self.by_speaker = {spk: sorted(files) for spk, files in sorted(self.meta["File_List_by_Speaker_Dict"].items())}
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
        rng = self.rng(step)
        T = int(rng.integers(self.lo, self.hi + 1))
        pool = self.eligible(T)
        names = sorted(pool)
        rows = []
        for si in rng.choice(len(names), self.S, replace=False):
            files = pool[names[si]]
            for fi in rng.choice(len(files), self.M, replace=False):
                rows.append((names[si], files[fi], int(rng.integers(0, self.lengths[files[fi]] - T + 1))))
        return T, rows

    def read(self, p):
        return np.asarray(p["Mel"], np.float32)

    def batch(self, step):
        """-> float32 tensor [S M, Mel, T] (host)"""
        T, rows = self.plan(step)
        return torch.from_numpy(np.stack([self.pattern(f)[o:o + T].T for _, f, o in rows]).astype(np.float32))


class GE2E_Trainer(aux_trainer.Trainer):
    PREFIX = "GE2E"

    def __init__(self, steps=0, hp=None, device="cuda:0", seed=0):
        hp = hp if hp is not None else get_hp()
        s = train_settings(hp)
        super().__init__(hp, s, steps, device, seed, Sampler, (s["Speakers"], s["Utterances"], s["Slice_Length"]["Min"], s["Slice_Length"]["Max"]))
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(self.seed)
            self.model = GE2E(self.hp, self.device, trainable=True)
        self.criterion = GE2ELoss().to(self.device)
        self.params = list(self.model.parameters()) + [self.criterion.w]
        self.optimizer = optim.RAdam(self.params, lr=float(s["Learning_Rate"]))
        if self.steps > 0:
            self.Load_Checkpoint()

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

    def state_dict(self):
        return {"Model": {k: v.detach().cpu() for k, v in self.model.state_dict().items()}, "Loss": {"w": self.criterion.w.detach().cpu()},
                "Optimizer": self.optimizer.state_dict(), "Steps": self.steps}

    def load_state_dict(self, state):
        with torch.no_grad():
            for k, v in ge2e_load(state, self.model.sizes).items():
                dict(self.model.named_parameters())[k].copy_(v)
            self.criterion.w.copy_(state["Loss"]["w"])
        self.model.invalidate_images()
        self.optimizer.load_state_dict(state["Optimizer"])
        self.steps = int(state["Steps"])

    def log_evaluation(self, loss, ev):
        logging.info("Step %d: loss %.4f%s", self.steps, float(loss), "" if ev is None else ", evaluation loss {:.4f}, EER {:.4f}".format(*ev))


def main(argv=None):
    aux_trainer.main("train the GE2E speaker encoder on the pattern directories of Train.Train_Pattern / Train.Eval_Pattern", GE2E_Trainer, argv)
