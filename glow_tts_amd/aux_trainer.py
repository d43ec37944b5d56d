"""What the trainers of the side models share (`ge2e_trainer.GE2E_Trainer`, `pwg_trainer.PWG_Trainer`): the seeded sampler over a pattern directory, the
constructor head, the checkpoint files, the `Train` loop and the command line.  A trainer subclasses `Trainer`, sets `PREFIX` and supplies `Train_Step`,
`Evaluation` and three hooks: `state_dict`, `load_state_dict`, `log_evaluation`.  Their settings are `hparams.overlay_settings` under their own rules."""
import argparse
import logging
import os
import pickle

import numpy as np
import torch

from .hparams import Recursive_Parse, get_hp, load_yaml


class PatternSampler:
    """One pattern directory of `Pattern_Generator.py` behind its metadata file.  A subclass draws batch `step` from `rng(step)`, a function of (seed, step)
    alone, and says with `read` what it keeps of a pattern file; `pattern` caches that unless `cache` is off."""

    def __init__(self, pattern_path, metadata_file, seed=0, cache=True):
        self.path, self.seed = pattern_path, int(seed)
        with open(os.path.join(pattern_path, metadata_file.upper()), "rb") as f:
            self.meta = pickle.load(f)
        self._cache = {} if cache else None

    def rng(self, step):
        return np.random.default_rng([self.seed, int(step)])

    def pattern(self, file):
        if self._cache is not None and file in self._cache:
            return self._cache[file]
        with open(os.path.join(self.path, file), "rb") as f:
            p = self.read(pickle.load(f))
        if self._cache is not None:
            self._cache[file] = p
        return p


class Trainer:
    PREFIX = None                                                   # the checkpoints are <Checkpoint_Path>/<PREFIX>_<steps>.pt

    def __init__(self, hp, settings, steps, device, seed, sampler, sampler_args):
        """The head of a constructor: the subclass resolves its settings, builds its model after this and ends with `Load_Checkpoint` when steps > 0."""
        self.hp, self.set = hp, settings
        self.device, self.steps, self.seed = torch.device(device), int(steps), int(seed)
        tp, ep = self.hp.Train.Train_Pattern, self.hp.Train.Eval_Pattern
        cache = bool(getattr(self.hp.Train, "Use_Pattern_Cache", True))
        self.sampler = {"Train": sampler(tp.Path, tp.Metadata_File, *sampler_args, seed=self.seed, cache=cache)}
        if ep.Path and os.path.exists(os.path.join(ep.Path, ep.Metadata_File.upper())):
            try:
                self.sampler["Eval"] = sampler(ep.Path, ep.Metadata_File, *sampler_args, seed=self.seed + 1, cache=cache)
            except ValueError as err:
                logging.warning("no evaluation: %s", err)
        self.last = {}

    def checkpoint_file(self, steps):
        return os.path.join(self.set["Checkpoint_Path"], "{}_{}.pt".format(self.PREFIX, steps))

    def Save_Checkpoint(self):
        os.makedirs(self.set["Checkpoint_Path"], exist_ok=True)
        torch.save(self.state_dict(), self.checkpoint_file(self.steps))
        logging.info("Checkpoint saved at %d steps.", self.steps)
        return self.checkpoint_file(self.steps)

    def Load_Checkpoint(self):
        self.load_state_dict(torch.load(self.checkpoint_file(self.steps), map_location="cpu"))

    def Train(self):
        s = self.set
        while self.steps < int(s["Max_Step"]):
            batch = self.sampler["Train"].batch(self.steps)
            loss = self.Train_Step(*(batch if isinstance(batch, tuple) else (batch,)))
            if self.steps % int(s["Evaluation_Interval"]) == 0:
                self.log_evaluation(loss, self.Evaluation())
            if self.steps % int(s["Checkpoint_Save_Interval"]) == 0:
                self.Save_Checkpoint()
        if not os.path.exists(self.checkpoint_file(self.steps)):
            self.Save_Checkpoint()


def main(description, trainer, argv=None):
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("-hp", "--hyper_parameters", default=None, help="yaml to read instead of ./Hyper_Parameters.yaml")
    ap.add_argument("-s", "--steps", default=0, type=int, help="resume from {}_<steps>.pt".format(trainer.PREFIX))
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    hp = Recursive_Parse(load_yaml(args.hyper_parameters)) if args.hyper_parameters else get_hp()
    trainer(steps=args.steps, hp=hp, device=args.device, seed=args.seed).Train()
