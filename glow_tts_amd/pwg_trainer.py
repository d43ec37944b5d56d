"""Trainer of the Parallel WaveGAN vocoder - `python Train_PWG.py -hp <yaml> -s <steps>`.  Stage one of its recipe (DESIGN.md "Training the Parallel WaveGAN
generator"): the generator alone under the multi-resolution STFT loss.  With the optional yaml block `Vocoder.Train.Discriminator`, stage two from its
`Start_Step` on (DESIGN.md "Training the Parallel WaveGAN discriminator"): the least-squares adversarial term joins the generator's loss and the
discriminator `vocoder.PWGDiscriminator` is trained beside it, with a clipping and a RAdam of its own.

Reads the pattern directories `Pattern_Generator.py` writes (through METADATA.PICKLE: `File_List`, `Mel_Length_Dict`, `Audio_Length_Dict`): every pattern
holds the raw `Audio` beside its `Mel`, frame f centred on sample f * Frame_Shift.  Draws seeded batches of mel segments with the audio under them, and steps
`vocoder.ParallelWaveGAN(trainable=True)` under `vocoder.MultiResolutionSTFTLoss` with the project's clipping and RAdam kernels (`optim`).  The checkpoints
`PWG_<steps>.pt` load unchanged through `Vocoder.Checkpoint_Path`.  The defaults of the optional yaml block `Vocoder.Train` restate the original recipe from
memory: they are this project's contract, not a pinned one."""
import argparse
import hashlib
import logging
import os
import pickle

import numpy as np
import torch

from . import optim
from .hparams import Recursive_Parse, get_hp, load_yaml
from .vocoder import (STFT_RESOLUTIONS, MultiResolutionSTFTLoss, ParallelWaveGAN, PWGDiscriminator, adversarial_mse, pwg_disc_load, pwg_disc_settings, pwg_geometry,
                      pwg_load, plain_block, stft_loss_geometry)

TRAIN_KEY = "Vocoder.Train"
DEFAULTS = {"Batch_Size": 8, "Segment_Frames": 100, "Learning_Rate": 1.0e-4, "Epsilon": 1.0e-6, "Gradient_Norm": 10.0,
            "Learning_Rate_Decay": {"Step": 200000, "Gamma": 0.5}, "STFT_Resolutions": [list(r) for r in STFT_RESOLUTIONS], "Max_Step": 100000,
            "Checkpoint_Save_Interval": 5000, "Evaluation_Interval": 1000, "Checkpoint_Path": "./pwg_results"}


def train_settings(hp):
    """The optional yaml block `Vocoder.Train` over DEFAULTS (absent block or key: the default), checked: a ValueError names every bad key.  The optional
    sub-block `Discriminator` (`vocoder.pwg_disc_settings`) appears in the result only when the yaml has it."""
    given = plain_block(getattr(getattr(hp, "Vocoder", None), "Train", None)) or {}
    unknown = sorted(set(given) - set(DEFAULTS) - {"Discriminator"})
    if unknown:
        raise ValueError("unknown key {}.{} (known: {})".format(TRAIN_KEY, unknown[0], ", ".join(DEFAULTS)))
    s = dict(DEFAULTS, **given)
    s["Learning_Rate_Decay"] = dict(DEFAULTS["Learning_Rate_Decay"], **(given.get("Learning_Rate_Decay") or {}))
    bad = []
    for k in ("Batch_Size", "Segment_Frames", "Max_Step", "Checkpoint_Save_Interval", "Evaluation_Interval"):
        if int(s[k]) < 1:
            bad.append("{}.{} = {} (at least 1)".format(TRAIN_KEY, k, s[k]))
    for k in ("Learning_Rate", "Epsilon", "Gradient_Norm"):
        if not float(s[k]) > 0:
            bad.append("{}.{} = {} (positive)".format(TRAIN_KEY, k, s[k]))
    d = s["Learning_Rate_Decay"]
    if int(d["Step"]) < 1 or not 0 < float(d["Gamma"]) <= 1:
        bad.append("{}.Learning_Rate_Decay = {{Step: {}, Gamma: {}}} (Step >= 1, 0 < Gamma <= 1)".format(TRAIN_KEY, d["Step"], d["Gamma"]))
    if bad:
        raise ValueError("the vocoder trainer does not support " + "; ".join(bad))
    s["STFT_Resolutions"] = stft_loss_geometry(s["STFT_Resolutions"], int(s["Segment_Frames"]) * int(hp.Sound.Frame_Shift))
    if "Discriminator" in given:
        s["Discriminator"] = pwg_disc_settings(hp)
    return s


def noise_seed_words(seed, step, index):
    """The two 32-bit seed words of the noise of batch row `index` at step `step` of the run `seed`: the first 8 bytes of blake2b of
    "<seed> NUL <step> NUL <index> NUL pwgtrain", little endian; z is drawn from them in `pwg_first`, so a run repeats and no z tensor exists."""
    d = hashlib.blake2b("{}\0{}\0{}\0pwgtrain".format(seed, step, index).encode()).digest()
    return int.from_bytes(d[:4], "little"), int.from_bytes(d[4:8], "little")


class Sampler:
    """Batches of (mel segment, the audio under it) from one pattern directory.  Batch `step` is a function of (seed, step) alone: `batch` files among those
    whose mel has at least `frames` frames and whose audio at least `frames * hop` samples, and for each a start frame f0 with
    (f0 + frames) * hop <= its audio length.  The target is the pattern's raw audio - final audio, without pre-emphasis or de-emphasis."""

    def __init__(self, pattern_path, metadata_file, batch, frames, hop, seed=0, cache=True):
        self.path, self.B, self.frames, self.hop, self.seed = pattern_path, int(batch), int(frames), int(hop), int(seed)
        with open(os.path.join(pattern_path, metadata_file.upper()), "rb") as f:
            meta = pickle.load(f)
        mel, audio = meta["Mel_Length_Dict"], meta["Audio_Length_Dict"]
        self.starts = {f: min(mel[f], audio[f] // self.hop) - self.frames for f in sorted(meta["File_List"])}          # the largest f0 of a file
        self.files = [f for f, n in self.starts.items() if n >= 0]
        self._cache = {} if cache else None
        if not self.files:
            raise ValueError("{}: no pattern has {} frames with {} samples of audio under them ({}.Segment_Frames)".format(
                pattern_path, self.frames, self.frames * self.hop, TRAIN_KEY))

    def plan(self, step):
        """-> [(file, f0)] * batch of batch `step`"""
        rng = np.random.default_rng([self.seed, int(step)])
        rows = []
        for _ in range(self.B):
            f = self.files[int(rng.integers(0, len(self.files)))]
            rows.append((f, int(rng.integers(0, self.starts[f] + 1))))
        return rows

    def pattern(self, file):
        if self._cache is not None and file in self._cache:
            return self._cache[file]
        with open(os.path.join(self.path, file), "rb") as f:
            p = pickle.load(f)
        p = (np.asarray(p["Mel"], np.float32), np.asarray(p["Audio"], np.float32))
        if self._cache is not None:
            self._cache[file] = p
        return p

    def batch(self, step):
        """-> (mel [B, Mel, frames], target [B, frames * hop]) float32 host tensors"""
        mels, wavs = [], []
        for f, f0 in self.plan(step):
            mel, audio = self.pattern(f)
            mels.append(mel[f0:f0 + self.frames].T)
            wavs.append(audio[f0 * self.hop:(f0 + self.frames) * self.hop])
        return torch.from_numpy(np.stack(mels).astype(np.float32)), torch.from_numpy(np.stack(wavs).astype(np.float32))


class PWG_Trainer:
    def __init__(self, steps=0, hp=None, device="cuda:0", seed=0):
        self.hp = hp if hp is not None else get_hp()
        self.geo = pwg_geometry(self.hp)
        self.set = train_settings(self.hp)
        self.device, self.steps, self.seed = torch.device(device), int(steps), int(seed)
        s, tp, ep = self.set, self.hp.Train.Train_Pattern, self.hp.Train.Eval_Pattern
        cache = bool(getattr(self.hp.Train, "Use_Pattern_Cache", True))
        args = (s["Batch_Size"], s["Segment_Frames"], self.geo["hop"])
        self.sampler = {"Train": Sampler(tp.Path, tp.Metadata_File, *args, seed=self.seed, cache=cache)}
        if ep.Path and os.path.exists(os.path.join(ep.Path, ep.Metadata_File.upper())):
            try:
                self.sampler["Eval"] = Sampler(ep.Path, ep.Metadata_File, *args, seed=self.seed + 1, cache=cache)
            except ValueError as err:
                logging.warning("no evaluation: %s", err)
        self.model = ParallelWaveGAN(self.hp, self.device, trainable=True, seed=self.seed)
        self.criterion = MultiResolutionSTFTLoss(s["STFT_Resolutions"], self.device)
        self.params = list(self.model.params.values())
        self.optimizer = optim.RAdam(self.params, lr=float(s["Learning_Rate"]), eps=float(s["Epsilon"]))
        # stage two (optional block Vocoder.Train.Discriminator): initialised from the seed at construction, untouched before Start_Step
        self.disc_set, self.discriminator, self.disc_steps = s.get("Discriminator"), None, 0
        if self.disc_set is not None:
            self.discriminator = PWGDiscriminator(self.hp, self.device, trainable=True, seed=self.seed)
            self.disc_params = list(self.discriminator.params.values())
            self.disc_optimizer = optim.RAdam(self.disc_params, lr=float(self.disc_set["Learning_Rate"]), eps=float(self.disc_set["Epsilon"]))
        self.last = {}
        if self.steps > 0:
            self.Load_Checkpoint()

    def checkpoint_file(self, steps):
        return os.path.join(self.set["Checkpoint_Path"], "PWG_{}.pt".format(steps))

    def learning_rate(self, step):
        """The host-side step decay: Learning_Rate * Gamma^(step // Step)"""
        d = self.set["Learning_Rate_Decay"]
        return float(self.set["Learning_Rate"]) * float(d["Gamma"]) ** (int(step) // int(d["Step"]))

    def seeds(self, step, B):
        return torch.tensor([noise_seed_words(self.seed, step, i) for i in range(B)], dtype=torch.int64)

    def disc_learning_rate(self, updates):
        """The discriminator's step decay counts its own updates: Learning_Rate * Gamma^(updates // Step)"""
        d = self.disc_set["Learning_Rate_Decay"]
        return float(self.disc_set["Learning_Rate"]) * float(d["Gamma"]) ** (int(updates) // int(d["Step"]))

    def adversarial(self, step):
        return self.disc_set is not None and int(step) >= int(self.disc_set["Start_Step"])

    def forward(self, mel, target, step, adversarial=False):
        """-> L_stft, or with `adversarial` (L_G = L_stft + Lambda_Adversarial L_adv, L_D, the unscaled (L_adv, real term, fake term) [3]): one discriminator
        forward over [target; wav]; L_G's backward reaches the generator alone, L_D's the discriminator alone."""
        mel, target = mel.to(self.device, non_blocking=True), target.to(self.device, non_blocking=True)
        B, _, L = mel.shape
        wav, _ = self.model.generate(mel, [L] * B, seeds=self.seeds(step, B))
        stft = self.criterion(wav, target)
        if not adversarial:
            return stft
        both, p_fake = self.discriminator.score_pair(target, wav)
        adv, adv_terms = adversarial_mse(p_fake, 1.0, float(self.disc_set["Lambda_Adversarial"]))
        d_loss, d_terms = adversarial_mse(both, (1.0, 0.0))
        return stft + adv, d_loss, torch.cat([adv_terms[:1], d_terms]), stft

    def Train_Step(self, mel, target):
        """One step on a host or device batch (mel [B, Mel, frames], target [B, frames * hop]); returns the generator's loss (0-d device tensor)."""
        if self.adversarial(self.steps):
            return self.Adversarial_Step(mel, target)
        loss = self.forward(mel, target, self.steps)
        for p in self.params:
            p.grad = None
        loss.backward()
        norm = optim.clip_grad_norm_(self.params, float(self.set["Gradient_Norm"]), _table_key=("pwg", id(self)))
        for group in self.optimizer.param_groups:
            group["lr"] = self.learning_rate(self.steps)
        self.optimizer.step()                                                              # (the next `generate` rebuilds the weight images from the parameters)
        self.steps += 1
        self.last = {"Loss": loss.detach(), "Terms": self.criterion.terms, "Gradient_Norm": norm}
        return loss.detach()

    def Adversarial_Step(self, mel, target):
        """A step of stage two: both updates are computed from the state before the step (the discriminator's forward and both backwards precede both updates)."""
        loss, d_loss, adv_terms, stft = self.forward(mel, target, self.steps, adversarial=True)
        for p in self.params + self.disc_params:
            p.grad = None
        loss.backward()                                                                    # the generator alone: the fake rows' data chain, no weight gradients
        d_loss.backward()                                                                  # the discriminator alone
        norm = optim.clip_grad_norm_(self.params, float(self.set["Gradient_Norm"]), _table_key=("pwg", id(self)))
        d_norm = optim.clip_grad_norm_(self.disc_params, float(self.disc_set["Gradient_Norm"]), _table_key=("pwg_disc", id(self)))
        for group in self.optimizer.param_groups:
            group["lr"] = self.learning_rate(self.steps)
        for group in self.disc_optimizer.param_groups:
            group["lr"] = self.disc_learning_rate(self.disc_steps)
        self.optimizer.step()
        self.disc_optimizer.step()
        self.steps += 1
        self.disc_steps += 1
        self.last = {"Loss": loss.detach(), "Terms": self.criterion.terms, "Gradient_Norm": norm, "STFT_Loss": stft.detach(), "Discriminator_Loss": d_loss.detach(),
                     "L_adv": adv_terms[0], "Real_Term": adv_terms[1], "Fake_Term": adv_terms[2], "Discriminator_Gradient_Norm": d_norm}
        return loss.detach()

    @torch.no_grad()
    def Evaluation(self, batches=4):
        """-> (mean loss, mean (L_sc, L_mag) per resolution [n, 2]) over `batches` batches of the evaluation set; with the discriminator block, a third
        element: the mean (L_adv, real term, fake term) [3] of the current discriminator on the generated and the target segments."""
        if "Eval" not in self.sampler:
            return None
        losses, terms, adv = [], [], []
        for b in range(batches):
            if self.discriminator is None:
                losses.append(float(self.forward(*self.sampler["Eval"].batch(b), step=-1 - b)))
            else:
                out = self.forward(*self.sampler["Eval"].batch(b), step=-1 - b, adversarial=True)
                losses.append(float(out[3]))
                adv.append(out[2].cpu().double())
            terms.append(self.criterion.terms.cpu().double())
        ev = float(np.mean(losses)), torch.stack(terms).mean(0)
        return ev if self.discriminator is None else ev + (torch.stack(adv).mean(0),)

    def Save_Checkpoint(self):
        os.makedirs(self.set["Checkpoint_Path"], exist_ok=True)
        state = {"generator": {k: v.detach().cpu() for k, v in self.model.params.items()}, "Optimizer": self.optimizer.state_dict(), "Steps": self.steps}
        if self.discriminator is not None:
            state.update(discriminator={k: v.detach().cpu() for k, v in self.discriminator.params.items()},
                         Discriminator_Optimizer=self.disc_optimizer.state_dict(), Discriminator_Steps=self.disc_steps)
        torch.save(state, self.checkpoint_file(self.steps))
        logging.info("Checkpoint saved at %d steps.", self.steps)
        return self.checkpoint_file(self.steps)

    def Load_Checkpoint(self):
        state = torch.load(self.checkpoint_file(self.steps), map_location="cpu")
        with torch.no_grad():
            for k, v in pwg_load(state, self.geo).items():
                self.model.params[k].copy_(v)
        self.optimizer.load_state_dict(state["Optimizer"])
        self.steps = int(state["Steps"])
        if self.discriminator is not None:
            if "discriminator" not in state:
                raise ValueError("{} holds no discriminator: it was written without the block {}.Discriminator".format(self.checkpoint_file(self.steps), TRAIN_KEY))
            with torch.no_grad():
                for k, v in pwg_disc_load(state["discriminator"], self.discriminator.geo).items():
                    self.discriminator.params[k].copy_(v)
            self.disc_optimizer.load_state_dict(state["Discriminator_Optimizer"])
            self.disc_steps = int(state["Discriminator_Steps"])

    def Train(self):
        s = self.set
        while self.steps < int(s["Max_Step"]):
            loss = self.Train_Step(*self.sampler["Train"].batch(self.steps))
            if self.steps % int(s["Evaluation_Interval"]) == 0:
                ev = self.Evaluation()
                logging.info("Step %d: loss %.4f%s", self.steps, float(loss), "" if ev is None else ", evaluation loss {:.4f}, terms {}".format(ev[0], ev[1].tolist()))
                if ev is not None and len(ev) > 2:
                    logging.info("Step %d: evaluation L_adv %.4f, real term %.4f, fake term %.4f", self.steps, *ev[2].tolist())
                if "L_adv" in self.last:
                    logging.info("Step %d: L_adv %.4f, real term %.4f, fake term %.4f, discriminator loss %.4f", self.steps, float(self.last["L_adv"]),
                                 float(self.last["Real_Term"]), float(self.last["Fake_Term"]), float(self.last["Discriminator_Loss"]))
            if self.steps % int(s["Checkpoint_Save_Interval"]) == 0:
                self.Save_Checkpoint()
        if not os.path.exists(self.checkpoint_file(self.steps)):
            self.Save_Checkpoint()


def main(argv=None):
    ap = argparse.ArgumentParser(description="train the Parallel WaveGAN generator (stage one: multi-resolution STFT loss) on the pattern directories of "
                                             "Train.Train_Pattern / Train.Eval_Pattern")
    ap.add_argument("-hp", "--hyper_parameters", default=None, help="yaml to read instead of ./Hyper_Parameters.yaml")
    ap.add_argument("-s", "--steps", default=0, type=int, help="resume from PWG_<steps>.pt")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    hp = Recursive_Parse(load_yaml(args.hyper_parameters)) if args.hyper_parameters else get_hp()
    PWG_Trainer(steps=args.steps, hp=hp, device=args.device, seed=args.seed).Train()
