"""Trainer of the Parallel WaveGAN vocoder - `python Train_PWG.py -hp <yaml> -s <steps>`.  Stage one of its recipe (DESIGN.md "Training the Parallel WaveGAN
generator"): the generator alone under the multi-resolution STFT loss.  With the optional yaml block `Vocoder.Train.Discriminator`, stage two from its
`Start_Step` on (DESIGN.md "Training the Parallel WaveGAN discriminator"): the least-squares adversarial term joins the generator's loss and the
discriminator `vocoder.PWGDiscriminator` is trained beside it, with a clipping and a RAdam of its own.

Reads the pattern directories `Pattern_Generator.py` writes (through METADATA.PICKLE: `File_List`, `Mel_Length_Dict`, `Audio_Length_Dict`): every pattern
holds the raw `Audio` beside its `Mel`, frame f centred on sample f * Frame_Shift.  Draws seeded batches of mel segments with the audio under them, and steps
`vocoder.ParallelWaveGAN(trainable=True)` under `vocoder.MultiResolutionSTFTLoss` with the project's clipping and RAdam kernels (`optim`).  The checkpoints
`PWG_<steps>.pt` load unchanged through `Vocoder.Checkpoint_Path`.  The defaults of the optional yaml block `Vocoder.Train` restate the original recipe from
memory: they are this project's contract, not a pinned one."""
import hashlib
import logging

import numpy as np
import torch

from . import aux_trainer, optim
from .hparams import get_hp, overlay_settings
from .vocoder import (STFT_RESOLUTIONS, MelSpectrogramLoss, MultiResolutionSTFTLoss, ParallelWaveGAN, PWGDiscriminator, adversarial_mse, mel_loss_geometry,
                      mel_loss_settings, pwg_disc_load, pwg_disc_settings, pwg_geometry, pwg_load, stft_loss_geometry)

TRAIN_KEY = "Vocoder.Train"
MEL_BLOCK = "Mel_Loss"                                     # the optional sub-block of the mel-L1 term, of every vocoder trainer
DEFAULTS = {"Batch_Size": 8, "Segment_Frames": 100, "Learning_Rate": 1.0e-4, "Epsilon": 1.0e-6, "Gradient_Norm": 10.0,
            "Learning_Rate_Decay": {"Step": 200000, "Gamma": 0.5}, "STFT_Resolutions": [list(r) for r in STFT_RESOLUTIONS], "Max_Step": 100000,
            "Checkpoint_Save_Interval": 5000, "Evaluation_Interval": 1000, "Checkpoint_Path": "./pwg_results"}
# What is updated in a step, the generator's first: (attribute prefix of params / optimizer / set / steps, the attribute of the model, the clipping's table
# key, the loader of its state dict, the checkpoint keys of its parameters / optimizer state / update count)
BUNDLES = (("", "model", "pwg", pwg_load, ("generator", "Optimizer", "Steps")),
           ("disc_", "discriminator", "pwg_disc", pwg_disc_load, ("discriminator", "Discriminator_Optimizer", "Discriminator_Steps")))


def train_settings(hp, defaults=DEFAULTS, also=("Discriminator",)):
    """The optional yaml block `Vocoder.Train` over `defaults` (`hparams.overlay_settings`), checked: a ValueError names every bad key.  The optional
    sub-block `Discriminator` (`vocoder.pwg_disc_settings`) appears in the result only when the yaml has it.  also: the sub-blocks the caller allows and
    reads (another trainer's stage two has another key).  The optional sub-block `Mel_Loss` (`vocoder.mel_loss_settings`, checked against the segment
    length by `vocoder.mel_loss_geometry`) is allowed beside them and appears in the result only when the yaml has it."""
    def rules(s, need):
        for k in ("Batch_Size", "Segment_Frames", "Max_Step", "Checkpoint_Save_Interval", "Evaluation_Interval"):
            need(k, lambda v: int(v) >= 1, "at least 1")
        for k in ("Learning_Rate", "Epsilon", "Gradient_Norm"):
            need(k, lambda v: float(v) > 0, "positive")
        need("Learning_Rate_Decay", lambda v: int(v["Step"]) >= 1 and 0 < float(v["Gamma"]) <= 1, "Step >= 1, 0 < Gamma <= 1")
    s = overlay_settings(getattr(getattr(hp, "Vocoder", None), "Train", None), defaults, TRAIN_KEY, "vocoder", rules, also=tuple(also) + (MEL_BLOCK,))
    s["STFT_Resolutions"] = stft_loss_geometry(s["STFT_Resolutions"], int(s["Segment_Frames"]) * int(hp.Sound.Frame_Shift))
    if "Discriminator" in s:
        s["Discriminator"] = pwg_disc_settings(hp)
    if MEL_BLOCK in s:
        s[MEL_BLOCK] = mel_loss_settings(hp)
        mel_loss_geometry(hp, s[MEL_BLOCK], int(s["Segment_Frames"]) * int(hp.Sound.Frame_Shift))
    return s


def step_decay(settings, count):
    """The host-side step decay of a rate: Learning_Rate * Gamma^(count // Step)"""
    d = settings["Learning_Rate_Decay"]
    return float(settings["Learning_Rate"]) * float(d["Gamma"]) ** (int(count) // int(d["Step"]))


def noise_seed_words(seed, step, index):
    """The two 32-bit seed words of the noise of batch row `index` at step `step` of the run `seed`: the first 8 bytes of blake2b of
    "<seed> NUL <step> NUL <index> NUL pwgtrain", little endian; z is drawn from them in `pwg_first`, so a run repeats and no z tensor exists."""
    d = hashlib.blake2b("{}\0{}\0{}\0pwgtrain".format(seed, step, index).encode()).digest()
    return int.from_bytes(d[:4], "little"), int.from_bytes(d[4:8], "little")


class Sampler(aux_trainer.PatternSampler):
    """Batches of (mel segment, the audio under it) from one pattern directory.  Batch `step` is a function of (seed, step) alone: `batch` files among those
    whose mel has at least `frames` frames and whose audio at least `frames * hop` samples, and for each a start frame f0 with
    (f0 + frames) * hop <= its audio length.  The target is the pattern's raw audio - final audio, without pre-emphasis or de-emphasis."""

    def __init__(self, pattern_path, metadata_file, batch, frames, hop, seed=0, cache=True):
        super().__init__(pattern_path, metadata_file, seed, cache)
        self.B, self.frames, self.hop = int(batch), int(frames), int(hop)
        mel, audio = self.meta["Mel_Length_Dict"], self.meta["Audio_Length_Dict"]
        self.starts = {f: min(mel[f], audio[f] // self.hop) - self.frames for f in sorted(self.meta["File_List"])}     # the largest f0 of a file
        self.files = [f for f, n in self.starts.items() if n >= 0]
        if not self.files:
            raise ValueError("{}: no pattern has {} frames with {} samples of audio under them ({}.Segment_Frames)".format(
                pattern_path, self.frames, self.frames * self.hop, TRAIN_KEY))

    def plan(self, step):
        """-> [(file, f0)] * batch of batch `step`"""
        rng = self.rng(step)
        rows = []
        for _ in range(self.B):
            f = self.files[int(rng.integers(0, len(self.files)))]
            rows.append((f, int(rng.integers(0, self.starts[f] + 1))))
        return rows

    def read(self, p):
        return np.asarray(p["Mel"], np.float32), np.asarray(p["Audio"], np.float32)

    def batch(self, step):
        """-> (mel [B, Mel, frames], target [B, frames * hop]) float32 host tensors"""
        mels, wavs = [], []
        for f, f0 in self.plan(step):
            mel, audio = self.pattern(f)
            mels.append(mel[f0:f0 + self.frames].T)
            wavs.append(audio[f0 * self.hop:(f0 + self.frames) * self.hop])
        return torch.from_numpy(np.stack(mels).astype(np.float32)), torch.from_numpy(np.stack(wavs).astype(np.float32))


class PWG_Trainer(aux_trainer.Trainer):
    """A subclass for another generator (`hifigan_trainer.HiFiGAN_Trainer`) replaces PREFIX, BUNDLES, DISC_BLOCK and the hooks below `__init__`."""
    PREFIX = "PWG"
    BUNDLES = BUNDLES
    DISC_BLOCK = "Discriminator"                           # the key of `settings` (and of Vocoder.Train) that holds stage two's block

    def __init__(self, steps=0, hp=None, device="cuda:0", seed=0):
        hp = hp if hp is not None else get_hp()
        self.geo = self.geometry(hp)
        s = self.settings(hp)
        super().__init__(hp, s, steps, device, seed, Sampler, (s["Batch_Size"], s["Segment_Frames"], self.geo["hop"]))
        self.model = self.make_model()
        self.criterion = MultiResolutionSTFTLoss(s["STFT_Resolutions"], self.device)
        # the mel-L1 term (optional block Vocoder.Train.Mel_Loss; DESIGN.md "Mel loss"): stateless, so no checkpoint knows of it
        self.mel_set, self.mel_criterion, self.last_evaluation_mel = s.get(MEL_BLOCK), None, None
        if self.mel_set is not None:
            self.mel_criterion = MelSpectrogramLoss(hp, self.device, self.mel_set)
        self.params = list(self.model.params.values())
        self.optimizer = optim.RAdam(self.params, lr=float(s["Learning_Rate"]), eps=float(s["Epsilon"]))
        # stage two (optional block Vocoder.Train.Discriminator): initialised from the seed at construction, untouched before Start_Step
        self.disc_set, self.discriminator, self.disc_steps = s.get(self.DISC_BLOCK), None, 0
        if self.disc_set is not None:
            self.discriminator = self.make_discriminator()
            self.disc_params = list(self.discriminator.params.values())
            self.disc_optimizer = optim.RAdam(self.disc_params, lr=float(self.disc_set["Learning_Rate"]), eps=float(self.disc_set["Epsilon"]))
        if self.steps > 0:
            self.Load_Checkpoint()

    geometry, settings = staticmethod(pwg_geometry), staticmethod(train_settings)

    def make_model(self):
        return ParallelWaveGAN(self.hp, self.device, trainable=True, seed=self.seed, precision="f32")            # (Vocoder.Precision is a serving setting)

    def make_discriminator(self):
        return PWGDiscriminator(self.hp, self.device, trainable=True, seed=self.seed)

    def adversarial_losses(self, target, wav, stft):
        """-> (L_G, L_D, the unscaled (L_adv, real term, fake term) [3], L_stft) from one discriminator forward over [target; wav]"""
        both, p_fake = self.discriminator.score_pair(target, wav)
        adv, adv_terms = adversarial_mse(p_fake, 1.0, float(self.disc_set["Lambda_Adversarial"]))
        d_loss, d_terms = adversarial_mse(both, (1.0, 0.0))
        return stft + adv, d_loss, torch.cat([adv_terms[:1], d_terms]), stft

    def without_discriminator(self, state):
        """The bundles to load from a checkpoint `state` that holds no discriminator although this run has one (here: none, an error)"""
        raise ValueError("{} holds no discriminator: it was written without the block {}.{}".format(self.checkpoint_file(self.steps), TRAIN_KEY, self.DISC_BLOCK))

    def generate(self, mel, lengths, step):
        """The generator's waveform of batch `step` with its backward"""
        return self.model.generate(mel, lengths, seeds=self.seeds(step, mel.shape[0]))[0]

    def learning_rate(self, step):
        return step_decay(self.set, step)

    def seeds(self, step, B):
        return torch.tensor([noise_seed_words(self.seed, step, i) for i in range(B)], dtype=torch.int64)

    def disc_learning_rate(self, updates):
        """The discriminator's step decay counts its own updates"""
        return step_decay(self.disc_set, updates)

    def adversarial(self, step):
        return self.disc_set is not None and int(step) >= int(self.disc_set["Start_Step"])

    def forward(self, mel, target, step, adversarial=False):
        """-> L_stft, or with `adversarial` (L_G = L_stft + Lambda_Adversarial L_adv, L_D, the unscaled (L_adv, real term, fake term) [3]): one discriminator
        forward over [target; wav]; L_G's backward reaches the generator alone, L_D's the discriminator alone.  With the block Vocoder.Train.Mel_Loss,
        L_stft + Lambda L_mel stands wherever L_stft does (L_D is unchanged); the unscaled L_mel is `self.mel_criterion.term`."""
        mel, target = mel.to(self.device, non_blocking=True), target.to(self.device, non_blocking=True)
        B, _, L = mel.shape
        wav = self.generate(mel, [L] * B, step)
        stft = self.criterion(wav, target)
        if self.mel_criterion is not None:
            stft = stft + float(self.mel_set["Lambda"]) * self.mel_criterion(wav, target)
        if not adversarial:
            return stft
        return self.adversarial_losses(target, wav, stft)

    def update(self, bundles, losses):
        """The backwards of `losses`, then the update of every bundle of `bundles` -> its gradient norms.  Phase by phase over the bundles, so that both
        updates of an adversarial step are computed from the state before it: zero gradients, every backward, every clipping, every rate, every optimizer
        step, every count."""
        get = lambda b, name: getattr(self, b[0] + name)
        for b in bundles:
            for p in get(b, "params"):
                p.grad = None
        for loss in losses:
            loss.backward()
        norms = [optim.clip_grad_norm_(get(b, "params"), float(get(b, "set")["Gradient_Norm"]), _table_key=(b[2], id(self))) for b in bundles]
        for b in bundles:
            for group in get(b, "optimizer").param_groups:
                group["lr"] = step_decay(get(b, "set"), get(b, "steps"))
        for b in bundles:
            get(b, "optimizer").step()                                                     # (the next forward rebuilds the weight images from the parameters)
        for b in bundles:
            setattr(self, b[0] + "steps", get(b, "steps") + 1)
        return norms

    def Train_Step(self, mel, target):
        """One step on a host or device batch (mel [B, Mel, frames], target [B, frames * hop]); returns the generator's loss (0-d device tensor)."""
        if self.adversarial(self.steps):
            return self.Adversarial_Step(mel, target)
        loss = self.forward(mel, target, self.steps)
        norm, = self.update(self.BUNDLES[:1], [loss])
        self.last = {"Loss": loss.detach(), "Terms": self.criterion.terms, "Gradient_Norm": norm}
        self.note_mel()
        return loss.detach()

    def Adversarial_Step(self, mel, target):
        """A step of stage two: both updates are computed from the state before the step (the discriminator's forward and both backwards precede both updates).
        The backward of `loss` reaches the generator alone (the fake rows' data chain, no weight gradients), that of `d_loss` the discriminator alone."""
        loss, d_loss, adv_terms, stft = self.forward(mel, target, self.steps, adversarial=True)
        norm, d_norm = self.update(self.BUNDLES, [loss, d_loss])
        self.last = {"Loss": loss.detach(), "Terms": self.criterion.terms, "Gradient_Norm": norm, "STFT_Loss": stft.detach(), "Discriminator_Loss": d_loss.detach(),
                     "L_adv": adv_terms[0], "Real_Term": adv_terms[1], "Fake_Term": adv_terms[2], "Discriminator_Gradient_Norm": d_norm}
        self.note_mel()
        return loss.detach()

    def note_mel(self):
        """`last` gains the unscaled mel term of the step when the block Vocoder.Train.Mel_Loss is there"""
        if self.mel_criterion is not None:
            self.last["Mel_Loss"] = self.mel_criterion.term

    @torch.no_grad()
    def Evaluation(self, batches=4):
        """-> (mean loss, mean (L_sc, L_mag) per resolution [n, 2]) over `batches` batches of the evaluation set; with the discriminator block, a third
        element: the mean (L_adv, real term, fake term) [3] of the current discriminator on the generated and the target segments.  With the block
        Vocoder.Train.Mel_Loss the loss is L_stft + Lambda L_mel and the mean unscaled L_mel goes to `self.last_evaluation_mel`."""
        if "Eval" not in self.sampler:
            return None
        losses, terms, adv, mel = [], [], [], []
        for b in range(batches):
            if self.discriminator is None:
                losses.append(float(self.forward(*self.sampler["Eval"].batch(b), step=-1 - b)))
            else:
                out = self.forward(*self.sampler["Eval"].batch(b), step=-1 - b, adversarial=True)
                losses.append(float(out[3]))
                adv.append(out[2].cpu().double())
            terms.append(self.criterion.terms.cpu().double())
            if self.mel_criterion is not None:
                mel.append(float(self.mel_criterion.term))
        self.last_evaluation_mel = float(np.mean(mel)) if mel else None
        ev = float(np.mean(losses)), torch.stack(terms).mean(0)
        return ev if self.discriminator is None else ev + (torch.stack(adv).mean(0),)

    def bundles(self):
        return self.BUNDLES if self.discriminator is not None else self.BUNDLES[:1]

    def state_dict(self):
        state = {}
        for prefix, model, _, _, (params, optimizer, steps) in self.bundles():
            state[params] = {k: v.detach().cpu() for k, v in getattr(self, model).params.items()}
            state[optimizer], state[steps] = getattr(self, prefix + "optimizer").state_dict(), getattr(self, prefix + "steps")
        return state

    def load_state_dict(self, state):
        bundles = self.bundles()
        if self.discriminator is not None and "discriminator" not in state:
            bundles = self.without_discriminator(state)
        for prefix, model, _, load, (_, optimizer, steps) in bundles:
            model = getattr(self, model)
            with torch.no_grad():
                for k, v in load(state, model.geo).items():
                    model.params[k].copy_(v)
            getattr(self, prefix + "optimizer").load_state_dict(state[optimizer])
            setattr(self, prefix + "steps", int(state[steps]))

    def log_evaluation(self, loss, ev):
        logging.info("Step %d: loss %.4f%s", self.steps, float(loss), "" if ev is None else ", evaluation loss {:.4f}, terms {}".format(ev[0], ev[1].tolist()))
        if ev is not None and len(ev) > 2:
            logging.info("Step %d: evaluation L_adv %.4f, real term %.4f, fake term %.4f", self.steps, *ev[2].tolist())
        if "Mel_Loss" in self.last:
            logging.info("Step %d: mel loss %.4f%s", self.steps, float(self.last["Mel_Loss"]),
                         "" if self.last_evaluation_mel is None else ", evaluation mel loss {:.4f}".format(self.last_evaluation_mel))
        if "L_adv" in self.last:
            logging.info("Step %d: L_adv %.4f, real term %.4f, fake term %.4f, discriminator loss %.4f", self.steps, float(self.last["L_adv"]),
                         float(self.last["Real_Term"]), float(self.last["Fake_Term"]), float(self.last["Discriminator_Loss"]))


def main(argv=None):
    aux_trainer.main("train the Parallel WaveGAN generator (stage one: multi-resolution STFT loss) on the pattern directories of Train.Train_Pattern / "
                     "Train.Eval_Pattern", PWG_Trainer, argv)
