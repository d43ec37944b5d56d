"""Trainer of the HiFi-GAN vocoder - `python Train_HiFiGAN.py -hp <yaml> [-s <steps>] [--seed 0]`.  Stage one (DESIGN.md "Training the HiFi-GAN
generator"): the generator `vocoder.HiFiGAN(trainable=True)` under the multi-resolution STFT loss, with the project's clipping and RAdam kernels and the
host-side step decay.  The sampler, the update, the evaluation and the checkpoint code are `pwg_trainer.PWG_Trainer`'s: the batches are the Parallel WaveGAN
trainer's (mel segments with the final audio under them, from the same pattern directories, so the `DIR/GTA` tree of `Align.py --gta` works unchanged).
The generator has no noise input: the seed fixes the initialisation and the batches.  The checkpoints `HIFIGAN_<steps>.pt` (`generator`, `Optimizer`, `Steps`)
load unchanged through `Vocoder.Checkpoint_Path` of a `Type: 'HiFiGAN'` block.  The settings are the optional block `Vocoder.Train` of such a block, with
`pwg_trainer`'s keys and rules; the defaults of an absent block are this project's contract, not a pinned recipe.  `Vocoder.Train.Precision: 'mixed'` trains the generator in mixed precision
(f16 forward, bf16 backward, fp32 master weights, optimizer and checkpoints; DESIGN.md "Training the HiFi-GAN generator: mixed precision") in both stages; the
discriminators, the losses and d wav stay f32, and a run may resume in either precision.

Stage two (DESIGN.md "Training the HiFi-GAN discriminator"), with the optional sub-block `Vocoder.Train.Adversarial` (`vocoder.hifigan_disc_settings`): from
`Start_Step` on every step is `PWG_Trainer.Adversarial_Step` with the multi-period discriminator `vocoder.HiFiGANPeriodDiscriminator` -
L_G = L_stft + Lambda_Adversarial sum_p mean((D_p(G) - 1)^2) + Lambda_Feature_Matching L_fm, L_D = sum_p [mean((D_p(y) - 1)^2) + mean(D_p(G.detach())^2)] -
both updates from the state before the step, the discriminator with a clipping, a RAdam and a step decay over its own update count; the checkpoint also
carries `discriminator`, `Discriminator_Optimizer`, `Discriminator_Steps`.  A stage-one checkpoint (no `discriminator`) whose `Steps <= Start_Step` resumes
with the seeded-init discriminator.  Without the sub-block nothing differs from stage one alone.  The optional sub-block
`Vocoder.Train.Mel_Loss` (DESIGN.md "Mel loss") adds Lambda L_mel to L_stft in both stages, through `PWG_Trainer.forward`.  The optional sub-block
`Vocoder.Train.Adversarial.Multi_Scale` (DESIGN.md "The multi-scale discriminator") adds the multi-scale discriminator: the discriminator is then
`vocoder.HiFiGANDiscriminators`, the sums over p above run over the periods and then the scales, L_fm is the periods' sum plus the scales', and the one
discriminator optimizer, clipping and step decay cover the union of the parameters (the scales' under `scale_discriminators.`), which is what the
checkpoint's `discriminator` then holds.  A checkpoint whose `discriminator` lacks the scales' names resumes such a run only under the stage-one rule
(`Steps <= Start_Step`: both seeded inits are untouched).  Without the sub-block nothing differs.  The optional key
`Vocoder.Train.Adversarial.Precision: 'bf16'` (DESIGN.md "The multi-period discriminator in bf16") runs the multi-period discriminator's middle convolutions
on bf16 MFMAs, forward and backward, over fp32 master weights, tensors, optimizer and checkpoints; it governs the period discriminator alone (the
multi-scale discriminator stays f32), is read by the discriminator's constructor from the yaml, and a run resumes in either precision.  A `Vocoder.Train.Discriminator` block - the Parallel
WaveGAN discriminator's - is refused."""
import logging

import torch

from . import aux_trainer, pwg_trainer
from .hparams import plain_block
from .vocoder import (HIFIGAN_TRAIN_PRECISIONS, MSD_BLOCK, MSD_KEY, MSD_PREFIX, HiFiGAN, HiFiGANDiscriminators, HiFiGANPeriodDiscriminator, adversarial_mse,
                      hifigan_disc_load, hifigan_disc_settings, hifigan_discs_load, hifigan_geometry, hifigan_load)

TRAIN_KEY = pwg_trainer.TRAIN_KEY
DEFAULTS = dict(pwg_trainer.DEFAULTS, Batch_Size=16, Segment_Frames=32, Learning_Rate=2.0e-4, Checkpoint_Path="./hifigan_results")
# The optional key `Vocoder.Train.Precision`: 'f32' (absent: f32), or 'mixed' - the generator's f16 forward and bf16 backward over fp32 master weights (DESIGN.md
# "... mixed precision").  It appears in the settings only when the yaml has it, and is a key of this trainer alone: Train_PWG.py refuses it by name like any
# other unknown key.
PRECISION_KEY = "Precision"
BUNDLES = (("", "model", "hifigan", hifigan_load, ("generator", "Optimizer", "Steps")),
           ("disc_", "discriminator", "hifigan_disc", hifigan_disc_load, ("discriminator", "Discriminator_Optimizer", "Discriminator_Steps")))
# with the sub-block Multi_Scale the discriminator bundle is the union of both discriminators, under the same checkpoint keys
BUNDLES_MULTI_SCALE = (BUNDLES[0], BUNDLES[1][:3] + (hifigan_discs_load,) + BUNDLES[1][4:])
DISC_KEYS = BUNDLES[1][4]
ADV_KEY = "Adversarial"


def train_settings(hp):
    """The optional yaml block `Vocoder.Train` of a `Type: 'HiFiGAN'` block over DEFAULTS, under `pwg_trainer.train_settings`' rules.  A block of another
    `Vocoder.Type` (or none) and a `Vocoder.Train.Discriminator` sub-block raise a ValueError naming the key.  The optional sub-block `Adversarial`
    (`vocoder.hifigan_disc_settings`) appears in the result only when the yaml has it, and so does `Mel_Loss` (allowed by `pwg_trainer.train_settings`)."""
    block = getattr(hp, "Vocoder", None)
    kind = getattr(block, "Type", None)
    if kind != "HiFiGAN":
        raise ValueError(f"Vocoder.Type = {kind!r}: Train_HiFiGAN.py trains the generator of a Vocoder block with Type: 'HiFiGAN' (Train_PWG.py trains a 'PWG' block)")
    train = plain_block(getattr(block, "Train", None)) or {}
    if isinstance(train, dict) and "Discriminator" in train:
        raise ValueError(f"{TRAIN_KEY}.Discriminator is the Parallel WaveGAN discriminator's block, which does not train this generator: the HiFi-GAN "
                         f"adversarial stage (multi-period discriminator, feature matching) is the block {TRAIN_KEY}.{ADV_KEY}")
    s = pwg_trainer.train_settings(hp, DEFAULTS, also=(ADV_KEY, PRECISION_KEY))
    if s.get(PRECISION_KEY, "f32") not in HIFIGAN_TRAIN_PRECISIONS:
        raise ValueError(f"{TRAIN_KEY}.{PRECISION_KEY} = {s[PRECISION_KEY]!r}: the HiFi-GAN generator trains in 'f32' or 'mixed'")
    if ADV_KEY in s:
        s[ADV_KEY] = hifigan_disc_settings(hp)
    return s


class HiFiGAN_Trainer(pwg_trainer.PWG_Trainer):
    PREFIX = "HIFIGAN"
    BUNDLES = BUNDLES
    DISC_BLOCK = ADV_KEY
    geometry, settings = staticmethod(hifigan_geometry), staticmethod(train_settings)

    def make_model(self):
        return HiFiGAN(self.hp, self.device, trainable=True, seed=self.seed)     # the training precision: the yaml's Vocoder.Train.Precision

    def generate(self, mel, lengths, step):
        return self.model.generate(mel, lengths)[0]

    def make_discriminator(self):
        """The multi-period discriminator; with the sub-block Multi_Scale, both discriminators as one (and the bundle that loads their union)"""
        self.multi_scale = MSD_BLOCK in self.disc_set
        if not self.multi_scale:
            return HiFiGANPeriodDiscriminator(self.hp, self.device, trainable=True, seed=self.seed)
        self.BUNDLES = BUNDLES_MULTI_SCALE
        return HiFiGANDiscriminators(self.hp, self.device, trainable=True, seed=self.seed)

    def adversarial_losses(self, target, wav, stft):
        """-> (L_G, L_D, the unscaled (sum_p L_adv_p, sum_p real term, sum_p fake term) [3], L_stft) from one discriminator forward per period (then per
        scale) over [target; wav]; `self.fm`: the unscaled L_fm and its terms [periods, widths + 1]; `self.fm_scale`: the scales' terms [scales, layers + 1]
        or None."""
        both, p_fake, l_fm, fm_terms, *scale_terms = self.discriminator.score_pair(target, wav)
        self.fm_scale = scale_terms[0] if scale_terms else None
        adv, d_loss, d_terms = 0.0, 0.0, 0.0
        for b, p in zip(both, p_fake):                                      # period order
            a, _ = adversarial_mse(p, 1.0)
            d, t = adversarial_mse(b, (1.0, 0.0))
            adv, d_loss, d_terms = adv + a, d_loss + d, d_terms + t
        self.fm = (l_fm.detach(), fm_terms)
        loss = stft + float(self.disc_set["Lambda_Adversarial"]) * adv + float(self.disc_set["Lambda_Feature_Matching"]) * l_fm
        return loss, d_loss, torch.cat([adv.detach().reshape(1), d_terms]), stft

    def Adversarial_Step(self, mel, target):
        loss = super().Adversarial_Step(mel, target)
        self.last["L_fm"], self.last["FM_Terms"] = self.fm
        if self.fm_scale is not None:
            self.last["FM_Terms_Scale"] = self.fm_scale
        return loss

    def load_state_dict(self, state):
        """With the sub-block Multi_Scale, a checkpoint whose discriminator lacks the scales' names is a stage-one checkpoint for this run when its
        `Steps <= Start_Step` (no discriminator has been touched: both seeded inits are their state); later it cannot be resumed: ValueError naming the key."""
        if getattr(self, "multi_scale", False) and DISC_KEYS[0] in state and not any(str(k).startswith(MSD_PREFIX) for k in state[DISC_KEYS[0]]):
            if int(state["Steps"]) > int(self.disc_set["Start_Step"]):
                raise ValueError("{} holds no multi-scale discriminator (no key {}discriminators.0.convs.0.weight): it was written without the block {} and is "
                                 "past its Start_Step".format(self.checkpoint_file(self.steps), MSD_PREFIX, MSD_KEY))
            state = {k: v for k, v in state.items() if k not in DISC_KEYS}
        super().load_state_dict(state)

    def without_discriminator(self, state):
        """A stage-one checkpoint: up to Start_Step the discriminator has not been touched, so the seeded init of the constructor IS its state"""
        if int(state["Steps"]) > int(self.disc_set["Start_Step"]):
            return super().without_discriminator(state)
        return self.BUNDLES[:1]

    def log_evaluation(self, loss, ev):
        super().log_evaluation(loss, ev)
        if "L_fm" in self.last:
            logging.info("Step %d: L_fm %.4f", self.steps, float(self.last["L_fm"]))


def main(argv=None):
    aux_trainer.main("train the HiFi-GAN generator (multi-resolution STFT loss; with Vocoder.Train.Adversarial the adversarial stage) on the pattern directories of Train.Train_Pattern / "
                     "Train.Eval_Pattern", HiFiGAN_Trainer, argv)
