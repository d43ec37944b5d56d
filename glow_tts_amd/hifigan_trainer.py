"""Trainer of the HiFi-GAN vocoder - `python Train_HiFiGAN.py -hp <yaml> [-s <steps>] [--seed 0]`.  Stage one alone (DESIGN.md "Training the HiFi-GAN
generator"): the generator `vocoder.HiFiGAN(trainable=True)` under the multi-resolution STFT loss, with the project's clipping and RAdam kernels and the
host-side step decay.  The sampler, the update, the evaluation and the checkpoint code are `pwg_trainer.PWG_Trainer`'s: the batches are the Parallel WaveGAN
trainer's (mel segments with the final audio under them, from the same pattern directories, so the `DIR/GTA` tree of `Align.py --gta` works unchanged).
The generator has no noise input: the seed fixes the initialisation and the batches.  The checkpoints `HIFIGAN_<steps>.pt` (`generator`, `Optimizer`, `Steps`)
load unchanged through `Vocoder.Checkpoint_Path` of a `Type: 'HiFiGAN'` block.  The settings are the optional block `Vocoder.Train` of such a block, with
`pwg_trainer`'s keys and rules; the defaults of an absent block are this project's contract, not a pinned recipe.  The multi-period and multi-scale
discriminators, the feature-matching and the mel losses are out of scope: a `Vocoder.Train.Discriminator` block is refused."""
from . import aux_trainer, pwg_trainer
from .hparams import plain_block
from .vocoder import HiFiGAN, hifigan_geometry, hifigan_load

TRAIN_KEY = pwg_trainer.TRAIN_KEY
DEFAULTS = dict(pwg_trainer.DEFAULTS, Batch_Size=16, Segment_Frames=32, Learning_Rate=2.0e-4, Checkpoint_Path="./hifigan_results")
BUNDLES = (("", "model", "hifigan", hifigan_load, ("generator", "Optimizer", "Steps")),)


def train_settings(hp):
    """The optional yaml block `Vocoder.Train` of a `Type: 'HiFiGAN'` block over DEFAULTS, under `pwg_trainer.train_settings`' rules.  A block of another
    `Vocoder.Type` (or none) and a `Vocoder.Train.Discriminator` sub-block raise a ValueError naming the key."""
    block = getattr(hp, "Vocoder", None)
    kind = getattr(block, "Type", None)
    if kind != "HiFiGAN":
        raise ValueError(f"Vocoder.Type = {kind!r}: Train_HiFiGAN.py trains the generator of a Vocoder block with Type: 'HiFiGAN' (Train_PWG.py trains a 'PWG' block)")
    train = plain_block(getattr(block, "Train", None)) or {}
    if isinstance(train, dict) and "Discriminator" in train:
        raise ValueError(f"{TRAIN_KEY}.Discriminator: the HiFi-GAN trainer is stage one alone (multi-resolution STFT loss); its discriminators are not implemented "
                         "and the Parallel WaveGAN discriminator does not train this generator")
    return pwg_trainer.train_settings(hp, DEFAULTS)


class HiFiGAN_Trainer(pwg_trainer.PWG_Trainer):
    PREFIX = "HIFIGAN"
    BUNDLES = BUNDLES
    geometry, settings = staticmethod(hifigan_geometry), staticmethod(train_settings)

    def make_model(self):
        return HiFiGAN(self.hp, self.device, trainable=True, seed=self.seed)

    def generate(self, mel, lengths, step):
        return self.model.generate(mel, lengths)[0]


def main(argv=None):
    aux_trainer.main("train the HiFi-GAN generator (stage one: multi-resolution STFT loss) on the pattern directories of Train.Train_Pattern / "
                     "Train.Eval_Pattern", HiFiGAN_Trainer, argv)
