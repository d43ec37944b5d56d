"""Trains the HiFi-GAN generator (stage one: multi-resolution STFT loss): `python Train_HiFiGAN.py -hp <yaml> [-s <steps to resume from>] [--seed 0]`;
the implementation is glow_tts_amd/hifigan_trainer.py."""
from glow_tts_amd.hifigan_trainer import HiFiGAN_Trainer, main  # noqa: F401

if __name__ == "__main__":
    main()
