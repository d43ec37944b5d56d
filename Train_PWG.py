"""Trains the Parallel WaveGAN generator (stage one: multi-resolution STFT loss): `python Train_PWG.py -hp <yaml> [-s <steps to resume from>] [--seed 0]`;
the implementation is glow_tts_amd/pwg_trainer.py."""
from glow_tts_amd.pwg_trainer import PWG_Trainer, main  # noqa: F401

if __name__ == "__main__":
    main()
