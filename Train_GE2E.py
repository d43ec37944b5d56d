"""Trains the GE2E speaker encoder: `python Train_GE2E.py -hp <yaml> [-s <steps to resume from>]`; the implementation is glow_tts_amd/ge2e_trainer.py."""
from glow_tts_amd.ge2e_trainer import GE2E_Trainer, main  # noqa: F401

if __name__ == "__main__":
    main()
