"""Teacher-forced alignment and ground-truth-aligned mels (no counterpart in the reference): `python Align.py -c <checkpoint> --patterns {train,eval}
[--limit N] -o DIR [--gta] [--seed 0] [--noise-scale 1.0]` runs a trained GlowTTS over its own training patterns and writes token durations, alignment
scores and - with --gta - a pattern tree whose mels are the model's own, frame-aligned with the recorded audio, for fine-tuning the vocoder; the
implementation is glow_tts_amd/aligner.py."""
from glow_tts_amd.aligner import main  # noqa: F401

if __name__ == "__main__":
    main()
