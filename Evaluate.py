"""Objective evaluation (no counterpart in the reference): `python Evaluate.py -hp <yaml> --pairs LIST.tsv -o DIR` compares existing mels / wavs,
`python Evaluate.py -c <checkpoint> --patterns [N] --seed 0 -o DIR` synthesises the evaluation patterns' texts and compares them with the recordings; the
implementation is glow_tts_amd/evaluation.py."""
from glow_tts_amd.evaluation import Evaluator, main  # noqa: F401

if __name__ == "__main__":
    main()
