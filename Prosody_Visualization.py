"""Maps of the prosody / speaker vectors by exact t-SNE on the device (the reference's Prosody_Visualization.py, made repeatable): `python
Prosody_Visualization.py -c <checkpoint> --patterns {train,eval} [--what prosody|speaker] [--speakers 50] [--per-speaker 100] [--seed 0] -o DIR [--no-plot]`,
or `--vectors X.npy --labels L.tsv -o DIR` for any vectors; the implementation is glow_tts_amd/visualizer.py and glow_tts_amd/projection.py."""
from glow_tts_amd.visualizer import main, write_map  # noqa: F401

if __name__ == "__main__":
    main()
