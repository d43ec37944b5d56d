"""How far is the neural vocoder's bf16 inference mode from its f32 mode on a TRAINED generator?  For every mel of a `--vocode` list (one
`label<TAB>mel.npy` per line, mels [T, Mel]) the checkpoint's generator vocodes in both precisions from the SAME noise (the seed words of
`vocoder.pwg_seed_words(seed, label)`), one utterance per call, and the tool prints
  * the SNR in dB of the bf16 waveform against the f32 one, 10 log10(sum f32^2 / sum (bf16 - f32)^2), and
  * the multi-resolution STFT loss (`vocoder.MultiResolutionSTFTLoss`, the training criterion's resolutions) of bf16 against f32
per utterance and their means.  The sizes come from the yaml's `Vocoder` block, like Inference.py's.  Needs a GPU: both paths are HIP kernels.
Usage: python tools/compare_pwg_precision.py --checkpoint PWG_x.pt --list LIST [--seed 0]"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def compare(hp, checkpoint, records, seed=0, device="cuda:0"):
    """records [(label, mel .npy path or array [T, Mel])] -> [{"label", "samples", "snr_db", "stft_loss"}], one per record"""
    from glow_tts_amd.vocoder import MultiResolutionSTFTLoss, ParallelWaveGAN, pwg_seed_words
    sd = torch.load(checkpoint, map_location="cpu")
    f32, bf16 = (ParallelWaveGAN(hp, device, state_dict=sd, precision=p) for p in ("f32", "bf16"))
    loss = MultiResolutionSTFTLoss(device=device)
    rows = []
    for label, mel in records:
        mel = torch.from_numpy(np.load(mel).astype(np.float32) if isinstance(mel, str) else np.asarray(mel, np.float32))
        mels, lengths = mel.T[None].contiguous().to(device), torch.tensor([mel.shape[0]])
        seeds = torch.tensor([pwg_seed_words(seed, label)], dtype=torch.int64)
        a, b = f32(mels, lengths, seeds=seeds)[0], bf16(mels, lengths, seeds=seeds)[0]
        noise = float((b.double() - a.double()).square().sum())
        snr = 10.0 * math.log10(float(a.double().square().sum()) / noise) if noise > 0 else math.inf
        rows.append({"label": str(label), "samples": int(a.shape[1]), "snr_db": snr, "stft_loss": float(loss(b, a))})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True, help="Parallel WaveGAN generator checkpoint (as --vocoder-checkpoint of Inference.py)")
    ap.add_argument("--list", required=True, help="one label<TAB>mel.npy ([T, Mel]) per line (the --vocode list of Inference.py)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "compare_pwg_precision.py runs both precisions on the GPU"
    from glow_tts_amd.hparams import get_hp
    from glow_tts_amd.inferencer import read_vocode_list
    rows = compare(get_hp(), args.checkpoint, read_vocode_list(args.list), args.seed)
    for r in rows:
        print("{label}\t{samples} samples\tSNR {snr_db:.2f} dB\tSTFT loss {stft_loss:.5f}".format(**r))
    print(json.dumps({"utterances": len(rows), "mean_snr_db": sum(r["snr_db"] for r in rows) / len(rows), "min_snr_db": min(r["snr_db"] for r in rows),
                      "mean_stft_loss": sum(r["stft_loss"] for r in rows) / len(rows)}))
    return rows


if __name__ == "__main__":
    main()
