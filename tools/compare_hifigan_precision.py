"""How far is the HiFi-GAN vocoder's fp16 inference mode from its f32 mode on a TRAINED generator?  The twin of tools/compare_pwg_precision.py.  For every
mel of a `--vocode` list (one `label<TAB>mel.npy` per line, mels [T, Mel]) the checkpoint's generator vocodes in both precisions, one utterance per call
(the generator has no noise input), and the tool prints
  * the SNR in dB of the f16 waveform against the f32 one, 10 log10(sum f32^2 / sum (f16 - f32)^2),
  * the multi-resolution STFT loss (`vocoder.MultiResolutionSTFTLoss`, the training criterion's resolutions) of f16 against f32, and
  * the mel-spectrogram L1 (`vocoder.MelSpectrogramLoss`: mean |ln mel(f32) - ln mel(f16)| at the analysis geometry of the yaml's `Sound` block)
per utterance and their means.  The sizes come from the yaml's `Vocoder` block (`Type: 'HiFiGAN'`), like Inference.py's.  Needs a GPU: both paths are HIP
kernels.
Usage: python tools/compare_hifigan_precision.py --checkpoint HIFIGAN_x.pt --list LIST"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def compare(hp, checkpoint, records, device="cuda:0"):
    """records [(label, mel .npy path or array [T, Mel])] -> [{"label", "samples", "snr_db", "stft_loss", "mel_l1"}], one per record"""
    from glow_tts_amd.vocoder import HiFiGAN, MelSpectrogramLoss, MultiResolutionSTFTLoss
    sd = torch.load(checkpoint, map_location="cpu") if isinstance(checkpoint, str) else checkpoint
    f32, f16 = (HiFiGAN(hp, device, state_dict=sd, precision=p) for p in ("f32", "f16"))
    stft, mel_l1 = MultiResolutionSTFTLoss(device=device), MelSpectrogramLoss(hp, device)
    rows = []
    for label, mel in records:
        mel = torch.from_numpy(np.load(mel).astype(np.float32) if isinstance(mel, str) else np.asarray(mel, np.float32))
        mels, lengths = mel.T[None].contiguous().to(device), torch.tensor([mel.shape[0]])
        a, b = f32(mels, lengths)[0], f16(mels, lengths)[0]
        noise = float((b.double() - a.double()).square().sum())
        snr = 10.0 * math.log10(float(a.double().square().sum()) / noise) if noise > 0 else math.inf
        rows.append({"label": str(label), "samples": int(a.shape[1]), "snr_db": snr, "stft_loss": float(stft(b, a)), "mel_l1": float(mel_l1(b, a))})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True, help="HiFi-GAN generator checkpoint (as --vocoder-checkpoint of Inference.py)")
    ap.add_argument("--list", required=True, help="one label<TAB>mel.npy ([T, Mel]) per line (the --vocode list of Inference.py)")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "compare_hifigan_precision.py runs both precisions on the GPU"
    from glow_tts_amd.hparams import get_hp
    from glow_tts_amd.inferencer import read_vocode_list
    rows = compare(get_hp(), args.checkpoint, read_vocode_list(args.list))
    for r in rows:
        print("{label}\t{samples} samples\tSNR {snr_db:.2f} dB\tSTFT loss {stft_loss:.5f}\tmel L1 {mel_l1:.5f}".format(**r))
    mean = lambda k: sum(r[k] for r in rows) / len(rows)
    print(json.dumps({"utterances": len(rows), "mean_snr_db": mean("snr_db"), "min_snr_db": min(r["snr_db"] for r in rows), "mean_stft_loss": mean("stft_loss"),
                      "mean_mel_l1": mean("mel_l1")}))
    return rows


if __name__ == "__main__":
    main()
