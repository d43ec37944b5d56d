"""Reference of the mel-spectrogram L1 loss, written from DESIGN.md ("Mel loss") and not from the product code: torch.stft with the Hann window padded to
n_fft, |X| = sqrt(re^2 + im^2 + 1e-9), the dense `audio.mel_filterbank` as a matmul, ln(max(., Floor)), the mean absolute difference - under autograd.
float64 by default; the same code in float32 on the CPU is the yardstick of the error bar (`pwg_train_ref.check`).  Shared by tests/test_mel_loss_cpu.py,
tests/test_gpu_mel_loss.py and tests/test_gpu_mel_loss_trainer.py."""
import copy
import math

import torch

from glow_tts_amd import audio

EPS = 1e-9
DEFAULT = {"n_fft": 2048, "hop": 256, "win": 1024, "mel": 80, "sample_rate": 24000, "f_min": 125.0, "f_max": 7600.0, "floor": 1e-5}
SMALL = dict(DEFAULT, n_fft=256, hop=50, win=240, mel=20)                       # win / hop is not an integer


def hp_dict(base, geo):
    """The yaml dict `base` with the Sound block of the geometry `geo`"""
    d = copy.deepcopy(base)
    d["Sound"].update(Spectrogram_Dim=geo["n_fft"] // 2 + 1, Frame_Length=geo["win"], Frame_Shift=geo["hop"], Mel_Dim=geo["mel"], Sample_Rate=geo["sample_rate"],
                      Mel_F_Min=geo["f_min"], Mel_F_Max=geo["f_max"])
    return d


def padded_window(geo, dtype):
    """The periodic Hann window of `win`, centred in n_fft"""
    n_fft, win = geo["n_fft"], geo["win"]
    w = 0.5 - 0.5 * torch.cos(2.0 * math.pi * torch.arange(win, dtype=torch.float64) / win)
    lpad = (n_fft - win) // 2
    return torch.nn.functional.pad(w, (lpad, n_fft - win - lpad)).to(dtype)


def mel(x, geo, eps=EPS):
    """x [B, T] -> mel [B, Mel, frames] (before the floor and the log) in x's dtype; eps: the constant inside the root (the contract's; 0 gives the plain
    magnitude, which is what tests/test_mel_loss_cpu.py sets beside the front end's)"""
    X = torch.stft(x, geo["n_fft"], geo["hop"], geo["n_fft"], padded_window(geo, x.dtype), center=True, pad_mode="reflect", return_complex=True)
    mag = torch.sqrt(X.real ** 2 + X.imag ** 2 + eps)
    fb = torch.from_numpy(audio.mel_filterbank(geo["sample_rate"], geo["n_fft"], geo["mel"], geo["f_min"], geo["f_max"])).to(x.dtype)
    return torch.matmul(fb, mag)


def log_mel(x, geo, eps=EPS):
    m = mel(x, geo, eps)
    return torch.log(torch.clamp(m, min=geo["floor"])), m


def mel_loss(pred, target, geo, dtype=torch.float64):
    """-> (L_mel, the smallest mel of the prediction, the smallest mel of the target), the mels before the floor"""
    mp, lin_p = log_mel(pred.to(dtype), geo)
    mt, lin_t = log_mel(target.to(dtype), geo)
    return (mt - mp).abs().mean(), float(lin_p.detach().min()), float(lin_t.detach().min())


def loss_and_grad(pred, target, geo, dtype=torch.float64):
    """-> {'L' [1], 'dpred' [B, T], 'low_pred', 'low_target' (the smallest mel of each signal)} by autograd of `mel_loss`"""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    L, low_p, low_t = mel_loss(p, target.detach(), geo, dtype)
    L.backward()
    return {"L": L.detach().reshape(1), "dpred": p.grad.detach(), "low_pred": low_p, "low_target": low_t}
