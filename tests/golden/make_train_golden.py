"""Generates tests/golden/tiny_train_*.npz: the UNMODIFIED reference (imported through _ref_harness.py) in train() mode, with the keep
masks of every torch.nn.Dropout call drawn from a seeded generator and recorded - the train-mode pin of the oracle's `drop` hooks
(oracle/glowtts_ref.py; replayed by tests/test_oracle_golden.py::test_model_oracle_matches_reference_in_train_mode).

Only runs in the build container (the reference never travels); never imported by a test.  The reference's files are not touched:
`torch.nn.Dropout.forward` is replaced at run time by a function that multiplies by `mask / (1 - p)`.  The state of the model is the one
of tiny_*.npz (make_golden.py), so the new fixtures hold no state dict: masks (np.packbits), the eight outputs, the two losses and
every parameter gradient.  Usage:  python tests/golden/make_train_golden.py
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
warnings.filterwarnings("ignore")

from _ref_harness import load_reference  # noqa: E402
from make_golden import TINY  # noqa: E402
from helpers import load_case  # noqa: E402


def make_train_case(mode, seed, src, fname):
    M = load_reference(dict(TINY, Mode=mode, **{"Speaker_Embedding.Type": "LUT"}))
    sd, _, r = load_case(src)
    model = M.GlowTTS()
    model.load_state_dict(sd)
    for mod in model.modules():
        if hasattr(mod, "initialized"):
            mod.initialized = True                       # ActNorm: the stored logs / bias ARE the initialised ones (Modules.py:685-687)
    model.train()
    names = {id(mod): name for name, mod in model.named_modules()}
    gen = torch.Generator().manual_seed(seed)
    calls, record = {}, {}

    def forward(self, x):
        name = names[id(self)]
        i = calls.get(name, 0)
        calls[name] = i + 1
        mask = torch.rand(x.shape, generator=gen) >= self.p
        record[(name, i)] = (mask, float(self.p))
        return x * (mask.to(x.dtype) / (1.0 - self.p))

    t = lambda k: torch.from_numpy(r[k])
    speakers = t("speakers") if "speakers" in r else None
    pitches = t("pitches") if "pitches" in r else None
    mel_lengths = t("mel_lengths")
    old = torch.nn.Dropout.forward
    torch.nn.Dropout.forward = forward
    try:
        out = model(t("tokens"), t("token_lengths"), t("mels"), mel_lengths, speakers, None, pitches)
    finally:
        torch.nn.Dropout.forward = old
    z, mel_mean, mel_log_std, log_dets, log_dur, log_dur_t, attn, classified = out
    mle = M.MLE_Loss()(z=z, mean=mel_mean, std=mel_log_std, log_dets=log_dets, lengths=mel_lengths)
    length = torch.nn.MSELoss()(log_dur, log_dur_t)
    model.zero_grad()
    (mle + length).backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}

    data = dict(z=z.detach().numpy(), mel_mean=mel_mean.detach().numpy(), mel_log_std=mel_log_std.detach().numpy(),
                log_dets=log_dets.detach().numpy(), log_dur=log_dur.detach().numpy(), log_dur_target=log_dur_t.detach().numpy(),
                attn=attn.numpy().astype(np.int8), mle=mle.detach().numpy(), length=length.detach().numpy())
    if classified is not None:
        data["classified"] = classified.detach().numpy()
    for (name, i), (mask, p) in record.items():
        data[f"mask/{name}/{i}"] = np.packbits(mask.numpy().reshape(-1))
        data[f"shape/{name}/{i}"] = np.array(mask.shape, dtype=np.int32)
        data[f"p/{name}/{i}"] = np.float64(p)
    data.update({"grad/" + k: v.numpy() for k, v in grads.items()})
    np.savez_compressed(os.path.join(HERE, fname), **data)
    kept = np.mean([m.float().mean().item() for m, _ in record.values()])
    print(f"wrote {fname}: {os.path.getsize(os.path.join(HERE, fname)) / 1024:.0f} KiB ({os.path.getsize(os.path.join(HERE, src)) / 1024:.0f} KiB in {src}); "
          f"{len(record)} dropout calls, mean kept fraction {kept:.3f}, mle {mle.item():.5f}, length {length.item():.5f}")


if __name__ == "__main__":
    make_train_case("Vanilla", 20261, "tiny_vanilla.npz", "tiny_train_vanilla.npz")
    make_train_case("SE", 20262, "tiny_se.npz", "tiny_train_se.npz")
