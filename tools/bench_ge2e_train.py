"""One training step of the GE2E speaker encoder (forward + GE2E loss + backward; csrc/ge2e_train_ops.hip through `speaker_encoder.GE2E(trainable=True).embed`
and `GE2ELoss`) on one MI355X at the trainer's default batch - 64 speakers x 10 utterances x 160 frames of 80 mel bins, 3 LSTM layers, 256-dimensional
embeddings - at H = 256 (the shipped width) and H = 768 (the widest supported).  The REFERENCE FOR TIME is the same weights in torch.nn.LSTM + torch.nn.Linear
(the vendor library's RNN) with the loss in torch ops and autograd, on the same device and input.  The two paths alternate call by call in one process so that
a drifting clock meets both; median of `--iters` (>= 20) steps each, every step a host clock around work that ends in a device synchronise; the largest
relative difference of the loss and of each gradient between the two paths is recorded with the times.
Usage: python tools/bench_ge2e_train.py [--iters 20] [--out profiles/bench_ge2e_train.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402

S, M, T, MEL, STACKS, E = 64, 10, 160, 80, 3, 256


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def torch_loss(e, w):
    """The GE2E softmax loss of speaker_encoder.GE2ELoss in torch ops (e [S M, E], speaker-major)"""
    N = S * M
    u = torch.nn.functional.normalize(e, dim=1, eps=1e-12)
    U = u.reshape(S, M, -1)
    sums = U.sum(1)
    cent, excl = sums / M, (sums[:, None, :] - U) / (M - 1)
    cos = (u @ cent.t()) / cent.norm(dim=1).clamp_min(1e-12)[None, :]
    own = torch.arange(N, device=e.device) // M
    mask = torch.zeros(N, S, dtype=torch.bool, device=e.device)
    mask[torch.arange(N, device=e.device), own] = True
    cos_own = ((U * excl).sum(-1) / excl.norm(dim=-1).clamp_min(1e-12)).reshape(N)
    scores = w * torch.where(mask, cos_own[:, None].expand(N, S), cos)
    return (torch.logsumexp(scores, 1) - scores[torch.arange(N, device=e.device), own]).mean()


def one_width(H, warmup, iters):
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.speaker_encoder import GE2E, GE2ELoss
    d = load_yaml(DEFAULT_YAML)
    d["Speaker_Embedding"]["GE2E"]["LSTM"] = {"Sizes": H, "Stacks": STACKS}
    torch.manual_seed(1234)
    enc = GE2E(Recursive_Parse(d), "cuda:0", trainable=True)
    crit = GE2ELoss().cuda()
    lstm = torch.nn.LSTM(MEL, H, STACKS, batch_first=True).cuda()
    linear = torch.nn.Linear(H, E).cuda()
    lstm.load_state_dict(enc.lstm.state_dict())
    linear.load_state_dict(enc.linear.state_dict())
    w = torch.tensor(10.0, device="cuda", requires_grad=True)
    x = (torch.rand(S * M, MEL, T, generator=torch.Generator().manual_seed(5)) * 8.0 - 4.0).cuda()
    xt = x.transpose(1, 2).contiguous()
    hip_params = list(enc.parameters()) + [crit.w]
    base_params = list(lstm.parameters()) + list(linear.parameters()) + [w]

    def hip():
        for p in hip_params:
            p.grad = None
        loss = crit(enc.embed(x), S, M)
        loss.backward()
        return loss

    def base():
        for p in base_params:
            p.grad = None
        top, _ = lstm(xt)
        loss = torch_loss(linear(top[:, -1]), w)
        loss.backward()
        return loss

    lh, lb = float(hip()), float(base())
    names = [n for n, _ in enc.named_parameters()] + ["w"]
    diffs = {n: float((a.grad - b.grad).abs().max() / b.grad.abs().max()) for n, a, b in zip(names, hip_params, base_params)}
    for _ in range(warmup):
        hip()
        base()
    torch.cuda.synchronize()
    th, tb = [], []
    for _ in range(iters):                                     # call by call, alternating
        th.append(timed(hip))
        tb.append(timed(base))
    h, b = stats(th), stats(tb)
    return {"H": H, "speakers": S, "utterances": M, "frames": T, "mel": MEL, "stacks": STACKS, "E": E, "launches_per_step": 2 * (T + STACKS - 1) + 2 * STACKS + 8,
            "loss_hip": lh, "loss_torch": lb, "max_relative_gradient_difference_hip_vs_torch": max(diffs.values()), "hip": h, "torch_lstm_linear_autograd": b,
            "speedup_hip_over_torch": round(b["ms_median"] / h["ms_median"], 3), "hip_faster": bool(h["ms_median"] < b["ms_median"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_ge2e_train.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed steps"
    assert torch.cuda.is_available(), "bench_ge2e_train.py measures on the GPU"
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup,
           "step": [one_width(H, args.warmup, args.iters) for H in (256, 768)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
