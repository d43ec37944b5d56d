"""The mel-spectrogram L1 loss (csrc/mel_loss_ops.hip through `vocoder.MelSpectrogramLoss`) on one MI355X: forward plus backward of the loss ALONE, at
the trainers' default shapes - 16 x 8192 samples (Train_HiFiGAN.py) and 8 x 25600 (Train_PWG.py) - and the analysis geometry of the default `Sound` block
((2048, 256, 1024) x 80 filters at 24 kHz).
  * ms per forward + backward of the HIP path; a timed call is `--inner` of them behind one synchronise, so that the window is not the launch latency alone;
  * the BASELINE: the same loss on `torch.stft` plus a dense filterbank matmul under autograd, float32 on the same device and inputs.  Three series
    ALTERNATE call by call - HIP, torch, torch again - so that a drifting clock meets all; medians of `--iters` (>= 20) each; the two torch series give the
    A/A spread a difference has to exceed;
  * the two losses and the largest difference of d pred relative to its largest element;
  * the HBM bytes a frame needs at the least (each sample and each kept value once) against the time: the distance to the bandwidth floor at 8 TB/s;
  * the loss's share of a stage-one `Train_Step` of each trainer at its defaults: the step with and without the block `Vocoder.Train.Mel_Loss`, alternating.
Usage: python tools/bench_mel_loss.py [--iters 20] [--inner 10] [--out profiles/bench_mel_loss.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tools"))
import torch  # noqa: E402

from bench_hifigan_train import write_corpus  # noqa: E402

SHAPES = {"hifigan": (16, 8192), "pwg": (8, 25600)}
HBM_TBS = 8.0
EPS = 1e-9


def torch_mel_loss(pred, target, geo, window, fb):
    ms = []
    for x in (pred, target):
        X = torch.stft(x, geo["n_fft"], geo["hop"], geo["n_fft"], window, center=True, pad_mode="reflect", return_complex=True)
        ms.append(torch.log(torch.clamp(torch.matmul(fb, torch.sqrt(X.real ** 2 + X.imag ** 2 + EPS)), min=geo["floor"])))
    return (ms[1] - ms[0]).abs().mean()


def timed(fn, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def series(fns, warmup, iters, inner=1):
    """The medians (and every series) of the callables `fns`, timed alternating call by call"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(iters):
        for ts, fn in zip(out, fns):
            ts.append(timed(fn, inner))
    return [statistics.median(ts) for ts in out], out


def frame_bytes(geo):
    """HBM bytes per frame at the least: forward reads hop new samples of each signal and writes Mel coefficients and one float64; backward reads hop samples
    and the coefficients and writes win frame gradients; the fold reads them and writes hop samples"""
    fwd = 2 * geo["hop"] * 4 + geo["mel"] * 4 + 8
    bwd = geo["hop"] * 4 + geo["mel"] * 4 + geo["win"] * 4
    fold = geo["win"] * 4 + geo["hop"] * 4
    return {"forward": fwd, "backward_frames": bwd, "backward_fold": fold, "total": fwd + bwd + fold}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_mel_loss.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_mel_loss.py measures on the GPU"
    from glow_tts_amd import audio, vocoder as V
    from glow_tts_amd.hifigan_trainer import HiFiGAN_Trainer
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.pwg_trainer import PWG_Trainer
    base = load_yaml(DEFAULT_YAML)
    hp = Recursive_Parse(copy.deepcopy(base))
    crit = V.MelSpectrogramLoss(hp, "cuda:0")
    geo, dev = crit.geo, crit.device
    window = torch.nn.functional.pad(crit.window, ((geo["n_fft"] - geo["win"]) // 2, geo["n_fft"] - geo["win"] - (geo["n_fft"] - geo["win"]) // 2))
    fb = torch.from_numpy(audio.mel_filterbank(geo["sample_rate"], geo["n_fft"], geo["mel"], geo["f_min"], geo["f_max"])).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "inner_calls_per_timed_call": args.inner, "geometry": geo,
           "kept_bytes_per_frame": {"coefficients (chosen)": geo["mel"] * 4, "spectrum and magnitude as the STFT loss keeps them": (geo["n_fft"] // 2 + 1) * 12},
           "hbm_bytes_per_frame": frame_bytes(geo), "hbm_tb_per_s": HBM_TBS, "loss_alone": {}, "train_step": {}}
    for name, (B, T) in SHAPES.items():
        g = torch.Generator().manual_seed(7)
        pred, target = ((torch.randn(B, T, generator=g) * 0.3).to(dev) for _ in range(2))
        p_hip, p_ref = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)

        def hip():
            p_hip.grad = None
            loss = crit(p_hip, target)
            loss.backward()
            return loss.detach()

        def ref():
            p_ref.grad = None
            loss = torch_mel_loss(p_ref, target, geo, window, fb)
            loss.backward()
            return loss.detach()

        l_hip, l_ref = hip(), ref()
        diff = float((p_hip.grad - p_ref.grad).abs().max() / p_ref.grad.abs().max())
        (m_hip, m_ref, m_ref2), (t_hip, t_ref, t_ref2) = series((hip, ref, ref), args.warmup, args.iters, args.inner)
        frames = B * (1 + T // geo["hop"])
        floor_us = frames * frame_bytes(geo)["total"] / (HBM_TBS * 1e12) * 1e6
        out["loss_alone"][name] = {
            "B": B, "T": T, "frames": frames, "loss_hip": float(l_hip), "loss_torch": float(l_ref), "dpred_max_diff_rel": diff,
            "hip_ms": round(m_hip, 4), "hip_ms_min_max": [round(min(t_hip), 4), round(max(t_hip), 4)],
            "torch_ms": round(m_ref, 4), "torch_ms_min_max": [round(min(t_ref), 4), round(max(t_ref), 4)],
            "torch_ms_second_series": round(m_ref2, 4), "torch_aa_spread_rel": round(abs(m_ref - m_ref2) / m_ref, 4),
            "speedup_hip_over_torch": round(m_ref / m_hip, 2), "hip_faster": bool(m_hip < m_ref),
            "hbm_bytes": frames * frame_bytes(geo)["total"], "bandwidth_floor_us": round(floor_us, 3), "hip_time_over_bandwidth_floor": round(m_hip * 1e3 / floor_us, 1)}

    # the share of a stage-one Train_Step, each trainer at its defaults on a synthetic pattern directory
    for name, Trainer, block, frames in (("hifigan", HiFiGAN_Trainer, V.HIFIGAN_DEFAULTS, 32), ("pwg", PWG_Trainer, V.PWG_DEFAULTS, 100)):
        with tempfile.TemporaryDirectory() as root:
            trainers = {}
            for key, train in (("without", {}), ("with", {"Mel_Loss": {}})):
                d = copy.deepcopy(base)
                d["Vocoder"] = dict(block, Train=dict(train, Checkpoint_Path=os.path.join(root, "ckpt")))
                d["Train"]["Train_Pattern"].update(Path=root, Metadata_File="METADATA.PICKLE")
                d["Train"]["Eval_Pattern"].update(Path="", Metadata_File="METADATA.PICKLE")
                if not trainers:
                    write_corpus(root, d["Sound"]["Mel_Dim"], d["Sound"]["Frame_Shift"], frames)
                trainers[key] = Trainer(hp=Recursive_Parse(d), seed=0)
            batch = tuple(t.to(dev).contiguous() for t in trainers["with"].sampler["Train"].batch(0))
        assert tuple(batch[1].shape) == SHAPES[name], batch[1].shape
        steps = [lambda tr=trainers[k]: tr.Train_Step(*batch) for k in ("without", "with", "without")]
        (m_without, m_with, m_without2), (t_without, t_with, _) = series(steps, args.warmup, args.iters)
        out["train_step"][name] = {
            "batch": list(batch[1].shape), "ms_without_block": round(m_without, 3), "ms_with_block": round(m_with, 3),
            "ms_min_max_without": [round(min(t_without), 3), round(max(t_without), 3)], "ms_min_max_with": [round(min(t_with), 3), round(max(t_with), 3)],
            "ms_without_block_second_series": round(m_without2, 3), "aa_spread_rel": round(abs(m_without - m_without2) / m_without, 4),
            "mel_loss_ms": round(m_with - m_without, 3), "mel_loss_share_of_step": round((m_with - m_without) / m_with, 4),
            "mel_loss": float(trainers["with"].last["Mel_Loss"])}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
