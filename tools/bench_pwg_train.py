"""One training step of the Parallel WaveGAN generator (forward + multi-resolution STFT loss + backward; csrc/pwg_ops.hip, csrc/pwg_train_ops.hip,
csrc/stft_loss_ops.hip) on one MI355X at the defaults: B = 8 x 100 frames, 30 layers, 64 / 128 / 64 channels, 80 mel bins, hop 256.
  * ms per step of the HIP path (`ParallelWaveGAN(trainable=True).generate` -> `MultiResolutionSTFTLoss` -> backward; no optimizer);
  * the BASELINE: the same generator on torch.nn.functional convs (tools/bench_pwg.py `torch_generator`) under autograd plus `torch.stft` for the loss, on
    the same device, weights and noise; the two paths ALTERNATE call by call, so that a drifting clock meets both; median of `--iters` (>= 20) each;
  * the two losses and the largest relative difference of the parameter gradients (both paths are float32);
  * the layer launches of a step alone - 30 forward layers, and per layer the backward's gate, data and weight-gradient launches on the step's own
    buffers - against the 155 TF/s the exact-f32 MFMA sustains: 4 x the forward's 2 (K G + R (R + S)) FLOP per sample and layer (K = 3 R + A).
Usage: python tools/bench_pwg_train.py [--iters 20] [--out profiles/bench_pwg_train.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_pwg import PEAK_TFLOPS, random_weights, torch_generator  # noqa: E402

B, FRAMES = 8, 100
CLAMP = 1e-7


def torch_stft_loss(pred, target, resolutions):
    total = 0.0
    for n_fft, hop, win in resolutions:
        window = torch.hann_window(win, periodic=True, device=pred.device)
        mags = []
        for x in (pred, target):
            X = torch.stft(x, n_fft, hop, win, window, center=True, pad_mode="reflect", return_complex=True)
            mags.append(torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=CLAMP)))
        mx, my = mags
        total = total + torch.norm(my - mx, p="fro") / torch.norm(my, p="fro") + (torch.log(my) - torch.log(mx)).abs().mean()
    return total / len(resolutions)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_pwg_train.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_pwg_train.py measures on the GPU"
    from glow_tts_amd import vocoder as V
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    d = load_yaml(DEFAULT_YAML)
    d["Vocoder"] = dict(V.PWG_DEFAULTS)
    hp = Recursive_Parse(d)
    geo = V.pwg_geometry(hp)
    sd = random_weights(V.pwg_expected_shapes(geo), 1234)
    voc = V.ParallelWaveGAN(hp, "cuda:0", state_dict=sd, trainable=True)
    crit = V.MultiResolutionSTFTLoss(None, "cuda:0")
    dev, T = voc.device, FRAMES * geo["hop"]
    g = torch.Generator().manual_seed(5)
    mels = (torch.rand(B, geo["A"], FRAMES, generator=g) * 8.0 - 4.0).to(dev)
    z, target = torch.randn(B, T, generator=g).to(dev), (torch.randn(B, T, generator=g) * 0.3).to(dev)
    lengths = torch.full((B,), FRAMES, dtype=torch.int32, device=dev)
    w_base = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}

    def hip():
        for p in voc.params.values():
            p.grad = None
        loss = crit(voc.generate(mels, lengths, noises=z)[0], target)
        loss.backward()
        return loss.detach()

    def base():
        for p in w_base.values():
            p.grad = None
        loss = torch_stft_loss(torch_generator(w_base, geo, mels, z), target, crit.resolutions)
        loss.backward()
        return loss.detach()

    for _ in range(args.warmup):
        l_hip, l_base = hip(), base()
    torch.cuda.synchronize()
    diff = max(float((voc.params[k].grad - w_base[k].grad).abs().max() / w_base[k].grad.abs().max().clamp_min(1e-30)) for k in sd if w_base[k].grad is not None)
    th, tb = [], []
    for _ in range(args.iters):                                     # alternating call by call
        th.append(timed(hip)[0])
        tb.append(timed(base)[0])
    hip_ms, base_ms = statistics.median(th), statistics.median(tb)

    # the layer launches of a step alone, on the buffers of one forward
    lib, P, st = V._lib.api(), V._lib.ptr, V._lib.stream()
    R, G, S, A, hop, L = geo["R"], geo["G"], geo["S"], geo["A"], geo["hop"], FRAMES
    voc._build_images({k: p.detach() for k, p in voc.params.items()})
    fwd = V.pwg_train_forward(voc, mels, lengths, None, z)
    f = lambda *shape: torch.zeros(*shape, device=dev)
    gate, dpre, dc, dxp, dx, dsk = f(B, T, R), f(B, T, G), f(B, T, A), f(B, T, R), f(B, T, R), f(B, T, S)
    work = f(lib.glowtts_pwg_train_work_floats(B, L, hop, R, S, A))
    grads = {k: f(*shape) for k, shape in V.pwg_expected_shapes(geo).items()}

    def layers():
        for i, (lw, d_) in enumerate(zip(voc.layer_weights, geo["dilations"])):
            V.ops.pwg_layer(fwd["keep"][i], fwd["c"], *lw, fwd["keep"][i + 1], fwd["skips"], lengths, L, hop, d_, i > 0)
        for i in reversed(range(geo["layers"])):
            (w1, b1, _, _), (w2t, w1t, wauxt), d_, q = voc.layer_weights[i], voc.layer_weights_t[i], geo["dilations"][i], f"conv_layers.{i}."
            lib.glowtts_pwg_train_layer_bwd(P(fwd["keep"][i]), P(fwd["c"]), P(w1), P(b1), P(w2t), P(w1t), P(wauxt), P(dxp), P(dsk), P(gate), P(dpre), P(dx), P(dc),
                                            P(lengths), B, L, hop, R, S, A, d_, int(i == geo["layers"] - 1), st)
            lib.glowtts_pwg_train_layer_wgrad(P(fwd["keep"][i]), P(fwd["c"]), P(gate), P(dpre), P(dxp), P(dsk), P(lengths), P(work), P(grads[q + "conv.weight"]),
                                              P(grads[q + "conv.bias"]), P(grads[q + "conv1x1_aux.weight"]), P(grads[q + "conv1x1_out.weight"]),
                                              P(grads[q + "conv1x1_out.bias"]), P(grads[q + "conv1x1_skip.weight"]), P(grads[q + "conv1x1_skip.bias"]),
                                              B, L, hop, R, S, A, d_, st)

    for _ in range(2):
        layers()
    torch.cuda.synchronize()
    lay_ms = statistics.median([timed(layers)[0] for _ in range(args.iters)])
    flop = 4 * 2.0 * ((3 * R + A) * G + R * (R + S)) * geo["layers"] * B * T
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup, "B": B, "frames": FRAMES,
           "geometry": {k: geo[k] for k in ("layers", "stacks", "R", "G", "S", "A", "ctx", "scales", "hop")}, "stft_resolutions": crit.resolutions,
           "f32_mfma_peak_tflops": PEAK_TFLOPS, "loss_hip": float(l_hip), "loss_baseline": float(l_base), "parameter_gradient_max_diff_rel": diff,
           "hip": {"ms_per_step": round(hip_ms, 3), "ms_min_max": [round(min(th), 3), round(max(th), 3)]},
           "baseline_torch": {"ms_per_step": round(base_ms, 3), "ms_min_max": [round(min(tb), 3), round(max(tb), 3)]},
           "speedup_hip_over_baseline": round(base_ms / hip_ms, 2), "hip_faster": bool(hip_ms < base_ms),
           "layers": {"ms": round(lay_ms, 3), "tflop": round(flop / 1e12, 3), "tflops": round(flop / (lay_ms * 1e-3) / 1e12, 2),
                      "fraction_of_f32_mfma_peak": round(flop / (lay_ms * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
                      "floor_ms_at_peak": round(flop / (PEAK_TFLOPS * 1e12) * 1e3, 2)}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
