"""What an embedding map (`projection.tsne`: exact t-SNE, csrc/tsne_ops.hip) costs on one MI355X against what a user has without it.
N = 5000 (the reference's 50 speakers x 100 patterns) and N = 1000 vectors of D = the default Prosody_Encoder.Size, 50 Gaussian clusters, perplexity 30,
1000 iterations of which 250 are exaggerated, learning rate 200.
  * hip         `projection.tsne`: 3 + 2 x 1000 + 2 launches, one synchronisation at the end
  * torch       the same iteration in torch operations on the device, over the SAME matrix P (the affinities are not timed on this side): distances of y
                by the Gram form, w, Z, the two force sums as (row sum) y - (matrix) @ y, gains, momentum, update, recentring; the cost every 50th iteration
  * sklearn     `sklearn.manifold.TSNE` on the host at 16 threads, when it imports: `barnes_hut` (an approximation) at both sizes, `exact` at N = 1000 only;
                one fit each (--no-sklearn skips them)
hip and torch alternate in ONE process, the torch side as two interleaved series (A/A): host wall clock around call + synchronize, median of `--calls`
timed calls after `--warmup`; |median(a1) - median(a2)| is the noise of this very run.  `forces_us`: device events around 200 back-to-back `tsne_forces`
launches on the fitted map, per launch, next to the time 4 N^2 bytes take at 8 TB/s.  The maps differ (the iteration is chaotic in the last bits); each
side's final KL and nearest-neighbour agreement with the clusters say that they are maps of the same quality.
Usage: python tools/bench_tsne.py [--calls 5] [--warmup 1] [--no-sklearn] [--out profiles/bench_tsne.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_sampling import interleaved, wall_ms  # noqa: E402

PERPLEXITY, ITERATIONS, EXAGGERATED, LR, CLUSTERS = 30.0, 1000, 250, 200.0, 50


def default_size():
    import yaml
    with open(os.path.join(REPO, "glow_tts_amd", "Hyper_Parameters.default.yaml")) as f:
        return int(yaml.safe_load(f)["Prosody_Encoder"]["Size"])


def vectors(N, D):
    rng = np.random.default_rng(N)
    centres = rng.normal(size=(CLUSTERS, D)) * 2.0
    labels = np.arange(N) % CLUSTERS
    return (centres[labels] + rng.normal(size=(N, D))).astype(np.float32), labels


def torch_fit(P, y0):
    """The iteration of DESIGN.md "Embedding maps" in torch operations -> y, the KL series"""
    N = P.shape[0]
    y, u, gain = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
    off = ~torch.eye(N, dtype=torch.bool, device=P.device)
    logP = torch.where(P > 0, P, torch.ones_like(P)).log()
    kl = []

    def weights(y):
        sq = (y * y).sum(1)
        w = 1.0 / (1.0 + (sq[:, None] + sq[None, :] - 2.0 * (y @ y.t())).clamp_(min=0))
        return w * off

    def cost(w):
        return (P * (logP - torch.where(off, w, torch.ones_like(w)).log())).sum() + w.sum().log() * P.sum()

    for t in range(ITERATIONS):
        w = weights(y)
        if t % 50 == 0:
            kl.append(cost(w))
        a, mu = (12.0, 0.5) if t < EXAGGERATED else (1.0, 0.8)
        pw, w2 = P * w, w * w
        g = 4.0 * (a * (pw.sum(1, keepdim=True) * y - pw @ y) - (w2.sum(1, keepdim=True) * y - w2 @ y) / w.sum())
        gain = torch.where(torch.sign(g) != torch.sign(u), gain + 0.2, gain * 0.8).clamp_(min=0.01)
        u = mu * u - LR * gain * g
        y = y + u
        y = y - y.mean(0, keepdim=True)
    kl.append(cost(weights(y)))
    return y, torch.stack(kl)


def case(N, D, args):
    from glow_tts_amd import _lib, projection
    dev = torch.device("cuda:0")
    x_host, labels = vectors(N, D)
    x, y0 = torch.from_numpy(x_host).to(dev), projection.initial_map(N, 0)
    fit = projection.Fit(x, PERPLEXITY)
    P = fit.matrix().contiguous()
    y0d = y0.to(dev)
    hip = lambda: projection.tsne(x, PERPLEXITY, ITERATIONS, EXAGGERATED, LR, y0=y0)
    tor = lambda: torch_fit(P, y0d)
    affinities = lambda: projection.Fit(x, PERPLEXITY)
    r = {"N": N, "D": D, "iterations": ITERATIONS}
    res, (yt, klt) = hip(), tor()
    lab = labels.tolist()
    r["final_kl"] = {"hip": round(res.kl[-1], 4), "torch": round(float(klt[-1]), 4)}
    r["nearest_neighbour_agreement"] = {"vectors": projection.nearest_neighbour_agreement(x, lab), "hip": projection.nearest_neighbour_agreement(res.y, lab),
                                        "torch": projection.nearest_neighbour_agreement(yt.contiguous(), lab)}
    t = interleaved({"torch_a1": tor, "hip": hip, "torch_a2": tor, "hip_affinities": affinities}, args.calls, args.warmup, wall_ms)
    a1, h, a2, aff = (statistics.median(t[k]) for k in ("torch_a1", "hip", "torch_a2", "hip_affinities"))
    both = statistics.median(t["torch_a1"] + t["torch_a2"])
    r["call_ms"] = {"torch_a1": round(a1, 3), "torch_a2": round(a2, 3), "torch_loop": round(both, 3), "hip_fit": round(h, 3), "hip_affinities": round(aff, 3),
                    "hip_loop": round(h - aff, 3), "aa_spread": round(abs(a1 - a2), 3), "torch_loop_over_hip_loop": round(both / (h - aff), 3)}
    # tsne_forces alone, on the fitted map
    fit.start(res.y.cpu())
    L, ld = _lib.api(), projection.pitch(N)
    sums, shares = torch.empty(N, 4, device=dev), torch.empty(N, 4, dtype=torch.float64, device=dev)
    launch = lambda: L.glowtts_tsne_forces(_lib.ptr(fit.work), _lib.ptr(fit.y), _lib.ptr(sums), _lib.ptr(shares), N, 0, _lib.stream())
    for _ in range(20):
        launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        launch()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / 200
    floor = 4.0 * N * ld / 8e12 * 1e6
    r["forces_us"] = {"per_launch": round(us, 2), "floor_4NN_bytes_at_8TBps": round(floor, 2), "bytes_per_s": round(4.0 * N * ld / (us * 1e-6) / 1e12, 3),
                      "P_MiB": round(4.0 * N * ld / 2 ** 20, 1)}
    if not args.no_sklearn:
        try:
            from sklearn.manifold import TSNE
        except ImportError:
            TSNE = None
        if TSNE is not None:
            sk = {}
            for method in ("barnes_hut",) + (("exact",) if N <= 1000 else ()):
                t0 = time.perf_counter()
                m = TSNE(n_components=2, perplexity=PERPLEXITY, early_exaggeration=12.0, learning_rate=LR, max_iter=ITERATIONS, init="random", method=method,
                         random_state=0, n_jobs=16).fit(x_host)
                sk[method] = {"fit_s": round(time.perf_counter() - t0, 2), "final_kl": round(float(m.kl_divergence_), 4),
                              "nearest_neighbour_agreement": projection.nearest_neighbour_agreement(torch.from_numpy(m.embedding_.astype(np.float32)).to(dev), lab)}
            r["sklearn_host_16_threads"] = sk
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_tsne.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsne.py measures on the GPU"
    torch.set_num_threads(16)
    D = default_size()
    rows = [case(N, D, args) for N in (5000, 1000)]
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup, "perplexity": PERPLEXITY, "rows": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
