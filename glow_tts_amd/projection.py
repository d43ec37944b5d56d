"""Embedding maps: exact t-SNE of a set of vectors into two dimensions, on the device (Prosody_Visualization.py, Trainer.Prosody_Check_Epoch).

    x [N, D] --tsne_sqdist, tsne_affinity, tsne_symmetrize (once)--> P [N, N] --(tsne_forces, tsne_step) x iterations, tsne_forces,kl + tsne_step,finish--> y [N, 2]

The contract is DESIGN.md "Embedding maps"; the kernels are csrc/tsne_ops.hip.  All N^2 pairs enter every iteration: no tree, no approximation, no float atomics,
so a map is bit-identical from run to run.  Nothing of torch runs inside the loop and the host does not wait before its end.  Barnes-Hut / FFT-accelerated
variants, more than two output dimensions, a PCA start, UMAP, N > 8192 and bf16 are out of scope."""
import torch

from . import _lib, abi
from .hparams import overlay_settings

KL_EVERY = 50
DEFAULTS = {"Perplexity": 30.0, "Iterations": 1000, "Exaggeration_Iterations": 250, "Learning_Rate": 200.0}


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def projection_settings(hp):
    """The optional yaml block `Projection` over its defaults; an unknown key or a bad value raises a ValueError naming the key."""
    s = overlay_settings(getattr(hp, "Projection", None), DEFAULTS, "Projection", "projection", lambda s, need: None)
    if not _number(s["Perplexity"]) or not s["Perplexity"] >= 1:
        raise ValueError("Projection.Perplexity = {!r} (a number >= 1, and <= (N - 1) / 3 for the N vectors mapped)".format(s["Perplexity"]))
    for k in ("Iterations", "Exaggeration_Iterations"):
        if not isinstance(s[k], int) or isinstance(s[k], bool) or s[k] < (1 if k == "Iterations" else 0):
            raise ValueError("Projection.{} = {!r} (an integer >= {})".format(k, s[k], 1 if k == "Iterations" else 0))
    if not _number(s["Learning_Rate"]) or not s["Learning_Rate"] > 0:
        raise ValueError("Projection.Learning_Rate = {!r} (a number > 0)".format(s["Learning_Rate"]))
    return s


def pitch(n):
    """floats per row of the fit's N x N matrix (rows are 16-byte aligned)"""
    return (n + 3) & ~3


def _points(name, x):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _lib.GlowTTSHipError("{}: expected a device tensor (the HIP path has no CPU fallback)".format(name))
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("{}: expected fp32 [N, D], got {} {}".format(name, x.dtype, list(x.shape)))
    N, D = x.shape
    if N < 8 or N > abi.TSNE_MAX_N:
        raise ValueError("{}: N = {} vectors, supported are 8 .. {}".format(name, N, abi.TSNE_MAX_N))
    if D < 1 or D > abi.TSNE_MAX_D:
        raise ValueError("{}: D = {} features, supported are 1 .. {}".format(name, D, abi.TSNE_MAX_D))
    return x.contiguous(), N, D


def sqdist(x):
    """x [N, D] -> squared Euclidean distances [N, N] by direct differences (`tsne_sqdist`): two identical rows are exactly 0 apart."""
    x, N, D = _points("sqdist: x", x)
    d2 = torch.empty(N, N, dtype=torch.float32, device=x.device)
    _lib.api().glowtts_tsne_sqdist(_lib.ptr(x), _lib.ptr(d2), N, D, N, _lib.stream())
    return d2


def _check_perplexity(perplexity, N, key="perplexity"):
    if not _number(perplexity) or not 1 <= perplexity <= (N - 1) / 3:
        raise ValueError("{} = {!r}: supported is 1 <= {} <= (N - 1) / 3 = {:.4g} at N = {}".format(key, perplexity, key, (N - 1) / 3, N))


class Fit:
    """The device state of one fit: the workspace (P at its start), y, u, gain [N, 2] and the KL slots."""

    def __init__(self, x, perplexity, joint=True, perplexity_key="perplexity"):
        x, self.N, self.D = _points("tsne: x", x)
        _check_perplexity(perplexity, self.N, perplexity_key)
        L = _lib.api()
        self.work = torch.empty(int(L.glowtts_tsne_work_bytes(self.N)), dtype=torch.uint8, device=x.device)
        L.glowtts_tsne_affinities(_lib.ptr(x), _lib.ptr(self.work), self.N, self.D, float(perplexity), 1 if joint else 0, _lib.stream())
        self.device = x.device

    def matrix(self):
        """[N, N] view of the workspace's matrix (P, or the conditional rows of joint=False)"""
        ld = pitch(self.N)
        return self.work[:self.N * ld * 4].view(torch.float32).view(self.N, ld)[:, :self.N]

    def start(self, y0):
        y0 = torch.as_tensor(y0, dtype=torch.float32)
        if tuple(y0.shape) != (self.N, 2):
            raise ValueError("tsne: y0 must be [N, 2] = [{}, 2], got {}".format(self.N, list(y0.shape)))
        self.y = y0.to(self.device).contiguous().clone()
        self.u, self.gain = torch.zeros_like(self.y), torch.ones_like(self.y)
        return self

    def iterate(self, t0, t1, exaggeration_iterations, learning_rate, kl_every=0, kl_final=False):
        """iterations [t0, t1) in place -> the KL slots (float64, on the device; None when nothing is measured)"""
        slots = ((t1 + kl_every - 1) // kl_every if kl_every > 0 else 0) + (1 if kl_final else 0)
        kl = torch.full((slots,), float("nan"), dtype=torch.float64, device=self.device) if slots else None
        _lib.api().glowtts_tsne_iterate(_lib.ptr(self.work), _lib.ptr(self.y), _lib.ptr(self.u), _lib.ptr(self.gain), _lib.ptr(kl), self.N, int(t0), int(t1),
                                        int(exaggeration_iterations), float(learning_rate), int(kl_every), 1 if kl_final else 0, _lib.stream())
        return kl


class TSNEResult:
    """y [N, 2] fp32 on the device (zero mean); kl: the Kullback-Leibler divergences (floats) at `kl_iterations` - iteration 0, every 50th, and the number of
    iterations for the final y."""
    __slots__ = ("y", "kl", "kl_iterations")

    def __init__(self, y, kl, kl_iterations):
        self.y, self.kl, self.kl_iterations = y, kl, kl_iterations


def initial_map(n, seed=0):
    """The default start: 1e-4 randn [N, 2] from a CPU generator seeded with `seed`"""
    return 1e-4 * torch.randn(n, 2, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)


def tsne(x, perplexity=30.0, iterations=1000, exaggeration_iterations=250, learning_rate=200.0, seed=0, y0=None):
    """Exact t-SNE of x [N, D] (fp32, on the device) into two dimensions -> TSNEResult.  3 + 2 `iterations` + 2 launches, one host synchronisation (reading the KL
    series) at the end."""
    if not isinstance(iterations, int) or iterations < 1:
        raise ValueError("iterations = {!r} (an integer >= 1)".format(iterations))
    if not isinstance(exaggeration_iterations, int) or exaggeration_iterations < 0:
        raise ValueError("exaggeration_iterations = {!r} (an integer >= 0)".format(exaggeration_iterations))
    if not _number(learning_rate) or not learning_rate > 0:
        raise ValueError("learning_rate = {!r} (a number > 0)".format(learning_rate))
    fit = Fit(x, perplexity)
    fit.start(initial_map(fit.N, seed) if y0 is None else y0)
    kl = fit.iterate(0, iterations, exaggeration_iterations, learning_rate, KL_EVERY, True)
    return TSNEResult(fit.y, kl.cpu().tolist(), list(range(0, iterations, KL_EVERY)) + [iterations])


def nearest_neighbours(points):
    """points [N, D] on the device -> index [N] of each point's nearest other point (squared Euclidean by `tsne_sqdist`, ties to the lowest index)"""
    d2 = sqdist(points)
    d2.fill_diagonal_(float("inf"))
    n = d2.shape[0]
    index = torch.arange(n, device=d2.device).expand(n, n)
    return torch.where(d2 == d2.min(1, keepdim=True).values, index, torch.full_like(index, n)).min(1).values


def nearest_neighbour_agreement(points, labels):
    """The share of points whose nearest other point carries the same label.  points: [N, D] fp32 on the device; labels: N hashable values."""
    labels = list(labels)
    if len(labels) != points.shape[0]:
        raise ValueError("nearest_neighbour_agreement: {} points, {} labels".format(points.shape[0], len(labels)))
    ids = {v: i for i, v in enumerate(sorted(set(labels), key=str))}
    lab = torch.tensor([ids[v] for v in labels], device=points.device)
    return float((lab[nearest_neighbours(points)] == lab).double().mean().item())
