"""The dropout keep masks the HIP kernels draw, restated on the host with numpy uint32 arithmetic (a plain helper module, no tests).

None of these masks is ever written to memory by the library: every kernel that needs one re-derives it from (seed, element id), and the
backward kernels re-derive it again (or recover it from `output != 0`).  A parity test restates the draw here and injects the result into
the oracle (oracle/glowtts_ref.py `drop=` hooks), whose forward and torch.autograd backward then see the same network.

  linear_keep / attention_keep   `drop_scale` of csrc/device_common.h (the one definition every site calls): the text encoder's sites
  hip_keep_multipliers           `drop_rowkey` / `drop_colkey` / `drop_draw` of csrc/device_common.h: the WaveNet gate pre-activations
"""
import numpy as np
import torch

ROW_PAD = 2


def _u32(v):
    return np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF)


def drop_scale(seed, ids, p):
    """`drop_scale(seed, id, p, 1 / (1 - p))`: murmur3 finalizer of id * 0x9E3779B1 + seed, 24-bit uniform >= p keeps.  ids: integer array (taken
    mod 2^32 like the kernels' uint32 casts) -> float32 array of {0, 1/(1-p)}; the comparison and the multiplier are float32 like the kernels'."""
    h = _u32(_u32(ids) * np.uint64(0x9E3779B1) + np.uint64(int(seed) & 0xFFFFFFFF))
    h ^= h >> np.uint64(16)
    h = _u32(h * np.uint64(0x85EBCA6B))
    h ^= h >> np.uint64(13)
    h = _u32(h * np.uint64(0xC2B2AE35))
    h ^= h >> np.uint64(16)
    u = (h >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    ik = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(u >= np.float32(p), ik, np.float32(0.0)).astype(np.float32)


def site_seed(seed, seed_word):
    """(site seed + the step's device seed word) mod 2^32: what every kernel computes as `seed += *seed_ptr`."""
    return (int(seed) + int(seed_word)) & 0xFFFFFFFF


def linear_keep(seed, rows, cols, p):
    """Keep multipliers [rows, cols] of an elementwise site on a rows tensor: element id = row * cols + col.  `seed`: see `site_seed`."""
    ids = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(cols) + np.arange(cols, dtype=np.uint64)[None, :]
    return torch.from_numpy(drop_scale(seed, ids, p))


def attention_keep(seed, B, H, Tp, p):
    """Keep multipliers [B, H, Tp, Tp] of the attention probabilities: element id = ((b * H + h) * Tp + i) * Tp + j over the PADDED length."""
    ids = np.arange(B * H * Tp * Tp, dtype=np.uint64).reshape(B, H, Tp, Tp)
    return torch.from_numpy(drop_scale(seed, ids, p))


def rows_to_bct(m, B, T):
    """[B * (T + 4), C] keep multipliers on the rows layout -> [B, C, T] (channel-first, pad rows dropped)."""
    return m.view(B, T + 2 * ROW_PAD, -1)[:, ROW_PAD:ROW_PAD + T].transpose(1, 2).contiguous()


def attention_to_bhtt(m, T):
    """[B, H, Tp, Tp] -> [B, H, T, T]: the tokens of the padded square."""
    return m[:, :, ROW_PAD:ROW_PAD + T, ROW_PAD:ROW_PAD + T].contiguous()


def hip_keep_multipliers(seed_word, flow, layer, B, T, H, p):
    """The WaveNet dropout multipliers the HIP epilogues draw (csrc/device_common.h: drop_rowkey / drop_colkey / drop_draw), restated with
    numpy uint32 arithmetic: [B, 2H, T] for gate pre-activation channel (tanh j | sigmoid H + j) of squeezed frame t of utterance b.
    Row index = position in the rows layout [B][T + 4] (two pad rows in front of every utterance)."""
    u = lambda v: np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF
    thr = int(p * 65536.0 + 0.5)
    ik = np.float32(65536.0) / np.float32(65536.0 - thr)
    seed = (1000003 * flow + int(seed_word) + layer) & 0xFFFFFFFF
    rows = (np.arange(B)[:, None] * (T + 4) + 2 + np.arange(T)[None, :]).astype(np.uint64)            # [B, T]
    x = u(rows * 0x9E3779B1 + seed)
    x ^= x >> 16
    x = u(x * 0x85EBCA6B)
    x ^= x >> 13
    ck = u((np.arange(H, dtype=np.uint64) + 1) * 0x27D4EB2F)                                          # [H]
    d = u((x[:, None, :] ^ ck[None, :, None]) * 0xC2B2AE35)                                           # [B, H, T]
    d ^= d >> 16
    keep_t, keep_s = (d & 0xFFFF) >= thr, (d >> 16) >= thr
    m = np.concatenate([keep_t, keep_s], 1).astype(np.float32) * ik
    return torch.from_numpy(m)


# ---- the text encoder's sites: names, rates, and the oracle hook that injects the restated masks
def site_rate(hp_encoder, site):
    """The dropout rate of a site from the hyper-parameters, by the site's name (never from the library's log)."""
    if site.startswith("Prenet.CLRD_"):
        return float(hp_encoder.Prenet.Dropout_Rate)
    if site.startswith("ANCRDCN_"):
        return float(hp_encoder.Transformer.Dropout_Rate)
    if site.startswith("CRND_"):
        return float(hp_encoder.Duration_Predictor.Dropout_Rate)
    raise KeyError(site)


class EncoderMasks:
    """Oracle `drop` hook for the text encoder that applies the masks the HIP path drew: seeds from the library's `encoder.DROP_LOG` (the seed
    ONLY), rates from the hyper-parameters by site name, shapes from the oracle's own tensors.  After the oracle ran, `check_log` asserts that the
    library logged exactly the sites the oracle called, with the kinds, rates and shapes derived here."""

    def __init__(self, log, hp_encoder, seed_word, B, T):
        self.log = list(log)
        self.seeds = {}
        for name, kind, seed, p, shape in self.log:
            assert name not in self.seeds, f"site {name} logged twice"
            self.seeds[name] = int(seed)
        self.hp, self.word, self.B, self.T = hp_encoder, int(seed_word), B, T
        self.masks = {}
        self.called = []

    def keep(self, site, shape):
        p = site_rate(self.hp, site)
        seed = site_seed(self.seeds[site], self.word)
        Tp = self.T + 2 * ROW_PAD
        if site.endswith(".Attention"):
            B, H, T, _ = shape
            full = attention_keep(seed, B, H, Tp, p)
            return full, attention_to_bhtt(full, T), ("attention", p, (B, H, Tp, Tp))
        B, C, T = shape
        full = linear_keep(seed, B * Tp, C, p)
        return full, rows_to_bct(full, B, T), ("linear", p, (B * Tp, C))

    def __call__(self, site, x):
        assert site in self.seeds, f"the oracle drops at {site}, the library logged no such site: {sorted(self.seeds)}"
        assert site not in self.masks, site
        full, m, meta = self.keep(site, tuple(x.shape))
        self.masks[site] = (full, meta)
        self.called.append(site)
        return x * m.to(x.dtype)

    def check_log(self):
        assert sorted(self.called) == sorted(self.seeds), (sorted(self.called), sorted(self.seeds))
        for name, kind, seed, p, shape in self.log:
            k, p_want, shape_want = self.masks[name][1]
            assert kind == k and abs(float(p) - p_want) < 1e-12 and tuple(shape) == shape_want, (name, kind, p, shape, k, p_want, shape_want)
        seeds = [s for s in self.seeds.values()]
        assert len(set(seeds)) == len(seeds), "two dropout sites share a stream"
