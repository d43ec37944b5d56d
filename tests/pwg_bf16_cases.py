"""The cases and the bars of the bf16 vocoder tests, shared by tests/test_pwg_bf16_cpu.py (which holds emu32 / emu32b themselves to the bars: the guard that
the bars are what reference arithmetic satisfies) and tests/test_gpu_pwg_bf16.py (which holds the kernel to them).  Inputs as in tests/test_gpu_pwg.py:
torch's default Conv initialisation under a fixed seed, mels uniform in [-4, 4], Gaussian rows.  Every reference is computed once per process and not
modified.

Notation: ref64 / ref32 the UNROUNDED restatement (tests/pwg_ref.py) in float64 / float32; emu64 the bf16 contract in float64 (tests/pwg_bf16_ref.py);
e32 = max |ref32 - ref64|, e_bf = max |emu64 - ref64|, scale = max |ref64|.

THE LAYER BAR, elementwise:  |got - emu64| <= (4 e32 + 1e-6 scale) + 2 * 2^-7 * max_k |rb(w2)[k, col]| |g64[k, t]|.  The first term is the project's f32 bar.
The second is derived: the fp32 pre-activation differs from the float64 one in its last bits, so a gate value next to a rounding midpoint of bf16 goes to the
neighbouring bf16 - one unit in the last place, at most 2^-7 |g| - and the term allows two such elements in the row's sum over k.

THE GENERATOR BARS (no closed bound for chained layers; both are multiples of e_bf, which is measured on reference arithmetic):
max |got - ref64| <= 1.5 e_bf  and  max |got - emu64| <= 0.75 e_bf.  When the bars were set, emu32 / emu32b gave 0.96 - 1.03 e_bf and 0 - 0.35 e_bf on the
default and narrow configurations with two weight seeds (margins 1.5 x and 2 x); on the cases below they give 0.96 - 1.11 e_bf and 0 - 0.36 e_bf
(tests/test_pwg_bf16_cpu.py prints them).  The second bar separates the contracted rounding points from any other bf16 scheme: an independent realisation of the rounding noise
lies about sqrt(2) e_bf away.  Guard: e_bf > 100 e32, otherwise the case tests nothing."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pwg_bf16_ref as E  # noqa: E402
import pwg_ref as P  # noqa: E402

ODD = dict(P.DEFAULT, layers=10, stacks=1, scales=[3, 5])                    # default widths, hop 15, dilations 1 .. 512
CFGS = {"default": P.DEFAULT, "narrow": P.NARROW, "odd": ODD, "thin": E.THIN, "wide": E.WIDE}
WEIGHT_SEED = 1234
RAGGED = [5, 2, 7]
LAYER_CASES = ([("default", (3, 1, 2), i) for i in (0, 1, 6, 9)] + [("odd", (7, 2, 5), i) for i in (0, 1, 6, 9)] +          # dilations 1, 2, 64, 512
               [(name, (7, 2, 5), i) for name in ("narrow", "thin", "wide") for i in (0, 1)])
GENERATOR_CASES = [("default", (3,)), ("default", tuple(RAGGED)), ("narrow", tuple(RAGGED))]
SEEDED_CASES = ["default", "narrow"]
SEEDED_LENGTHS, SEEDED_LABELS, SEEDED_RUN = (3, 2), ("A", "B"), 7
_SD, _LAYER, _GEN = {}, {}, {}


def sd_of(name):
    if name not in _SD:
        _SD[name] = P.random_state_dict(CFGS[name], WEIGHT_SEED)
    return _SD[name]


def noise_of(T, seed):
    return torch.randn(T, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------- one layer
def layer_case(name, lengths, layer):
    """The rows of every utterance ([T_b, channels], as the kernel takes them) and, for utterance 0, per output ("x", "skips"): emu64, emu32, emu32b and the
    elementwise bar, all [channels, T]."""
    key = (name, lengths, layer)
    if key in _LAYER:
        return _LAYER[key]
    cfg, sd = CFGS[name], sd_of(name)
    hop, R, S, A = P.hop(cfg), cfg["R"], cfg["S"], cfg["A"]
    g = torch.Generator().manual_seed(300 + layer)
    xs = [torch.randn(L * hop, R, generator=g) for L in lengths]
    cs = [torch.randn(L * hop, A, generator=g) for L in lengths]
    s0 = [torch.randn(L * hop, S, generator=g) for L in lengths]
    x, c, s = xs[0].T, cs[0].T, s0[0].T
    r64, r32 = P.layer(sd, cfg, layer, x, c), P.layer(sd, cfg, layer, x, c, torch.float32)
    emu = {v: E.layer_emu(sd, cfg, layer, x, c, v) for v in E.VARIANTS}
    gate64 = emu["emu64"][2].abs()
    q = "conv_layers.{}.".format(layer)
    out = {"xs": xs, "cs": cs, "s0": s0}
    for what, j, ref64, ref32, w2 in (("x", 0, r64[0], r32[0], sd[q + "conv1x1_out.weight"]), ("skips", 1, s.double() + r64[1], s + r32[1], sd[q + "conv1x1_skip.weight"])):
        e32, scale = float((ref32.double() - ref64).abs().max()), float(ref64.abs().max())
        flips = (E.rb(w2[:, :, 0]).double().abs()[:, :, None] * gate64[None]).amax(dim=1)             # [col, t]: max over k
        out[what] = {"bar": 4 * e32 + 1e-6 * scale + 2 * 2.0 ** -7 * flips, "e32": e32, "scale": scale,
                     **{v: emu[v][j] if what == "x" else s.to(emu[v][j].dtype) + emu[v][j] for v in E.VARIANTS}}
        assert 0 < e32 < 1e-3 * scale and scale > 1e-3, "degenerate case"
    _LAYER[key] = out
    return out


def check_layer(tag, got, case):
    """got [channels, T] against the case's emu64 under the elementwise bar; prints the worst use of the bar and how much of it is the f32 term"""
    err = (got.double().cpu() - case["emu64"]).abs()
    use = float((err / case["bar"]).max())
    print(f"{tag}: max |got - emu64| {float(err.max()):.3e}  worst err / bar {use:.3f}  f32 term {4 * case['e32'] + 1e-6 * case['scale']:.3e}  scale {case['scale']:.3e}")
    assert bool((err <= case["bar"]).all()), tag
    return use


# ---------------------------------------------------------------------------------------------------------------- whole generator
def generator_refs(name, mel, z):
    """ref64, ref32, emu64, emu32, emu32b [T] and e_bf, e32, scale of one utterance (cached by configuration and the inputs' bytes)"""
    key = (name, mel.numpy().tobytes(), z.numpy().tobytes())
    if key not in _GEN:
        cfg, sd = CFGS[name], sd_of(name)
        r = {"ref64": P.generator(sd, cfg, mel, z), "ref32": P.generator(sd, cfg, mel, z, torch.float32)}
        r.update({v: E.generator_emu(sd, cfg, mel, z, v) for v in E.VARIANTS})
        r["e_bf"] = float((r["emu64"] - r["ref64"]).abs().max())
        r["e32"] = float((r["ref32"].double() - r["ref64"]).abs().max())
        r["scale"] = float(r["ref64"].abs().max())
        _GEN[key] = r
    return _GEN[key]


def check_generator(tag, got, r):
    d64, demu = float((got.double().cpu() - r["ref64"]).abs().max()), float((got.double().cpu() - r["emu64"]).abs().max())
    print(f"{tag}: e_bf / scale {r['e_bf'] / r['scale']:.3e}  e32 / scale {r['e32'] / r['scale']:.3e}  |got - ref64| / e_bf {d64 / r['e_bf']:.3f}  "
          f"|got - emu64| / e_bf {demu / r['e_bf']:.3f}")
    assert r["e_bf"] > 100 * r["e32"] > 0 and r["scale"] > 1e-3, "the case tests nothing"
    assert d64 <= 1.5 * r["e_bf"], tag
    assert demu <= 0.75 * r["e_bf"], tag
    return d64 / r["e_bf"], demu / r["e_bf"]


def generator_inputs(name, lengths):
    """mels [A, L] and noises [L * hop] of a generator case: the seeds of tests/test_gpu_pwg.py"""
    cfg = CFGS[name]
    return [P.uniform_mel(cfg["A"], L, 10 + L) for L in lengths], [noise_of(L * P.hop(cfg), 110 + L) for L in lengths]


def seeded_inputs(name):
    """mels, seed words and the restated noises of the seeded case"""
    cfg = CFGS[name]
    mels = [P.uniform_mel(cfg["A"], L, 40 + L) for L in SEEDED_LENGTHS]
    words = [P.pwg_seed_words(SEEDED_RUN, label, 0) for label in SEEDED_LABELS]
    return mels, words, [P.seeded_noise(*w, L * P.hop(cfg)) for w, L in zip(words, SEEDED_LENGTHS)]
