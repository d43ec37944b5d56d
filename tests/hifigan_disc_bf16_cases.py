"""Shapes, inputs and bars of the multi-period discriminator's bf16 tests (tests/test_gpu_hifigan_disc_bf16.py, .._trainer.py, test_hifigan_disc_bf16_cpu.py).

Four references per (case, seed), computed once on the CPU, shared and left unchanged:
    ref64 / ref32   hifigan_disc_ref.score_grads in float64 / float32: the UNROUNDED network and float32's distance from it, e32 = max |ref32 - ref64|
    emu64 / emu32   hifigan_disc_bf16_ref.score_grads in float64 / float32: the bf16 contract and one float32 realisation of it
e_mix = max |emu64 - ref64| is what the mode costs on a tensor.  The bars are in units of e_mix and come from these four alone, never from the kernels:
    bar (a), every case     |got - ref64| <= BAR_A e_mix,  BAR_A = 1.5 x the largest |emu32 - ref64| / e_mix (1.5: the margin of hifigan_mixed_cases.py - the
                            kernels sum in another order than emu32)
    bar (b), narrow cases   |got - emu64| <= BAR_B e_mix,  BAR_B = 2 x the largest |emu32 - emu64| / e_mix there.  The wide case is excluded: float32 summation
                            order flips bf16 roundings in its 1024-wide layers, so two float32 realisations differ by a large part of e_mix.
    guard                   a pair (tensor, case) is compared only when e_mix > 100 e32; the dropped pairs are listed by name (DROPPED) and are at most 5 %.
The operator bar is hifigan_mixed_cases.py's: on float32 inputs the kernels round exactly, so max |got - emu64| / max |emu64| <= 4 e32' + 1e-6 with e32' the
float32 realisation's error on the same operator call.

Measured on the CPU by `python tests/hifigan_disc_bf16_cases.py` (MEASURED below is that run's table; test_hifigan_disc_bf16_cpu.py re-measures and asserts
that BAR_A, BAR_B and DROPPED follow from it)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import hifigan_disc_bf16_ref as BR  # noqa: E402
import hifigan_disc_ref as HR  # noqa: E402

SLOPE, WEIGHT_SCALE, AMPLITUDE = 0.1, 3.0, 0.3
SEEDS = (1234, 4321)
NARROW = [16, 32, 16]
DEFAULT = [32, 128, 512, 1024, 1024]
CASES = {
    # name: (Periods, Channels, B, T) - the first eight and c64_80: tests/test_gpu_hifigan_disc.py's geometry
    "narrow_b3": ([2, 3], NARROW, 3, 50),
    "p7_pad6": ([7], NARROW, 2, 50),
    "t2p": ([5], NARROW, 2, 10),
    "rows63": ([3], NARROW, 2, 542),
    "rows64": ([2], NARROW, 2, 559),
    "rows65": ([5], NARROW, 2, 541),
    "splits": ([3], NARROW, 1, 3300),                  # two weight-gradient chunks
    "c64_80": ([3], [64, 64, 80], 2, 200),             # the (4, 1) layout; a K walk of 64 + 16 -> 32
    "k48_80": ([3], [16, 48, 80, 16], 2, 200),         # K chunks padded 48 -> 64 and 16 -> 32; the (1, 1), (1, 1) and (1, 1) layouts over 80 columns
    "default_p11": ([11], DEFAULT, 1, 600),            # 16 K chunks, 8 column groups
    "p16": ([16], NARROW, 2, 203),                     # the largest period: H0 = 13, pad 5
}
NARROW_CASES = tuple(c for c, v in CASES.items() if v[1] == NARROW)
GUARD, MAX_DROPPED = 100.0, 0.05

# ---- the measured constants (MEASURED: the run they come from) ----
WORST_A, WORST_B = 1.0515, 0.01173   # the largest |emu32 - ref64| / e_mix over all cases; the largest |emu32 - emu64| / e_mix over the narrow cases
BAR_A, BAR_B = 1.5 * WORST_A, 2.0 * WORST_B
DROPPED = ()                         # "case/seed/tensor" of the pairs that miss the guard: none

MEASURED = """
case         seed  pairs dropped  max|emu32-ref64|/e_mix  max|emu32-emu64|/e_mix (tensor)                          max e_mix/max|ref64| (tensor)   min cos
narrow_b3     1234    25       0                  1.0000     0.01173 d.1.conv_post.bias                           0.0191 d.0.convs.2.weight       0.99987
narrow_b3     4321    25       0                  1.0000     0.00011 d.1.conv_post.weight                         0.2513 dwav                     0.98674
p7_pad6       1234    13       0                  1.0000     0.00070 d.0.conv_post.bias                           0.3799 dwav                     0.97335
p7_pad6       4321    13       0                  1.0001     0.00009 d.0.convs.2.bias                             0.0111 scores[0]                0.99996
t2p           1234    13       0                  1.0012     0.00124 d.0.conv_post.bias                           0.0043 dwav                     1.00000
t2p           4321    13       0                  1.0000     0.00069 d.0.conv_post.bias                           0.0078 dwav                     0.99998
rows63        1234    13       0                  1.0001     0.00009 map[0][1]                                    0.1229 dwav                     0.99955
rows63        4321    13       0                  1.0003     0.00667 d.0.convs.0.bias                             0.2433 dwav                     0.99654
rows64        1234    13       0                  1.0003     0.00029 d.0.conv_post.bias                           0.0815 dwav                     0.99937
rows64        4321    13       0                  1.0001     0.00012 d.0.conv_post.bias                           0.2051 dwav                     0.99822
rows65        1234    13       0                  1.0001     0.00007 scores[0]                                    0.1286 dwav                     0.99842
rows65        4321    13       0                  1.0000     0.00021 d.0.conv_post.bias                           0.1161 dwav                     0.99807
splits        1234    13       0                  1.0000     0.00461 scores[0]                                    0.2583 dwav                     0.99789
splits        4321    13       0                  1.0002     0.00376 dwav                                         0.2129 dwav                     0.99701
c64_80        1234    13       0                  1.0000     0.00006 map[0][1]                                    0.0861 dwav                     0.99810
c64_80        4321    13       0                  1.0000     0.00817 d.0.conv_post.bias                           0.1891 dwav                     0.99800
k48_80        1234    16       0                  1.0000     0.00006 map[0][1]                                    0.0074 d.0.convs.1.bias         0.99999
k48_80        4321    16       0                  1.0000     0.00007 scores[0]                                    0.0850 dwav                     0.99715
default_p11   1234    19       0                  1.0515     0.67700 d.0.conv_post.bias                           0.1095 dwav                     0.99751
default_p11   4321    19       0                  1.0143     0.01434 d.0.conv_post.bias                           0.1055 d.0.convs.4.weight       0.99764
p16           1234    13       0                  1.0000     0.00022 d.0.conv_post.bias                           0.1731 dwav                     0.99851
p16           4321    13       0                  1.0000     0.00003 map[0][1]                                    0.2804 dwav                     0.99777
pairs 328, dropped 0: []; worst (a) 1.0515, worst (b) on the narrow cases 0.01173
"""

_cache = {}


def case_inputs(case, seed):
    periods, channels, B, T = CASES[case]
    g = torch.Generator().manual_seed(7)
    return HR.random_state_dict(periods, channels, seed, WEIGHT_SCALE), (torch.randn(B, T, generator=g) * AMPLITUDE).float()


def references(case, seed):
    """-> dict(ref64, ref32, emu64, emu32), each score_grads' dict"""
    if (case, seed) not in _cache:
        periods, channels, _, _ = CASES[case]
        sd, wav = case_inputs(case, seed)
        n = len(channels)
        _cache[(case, seed)] = {"ref64": HR.score_grads(sd, wav, periods, n, SLOPE, 1.0, dtype=torch.float64),
                                "ref32": HR.score_grads(sd, wav, periods, n, SLOPE, 1.0, dtype=torch.float32),
                                "emu64": BR.score_grads(sd, wav, periods, n, SLOPE, 1.0, dtype=torch.float64),
                                "emu32": BR.score_grads(sd, wav, periods, n, SLOPE, 1.0, dtype=torch.float32)}
    return _cache[(case, seed)]


def tensors(result):
    """A score_grads-shaped dict -> {name: tensor}: per period scores, every feature map the mode reaches, d wav and every parameter gradient.  map[i][0] is
    the first layer's output, f32 launches on the waveform in both modes (e_mix = 0 by construction): it is no pair of these bars - the GPU test holds it
    to the f32 mode's bits instead."""
    out = {}
    for i, s in enumerate(result["scores"]):
        out[f"scores[{i}]"] = s
    for i, maps in enumerate(result["maps"]):
        for j, m in enumerate(maps):
            if j:
                out[f"map[{i}][{j}]"] = m
    out["dwav"] = result["dwav"]
    out.update(result["grads"])
    return out


def dist(a, b):
    return float((a.double() - b.double()).abs().max())


def pair_figures(case, seed):
    """-> {tensor: dict(e_mix, e32, a = |emu32 - ref64| / e_mix, b = |emu32 - emu64| / e_mix, scale = max |ref64|, cos)}"""
    r = {k: tensors(v) for k, v in references(case, seed).items()}
    out = {}
    for name, ref in r["ref64"].items():
        e_mix, e32 = dist(r["emu64"][name], ref), dist(r["ref32"][name], ref)
        cos = float(torch.nn.functional.cosine_similarity(r["emu64"][name].double().flatten(), ref.double().flatten(), dim=0))
        out[name] = {"e_mix": e_mix, "e32": e32, "a": dist(r["emu32"][name], ref) / e_mix if e_mix else float("inf"),
                     "b": dist(r["emu32"][name], r["emu64"][name]) / e_mix if e_mix else float("inf"), "scale": float(ref.abs().max()), "cos": cos}
    return out


def compared(fig):
    return fig["e_mix"] > GUARD * fig["e32"]


def measure(cases=None, seeds=SEEDS):
    """-> dict(worst_a, worst_b, dropped, pairs, rows): the figures the bars come from"""
    rows, dropped, pairs, worst_a, worst_b = [], [], 0, 0.0, 0.0
    for case in cases or CASES:
        for seed in seeds:
            figs = pair_figures(case, seed)
            live = {k: f for k, f in figs.items() if compared(f)}
            pairs += len(figs)
            dropped += [f"{case}/{seed}/{k}" for k in figs if k not in live]
            a = max(live.values(), key=lambda f: f["a"])
            b = max(live.items(), key=lambda kv: kv[1]["b"])
            worst_a = max(worst_a, a["a"])
            if case in NARROW_CASES:
                worst_b = max(worst_b, b[1]["b"])
            rel = max((f["e_mix"] / f["scale"], k) for k, f in live.items())
            rows.append((case, seed, len(figs), len(figs) - len(live), a["a"], b[1]["b"], b[0], rel[0], rel[1], min(f["cos"] for f in live.values())))
    return {"worst_a": worst_a, "worst_b": worst_b, "dropped": dropped, "pairs": pairs, "rows": rows}


def table(m):
    lines = ["case         seed  pairs dropped  max|emu32-ref64|/e_mix  max|emu32-emu64|/e_mix (tensor)                          max e_mix/max|ref64| (tensor)   min cos"]
    for case, seed, n, d, a, b, bk, rel, rk, cos in m["rows"]:
        lines.append(f"{case:12s} {seed:5d} {n:5d} {d:7d}  {a:22.4f}  {b:10.5f} {bk.replace('discriminators.', 'd.'):42s} {rel:8.4f} {rk.replace('discriminators.', 'd.'):24s} {cos:.5f}")
    lines.append(f"pairs {m['pairs']}, dropped {len(m['dropped'])}: {m['dropped']}; worst (a) {m['worst_a']:.4f}, worst (b) on the narrow cases {m['worst_b']:.5f}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(table(measure()))
