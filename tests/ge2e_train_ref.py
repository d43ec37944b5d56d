"""The reference of the GE2E speaker encoder's training step (DESIGN.md "Training the GE2E speaker encoder"): `torch.nn.LSTM` + `torch.nn.Linear` of
tests/ge2e_ref.py with autograd on the CPU and the GE2E softmax loss written out, float64 by default; `dtype=torch.float32` runs the very same code in single
precision (the yardstick of the error bar).  Shared by tests/test_ge2e_train_cpu.py, tests/test_gpu_ge2e_train.py and tests/test_gpu_ge2e_trainer.py."""
import torch

import ge2e_ref as R

# (S, M, T, Mel, H, Stacks, E, weight scale): the cases of the GPU bar tests
CASES = {
    "one_cell": (2, 2, 1, 4, 16, 1, 8, 1),                 # one cell, no recurrence: dW_hh is exactly zero
    "two_layers": (2, 3, 5, 12, 16, 2, 16, 1),             # both inflows of dh
    "odd": (3, 2, 7, 20, 48, 3, 24, 3),                    # odd sizes, saturating gates
    "second_tile": (9, 2, 3, 12, 80, 2, 16, 3),            # N = 18: a second sequence tile; N T = 54: a ragged reduction
    "chunks": (5, 4, 37, 12, 32, 2, 16, 1),                # N T = 740: several reduction chunks, odd T
    "wide": (2, 2, 2, 4, 768, 2, 8, 1),                    # H = 768: the chunked K range of the backward cell
    "shipped": (2, 2, 64, 80, 256, 3, 256, 1),             # the shipped widths
}
WEIGHT_SEED, INPUT_SEED, W0 = 11, 5, 10.0
MUTATIONS = ("inclusive", "mean", "gates")


def ge2e_loss(e, w, S, M, mutate=None, bias=0.0):
    """The GE2E softmax loss over e [S M, E] (row j M + i: speaker j's utterance i).  mutate: 'inclusive' (the own speaker's centroid keeps the utterance),
    'mean' (the own speaker's mean stands in for sum / (M - 1): c_j - u_ji / (M - 1)); bias: added to every score (the loss does not depend on it)."""
    N, E = e.shape
    assert N == S * M and S >= 2 and M >= 2
    u = e / e.norm(dim=1, keepdim=True).clamp_min(1e-12)
    U = u.reshape(S, M, E)
    sums = U.sum(1)
    cent = sums / M
    if mutate == "inclusive":
        excl = cent[:, None, :].expand(S, M, E)
    elif mutate == "mean":
        excl = cent[:, None, :] - U / (M - 1)
    else:
        excl = (sums[:, None, :] - U) / (M - 1)
    cos_all = (u @ cent.t()) / cent.norm(dim=1).clamp_min(1e-12)[None, :]                    # [N, S]
    cos_own = ((U * excl).sum(-1) / excl.norm(dim=-1).clamp_min(1e-12)).reshape(N)            # [N]
    own = torch.arange(N) // M
    mask = torch.zeros(N, S, dtype=torch.bool)
    mask[torch.arange(N), own] = True
    scores = w * torch.where(mask, cos_own[:, None].expand(N, S), cos_all) + bias
    return (torch.logsumexp(scores, dim=1) - scores[torch.arange(N), own]).mean()


def _swap_g_o(t):
    i, f, g, o = t.chunk(4, 0)
    return torch.cat([i, f, o, g], 0)


def network(sd, sizes, dtype=torch.float64, mutate=None):
    """(lstm, linear) holding sd in `dtype`, parameters requiring gradients; mutate 'gates': the weights read in the gate order i, f, o, g."""
    lstm, linear = R.modules(sizes, dtype)
    state = {k[len("lstm."):]: v.to(dtype) for k, v in sd.items() if k.startswith("lstm.")}
    if mutate == "gates":
        state = {k: _swap_g_o(v) for k, v in state.items()}
    lstm.load_state_dict(state)
    linear.load_state_dict({k[len("linear."):]: v.to(dtype) for k, v in sd.items() if k.startswith("linear.")})
    return lstm, linear


def embed(lstm, linear, x):
    top, _ = lstm(x.to(lstm.weight_ih_l0.dtype).transpose(1, 2))
    return linear(top[:, -1])


def run(sd, sizes, x, S, M, w=W0, dtype=torch.float64, mutate=None):
    """-> {'L', 'e', 'de', 'dw', 'grads': {parameter name: gradient}} of one forward + loss + backward in `dtype`"""
    lstm, linear = network(sd, sizes, dtype, mutate if mutate == "gates" else None)
    wt = torch.tensor(float(w), dtype=dtype, requires_grad=True)
    e = embed(lstm, linear, x)
    e.retain_grad()
    L = ge2e_loss(e, wt, S, M, mutate if mutate != "gates" else None)
    L.backward()
    grads = {"lstm." + k: p.grad.detach() for k, p in lstm.named_parameters()}
    grads.update({"linear." + k: p.grad.detach() for k, p in linear.named_parameters()})
    if mutate == "gates":
        grads = {k: (_swap_g_o(v) if k.startswith("lstm.") else v) for k, v in grads.items()}
    return {"L": L.detach().reshape(1), "e": e.detach(), "de": e.grad.detach(), "dw": wt.grad.detach().reshape(1), "grads": grads}


def case_inputs(case):
    S, M, T, Mel, H, Stacks, E, scale = CASES[case]
    sizes = R.sizes_of(Mel, H, Stacks, E)
    return sizes, R.random_state_dict(sizes, WEIGHT_SEED, scale), R.uniform_input(S * M, Mel, T, INPUT_SEED)


_CACHE = {}


def case_reference(case):
    """(ref64, ref32) of a case, computed once per process and shared (callers leave it unchanged)."""
    if case not in _CACHE:
        S, M = CASES[case][:2]
        sizes, sd, x = case_inputs(case)
        _CACHE[case] = (run(sd, sizes, x, S, M), run(sd, sizes, x, S, M, dtype=torch.float32))
    return _CACHE[case]


def tensors(result):
    """name -> tensor for everything the bar applies to"""
    out = {"L": result["L"], "de": result["de"], "dw": result["dw"]}
    out.update(result["grads"])
    return out
