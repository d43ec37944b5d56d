"""The reference of the GE2E speaker encoder as DESIGN.md ("GE2E speaker encoder") states it: `torch.nn.LSTM` + `torch.nn.Linear` on the CPU and the
normalisation written out, float64 by default; `dtype=torch.float32` runs the very same code in single precision (the yardstick of the error bar).
Shared by tests/test_ge2e_cpu.py, tests/test_gpu_ge2e.py and tests/test_gpu_ge2e_entrypoints.py."""
import torch


def sizes_of(Mel, H, Stacks, E):
    return {"Mel": Mel, "H": H, "Stacks": Stacks, "E": E}


def modules(sizes, dtype=torch.float64):
    lstm = torch.nn.LSTM(sizes["Mel"], sizes["H"], sizes["Stacks"], batch_first=True)
    linear = torch.nn.Linear(sizes["H"], sizes["E"])
    return lstm.to(dtype), linear.to(dtype)


def random_state_dict(sizes, seed, scale=1.0):
    """torch's default initialisation of LSTM and Linear under a fixed seed (the global generator is left as it was), every tensor multiplied by `scale`
    (scale 3 drives the gates into saturation)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lstm, linear = modules(sizes, torch.float32)
    sd = {"lstm." + k: v.detach().clone() * scale for k, v in lstm.state_dict().items()}
    sd.update({"linear." + k: v.detach().clone() * scale for k, v in linear.state_dict().items()})
    return sd


def uniform_input(N, Mel, T, seed):
    """[N, Mel, T] uniform in [-4, 4]"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, Mel, T, generator=g) * 8.0 - 4.0


@torch.no_grad()
def forward(sd, sizes, x, samples, dtype=torch.float64):
    """x [B * samples, Mel, T] -> (hs [Stacks, N, T, H], e [N, E], d [B, E]) in `dtype`.  All hidden states come from running the layers one by one."""
    lstm, linear = modules(sizes, dtype)
    lstm.load_state_dict({k[len("lstm."):]: v.to(dtype) for k, v in sd.items() if k.startswith("lstm.")})
    linear.load_state_dict({k[len("linear."):]: v.to(dtype) for k, v in sd.items() if k.startswith("linear.")})
    inp = x.to(dtype).transpose(1, 2)                                        # [N, T, Mel]
    top, _ = lstm(inp)
    hs = []
    cur = inp
    for k in range(sizes["Stacks"]):                                         # the same layers, one at a time, to expose every hidden state
        one = torch.nn.LSTM(cur.shape[2], sizes["H"], 1, batch_first=True).to(dtype)
        one.load_state_dict({n[:-1] + "0": getattr(lstm, n).detach() for n in ("weight_ih_l%d" % k, "weight_hh_l%d" % k, "bias_ih_l%d" % k, "bias_hh_l%d" % k)})
        cur, _ = one(cur)
        hs.append(cur)
    hs = torch.stack(hs)
    assert torch.equal(hs[-1], top)
    e = linear(top[:, -1])
    w = e / e.norm(dim=1, keepdim=True).clamp_min(1e-12)
    m = w.reshape(-1, samples, w.shape[1]).mean(1)
    d = m / m.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return hs, e, d


def errors(got, ref64, ref32):
    """(err, e32, scale): max |got - ref64| / max |ref64|, the same for the float32 run of the reference, and max |ref64|"""
    scale = float(ref64.abs().max())
    return float((got.double().cpu() - ref64).abs().max()) / scale, float((ref32.double() - ref64).abs().max()) / scale, scale


def check(name, got, ref64, ref32):
    """The bar: err <= 4 e32 + 1e-6 with the guards 0 < e32 < 1e-3 and max |ref64| > 1e-3; the figures are printed before they are asserted."""
    err, e32, scale = errors(got, ref64, ref32)
    print("{}: err {:.3e}  e32 {:.3e}  ratio {:.3f}  max|ref| {:.3e}".format(name, err, e32, err / (4 * e32 + 1e-6), scale))
    assert 0 < e32 < 1e-3 and scale > 1e-3, (name, e32, scale)
    assert err <= 4 * e32 + 1e-6, (name, err, e32)
