"""Helpers of the fused coupling kernels' GPU tests (tests/test_gpu_wavenet_fused.py, tests/test_gpu_wavenet_fused_contract.py): a seeded full-width decoder
on the device, the training forward / the gradients with the fused launches switched on or off, the PAIR-packed columns of the kept (m, logs) rows, the
fraction-of-elements comparison and the rows next to the workgroups' window seams.  A plain helper module, no tests."""
import torch

from helpers import full_width_state, launch_counts, launch_reset


def setup(n_flows, lengths, tm, spk_dim=0, seed=0, mel_dim=80, n_layers=4):
    from glow_tts_amd import decoder as D
    g = torch.Generator().manual_seed(seed)
    cfg, sd = full_width_state(n_flows, g, spk_dim=spk_dim, mel_dim=mel_dim, n_layers=n_layers)
    dc = D.DecoderConfig(cfg.mel_dim, cfg.n_flows, cfg.n_squeeze, cfg.n_split, cfg.wn_channels, cfg.wn_layers, cfg.wn_kernel, 1)
    P = {k: v.cuda() for k, v in sd.items()}
    B = len(lengths)
    mels = (torch.randn(B, mel_dim, tm, generator=g) * 1.5).clamp(-4, 4).cuda()
    ml = torch.tensor(lengths).cuda()
    spk = None
    if spk_dim:
        spk = torch.randn(B, spk_dim, generator=g)
        spk = (spk / spk.norm(dim=1, keepdim=True)).cuda()
    W = dict(zip(D.WEIGHT_KEYS, [w.contiguous() for w in D.stack_decoder_weights(P, dc)]))
    cond = D.conditioning(P, dc, speakers=spk) if spk is not None else None
    return D, dc, W, mels, ml, cond


def forward(D, dc, W, mels, ml, cond, fused, drop_p=0.0, seed=None):
    D.TUNE["fused_wn"] = fused
    try:
        with torch.no_grad():
            prep = D._Prepared(dc, W, need_bwd=False, cond=cond)
            launch_reset()
            z, logdet, buf, rowmask, T, _ = D._run_forward(dc, prep, mels, ml, drop_p, seed)
            torch.cuda.synchronize()
            return z, logdet, buf, rowmask, launch_counts()
    finally:
        D.TUNE["fused_wn"] = True


def outs_columns(c2=80):
    """Columns of the kept (m, logs) buffer: packed column p * 64 + h * 32 + j holds half h (0 = m, 1 = logs) of channel p * 32 + j < c2."""
    m = [p * 64 + j for p in range(3) for j in range(32) if p * 32 + j < c2]
    return torch.tensor(m, device="cuda"), torch.tensor([c + 32 for c in m], device="cuda")


def close_rows(a, b, what, rowmask=None, atol=0.0, frac=0.0, big=None):
    """|a - b| <= atol everywhere except on at most `frac` of the elements (bf16 one-ulp flips), where it stays <= big."""
    a, b = a.float(), b.float()
    if rowmask is not None:
        m = rowmask.view(-1, *([1] * (a.dim() - 1)))
        a, b = a * m, b * m
    d = (a - b).abs()
    bad = (d > atol).float().mean().item()
    assert bad <= frac, (what, "fraction above atol", bad, "max", d.max().item())
    if big is not None:
        assert d.max().item() <= big, (what, d.max().item())


def grads(D, dc, P, mels, ml, wz, wl, fused_bwd, drop_p=0.0, cond=None, seed=None):
    """seed: None (the function draws the step's dropout word from torch's generator) or the word as an int32 device tensor [1]"""
    default = D.TUNE["fused_wn_bwd"]
    D.TUNE["fused_wn_bwd"] = fused_bwd
    try:
        Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        x = mels.clone().requires_grad_(True)
        W = D.stack_decoder_weights(Pg, dc)
        c = cond.clone().requires_grad_(True) if cond is not None else None
        launch_reset()
        if seed is not None:
            D.AUX["seed"] = seed
        z, logdet, _ = D.DecoderFunction.apply(dc, x, ml, c, drop_p, None, None, None, *W)
        ((z * wz).sum() + (logdet * wl).sum()).backward()
        torch.cuda.synchronize()
        g = {k: p.grad for k, p in Pg.items() if p.grad is not None}
        if c is not None:
            g["<conditioning>"] = c.grad
        return g, x.grad, launch_counts()
    finally:
        D.TUNE["fused_wn_bwd"] = default


def seam_rows(R, stride, width):
    """bool [R] on the device: the flat rows within `width` rows of a multiple of `stride` (the first owned row of a workgroup's window)"""
    seam = torch.zeros(R, dtype=torch.bool, device="cuda")
    for k in range(0, R, stride):
        seam[max(k - width, 0):k + width] = True
    return seam
