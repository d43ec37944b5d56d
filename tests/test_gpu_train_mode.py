"""Train-mode parity of the text encoder: the dropout masks of the HIP path injected into float64 references.

Every published number of this project is a training step, and the shipped hyper-parameters train the text encoder with dropout at the
prenet (0.5), four sites of every transformer layer (0.1: attention probabilities, after Projection, after Conv_0 + ReLU, after Conv_1) and the
duration predictor (0.1).  The library writes none of its keep masks down: every kernel re-derives them from (seed, element id), the
backward kernels again, or recovers them from `output != 0`.  tests/dropout_masks.py restates the draw on the host; here it is
  (a) shown to BE the kernels' draw (p = 0 run against p > 0 run of the same launch),
  (b) applied inside float64 torch expressions of the single operators (LayerNormRows, ConvRows, RPRAttention in its three kernel
      families, the fused projection + LayerNorm), forward and every gradient,
  (c, d) injected into the oracle's encoder (oracle/glowtts_ref.py `drop=` hooks, pinned against the reference in train mode by
      tests/test_oracle_golden.py) for the whole encoder in f32 and on the benchmarked bf16 block path,
  (e) and into `O.forward_train` for the whole model in train(), encoder and WaveNet masks from the step's ONE seed word.
References are float64 expressions or the oracle, never another HIP path.  Site seeds come from the library's `encoder.DROP_LOG`; rates, site
names and shapes come from the hyper-parameters and the oracle's own hook calls (a logged rate or site that differs is a failure)."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_masks as DM
from oracle import glowtts_ref as O
from helpers import launch_counts, launch_reset, load_case, tiny_cfg, tiny_hp_dict

pytestmark = pytest.mark.gpu

WORD = 0x2B5E7A11                       # a given seed word (what `decoder.step_seed` would draw)


def _seed_t(word=WORD):
    return torch.tensor([word], dtype=torch.int32, device="cuda")


def _rowmask(B, T, lens):
    m = torch.zeros(B, T + 4)
    for b, n in enumerate(lens):
        m[b, 2:2 + n] = 1.0
    return m.reshape(-1)


def _rel(a, b):
    """Largest difference relative to the reference tensor's largest entry."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


def _cos_ratio(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item(), (a.norm() / (b.norm() + 1e-30)).item()


def _keep_stats(keep, p):
    """Whole-tensor keep fraction within 5 sigma of 1 - p."""
    n = keep.numel()
    frac = keep.ne(0).double().mean().item()
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(frac - (1 - p)) <= 5 * sigma, (frac, p, n)
    vals = set(torch.unique(keep).tolist())
    assert vals <= {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}, vals


# ------------------------------------------------------------------------------------------------ (a) the restated masks are the kernels' masks
@pytest.mark.parametrize("C,relu,p", [(192, True, 0.5), (256, False, 0.1), (100, True, 0.1), (32, False, 0.5)])
def test_layernorm_site_draws_the_restated_mask(C, relu, p):
    """LayerNormRows at p = 0 and p > 0 on the same inputs: y_p == keep * y_0 bit for bit (keep in {0, 1/(1-p)} is applied to the finished value)."""
    from glow_tts_amd.conv_fn import layernorm_rows
    g = torch.Generator().manual_seed(C)
    B, T = 3, 41
    R = B * (T + 4)
    rowmask = _rowmask(B, T, [41, 30, 7]).cuda()
    a, gamma, beta = torch.randn(R, C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
    y0 = layernorm_rows(a, None, gamma, beta, rowmask, relu=relu, drop_p=0.0, seed=7919, seed_t=_seed_t())
    yp = layernorm_rows(a, None, gamma, beta, rowmask, relu=relu, drop_p=p, seed=7919, seed_t=_seed_t())
    keep = DM.linear_keep(DM.site_seed(7919, WORD), R, C, p)
    _keep_stats(keep, p)
    assert torch.equal(yp.cpu(), keep * y0.cpu())
    other = layernorm_rows(a, None, gamma, beta, rowmask, relu=relu, drop_p=p, seed=2 * 7919, seed_t=_seed_t())
    assert not torch.equal(other, yp)                                     # another site seed: another stream
    k2 = DM.linear_keep(DM.site_seed(2 * 7919, WORD), R, C, p)
    assert torch.equal(other.cpu(), k2 * y0.cpu())
    a_, b_ = keep.ne(0).double().flatten(), k2.ne(0).double().flatten()
    corr = torch.corrcoef(torch.stack([a_, b_]))[0, 1].item()
    assert abs(corr) * math.sqrt(a_.numel()) <= 5, corr


@pytest.mark.parametrize("Cin,O_,k,precision,out_bf16,p", [(192, 768, 3, 0, False, 0.1), (32, 48, 5, 0, False, 0.5), (192, 192, 1, 0, False, 0.1),
                                                           (192, 768, 3, 1, True, 0.1), (448, 256, 3, 1, False, 0.1), (768, 192, 3, 1, False, 0.5)])
def test_conv_site_draws_the_restated_mask(Cin, O_, k, precision, out_bf16, p):
    """ConvRows (LINEAR epilogue: bias, ReLU, dropout, row mask) at p = 0 and p > 0: out_p == keep * out_0 - exactly for fp32 outputs (the same
    accumulation, one multiplication more), to one bf16 rounding for bf16-stored outputs; zeros in exactly the restated places."""
    from glow_tts_amd.conv_fn import conv_rows
    g = torch.Generator().manual_seed(Cin + O_ + k)
    B, T = 2, 37
    R = B * (T + 4)
    rowmask = _rowmask(B, T, [37, 20]).cuda()
    x = (torch.randn(R, Cin, generator=g).cuda() * rowmask[:, None]).contiguous()
    w, b = (torch.randn(O_, Cin, k, generator=g) / (Cin * k) ** 0.5).cuda(), torch.randn(O_, generator=g).cuda()
    xb = x.to(torch.bfloat16) if precision == 1 else None
    run = lambda p_: conv_rows(x, w, b, rowmask, relu=True, mask_out=True, precision=precision, drop_p=p_, seed=3 * 7919, seed_t=_seed_t(), xb=xb,
                               out_bf16=out_bf16)
    y0, yp = run(0.0), run(p)
    assert yp.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
    keep = DM.linear_keep(DM.site_seed(3 * 7919, WORD), R, O_, p)
    _keep_stats(keep, p)
    y0c, ypc = y0.float().cpu(), yp.float().cpu()
    nz = y0c != 0
    assert torch.equal((ypc != 0) & nz, (keep != 0) & nz)
    if out_bf16:
        assert ((ypc - keep * y0c).abs() <= 2 ** -7 * (keep * y0c).abs()).all()
    else:
        assert torch.equal(ypc, keep * y0c)


# ------------------------------------------------------------------------------------------------ (b) operators against float64
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("C", [192, 256, 32, 100])
def test_layernorm_rows_train_mode_against_float64(C, residual, relu, p):
    """LayerNormRows (the unrolled 192 / 256 kernels and the generic one): y, d a, d b, d gamma, d beta against float64 with the restated mask applied
    behind the ReLU and ahead of the row mask (Modules.py:485-487); 2e-5 of each tensor's largest entry."""
    from glow_tts_amd.conv_fn import layernorm_rows
    g = torch.Generator().manual_seed(1000 * C + 10 * int(residual) + int(relu))
    B, T = 3, 53
    R = B * (T + 4)
    rowmask = _rowmask(B, T, [53, 44, 9])
    seed = 5 * 7919
    a = torch.randn(R, C, generator=g)
    b = torch.randn(R, C, generator=g) if residual else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    dy = torch.randn(R, C, generator=g)
    leaves = [t.cuda().requires_grad_(True) for t in (a, gamma, beta)] + ([b.cuda().requires_grad_(True)] if residual else [])
    y = layernorm_rows(leaves[0], leaves[3] if residual else None, leaves[1], leaves[2], rowmask.cuda(), relu=relu, drop_p=p, seed=seed, seed_t=_seed_t())
    y.backward(dy.cuda())
    keep = DM.linear_keep(DM.site_seed(seed, WORD), R, C, p).double()
    ref = [t.double().requires_grad_(True) for t in (a, gamma, beta)] + ([b.double().requires_grad_(True)] if residual else [])
    s = ref[0] + ref[3] if residual else ref[0]
    want = F.layer_norm(s, (C,), ref[1], ref[2], 1e-4)
    if relu:
        want = torch.relu(want)
    want = want * keep * rowmask.double()[:, None]
    want.backward(dy.double())
    assert _rel(y, want) <= 2e-5, ("y", _rel(y, want))
    for name, got, w_ in zip(("da", "dgamma", "dbeta", "db"), leaves, ref):
        assert _rel(got.grad, w_.grad) <= 2e-5, (name, _rel(got.grad, w_.grad))


CONV_SHAPES = [(192, 192), (192, 768), (768, 192), (32, 48), (448, 256)]
# precision, bf16-stored operand, bf16-stored output
CONV_VARIANTS = [(0, False, False), (1, False, False), (1, True, False), (1, True, True)]


@pytest.mark.parametrize("variant", range(len(CONV_VARIANTS)))
@pytest.mark.parametrize("Cin,O_", CONV_SHAPES)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_conv_rows_train_mode_against_float64(k, Cin, O_, variant):
    """ConvRows = Conv1d + the elementwise tail the reference applies behind it (bias, ReLU, dropout, then the row mask: Modules.py:565-569, 643-646):
    output, dx, dw, db against float64 with the restated mask, for ReLU / mask_out on and off and p in {0.1, 0.5}.  f32: 2e-5 of the tensor's largest
    entry; bf16: 2e-2 (tests/test_gpu_conv.py).  In the bf16 variants x and w hold bf16-representable values: the products are then exact in both
    arithmetics and a ReLU gate cannot flip on an operand rounding - what remains is the kernels' own rounding of gradients and stored outputs."""
    from glow_tts_amd.conv_fn import conv_rows
    precision, stored, out_bf16 = CONV_VARIANTS[variant]
    tol = 2e-5 if precision == 0 else 2e-2
    g = torch.Generator().manual_seed(100 * Cin + O_ + k + 7 * variant)
    B, T = 3, 29
    R = B * (T + 4)
    rowmask = _rowmask(B, T, [29, 18, 5])
    x0 = torch.randn(R, Cin, generator=g) * rowmask[:, None]
    w0, b0 = torch.randn(O_, Cin, k, generator=g) / (Cin * k) ** 0.5, torch.randn(O_, generator=g) * 0.5
    if precision == 1:
        x0, w0 = x0.to(torch.bfloat16).float(), w0.to(torch.bfloat16).float()
    dy0 = torch.randn(R, O_, generator=g) * rowmask[:, None]
    case = 0
    for relu in (False, True):
        for mask_out in (False, True):
            for p in (0.1, 0.5):
                case += 1
                seed = case * 7919
                x, w, b = (t.cuda().requires_grad_(True) for t in (x0, w0, b0))
                xb = x.detach().to(torch.bfloat16) if stored else None
                y = conv_rows(x, w, b, rowmask.cuda(), relu=relu, mask_out=mask_out, precision=precision, drop_p=p, seed=seed, seed_t=_seed_t(), xb=xb,
                              out_bf16=out_bf16)
                y.backward(dy0.cuda().to(y.dtype))
                keep = DM.linear_keep(DM.site_seed(seed, WORD), R, O_, p).double()
                xr, wr, br = (t.double().requires_grad_(True) for t in (x0, w0, b0))
                want = F.conv1d(xr.view(B, T + 4, Cin).transpose(1, 2), wr, br, padding=(k - 1) // 2).transpose(1, 2).reshape(R, O_)
                if relu:
                    want = torch.relu(want)
                want = want * keep
                if mask_out:
                    want = want * rowmask.double()[:, None]
                want.backward(dy0.double())
                tag = (relu, mask_out, p)
                assert _rel(y, want) <= tol, (tag, "y", _rel(y, want))
                for name, got, w_ in (("dx", x, xr), ("dw", w, wr), ("db", b, br)):
                    assert _rel(got.grad, w_.grad) <= tol, (tag, name, _rel(got.grad, w_.grad))


def _attn_class(Tp, D):
    if D in (64, 96) and Tp <= 128:
        return "mfma"
    if D in (64, 96) and Tp <= 256:
        return "long"
    return "gen"


ATTN_SHAPES = [(120, 96), (57, 96), (100, 64), (150, 96), (200, 96), (252, 64), (125, 96), (40, 16), (250, 16)]
ATTN_CASES = [(T, D, 0) for T, D in ATTN_SHAPES] + [(T, D, 1) for T, D in [(120, 96), (57, 96), (100, 64), (124, 96)]]


@pytest.mark.parametrize("T,D,precision", ATTN_CASES)
def test_rpr_attention_train_mode_against_float64(T, D, precision):
    """The attention core with dropout 0.1 on the probabilities (RPR_MHA.py:119-126: the DROPPED probabilities feed both P @ V and the relative-V
    term, and the softmax is differentiated through the keep factor) in its three kernel families - single-workgroup MFMA (f32 and bf16), long MFMA,
    general - against float64 with the restated mask: output, dqkv, d relK, d relV.  The mask is written down nowhere: each family re-derives it
    in its forward and in its backward kernels.  Bars: 2e-5 in f32, 2e-2 and cosine >= 0.999 in bf16 (tests/test_gpu_encoder.py at p = 0)."""
    from glow_tts_amd.conv_fn import RPRAttention
    from test_gpu_encoder import attention_core_ref
    B, H, win, p = 3, 2, 4, 0.1
    Tp = T + 4
    seed = 11 * 7919
    g = torch.Generator().manual_seed(T + D)
    lens = [T, T - 9, max(5, T // 3)]
    rowmask = _rowmask(B, T, lens).cuda()
    qkv = (torch.randn(B * Tp, 3 * H * D, generator=g) * 0.5).cuda().requires_grad_(True)
    relk = (torch.randn(1, 2 * win + 1, D, generator=g) * D ** -0.5).cuda().requires_grad_(True)
    relv = (torch.randn(1, 2 * win + 1, D, generator=g) * D ** -0.5).cuda().requires_grad_(True)
    dout = torch.randn(B * Tp, H * D, generator=g).cuda() * rowmask[:, None]
    launch_reset()
    out = RPRAttention.apply(qkv, relk, relv, rowmask, B, Tp, H, win, p, seed, _seed_t(), precision)
    out.backward(dout)
    torch.cuda.synchronize()
    counts = launch_counts()
    cls = _attn_class(Tp, D)
    names = {"mfma": (f"attn_fwd_mfma<{D},{'bf16' if precision else 'f32'}>", f"attn_bwd_mfma<{D},{'bf16' if precision else 'f32'}>"),
             "long": (f"attn_fwd_long<{D}>", f"attn_bwd_long<{D}>"), "gen": ("attn_fwd_gen", "attn_bwd_gen")}[cls]
    assert counts.get(names[0], 0) == 1 and counts.get(names[1], 0) == 1, (names, {k: v for k, v in counts.items() if k.startswith("attn")})
    assert sum(v for k, v in counts.items() if k.startswith("attn_")) == 2, counts
    got = [out.detach(), qkv.grad.clone(), relk.grad.clone(), relv.grad.clone()]
    qkv.grad = relk.grad = relv.grad = None
    keep = DM.attention_keep(DM.site_seed(seed, WORD), B, H, Tp, p)
    _keep_stats(keep, p)
    ref = attention_core_ref(qkv.double(), relk[0].double(), relv[0].double(), rowmask.double(), B, Tp, H, win, keep=keep.double().cuda())
    ref.backward(dout.double())
    want = [ref.detach(), qkv.grad, relk.grad, relv.grad]
    valid = rowmask[:, None] > 0
    for name, a, b_ in zip(("out", "dqkv", "drelK", "drelV"), got, want):
        a, b_ = a.double(), b_.double()
        if name in ("out", "dqkv"):
            a, b_ = a * valid, b_ * valid               # padding rows carry no signal in the model
        err = (a - b_).abs().max().item() / max(1.0, b_.abs().max().item())
        cos = (a.flatten() @ b_.flatten() / (a.norm() * b_.norm())).item()
        if precision == 0:
            assert err < 2e-5, (name, err)
        else:
            assert err < 2e-2 and cos > 0.999, (name, err, cos)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_projection_and_layernorm_with_dropout_against_float64(p):
    """`glowtts_proj_layernorm` (csrc/gemm_cl.hip proj_ln_kernel; Modules.py:560-562): LayerNorm_0(Dropout(Projection(att)) + x) against float64 with the
    restated mask on the projection AFTER its bias and AHEAD of the residual.  The attention rows and the weight hold bf16-representable values
    (the launch contracts bf16 operands): products exact, fp32 accumulation - the kept projection and s = kept projection + x at 2e-5 of their largest
    entries, the kept projection's zeros exactly the mask's, y at 2e-5, the bf16 copy of y within one bf16 step."""
    from glow_tts_amd import conv_fn as CF, ops, _lib
    L = CF._L()
    g = torch.Generator().manual_seed(int(p * 10))
    R, C = 32 * 11 + 7, 192
    att = (torch.randn(R, C, generator=g)).to(torch.bfloat16).float()
    w = (torch.randn(C, C, 1, generator=g) * 0.1).to(torch.bfloat16).float()
    x, b = torch.randn(R, C, generator=g), torch.randn(C, generator=g) * 0.1
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rowmask = (torch.rand(R, generator=g) > 0.2).float()
    pw = ops.pack_weight(w.cuda(), precision=ops.BF16)
    seed = 13 * 7919
    dev = [t.cuda() for t in (att, b, x, gamma, beta, rowmask)]
    pk, s1, st1 = torch.full((R, C), 3.0, device="cuda"), torch.empty(R, C, device="cuda"), torch.empty(R, 2, device="cuda")
    y1, yb1 = torch.empty(R, C, device="cuda"), torch.empty(R, C, device="cuda", dtype=torch.bfloat16)
    st = _seed_t()
    _lib.check(L.glowtts_proj_layernorm(dev[0].data_ptr(), C, pw.data.data_ptr(), pw.npad, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(),
                                        dev[5].data_ptr(), pk.data_ptr(), s1.data_ptr(), st1.data_ptr(), y1.data_ptr(), yb1.data_ptr(),
                                        R, C, 1e-4, p, seed, st.data_ptr(), _lib.stream()), "proj_ln")
    torch.cuda.synchronize()
    keep = DM.linear_keep(DM.site_seed(seed, WORD), R, C, p).double()
    _keep_stats(keep, p)
    proj = (att.double() @ w[:, :, 0].double().t() + b.double()) * keep
    s = proj + x.double()
    y = F.layer_norm(s, (C,), gamma.double(), beta.double(), 1e-4) * rowmask.double()[:, None]
    assert torch.equal(pk.cpu() == 0, keep == 0)
    assert _rel(pk, proj) <= 2e-5 and _rel(s1, s) <= 2e-5 and _rel(y1, y) <= 2e-5, (_rel(pk, proj), _rel(s1, s), _rel(y1, y))
    assert (yb1.float().cpu().double() - y).abs().max().item() <= 2 ** -7 * y.abs().max().item()
    assert bool((y1[dev[5] == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ (c, d) the encoder as a whole
def _full_hp(precision, mode="Vanilla"):
    from glow_tts_amd import hparams
    d = copy.deepcopy(hparams.load_yaml(hparams.DEFAULT_YAML))
    d["Mode"] = mode
    d["HIP_Precision"] = precision
    return d


def _make_model(hp_dict, sd=None, seed=0):
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    torch.manual_seed(seed)
    model = GlowTTS(Recursive_Parse(hp_dict))
    if sd is not None:
        missing, unexpected = model.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
    for f in model.layer_Dict["Decoder"].layer_Dict["Flows"]:
        f.layers[0].initialized = True
    return model.cuda()


def _perturb_encoder(model, seed):
    """LayerNorm gains / offsets and biases away from their 1 / 0 initial values, so that every term of the backward carries signal."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "Encoder" in k and p.dim() == 1:
                p.add_((torch.randn(p.shape, generator=g) * 0.1).to(p.device))


def _upstream(B, M, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, M, T, generator=g), torch.randn(B, M, T, generator=g), torch.randn(B, 1, T, generator=g)


def _hip_encoder(model, tokens, tl, speakers, precision, training, up, word=WORD):
    """-> outputs, encoder gradients, DROP_LOG, launch counts of one `encoder_forward` + backward under the upstream gradients `up`."""
    from glow_tts_amd import encoder as E
    P = model._params()
    for p_ in P.values():
        p_.grad = None
    T = tokens.shape[1]
    mask, rowmask = E.token_masks(tl.cuda(), T)
    spk = F.embedding(speakers.cuda(), P["layer_Dict.LUT.weight"]) if speakers is not None else None
    E.DROP_LOG = []
    launch_reset()
    try:
        mean, log_std, log_dur = E.encoder_forward(P, model.hp, tokens.cuda(), mask, spk, None, training, precision=precision, cache=model._enc_cache,
                                                   rowmask=rowmask, seed_t=_seed_t(word))
        log = E.DROP_LOG
    finally:
        E.DROP_LOG = None
    ((mean * up[0].cuda()).sum() + (log_std * up[1].cuda()).sum() + (log_dur * up[2].cuda()).sum()).backward()
    torch.cuda.synchronize()
    grads = {k: p_.grad.detach().cpu() for k, p_ in P.items() if k.startswith("layer_Dict.Encoder") and p_.grad is not None}
    return [t.detach().cpu() for t in (mean, log_std, log_dur)], grads, log, launch_counts()


def _oracle_encoder(model, cfg, tokens, tl, speakers, up, drop):
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items() if k.startswith(("layer_Dict.Encoder", "layer_Dict.LUT"))}
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    tmask = O.mask_from_lengths(tl, tokens.shape[1]).double()
    spk = F.embedding(speakers, sd["layer_Dict.LUT.weight"]) if speakers is not None else None
    mean, log_std, log_dur = O.encoder(sdg, tokens, tmask, cfg, spk, None, drop=drop)
    ((mean * up[0].double()).sum() + (log_std * up[1].double()).sum() + (log_dur * up[2].double()).sum()).backward()
    grads = {k: v.grad for k, v in sdg.items() if k.startswith("layer_Dict.Encoder") and v.grad is not None}
    return [t.detach() for t in (mean, log_std, log_dur)], grads


def _assert_encoder_grads(grads, wgrads, tol=5e-3):
    """Every encoder parameter gradient within `tol` of the float64 oracle's, relative to the tensor's largest entry.  Key.bias is the exception that has
    no largest entry: a constant added to every key shifts all scores of a query alike and softmax cancels it (dropout sits behind the softmax), so
    its true gradient is ZERO - the float64 oracle holds 1e-17, the fp32 kernels the rounding residue of the same sums that form Key.weight's gradient.
    It is therefore bounded by `tol` of Key.weight's largest gradient entry, and the oracle's own value by 1e-9 of it."""
    worst = ("", 0.0)
    for k, w_ in wgrads.items():
        got = grads.get(k, torch.zeros_like(w_)).double()
        if k.endswith("Key.bias"):
            scale = wgrads[k[:-len("bias")] + "weight"].abs().max().item()
            assert w_.abs().max().item() <= 1e-9 * scale, (k, w_.abs().max().item(), scale)
            err = got.abs().max().item() / scale
        else:
            err = (got - w_).abs().max().item() / (w_.abs().max().item() + 1e-6)
        worst = max(worst, (k, err), key=lambda t: t[1])
        assert err <= tol, (k, err)
    return worst


def _check_mask_statistics(hook):
    """Whole-tensor keep fractions, and the correlation of every two sites of equal shape in one forward: |corr| sqrt(N) <= 5."""
    by_shape = {}
    for site, (full, (kind, p, shape)) in hook.masks.items():
        _keep_stats(full, p)
        by_shape.setdefault(shape, []).append((site, full.ne(0).double().flatten()))
    pairs = 0
    for shape, sites in by_shape.items():
        for i in range(len(sites)):
            for j in range(i + 1, len(sites)):
                a, b = sites[i][1], sites[j][1]
                a, b = a - a.mean(), b - b.mean()
                corr = (a @ b / (a.norm() * b.norm())).item()
                assert abs(corr) * math.sqrt(a.numel()) <= 5, (sites[i][0], sites[j][0], corr)
                pairs += 1
    return pairs


ENC_CASES = {"4x120": (4, 120, [120, 104, 75, 31]), "2x202": (2, 202, [202, 137])}


def _tokens(B, T, lens, seed):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, 35, (B, T), generator=g)
    for b in range(B):
        tokens[b, lens[b]:] = 1
    return tokens, torch.tensor(lens)


@pytest.mark.parametrize("mode,fname", [("Vanilla", "tiny_vanilla.npz"), ("SE", "tiny_se.npz")])
def test_tiny_encoder_train_mode_f32(mode, fname):
    """The tiny golden encoders (SE: conditioned duration predictor) in train mode with the yaml's rates, f32, against the oracle under the same masks:
    outputs within 1e-4, every encoder parameter gradient within 5e-3 of its largest entry (the eval-mode bars of tests/test_gpu_fullsize.py)."""
    from glow_tts_amd import ops
    sd, _, r = load_case(fname)
    hp = tiny_hp_dict(mode)
    hp["HIP_Precision"] = "f32"
    model = _make_model(hp, sd)
    cfg = tiny_cfg(mode)
    tokens, tl = torch.from_numpy(r["tokens"]), torch.from_numpy(r["token_lengths"])
    speakers = torch.from_numpy(r["speakers"]) if "speakers" in r else None
    B, T = tokens.shape
    up = _upstream(B, cfg.mel_dim, T, 5)
    outs, grads, log, _ = _hip_encoder(model, tokens, tl, speakers, ops.F32, True, up)
    hook = DM.EncoderMasks(log, model.hp.Encoder, WORD, B, T)
    want, wgrads = _oracle_encoder(model, cfg, tokens, tl, speakers, up, hook)
    hook.check_log()
    assert len(hook.called) == cfg.prenet_stacks + 4 * cfg.enc_stacks + cfg.dp_stacks
    for name, a, b in zip(("mean", "log_std", "log_dur"), outs, want):
        assert (a.double() - b).abs().max().item() <= 1e-4, (name, (a.double() - b).abs().max().item())
    _assert_encoder_grads(grads, wgrads)
    # eval mode is another network: the masks were applied
    ev, _, log0, _ = _hip_encoder(model, tokens, tl, speakers, ops.F32, False, up)
    assert log0 == [] and (ev[2] - outs[2]).abs().max() > 1e-3


@pytest.fixture(scope="module")
def full_encoder():
    model = _make_model(_full_hp("f32"), seed=2024)
    _perturb_encoder(model, 3)
    return model, O.Cfg.from_yaml_dict(_full_hp("f32"))


@pytest.mark.parametrize("case", list(ENC_CASES))
def test_full_width_encoder_train_mode_f32(full_encoder, case):
    """Full width (C = 192, 6 layers, the shipped rates 0.5 / 0.1 / 0.1), f32: B = 4 x 120 tokens ragged (single-workgroup attention kernels) and
    B = 2 x 202 tokens (the long attention kernels), against the oracle under the same masks.  Outputs within 1e-4, every encoder parameter gradient
    within 5e-3 of its largest entry.  Also: all site seeds distinct, whole-tensor keep fractions within 5 sigma, |corr| sqrt(N) <= 5 between every
    two sites of equal shape.  Observed: 2e-6 on every tensor, except that the 4 x 120 case holds one ReLU near-tie in the duration predictor's second
    conv (float64 pre-activation + 1.8e-7, frame 10 of utterance 1, channel 210): fp32 cuts it, and that one element is 3.9e-3 of CRND_1.Conv.weight's
    largest gradient entry - inside the bar, and not a defect."""
    from glow_tts_amd import ops
    model, cfg = full_encoder
    B, T, lens = ENC_CASES[case]
    tokens, tl = _tokens(B, T, lens, 31 + T)
    up = _upstream(B, cfg.mel_dim, T, 7 + T)
    outs, grads, log, counts = _hip_encoder(model, tokens, tl, None, ops.F32, True, up)
    hook = DM.EncoderMasks(log, model.hp.Encoder, WORD, B, T)
    want, wgrads = _oracle_encoder(model, cfg, tokens, tl, None, up, hook)
    hook.check_log()
    assert len(hook.called) == 3 + 4 * 6 + 2
    assert _check_mask_statistics(hook) >= 100
    fam = "attn_fwd_mfma<96,f32>" if T + 4 <= 128 else "attn_fwd_long<96>"
    assert counts.get(fam, 0) == 6 and counts.get(fam.replace("fwd", "bwd"), 0) == 6, {k: v for k, v in counts.items() if k.startswith("attn")}
    for name, a, b in zip(("mean", "log_std", "log_dur"), outs, want):
        assert (a.double() - b).abs().max().item() <= 1e-4, (name, (a.double() - b).abs().max().item())
    print(f"train mode, f32, full-width encoder {case}: worst gradient {_assert_encoder_grads(grads, wgrads)}")


@pytest.mark.parametrize("case", list(ENC_CASES))
def test_full_width_encoder_train_mode_bf16_block_path(full_encoder, case):
    """The benchmarked path: bf16-stored rows, two hand-ordered autograd nodes per layer (conv_fn.AttentionBlock / FFNBlock) whose backward chains route
    the dropout gates through LayerNorm's backward and a data-gradient conv's epilogue; `proj_ln` and `ln_qkv` fused launches (asserted from the launch
    log).  Against the float64 oracle under the same masks: every encoder gradient cosine >= 0.99 and norm ratio in [0.95, 1.05], log_dur within 3e-2 -
    the bars tests/test_gpu_fullsize.py::test_full_size_bf16_nll_within_1e3 holds in eval mode.  The same case runs at p = 0 first.
    (Key.bias: softmax cancels a constant added to every key - its true gradient is zero and both sides hold rounding noise only.)

    Measured on an MI355X (worst encoder gradient tensor; norm ratio over all of them; log_dur): 4 x 120 tokens: train 0.9960, 0.9955 .. 1.0070, 1.6e-3
    (p = 0: 0.9949, 0.9857 .. 1.0107, 1.4e-3); 2 x 202 tokens: train 0.9964, 0.9914 .. 1.0124, 2.1e-3 (p = 0: 0.9935, 0.9939 .. 1.0086, 1.2e-3).  Dropout
    costs this path nothing; no bar had to move."""
    from glow_tts_amd import ops
    model, cfg = full_encoder
    B, T, lens = ENC_CASES[case]
    tokens, tl = _tokens(B, T, lens, 31 + T)
    up = _upstream(B, cfg.mel_dim, T, 7 + T)
    tmask = O.mask_from_lengths(tl, T)
    report = {}
    for training in (False, True):
        outs, grads, log, counts = _hip_encoder(model, tokens, tl, None, ops.BF16, training, up)
        assert counts.get("proj_ln<192>", 0) == 6 and counts.get("ln_qkv<192>", 0) == 5, {k: v for k, v in counts.items() if "ln" in k}
        fam = "attn_fwd_mfma<96,bf16>" if T + 4 <= 128 else "attn_fwd_long<96>"
        assert counts.get(fam, 0) == 6 and counts.get(fam.replace("fwd", "bwd"), 0) == 6, {k: v for k, v in counts.items() if k.startswith("attn")}
        assert counts.get("conv_dma<LINEAR,3>", 0) >= 24, {k: v for k, v in counts.items() if "conv" in k}
        hook = DM.EncoderMasks(log, model.hp.Encoder, WORD, B, T) if training else None
        assert training or log == []
        want, wgrads = _oracle_encoder(model, cfg, tokens, tl, None, up, hook)
        if training:
            hook.check_log()
            assert len(hook.called) == 3 + 4 * 6 + 2
        dld = ((outs[2].double() - want[2]) * tmask).abs().max().item()
        rows = []
        for k, w_ in wgrads.items():
            if w_.abs().max() == 0 or k.endswith("Key.bias"):
                continue
            cos, ratio = _cos_ratio(grads[k], w_)
            rows.append((cos, ratio, k))
        rows.sort()
        lo, hi = min(r_[1] for r_ in rows), max(r_[1] for r_ in rows)
        report[training] = (rows[0], lo, hi, dld)
        print(f"bf16 block path {case}, {'train' if training else 'p = 0'}: worst cosine {rows[0][0]:.5f} ({rows[0][2]}), norm ratio {lo:.4f} .. {hi:.4f}, "
              f"|d log_dur| {dld:.2e}, mean {(outs[0].double() - want[0]).abs().max().item():.2e}")
        assert dld <= 3e-2, dld
        for cos, ratio, k in rows:
            assert cos >= 0.99 and 0.95 <= ratio <= 1.05, (training, k, cos, ratio)


# ------------------------------------------------------------------------------------------------ (e) the whole model in train()
def _record_seed_words(monkeypatch):
    from glow_tts_amd import decoder as D
    words, orig = [], D.step_seed

    def recording(device):
        w = orig(device)
        words.append(w)
        return w
    monkeypatch.setattr(D, "step_seed", recording)
    return words


def _whole_model_train_step(model, cfg, sd, tokens, tl, mels, ml, speakers, pitches, words, gr):
    """One train() forward + losses + backward on the HIP path and on the oracle under the masks of the step's one seed word."""
    from glow_tts_amd import encoder as E
    from glow_tts_amd.modules import MLE_Loss
    hp = model.hp
    model.train()
    model.zero_grad()
    c = lambda t: None if t is None else t.cuda()
    E.DROP_LOG = []
    try:
        z, mel_mean, mel_log_std, log_dets, log_dur, log_dur_t, attn, classified = model(c(tokens), c(tl), c(mels), c(ml), c(speakers), None, c(pitches))
        log = E.DROP_LOG
    finally:
        E.DROP_LOG = None
    mle = MLE_Loss(hp)(z=z, mean=mel_mean, std=mel_log_std, log_dets=log_dets, lengths=c(ml))
    length = F.mse_loss(log_dur, log_dur_t)
    total = mle + length
    if gr:
        ce = F.cross_entropy(classified, c(speakers))
        total = total + ce
    total.backward()
    torch.cuda.synchronize()
    assert len(words) == 1, "one seed word per step"
    word = int(words[0].item())
    B, T = tokens.shape
    hook = DM.EncoderMasks(log, hp.Encoder, word, B, T)
    p_wn = float(hp.Decoder.Affine_Coupling.WaveNet.Dropout_Rate)
    wn_masks = {}

    def wn_drop(pfx, layer, ins):
        flow = int(pfx.split(".Flows.")[1].split(".")[0])
        assert (flow, layer) not in wn_masks
        wn_masks[(flow, layer)] = DM.hip_keep_multipliers(word, flow, layer, ins.shape[0], ins.shape[2], cfg.wn_channels, p_wn)
        return ins * wn_masks[(flow, layer)].to(ins.dtype)
    sdg = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    o = O.forward_train(sdg, cfg, tokens, tl, mels, ml, speakers, pitches=pitches, enc_drop=hook, wn_drop=wn_drop)
    hook.check_log()
    assert len(wn_masks) == cfg.n_flows * cfg.wn_layers
    losses = O.train_losses(o, ml, cfg, speakers if gr else None)
    sum(losses).backward()
    cpu = lambda t: t.detach().cpu()
    got = dict(z=cpu(z), mel_mean=cpu(mel_mean), mel_log_std=cpu(mel_log_std), log_dets=cpu(log_dets), log_dur=cpu(log_dur), log_dur_target=cpu(log_dur_t),
               attn=cpu(attn), mle=mle.item(), length=length.item(), classified=None if classified is None else cpu(classified))
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return got, grads, o, losses, sdg, word


@pytest.mark.parametrize("mode,fname", [("Vanilla", "tiny_vanilla.npz"), ("SE", "tiny_se.npz"), ("PE", "tiny_pe.npz"), ("GR", "tiny_gr.npz")])
def test_whole_model_train_step_f32_under_the_same_masks(mode, fname, monkeypatch):
    """`model.train()` with the yaml's rates (prenet 0.5, transformer 0.1, duration predictor 0.1, WaveNet 0.05), f32, every Mode: forward, MLE + duration
    (+ speaker CE in GR) losses, backward, against `O.forward_train` with both hooks - the encoder masks and the WaveNet masks restated from the step's
    ONE seed word, which the encoder's stream and the decoder's stream must both have read.  Alignment equal, outputs and every gradient at the bars of
    tests/test_gpu_model.py::test_train_forward_losses_grads_f32.  Two consecutive train() forwards draw different words."""
    sd, _, r = load_case(fname)
    hp = tiny_hp_dict(mode)
    hp["HIP_Precision"] = "f32"
    model = _make_model(hp, sd)
    cfg = tiny_cfg(mode)
    t = lambda k: torch.from_numpy(r[k]) if k in r else None
    words = _record_seed_words(monkeypatch)
    torch.manual_seed(1234)
    got, grads, o, losses, sdg, word = _whole_model_train_step(model, cfg, sd, t("tokens"), t("token_lengths"), t("mels"), t("mel_lengths"), t("speakers"),
                                                               t("pitches"), words, mode == "GR")
    assert torch.equal(got["attn"], o["attn"]), "alignment differs from the oracle's under the same masks"
    for key, tol in [("z", 1e-4), ("mel_mean", 1e-4), ("mel_log_std", 1e-4), ("log_dur", 1e-4), ("log_dur_target", 1e-5), ("log_dets", 1e-3)]:
        assert (got[key] - o[key].detach()).abs().max() <= tol, (key, (got[key] - o[key].detach()).abs().max().item())
    assert abs(got["mle"] - losses[0].item()) <= 1e-4 and abs(got["length"] - losses[1].item()) <= 1e-4
    if mode == "GR":
        assert (got["classified"] - o["classified"].detach()).abs().max() <= 1e-4
    worst = ("", 0.0)
    for k, p in model.named_parameters():
        want = sdg[k].grad
        if want is None:
            continue
        g_ = grads[k] if k in grads else torch.zeros_like(want)
        err = (g_ - want).abs().max().item() / (want.abs().max().item() + 1e-5)
        worst = max(worst, (k, err), key=lambda x: x[1])
        assert err < 5e-3, (k, err)
    print(f"train mode, f32, whole tiny {mode} model: worst relative gradient error {worst}")
    # train mode is another network than eval mode (the fixture's eval outputs), and the next step draws another word
    assert (got["log_dur"] - torch.from_numpy(r["log_dur"])).abs().max() > 1e-3
    with torch.no_grad():
        c = lambda v: None if v is None else v.cuda()
        model(c(t("tokens")), c(t("token_lengths")), c(t("mels")), c(t("mel_lengths")), c(t("speakers")), None, c(t("pitches")))
    assert len(words) == 2 and int(words[1].item()) != word


def test_whole_full_size_model_train_step_f32_under_the_same_masks(monkeypatch):
    """The default Hyper_Parameters model (12 flows x 4 WaveNet layers x 192 channels, 6 encoder layers) by the fixture recipe of
    tests/test_gpu_fullsize.py (seeded, End layers not the identity, ActNorm initialised from the batch by the f32 HIP path), B = 4 ragged, 120 tokens /
    800 frames, one train() step in f32 against `O.forward_train` under the masks of the step's one seed word.  Bars: the f32 eval-mode bars of
    tests/test_gpu_fullsize.py (alignment exact, encoder outputs 1e-4, z 1e-3, log-determinants 1e-3 relative, losses 1e-3, every gradient 5e-3) - at
    this size a log-determinant is a sum of 64 000 terms of magnitude 1e4, where fp32 resolves 1e-3: the tiny model's absolute bars are below either
    side's arithmetic."""
    B, TT, TM = 4, 120, 800
    tok_len, mel_len = [120, 104, 75, 31], [800, 702, 500, 210]
    d = _full_hp("f32")
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    torch.manual_seed(2024)
    model = GlowTTS(Recursive_Parse(d))
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for f in model.layer_Dict["Decoder"].layer_Dict["Flows"]:
            end = f.layers[2].layer_Dict["End"]
            end.weight.copy_(torch.randn(end.weight.shape, generator=g) * 0.02)
            end.bias.copy_(torch.randn(end.bias.shape, generator=g) * 0.02)
            f.layers[1].weight.add_(0.05 * torch.randn(4, 4, generator=g))
    tokens = torch.randint(0, 35, (B, TT), generator=g)
    mels = (torch.randn(B, 80, TM, generator=g) * 1.5).clamp(-4, 4)
    tl, ml = torch.tensor(tok_len), torch.tensor(mel_len)
    for b in range(B):
        tokens[b, tok_len[b]:] = 1
        mels[b, :, mel_len[b]:] = -4.0
    model = model.cuda().eval()
    with torch.no_grad():
        model(tokens.cuda(), tl.cuda(), mels.cuda(), ml.cuda(), None, None, None)        # first call: ActNorm data init (Modules.py:685-687)
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    cfg = O.Cfg.from_yaml_dict(d)
    words = _record_seed_words(monkeypatch)
    torch.manual_seed(4321)
    got, grads, o, losses, sdg, word = _whole_model_train_step(model, cfg, sd, tokens, tl, mels, ml, None, None, words, False)
    tmask, mmask = O.mask_from_lengths(tl, TT), O.mask_from_lengths(ml, TM)
    assert torch.equal(got["attn"], o["attn"]), f"{(got['attn'] != o['attn']).any(1).sum().item()} frames aligned differently"
    for key, m, tol in [("mel_mean", mmask, 1e-4), ("mel_log_std", mmask, 1e-4), ("log_dur", tmask, 1e-4), ("z", mmask, 1e-3)]:
        assert ((got[key] - o[key].detach()) * m).abs().max() <= tol, (key, ((got[key] - o[key].detach()) * m).abs().max().item())
    assert (got["log_dur_target"] - o["log_dur_target"].detach()).abs().max() <= 1e-5
    ldo = o["log_dets"].detach()
    assert ((got["log_dets"] - ldo).abs() <= 1e-3 * ldo.abs().clamp_min(1.0)).all()
    assert abs(got["mle"] - losses[0].item()) <= 1e-3 and abs(got["length"] - losses[1].item()) <= 1e-3
    worst = ("", 0.0)
    for k, p in model.named_parameters():
        want = sdg[k].grad
        if want is None:
            continue
        g_ = grads[k] if k in grads else torch.zeros_like(want)
        err = (g_ - want).abs().max().item() / (want.abs().max().item() + 1e-6)
        worst = max(worst, (k, err), key=lambda x: x[1])
        assert err <= 5e-3, (k, err)
    print(f"train mode, f32, whole full-size model: NLL {got['mle']:.6f} vs oracle {losses[0].item():.6f}; worst gradient {worst}")
