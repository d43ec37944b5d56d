"""Long texts: the eval-mode attention core for any Tp (glowtts_rpr_attention_fwd_eval) and everything on the inference path that runs on
it - GlowTTS.inference on prompts of 300 to 700 tokens against the oracle, the full-width encoder at 600 tokens, batch invariance, serving
beyond the largest mel bucket (child process: it captures hipGraphs) and `Inference.py` on a 600-character prompt (child process)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import launch_counts, launch_reset, load_case, tiny_cfg, tiny_hp_dict
from oracle import glowtts_ref as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def banded_ref(qkv, relk, relv, rowmask, B, Tp, H, win):
    """float64 restatement of oracle.rpr_attention's banded form on fused rows [B*Tp, 3*H*D] -> [B*Tp, H*D] (no projection)."""
    D = qkv.shape[1] // (3 * H)
    x = qkv.double().view(B, Tp, 3, H, D)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))                     # [B, H, Tp, D]
    relk, relv = relk.double(), relv.double()
    idx = torch.arange(Tp, device=qkv.device)
    dmat = idx[None, :] - idx[:, None]                                           # d = j - i
    band = dmat.abs() <= win
    gather = (dmat.clamp(-win, win) + win).view(1, 1, Tp, Tp).expand(B, H, Tp, Tp)
    scores = (q @ k.transpose(2, 3) + torch.gather(q @ relk.t(), 3, gather) * band) / math.sqrt(D)
    m = rowmask.double().view(B, Tp)
    scores = scores.masked_fill((m[:, :, None] * m[:, None, :]).unsqueeze(1) == 0, -1e4)
    pr = torch.softmax(scores, dim=-1)
    out = pr @ v
    pb = torch.zeros(B, H, Tp, 2 * win + 1, device=qkv.device, dtype=torch.float64)
    for d in range(-win, win + 1):
        lo, hi = max(0, -d), min(Tp, Tp - d)
        if hi > lo:
            ii = torch.arange(lo, hi, device=qkv.device)
            pb[:, :, ii, d + win] = pr[:, :, ii, ii + d]
    out = out + pb @ relv
    return out.transpose(1, 2).reshape(B * Tp, H * D)


def attn_case(Tp, D, win, seed, B=3, H=2):
    """Random operands with ragged row masks: utterance 0 fully valid, 1 a single valid row, 2 (if any) about two thirds valid behind pad rows."""
    g = torch.Generator().manual_seed(seed)
    rowmask = torch.zeros(B, Tp)
    rowmask[0] = 1.0
    if B > 1:
        rowmask[1, min(2, Tp - 1)] = 1.0
    if B > 2:
        n = max(1, (2 * Tp) // 3)
        lo = min(2, Tp - 1)
        rowmask[2, lo:min(Tp, lo + n)] = 1.0
    for b in range(3, B):                                        # more utterances: random lengths behind two pad rows
        n = int(torch.randint(1, max(2, Tp - 3), (1,), generator=g))
        rowmask[b, 2:2 + n] = 1.0
    qkv = (torch.randn(B * Tp, 3 * H * D, generator=g) * 0.6).cuda()
    relk = (torch.randn(2 * win + 1, D, generator=g) * D ** -0.5).cuda()
    relv = (torch.randn(2 * win + 1, D, generator=g) * D ** -0.5).cuda()
    return qkv, relk, relv, rowmask.reshape(-1).cuda()


def compare(got, want, rowmask, precision):
    valid = rowmask[:, None] > 0
    a, b = got.double()[valid.expand_as(got)], want[valid.expand_as(want)]
    err = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
    cos = (a @ b / (a.norm() * b.norm() + 1e-30)).item()
    if precision == 0:
        assert err < 2e-5, err
    else:
        assert err < 2e-2 and cos > 0.999, (err, cos)
    return err


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("win", [0, 4])
@pytest.mark.parametrize("D", [16, 64, 96])
@pytest.mark.parametrize("Tp", [1, 5, 64, 129, 257, 300, 511, 1024, 2052])
def test_eval_attention_against_float64(Tp, D, win, precision):
    """The new entry through the C ABI against the float64 banded form, valid rows only; every row of the output finite."""
    from glow_tts_amd.conv_fn import rpr_attention_eval
    B, H = 3, 2
    qkv, relk, relv, rowmask = attn_case(Tp, D, win, 7 * Tp + D + win)
    launch_reset()
    out = rpr_attention_eval(qkv, relk, relv, rowmask, B, Tp, H, win, precision)
    torch.cuda.synchronize()
    counts = launch_counts()
    kind = f"attn_fwd_eval_mfma<{D},{'bf16' if precision else 'f32'}," if D in (64, 96) else "attn_fwd_eval_gen"
    assert sum(v for k, v in counts.items() if k.startswith(kind)) == 1, counts
    assert torch.isfinite(out).all()
    compare(out, banded_ref(qkv, relk, relv, rowmask, B, Tp, H, win), rowmask, precision)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("B,Tp,D,nwv", [(3, 300, 96, 2), (8, 700, 64, 2), (32, 520, 96, 4), (56, 300, 64, 4), (32, 2052, 96, 4), (64, 1000, 64, 4)])
def test_eval_attention_multiwave_workgroups(B, Tp, D, nwv, precision):
    """Both workgroup shapes of the MFMA path: 2 waves below 512 32-query tiles (B H ceil(Tp / 32)), 4 from there (batched long texts), the variant
    asserted from the launch log; Tp not a multiple of the workgroup's queries, ragged utterances; every valid row against the float64 banded form."""
    from glow_tts_amd.conv_fn import rpr_attention_eval
    H, win = 2, 4
    qkv, relk, relv, rowmask = attn_case(Tp, D, win, 13 * Tp + B + D, B=B)
    launch_reset()
    out = rpr_attention_eval(qkv, relk, relv, rowmask, B, Tp, H, win, precision)
    torch.cuda.synchronize()
    counts = launch_counts()
    assert counts.get(f"attn_fwd_eval_mfma<{D},{'bf16' if precision else 'f32'},{nwv}>", 0) == 1, counts
    assert torch.isfinite(out).all()
    compare(out, banded_ref(qkv, relk, relv, rowmask, B, Tp, H, win), rowmask, precision)


@pytest.mark.parametrize("Tp,D", [(64, 96), (124, 96), (100, 64), (204, 96), (256, 64), (200, 16), (5, 16)])
def test_eval_attention_agrees_with_training_kernels(Tp, D):
    """At Tp <= 256 the new kernel and the existing ones give the same output on the same inputs (f32 bar), and RPRAttention keeps
    launching only the existing kernels there."""
    from glow_tts_amd.conv_fn import RPRAttention, rpr_attention_eval
    B, H, win = 3, 2, 4
    qkv, relk, relv, rowmask = attn_case(Tp, D, win, 11 * Tp + D)
    launch_reset()
    with torch.no_grad():
        old = RPRAttention.apply(qkv, relk.unsqueeze(0), relv.unsqueeze(0), rowmask, B, Tp, H, win, 0.0, 0, None)
    torch.cuda.synchronize()
    counts = launch_counts()
    assert sum(v for k, v in counts.items() if k.startswith("attn_fwd_eval")) == 0, counts
    if D in (64, 96) and Tp <= 128:
        assert counts.get(f"attn_fwd_mfma<{D},f32>", 0) == 1, counts
    new = rpr_attention_eval(qkv, relk, relv, rowmask, B, Tp, H, win, 0)
    compare(new, old.double(), rowmask, 0)


@pytest.mark.parametrize("D", [96, 16])
def test_rpr_attention_dispatch_beyond_256(D):
    """Tp > 256 under no_grad: RPRAttention takes the new kernel only, with no autograd node; with grad enabled and an input that requires it
    the call keeps its current behaviour (the training kernels' Tp <= 256 limit)."""
    from glow_tts_amd import _lib
    from glow_tts_amd.conv_fn import RPRAttention
    B, H, win, Tp = 2, 2, 4, 300
    qkv, relk, relv, rowmask = attn_case(Tp, D, win, 5 + D, B=B)
    launch_reset()
    with torch.no_grad():
        out = RPRAttention.apply(qkv, relk.unsqueeze(0), relv.unsqueeze(0), rowmask, B, Tp, H, win, 0.0, 0, None)
    torch.cuda.synchronize()
    counts = launch_counts()
    assert sum(v for k, v in counts.items() if k.startswith("attn_fwd_eval")) == 1, counts
    assert sum(v for k, v in counts.items() if k.startswith("attn_fwd_mfma") or k.startswith("attn_bwd")) == 0, counts
    assert out.grad_fn is None
    compare(out, banded_ref(qkv, relk, relv, rowmask, B, Tp, H, win), rowmask, 0)
    qg = qkv.clone().requires_grad_(True)
    with pytest.raises(_lib.GlowTTSHipError):
        RPRAttention.apply(qg, relk.unsqueeze(0), relv.unsqueeze(0), rowmask, B, Tp, H, win, 0.0, 0, None)


def test_eval_attention_keeps_no_probability_matrix():
    """B = 1, Tp = 4096, D = 96: the call's peak allocation above its inputs and output is under 16 MiB (P alone would be 128 MiB)."""
    from glow_tts_amd.conv_fn import rpr_attention_eval
    B, H, win, Tp, D = 1, 2, 4, 4096, 96
    qkv, relk, relv, rowmask = attn_case(Tp, D, win, 3, B=B)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = rpr_attention_eval(qkv, relk, relv, rowmask, B, Tp, H, win, 0)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base - out.numel() * 4
    assert extra < 16 * 2 ** 20, extra
    sel = torch.arange(0, Tp, 97, device="cuda")                  # spot rows against float64 (the full 4096^2 reference is the expensive part)
    want = banded_ref(qkv, relk, relv, rowmask, B, Tp, H, win)
    compare(out[sel], want[sel], rowmask[sel], 0)


# ------------------------------------------------------------------------------------------------ whole models
TINY = [("Vanilla", "tiny_vanilla.npz"), ("SE", "tiny_se.npz"), ("PE", "tiny_pe.npz"), ("GR", "tiny_gr.npz")]


def build_tiny(mode, precision, sd):
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    hp = tiny_hp_dict(mode)
    hp["HIP_Precision"] = precision
    model = GlowTTS(Recursive_Parse(hp))
    model.load_state_dict(sd)
    for f in model.layer_Dict["Decoder"].layer_Dict["Flows"]:
        f.layers[0].initialized = True
    return model.cuda().eval()


def long_tokens(lengths, vocab, g):
    T = max(lengths)
    tokens = torch.randint(1, vocab, (len(lengths), T), generator=g)
    for b, n in enumerate(lengths):
        tokens[b, n:] = 0
    return tokens, torch.tensor(lengths)


@pytest.mark.parametrize("mode,fname", TINY)
def test_tiny_inference_long_prompts_match_oracle(mode, fname):
    """GlowTTS.inference with 300- and 700-token prompts in one ragged batch (f32, injected noise) against oracle.inference: lengths and
    attentions equal, mels within the f32 long-form bar."""
    sd, _, r = load_case(fname)
    model = build_tiny(mode, "f32", sd)
    vocab = sd["layer_Dict.Encoder.layer_Dict.Embedding.weight"].shape[0]
    g = torch.Generator().manual_seed(31)
    tokens, tl = long_tokens([300, 700], vocab, g)
    B = 2
    ls = torch.tensor([1.0, 0.8])
    spk = torch.tensor([1, 3]) if mode in ("SE", "GR") and "speakers" in r else None
    pm = torch.from_numpy(r["mels"][:B]) if mode in ("PE", "GR") else None
    pl = torch.from_numpy(r["mel_lengths"][:B]) if mode in ("PE", "GR") else None
    pit = torch.from_numpy(r["pitches"][:B]) if mode == "GR" else None
    kw = dict(mels_for_prosody=pm, mel_lengths_for_prosody=pl) if pm is not None else {}
    if pit is not None:
        kw.update(pitches=pit, pitch_lengths=pl)
    noise = torch.randn(B, 12, 16384, generator=g)
    want, wl, wa = O.inference(sd, tiny_cfg(mode), tokens, tl, noise, ls, noise_scale=0.667, speakers=spk, **kw)
    c = lambda t: None if t is None else t.cuda()
    mels, lengths, attn = model.inference(tokens.cuda(), tl.cuda(), c(pm), c(pl), c(spk), None, c(pit), c(pl) if pit is not None else None,
                                          noise_scale=0.667, length_scale=ls.cuda(), noises=noise.cuda())
    torch.cuda.synchronize()
    assert torch.equal(lengths.cpu(), wl), (lengths, wl)
    assert attn.shape == wa.shape and torch.equal(attn.cpu().to(wa.dtype), wa)
    err = (mels.cpu() - want).abs().max().item()
    assert mels.shape == want.shape and err <= 2e-4, err


def test_batch_invariance_long_utterance():
    """A 400-token utterance alone and beside two short ones (padded batch, Tp = 404: the new kernel): equal length and alignment, mels within
    the f32 bar."""
    sd, _, _ = load_case("tiny_vanilla.npz")
    model = build_tiny("Vanilla", "f32", sd)
    vocab = sd["layer_Dict.Encoder.layer_Dict.Embedding.weight"].shape[0]
    g = torch.Generator().manual_seed(41)
    tokens, tl = long_tokens([400, 9, 57], vocab, g)
    noise = torch.randn(3, 12, 16384, generator=g)
    ls = torch.ones(3)
    launch_reset()
    with torch.no_grad():
        m1, l1, a1 = model.inference(tokens[:1].cuda(), tl[:1].cuda(), noise_scale=0.667, length_scale=ls[:1].cuda(), noises=noise[:1].cuda())
        m3, l3, a3 = model.inference(tokens.cuda(), tl.cuda(), noise_scale=0.667, length_scale=ls.cuda(), noises=noise.cuda())
    torch.cuda.synchronize()
    assert sum(v for k, v in launch_counts().items() if k.startswith("attn_fwd_eval")) > 0
    n = int(l1[0])
    assert int(l3[0]) == n
    T1 = m1.shape[2]
    assert torch.equal(a3[0, :400, :a1.shape[2]], a1[0]) and not a3[0, :, a1.shape[2]:].any()
    assert (m3[0, :, :T1] - m1[0]).abs().max().item() <= 2e-4


def test_full_width_encoder_600_tokens():
    """Default-size model (D = 96): encoder outputs at 600 tokens against the oracle encoder (f32), the bf16 encoder against f32, and one
    whole f32 inference of a 320-token prompt against the oracle."""
    from glow_tts_amd import encoder
    from test_gpu_benchmarked_sizes import _build, _hp
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(6)
    model = _build("Vanilla", "f32")
    with torch.no_grad():
        for f in model.layer_Dict["Decoder"].layer_Dict["Flows"]:
            end = f.layers[2].layer_Dict["End"]
            end.weight.copy_(torch.randn(end.weight.shape, generator=g) * 0.02)
            end.bias.copy_(torch.randn(end.bias.shape, generator=g) * 0.02)
            f.layers[0].initialized = True
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    cfg = O.Cfg.from_yaml_dict(_hp("Vanilla", "f32"))
    tokens, tl = long_tokens([600, 411], 35, g)
    tmask = O.mask_from_lengths(tl, tokens.shape[1])                   # [B, 1, T]
    with torch.no_grad():
        want = O.encoder(sd, tokens, tmask, cfg)
    outs = {}
    for precision in ("f32", "bf16"):
        m = _build("Vanilla", precision, sd).cuda().eval()
        with torch.no_grad():
            mask = m.Mask_Generate(tl.cuda(), tokens.shape[1])
            outs[precision] = [t.cpu().double() for t in encoder.encoder_forward(m._params(), m.hp, tokens.cuda(), mask, None, None, False,
                                                                                  precision=m.dec_cfg.precision, cache=m._enc_cache)]
        torch.cuda.synchronize()
    valid = tmask.double()
    for name, a, b, c in zip(("mean", "log_std", "log_dur"), outs["f32"], want, outs["bf16"]):
        b = b.double()
        err = ((a - b) * valid).abs().max().item() / max(1.0, b.abs().max().item())
        assert err < 1e-4, (name, err)
        cf, af = (c * valid).flatten(), (a * valid).flatten()
        cos = (cf @ af / (cf.norm() * af.norm() + 1e-30)).item()
        errb = (cf - af).abs().max().item() / max(1.0, af.abs().max().item())
        assert cos > 0.999 and errb < 5e-2, (name, cos, errb)
    # one whole f32 inference at 320 tokens
    tok1, tl1 = long_tokens([320], 35, g)
    noise = torch.randn(1, 80, 8192, generator=g)
    ls = torch.tensor([1.0])
    with torch.no_grad():
        wm, wl, wa = O.inference(sd, cfg, tok1, tl1, noise, ls, noise_scale=0.667)
        m = _build("Vanilla", "f32", sd).cuda().eval()
        mels, lengths, attn = m.inference(tok1.cuda(), tl1.cuda(), noise_scale=0.667, length_scale=ls.cuda(), noises=noise.cuda())
    torch.cuda.synchronize()
    assert torch.equal(lengths.cpu(), wl) and torch.equal(attn.cpu().to(wa.dtype), wa)
    assert mels.shape == wm.shape and (mels.cpu() - wm).abs().max().item() <= 2e-4


def test_serving_beyond_the_largest_bucket():
    """tests/long_text_serving_check.py in a child process (it captures hipGraphs)."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "long_text_serving_check.py")], capture_output=True, text=True, timeout=900, cwd=REPO)
    assert out.returncode == 0 and "LONG TEXT SERVING OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_inference_entry_point_long_prompt(tmp_path):
    """`python Inference.py -c <checkpoint> -t prompts.tsv` with a 600-character prompt writes NPY/<label>.npy of shape [T, Mel], T > 2048."""
    import yaml
    from glow_tts_amd import data
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    rng = np.random.default_rng(3)
    words = ["glow", "flow", "speech", "long", "text", "prompt", "model", "voice", "the", "of", "and", "synthesis"]
    text = ""
    while len(text) < 600:
        text += words[int(rng.integers(len(words)))] + " "
    text = text[:599] + "."
    ftext = data.text_filtering(text)
    token_dict = data.make_token_dict([ftext])
    with open(tmp_path / "Token.yaml", "w") as f:
        yaml.dump(token_dict, f)
    hp = tiny_hp_dict("Vanilla")
    hp["Token_Path"] = str(tmp_path / "Token.yaml")
    hp["Encoder"]["Embedding_Tokens"] = len(token_dict)
    with open(tmp_path / "Hyper_Parameters.yaml", "w") as f:
        yaml.dump(hp, f)
    torch.manual_seed(0)
    model = GlowTTS(Recursive_Parse(hp))
    sd = model.state_dict()
    wq = "layer_Dict.Encoder.layer_Dict.Duration_Predictor.layer_Dict.Projection"
    sd[wq + ".weight"].zero_()
    sd[wq + ".bias"].fill_(math.log(4.5))                    # five frames per token: > 3000 frames for > 600 tokens
    torch.save({"Model": sd, "Steps": 0}, tmp_path / "ckpt.pt")
    with open(tmp_path / "prompts.tsv", "w") as f:
        f.write("Label\tText\tLength_Scale\tSpeaker\tGE2E\tProsody\tPitch\n")
        f.write(f"LONG\t{text}\t1.0\t0\tx\tx\tx\n")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(REPO, "Inference.py"), "-c", str(tmp_path / "ckpt.pt"), "-t", str(tmp_path / "prompts.tsv"),
                          "-o", str(tmp_path / "out")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    mel = np.load(tmp_path / "out" / "NPY" / "LONG.npy")
    assert mel.ndim == 2 and mel.shape[1] == 12 and mel.shape[0] > 2048 and np.isfinite(mel).all(), mel.shape


def test_full_width_inverse_path_2000_tokens_20000_frames():
    """The whole inference path at 2 000 tokens and 20 000 frames (default sizes, f32): embedding, prenet / FFN convs, LayerNorms, PriorSplit,
    the duration projection, the alignment expansion and the inverse flows take it; encoder outputs against the oracle encoder, the one-hot
    alignment and the mel's valid / padded frames checked."""
    from glow_tts_amd import encoder
    from test_gpu_benchmarked_sizes import _build, _hp
    torch.manual_seed(8)
    g = torch.Generator().manual_seed(9)
    model = _build("Vanilla", "f32")
    wq = "layer_Dict.Encoder.layer_Dict.Duration_Predictor.layer_Dict.Projection"
    with torch.no_grad():
        model.state_dict()[wq + ".weight"].zero_()
        model.state_dict()[wq + ".bias"].fill_(math.log(9.5))        # ten frames per token
        for f in model.layer_Dict["Decoder"].layer_Dict["Flows"]:
            f.layers[0].initialized = True
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.cuda().eval()
    tokens, tl = long_tokens([2000], 35, g)
    with torch.no_grad():
        mask = model.Mask_Generate(tl.cuda(), tokens.shape[1])
        got = encoder.encoder_forward(model._params(), model.hp, tokens.cuda(), mask, None, None, False, precision=model.dec_cfg.precision,
                                      cache=model._enc_cache)
        want = O.encoder(sd, tokens, O.mask_from_lengths(tl, 2000), O.Cfg.from_yaml_dict(_hp("Vanilla", "f32")))
        for name, a, b in zip(("mean", "log_std", "log_dur"), got, want):
            err = (a.cpu().double() - b.double()).abs().max().item() / max(1.0, b.abs().max().item())
            assert err < 1e-4, (name, err)
        noise = torch.randn(1, 80, 20000, generator=g).cuda()
        mels, lengths, attn = model.inference(tokens.cuda(), tl.cuda(), noise_scale=0.667, noises=noise)
    torch.cuda.synchronize()
    assert int(lengths[0]) == 20000 and mels.shape == (1, 80, 20000) and attn.shape == (1, 2000, 20000)
    assert torch.isfinite(mels).all() and mels.abs().max() < 1e3
    assert torch.equal(attn.sum(1), torch.ones(1, 20000, device="cuda"))
    assert torch.equal(attn[0].argmax(0).cpu(), torch.arange(20000) // 10)
