"""Child process of tests/test_gpu_prior_sample.py::test_graphed_inference_with_seeds (it captures hipGraphs): `GraphedInference(seeds=)` on the tiny
Vanilla model - the same seed twice gives the same bits, new seeds and new scales on a replay of the SAME captured graph change the mel (they are read
from device buffers, not baked in), a prompt alone and beside a much longer one (another bucket) keeps its length and, within the f32 bar, its mel; the
eager path beyond the largest bucket takes the seeds too."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from helpers import load_case                                          # noqa: E402
from test_gpu_prior_sample import build_tiny                           # noqa: E402
from glow_tts_amd.graph_infer import GraphedInference                 # noqa: E402

sd, _, r = load_case("tiny_vanilla.npz")
model = build_tiny("Vanilla", "f32", sd)
vocab = sd["layer_Dict.Encoder.layer_Dict.Embedding.weight"].shape[0]
g = torch.Generator().manual_seed(23)
lengths = [11, 120]
tokens = torch.randint(1, vocab, (2, max(lengths)), generator=g)
tokens[0, lengths[0]:] = 0
tokens, tl = tokens.cuda(), torch.tensor(lengths).cuda()
gi = GraphedInference(model, mel_buckets=(32, 64, 128, 256, 512, 1024))
s1 = torch.tensor([[11, 12]], dtype=torch.int64)
s2 = torch.tensor([[11, 13]], dtype=torch.int64)

# the short prompt alone
a, la, aa = gi(tokens[:1, :lengths[0]], tl[:1], noise_scale=0.667, seeds=s1)
a, aa = a.clone(), aa.clone()
assert len(gi.back) == 1 and list(gi.back)[0][2] == "seeded"
b, lb, _ = gi(tokens[:1, :lengths[0]], tl[:1], noise_scale=0.667, seeds=s1)
b = b.clone()
assert torch.equal(la, lb) and torch.equal(a, b), "the same seed twice differs"
c, lc, _ = gi(tokens[:1, :lengths[0]], tl[:1], noise_scale=0.667, seeds=s2)
c = c.clone()
assert len(gi.back) == 1, "a new seed captured a new graph"
n = (int(la[0]) // 2) * 2
assert n >= 4 and torch.equal(la, lc) and not torch.equal(a[:, :, :n], c[:, :, :n]), "new seeds on the same graph left the mel unchanged"
d, _, _ = gi(tokens[:1, :lengths[0]], tl[:1], noise_scale=torch.tensor([0.2]), seeds=s1)
assert len(gi.back) == 1 and not torch.equal(a[:, :, :n], d[:, :, :n]), "a new noise scale on the same graph left the mel unchanged"
# eager reference of the same call: the graph computes what the eager seeded path computes
e, le, ae = model.inference(tokens[:1, :lengths[0]], tl[:1], noise_scale=0.667, seeds=s1)
assert torch.equal(le, la) and torch.equal(ae, aa) and (e - a).abs().max().item() <= 1e-5, (e - a).abs().max().item()

# beside a much longer prompt: another bucket, a padded token axis
both = torch.cat([s1, torch.tensor([[99, 98]], dtype=torch.int64)])
m2, l2, a2 = gi(tokens, tl, noise_scale=0.667, seeds=both)
torch.cuda.synchronize()
buckets = sorted(k[1] for k in gi.back)
assert len(buckets) == 2 and buckets[0] < buckets[1], buckets
assert int(l2[0]) == int(la[0]), (l2, la)
assert torch.equal(a2[0, :lengths[0], :aa.shape[2]], aa[0]) and not a2[0, :, aa.shape[2]:].any()
err = (m2[0, :, :n] - a[0, :, :n]).abs().max().item()
assert err <= 2e-4, err

# beyond the largest bucket: the eager back half takes seeds and scales through
small = GraphedInference(model, mel_buckets=(8,))
f, lf, _ = small(tokens, tl, noise_scale=0.667, seeds=both)
torch.cuda.synchronize()
assert len(small.back) == 0 and torch.equal(lf, l2) and (f - m2).abs().max().item() <= 1e-5
print("SEEDED GRAPH OK")
