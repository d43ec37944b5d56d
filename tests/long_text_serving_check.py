"""Child of tests/test_gpu_long_text.py::test_serving_beyond_the_largest_bucket (it captures hipGraphs; a failed capture takes the process down).
`GraphedInference` on a prompt of more than 252 tokens whose mel runs past the largest bucket (2048 frames): the back half runs eagerly and
returns what eager `GlowTTS.inference` returns with the same noise (lengths and attentions equal, mels within 1e-5) in tensors of its own; a later
call that fits a bucket captures once, and its result (on both calls) is a view of that captured graph's output buffer, i.e. the replay wrote it."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from helpers import load_case, tiny_hp_dict                          # noqa: E402
from glow_tts_amd.graph_infer import GraphedInference                 # noqa: E402
from glow_tts_amd.hparams import Recursive_Parse                      # noqa: E402
from glow_tts_amd.modules import GlowTTS                              # noqa: E402


def main():
    sd, _, _ = load_case("tiny_vanilla.npz")
    sd = dict(sd)
    wq = "layer_Dict.Encoder.layer_Dict.Duration_Predictor.layer_Dict.Projection"
    sd[wq + ".weight"] = torch.zeros_like(sd[wq + ".weight"])
    sd[wq + ".bias"] = torch.full_like(sd[wq + ".bias"], math.log(7.5))      # eight frames per token
    hp = tiny_hp_dict("Vanilla")
    hp["HIP_Precision"] = "f32"
    model = GlowTTS(Recursive_Parse(hp))
    model.load_state_dict(sd)
    for f in model.layer_Dict["Decoder"].layer_Dict["Flows"]:
        f.layers[0].initialized = True
    model = model.cuda().eval()
    vocab = sd["layer_Dict.Encoder.layer_Dict.Embedding.weight"].shape[0]
    g = torch.Generator().manual_seed(3)
    gi = GraphedInference(model)
    assert gi.buckets[-1] == 2048

    def run(lengths, ls):
        B = len(lengths)
        tokens = torch.randint(1, vocab, (B, max(lengths)), generator=g)
        for b, n in enumerate(lengths):
            tokens[b, n:] = 0
        tl = torch.tensor(lengths)
        noise = torch.randn(B, 12, 4096, generator=g).cuda()
        lsc = torch.tensor(ls).cuda()
        with torch.no_grad():
            want = model.inference(tokens.cuda(), tl.cuda(), noise_scale=0.667, length_scale=lsc, noises=noise)
        got = gi(tokens.cuda(), tl.cuda(), noise_scale=0.667, length_scale=lsc, noises=noise)
        torch.cuda.synchronize()
        graph_outs = {o[3][0].data_ptr() for o in gi.back.values()}
        replayed = got[0].data_ptr() in graph_outs                    # the returned mels are a view of a captured graph's output
        assert torch.equal(got[1], want[1]), (got[1], want[1])
        assert got[2].shape == want[2].shape and torch.equal(got[2], want[2])
        err = (got[0] - want[0]).abs().max().item()
        assert got[0].shape == want[0].shape and err <= 1e-5, err
        return want[1], err, replayed

    lengths, err, replayed = run([300, 120], [1.0, 1.0])
    assert int(lengths.max()) > 2048 and not replayed, lengths
    assert len(gi.back) == 0, "nothing is captured for a call beyond the largest bucket"
    print(f"beyond the largest bucket: frames {lengths.tolist()}, max |graphed - eager| {err:.2e}")
    for rep in range(2):                                              # in-bucket: captured on the first call, replayed on both; never recaptured
        lengths, err, replayed = run([60, 41], [1.0, 0.5])
        assert int(lengths.max()) <= 2048 and len(gi.back) == 1 and replayed, (lengths, len(gi.back), replayed)
    print(f"in-bucket: frames {lengths.tolist()}, max |graphed - eager| {err:.2e}")
    lengths, err, replayed = run([260, 300], [1.0, 1.0])
    assert int(lengths.max()) > 2048 and len(gi.back) == 1 and not replayed
    print("LONG TEXT SERVING OK")


main()
