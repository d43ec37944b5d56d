"""GE2E speaker encoder (glow_tts_amd/speaker_encoder.py: GE2E, csrc/ge2e_ops.hip) on one MI355X at the default sizes (80 mel bins, 3 LSTM layers of 256,
256-dimensional d-vectors, 5 slices of 64 frames per utterance).
  1. The encoder alone at B = 32 and B = 1 utterances: ms per call of the HIP path (T + Stacks - 1 cell launches + one head launch) against the REFERENCE FOR
     TIME, the same weights in torch.nn.LSTM + torch.nn.Linear (the vendor library's RNN) with the normalisation in torch, on the same device and input;
     the two paths alternate call by call in one process so that a drifting clock meets both; median of `--iters` (>= 20) calls each, every call a host
     clock around work that ends in a device synchronise; the largest difference of the d-vectors.
  2. `Trainer.Train_Step` of BASELINE config 4 (SE mode, GE2E d-vectors, B = 16, through the real loader's batches held in memory) in two ways, alternating
     in blocks: with this encoder in front of the step, and with a stand-in callable that returns fixed d-vectors (the path before the encoder existed);
     median ms per step of each and their difference - what the encoder costs a training step.
Usage: python tools/bench_ge2e.py [--iters 20] [--steps 40] [--blocks 5] [--out profiles/bench_ge2e.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def encoder_alone(enc, B, warmup, iters):
    s, dev = enc.sizes, enc.linear.weight.device
    samples, T = enc.samples, 64
    lstm = torch.nn.LSTM(s["Mel"], s["H"], s["Stacks"], batch_first=True).to(dev)
    linear = torch.nn.Linear(s["H"], s["E"]).to(dev)
    lstm.load_state_dict(enc.lstm.state_dict())
    linear.load_state_dict(enc.linear.state_dict())
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B * samples, s["Mel"], T, generator=g) * 8.0 - 4.0).to(dev)

    @torch.no_grad()
    def base():
        top, _ = lstm(x.transpose(1, 2))
        w = torch.nn.functional.normalize(linear(top[:, -1]), dim=1)
        return torch.nn.functional.normalize(w.reshape(B, samples, -1).mean(1), dim=1)

    hip = lambda: enc(x)
    diff = float((hip() - base()).abs().max())
    for _ in range(warmup):
        hip()
        base()
    torch.cuda.synchronize()
    th, tb = [], []
    for _ in range(iters):                                     # call by call, alternating
        th.append(timed(hip))
        tb.append(timed(base))
    h, b = stats(th), stats(tb)
    return {"B": B, "slices": B * samples, "slice_frames": T, "launches_per_call": T + s["Stacks"], "d_vector_max_abs_diff_hip_vs_torch": diff, "hip": h,
            "torch_lstm_linear": b, "speedup_hip_over_torch": round(b["ms_median"] / h["ms_median"], 2), "hip_faster": bool(h["ms_median"] < b["ms_median"])}


def trainer_steps(enc_path, steps, blocks, utterances):
    from bench_loader import make_corpus
    from glow_tts_amd import hparams
    from glow_tts_amd.trainer import Trainer
    root = tempfile.mkdtemp(prefix="glowtts_ge2e_corpus_")
    token_dict = make_corpus(root, utterances)
    d = copy.deepcopy(hparams.load_yaml(hparams.DEFAULT_YAML))
    d["Mode"] = "SE"
    d["Speaker_Embedding"]["Type"] = "GE2E"
    d["Speaker_Embedding"]["GE2E"]["Checkpoint_Path"] = enc_path
    d["Token_Path"] = os.path.join(root, "Token.yaml")
    d["Encoder"]["Embedding_Tokens"] = len(token_dict)
    for split, key in (("Train", "Train_Pattern"), ("Eval", "Eval_Pattern")):
        d["Train"][key].update(Path=os.path.join(root, split), Metadata_File="METADATA.PICKLE")
    d["Train"].update(Batch_Size=16, Max_Step=10 ** 9, Checkpoint_Save_Interval=10 ** 9, Logging_Interval=10 ** 9, Evaluation_Interval=10 ** 9)
    d["Checkpoint_Path"] = os.path.join(root, "Checkpoint")
    E, samples = int(d["Speaker_Embedding"]["Embedding_Size"]), int(d["Speaker_Embedding"]["GE2E"]["Inference"]["Samples"])
    fixed = torch.nn.functional.normalize(torch.randn(16, E, generator=torch.Generator().manual_seed(1)), dim=1).cuda()
    stand_in = lambda stack: fixed[:stack.shape[0] // samples]
    trainers = {}
    for name, callable_ in (("with_encoder", None), ("stand_in", stand_in)):
        torch.manual_seed(0)
        trainers[name] = Trainer(steps=0, hp=hparams.Recursive_Parse(copy.deepcopy(d)), speaker_encoder=callable_, workers=0)
    batches = []
    for batch in trainers["with_encoder"].dataLoader_Dict["Train"]:    # the loader's own batches, held in memory: the loader is not what is measured
        batches.append(tuple(t.clone() if torch.is_tensor(t) else t for t in batch))      # (copies: the collater reuses its pinned staging buffers)
        if len(batches) == 8:
            break
    for tr in trainers.values():                               # every shape captured before anything is timed
        for _ in range(3):
            for batch in batches:
                tr.Train_Step(*batch)
    torch.cuda.synchronize()
    per = {name: [] for name in trainers}
    for _ in range(blocks):
        for name, tr in trainers.items():
            def block():
                for i in range(steps):
                    tr.Train_Step(*batches[i % len(batches)])
            per[name].append(timed(block) / steps)
    out = {name: dict(stats(ts), blocks_ms_per_step=[round(t, 4) for t in ts]) for name, ts in per.items()}
    out.update(batch_size=16, steps_per_block=steps, blocks=blocks, captured_shapes=len(trainers["with_encoder"]._graphed.graphs),
               encoder_cost_ms_per_step=round(out["with_encoder"]["ms_median"] - out["stand_in"]["ms_median"], 4))
    for tr in trainers.values():
        tr.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--utterances", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_ge2e.json"))
    args = ap.parse_args()
    assert args.iters >= 20, "at least 20 timed calls"
    assert torch.cuda.is_available(), "bench_ge2e.py measures on the GPU"
    from glow_tts_amd.hparams import DEFAULT_YAML, Recursive_Parse, load_yaml
    from glow_tts_amd.speaker_encoder import GE2E
    torch.manual_seed(1234)
    enc = GE2E(Recursive_Parse(load_yaml(DEFAULT_YAML)), "cuda:0")
    enc_path = os.path.join(tempfile.mkdtemp(prefix="glowtts_ge2e_"), "ge2e.pt")
    torch.save({"Model": {k: v.cpu() for k, v in enc.state_dict().items()}}, enc_path)
    ghz, _ = bench.sustained_mfma_clock()
    out = {"device": torch.cuda.get_device_name(0), "sustained_mfma_ghz": round(ghz, 3), "iters": args.iters, "warmup": args.warmup, "sizes": enc.sizes,
           "samples": enc.samples, "encoder_alone": [encoder_alone(enc, B, args.warmup, args.iters) for B in (32, 1)],
           "trainer_config4": trainer_steps(enc_path, args.steps, args.blocks, args.utterances)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
