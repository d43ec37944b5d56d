"""The reference's training entry point (`Train.py:49-598`: `Trainer(steps).Train()`), thin, over this package's pieces: `data.PatternDataset` +
`data.Collater` (shape buckets, pinned staging) -> `GlowTTS.forward` + `MLE_Loss` (+ duration MSE, + speaker CE in GR mode; Train.py:193-216)
-> backward -> clip_grad_norm_ -> RAdam -> Modified_Noam_Scheduler, the whole `Train_Step` replayed as one hipGraph per batch shape
(`graph_step.GraphedTrainStep`), checkpoints in the reference's `S_{steps}.pt` layout (`checkpoint.py`).  Same class / method names and the same
`python Train.py -s <steps>` command line; no TensorBoard writer, no plots (Logger.py is out of scope): scalars go to
`logging`.  Launched under torchrun (WORLD_SIZE > 1) it trains data parallel: utterances sharded per rank, gradients summed over RCCL
(`distributed.FlatGradReducer`), ActNorm initialised from the global batch, losses weighted by global frame counts."""
import logging
import math
import os
from collections import defaultdict

import torch

from . import checkpoint, data, encoder
from .hparams import get_hp
from .modules import GlowTTS, MLE_Loss
from .optim import Modified_Noam_Scheduler, RAdam, clip_grad_norm_


def duration_loss(log_durations, log_duration_targets, token_lengths, extent=None):
    """The reference's `MSELoss()(log_Durations, log_Duration_Targets)` (Train.py:210): a mean over B x (longest text OF THE BATCH) elements -
    its collater pads to the batch maximum (Datasets.py:225-250).  This package pads the token axis to a shape bucket, so the mean is taken
    over the unpadded extent explicitly: padded positions are zero in both tensors and must not enlarge the denominator (a plain MSELoss would
    scale the loss and its gradient by max_len / bucket_len, a batch-dependent factor down to ~0.75).  No host sync: the extent stays on the device."""
    # extent (data parallel): the longest text of the GLOBAL batch, a 0-d device tensor (`distributed.global_token_extent`) - the single-process
    # step divides every rank's shard by the same B x max length (VERDICT r3 / ADVICE r3: each rank used its own longest text).
    # One launch per direction (alignment.DurationMSE; was six torch launches forward and backward on the text encoder's stream).
    if log_durations.is_cuda:
        from .alignment import duration_mse
        return duration_mse(log_durations, log_duration_targets, token_lengths, extent)
    # host tensors (the world-2 gloo tests of the loss weighting, tests/test_trainer_losses.py): the same expression in torch
    d = (log_durations - log_duration_targets).reshape(log_durations.shape[0], -1)
    ext = token_lengths.max() if extent is None else extent
    return (d * d).sum() / (d.shape[0] * ext.to(d.dtype))


def default_buckets(max_len, step, multiple=1, offset=0):
    """Ascending padded lengths: the multiples of `step` below `max_len`, then `max_len` itself (rounded up to `multiple`) - the longest
    pattern the filters admit needs no more padding than that (a top bucket of ceil(max / step) * step - 896 frames for the yaml's 800 - was 23 %
    slower per step than the 800-frame shape, see `mel_bucket_step`)."""
    top = int(math.ceil(max_len / multiple)) * multiple
    return [b + offset for b in range(step, top - offset, step) if b + offset > 0] + [top]


def mel_bucket_step(hp):
    """Frames per mel bucket step: the rows ONE workgroup of the fused coupling-network kernels owns (csrc/wavenet_fused.hip: a 64-row window
    less a 2-row halo per remaining layer on each side, 52 rows at 4 layers) times Num_Squeeze.  Those kernels run one workgroup per 52 rows of
    the batch's row tensor (every utterance: T / Num_Squeeze + 2 x ROW_PAD rows), so padding inside a window is free for them while one window
    more per utterance is B workgroups more: buckets of 104 k - 8 frames make every utterance exactly k windows, and at B = 32 the 824-frame
    bucket is the last that fits the chip's 256 CUs in one round (832 frames: 259 workgroups, a second round for every one of the step's 19 fused
    launches - 6.29 vs 5.2 ms per step measured; 896 frames: 7.2 ms)."""
    wn = hp.Decoder.Affine_Coupling.WaveNet
    owned = 64 - 2 * ((int(wn.Kernel_Size) - 1) // 2) * (int(wn.Num_Layers) - 1)
    return max(16, owned) * int(hp.Decoder.Num_Squeeze)


class Trainer:
    def __init__(self, steps=0, hp=None, speaker_encoder=None, use_graph=True, workers=None):
        """speaker_encoder: GE2E mode only - a callable mapping the collater's slice stack [B * Samples, Mel, Slice] to L2-normalised d-vectors
        [B, Embedding_Size].  None with `Speaker_Embedding.GE2E.Checkpoint_Path` set: the `speaker_encoder.GE2E` of that checkpoint (the reference's pre-trained
        GE2E network is an un-vendored submodule; DESIGN.md "GE2E speaker encoder" states this package's own)."""
        self.hp = hp if hp is not None else get_hp()
        self.steps, self.epochs = steps, 0
        self.speaker_encoder, self.use_graph, self.workers = speaker_encoder, use_graph, workers       # workers: overrides hp.Train.Num_Workers
        self.rank, self.world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        self.device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(self.device)
        if self.world > 1 and not torch.distributed.is_initialized():
            torch.distributed.init_process_group("nccl")                       # RCCL
        from . import distributed as gd
        self.dp = gd.is_dist()                                                 # (also a one-rank group under distributed.SINGLE_RANK_IS_DIST: the RCCL path on one GPU)
        self.Datset_Generate()
        self.Model_Generate()
        ge2e_path = getattr(self.hp.Speaker_Embedding.GE2E, "Checkpoint_Path", None)
        if self.hp.Mode.upper() in ("SE", "GR") and self.hp.Speaker_Embedding.Type.upper() == "GE2E" and self.speaker_encoder is None and ge2e_path:
            from .speaker_encoder import GE2E
            self.speaker_encoder = GE2E.from_checkpoint(self.hp, self.device, ge2e_path)
        self.scalar_Dict = {"Train": defaultdict(float), "Evaluation": defaultdict(float)}
        self.Load_Checkpoint()

    # ------------------------------------------------------------------ Train.py:69-139
    def Datset_Generate(self):
        hp = self.hp
        self.token_Dict = data.load_token_dict(hp.Token_Path)
        mk = lambda p, acc: data.PatternDataset(
            pattern_path=p.Path, metadata_file=p.Metadata_File, token_dict=self.token_Dict, accumulated_dataset_epoch=acc,
            mel_length_min=p.Mel_Length.Min, mel_length_max=p.Mel_Length.Max, text_length_min=p.Text_Length.Min, text_length_max=p.Text_Length.Max,
            use_cache=hp.Train.Use_Pattern_Cache)
        train = mk(hp.Train.Train_Pattern, hp.Train.Train_Pattern.Accumulated_Dataset_Epoch)
        dev = mk(hp.Train.Eval_Pattern, 1)
        logging.info("The number of train patterns = {}.".format(len(train) // hp.Train.Train_Pattern.Accumulated_Dataset_Epoch))
        logging.info("The number of development patterns = {}.".format(len(dev)))
        ge = hp.Speaker_Embedding.GE2E.Inference
        ge2e = (ge.Samples, ge.Slice_Length, ge.Overlap_Length) if (hp.Mode.upper() in ("SE", "GR") and hp.Speaker_Embedding.Type.upper() == "GE2E") else None
        buckets = getattr(hp, "HIP_Buckets", None)          # optional extra yaml key: {Mel: [...], Token: [...]} padded shapes (one hipGraph each)
        # (the Dev loader shares the collater: the top bucket covers the longer of the two filters' maxima - ADVICE r4)
        mel_max = max(int(hp.Train.Train_Pattern.Mel_Length.Max), int(hp.Train.Eval_Pattern.Mel_Length.Max))
        txt_max = max(int(hp.Train.Train_Pattern.Text_Length.Max), int(hp.Train.Eval_Pattern.Text_Length.Max))
        mel_b = list(buckets.Mel) if buckets is not None else default_buckets(mel_max, mel_bucket_step(hp), int(hp.Decoder.Num_Squeeze),
                                                                              offset=-2 * encoder.ROW_PAD * int(hp.Decoder.Num_Squeeze))
        # token buckets: the encoder's rows carry 2 x GLOWTTS_ROW_PAD zero rows per utterance and its attention kernels work on 32-row tiles, the one-workgroup
        # MFMA kernels up to 128 rows: buckets of 32 k - 4 tokens fill whole tiles, and 124 tokens (not 128) is the longest text on the fast kernels -
        # a 128-token bucket ran the step at 6.1 instead of 5.2 ms (attention forward 25 -> 63 us, backward 41 -> 166 us, x 6 blocks)
        tok_b = list(buckets.Token) if buckets is not None else default_buckets(txt_max + 2, 32, offset=-2 * encoder.ROW_PAD)
        # Collation (unpickling, padding to the shape bucket): in worker processes like the reference's DataLoader(num_workers = hp.Train.Num_Workers,
        # pin_memory = True) (Train.py:100-107) - at ~6 ms per B = 32 step one Python thread cannot unpickle and pad 5 300 utterances per second.
        # Workers return plain CPU tensors, the loader's pin thread stages them in pinned memory, `_batch_to_device` issues the async copy.
        # num_workers = 0 (tests, tiny corpora): the collater runs here and owns a ring of reused pinned buffers.
        nw = max(0, int(getattr(hp.Train, "Num_Workers", 0))) if self.workers is None else int(self.workers)
        self.num_workers = nw
        self.collater = data.Collater.from_hp(hp, self.token_Dict, token_buckets=tok_b, mel_buckets=mel_b, pin_memory=(nw == 0), ge2e=ge2e)
        self.sampler = torch.utils.data.distributed.DistributedSampler(train, self.world, self.rank, shuffle=True, drop_last=True) if self.world > 1 else None
        bs = hp.Train.Batch_Size                              # per process (= per GPU)
        kw = dict(num_workers=nw, pin_memory=nw > 0, persistent_workers=nw > 0)
        if nw > 0:
            kw["prefetch_factor"] = 4
        self.dataLoader_Dict = {
            "Train": torch.utils.data.DataLoader(train, batch_size=bs, shuffle=self.sampler is None, sampler=self.sampler, collate_fn=self.collater,
                                                 drop_last=True, **kw),
            "Dev": torch.utils.data.DataLoader(dev, batch_size=bs, shuffle=False, collate_fn=self.collater, num_workers=0),
        }
        # Train.py:91-93, 116-123: the prompts synthesised every hp.Train.Inference_Interval steps (null / missing file: no inference epochs)
        inf_path = getattr(hp.Train, "Inference_Pattern_File_in_Train", None)
        if inf_path and os.path.exists(inf_path):
            inference = data.InferenceDataset(inf_path, self.token_Dict, hp)
            logging.info("The number of inference patterns = {}.".format(len(inference)))
            self.dataLoader_Dict["Inference"] = torch.utils.data.DataLoader(
                inference, batch_size=getattr(hp, "Inference_Batch_Size", None) or bs, shuffle=False, collate_fn=data.InferenceCollater(self.token_Dict, hp),
                num_workers=0)

    # ------------------------------------------------------------------ Train.py:143-180
    def Model_Generate(self):
        hp = self.hp
        model = GlowTTS(hp).to(self.device)
        self.model_Dict = {"GlowTTS": model}
        self.criterion_Dict = {"MSE": duration_loss, "MLE": MLE_Loss(hp), "CE": torch.nn.CrossEntropyLoss()}
        self.optimizer = RAdam(model.parameters(), lr=hp.Train.Learning_Rate.Initial, betas=(hp.Train.ADAM.Beta1, hp.Train.ADAM.Beta2),
                               eps=hp.Train.ADAM.Epsilon, weight_decay=hp.Train.Weight_Decay)
        self.scheduler = Modified_Noam_Scheduler(self.optimizer, base=hp.Train.Learning_Rate.Base)
        self.reducer = None
        if self.dp:
            from .distributed import FlatGradReducer, actnorm_stats_allreduce, broadcast_parameters
            broadcast_parameters(model)
            model.actnorm_allreduce = actnorm_stats_allreduce
            self.reducer = FlatGradReducer(list(model.parameters()))
        self._comp = torch.zeros(4, device=self.device)      # MLE, Length, Total, Speaker of the last step (written inside the graph)
        self._inv_world = None
        self._graphed = None

    def _losses(self, model, tokens, token_lengths, mels, mel_lengths, speakers, mels_for_ge2e, pitches, frame_weight=None, token_extent=None):
        """Train.py:193-216 -> the loss to differentiate, as its terms (`alignment.LossTerms`; `.backward()` also writes [MLE, Length, Total, Speaker] into
        `self._comp`).  frame_weight (data parallel): this rank's share of the global batch's mel frames, a 0-d device tensor computed outside the captured
        step (`distributed.global_frame_weight`)."""
        z, mel_Mean, mel_Log_Std, log_Dets, log_Durations, log_Duration_Targets, _, classified = model(
            tokens, token_lengths, mels, mel_lengths, speakers, mels_for_ge2e, pitches)
        # (GR: the duration loss and the speaker classifier's on the encoder's stream, beside the MLE reduction: neither they nor their backward
        # sit in front of the flow decoder's backward on this stream)
        from .modules import Beside
        if self.dp and (token_extent is None or frame_weight is None):
            from .distributed import global_step_scalars
            fw, te = global_step_scalars(mel_lengths.sum(), token_lengths.max())
            frame_weight = fw if frame_weight is None else frame_weight
            token_extent = te if token_extent is None else token_extent
        from . import alignment
        # what the terms will be seeded with by `LossTerms.backward` (data parallel: this rank's frame share / 1 / world, device scalars): loss nodes that know
        # their seed write their gradients in the forward launch
        inv_world = None
        if self.dp:
            if self._inv_world is None:
                self._inv_world = torch.full((), 1.0 / self.world, device=self.device)
            inv_world = self._inv_world
        alignment.SEEDS["mle"], alignment.SEEDS["rest"] = (frame_weight if self.dp else None), inv_world
        try:
            if classified is None:
                # round 6: the duration loss is one HIP launch per direction now - it stays on this stream (a fork and a join of the encoder's stream around it cost the
                # replayed graph more than the two launches take: 4.78 against 4.81-4.84 ms/step)
                length = duration_loss(log_Durations, log_Duration_Targets, token_lengths, token_extent)
                ce = None
                mle = self.criterion_Dict["MLE"](z=z, mean=mel_Mean, std=mel_Log_Std, log_dets=log_Dets, lengths=mel_lengths)
            else:
                with Beside(model) as beside:                     # GR: the speaker classifier's cross entropy is a dozen torch launches
                    beside.uses(log_Durations, log_Duration_Targets, token_lengths, token_extent, classified, speakers)
                    length = duration_loss(log_Durations, log_Duration_Targets, token_lengths, token_extent)
                    ce = self.criterion_Dict["CE"](classified, speakers)
                mle = self.criterion_Dict["MLE"](z=z, mean=mel_Mean, std=mel_Log_Std, log_dets=log_Dets, lengths=mel_lengths)
                beside.join(length, ce)
        finally:
            alignment.SEEDS["mle"] = alignment.SEEDS["rest"] = None

        def log_components():
            # [MLE, Length, Total, Speaker] of this step (Train.py:218-222), queued BEHIND the backward: three small launches that used to sit between the loss and
            # the flow decoder's backward
            total = mle.detach() + length.detach()
            self._comp.copy_(torch.stack([mle.detach(), length.detach(), total, ce.detach() if ce is not None else torch.zeros((), device=mle.device)]))
        # Train.py:213-216: loss = MLE + Length (+ Speaker); data parallel: this rank's MLE (a mean over ITS frames) weighs its share of the global frames, the
        # other terms 1 / world, gradients are SUMMED
        seeds = [frame_weight, inv_world, inv_world] if self.dp else None
        return alignment.LossTerms([mle, length, ce], seeds, after=log_components)

    def _batch_to_device(self, batch):
        # (worker-collated batches arrive in the loader's pinned memory; in-process ones in the collater's own pinned ring, whose slot the copy guards)
        pinned_ring = self.collater.pin and batch[0].is_pinned()
        tokens, token_lengths, mels, mel_lengths, speakers, ge2e, pitches = (self.collater.to_device if pinned_ring else data.to_device)(batch, self.device)
        mode = self.hp.Mode.upper()
        if mode in ("SE", "GR") and self.hp.Speaker_Embedding.Type.upper() == "GE2E":
            if self.speaker_encoder is None:
                raise RuntimeError("GE2E mode: pass Trainer(speaker_encoder=...) producing d-vectors (the GE2E network is not part of this package)")
            ge2e = self.speaker_encoder(ge2e).detach()
        else:
            ge2e = None
        if mode not in ("SE", "GR") or "LUT" not in self.model_Dict["GlowTTS"].layer_Dict:
            speakers = speakers if mode == "GR" else None
        return tokens, token_lengths, mels, mel_lengths, speakers, ge2e, (pitches if mode == "GR" else None)

    # ------------------------------------------------------------------ Train.py:182-238
    def Train_Step(self, *batch):
        hp, model = self.hp, self.model_Dict["GlowTTS"]
        inputs = self._batch_to_device(batch)

        def loss_fn(m, *inp):
            return self._losses(m, *inp)
        if self.dp:                                            # one tiny all-gather per step, outside the captured graphs
            from .distributed import global_step_scalars
            inputs = tuple(inputs) + global_step_scalars(inputs[3].sum(), inputs[1].max())
        if self.use_graph:
            # one process or data parallel: the same captured step (data parallel: three graphs around the gradient exchange, graph_step.py)
            if self._graphed is None:
                from .graph_step import GraphedTrainStep
                self._graphed = GraphedTrainStep(model, loss_fn, warmup=2, optimizer=self.optimizer, scheduler=self.scheduler,
                                                 max_grad_norm=hp.Train.Gradient_Norm)
            before = self._graphed.steps_taken
            self._graphed(*inputs)
            self.steps += self._graphed.steps_taken - before       # (always 1: a new batch shape costs dry warm-up passes, not optimizer steps)
        else:
            loss = loss_fn(model, *inputs)
            self.optimizer.zero_grad(set_to_none=True)
            loss.backward()
            if self.reducer is not None:
                self.reducer.reduce(average=False)
            clip_grad_norm_(list(model.parameters()), hp.Train.Gradient_Norm)
            self.optimizer.step()
            self.scheduler.step()
            self.steps += 1
            loss.detach()                                          # (LossTerms: writes the step's loss components into self._comp)
        for tag, v in zip(("MLE", "Length", "Total", "Speaker"), self._comp.unbind(0)):
            self.scalar_Dict["Train"]["Loss/" + tag] += v          # device scalars: no host sync per step

    # ------------------------------------------------------------------ Train.py:240-264
    def Train_Epoch(self):
        hp = self.hp
        if self.sampler is not None:
            self.sampler.set_epoch(self.epochs)
        for batch in self.dataLoader_Dict["Train"]:
            last = self.steps
            self.Train_Step(*batch)
            crossed = lambda n: self.steps // n != last // n
            if crossed(hp.Train.Checkpoint_Save_Interval):
                self.Save_Checkpoint()
            if crossed(hp.Train.Logging_Interval):
                msg = {tag: float(v) / hp.Train.Logging_Interval for tag, v in self.scalar_Dict["Train"].items()}
                msg["Learning_Rate"] = self.scheduler.get_last_lr()[0]
                if self.rank == 0:
                    logging.info("(Steps: {}) {}".format(self.steps, msg))
                self.scalar_Dict["Train"] = defaultdict(float)
            if crossed(hp.Train.Evaluation_Interval):
                self.Evaluation_Epoch()
            if crossed(hp.Train.Inference_Interval):
                self.Inference_Epoch()
            if self.steps >= hp.Train.Max_Step:
                return
        self.epochs += hp.Train.Train_Pattern.Accumulated_Dataset_Epoch

    # ------------------------------------------------------------------ Train.py:266-316
    @torch.no_grad()
    def Evaluation_Step(self, *batch):
        """Losses of `GlowTTS.forward` on a development batch AND `GlowTTS.inference` on the same batch (Train.py:279-316: the reference runs both
        on every dev batch; its TensorBoard images of the last batch are out of scope - the tensors are returned and kept in `last_Evaluation`)."""
        inputs = self._batch_to_device(batch)
        model = self.model_Dict["GlowTTS"]
        tokens, token_lengths, mels, mel_lengths, speakers, ge2e, pitches = inputs
        z, mel_Mean, mel_Log_Std, log_Dets, log_Durations, log_Duration_Targets, attentions_from_Train, classified = model(*inputs)
        mle = self.criterion_Dict["MLE"](z=z, mean=mel_Mean, std=mel_Log_Std, log_dets=log_Dets, lengths=mel_lengths)
        length = duration_loss(log_Durations, log_Duration_Targets, token_lengths)
        comp = {"MLE": mle, "Length": length, "Total": mle + length}
        if classified is not None:
            comp["Speaker"] = self.criterion_Dict["CE"](classified, speakers)
        for tag, v in comp.items():
            self.scalar_Dict["Evaluation"]["Loss/" + tag] += v
        mel_Predictions, _, attentions_from_Inference = model.inference(
            tokens, token_lengths, mels_for_prosody=mels, mel_lengths_for_prosody=mel_lengths, speakers=speakers, mels_for_ge2e=ge2e,
            pitches=pitches, pitch_lengths=mel_lengths, length_scale=torch.tensor([1.0], device=tokens.device))
        self.last_Evaluation = (mel_Predictions, attentions_from_Train, attentions_from_Inference, classified)
        return self.last_Evaluation

    # ------------------------------------------------------------------ Train.py:371-440 (the PNG plots are out of scope: mels are saved as .npy)
    @torch.no_grad()
    def Inference_Step(self, tokens, token_lengths, mels_for_prosody, mel_lengths_for_prosody, speakers, mels_for_ge2e, pitches, pitch_lengths,
                       length_scales, labels, texts, start_index=0, tag_step=False, tag_index=False):
        """Same arguments and file naming as the reference; writes `<Inference_Path>/Step-<steps>/NPY/<file>.npy` ([T_mel, Mel_Dim] per utterance,
        trimmed to its length) and returns the file names."""
        import numpy as np
        dev = self.device
        mv = lambda t: t.to(dev) if torch.is_tensor(t) else t
        mode = self.hp.Mode.upper()
        lut = "LUT" in self.model_Dict["GlowTTS"].layer_Dict
        if mode in ("SE", "GR") and not lut:
            # GE2E: the loader hands over the raw slice stack [B * Samples, Mel, Slice]; the model takes d-vectors [B, Embedding_Size] - the same
            # conversion `_batch_to_device` applies to training batches (Modules.py:154-156 runs the GE2E network inside `inference`)
            if self.speaker_encoder is None:
                raise RuntimeError("GE2E mode: pass Trainer(speaker_encoder=...) producing d-vectors (the GE2E network is not part of this package)")
            mels_for_ge2e = self.speaker_encoder(mv(mels_for_ge2e)).detach()
        mels, mel_Lengths, attentions = self.model_Dict["GlowTTS"].inference(
            mv(tokens), mv(token_lengths), mels_for_prosody=mv(mels_for_prosody) if mode in ("PE", "GR") else None,
            mel_lengths_for_prosody=mv(mel_lengths_for_prosody) if mode in ("PE", "GR") else None,
            speakers=mv(speakers) if (mode in ("SE", "GR") and lut) else None, mels_for_ge2e=mv(mels_for_ge2e) if (mode in ("SE", "GR") and not lut) else None,
            pitches=mv(pitches) if mode == "GR" else None, pitch_lengths=mv(pitch_lengths) if mode == "GR" else None, length_scale=mv(length_scales))
        files = []
        for index, label in enumerate(labels):
            tags = (["Step-{}".format(self.steps)] if tag_step else []) + [label] + (["IDX_{}".format(index + start_index)] if tag_index else [])
            files.append(".".join(tags))
        out_dir = os.path.join(self.hp.Inference_Path, "Step-{}".format(self.steps), "NPY").replace("\\", "/")
        os.makedirs(out_dir, exist_ok=True)
        for mel, n, file in zip(mels.cpu().numpy(), mel_Lengths.cpu().numpy(), files):
            np.save(os.path.join(out_dir, file + ".npy"), mel[:, :int(n)].T.astype(np.float32), allow_pickle=False)
        return files

    # ------------------------------------------------------------------ Train.py:445-461
    def Inference_Epoch(self):
        """Synthesises the prompts of `hp.Train.Inference_Pattern_File_in_Train` with the current weights (eval mode) and writes one .npy per prompt
        under <Inference_Path>/Step-<steps>/NPY (rank 0 only when data parallel; the reference's PNG plots are out of scope)."""
        loader = self.dataLoader_Dict.get("Inference")
        if loader is None or self.rank != 0:
            return []
        logging.info("(Steps: {}) Start inference.".format(self.steps))
        model = self.model_Dict["GlowTTS"]
        model.eval()
        files, bs = [], loader.batch_size
        for step, batch in enumerate(loader):
            files += self.Inference_Step(*batch, start_index=step * bs)
        model.train()
        return files

    def Evaluation_Epoch(self):
        logging.info("(Steps: {}) Start evaluation.".format(self.steps))
        model = self.model_Dict["GlowTTS"]
        model.eval()
        n = 0
        for n, batch in enumerate(self.dataLoader_Dict["Dev"], 1):
            self.Evaluation_Step(*batch)
        if n and self.rank == 0:
            logging.info("(Steps: {}) Evaluation {}".format(self.steps, {t: float(v) / n for t, v in self.scalar_Dict["Evaluation"].items()}))
        self.scalar_Dict["Evaluation"] = defaultdict(float)
        model.train()
        if getattr(self.hp.Train, "Prosody_Check", None) is not None and self.hp.Mode.upper() in ("PE", "GR") and \
                self.steps % int(self.hp.Train.Prosody_Check_Interval) == 0:                                    # Train.py:357-358
            self.Prosody_Check_Epoch()

    # ------------------------------------------------------------------ Train.py:463-492, Datasets.py:168-214
    def Prosody_Check_Epoch(self):
        """The prosody vectors of up to Speakers x Samples_per_Speaker training patterns, mapped by exact t-SNE on the device (`visualizer.write_map`) into
        <Inference_Path>/Step-<steps>/PROSODY - the reference hands them to TensorBoard's projector.  Only with the optional yaml block `Train.Prosody_Check`
        (without it: nothing, as before the block existed), on rank 0, in eval mode.  -> the dict of map.json, or None"""
        from . import projection, visualizer
        check = visualizer.prosody_check_settings(self.hp)
        if check is None or self.rank != 0:
            return None
        hp = self.hp
        logging.info("(Steps: {}) Start prosody check.".format(self.steps))
        settings = projection.projection_settings(hp)
        root, files = visualizer.pattern_selection(hp, "train", check["Speakers"], check["Samples_per_Speaker"], 0)
        rows, mels = visualizer.load_patterns(root, files)
        model = self.model_Dict["GlowTTS"]
        model.eval()
        try:
            vectors = visualizer.prosody_vectors(model, mels, int(hp.Inference_Batch_Size or hp.Train.Batch_Size), hp.Sound.Max_Abs_Mel, self.device)
        finally:
            model.train()
        out_dir = os.path.join(hp.Inference_Path, "Step-{}".format(self.steps), "PROSODY").replace("\\", "/")
        info = visualizer.write_map(out_dir, vectors, rows, settings, 0, {"what": "prosody", "steps": int(self.steps)})
        logging.info("(Steps: {}) Prosody check: final KL {:.4f}; nearest-neighbour agreement with the speakers: embeddings {:.3f}, map {:.3f}".format(
            self.steps, info["kl"][-1], info["nearest_neighbour_agreement"]["embeddings"], info["nearest_neighbour_agreement"]["map"]))
        return info

    # ------------------------------------------------------------------ Train.py:498-553
    def Load_Checkpoint(self):
        got = checkpoint.load_checkpoint(self.hp.Checkpoint_Path, self.model_Dict["GlowTTS"], self.optimizer, self.scheduler, self.steps) \
            if (self.steps != 0 or os.path.isdir(self.hp.Checkpoint_Path)) else None
        if got is None:
            return                                              # initial training
        self.steps, self.epochs = got
        logging.info("Checkpoint loaded at {} steps.".format(self.steps))

    def Save_Checkpoint(self):
        if self.rank != 0:
            return
        path = checkpoint.save_checkpoint(self.hp.Checkpoint_Path, self.model_Dict["GlowTTS"], self.optimizer, self.scheduler, self.steps, self.epochs)
        logging.info("Checkpoint saved at {} steps: {}".format(self.steps, path))

    # ------------------------------------------------------------------ Train.py:563-590
    def Train(self):
        hp = self.hp
        hp_Path = os.path.join(hp.Checkpoint_Path, "Hyper_Parameters.yaml").replace("\\", "/")
        if self.rank == 0 and not os.path.exists(hp_Path) and os.path.exists("Hyper_Parameters.yaml"):
            from shutil import copyfile
            os.makedirs(hp.Checkpoint_Path, exist_ok=True)
            copyfile("Hyper_Parameters.yaml", hp_Path)
        if self.steps == 0:
            self.Evaluation_Epoch()
        if getattr(hp.Train, "Initial_Inference", False):
            self.Inference_Epoch()
        while self.steps < hp.Train.Max_Step:
            try:
                self.Train_Epoch()
            except KeyboardInterrupt:
                self.Save_Checkpoint()
                raise SystemExit(1)
        logging.info("Finished training.")
        self.close()

    def close(self):
        """Stops the train loader's worker processes now.  Left to the garbage collector they stop late and slowly: the Trainer, its DataLoader and the
        loader's persistent iterator sit in a reference cycle, the cycle collector finalises the iterator's queues before the iterator, the workers
        never see the shutdown message and every one of them is joined with a 5-s timeout (20 s per Trainer with 4 workers: the GPU test suite spent
        a quarter of its time there).  A later `Train()` starts new workers."""
        for dl in self.dataLoader_Dict.values():
            it = getattr(dl, "_iterator", None)
            if it is not None and hasattr(it, "_shutdown_workers"):
                it._shutdown_workers()
                dl._iterator = None


def main(argv=None):
    import argparse
    logging.basicConfig(level=logging.INFO, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", "--steps", default=0, type=int)
    args = ap.parse_args(argv)
    Trainer(steps=args.steps).Train()
