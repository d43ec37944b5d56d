"""The reference's inference entry point (`Inference.py:111-313`: `Inferencer(checkpoint_path).Inference(labels, texts, scales, speakers,
references, inference_path)`), thin: text -> tokens (`Token.yaml`), optional reference mels for the prosody encoder / pitch tracks, `S_*.pt`
checkpoint (ActNorm marked initialised, `Inference.py:258-270`), `GlowTTS.inference` (replayed as hipGraphs through `graph_infer.GraphedInference`
where the mode allows it), one `.npy` mel per utterance (`Inference.py:213-220`; the PNG plots are out of scope) and, with `wav=True`, one
`WAV/<label>.wav` next to it from the active vocoder: Griffin-Lim (`vocoder.GriffinLim`: a baseline vocoder, not a neural one) or, with the yaml block
`Vocoder` / `vocoder='pwg'` and a checkpoint, the Parallel WaveGAN generator (`vocoder.ParallelWaveGAN`), or, with `Type: 'HiFiGAN'` in that block /
`vocoder='hifigan'`, the HiFi-GAN generator (`vocoder.HiFiGAN`).  `references` are either
`.npy` files / arrays holding mels [T, Mel] (what `Pattern_Generator.Pattern_Generate` produces) or wav files, which go through
`glow_tts_amd.audio` (librosa-free restatement of `Audio.py`; resampling is not implemented: the wav must be at hp.Sound.Sample_Rate).
With `Speaker_Embedding.Type: 'GE2E'` the speaker is given by `speaker_references` (wav files, mels or ready d-vectors), which go through
`data.mels_for_ge2e` and the GE2E speaker encoder (`speaker_encoder.GE2E`; the reference runs it inside `GlowTTS.inference`, Modules.py:154-156)."""
import hashlib
import logging
import os

import numpy as np
import torch

from . import data
from .hparams import get_hp
from .modules import GlowTTS


def utterance_seed_words(seed, label, k=0):
    """The two 32-bit seed words of sample `k` of the utterance `label` under the run seed `seed`: the first 8 bytes of blake2b of "<seed> NUL <label> NUL <k>", little
    endian.  A function of the three only (not Python's per-process salted hash()): the same in every process, whatever the order or the batch size."""
    d = hashlib.blake2b("{}\0{}\0{}".format(seed, label, k).encode()).digest()
    return int.from_bytes(d[:4], "little"), int.from_bytes(d[4:8], "little")


class Inferencer:
    def __init__(self, checkpoint_path, hp=None, device="cuda:0", device_frontend=False, vocoder=None, vocoder_checkpoint=None, speaker_encoder=None,
                 vocoder_precision=None):
        """device_frontend: wav references and wav voice-conversion sources are analysed on the device (`frontend.Analyzer`) instead of the host's
        `audio.pattern_from_wav`; decoding, trimming and normalisation stay `audio.audio_prep` either way.
        vocoder: 'pwg' or 'hifigan' (the neural vocoders), 'griffin_lim' (forces the baseline) or None: 'hifigan' when the yaml's `Vocoder` block has
        `Type: 'HiFiGAN'`, 'pwg' for any other `Vocoder` block or when `vocoder_checkpoint` (overrides `Vocoder.Checkpoint_Path`) is given, Griffin-Lim
        otherwise (`vocoder.vocoder_kind`; `vocoder.make_vocoder` builds it).
        vocoder_precision: 'f32', 'bf16', 'f16' or None (the yaml's `Vocoder.Precision`, default 'f32') - 'bf16' is the Parallel WaveGAN's layer arithmetic
        (`vocoder.ParallelWaveGAN`), 'f16' the HiFi-GAN generator's convolution arithmetic (`vocoder.HiFiGAN`); each generator refuses the other's mode
        naming `Vocoder.Precision`; Griffin-Lim ignores it.
        speaker_encoder: GE2E mode only - a callable mapping a slice stack [B * Samples, Mel, Slice] to unit d-vectors [B, Embedding_Size].  None: the
        `speaker_encoder.GE2E` of `Speaker_Embedding.GE2E.Checkpoint_Path`, else the one the GlowTTS checkpoint carries under `layer_Dict.GE2E.*` (keys of
        another layout: a warning, and they are dropped), else none - then only ready d-vectors can be given."""
        self.hp = hp if hp is not None else get_hp()
        from .vocoder import vocoder_kind
        self.vocoder_kind = vocoder_kind(self.hp, vocoder, vocoder_checkpoint)
        self.vocoder_checkpoint = vocoder_checkpoint
        if vocoder_precision not in (None, "f32", "bf16", "f16"):
            raise ValueError("vocoder_precision must be 'f32', 'bf16', 'f16' or None, got {!r}".format(vocoder_precision))
        self.vocoder_precision = vocoder_precision
        self.device = torch.device(device)
        self.device_frontend, self._analyzer = bool(device_frontend), None
        self.token_Dict = data.load_token_dict(self.hp.Token_Path)
        self.last_wav_files = []                                                 # the wav files the last Inference / Voice_Conversion / Vocode call wrote
        self._vocoder = None
        self.ge2e_mode = self.hp.Mode.upper() in ("SE", "GR") and self.hp.Speaker_Embedding.Type.upper() == "GE2E"
        self.speaker_encoder = speaker_encoder
        self.Model_Generate()
        self.Load_Checkpoint(checkpoint_path)

    def Model_Generate(self):                                                    # Inference.py:116-136
        # Arithmetic of the inverse flow: exact fp32 (the reference's; mels within 2e-4 of it) unless the yaml asks otherwise with the optional key
        # `HIP_Inference_Precision`.  bf16 - the TRAINING default, `HIP_Precision` - leaves ~1e-2 rms / 0.3 worst-element error on the generated mel
        # (tests/longform_check.py "BF16 INVERSE MEL"), above the 1e-3 the path promises, and inference is not the throughput-critical half.
        import copy
        self.hp = copy.copy(self.hp)
        self.hp.HIP_Precision = str(getattr(self.hp, "HIP_Inference_Precision", "f32"))
        self.model_Dict = {"GlowTTS": GlowTTS(self.hp).to(self.device).eval()}
        self._graphed = None

    def Load_Checkpoint(self, checkpoint_path):                                  # Inference.py:258-275
        state_Dict = torch.load(checkpoint_path, map_location="cpu")
        if self.ge2e_mode and self.speaker_encoder is None:
            from . import speaker_encoder
            path = getattr(self.hp.Speaker_Embedding.GE2E, "Checkpoint_Path", None)
            self.speaker_encoder = speaker_encoder.GE2E.from_checkpoint(self.hp, self.device, path) if path else \
                speaker_encoder.from_glowtts_checkpoint(self.hp, self.device, state_Dict["Model"])
        self.model_Dict["GlowTTS"].load_state_dict(state_Dict["Model"])
        for flow in self.model_Dict["GlowTTS"].layer_Dict["Decoder"].layer_Dict["Flows"]:
            flow.layers[0].initialized = True      # Activation_Norm is already initialized when checkpoint is loaded.
        self.model_Dict["GlowTTS"].to(self.device)
        logging.info("Checkpoint loaded at {} steps.".format(state_Dict.get("Steps")))

    def _make_vocoder(self):
        from .vocoder import make_vocoder
        return make_vocoder(self.hp, self.device, self.vocoder_kind, self.vocoder_checkpoint, self.vocoder_precision)

    def _write_wavs(self, mels, mel_lengths, names, inference_path, seeds=None, vocoder_seeds=None):
        """The active vocoder on the mels as the model produced them ([B, Mel, T], on the device) -> WAV/<name>.wav, 16-bit, Sound.Sample_Rate.
        Neural vocoder: frames * Frame_Shift samples, clipped to [-1, 1], no de-emphasis; vocoder_seeds (integer [B, 2], `vocoder.pwg_seed_words`): its noise is
        the counter hash of those words, so the wav repeats byte for byte; None: torch's device generator.  The HiFi-GAN generator has no noise: it ignores
        the words and its wav repeats byte for byte with or without them.
        Griffin-Lim: de-emphasised.
        seeds (integer [B, 2], seeded sampling): Griffin-Lim's start phase of every utterance is drawn from a host generator seeded with its two seed words,
        over that utterance's own frames (zero beyond) - a function of the seed and the utterance's length only, so the wav is as reproducible as the mel.
        None: torch's device generator, as before."""
        from . import audio
        if self._vocoder is None:
            self._vocoder = self._make_vocoder()
        mels = mels[:, :, :int(mel_lengths.max())]                                # a served batch may be padded beyond its longest utterance
        phase, neural = None, self.vocoder_kind != "griffin_lim"
        if neural:
            wavs = self._vocoder.to_host(*self._vocoder(mels, mel_lengths, seeds=vocoder_seeds))
        elif seeds is not None:
            T, F = mels.shape[2], self._vocoder.n_freq
            phase = torch.zeros(mels.shape[0], T, F)
            for b, (n, (s0, s1)) in enumerate(zip(mel_lengths.cpu().tolist(), seeds.tolist())):
                n = min(int(n), T)
                g = torch.Generator().manual_seed((int(s0) & 0xFFFFFFFF) | ((int(s1) & 0x7FFFFFFF) << 32))
                phase[b, :n] = (torch.rand(n, F, generator=g) * 2.0 - 1.0) * float(np.pi)
        if not neural:
            wavs = self._vocoder.to_host(*self._vocoder(mels, mel_lengths, initial_phase=phase))
        os.makedirs(os.path.join(inference_path, "WAV").replace("\\", "/"), exist_ok=True)
        for name, x in zip(names, wavs):
            path = os.path.join(inference_path, "WAV", name + ".wav").replace("\\", "/")
            audio.write_wav(path, x, self.hp.Sound.Sample_Rate)
            self.last_wav_files.append(path)

    def _reference(self, ref):
        """-> (mel [T, Mel] float32, pitch [T] float32 or None)"""
        if isinstance(ref, (tuple, list)):
            return np.asarray(ref[0], np.float32), np.asarray(ref[1], np.float32)
        if isinstance(ref, np.ndarray):
            return ref.astype(np.float32), None
        if str(ref).lower().endswith(".npy"):
            return np.load(ref).astype(np.float32), None
        from . import audio
        gr = self.hp.Mode.upper() == "GR"                                        # GR: the YIN pitch track (Inference.py:56-58, Pattern_Generator.py:41-52)
        if self.device_frontend:
            if self._analyzer is None:
                from .frontend import Analyzer
                self._analyzer = Analyzer(self.hp, self.device, with_pitch=gr)
            return self._analyzer([audio.audio_prep(ref, self.hp.Sound.Sample_Rate, 30)], with_pitch=gr)[0]
        return audio.pattern_from_wav(ref, self.hp, with_pitch=gr)

    def D_Vectors(self, references, rngs=None):
        """GE2E mode: one speaker reference per utterance -> d-vectors, np.ndarray [n, Embedding_Size].  A reference is a wav path, a `.npy` path or an array
        [T, Mel] holding a mel, or a 1-D array [Embedding_Size] taken as a d-vector as it is.  Mels are cut into slices by `data.mels_for_ge2e`
        (Datasets.py:41-65) - rngs: one generator per reference for its random offset, None: `np.random` as in the reference - and go through the speaker
        encoder in one batch."""
        hp = self.hp
        ge, E = hp.Speaker_Embedding.GE2E.Inference, int(hp.Speaker_Embedding.Embedding_Size)
        out = np.zeros((len(references), E), np.float32)
        stacks, where = [], []
        for i, ref in enumerate(references):
            if torch.is_tensor(ref):
                ref = ref.detach().cpu().numpy()
            if isinstance(ref, np.ndarray) and ref.ndim == 1:
                if ref.shape[0] != E:
                    raise ValueError("speaker reference {}: a 1-D array is taken as a d-vector and must have Speaker_Embedding.Embedding_Size = {} elements, got {}"
                                     .format(i, E, ref.shape[0]))
                out[i] = ref
                continue
            mel = self._reference(ref)[0]
            stacks.append(data.mels_for_ge2e([mel], int(ge.Samples), int(ge.Slice_Length), int(ge.Overlap_Length), rng=rngs[i] if rngs is not None else np.random))
            where.append(i)
        if stacks:
            if self.speaker_encoder is None:
                raise ValueError("GE2E mode: wav / mel speaker references need a speaker encoder - set Speaker_Embedding.GE2E.Checkpoint_Path, pass "
                                 "Inferencer(speaker_encoder=...) or give ready d-vectors [Embedding_Size]")
            x = torch.from_numpy(np.concatenate(stacks).astype(np.float32)).transpose(2, 1).contiguous().to(self.device)
            with torch.no_grad():
                out[where] = self.speaker_encoder(x).detach().float().cpu().numpy()
        return out

    @torch.no_grad()
    def Inference_Step(self, tokens, token_lengths, prosodies, prosody_lengths, speakers, ge2es, pitches, pitch_lengths, length_scales, labels, texts,
                       start_index=0, tag_index=False, inference_path="./inference", noise_scale=1.0, wav=False, seeds=None, sample_index=None, vocoder_seeds=None):
        """Inference.py:139-223 without the plots: returns the list of written .npy files.  seeds: integer [B, 2], the utterances' seed words (None: the
        unseeded draw); sample_index k: the files are <label>.S<k>.npy / .wav; vocoder_seeds: the neural vocoder's seed words (`_write_wavs`)."""
        dev = self.device
        mv = lambda t: t if t is None else t.to(dev)
        model = self.model_Dict["GlowTTS"]
        kw = dict(mels_for_prosody=mv(prosodies), mel_lengths_for_prosody=mv(prosody_lengths), speakers=mv(speakers), mels_for_ge2e=mv(ge2es))
        if seeds is not None:
            kw["seeds"] = seeds
            if torch.is_tensor(noise_scale):
                noise_scale = noise_scale.to(dev)
        if "Pitch_Interpolater" in model.layer_Dict:                             # GR: the pitch track rides the eager path
            mels, mel_Lengths, attentions = model.inference(mv(tokens), mv(token_lengths), pitches=mv(pitches), pitch_lengths=mv(pitch_lengths),
                                                            noise_scale=noise_scale, length_scale=mv(length_scales), **kw)
        else:
            if self._graphed is None:
                from .graph_infer import GraphedInference
                self._graphed = GraphedInference(model)
            mels, mel_Lengths, attentions = self._graphed(mv(tokens), mv(token_lengths), noise_scale=noise_scale, length_scale=mv(length_scales), **kw)
        os.makedirs(os.path.join(inference_path, "NPY").replace("\\", "/"), exist_ok=True)
        names = [".".join([str(label)] + (["S{}".format(sample_index)] if sample_index is not None else []) +
                          (["IDX_{}".format(index + start_index)] if tag_index else [])) for index, label in enumerate(labels)]
        if wav:                                                                  # on the device, before the copy to the host
            if vocoder_seeds is not None:
                self._write_wavs(mels, mel_Lengths, names, inference_path, seeds=seeds, vocoder_seeds=vocoder_seeds)
            else:
                self._write_wavs(mels, mel_Lengths, names, inference_path, seeds=seeds)
        files = []
        for name, mel, n in zip(names, mels.cpu().numpy(), mel_Lengths.cpu().tolist()):
            path = os.path.join(inference_path, "NPY", name + ".npy").replace("\\", "/")
            np.save(path, mel[:, :n].T, allow_pickle=False)                      # [T, Mel], Inference.py:216-220
            files.append(path)
        return files

    def Inference(self, labels, texts, scales, speakers=None, references=None, inference_path="./inference", noise_scale=1.0, wav=False, seed=None, samples=1,
                  speaker_references=None):
        """Inference.py:225-256.  wav: also WAV/<label>.wav per utterance (paths in `last_wav_files`; the returned list stays the .npy files).
        seed (an int): reproducible sampling - every utterance draws its noise from `utterance_seed_words(seed, label, k)`, so its mel depends on the seed, its
        label and the sample number k only, not on the order of the prompts or Inference_Batch_Size; None: the unseeded draw.  noise_scale: the sampling
        temperature, a float or - seeded only - one float per utterance.  samples = N > 1: N takes of every prompt, written as <label>.S<k>.npy (and .wav),
        k < N; samples = 1 keeps the plain names.
        speaker_references (GE2E mode, required there): one per utterance, see `D_Vectors`.  The slices' random offset comes from `np.random` as in the
        reference or, with `seed`, from an `np.random.RandomState` of the first word of `utterance_seed_words(seed, label)`: a seeded run repeats."""
        logging.info("Start inference.")
        self.last_wav_files = []
        hp = self.hp
        samples = int(samples)
        if samples < 1:
            raise ValueError("`samples` must be at least 1")
        per_utterance = isinstance(noise_scale, (list, tuple))
        if per_utterance and seed is None:
            raise ValueError("a per-utterance `noise_scale` list needs `seed` (the unseeded draw takes one `noise_scale` for all utterances)")
        if per_utterance and len(noise_scale) != len(texts):
            raise ValueError("`noise_scale` lists one value per text")
        bs = hp.Inference_Batch_Size or hp.Train.Batch_Size
        speakers = speakers or [None] * len(texts)
        references = references or [None] * len(texts)
        if self.ge2e_mode and (speaker_references is None or len(speaker_references) != len(texts) or any(r is None for r in speaker_references)):
            raise ValueError("Speaker_Embedding.Type 'GE2E': `speaker_references` must give every utterance a wav, a mel or a d-vector (and wavs / mels need a "
                             "speaker encoder: Speaker_Embedding.GE2E.Checkpoint_Path or Inferencer(speaker_encoder=...))")
        files = []
        for s in range(0, len(texts), bs):
            sl = slice(s, s + bs)
            toks = [data.text_to_token(data.text_filtering(t), self.token_Dict) for t in texts[sl]]
            tl = torch.tensor([len(t) for t in toks], dtype=torch.int64)
            tokens = torch.full((len(toks), int(tl.max())), self.token_Dict["<E>"], dtype=torch.int64)
            for b, t in enumerate(toks):
                tokens[b, :len(t)] = torch.from_numpy(t.astype(np.int64))
            refs = references[sl]
            pros = pl = pit = pitl = None
            if not any(r is None for r in refs):                                 # Inference.py:84-100
                mp = [self._reference(r) for r in refs]
                pl = torch.tensor([m.shape[0] for m, _ in mp], dtype=torch.int64)
                pros = torch.full((len(mp), hp.Sound.Mel_Dim, int(pl.max())), -float(hp.Sound.Max_Abs_Mel))
                for b, (m, _) in enumerate(mp):
                    pros[b, :, :m.shape[0]] = torch.from_numpy(m.T)
                if all(p is not None for _, p in mp):
                    pitl = torch.tensor([p.shape[0] for _, p in mp], dtype=torch.int64)
                    pit = torch.zeros(len(mp), int(pitl.max()))
                    for b, (_, p) in enumerate(mp):
                        pit[b, :p.shape[0]] = torch.from_numpy(p)
            # (GE2E mode: the speaker is the d-vector; speaker indices, which `main` passes in every SE / GR mode, are not read)
            spk = None if self.ge2e_mode or any(x is None for x in speakers[sl]) else torch.tensor(speakers[sl], dtype=torch.int64)
            ns = torch.tensor([float(x) for x in noise_scale[sl]], dtype=torch.float32) if per_utterance else noise_scale
            ge2es = None
            if self.ge2e_mode:
                rngs = None if seed is None else [np.random.RandomState(utterance_seed_words(seed, label)[0]) for label in labels[sl]]
                ge2es = torch.from_numpy(self.D_Vectors(speaker_references[sl], rngs))
            for k in range(samples):
                seeds = None if seed is None else torch.tensor([utterance_seed_words(seed, label, k) for label in labels[sl]], dtype=torch.int64)
                vseeds = None
                if seed is not None and wav and self.vocoder_kind == "pwg":
                    from .vocoder import pwg_seed_words
                    vseeds = torch.tensor([pwg_seed_words(seed, label, k) for label in labels[sl]], dtype=torch.int64)
                files += self.Inference_Step(tokens, tl, pros, pl, spk, ge2es, pit, pitl, torch.tensor(scales[sl], dtype=torch.float32), labels[sl], texts[sl],
                                             start_index=s, inference_path=inference_path, noise_scale=ns, wav=wav, seeds=seeds,
                                             sample_index=k if samples > 1 else None, vocoder_seeds=vseeds)
        return files

    @torch.no_grad()
    def Align(self, texts, mels_or_wavs, speakers=None, speaker_references=None, pitches=None, labels=None, seed=None, noise_scale=1.0, reconstruct=False):
        """Teacher-forced pass (`GlowTTS.teacher_forced`) over recordings and their texts: the monotonic alignment of every recording to its text and,
        `reconstruct`, the model's own mel for it, frame-aligned with the recording (a ground-truth-aligned mel).  texts: strings (filtered and tokenised
        as `Inference` does) or ready token id arrays (<S> and <E> included); mels_or_wavs: one per text, the formats of `_reference` (mel array or .npy
        [T, Mel], wav file, (mel, pitch) pair); pitches: GR mode, one track per recording where the recording itself does not give one.  speakers /
        speaker_references as in `Inference` (PE / GR: the prosody vector is the recording's own).  Batches of Inference_Batch_Size, sorted by mel length;
        results in input order: one dict per utterance with label, tokens [Tt] i32, durations [Tt] i32 (frames per token, <S> and <E> included; they sum
        to `frames`), frames (the mel length cut to whole squeeze groups), score (the mean log-prior density per element along the alignment - what
        the alignment search maximised, not a likelihood) and mel ([frames, Mel] f32, or None).  seed: the noise of the reconstruction comes from
        `utterance_seed_words(seed, label, 0)`; without a seed noise_scale must be 0 (the prior's mean) - there is no unseeded draw.  GE2E mode: the random
        offset of the speaker references' slices comes from `utterance_seed_words(seed, label)` as in `Inference` and, without a seed, from the run seed 0 -
        never from `np.random` - so every result is a function of the inputs, the labels and the seed."""
        hp, dev = self.hp, self.device
        model = self.model_Dict["GlowTTS"]
        n = len(texts)
        if len(mels_or_wavs) != n:
            raise ValueError("`mels_or_wavs` gives one recording per text")
        labels = [str(x) for x in labels] if labels is not None else [str(i) for i in range(n)]
        if self.ge2e_mode and (speaker_references is None or len(speaker_references) != n or any(r is None for r in speaker_references)):
            raise ValueError("Speaker_Embedding.Type 'GE2E': `speaker_references` must give every utterance a wav, a mel or a d-vector")
        if reconstruct and seed is None and float(noise_scale) != 0.0:
            raise ValueError("a reconstruction draws its noise from `seed` only: without `seed`, `noise_scale` must be 0 (the prior's mean)")
        toks = []
        for t in texts:
            if isinstance(t, str):
                f = data.text_filtering(t)
                if f is None:
                    raise ValueError("text {!r} holds symbols outside the training alphabet".format(t))
                t = data.text_to_token(f, self.token_Dict)
            toks.append(np.asarray(t, np.int64))
        mp = [self._reference(r) for r in mels_or_wavs]
        if pitches is not None:
            mp = [(m, p if q is None else np.asarray(q, np.float32)) for (m, p), q in zip(mp, pitches)]
        gr = "Pitch_Interpolater" in model.layer_Dict
        if gr and any(p is None for _, p in mp):
            raise ValueError("GR mode: every recording needs its pitch track (a wav, a (mel, pitch) pair or `pitches`)")
        lut = "LUT" in model.layer_Dict
        if lut and (speakers is None or any(s is None for s in speakers)):
            raise ValueError("Speaker_Embedding.Type 'LUT': `speakers` must give every utterance its speaker index")
        bs = hp.Inference_Batch_Size or hp.Train.Batch_Size
        order = sorted(range(n), key=lambda i: (mp[i][0].shape[0], i))
        out = [None] * n
        for s in range(0, n, bs):
            part = order[s:s + bs]
            tl = torch.tensor([len(toks[i]) for i in part], dtype=torch.int64)
            tokens = torch.full((len(part), int(tl.max())), self.token_Dict["<E>"], dtype=torch.int64)
            for b, i in enumerate(part):
                tokens[b, :len(toks[i])] = torch.from_numpy(toks[i])
            mels, ml, pit = self._pad_mels([mp[i] if gr else (mp[i][0], None) for i in part])
            ge2es = None
            if self.ge2e_mode:
                # (no unseeded draw here either: without a seed the slices' offset comes from the label under the run seed 0, never from `np.random`)
                rngs = [np.random.RandomState(utterance_seed_words(0 if seed is None else seed, labels[i])[0]) for i in part]
                ge2es = torch.from_numpy(self.D_Vectors([speaker_references[i] for i in part], rngs)).to(dev)
            spk = torch.tensor([int(speakers[i]) for i in part], dtype=torch.int64, device=dev) if lut else None
            seeds = None if (seed is None or not reconstruct) else torch.tensor([utterance_seed_words(seed, labels[i], 0) for i in part], dtype=torch.int64)
            r = model.teacher_forced(tokens.to(dev), tl.to(dev), mels.to(dev), ml.to(dev), speakers=spk, mels_for_ge2e=ge2es,
                                     pitches=None if pit is None else pit.to(dev), noise_scale=float(noise_scale) if seeds is not None else 0.0, seeds=seeds,
                                     reconstruct=reconstruct)
            dur, score, frames = r.durations.cpu().numpy(), r.score.cpu().numpy(), r.mel_lengths.cpu().tolist()
            rec = r.mels.cpu().numpy() if reconstruct else None
            for b, i in enumerate(part):
                out[i] = {"label": labels[i], "tokens": toks[i].astype(np.int32), "durations": dur[b, :len(toks[i])].copy(), "frames": int(frames[b]),
                          "score": float(score[b]), "mel": np.ascontiguousarray(rec[b, :, :frames[b]].T) if reconstruct else None}
        return out

    def Vocode(self, labels, mels, inference_path="./inference"):
        """Recorded or previously generated mels - .npy paths or arrays [T, Mel] - through the active vocoder, in batches of Inference_Batch_Size:
        one WAV/<label>.wav per mel; returns the written files (also in `last_wav_files`)."""
        logging.info("Start vocoding.")
        hp = self.hp
        bs = hp.Inference_Batch_Size or hp.Train.Batch_Size
        self.last_wav_files = []
        for s in range(0, len(mels), bs):
            sl = slice(s, s + bs)
            batch, lengths, _ = self._pad_mels([(np.load(m).astype(np.float32) if isinstance(m, str) else np.asarray(m, np.float32), None) for m in mels[sl]])
            self._write_wavs(batch.to(self.device), lengths.to(self.device), [str(x) for x in labels[sl]], inference_path)
        return list(self.last_wav_files)


    def _pad_mels(self, mp):
        """[(mel [T, Mel], pitch [T] or None)] -> (mels [B, Mel, Tmax] padded with -Max_Abs_Mel, lengths, pitches [B, Tmax] or None)"""
        hp = self.hp
        lengths = torch.tensor([m.shape[0] for m, _ in mp], dtype=torch.int64)
        mels = torch.full((len(mp), hp.Sound.Mel_Dim, int(lengths.max())), -float(hp.Sound.Max_Abs_Mel))
        for b, (m, _) in enumerate(mp):
            mels[b, :, :m.shape[0]] = torch.from_numpy(m.T)
        pitches = None
        if all(p is not None for _, p in mp):
            pitches = torch.zeros(len(mp), int(lengths.max()))
            for b, (_, p) in enumerate(mp):
                n = min(p.shape[0], mels.shape[2])
                pitches[b, :n] = torch.from_numpy(p[:n])
        return mels, lengths, pitches

    def Voice_Conversion(self, labels, sources, source_speakers=None, target_speakers=None, target_references=None, inference_path="./inference",
                         wav=False):
        """Voice conversion through the invertible decoder (GlowTTS.voice_conversion): `sources` - recorded mels as .npy files / arrays [T, Mel]
        or wav files (GR: a wav also gives the YIN pitch track the flows read; (mel, pitch) pairs are taken as they are) - go through the flows
        forward under their own conditioning and back under the target's.  SE-LUT: speaker indices; SE-GE2E: d-vectors [E], wav files or mels (`D_Vectors`); PE / GR:
        `target_references` (same formats as `sources`) give the target prosody vector (GR: plus the target speaker).  A None target takes
        the source's value.  Batches of Inference_Batch_Size; one NPY/<label>.npy [T, Mel] per utterance (wav: and WAV/<label>.wav, paths in
        `last_wav_files`); returns the written .npy files."""
        logging.info("Start voice conversion.")
        self.last_wav_files = []
        hp = self.hp
        model = self.model_Dict["GlowTTS"]
        mode = hp.Mode.upper()
        lut = "LUT" in model.layer_Dict
        bs = hp.Inference_Batch_Size or hp.Train.Batch_Size
        n = len(sources)
        source_speakers = source_speakers or [None] * n
        target_speakers = target_speakers or [None] * n
        target_references = target_references or [None] * n
        os.makedirs(os.path.join(inference_path, "NPY").replace("\\", "/"), exist_ok=True)
        dev = self.device

        def speakers_of(vals):
            if any(v is None for v in vals):
                return None
            if lut:
                return torch.tensor([int(v) for v in vals], dtype=torch.int64, device=dev)
            if not self.ge2e_mode:
                return torch.from_numpy(np.stack([np.asarray(v, np.float32) for v in vals])).to(dev)
            return torch.from_numpy(self.D_Vectors([v if isinstance(v, str) or torch.is_tensor(v) else np.asarray(v, np.float32) for v in vals])).to(dev)

        files = []
        for s in range(0, n, bs):
            sl = slice(s, s + bs)
            mels, lengths, pitches = self._pad_mels([self._reference(r) for r in sources[sl]])
            spk, tspk = speakers_of(source_speakers[sl]), speakers_of(target_speakers[sl])
            kw = {}
            if mode in ("SE", "GR") and lut:
                kw.update(speakers=spk, target_speakers=tspk)
            elif mode in ("SE", "GR"):
                kw.update(mels_for_ge2e=spk, target_mels_for_ge2e=tspk)
            refs = target_references[sl]
            if mode in ("PE", "GR") and not any(r is None for r in refs):
                tm, tl, _ = self._pad_mels([self._reference(r) for r in refs])
                kw.update(target_mels_for_prosody=tm.to(dev), target_mel_lengths_for_prosody=tl.to(dev))
            out, out_lengths = model.voice_conversion(mels.to(dev), lengths.to(dev), pitches=None if pitches is None else pitches.to(dev), **kw)
            if wav:
                self._write_wavs(out, out_lengths, [str(x) for x in labels[sl]], inference_path)
            for label, mel, m in zip(labels[sl], out.cpu().numpy(), out_lengths.cpu().tolist()):
                path = os.path.join(inference_path, "NPY", "{}.npy".format(label)).replace("\\", "/")
                np.save(path, mel[:, :m].T, allow_pickle=False)                   # [T, Mel], like Inference_Step
                files.append(path)
        return files


def read_convert_list(path):
    """The --convert TSV: label, source path, source speaker, target speaker and, optionally, a target reference path, tab-separated; an
    optional header line whose first column is `Label`.  Empty speaker / reference columns are None; a speaker column that is not an integer is kept as a
    string: the path of a wav or `.npy` mel (GE2E mode)."""
    out = []
    with open(path, "r", encoding="utf-8") as f:
        for i, line in enumerate(f.read().splitlines()):
            if not line.strip():
                continue
            cols = [x.strip() for x in line.split("\t")]
            if i == 0 and cols[0].lower() == "label":
                continue
            if len(cols) < 4:
                raise ValueError("{}:{}: expected label, source, source speaker, target speaker[, target reference]".format(path, i + 1))
            def spk(x):
                if not x:
                    return None
                try:
                    return int(x)
                except ValueError:
                    return x
            out.append({"label": cols[0], "source": cols[1], "source_speaker": spk(cols[2]), "target_speaker": spk(cols[3]),
                        "target_reference": (cols[4] or None) if len(cols) > 4 else None})
    return out


def read_vocode_list(path):
    """The --vocode list: one `label<TAB>mel.npy` per line; blank lines are skipped.  -> [(label, mel path)]"""
    out = []
    with open(path, "r", encoding="utf-8") as f:
        for i, line in enumerate(f.read().splitlines()):
            if not line.strip():
                continue
            cols = [x.strip() for x in line.split("\t")]
            if len(cols) != 2 or not cols[0] or not cols[1]:
                raise ValueError("{}:{}: expected label<TAB>mel.npy".format(path, i + 1))
            out.append((cols[0], cols[1]))
    return out


def build_parser():
    """The command line of Inference.py."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--checkpoint", required=True)
    ap.add_argument("-t", "--prompts", default=None, help="inference prompt TSV (Datasets.py:137-144); default: the reference's two example sentences")
    ap.add_argument("-o", "--out", default="./inference")
    ap.add_argument("--convert", default=None, metavar="LIST.tsv",
                    help="voice conversion instead of text-to-mel: label, source mel (.npy [T, Mel] or wav), source speaker, target speaker[, target reference]")
    ap.add_argument("--wav", action="store_true", help="also write WAV/<label>.wav per utterance: Griffin-Lim (a baseline vocoder, not a neural one) or, see --vocoder, the Parallel WaveGAN or the HiFi-GAN generator")
    ap.add_argument("--vocoder", choices=["griffin_lim", "pwg", "hifigan"], default=None,
                    help="the vocoder behind --wav / --vocode: pwg / hifigan = the neural vocoders (Parallel WaveGAN / HiFi-GAN generator; they need a checkpoint), "
                         "griffin_lim = the baseline; default: hifigan when the yaml's `Vocoder` block has Type: 'HiFiGAN', pwg for any other `Vocoder` block or when "
                         "--vocoder-checkpoint is given, else griffin_lim")
    ap.add_argument("--vocoder-checkpoint", default=None, metavar="PATH", help="generator checkpoint of the neural vocoder (overrides Vocoder.Checkpoint_Path of the yaml)")
    ap.add_argument("--vocoder-precision", choices=["f32", "bf16", "f16"], default=None,
                    help="arithmetic of the neural vocoder's layers (overrides Vocoder.Precision of the yaml; default f32): bf16 (--vocoder pwg) rounds the layers' "
                         "operands, weights and gate to bf16, f16 (--vocoder hifigan) the convolutions' rows and weights to fp16 - faster, and with --seed its own "
                         "reproducible wav, not the f32 one")
    ap.add_argument("--vocode", default=None, metavar="LIST", help="vocode existing mels instead of synthesising: one label<TAB>mel.npy ([T, Mel]) per line")
    ap.add_argument("--device-frontend", action="store_true", help="analyse wav references / conversion sources on the device instead of the host")
    ap.add_argument("--seed", type=int, default=None, help="reproducible sampling: an utterance's mel depends on this seed, its label and the sample number only")
    ap.add_argument("--noise-scale", type=float, default=1.0, help="sampling temperature (the standard deviation of the prior is multiplied by it)")
    ap.add_argument("--samples", type=int, default=1, help="takes per prompt; N > 1 writes <label>.S<k>.npy (and .wav) for k < N")
    return ap


def main(argv=None):
    logging.basicConfig(level=logging.INFO)
    args = build_parser().parse_args(argv)
    inf = Inferencer(checkpoint_path=args.checkpoint, device_frontend=args.device_frontend, vocoder=args.vocoder, vocoder_checkpoint=args.vocoder_checkpoint,
                     vocoder_precision=args.vocoder_precision)
    if args.vocode:
        recs = read_vocode_list(args.vocode)
        print("\n".join(inf.Vocode([r[0] for r in recs], [r[1] for r in recs], args.out)))
        return
    if args.convert:
        recs = read_convert_list(args.convert)
        print("\n".join(inf.Voice_Conversion([r["label"] for r in recs], [r["source"] for r in recs], [r["source_speaker"] for r in recs],
                                              [r["target_speaker"] for r in recs], [r["target_reference"] for r in recs], args.out, wav=args.wav)
                        + inf.last_wav_files))
        return
    speaker_references = None
    if args.prompts:
        recs = [r for r in data.read_inference_prompts(args.prompts) if r["text"] is not None]
        labels, texts, scales, speakers = [r["label"] for r in recs], [r["text"] for r in recs], [r["length_scale"] for r in recs], [r["speaker"] for r in recs]
        if inf.ge2e_mode:                                                          # Inference.py:84-100: the prompt's wav for GE2E
            speaker_references = [r["wav_for_ge2e"] for r in recs]
    else:                                                                         # Inference.py:290-301
        labels, texts, scales, speakers = ["Alpha", "Bravo"], ["Birds of a feather flock together.",
                                                               "A creative artist works on his next composition because he was not satisfied with his previous one."], [1.0, 0.9], [0, 1]
    mode = inf.hp.Mode.upper()
    print("\n".join(inf.Inference(labels, texts, scales, speakers if mode in ("SE", "GR") else None, None, args.out, wav=args.wav, seed=args.seed,
                                  noise_scale=args.noise_scale, samples=args.samples, speaker_references=speaker_references) + inf.last_wav_files))
