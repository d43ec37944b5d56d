"""The GE2E speaker encoder (DESIGN.md "GE2E speaker encoder"): `Speaker_Embedding.GE2E.LSTM.Stacks` LSTM layers of width `.Sizes` over a mel slice, a linear
layer to `Speaker_Embedding.Embedding_Size`, L2 normalisation per slice, the mean over an utterance's slices, L2 normalisation again - the d-vector `GlowTTS`
takes as `mels_for_ge2e`.  The reference runs a pre-trained network of this kind inside `GlowTTS.forward` / `inference` (Modules.py:29-35, 75-77, 154-156); its
source is an un-vendored submodule, so the network is restated here as this project's own contract and the checkpoint layout is NOT pinned against a real file:
CHECKPOINT_NAMES is the one place a differently named checkpoint is mapped.  Device only, no CPU fallback: the inference forward is csrc/ge2e_ops.hip;
`GE2E(..., trainable=True).embed` and `GE2ELoss` are the training path (csrc/ge2e_train_ops.hip, DESIGN.md "Training the GE2E speaker encoder")."""
import logging

import torch

from . import _lib, abi

# parameter of this module -> its name in a checkpoint ({k}: the layer); torch.nn.LSTM's and torch.nn.Linear's own names on both sides
CHECKPOINT_NAMES = {
    "lstm.weight_ih_l{k}": "lstm.weight_ih_l{k}",
    "lstm.weight_hh_l{k}": "lstm.weight_hh_l{k}",
    "lstm.bias_ih_l{k}": "lstm.bias_ih_l{k}",
    "lstm.bias_hh_l{k}": "lstm.bias_hh_l{k}",
    "linear.weight": "linear.weight",
    "linear.bias": "linear.bias",
}
GLOWTTS_PREFIX = "layer_Dict.GE2E."                                         # where a reference GlowTTS checkpoint carries the encoder (Modules.py:30-35)
KEYS = {"H": "Speaker_Embedding.GE2E.LSTM.Sizes", "Stacks": "Speaker_Embedding.GE2E.LSTM.Stacks", "E": "Speaker_Embedding.Embedding_Size", "Mel": "Sound.Mel_Dim"}


def ge2e_sizes(hp):
    """{Mel, H, Stacks, E} of a Hyper_Parameters namespace"""
    ge = hp.Speaker_Embedding.GE2E
    return {"Mel": int(hp.Sound.Mel_Dim), "H": int(ge.LSTM.Sizes), "Stacks": int(ge.LSTM.Stacks), "E": int(hp.Speaker_Embedding.Embedding_Size)}


def ge2e_check_sizes(sizes):
    """Raises a ValueError naming the yaml keys of every size the kernels do not support (include/glowtts_hip.h, glowtts_ge2e_supported)."""
    Mel, H, Stacks, E = (int(sizes[k]) for k in ("Mel", "H", "Stacks", "E"))
    bad = []
    if Mel < 4 or Mel % 4 or Mel > abi.GE2E_MAX_MEL:
        bad.append("{} = {} (a multiple of 4, at most {})".format(KEYS["Mel"], Mel, abi.GE2E_MAX_MEL))
    if H < 16 or H % 16 or H > abi.GE2E_MAX_H:
        bad.append("{} = {} (a multiple of 16, at most {})".format(KEYS["H"], H, abi.GE2E_MAX_H))
    if not 1 <= Stacks <= abi.GE2E_MAX_STACKS:
        bad.append("{} = {} (1 .. {})".format(KEYS["Stacks"], Stacks, abi.GE2E_MAX_STACKS))
    if not 1 <= E <= abi.GE2E_MAX_E:
        bad.append("{} = {} (1 .. {})".format(KEYS["E"], E, abi.GE2E_MAX_E))
    if bad:
        raise ValueError("the GE2E speaker encoder does not support " + "; ".join(bad))


def ge2e_shapes(sizes):
    """parameter name of this module -> shape"""
    Mel, H, Stacks, E = (int(sizes[k]) for k in ("Mel", "H", "Stacks", "E"))
    out = {}
    for k in range(Stacks):
        out["lstm.weight_ih_l{}".format(k)] = (4 * H, Mel if k == 0 else H)
        out["lstm.weight_hh_l{}".format(k)] = (4 * H, H)
        out["lstm.bias_ih_l{}".format(k)] = (4 * H,)
        out["lstm.bias_hh_l{}".format(k)] = (4 * H,)
    out["linear.weight"], out["linear.bias"] = (E, H), (E,)
    return out


def _checkpoint_name(name):
    """this module's parameter name -> the checkpoint's (through CHECKPOINT_NAMES)"""
    for mine, theirs in CHECKPOINT_NAMES.items():
        if "{k}" not in mine:
            if name == mine:
                return theirs
            continue
        head, tail = mine.split("{k}")
        if name.startswith(head) and name.endswith(tail) and name[len(head):len(name) - len(tail)].isdigit():
            return theirs.format(k=name[len(head):len(name) - len(tail)])
    raise KeyError(name)


def _roots():
    return sorted({theirs.split(".")[0] + "." for theirs in CHECKPOINT_NAMES.values()})


def ge2e_find_state_dict(obj):
    """The encoder's tensors inside a loaded checkpoint object, as {checkpoint name: tensor} with any prefix stripped, or None.  Looked for, in this order: at the
    top level, under the `layer_Dict.GE2E.` prefix at the top level, under 'Model' (the reference reads `state_Dict['Model']`), under that prefix inside 'Model'
    (a GlowTTS checkpoint)."""
    def at(d):
        if not isinstance(d, dict):
            return None
        keys = [k for k in d if isinstance(k, str)]
        if any(k.startswith(r) for k in keys for r in _roots()):
            return {k: d[k] for k in keys if torch.is_tensor(d[k]) or any(k.startswith(r) for r in _roots())}
        if any(k.startswith(GLOWTTS_PREFIX) for k in keys):
            return {k[len(GLOWTTS_PREFIX):]: d[k] for k in keys if k.startswith(GLOWTTS_PREFIX)}
        return None
    found = at(obj)
    if found is None and isinstance(obj, dict):
        found = at(obj.get("Model"))
    return found


def ge2e_load(obj, sizes):
    """-> {this module's parameter name: float32 tensor} from a checkpoint object (`ge2e_find_state_dict`).  A missing, surplus or wrongly shaped tensor raises
    a ValueError naming the key."""
    found = ge2e_find_state_dict(obj)
    if found is None:
        raise ValueError("no GE2E speaker encoder in the checkpoint: expected keys such as '{}' at the top level, under 'Model' or under the '{}' prefix"
                         .format(_checkpoint_name("lstm.weight_ih_l0"), GLOWTTS_PREFIX))
    out, used = {}, set()
    for name, shape in ge2e_shapes(sizes).items():
        key = _checkpoint_name(name)
        if key not in found:
            raise ValueError("GE2E checkpoint: missing key '{}' (shape {})".format(key, list(shape)))
        t = found[key]
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
            raise ValueError("GE2E checkpoint: key '{}' has shape {}, expected {} ({})".format(
                key, list(t.shape) if torch.is_tensor(t) else type(t).__name__, list(shape), ", ".join("{} = {}".format(KEYS[k], sizes[k]) for k in ("Mel", "H", "Stacks", "E"))))
        out[name] = t.detach().to(torch.float32)
        used.add(key)
    surplus = sorted(set(found) - used)
    if surplus:
        raise ValueError("GE2E checkpoint: surplus key '{}'".format(surplus[0]))
    return out


class GE2E(torch.nn.Module):
    """hp: the Hyper_Parameters namespace; state_dict: a checkpoint object for `ge2e_load` (None: torch's default initialisation).  Calling it maps the slice stack
    [B * Samples, Mel, Slice] to unit-norm d-vectors [B, Embedding_Size] under no_grad through `glowtts_ge2e_forward` alone.  The parameters live in a
    torch.nn.LSTM + torch.nn.Linear (their names are the state dict's) that is never called.  trainable=True: the parameters require gradients and
    `embed` maps a slice stack to the raw embeddings e [N, Embedding_Size] with a backward (`_Embed`); the plain call stays the frozen inference path."""

    def __init__(self, hp, device, state_dict=None, trainable=False):
        super().__init__()
        self.sizes = ge2e_sizes(hp)
        ge2e_check_sizes(self.sizes)
        self.samples = int(hp.Speaker_Embedding.GE2E.Inference.Samples)
        loaded = ge2e_load(state_dict, self.sizes) if state_dict is not None else None
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.GlowTTSHipError("the GE2E speaker encoder runs on the device only (the HIP path has no CPU fallback)")
        s = self.sizes
        self.lstm = torch.nn.LSTM(s["Mel"], s["H"], s["Stacks"], batch_first=True)
        self.linear = torch.nn.Linear(s["H"], s["E"])
        if loaded is not None:
            torch.nn.Module.load_state_dict(self, loaded, strict=True)
        self.trainable = bool(trainable)
        if self.trainable:
            self.to(device).requires_grad_(True)
        else:
            self.to(device).requires_grad_(False).eval()
        self._images = self._biases = self._images_t = self._packed_sig = None

    @classmethod
    def from_checkpoint(cls, hp, device, path):
        return cls(hp, device, state_dict=torch.load(path, map_location="cpu"))

    def _lstm_params(self):
        return [[getattr(self.lstm, "{}_l{}".format(n, k)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] for k in range(self.sizes["Stacks"])]

    def _pack(self):
        """The weight images and summed biases: packed at the first call and again only when a parameter has been replaced or written since."""
        params = self._lstm_params()
        sig = tuple((p.data_ptr(), p._version) for layer in params for p in layer)
        if sig == self._packed_sig:
            return
        s, L = self.sizes, _lib.api()
        dev = params[0][0].device
        if self._images is None or self._images.device != dev:
            self._images = torch.empty(L.glowtts_ge2e_image_floats(s["Mel"], s["H"], s["Stacks"]), dtype=torch.float32, device=dev)
            self._biases = torch.empty(s["Stacks"], 4 * s["H"], dtype=torch.float32, device=dev)
        for k, layer in enumerate(params):
            L.glowtts_ge2e_pack(*[_lib.ptr(p) for p in layer], _lib.ptr(self._images), _lib.ptr(self._biases), k, s["Mel"], s["H"], s["Stacks"], _lib.stream())
        if self.trainable:                                                  # the backward's transposed images: re-packed exactly when the forward's are
            if self._images_t is None or self._images_t.device != dev:
                self._images_t = torch.empty(L.glowtts_ge2e_train_image_floats(s["H"], s["Stacks"]), dtype=torch.float32, device=dev)
            for k, layer in enumerate(params):
                above = _lib.ptr(params[k + 1][0]) if k + 1 < s["Stacks"] else None
                L.glowtts_ge2e_train_pack(_lib.ptr(layer[1]), above, _lib.ptr(self._images_t), k, s["H"], s["Stacks"], _lib.stream())
        self._packed_sig = sig

    def invalidate_images(self):
        """The parameters were written behind torch's version counters (the `optim` kernels update them through raw pointers): pack again at the next call."""
        self._packed_sig = None

    def _check_stack(self, stack):
        s = self.sizes
        if stack.dim() != 3 or stack.shape[1] != s["Mel"] or stack.shape[0] < 1 or stack.shape[2] < 1:
            raise ValueError("GE2E: expected a slice stack [N, {}, Slice], got {}".format(s["Mel"], list(stack.shape)))
        if stack.dtype != torch.float32 or not stack.is_cuda:
            raise _lib.GlowTTSHipError("GE2E: expected an fp32 device tensor (the HIP path has no CPU fallback)")

    def embed(self, stack):
        """stack [N, Mel, T] fp32 on the device -> the raw embeddings e [N, E] (before any normalisation), differentiable in the parameters.  After an
        optimizer step of `optim.RAdam` call `invalidate_images()` (torch's own in-place ops are seen without it)."""
        if not self.trainable:
            raise _lib.GlowTTSHipError("GE2E.embed is the training path: construct the encoder with trainable=True")
        self._check_stack(stack)
        flat = [p for layer in self._lstm_params() for p in layer] + [self.linear.weight, self.linear.bias]
        return _Embed.apply(self, stack.detach().contiguous(), *flat)

    @torch.no_grad()
    def forward_all(self, stack, samples=None, hidden=False, raw=False):
        """stack [N = B * samples, Mel, T] fp32 on the device -> (hs [Stacks, N, T, H] or None, e [N, E] or None, d [B, E])"""
        s, L = self.sizes, _lib.api()
        samples = self.samples if samples is None else int(samples)
        if stack.dim() != 3 or stack.shape[1] != s["Mel"] or stack.shape[0] < 1 or stack.shape[2] < 1 or stack.shape[0] % samples:
            raise ValueError("GE2E: expected a slice stack [B * {}, {}, Slice], got {}".format(samples, s["Mel"], list(stack.shape)))
        if stack.dtype != torch.float32 or not stack.is_cuda:
            raise _lib.GlowTTSHipError("GE2E: expected an fp32 device tensor (the HIP path has no CPU fallback)")
        self._pack()
        x = stack if stack.is_contiguous() else stack.contiguous()
        N, _, T = x.shape
        dev = x.device
        hs = torch.empty(s["Stacks"], N, T, s["H"], dtype=torch.float32, device=dev) if hidden else None
        e = torch.empty(N, s["E"], dtype=torch.float32, device=dev) if raw else None
        d = torch.empty(N // samples, s["E"], dtype=torch.float32, device=dev)
        work = torch.empty(s["Stacks"] * N * s["H"] * (1 if hidden else T + 1), dtype=torch.float32, device=dev)
        L.glowtts_ge2e_forward(_lib.ptr(x), _lib.ptr(self._images), _lib.ptr(self._biases), _lib.ptr(self.linear.weight), _lib.ptr(self.linear.bias),
                               _lib.ptr(work), _lib.ptr(hs), _lib.ptr(e), _lib.ptr(d), N, samples, s["Mel"], T, s["H"], s["Stacks"], s["E"], _lib.stream())
        return hs, e, d

    def forward(self, stack, samples=None):
        return self.forward_all(stack, samples)[2]


def train_forward(enc, x):
    """-> (keep, e): `glowtts_ge2e_train_forward` of a trainable encoder on x [N, Mel, T] (contiguous)"""
    s, L = enc.sizes, _lib.api()
    enc._pack()
    N, _, T = x.shape
    keep = torch.empty(L.glowtts_ge2e_train_keep_floats(N, T, s["H"], s["Stacks"]), dtype=torch.float32, device=x.device)
    e = torch.empty(N, s["E"], dtype=torch.float32, device=x.device)
    L.glowtts_ge2e_train_forward(_lib.ptr(x), _lib.ptr(enc._images), _lib.ptr(enc._biases), _lib.ptr(enc.linear.weight), _lib.ptr(enc.linear.bias),
                                 _lib.ptr(keep), _lib.ptr(e), N, s["Mel"], T, s["H"], s["Stacks"], s["E"], _lib.stream())
    return keep, e


def train_backward(enc, x, keep, de, da=None):
    """-> {parameter name: gradient} (and da [Stacks, N, T, 4 H] is filled when given): `glowtts_ge2e_train_backward`, then `glowtts_ge2e_train_wgrad`
    per layer.  The images are those of the forward (`_pack` ran there)."""
    s, L = enc.sizes, _lib.api()
    N, _, T = x.shape
    dev = x.device
    if da is None:
        da = torch.empty(s["Stacks"], N, T, 4 * s["H"], dtype=torch.float32, device=dev)
    work = torch.empty(L.glowtts_ge2e_train_work_floats(N, T, s["Mel"], s["H"], s["Stacks"]), dtype=torch.float32, device=dev)
    grads = {name: torch.empty(shape, dtype=torch.float32, device=dev) for name, shape in ge2e_shapes(s).items()}
    L.glowtts_ge2e_train_backward(_lib.ptr(enc._images_t), _lib.ptr(keep), _lib.ptr(enc.linear.weight), _lib.ptr(de), _lib.ptr(da), _lib.ptr(work),
                                  _lib.ptr(grads["linear.weight"]), _lib.ptr(grads["linear.bias"]), N, T, s["H"], s["Stacks"], s["E"], _lib.stream())
    for k in range(s["Stacks"]):
        g = [grads["lstm.{}_l{}".format(n, k)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        L.glowtts_ge2e_train_wgrad(_lib.ptr(x), _lib.ptr(keep), _lib.ptr(da), _lib.ptr(work), *[_lib.ptr(t) for t in g], k, N, s["Mel"], T, s["H"],
                                   s["Stacks"], _lib.stream())
    return grads


class _Embed(torch.autograd.Function):
    """e = GE2E.embed(stack): forward and backward are the HIP launches of csrc/ge2e_train_ops.hip; the gradient of the input is not computed."""

    @staticmethod
    def forward(ctx, enc, x, *flat):
        keep, e = train_forward(enc, x)
        ctx.enc, ctx.x, ctx.keep = enc, x, keep
        return e

    @staticmethod
    def backward(ctx, de):
        enc = ctx.enc
        grads = train_backward(enc, ctx.x, ctx.keep, de.contiguous())
        ctx.keep = None
        order = ["lstm.{}_l{}".format(n, k) for k in range(enc.sizes["Stacks"]) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        return (None, None) + tuple(grads[n] for n in order + ["linear.weight", "linear.bias"])


def ge2e_loss_launch(e, w, S, M):
    """-> (loss [1], de [N, E], dw [1]) of `glowtts_ge2e_train_loss` for e [S M, E] (row j M + i: speaker j's utterance i) and the device scalar w"""
    L = _lib.api()
    N, E = e.shape
    dev = e.device
    work = torch.empty(L.glowtts_ge2e_train_loss_work_floats(N, S, E), dtype=torch.float32, device=dev)
    loss, dw, de = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev), torch.empty_like(e)
    L.glowtts_ge2e_train_loss(_lib.ptr(e), _lib.ptr(w), _lib.ptr(work), _lib.ptr(loss), _lib.ptr(de), _lib.ptr(dw), S, M, E, _lib.stream())
    return loss, de, dw


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, w, S, M):
        loss, de, dw = ge2e_loss_launch(e.detach().contiguous(), w.detach(), S, M)
        ctx.save_for_backward(de, dw)
        ctx.w_shape = w.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        de, dw = ctx.saved_tensors
        return de * g, (dw * g).reshape(ctx.w_shape), None, None


class GE2ELoss(torch.nn.Module):
    """The GE2E softmax loss (Wan et al. 2018, eq. 6 with the exclusive centroid of eq. 8-9) over raw embeddings e [speakers * utterances, E], speaker-major.
    Invariant to a bias on the scores, so its one parameter is the scale `w`."""

    def __init__(self, init_w=10.0):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(float(init_w)))

    def forward(self, e, speakers, utterances):
        S, M = int(speakers), int(utterances)
        if S < 2 or M < 2 or e.dim() != 2 or e.shape[0] != S * M:
            raise ValueError("GE2ELoss: expected e [speakers * utterances, E] with speakers >= 2 and utterances >= 2, got {} for {} x {}".format(
                list(e.shape), S, M))
        if e.shape[1] > abi.GE2E_MAX_E:
            raise ValueError("GE2ELoss: {} = {} (at most {})".format(KEYS["E"], e.shape[1], abi.GE2E_MAX_E))
        if e.dtype != torch.float32 or not e.is_cuda or not self.w.is_cuda:
            raise _lib.GlowTTSHipError("GE2ELoss: expected fp32 device tensors (the HIP path has no CPU fallback)")
        return _Loss.apply(e, self.w, S, M)


def from_glowtts_checkpoint(hp, device, model_state):
    """The encoder a GlowTTS checkpoint carries under `layer_Dict.GE2E.*`, or None (no such keys; keys of another layout: a warning, and they are dropped)."""
    if not any(isinstance(k, str) and k.startswith(GLOWTTS_PREFIX) for k in model_state):
        return None
    try:
        return GE2E(hp, device, state_dict={k: v for k, v in model_state.items() if k.startswith(GLOWTTS_PREFIX)})
    except ValueError as err:
        logging.warning("the checkpoint's %s* keys are not this package's GE2E speaker encoder and are dropped: %s", GLOWTTS_PREFIX, err)
        return None
