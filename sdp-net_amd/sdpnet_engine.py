"""Host-side plumbing shared by the drop-in modules (layers.py / model.py).

* compute-dtype policy: bf16 when the input is bf16, the module's parameters are
  bf16, or a CUDA bf16 autocast region is active (the reference's "bf16 forward"
  is autocast, training_tools.py:85); fp32 otherwise.
* activation callables -> epilogue codes (model.py:13-24 registry, KeLu).
* per-module prepared-weight caches (bf16 casts, fused Wqkv, padded patch
  weight), keyed on the parameters' version counters and addresses so
  load_state_dict / optimizer steps invalidate them (sdpnet_train.AdamW, which
  writes through raw addresses, bumps the counters itself); ``invalidate`` for
  writes nobody can see.  Not part of the state_dict.
"""
from __future__ import annotations

from typing import Callable, Dict, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

import sdpnet_hip as sp


def compute_dtype(x: torch.Tensor, module: nn.Module) -> torch.dtype:
    if not x.is_cuda:
        raise RuntimeError("sdpnet: the HIP forward needs CUDA (ROCm) tensors; there is no CPU fallback "
                           "(move the model and inputs with .to('cuda'))")
    if x.dtype == torch.float16:
        raise TypeError("sdpnet HIP path supports float32 and bfloat16 (not float16)")
    if torch.is_autocast_enabled("cuda"):
        ad = torch.get_autocast_dtype("cuda")
        if ad == torch.bfloat16:
            return torch.bfloat16
        raise TypeError(f"sdpnet HIP path supports bf16 autocast only, got {ad}")
    if x.dtype == torch.bfloat16:
        return torch.bfloat16
    for p in module.parameters():
        if p.dtype == torch.bfloat16:
            return torch.bfloat16
        break
    return torch.float32


def act_code(fn: Callable) -> int:
    """Map the reference's activation objects to epilogue codes."""
    if fn is None:
        return 0
    if isinstance(fn, nn.GELU):
        if fn.approximate != "none":
            # nn.GELU("fast") (model.py:16) raises at forward in the reference too.
            raise RuntimeError(f"approximate argument must be either none or tanh (got {fn.approximate!r}); "
                               "the HIP path implements exact-erf GELU only")
        return sp.ACT_CODES["gelu"]
    if fn is F.gelu:
        return sp.ACT_CODES["gelu"]
    if isinstance(fn, nn.ReLU) or fn is F.relu or fn is torch.relu:
        return sp.ACT_CODES["relu"]
    if isinstance(fn, nn.Tanh) or fn is torch.tanh:
        return sp.ACT_CODES["tanh"]
    if isinstance(fn, nn.Sigmoid) or fn is torch.sigmoid:
        return sp.ACT_CODES["sigmoid"]
    if isinstance(fn, nn.LeakyReLU):
        if abs(fn.negative_slope - 0.01) > 0:
            raise NotImplementedError("sdpnet HIP path implements LeakyReLU(0.01) only")
        return sp.ACT_CODES["leaky_relu"]
    if isinstance(fn, nn.SELU) or fn is F.selu:
        return sp.ACT_CODES["selu"]
    if isinstance(fn, nn.Identity):
        return sp.ACT_CODES["none"]
    if getattr(fn, "__name__", "") == "KeLu":
        return sp.ACT_CODES["kelu"]
    raise NotImplementedError(f"sdpnet HIP path: unsupported activation {fn!r}")


def _key(params, dtype, device):
    # a tensor made under torch.inference_mode() (TeacherModel.forward) has no version counter
    return (dtype, str(device)) + tuple((-1 if p.is_inference() else p._version, p.data_ptr()) for p in params)


_INVALIDATIONS = 0  # bumped by every invalidation the version key cannot show (GraphedForward watches it)


def _drop_cache(module: nn.Module, incompatible_keys=None) -> None:
    """load_state_dict post-hook of every module that holds a cache: the copy into an inference
    tensor (no version counter, _key) is a write the key cannot see."""
    global _INVALIDATIONS
    _INVALIDATIONS += 1
    module.__dict__.pop("_sdp_cache", None)


def invalidate(module: nn.Module) -> None:
    """Drop the prepared-weight caches of ``module`` and its children; the next forward rebuilds
    them from the parameters as they are.  For writes torch's version counters do not record:
    ``p.data.mul_()`` / ``p.data.copy_()``, a kernel of your own writing through ``data_ptr()``.
    (Optimizers, ``load_state_dict``, ``nn.init`` and in-place ops on ``p`` / ``p.detach()`` are
    seen and need no call; sdpnet_train.AdamW marks what it writes.)"""
    global _INVALIDATIONS
    _INVALIDATIONS += 1
    for m in module.modules():
        m.__dict__.pop("_sdp_cache", None)


def cached(module: nn.Module, name: str, params, dtype: torch.dtype, build: Callable[[], Dict]):
    """Return module._sdp_cache[name] rebuilt when any param changed (its version counter or its
    address; see ``invalidate`` for the writes neither shows)."""
    cache = module.__dict__.get("_sdp_cache")
    if cache is None:
        cache = module.__dict__["_sdp_cache"] = {}
        if not any(h is _drop_cache for h in module._load_state_dict_post_hooks.values()):
            module.register_load_state_dict_post_hook(_drop_cache)
    params = [p for p in params if p is not None]
    key = _key(params, dtype, params[0].device if params else "cpu")
    ent = cache.get(name)
    if ent is None or ent[0] != key:
        with torch.no_grad():
            ent = (key, build())
        cache[name] = ent
    return ent[1]


def as_dtype(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Cast a parameter for the kernels (HIP cast kernel; no copy when already right)."""
    t = t.detach()
    if not t.is_contiguous():
        t = t.contiguous()
    if t.dtype == dtype:
        return t
    return sp.cast(t, dtype)


def f32(t):
    return None if t is None else as_dtype(t, torch.float32)


def num_reg_rows(max_num: int, num_registers: int) -> int:
    """Rows selected by `buffer[:num_registers+1]` (layers.py:157, :206)."""
    return len(range(max_num)[: num_registers + 1])


def reg_rows(model: nn.Module, num_registers: int) -> int:
    """Register rows R at the head of every image's token rows."""
    emb = model.embedding_layer
    conv_emb = not hasattr(emb, "horizontal_embedding_layer")
    return num_reg_rows(emb.register.shape[0] if conv_emb else emb.max_num_registers, num_registers)


def out_features(model: nn.Module) -> int:
    """Width of the logits: the head's last Linear."""
    return [m for m in model.output_head.output_head if isinstance(m, nn.Linear)][-1].out_features


def geometry(model: nn.Module, image_shape, num_registers: int):
    """(B, R, Hp, Wp, N, C) of a MainModel forward on an image batch of ``image_shape``: the patch
    grid, the register rows and N = R + Hp*Wp token rows per image of width C.  Integer arithmetic
    only, so the shapes may be Dynamo's symbolic ints (the custom ops' fakes)."""
    B, _, Hi, Wi = image_shape
    p = model.conv_init.patch_size
    Hp, Wp = Hi // p, Wi // p
    R = reg_rows(model, num_registers)
    return B, R, Hp, Wp, R + Hp * Wp, model.conv_init.conv.out_channels


def hooked(module: nn.Module) -> bool:
    """True if any submodule has forward (pre-)hooks: the caller then composes
    the forward module by module so every hooked __call__ fires."""
    for m in module.modules():
        if m is module:
            continue
        if m._forward_hooks or m._forward_pre_hooks:
            return True
    return False


class GraphedForward:
    """One eval forward of ``model`` captured into a HIP graph and replayed per call: the forward's
    several hundred launches become one, which is most of the latency at small batch.

    ``GraphedForward(model, example, num_registers=3)`` warms up (which builds the prepared-weight
    caches) and captures ``model(example, num_registers)`` into a static input and static logits.
    ``gf(x)`` copies ``x`` into the static input, replays and returns the static logits: the SAME
    tensor every call, overwritten by the next call (clone it to keep it).  ``x`` must have the
    example's shape, dtype and device.

    A replay never computes with stale prepared weights: every call compares the version key
    ``cached`` uses (version counter and address of every parameter) and the count of
    ``invalidate`` / ``load_state_dict`` calls with those of the capture, and captures again when
    either changed, or when the model's low_latency or mx_fp8 setting did.  Whatever ``model(x)`` would run
    eagerly is what is captured (streams, low_latency, mx_fp8, final_rows ...); no environment variable
    and no queue setting is touched."""

    def __init__(self, model: nn.Module, example: torch.Tensor, num_registers: int = 3):
        if model.training:
            raise RuntimeError("GraphedForward captures the eval forward: call model.eval() first")
        if not example.is_cuda:
            raise RuntimeError("GraphedForward needs a CUDA (ROCm) example input")
        self.model = model
        self.num_registers = num_registers
        self._x = example.detach().clone(memory_format=torch.contiguous_format)
        self._graph = None
        self._y = None
        self._state = None
        self.captures = 0
        self._capture()

    def _current_state(self):
        ll = getattr(self.model, "_low_latency_on", None)
        mx = getattr(self.model, "_mx_fp8_on", None)
        return (_key(list(self.model.parameters()), self._x.dtype, self._x.device), _INVALIDATIONS,
                ll() if ll is not None else sp.low_latency_enabled(),
                mx() if mx is not None else sp.mx_fp8_enabled())

    def _capture(self):
        dev = self._x.device
        self._graph = self._y = None  # the old graph's pool goes before the new one is built
        with torch.no_grad(), torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(cur)
            with torch.cuda.stream(side):  # warm-up off the capture: weight caches, stream pool, allocator
                for _ in range(2):
                    self.model(self._x, self.num_registers)
            cur.wait_stream(side)
            state = self._current_state()  # after the warm-up: building a cache must not look like a change
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                y = self.model(self._x, self.num_registers)
        self._graph, self._y, self._state = graph, y, state
        self.captures += 1

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if x.shape != self._x.shape or x.dtype != self._x.dtype or x.device != self._x.device:
            raise ValueError(f"GraphedForward was captured for {tuple(self._x.shape)} {self._x.dtype} on "
                             f"{self._x.device}, got {tuple(x.shape)} {x.dtype} on {x.device}")
        if self.model.training:
            raise RuntimeError("GraphedForward replays the eval forward; the model is in train mode")
        self._x.copy_(x)
        if self._current_state() != self._state:
            self._capture()
        self._graph.replay()
        return self._y


# ---------------------------------------------------------------------------
# Moving a checkpoint to another patch grid.  The reference defines no resampling of its position
# parameters, so this project does: on the CPU in fp64, rounded once to fp32 (then to the stored
# dtype).  A size that does not change returns the stored tensor itself.
_DDP_PREFIXES = ("module.", "_orig_mod.")


def _resample_table(w: torch.Tensor, n_new: int) -> torch.Tensor:
    """[n_old, C] -> [n_new, C] along its length: linear, half-pixel centres, edges clamped."""
    if w.shape[0] == n_new:
        return w
    r = F.interpolate(w.detach().cpu().double().t()[None], size=n_new, mode="linear", align_corners=False)
    return r[0].t().contiguous().float().to(dtype=w.dtype, device=w.device)


def _resample_bone(b: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """[1, C, H0 + k, W0 + k] -> [1, C, H1 + k, W1 + k]: bicubic, half-pixel centres."""
    if tuple(b.shape[-2:]) == tuple(size):
        return b
    r = F.interpolate(b.detach().cpu().double(), size=tuple(size), mode="bicubic", align_corners=False)
    return r.float().to(dtype=b.dtype, device=b.device)


def resize_positions(state_dict: Dict[str, torch.Tensor], config: dict, max_image_size, *, prefix: str = ""):
    """(state_dict, config) of the same MainModel at another ``max_image_size``.

    EmbeddingLayer: each of the two tables is resampled along its own length to its own new length
    (``vertical_*`` is sized by ``max_image_size[0]``, ``horizontal_*``, the one indexed by rows,
    by ``max_image_size[1]``, as the model has them) and the two ``arange`` buffers are rebuilt.
    ConvEmbedding: ``bone`` goes to ``[1, C, H1 + k, W1 + k]`` with k the config's
    ``conv_embedding_kernel_size``.  Every other tensor, the register table and buffers among
    them, is passed through as the same object.  DDP / torch.compile key prefixes (``module.``,
    ``_orig_mod.``) are stripped, as eval_harness.preprocess_weights strips them; ``prefix`` names
    where the model sits inside a larger dict (``"student."``) and is kept.  The result loads with
    ``strict=True`` into ``MainModel.from_dict(**config)``."""
    new = [int(max_image_size[0]), int(max_image_size[1])]
    if new[0] <= 0 or new[1] <= 0:
        raise ValueError(f"resize_positions: max_image_size {list(max_image_size)} must be positive")
    k = int(config.get("conv_embedding_kernel_size", 5))
    emb = prefix + "embedding_layer."
    sized = {emb + "vertical_embedding_layer.weight": 0, emb + "horizontal_embedding_layer.weight": 1,
             emb + "vertical_embedding": 0, emb + "horizontal_embedding": 1}
    out, seen = {}, 0
    for key, t in state_dict.items():
        while key.startswith(_DDP_PREFIXES):
            key = key[len(next(p for p in _DDP_PREFIXES if key.startswith(p))):]
        if key in sized:
            n = new[sized[key]]
            if key.endswith(".weight"):
                t = _resample_table(t, n)
            elif t.shape[0] != n:
                t = torch.arange(n, dtype=t.dtype, device=t.device)
            seen += 1
        elif key == emb + "bone":
            t = _resample_bone(t, (new[0] + k, new[1] + k))
            seen += 1
        out[key] = t
    if seen == 0:
        raise KeyError(f"resize_positions: no position tensors under {emb!r}")
    cfg = dict(config)
    cfg["max_image_size"] = new
    return out, cfg


def with_max_image_size(model: nn.Module, max_image_size) -> nn.Module:
    """A new MainModel at ``max_image_size`` holding ``model``'s weights with its position
    parameters resampled (resize_positions); same device, parameter dtype and train/eval mode."""
    from model import MainModel
    state, cfg = resize_positions(model.state_dict(), model.config, max_image_size)
    new = MainModel.from_dict(**cfg)
    p = next(model.parameters())
    new = new.to(device=p.device, dtype=p.dtype)
    new.load_state_dict(state, strict=True)
    new.train(model.training)
    return new
