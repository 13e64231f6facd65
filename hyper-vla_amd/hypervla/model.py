"""``hypervla.model.HyperVLA`` — the reference's model API (hypervla/model.py:24-224) hosted on
libhvla.  Same surface, MI355X-native inside:

    model = HyperVLA.load_pretrained(path, step=None)      # model.py:139-224
    model = model.replace(params=ema_params)                # flax struct.dataclass .replace
    base_params, tasks, _ = model.create_tasks(instruction_dict=..., initial_state=...)   # :35-83
    actions, _ = model.sample_actions(images, instruction_dict, tasks, pad_mask, base_params, rng=key)  # :85-137

Differences a caller can observe, all by design:
  * ``create_tasks`` accepts B >= 1 episodes (the reference squeezes B == 1, model.py:81) and returns
    an opaque :class:`GeneratedWeights` handle that owns the device arena; ``.to_pytree()`` gives the
    reference's ``base_params`` pytree back.
  * of the per-step intermediates (every attention map, base_vit.py:117-118) the two slices a caller of the path reads
    (data/utils/hypervla_interface.py:208-217) are materialised on request: ``sample_actions(..., attention_maps=True)``
    adds ``"dino_cls_attention"`` [B, 12, 12, P] and ``"head_attention"`` [B, 4, 4, P] to its second value, which
    otherwise is ``{"gripper_logits": ...}``.
  * arrays may be numpy (copied to the device) or torch CUDA tensors (used in place); results come
    back in the same kind.

There is no CPU / eager fallback: constructing a model without a gfx950 device and a built
``libhvla.so`` raises.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, Optional

import numpy as np

from . import _native
from .config import (FULL, Geometry, default_config, generated_leaves, geometry_from_config,
                     hypernet_param_shapes, pytree_from_theta, theta_from_pytree)


def _torch():
    import torch
    return torch


class GeneratedWeights:
    """Handle to one batch of generated policy weights on the device (what the reference calls
    ``base_params``); freed on garbage collection.  What `create_tasks` returns is immutable from the caller's side.  An
    episode pool is mutable in place: `HyperVLA.assign_tasks` regenerates slots of a handle from `create_pool` (or from
    `create_tasks`) and leaves its other rows as they are; `batch` is then the pool's capacity."""

    def __init__(self, model: "HyperVLA", handle, batch: int, tokens=None):
        self._model, self._h, self.batch = model, handle, batch
        # use_language_token: the token embeddings [batch, T, lang_dim] the rows' language prefixes were built from (a device tensor
        # of the handle's own; None without the option) -- the prefix is not part of theta, so `save` needs them
        self._tokens = tokens

    def __del__(self):
        try:
            if self._h is not None:
                self._model._ctx.weights_free(self._h)
                self._h = None
        except Exception:
            pass

    def export(self):
        """(theta [B, G] in reference leaf order, context embedding [B, C]) as torch CUDA tensors; with share_layer_index=False
        (`Geometry.layer_tokens`) the context embedding is [B, NL, C], one row per layer token."""
        torch = _torch()
        m = self._model
        dev = m.device
        theta = torch.empty(self.batch, m._ctx.num_generated, dtype=torch.float32, device=dev)
        ctx = torch.empty((self.batch,) + m._context_shape(), dtype=torch.float32, device=dev)
        m._ctx.weights_export(self._h, theta.data_ptr(), ctx.data_ptr(), m._stream())
        return theta, ctx

    def to_pytree(self, squeeze: bool = False) -> Dict[str, Any]:
        """The reference's nested ``base_params`` dict (generated leaves only; the shared DINOv2 leaves
        live once on the device and are not broadcast, hypernetwork.py:233)."""
        return pytree_from_theta(self._model.geometry, self.export()[0].cpu().numpy(), squeeze)

    def save(self, path: str) -> None:
        """Write the handle's policies to `path` as an npz: ``theta`` [B, G] and ``context`` [B, C] ([B, NL, C] with layer tokens) as `export` returns them and the
        geometry's ``G``; with use_language_token also the ``token_embedding`` [B, T, lang_dim] the rows were built from.
        `HyperVLA.load_tasks` reads it back (through `import_tasks`: the same theta and context bit for bit)."""
        m = self._model
        theta, ctx = self.export()
        arrays = {"theta": theta.cpu().numpy(), "context": ctx.cpu().numpy(), "G": np.int64(m._ctx.num_generated)}
        if m.geometry.lang_in_policy:
            arrays["token_embedding"] = self._tokens.cpu().numpy()
        with open(path, "wb") as f:
            np.savez(f, **arrays)


class HyperVLA:
    def __init__(self, config: Dict, params: Dict[str, np.ndarray], example_batch: Optional[Dict] = None,
                 dataset_statistics: Optional[Dict] = None, device: int = 0, max_batch: int = 256,
                 enc_dtype: str = "f16", streams: int = 1, _shared_ctx=None, *, position_table_source=None):
        torch = _torch()
        self.config = config
        self.params = params
        # the un-resized DINOv2 position table of a converted checkpoint (float32 [1, 1 + n*n, E]; hypervla/convert.py): not a
        # parameter of the serving path, which reads the baked table in `params`, but the leaf FineTuner(train_encoder=True) trains
        self.position_table_source = position_table_source
        self.example_batch = example_batch
        self.dataset_statistics = dataset_statistics
        self.geometry: Geometry = geometry_from_config(config)
        self.base_net_metadata = {"leaves": generated_leaves(self.geometry)}
        if not torch.cuda.is_available():
            raise RuntimeError("HyperVLA needs an MI355X (gfx950) device: torch.cuda.is_available() is False "
                               "and there is no CPU fallback")
        self.device = torch.device("cuda", device)
        self.max_batch, self.enc_dtype, self.streams = max_batch, enc_dtype, streams
        self._ctx = _native.Context(self.geometry, device, max_batch, enc_dtype, streams)
        want = hypernet_param_shapes(self.geometry)
        missing = [k for k in want if k not in params]
        if missing:
            raise ValueError(f"checkpoint is missing {len(missing)} tensors, e.g. {missing[:3]}")
        self._ctx.load_weights({k: params[k] for k in want})

    @property
    def position_table_source(self) -> Optional[np.ndarray]:
        return self._position_table_source

    @position_table_source.setter
    def position_table_source(self, value) -> None:
        if value is not None:
            value = np.ascontiguousarray(np.asarray(value, np.float32))
            E = geometry_from_config(self.config).enc_dim
            n = int(round(np.sqrt(max(value.shape[1] - 1, 0)))) if value.ndim == 3 else 0
            if value.ndim != 3 or value.shape[0] != 1 or value.shape[2] != E or n < 2 or 1 + n * n != value.shape[1]:
                raise ValueError(f"position_table_source must be float32 [1, 1 + n*n, {E}], got {value.shape}")
        self._position_table_source = value

    @property
    def params(self) -> Dict[str, np.ndarray]:
        """The host tensors of the weights being served.  After `FineTuner.publish(host_copy=False)` the device serves weights
        the host has no copy of: reading them (and `save_pretrained`) raises until a `publish(host_copy=True)`."""
        if self._params_stale:
            raise RuntimeError("the device serves weights published without a host copy (FineTuner.publish(host_copy=False)): "
                               "model.params would be stale; call publish(host_copy=True) first")
        return self._params

    @params.setter
    def params(self, value: Dict[str, np.ndarray]) -> None:
        self._params, self._params_stale = value, False

    def release_pooled_arenas(self) -> None:
        """Free the generated-weight arenas that freed `GeneratedWeights` parked for re-use (hvla_release_pooled_arenas:
        up to four per context, about 0.8 MB per episode each).  `create_tasks` allocates again when it next needs one."""
        self._ctx.release_pooled_arenas()

    # ------------------------------------------------------------------ construction
    @classmethod
    def load_pretrained(cls, checkpoint_path: str, step: Optional[int] = None, audit="raise", **kw) -> "HyperVLA":
        """Reads ``config.json``, ``example_batch.msgpack`` (flax msgpack, read without flax: hypervla/convert.py),
        ``dataset_statistics.json`` and the parameter file written by :meth:`save_pretrained` (``params_<step>.npz`` /
        ``params.npz``; flat '/'-joined flax names) -- the files of hypervla/model.py:152-214 except that
        the parameters are an npz instead of an Orbax step directory (exporter-only: INTEGRATION.md).

        `audit`: what the operand-range audit of the checkpoint's example batch does when activations leave the 16-bit operand
        type's range -- "raise" (default: refuse the checkpoint), "warn" (load it and warn; `model.operand_range` has the
        numbers) or False / "off" (no audit: no encoder pass at load time).  When the checkpoint has no example batch the audit
        cannot run; that is reported with a warning instead of passing silently."""
        if audit not in ("raise", "warn", "off", False, None):
            raise ValueError(f"audit must be 'raise', 'warn' or 'off', got {audit!r}")
        with open(os.path.join(checkpoint_path, "config.json")) as f:
            config = json.load(f)
        if "action_head_kwargs" not in config["base_net_kwargs"]:        # model.py:157-163
            config["base_net_kwargs"]["action_head_kwargs"] = dict(
                token_per_horizon=False, squash_continuous_action=True, clip_target=False, max_action=5.0)
        stats = None
        sp = os.path.join(checkpoint_path, "dataset_statistics.json")
        if os.path.exists(sp):
            with open(sp) as f:
                stats = _tree_map(np.array, json.load(f))
        cands = sorted(p for p in os.listdir(checkpoint_path) if p.startswith("params") and p.endswith(".npz"))
        if step is not None:
            cands = [p for p in cands if p == f"params_{step}.npz"]
        if not cands:
            raise FileNotFoundError(f"no params*.npz under {checkpoint_path} (step={step})")
        from .convert import load_example_batch
        params, source = read_params_file(os.path.join(checkpoint_path, cands[-1]))
        model = cls(config, params, load_example_batch(checkpoint_path), stats, position_table_source=source, **kw)
        if audit in ("raise", "warn"):         # a real checkpoint's activations must fit the 16-bit operand type
            import warnings
            try:
                if model.audit_operand_range() is None:
                    warnings.warn("operand-range audit skipped: the checkpoint has no example batch with image_primary frames; "
                                  "call model.audit_operand_range(images) on real observations", RuntimeWarning)
            except ValueError as e:             # operands out of range, or example frames the resize refuses: under 'warn' neither blocks the
                                                # load; a native / HIP failure of the audit itself is never downgraded
                if audit == "raise":
                    raise
                warnings.warn(f"{e} (audit='warn': loaded anyway)", RuntimeWarning)
        return model

    FP16_OPERAND_LIMIT = 32768.0               # half of fp16's largest finite value (65504)

    def audit_operand_range(self, images=None):
        """Run the image encoder once with a range audit of every 16-bit MFMA operand it writes (LayerNorm outputs, q / k /
        v, attention outputs, GELU outputs, all layers: `hvla_encode_audit`) and refuse a checkpoint whose activations leave
        the operand type's range: a trained DINOv2 carries outlier channels that the synthetic weights do not (DESIGN.md
        section 2).  `images` defaults to the checkpoint's example batch; returns {site: largest |operand|}, or None when
        there is nothing to audit on."""
        torch = _torch()
        if images is None:
            try:
                images = np.asarray(self.example_batch["observation"]["image_primary"])
            except (TypeError, KeyError):
                return None
        images = images[: self.max_batch]       # (sliced first, as it is -- ndarray or tensor, on any device: an example batch of many large frames is neither moved nor resized in full)
        img = self._dev(images, torch.uint8)
        if img.dim() == 5:
            img = img[:, 0].contiguous()
        g = self.geometry
        if tuple(img.shape[1:]) != (g.image_size, g.image_size, 3):
            try:
                img = self.preprocess_images(img)  # example frames of another size: the evaluators' resize (InferenceWrapper._resize_image)
            except _native.NativeError as e:       # frames the resize refuses are a property of the example batch (ValueError), not a device failure
                raise ValueError(f"the example frames {tuple(img.shape)} cannot be resized for the audit: {e}") from e
        img = img.contiguous()
        audit = self._ctx.encode_audit(img.data_ptr(), img.shape[0], self._stream())      # {site: (max |x|, non-finite count)}
        sites = {k: v[0] for k, v in audit.items()}
        bad = {k: v[1] for k, v in audit.items() if v[1]}
        limit = self.FP16_OPERAND_LIMIT if self.enc_dtype == "f16" else 3.0e38
        if bad or max(sites.values()) > limit:
            raise ValueError(f"encoder activations leave the {self.enc_dtype} operand range on the example batch: largest "
                             f"|operand| per site {sites}, non-finite values {bad}; load with enc_dtype='bf16' "
                             "(8 exponent bits) instead")
        self.operand_range = sites
        return sites

    def save_pretrained(self, step: int, checkpoint_path: str):
        os.makedirs(checkpoint_path, exist_ok=True)
        from .convert import POSITION_SOURCE_KEY
        src = self.position_table_source
        np.savez(os.path.join(checkpoint_path, f"params_{step}.npz"), **self.params,
                 **({POSITION_SOURCE_KEY: src} if src is not None else {}))
        cp = os.path.join(checkpoint_path, "config.json")
        if not os.path.exists(cp):
            with open(cp, "w") as f:
                json.dump(self.config, f)
        sp = os.path.join(checkpoint_path, "dataset_statistics.json")
        if self.dataset_statistics is not None and not os.path.exists(sp):
            with open(sp, "w") as f:
                json.dump(_tree_map(lambda x: np.asarray(x).tolist(), self.dataset_statistics), f)
        ep = os.path.join(checkpoint_path, "example_batch.msgpack")          # hypervla/model.py:270-274
        if self.example_batch is not None and not os.path.exists(ep):
            from .convert import msgpack_serialize
            with open(ep, "wb") as f:
                f.write(msgpack_serialize(self.example_batch))

    @classmethod
    def from_synthetic(cls, geometry: Geometry = FULL, params: Optional[Dict[str, np.ndarray]] = None, *,
                       position_table_source=None, **kw) -> "HyperVLA":
        """`position_table_source` (e.g. `synthetic.synthetic_position_table_hub(g, n)`): the model is what the converter makes of a
        checkpoint with that table -- the served table is its baking, the config carries the marker, the source rides along."""
        from . import synthetic
        config = default_config(geometry)
        params = synthetic.synthetic_params(geometry) if params is None else params
        if position_table_source is not None:
            from .convert import bake_position_embeddings
            src = np.asarray(position_table_source, np.float32)
            n = int(round(np.sqrt(src.shape[1] - 1)))
            params = dict(params)
            key = next(k for k in params if k.endswith("embeddings_position_embeddings"))
            params[key] = bake_position_embeddings(src, geometry.image_size // geometry.patch).reshape(params[key].shape)
            config["position_embeddings_baked_from"] = [n, n]
        return cls(config, params, None, synthetic.synthetic_dataset_statistics(geometry),
                   position_table_source=position_table_source, **kw)

    def replace(self, **changes) -> "HyperVLA":
        """flax ``struct.dataclass.replace``: the evaluators swap in EMA params this way
        (data/simpler/evaluate.py:440-444)."""
        if set(changes) - {"params", "config", "dataset_statistics", "example_batch", "position_table_source"}:
            raise TypeError(f"cannot replace {set(changes)}")
        if "params" in changes or "config" in changes:
            # the source table goes along while it still is the source of the served table: parameters that bring another
            # position table leave it behind unless theirs is passed too
            source = changes.get("position_table_source", self.position_table_source)
            if "position_table_source" not in changes and source is not None and "params" in changes:
                key = next(k for k in self.params if k.endswith("embeddings_position_embeddings"))
                if key not in changes["params"] or not np.array_equal(np.asarray(changes["params"][key]).reshape(-1),
                                                                     np.asarray(self.params[key]).reshape(-1)):
                    source = None
            return HyperVLA(changes.get("config", self.config), changes.get("params", self.params),
                            changes.get("example_batch", self.example_batch),
                            changes.get("dataset_statistics", self.dataset_statistics),
                            self.device.index or 0, self.max_batch, self.enc_dtype, self.streams,
                            position_table_source=source)
        import copy
        other = copy.copy(self)
        for k, v in changes.items():
            setattr(other, k, v)
        return other

    # ------------------------------------------------------------------ helpers
    def _context_shape(self):
        """The shape of one episode's context embedding: (C,), or (NL, C) with share_layer_index=False."""
        g = self.geometry
        return (g.num_layer_tokens, g.ctx_dim) if g.layer_tokens else (g.ctx_dim,)

    def _stream(self) -> int:
        return int(_torch().cuda.current_stream(self.device).cuda_stream)

    def _dev(self, a, dtype):
        torch = _torch()
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(np.asarray(a))).to(device=self.device, dtype=dtype).contiguous()

    # ------------------------------------------------------------------ observation preprocessing
    def preprocess_images(self, frames, crop: bool = False, padded_resize: bool = False):
        """`InferenceWrapper._resize_image` (data/utils/hypervla_interface.py:89-121) on the device: uint8 camera frames
        [B, H, W, 3] (or [H, W, 3]) -> uint8 [B, image_size, image_size, 3] CUDA tensor.  `padded_resize` first fits the
        frame into 256 x 320 with zero padding (`tf.image.resize_with_pad`, the "rtx" augmentation style)."""
        torch = _torch()
        f = self._dev(frames, torch.uint8)
        if f.dim() == 3:
            f = f[None].contiguous()
        if f.dim() != 4 or f.shape[-1] != 3:
            raise ValueError(f"frames must be [B, H, W, 3] uint8, got {tuple(f.shape)}")
        B, H, W, _ = f.shape
        S = self.geometry.image_size
        out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=self.device)
        self._ctx.preprocess(f.data_ptr(), B, H, W, crop, out.data_ptr(), self._stream(), padded_resize)
        return out

    # ------------------------------------------------------------------ frozen instruction encoder (optional)
    def load_language_encoder(self, t5_params: Dict[str, np.ndarray], t5_geometry=None, max_batch: Optional[int] = None):
        """Put the frozen T5 encoder of `LanguageTokenizer('t5-base')` on the device
        (data/utils/language_tokenizer.py:9-28).  `t5_params`: FlaxT5EncoderModel tree flattened with '/'."""
        from .config import T5_BASE
        t = T5_BASE if t5_geometry is None else t5_geometry
        if t.d_model != self.geometry.lang_dim:
            raise ValueError(f"T5 d_model {t.d_model} != lang_dim {self.geometry.lang_dim}")
        self._ctx.t5_load(t, t5_params, self.geometry.lang_tokens, max_batch or self.max_batch)
        self.language_encoder = t
        return self

    def encode_instructions(self, tokens: Dict) -> Dict:
        """`token_to_embedding` (data/utils/language_tokenizer.py:24-28) on the device: {"input_ids", "attention_mask"}
        i64 [B, T] -> the same dict plus "token_embedding" f32 [B, T, lang_dim] (a CUDA tensor)."""
        torch = _torch()
        if getattr(self, "language_encoder", None) is None:
            raise RuntimeError("no language encoder loaded: call load_language_encoder(t5_params) first")
        ids = self._dev(tokens["input_ids"], torch.int64)
        mask = self._dev(tokens["attention_mask"], torch.int64)
        if ids.dim() != 2 or ids.shape != mask.shape:
            raise ValueError(f"input_ids {tuple(ids.shape)} / attention_mask {tuple(mask.shape)} must be [B, T]")
        B, T = ids.shape
        emb = torch.empty(B, T, self.geometry.lang_dim, dtype=torch.float32, device=self.device)
        self._ctx.t5_encode(ids.data_ptr(), mask.data_ptr(), emb.data_ptr(), B, T, self._stream())
        out = dict(tokens)
        out["token_embedding"] = emb
        return out

    # ------------------------------------------------------------------ the hot path
    def _task_inputs(self, instruction_dict: Dict, initial_state: Dict):
        """(language_instruction dict, B, token_embedding, attention_mask, CLS rows) on the device, shapes checked."""
        torch = _torch()
        if instruction_dict is None or initial_state is None:
            raise ValueError("the built path is language + initial-image conditioned: instruction_dict and "
                             "initial_state are required (use_initial_image=True, README.md:42)")
        li = instruction_dict["language_instruction"]
        if "token_embedding" not in li and getattr(self, "language_encoder", None) is not None:
            li = self.encode_instructions(li)                      # scripts/train.py:407-415 does this inside the step
        g = self.geometry
        B = int(np.shape(li["input_ids"])[0])
        tok = self._dev(li["token_embedding"], torch.float32)
        mask = self._dev(li["attention_mask"], torch.int64)
        pe = initial_state["patch_embeddings"]
        cls = self._dev(pe[:, 0] if not isinstance(pe, torch.Tensor) else pe[:, 0], torch.float32)
        if tuple(tok.shape) != (B, g.lang_tokens, g.lang_dim) or tuple(mask.shape) != (B, g.lang_tokens) \
                or tuple(cls.shape) != (B, g.enc_dim):
            raise ValueError(f"bad shapes: token_embedding {tuple(tok.shape)}, attention_mask {tuple(mask.shape)}, "
                             f"patch_embeddings[:,0] {tuple(cls.shape)} for B={B}")
        return li, B, tok, mask, cls

    def create_tasks(self, goals=None, instruction_dict: Dict = None, initial_state: Dict = None):
        """hypervla/model.py:35-83.  Returns (base_params handle, tasks dict, intermediates)."""
        torch = _torch()
        li, B, tok, mask, cls = self._task_inputs(instruction_dict, initial_state)
        h = self._ctx.generate(tok.data_ptr(), mask.data_ptr(), cls.data_ptr(), B, self._stream())
        torch.cuda.current_stream(self.device).synchronize()      # inputs may be temporaries
        tasks = {"pad_mask_dict": {"language_instruction": np.ones(B, dtype=bool)},     # model.py:51-70
                 "language_instruction": li}
        return GeneratedWeights(self, h, B, tok.clone() if self.geometry.lang_in_policy else None), tasks, {}

    # ------------------------------------------------------------------ episode pool
    def create_pool(self, capacity: int) -> GeneratedWeights:
        """An episode pool of `capacity` empty slots (`hvla_weights_alloc`): zero weights, which step to finite actions, and
        fresh ensemble counters.  Fill slots with :meth:`assign_tasks`; step any subset with ``sample_actions(..., slots=)``."""
        capacity = int(capacity)
        if not 1 <= capacity <= self.max_batch:
            raise ValueError(f"pool capacity {capacity} outside [1, max_batch={self.max_batch}]")
        h = self._ctx.weights_alloc(capacity, self._stream())
        return GeneratedWeights(self, h, capacity, self._empty_tokens(capacity))

    def _empty_tokens(self, rows: int):
        g = self.geometry
        if not g.lang_in_policy:
            return None
        return _torch().zeros(rows, g.lang_tokens, g.lang_dim, dtype=_torch().float32, device=self.device)

    def _slot_map(self, slots, pool: GeneratedWeights):
        """`slots` checked on the host (hypervla.pool.check_slots), then as a device int32 tensor."""
        from .pool import check_slots
        s = check_slots(slots, pool.batch)
        if len(s) > self.max_batch:
            raise ValueError(f"{len(s)} slots in one call: more than max_batch={self.max_batch}")
        return s, _torch().as_tensor(s).to(self.device)

    def assign_tasks(self, pool: GeneratedWeights, slots, instruction_dict: Dict = None, initial_state: Dict = None):
        """`create_tasks` for K new episodes into slots `slots` of `pool` (`hvla_generate_slots`): the same inputs for K episodes
        (bare `input_ids` / `attention_mask` are encoded by a loaded T5 first).  Those slots' weights, context and ensemble
        counter are replaced -- bitwise what `create_tasks` gives the same tasks -- and every other slot is left as it was.
        Returns the tasks dict of the K episodes."""
        torch = _torch()
        if not isinstance(pool, GeneratedWeights) or pool._model is not self:
            raise TypeError("pool must be a handle of this model (create_pool / create_tasks)")
        s, sd = self._slot_map(slots, pool)
        li, K, tok, mask, cls = self._task_inputs(instruction_dict, initial_state)
        if K != len(s):
            raise ValueError(f"{K} tasks for {len(s)} slots")
        self._ctx.generate_slots(pool._h, sd.data_ptr(), K, tok.data_ptr(), mask.data_ptr(), cls.data_ptr(), self._stream())
        if pool._tokens is not None:
            pool._tokens[sd.long()] = tok
        torch.cuda.current_stream(self.device).synchronize()      # inputs may be temporaries
        return {"pad_mask_dict": {"language_instruction": np.ones(K, dtype=bool)}, "language_instruction": li}

    # ------------------------------------------------------------------ policies as values
    def _theta_arg(self, base_params):
        """`base_params` as a device f32 [B, G] tensor: the reference's nested dict, a numpy [B, G], or a torch tensor already on the
        model's device, which is used in place."""
        torch = _torch()
        G = self._ctx.num_generated
        if isinstance(base_params, GeneratedWeights):
            raise TypeError("base_params is already a device handle: step it as it is, or copy_tasks() it")
        if isinstance(base_params, dict):
            base_params = theta_from_pytree(self.geometry, base_params)
        if isinstance(base_params, torch.Tensor):
            if base_params.device != self.device:
                raise ValueError(f"a theta tensor must be on the model's device {self.device}, got {base_params.device}")
            theta = base_params
        else:
            theta = torch.as_tensor(np.ascontiguousarray(np.asarray(base_params), dtype=np.float32)).to(self.device)
        if theta.dim() != 2 or theta.shape[1] != G or theta.shape[0] < 1:
            raise ValueError(f"theta must be [B, {G}], got {tuple(theta.shape)}")
        if theta.dtype != torch.float32 or not theta.is_contiguous():
            theta = theta.to(torch.float32).contiguous()
        return theta

    def _import_inputs(self, base_params, instruction_dict, context):
        """(theta [B, G], context [B, C] or None, token embeddings [B, T, lang_dim] or None) on the device, shapes checked."""
        torch = _torch()
        g = self.geometry
        theta = self._theta_arg(base_params)
        B = theta.shape[0]
        ctx = None
        if context is not None:
            ctx = self._dev(context, torch.float32)
            if tuple(ctx.shape) != (B,) + self._context_shape():
                raise ValueError(f"context must be {[B, *self._context_shape()]}, got {tuple(ctx.shape)}")
        tok = None
        if g.lang_in_policy:                      # the only thing instruction_dict is read for
            if instruction_dict is None:
                raise ValueError("a use_language_token model imports a policy together with the episodes' instruction tokens: "
                                 "instruction_dict is required (its token embeddings become the rows' language prefix)")
            li = instruction_dict["language_instruction"]
            if "token_embedding" not in li and getattr(self, "language_encoder", None) is not None:
                li = self.encode_instructions(li)
            tok = self._dev(li["token_embedding"], torch.float32)
            if tuple(tok.shape) != (B, g.lang_tokens, g.lang_dim):
                raise ValueError(f"token_embedding must be [{B}, {g.lang_tokens}, {g.lang_dim}], got {tuple(tok.shape)}")
        return theta, ctx, tok

    def import_tasks(self, base_params, instruction_dict: Dict = None, context=None) -> GeneratedWeights:
        """A handle for policies that `create_tasks` did not return (`hvla_weights_import`): `base_params` is the reference's nested
        dict (leaves [B, *shape], or [*shape] for one episode), a numpy [B, G] in reference leaf order, or a torch tensor of that
        shape on the model's device (used in place).  `context` [B, C] rides along for `export` (default zeros; the policy does not
        read it).  `instruction_dict` is read only by a use_language_token model, for the token embeddings (bare `input_ids` are
        encoded by a loaded T5 first).  `export()` of the result returns the vector leaves bit for bit and every matrix element as
        the sum of its two bf16 halves; an exported theta comes back unchanged."""
        theta, ctx, tok = self._import_inputs(base_params, instruction_dict, context)
        B = theta.shape[0]
        if B > self.max_batch:
            raise ValueError(f"{B} episodes: more than max_batch={self.max_batch}")
        h = self._ctx.weights_import(theta.data_ptr(), ctx.data_ptr() if ctx is not None else 0,
                                     tok.data_ptr() if tok is not None else 0, B, self._stream())
        _torch().cuda.current_stream(self.device).synchronize()   # inputs may be temporaries
        return GeneratedWeights(self, h, B, tok.clone() if tok is not None else None)

    def assign_base_params(self, pool: GeneratedWeights, slots, base_params, instruction_dict: Dict = None, context=None) -> None:
        """`import_tasks` for K policies into slots `slots` of `pool` (`hvla_weights_import_slots`): those slots' weights, context
        and ensemble counter are replaced -- a slot then steps bitwise as the same row imported alone -- and every other slot is
        left as it was."""
        if not isinstance(pool, GeneratedWeights) or pool._model is not self:
            raise TypeError("pool must be a handle of this model (create_pool / create_tasks / import_tasks)")
        s, sd = self._slot_map(slots, pool)
        theta, ctx, tok = self._import_inputs(base_params, instruction_dict, context)
        if theta.shape[0] != len(s):
            raise ValueError(f"{theta.shape[0]} policies for {len(s)} slots")
        self._ctx.weights_import_slots(pool._h, sd.data_ptr(), len(s), theta.data_ptr(), ctx.data_ptr() if ctx is not None else 0,
                                       tok.data_ptr() if tok is not None else 0, self._stream())
        if pool._tokens is not None:
            pool._tokens[sd.long()] = tok
        _torch().cuda.current_stream(self.device).synchronize()   # inputs may be temporaries

    def copy_tasks(self, dst: GeneratedWeights, dst_slots, src: GeneratedWeights, src_slots=None) -> None:
        """Rows `src_slots` (None: 0 .. K-1) of `src` into slots `dst_slots` of `dst` (`hvla_weights_copy_slots`): weights, language
        prefix and context byte for byte -- the copy steps bitwise as its source -- and the destination slots' ensemble counters
        restarted.  Within one handle the two maps must not share a slot (ValueError)."""
        from .pool import check_slots
        for h in (dst, src):
            if not isinstance(h, GeneratedWeights) or h._model is not self:
                raise TypeError("dst and src must be handles of this model")
        d = check_slots(dst_slots, dst.batch)
        s = check_slots(np.arange(len(d)) if src_slots is None else src_slots, src.batch)
        if len(s) != len(d):
            raise ValueError(f"{len(s)} source slots for {len(d)} destination slots")
        if dst is src and set(d.tolist()) & set(s.tolist()):
            raise ValueError(f"copy within one handle with overlapping maps: slots {sorted(set(d.tolist()) & set(s.tolist()))} are "
                             "both read and written")
        torch = _torch()
        dd, sd = torch.as_tensor(d).to(self.device), torch.as_tensor(s).to(self.device)
        self._ctx.weights_copy_slots(dst._h, dd.data_ptr(), src._h, sd.data_ptr(), len(d), self._stream())
        if dst._tokens is not None:
            dst._tokens[dd.long()] = src._tokens[sd.long()]
        torch.cuda.current_stream(self.device).synchronize()      # the maps are temporaries

    def load_tasks(self, path: str) -> GeneratedWeights:
        """The handle `GeneratedWeights.save(path)` wrote, through `import_tasks`; a file of another geometry's G, or whose context
        rows are not this model's ([C], or [NL, C] with layer tokens), is refused."""
        with np.load(path) as z:
            G = int(z["G"])
            if G != self._ctx.num_generated:
                raise ValueError(f"{path} holds policies of G={G} generated parameters, this model's geometry has "
                                 f"G={self._ctx.num_generated}")
            theta, context = z["theta"], z["context"]
            if tuple(context.shape[1:]) != self._context_shape():
                raise ValueError(f"{path} holds context rows of shape {tuple(context.shape[1:])}, this model's are "
                                 f"{self._context_shape()}")
            tok = z["token_embedding"] if "token_embedding" in z.files else None
        ins = None
        if self.geometry.lang_in_policy:
            if tok is None:
                raise ValueError(f"{path} was saved without token embeddings: a use_language_token model cannot build its rows' "
                                 "language prefix from it")
            ins = {"language_instruction": {"token_embedding": tok}}
        return self.import_tasks(theta, ins, context)

    def ensemble_actions(self, pool: GeneratedWeights, actions, stats, slots):
        """Un-normalise + temporal ensemble per slot on the device (`hvla_ensemble_slots`): actions [K, horizon, action_dim] of
        slots `slots` -> [K, action_dim].  `stats` = (mean, std, mask) of `interface.device_unnormalization`.  Each slot keeps its
        own history, restarted when `assign_tasks` fills the slot.  Numpy in -> numpy out, torch in -> torch out."""
        torch = _torch()
        g = self.geometry
        s, sd = self._slot_map(slots, pool)
        as_torch = isinstance(actions, torch.Tensor)
        act = self._dev(actions, torch.float32)
        if tuple(act.shape) != (len(s), g.horizon, g.action_dim):
            raise ValueError(f"actions must be [{len(s)}, {g.horizon}, {g.action_dim}], got {tuple(act.shape)}")
        mean, std, mask = (self._dev(stats[0], torch.float32), self._dev(stats[1], torch.float32), self._dev(stats[2], torch.uint8))
        if not mean.numel() == std.numel() == mask.numel() == g.action_dim:
            raise ValueError(f"mean / std / mask must have {g.action_dim} entries")
        out = torch.empty(len(s), g.action_dim, dtype=torch.float32, device=self.device)
        self._ctx.ensemble_slots(pool._h, sd.data_ptr(), len(s), act.data_ptr(), mean.data_ptr(), std.data_ptr(), mask.data_ptr(),
                                 out.data_ptr(), self._stream())
        if as_torch:
            return out
        torch.cuda.current_stream(self.device).synchronize()
        return out.cpu().numpy()

    def sample_actions(self, images, instruction_dict=None, task=None, timestep_pad_mask=None,
                       base_params: GeneratedWeights = None, train: bool = False, rng=None,
                       image_embeddings=None, attention_maps: bool = False, slots=None):
        """hypervla/model.py:85-137.  images uint8 [B, 1, H, W, 3] (or [B, H, W, 3]) -> actions
        [B, horizon, action_dim].  `attention_maps=True` also returns the two attention slices the reference's wrapper keeps
        from the intermediates (hypervla_interface.py:208-217): DINOv2's CLS-query attention over the patches, every layer and
        head, and the generated policy's action-token attention over the patches (with use_language_token: over the language
        tokens first, then the patches, [B, layers, heads, lang_tokens + P]).
        With use_language_token the language tokens the policy reads are those given to create_tasks / assign_tasks for these
        episodes (kept beside their weights); `instruction_dict` is not read here, as before.
        `slots` (episode pool): step only these K slots of `base_params` (`hvla_step_slots`): images [K, ...] in, every output
        [K, ...] out, row k that of slot slots[k]."""
        if attention_maps and getattr(self.geometry, "differential", False):
            raise ValueError("attention_maps=True with vit_kwargs.use_differential_transformer: the reference sows neither "
                             "attention_weights nor attention_map in that branch (transformer.py:166-171), so there is no head map "
                             "to return; reference_attention_map (DINOv2's) is available")
        torch = _torch()
        if train:
            # train=True switches on nn.Dropout(dropout_rate) (base_vit.py:205, transformer.py:67,74,192,244) and the
            # image_embedding_noise (base_vit.py:123-127).  Every shipped config sets all of them to 0
            # (scripts/configs/hypervla_pretrain_config.py:333-339,376-380), where train=True is the same function as
            # train=False; a checkpoint that really asks for noise is refused rather than silently run without it.
            v = self.config["base_net_kwargs"]["vit_kwargs"]
            rates = {k: float(v.get(k, 0.0) or 0.0) for k in ("dropout_rate", "attention_dropout_rate", "image_embedding_noise")}
            rates["embedding_dropout_rate"] = float(self.config["base_net_kwargs"].get("embedding_dropout_rate", 0.0) or 0.0)
            if any(r > 0 for r in rates.values()):
                raise NotImplementedError(f"train=True with {rates}: dropout / embedding noise are not built (the README run uses 0)")
        if not isinstance(base_params, GeneratedWeights):
            raise TypeError("base_params must be the handle returned by create_tasks; a pytree or a theta array becomes one "
                            "through import_tasks (once per episode, not per step)")
        g = self.geometry
        as_torch = isinstance(images, torch.Tensor)
        img = self._dev(images, torch.uint8)
        if img.dim() == 5:
            if img.shape[1] != 1:
                raise ValueError("window size must be 1 (images.squeeze(1), model.py:117)")
            img = img[:, 0].contiguous()
        B = base_params.batch
        if slots is not None:
            slots_host, slots_dev = self._slot_map(slots, base_params)
            B = len(slots_host)
        if tuple(img.shape) != (B, g.image_size, g.image_size, 3):    # base_vit.py:86-89
            raise ValueError(f"Input image size must be {g.image_size}x{g.image_size}: got {tuple(img.shape)} for B={B}")
        actions = torch.empty(B, g.horizon, g.action_dim, dtype=torch.float32, device=self.device)
        logits = torch.empty(B, g.horizon, dtype=torch.float32, device=self.device)
        inter = {"gripper_logits": logits}
        if attention_maps:
            inter["dino_cls_attention"] = torch.empty(B, g.enc_layers, g.enc_heads, g.patches, dtype=torch.float32, device=self.device)
            # with use_language_token the action token's keys are [T language | P patches] (hypervla_interface.py:215 `[:-1]`)
            keys = g.patches + (g.lang_tokens if g.lang_in_policy else 0)
            inter["head_attention"] = torch.empty(B, g.layers, g.heads, keys, dtype=torch.float32, device=self.device)
            self._ctx.set_attention_outputs(inter["dino_cls_attention"].data_ptr(), inter["head_attention"].data_ptr())
        try:
            if slots is None:
                self._ctx.step(base_params._h, img.data_ptr(), actions.data_ptr(), logits.data_ptr(), B, self._stream())
            else:
                self._ctx.step_slots(base_params._h, slots_dev.data_ptr(), B, img.data_ptr(), actions.data_ptr(), logits.data_ptr(),
                                     self._stream())
        finally:
            if attention_maps:
                self._ctx.set_attention_outputs(0, 0)
        if as_torch:
            return actions, inter
        torch.cuda.current_stream(self.device).synchronize()
        return actions.cpu().numpy(), {k: v.cpu().numpy() for k, v in inter.items()}

    # stage-level entry points (policy-only variant of BASELINE config 2, parity tests)
    def encode_images(self, images):
        torch = _torch()
        g = self.geometry
        img = self._dev(images, torch.uint8)
        if img.dim() == 5:
            img = img[:, 0].contiguous()
        if tuple(img.shape[1:]) != (g.image_size, g.image_size, 3):      # the kernel reads B H W 3 bytes whatever it is given
            raise ValueError(f"encode_images wants uint8 frames [B, (1,) {g.image_size}, {g.image_size}, 3], got {tuple(img.shape)}")
        B = img.shape[0]
        tokens = torch.empty(B, g.patches, g.enc_dim, dtype=torch.float32, device=self.device)
        self._ctx.encode(img.data_ptr(), tokens.data_ptr(), B, self._stream())
        return tokens

    def reference_attention_map(self, images):
        """The alignment term's target of the fine-tune step (`FineTuner(attention_map_alignment=...)`): uint8 frames
        [B, (1,) H, W, 3] -> f32 [B, P] CUDA tensor, DINOv2's last-layer attention of the CLS query over the patches, mean over
        heads -- the reference's `DINO_outputs.attentions[-1][:, :, 0, 1:].mean(1)` (scripts/train.py:366-368,432-438).
        It is the serving encoder's `dino_cls_attention` output (`sample_actions(..., attention_maps=True)`), last layer.  The
        reference takes this map from the PRETRAINED encoder (`pretrained_image_encoder`, not the copy being fine-tuned): take it
        before any `publish()` of a trained encoder, or from a second model that keeps the pretrained weights.  The serving encoder
        computes with 16-bit operands; for a constant target that the loss only pulls towards, that precision is enough."""
        torch = _torch()
        g = self.geometry
        img = self._dev(images, torch.uint8)
        if img.dim() == 5:
            img = img[:, 0].contiguous()
        B = img.shape[0]
        tokens = torch.empty(B, g.patches, g.enc_dim, dtype=torch.float32, device=self.device)
        maps = torch.empty(B, g.enc_layers, g.enc_heads, g.patches, dtype=torch.float32, device=self.device)
        self._ctx.set_attention_outputs(maps.data_ptr(), 0)
        try:
            self._ctx.encode(img.data_ptr(), tokens.data_ptr(), B, self._stream())
        finally:
            self._ctx.set_attention_outputs(0, 0)
        return maps[:, -1].mean(1)

    def encode_initial_image(self, images):
        """The evaluators' `DINO_encode_image(initial_image).last_hidden_state` on the device
        (data/simpler/evaluate.py:155-163,264-274): uint8 [B, (1,) H, W, 3] -> f32 [B, 1 + P, E] (row 0 = CLS), ready to
        be passed as ``initial_state["patch_embeddings"]``.  Uses the DINOv2 weights of this checkpoint (the
        evaluators use the pretrained ones, which are the same tensors unless the encoder was fine-tuned)."""
        torch = _torch()
        g = self.geometry
        img = self._dev(images, torch.uint8)
        if img.dim() == 5:
            img = img[:, 0].contiguous()
        B = img.shape[0]
        hidden = torch.empty(B, g.patches + 1, g.enc_dim, dtype=torch.float32, device=self.device)
        self._ctx.encode_hidden(img.data_ptr(), hidden.data_ptr(), B, self._stream())
        return hidden

    def policy_from_tokens(self, tokens, base_params: GeneratedWeights):
        torch = _torch()
        g = self.geometry
        tok = self._dev(tokens, torch.float32)
        B = base_params.batch
        if tuple(tok.shape) != (B, g.patches, g.enc_dim):
            raise ValueError(f"tokens must be [{B}, {g.patches}, {g.enc_dim}]")
        actions = torch.empty(B, g.horizon, g.action_dim, dtype=torch.float32, device=self.device)
        logits = torch.empty(B, g.horizon, dtype=torch.float32, device=self.device)
        self._ctx.policy(base_params._h, tok.data_ptr(), actions.data_ptr(), logits.data_ptr(), B, self._stream())
        return actions, logits


    def action_loss(self, actions, gripper_logits, batch):
        """Per-sample MixActionHead.loss (action_heads.py:474-522) of policy outputs against an OXE batch
        {"action" [B,1,H,7], "action_pad_mask" [B,1,H,7], "timestep_pad_mask" [B,1]}; returns (loss [B], mean)."""
        torch = _torch()
        g = self.geometry
        act = self._dev(actions, torch.float32)
        lg = self._dev(gripper_logits, torch.float32)
        B = act.shape[0]
        tgt = self._dev(np.asarray(batch["action"])[:, 0], torch.float32)
        am = self._dev(np.asarray(batch["action_pad_mask"])[:, 0].astype(np.uint8), torch.uint8)
        tm = self._dev(np.asarray(batch["timestep_pad_mask"])[:, 0].astype(np.uint8), torch.uint8)
        if tuple(tgt.shape) != (B, g.horizon, g.action_dim) or tuple(lg.shape) != (B, g.horizon):
            raise ValueError("bad loss shapes")
        out = torch.empty(B, dtype=torch.float32, device=self.device)
        self._ctx.loss(act.data_ptr(), lg.data_ptr(), tgt.data_ptr(), tm.data_ptr(), am.data_ptr(), out.data_ptr(), B,
                       self._stream())
        return out, out.mean()


def read_params_file(path: str):
    """params_<step>.npz -> (parameters, position_table_source or None): the un-resized position table a converted checkpoint
    carries beside its parameters (hypervla/convert.py) is not one of them."""
    from .convert import POSITION_SOURCE_KEY
    with np.load(path) as z:
        params = {k: z[k] for k in z.files}
    return params, params.pop(POSITION_SOURCE_KEY, None)


HyperVLAModel = HyperVLA        # the name BASELINE.json's north_star uses


def _tree_map(fn, tree):
    if isinstance(tree, dict):
        return {k: _tree_map(fn, v) for k, v in tree.items()}
    return fn(tree)
