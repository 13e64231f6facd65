"""Host side of the fine-tune step (reference: scripts/train.py:405-542 ``train_step_pmap``,
octo/utils/train_utils.py:295-443 ``create_optimizer``).

    ft = FineTuner(model, batch=32)                         # image encoder frozen (the config default)
    ft = FineTuner(model, batch=32, train_encoder=True)     # README.md:55 fine_tune_pretrained_image_encoder=True
    loss = ft.step(instruction_dict, initial_state, images, batch)       # fwd + bwd + all-reduce + AdamW + EMA

All arithmetic is in libhvla (csrc/train.hip, the vector's layout in csrc/train_layout.h); torch owns the device buffers and, when a process group is
initialised, all-reduces the flat gradient (RCCL over xGMI on the GPU box — the `pmean` of train.py:460).
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from . import _native
from .config import Geometry, encoder_leaves, generated_leaves, shared_name, token_of


POSITION_SOURCE = "position_table_source"      # the layout's name of the tail: no checkpoint tensor (model.position_table_source)
POSITION_LEAF = "encoder_image_encoder_embeddings_position_embeddings"


def head_columns(g: Geometry):
    """[(leaf, head name, head column)] in `generated_leaves` order, and Gh: where a leaf's output head sits in the fused heads
    "W_cat" [C, Gh] / "b_cat" [Gh] (csrc/train_layout.h, the run table's hcol).  Without ``shared_block_heads`` the head column is the
    leaf's theta column and Gh = G; with it the L blocks' leaves of one name are ONE head, named `shared_head_name` and placed where
    the first block's leaf is, so Gh = G - (L - 1) (block floats)."""
    at, out, hc = {}, [], 0
    for l in generated_leaves(g):
        name = l.shared_head_name if g.shared_block_heads else l.head_name
        if name not in at:
            at[name] = hc
            hc += l.size
        out.append((l, name, at[name]))
    return out, hc


def token_runs(g: Geometry):
    """[(theta column, width, head column, token)]: the run table of csrc/train_layout.h (``layer_tokens``), one entry per
    maximal run of theta columns that reads one layer token and one contiguous range of head columns -- one per generated module."""
    runs = []
    for l, _, h in head_columns(g)[0]:
        t = token_of(g, l)
        if runs and runs[-1][3] == t and runs[-1][0] + runs[-1][1] == l.offset and runs[-1][2] + runs[-1][1] == h:
            runs[-1] = (runs[-1][0], runs[-1][1] + l.size, runs[-1][2], t)
        else:
            runs.append((l.offset, l.size, h, t))
    return runs


def _unique_heads(g: Geometry):
    """[(leaf, head name, head column)] with every head once (a shared head under its first block's leaf)."""
    seen, out = set(), []
    for l, name, h in head_columns(g)[0]:
        if name not in seen:
            seen.add(name)
            out.append((l, name, h))
    return out


def train_param_layout(g: Geometry, train_encoder: bool = False,
                       position_source: int = 0) -> Tuple[List[Tuple[str, int, Tuple[int, ...]]], int]:
    """[(name, offset, shape)] of the flat trainable-parameter vector == make_train_layout() in csrc/train_layout.h.
    The 73 output heads are the fused entries "W_cat" [C, G] and "b_cat" [G] (columns in pytree leaf order); with
    `train_encoder` the shared DINOv2 leaves follow as flat vectors under their checkpoint names.  `position_source` = n
    (hvla_train_position_source, trained encoder only): the n x n source of the position table follows them as the tail
    "position_table_source" [1, 1 + n*n, E]; the baked table keeps its slot among the leaves as a derived quantity."""
    C, F = g.ctx_dim, g.ctx_mlp
    out, off = [], 0

    def add(name, shape):
        nonlocal off
        out.append((name, off, tuple(shape)))
        off += int(np.prod(shape))

    add("task_token_projection/kernel", (g.lang_dim, C)); add("task_token_projection/bias", (C,))
    add("initial_image_projection/kernel", (g.enc_dim, C)); add("initial_image_projection/bias", (C,))
    add("task_pos_embedding", (1, g.lang_tokens, C)); add("initial_image_pos_embedding", (1, 1, C))
    add("layer_pos_embedding", (1, g.num_layer_tokens, C))      # NL rows with layer_tokens, else the one token
    for l in range(g.ctx_layers):
        b = f"Transformer_0/encoderblock_{l}/"
        a = b + "MultiHeadDotProductAttention_0/"
        hc = C // g.ctx_heads
        add(b + "LayerNorm_0/scale", (C,)); add(b + "LayerNorm_0/bias", (C,))
        add(b + "LayerNorm_1/scale", (C,)); add(b + "LayerNorm_1/bias", (C,))
        for nm in ("query", "key", "value"):
            add(a + nm + "/kernel", (C, g.ctx_heads, hc)); add(a + nm + "/bias", (g.ctx_heads, hc))
        add(a + "out/kernel", (g.ctx_heads, hc, C)); add(a + "out/bias", (C,))
        add(b + "MlpBlock_0/Dense_0/kernel", (C, F)); add(b + "MlpBlock_0/Dense_0/bias", (F,))
        add(b + "MlpBlock_0/Dense_1/kernel", (F, C)); add(b + "MlpBlock_0/Dense_1/bias", (C,))
    add("Transformer_0/encoder_norm/scale", (C,)); add("Transformer_0/encoder_norm/bias", (C,))
    Gh = head_columns(g)[1]                                     # == G unless shared_block_heads
    add("W_cat", (C, Gh)); add("b_cat", (Gh,))
    if train_encoder:
        for path, shape in encoder_leaves(g):
            add(shared_name(path), (int(np.prod(shape)),))
        if position_source:
            add(POSITION_SOURCE, (1, 1 + int(position_source) ** 2, g.enc_dim))
    return out, off


def gradient_buckets(g: Geometry, train_encoder: bool = False, position_source: int = 0) -> List[Tuple[str, int, int]]:
    """[(name, offset, length)] of the flat gradient in the order hvla_train_step finishes them (include/hvla.h,
    hvla_train_bucket_ranges): the shared DINOv2 leaves after the image encoder's backward, the output heads (W_cat,
    b_cat) after the weight-generation backward, the context encoder at the end of the step.  Contiguous, disjoint, and
    together the whole vector -- what `pmean(grads)` (scripts/train.py:460) is cut into so that each all-reduce runs
    under the rest of the backward pass.  The position table's source (`position_source`) is the tail of the encoder's bucket."""
    layout, total = train_param_layout(g, train_encoder, position_source)
    at = {name: off for name, off, _ in layout}
    wcat = at["W_cat"]
    n_hyper = at["b_cat"] + head_columns(g)[1]
    out = []
    if train_encoder:
        out.append(("image_encoder", n_hyper, total - n_hyper))
    out.append(("output_heads", wcat, n_hyper - wcat))
    out.append(("context_encoder", 0, wcat))
    return out


def _source_side(position_source) -> int:
    """n of a source table [1, 1 + n*n, E] (None: 0)."""
    return 0 if position_source is None else int(round(np.sqrt(np.shape(position_source)[1] - 1)))


def pack_params(g: Geometry, params: Dict[str, np.ndarray], train_encoder: bool = False, position_source=None) -> np.ndarray:
    """`position_source`: the source table itself (float32 [1, 1 + n*n, E]), packed as the tail."""
    layout, total = train_param_layout(g, train_encoder, _source_side(position_source) if train_encoder else 0)
    flat = np.zeros(total, np.float32)
    heads = _unique_heads(g)                                   # head columns ascend in this order
    for name, off, shape in layout:
        n = int(np.prod(shape))
        if name == "W_cat":
            w = np.concatenate([np.asarray(params[h + "/kernel"], np.float32) for _, h, _ in heads], axis=1)
            flat[off:off + n] = w.reshape(-1)
        elif name == "b_cat":
            flat[off:off + n] = np.concatenate([np.asarray(params[h + "/bias"], np.float32).reshape(-1) for _, h, _ in heads])
        elif name == POSITION_SOURCE:
            flat[off:off + n] = np.asarray(position_source, np.float32).reshape(-1)
        else:
            flat[off:off + n] = np.asarray(params[name], np.float32).reshape(-1)
    return flat


def unpack_params(g: Geometry, flat: np.ndarray, train_encoder: bool = False, position_source: int = 0):
    """flat vector (parameters or gradients) -> reference-named tensors.  With `position_source` = n the result is
    (tensors, source [1, 1 + n*n, E]): the tail is no checkpoint tensor and stays out of the dict."""
    layout, _ = train_param_layout(g, train_encoder, position_source)
    heads = _unique_heads(g)
    out: Dict[str, np.ndarray] = {}
    source = None
    for name, off, shape in layout:
        v = np.asarray(flat[off:off + int(np.prod(shape))]).reshape(shape)
        if name == "W_cat":
            for l, h, c in heads:
                out[h + "/kernel"] = v[:, c:c + l.size].copy()
        elif name == "b_cat":
            for l, h, c in heads:
                out[h + "/bias"] = v[c:c + l.size].copy()
        elif name == POSITION_SOURCE:
            source = v.copy()
        else:
            out[name] = v.copy()
    return (out, source) if (train_encoder and position_source) else out


def lr_rsqrt(step: int, peak: float, warmup: int = 2000, timescale: int = 10000, init: float = 0.0) -> float:
    """octo/utils/train_utils.py:212-225 ("rsqrt": linear warm-up joined to peak / sqrt((s + ts) / ts))."""
    if step < warmup:
        return init + (peak - init) * step / warmup
    s = step - warmup
    return peak / float(np.sqrt((s + timescale) / timescale))


def weight_decay_mask(g: Geometry, strategy: str, train_encoder: bool = False, position_source: int = 0) -> np.ndarray:
    """uint8 [n_params]: where `create_optimizer`'s decoupled weight decay applies (octo/utils/train_utils.py:325-382).
    The reference tests `jax.tree_util.keystr(path)` of every leaf of the hypernetwork's parameter tree; an output head is
    the module `output_head_<flat base-net leaf name>` (hypervla/model.py:342) with leaves `kernel` and `bias`, so the
    NAME of the generated leaf is part of the path of both.

    "v1" (the config default, hypervla_pretrain_config.py:290; train_utils.py:378-382): `"kernel" in keystr(path)` -- every
    Dense kernel of the hypernetwork, every output head's kernel, the BIAS of every head that generates a base-net
    *kernel* leaf (its path contains `..._kernel`), and the encoder leaves named *kernel*.
    "v2" (:326-330): everything except leaves with "norm" in the path that are not output heads.
    "v3" (:335-350): output heads that generate *kernel* leaves (kernel and bias), every leaf of the shared image
    encoder, and the remaining *kernel* leaves (context encoder, projections).
    "v5" (the README run, README.md:29; :354-363): as v3 without the context-encoder kernels.
    "v4" adds a second backward pass through a weight-decay loss (scripts/train.py:473-480) and is not built.
    With `position_source` the tail IS the reference's leaf `encoder_image_encoder_embeddings_position_embeddings` and gets that
    leaf's value; the baked slot is no parameter and gets 0."""
    if strategy not in ("v1", "v2", "v3", "v5"):
        raise ValueError(f"weight_decay_strategy {strategy!r}: 'v1', 'v2', 'v3' and 'v5' are built (v4 is not)")
    layout, total = train_param_layout(g, train_encoder, position_source)
    if train_encoder and position_source:          # the tail under the leaf's name, the slot under one that no rule matches
        layout = [(POSITION_LEAF if name == POSITION_SOURCE else "" if name == POSITION_LEAF else name, off, shape)
                  for name, off, shape in layout]
    heads, Gh = _unique_heads(g), head_columns(g)[1]
    mask = np.zeros(total, np.uint8)
    cols = np.zeros(Gh, np.uint8)
    for l, _, c in heads:
        if "kernel" in l.flat_name:
            cols[c:c + l.size] = 1
    for name, off, shape in layout:
        n = int(np.prod(shape))
        if name == "":                            # the baked position table's slot (a derived quantity)
            continue
        if name == "W_cat":                       # [C, G]: the kernels of the 73 output heads
            mask[off:off + n] = 1 if strategy in ("v1", "v2") else np.tile(cols, shape[0])
        elif name == "b_cat":                     # their biases: `output_head_<..._kernel>/bias` contains "kernel"
            mask[off:off + n] = 1 if strategy == "v2" else cols
        elif name.startswith("encoder_image_encoder_"):
            if strategy == "v1":
                mask[off:off + n] = 1 if "kernel" in name else 0
            elif strategy == "v2":
                mask[off:off + n] = 0 if "norm" in name.lower() else 1
            else:
                mask[off:off + n] = 1
        elif strategy == "v2":
            mask[off:off + n] = 0 if "norm" in name.lower() else 1
        elif strategy in ("v1", "v3") and "kernel" in name:
            mask[off:off + n] = 1
    return mask


def frozen_plan(g: Geometry, frozen_keys, train_encoder: bool = False, position_source: int = 0,
                base_weight_decay: float = 0.0) -> Tuple[np.ndarray, int]:
    """(mask uint8 [n_params], frozen_buckets): `create_optimizer(frozen_keys=...)` (octo/utils/train_utils.py:242-292, 385,
    428-439) over the flat vector.  The reference flattens the parameter tree, names a leaf `".".join(path)` and freezes it
    (`multi_transform({"trainable": tx, "frozen": set_to_zero()})` round the whole chain) iff `fnmatch(name, key)` holds for any
    key; a leaf's name here is its checkpoint name with "/" replaced by ".":  `Transformer_0.encoderblock_3.MlpBlock_0.Dense_0.kernel`,
    `task_token_projection.bias`, `output_head_<flat base-net leaf>.kernel` / `.bias`, and the encoder leaves
    `encoder_image_encoder_<...>`, each a single key without a dot.  Keys that match nothing are accepted silently, as by the
    reference (its default `("*hf_model*",)` matches nothing in this tree).

    W_cat / b_cat are the 73 heads fused: a frozen head freezes its column range in every row of W_cat (`.kernel`) or its range
    of b_cat (`.bias`), per element, the way weight_decay_mask builds `cols`.  With `position_source` the tail IS the leaf
    `encoder_image_encoder_embeddings_position_embeddings` and has its status; so has the baked slot, which is derived from it
    (re-derived from an unchanged tail it keeps its bits).

    `frozen_buckets` has bit b set iff every element of gradient bucket b (hvla_train_bucket_ranges: 0 encoder, 1 output heads,
    2 context encoder) is frozen: hvla_train_step then does not compute that bucket.

    ValueError: nothing trainable is left; the whole encoder is frozen with train_encoder=True (that is train_encoder=False);
    an encoder leaf is frozen while base_weight_decay > 0 -- the reference adds its `delta_change_decay`
    (scripts/train.py:465-471) after `tx.update`, so there a "frozen" encoder leaf still moves towards the pretrained weights.
    That is not reproduced: frozen means untouched here."""
    from fnmatch import fnmatch
    keys = (frozen_keys,) if isinstance(frozen_keys, str) else tuple(frozen_keys)
    hit = lambda name: any(fnmatch(name.replace("/", "."), k) for k in keys)
    layout, total = train_param_layout(g, train_encoder, position_source)
    heads, Gh = _unique_heads(g), head_columns(g)[1]           # a shared head is frozen once: it is one range of columns
    wcols, bcols = np.zeros(Gh, np.uint8), np.zeros(Gh, np.uint8)
    for l, h, c in heads:
        wcols[c:c + l.size] = hit(h + "/kernel")
        bcols[c:c + l.size] = hit(h + "/bias")
    mask = np.zeros(total, np.uint8)
    for name, off, shape in layout:
        n = int(np.prod(shape))
        if name == "W_cat":
            mask[off:off + n] = np.tile(wcols, shape[0])
        elif name == "b_cat":
            mask[off:off + n] = bcols
        else:                                     # the tail under the name of the leaf it is
            mask[off:off + n] = hit(POSITION_LEAF if name == POSITION_SOURCE else name)
    if mask.all():
        raise ValueError(f"frozen_keys {keys!r} freeze every parameter: nothing is left to train")
    flags = 0
    for name, off, n in gradient_buckets(g, train_encoder, position_source):
        if mask[off:off + n].all():
            flags |= 1 << {"image_encoder": 0, "output_heads": 1, "context_encoder": 2}[name]
    if flags & 1:
        raise ValueError(f"frozen_keys {keys!r} freeze every leaf of the image encoder: use train_encoder=False, which neither "
                         "differentiates the encoder nor keeps optimizer state for it")
    n_hyper = total if not train_encoder else gradient_buckets(g, True, position_source)[0][1]
    if base_weight_decay > 0 and mask[n_hyper:].any():
        raise ValueError("frozen_keys freeze image-encoder leaves while base_weight_decay > 0: the reference adds its pull towards "
                         "the pretrained encoder (delta_change_decay, scripts/train.py:465-471) after the optimizer's update, so "
                         "its 'frozen' encoder leaves still move.  That is not reproduced here (a frozen element is never "
                         "written): freeze encoder leaves with base_weight_decay=0, or freeze none of them")
    return mask, flags


def attention_loss_plan(attention_entropy: float = 0.0, attention_map_alignment: float = 0.0, num_steps=None):
    """(entropy coefficient, alignment coefficient, num_steps) of `config.auxiliary_loss.attention_entropy` /
    `.attention_map_alignment` (scripts/train.py:348-373), checked.  The alignment term is annealed by 1 - step / num_steps
    (:370-371), so a positive alignment coefficient needs the run's `num_steps`."""
    ent, ali = float(attention_entropy), float(attention_map_alignment)
    if not (np.isfinite(ent) and np.isfinite(ali) and ent >= 0.0 and ali >= 0.0):
        raise ValueError(f"attention_entropy {attention_entropy!r} / attention_map_alignment {attention_map_alignment!r} must be finite and >= 0")
    if ali > 0.0 and (num_steps is None or int(num_steps) < 1):
        raise ValueError("attention_map_alignment > 0 needs num_steps >= 1: the reference anneals the term by 1 - step / num_steps "
                         "(scripts/train.py:370-371)")
    return ent, ali, None if num_steps is None else int(num_steps)


def alignment_weight(attention_map_alignment: float, step: int, num_steps) -> float:
    """`annealing_factor * attention_map_alignment` of scripts/train.py:370-371 at update `step` (the reference's `state.step`);
    zero, not negative, past the end of the schedule."""
    if not attention_map_alignment > 0.0:
        return 0.0
    return max(0.0, 1.0 - float(step) / float(num_steps)) * float(attention_map_alignment)


def check_reference_attention(attention_map_alignment: float, reference_attention, batch: int, patches: int):
    """`reference_attention` is needed exactly when the alignment coefficient is positive, as [batch, patches]."""
    if not attention_map_alignment > 0.0:
        return
    if reference_attention is None:
        raise ValueError("attention_map_alignment > 0 needs reference_attention [B, P]: the pretrained DINOv2's last-layer CLS "
                         "attention over the patches, mean over heads (HyperVLA.reference_attention_map)")
    shape = tuple(reference_attention.shape) if hasattr(reference_attention, "shape") else np.shape(reference_attention)
    if shape != (batch, patches):
        raise ValueError(f"reference_attention must be [{batch}, {patches}], got {shape}")


# ---- the train=True noise (hvla_train_noise_set; csrc/noise.h), restated on the host bit for bit -----------------
# kinds of a noise site; site = kind | layer << 8
(NOISE_POLICY_INPUT, NOISE_ATTN_OUT, NOISE_MLP_HIDDEN, NOISE_MLP_OUT, NOISE_TOKENS, NOISE_CONTEXT, NOISE_IMAGE_CLS) = range(1, 8)


def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32 (Salmon et al., SC'11; Random123's constants): `counter` uint32 [..., 4] and `key` uint32 [..., 2] (broadcast
    against each other) -> uint32 [..., 4].  csrc/noise.h's philox4x32_10 word for word."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def noise_site(kind: int, layer: int = 0) -> int:
    return int(kind) | int(layer) << 8


def noise_words(seed: int, site: int, sample_id: int, draw: int, n: int) -> np.ndarray:
    """uint32 [n]: the word of elements [0, n) of `site` for the sample with GLOBAL index `sample_id`: element e is word e & 3 of
    the block with counter (e >> 2, sample_id, site, draw) under key (seed lo, seed hi)."""
    blocks = (int(n) + 3) // 4
    ctr = np.empty((blocks, 4), np.uint32)
    ctr[:, 0] = np.arange(blocks, dtype=np.uint32)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = int(sample_id) & 0xFFFFFFFF, int(site) & 0xFFFFFFFF, int(draw) & 0xFFFFFFFF
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)).reshape(-1)[:int(n)]


def dropout_threshold(rate: float) -> int:
    """ceil(rate 2^24) on the float32 rate in double, as the library computes it: P(keep) = 1 - threshold / 2^24."""
    return int(np.ceil(float(np.float32(rate)) * 2.0 ** 24))


def noise_multipliers(rate: float, seed: int, site: int, sample_id: int, draw: int, n: int) -> np.ndarray:
    """float32 [n]: 1 / keep_prob where (word >> 8) >= threshold, else 0; keep_prob = float32(1) - float32(rate)."""
    keep = (noise_words(seed, site, sample_id, draw, n) >> np.uint32(8)) >= np.uint32(dropout_threshold(rate))
    return np.where(keep, np.float32(1.0) / (np.float32(1.0) - np.float32(rate)), np.float32(0.0)).astype(np.float32)


def noise_normals(seed: int, site: int, sample_id: int, draw: int, n: int) -> np.ndarray:
    """float64 [n]: Box-Muller on the word pairs (w0, w1) and (w2, w3) of every block, evaluated in double (the device evaluates
    the same expression in float32): u1 = ((w >> 8) + 1) 2^-24, u2 = (w' >> 8) 2^-24, z0 = sqrt(-2 ln u1) cos(2 pi u2) for the
    pair's first element and z1 = sqrt(-2 ln u1) sin(2 pi u2) for its second."""
    w = noise_words(seed, site, sample_id, draw, (int(n) + 3) // 4 * 4).reshape(-1, 2)
    u1 = ((w[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=-1).reshape(-1)[:int(n)]


def train_noise_from_config(config) -> Dict[str, float]:
    """FineTuner's noise keywords from a reference-shaped config (the dict of `config.model`, or one that holds it under "model"):
    vit_kwargs.dropout_rate, vit_kwargs.image_embedding_noise, hypernet_kwargs.embedding_dropout_rate, hypernet_kwargs.image_dropout.
    ValueError, naming the key, for the noise that is not built: a non-zero context_encoder_kwargs.dropout_rate or
    .attention_dropout_rate, or hypernet_kwargs.final_dropout_rate."""
    cfg = config.get("model", config)
    h = cfg.get("hypernet_kwargs", {})
    v = cfg.get("base_net_kwargs", {}).get("vit_kwargs", {})
    ce = h.get("context_encoder_kwargs", {})
    for where, d, key in (("hypernet_kwargs.context_encoder_kwargs", ce, "dropout_rate"),
                          ("hypernet_kwargs.context_encoder_kwargs", ce, "attention_dropout_rate"),
                          ("hypernet_kwargs", h, "final_dropout_rate")):
        if float(d.get(key, 0.0) or 0.0) != 0.0:
            raise ValueError(f"{where}.{key}={d.get(key)!r} is not built: the fine-tune step draws the policy's dropout, the image "
                             "embedding noise, embedding_dropout_rate and image_dropout only (DESIGN.md §21)")
    return dict(dropout_rate=float(v.get("dropout_rate", 0.0) or 0.0),
                image_embedding_noise=float(v.get("image_embedding_noise", 0.0) or 0.0),
                embedding_dropout_rate=float(h.get("embedding_dropout_rate", 0.0) or 0.0),
                image_dropout=float(h.get("image_dropout", 0.0) or 0.0))


# The keys of the reference's `info` (scripts/train.py:506-529) that FineTuner.info() returns, in its order; one
# `task_loss_<name>` per task follows, and the two attention terms are present only while their coefficient is positive.
INFO_KEYS = ("training_loss", "grad_norm", "update_norm", "param_norm", "learning_rate", "continuous_loss", "gripper_loss",
             "base_params_norm", "attention_entropy_loss", "attention_alignment_loss")
# key -> (slot of hvla_train_metrics' vector, whether the slot is behind the 2 n_tasks task slots: the replicated block)
_INFO_SLOT = {"training_loss": (_native.HVLA_METRIC_TRAINING_LOSS, False), "grad_norm": (_native.HVLA_METRIC_GRAD_NORM, True),
              "update_norm": (_native.HVLA_METRIC_UPDATE_NORM, True), "param_norm": (_native.HVLA_METRIC_PARAM_NORM, True),
              "continuous_loss": (_native.HVLA_METRIC_CONTINUOUS_LOSS, False), "gripper_loss": (_native.HVLA_METRIC_GRIPPER_LOSS, False),
              "base_params_norm": (_native.HVLA_METRIC_BASE_PARAMS_NORM, False),
              "attention_entropy_loss": (_native.HVLA_METRIC_ATTENTION_ENTROPY, False),
              "attention_alignment_loss": (_native.HVLA_METRIC_ATTENTION_ALIGNMENT, False)}


def resolve_task_index(task_index, task_names, batch: int) -> np.ndarray:
    """int32 [batch]: the reference's `task_index` ({name: bool [B]}, scripts/train.py:455-456: one mask per dataset of the mix) as
    one task id per sample, the position of the name in `task_names`; -1 for a sample no mask claims (counted nowhere).  ValueError: a
    name that is not in `task_names`, a mask of another length, a sample two masks claim (an id cannot say that)."""
    names = tuple(task_names)
    ids = np.full(batch, -1, np.int32)
    for name, mask in (task_index or {}).items():
        if name not in names:
            raise ValueError(f"task_index names {name!r}, task_names are {names!r}")
        m = np.asarray(mask).astype(bool).reshape(-1)
        if m.shape[0] != batch:
            raise ValueError(f"task_index[{name!r}] has {m.shape[0]} entries, the batch has {batch}")
        if (ids[m] >= 0).any():
            b = int(np.nonzero(m & (ids >= 0))[0][0])
            raise ValueError(f"task_index masks overlap: sample {b} is in {names[ids[b]]!r} and in {name!r}")
        ids[m] = names.index(name)
    return ids


def reduce_info_vector(vec, n_tasks: int, world: int):
    """The cross-rank half of the reference's `info` (scripts/train.py:498, 522-528), in place on hvla_train_metrics' vector (a device
    or a CPU tensor, f32 [HVLA_METRIC_N + 2 n_tasks]): ONE all_reduce(SUM) over the rank-local means and the task sums and counts, then
    the means divided by `world` (pmean; the sums and counts stay sums: psum).  The replicated block (grad, param and update norm) is
    not touched: after the gradient all-reduce it is equal on every rank already.  Needs an initialised process group; returns vec."""
    import torch.distributed as dist
    local = _native.HVLA_METRIC_LOCAL_N
    head = vec[:local + 2 * int(n_tasks)]
    dist.all_reduce(head, op=dist.ReduceOp.SUM)
    head[:local] /= world
    return vec


def info_from_vector(vec, task_names=(), learning_rate=None, attention_entropy=True, attention_alignment=True) -> Dict[str, object]:
    """hvla_train_metrics' vector as the reference's `info` dict: 0-d views into `vec` (nothing is copied or synchronised), in
    INFO_KEYS order, then `task_loss_<name>` = sum / count (NaN for a task without a sample, as the reference's 0 / 0)."""
    n = len(tuple(task_names))
    out = {}
    for key in INFO_KEYS:
        if key == "learning_rate":
            if learning_rate is not None:
                out[key] = learning_rate
            continue
        if (key == "attention_entropy_loss" and not attention_entropy) or (key == "attention_alignment_loss" and not attention_alignment):
            continue
        slot, replicated = _INFO_SLOT[key]
        out[key] = vec[slot + (2 * n if replicated else 0)]
    local = _native.HVLA_METRIC_LOCAL_N
    for t, name in enumerate(task_names):
        out[f"task_loss_{name}"] = vec[local + t] / vec[local + n + t]
    return out


class FineTuner:
    """One optimizer state of the fine-tune step.  Defaults are the README run's (README.md:29-31,61 and
    scripts/configs/hypervla_pretrain_config.py:286-321): weight_decay_strategy v5, learning rate 3e-4 (rsqrt) for the
    hypernetwork and 3e-5 for the shared image encoder, base_weight_decay 0, no gradient accumulation, EMA 0.999 started at
    update 5000 (`ema_start_step`; the EMA is a copy of the parameters at that update and an average afterwards,
    scripts/train.py:681-690).  `frozen_keys`: the reference's create_optimizer(frozen_keys=...) -- fnmatch patterns over the dotted
    leaf names (frozen_plan); matching elements keep their parameters, moments and EMA bit for bit, stay out of the clip's global
    norm, and a gradient bucket that is frozen as a whole is neither computed nor all-reduced.
    `attention_entropy`, `attention_map_alignment`: the coefficients of `config.auxiliary_loss` (scripts/train.py:348-373, default 0 =
    off): the entropy of the action token's attention row in the last policy layer, and its squared distance to `reference_attention`
    (forward_backward / step; `model.reference_attention_map(images)`), annealed by 1 - step_count / `num_steps`.  Both are added to
    every sample's loss; `aux_metrics` holds the un-weighted terms of the last step under the reference's metric names.
    `metrics=True` (default off: nothing is allocated and step / apply do exactly what they do without it): what the reference logs
    every step (scripts/train.py:494-529), computed on the device by hvla_train_metrics around the optimizer and read with `info()`;
    costs one more [n] f32 vector (the snapshot for update_norm).  `task_names`: the datasets of the mix, for `task_loss_<name>`
    (`forward_backward(task_index=...)`).
    `language_tokens=True`: fine-tune a model with `vit_kwargs.use_language_token` (hvla_train_language_tokens): the
    policy runs with the instruction's token embeddings in front of the patches, as the reference's loop does for such a model; the
    two heads `output_head_encoder_language_token_projection_{kernel,bias}` train (or freeze, `frozen_keys`) like every other head.
    Without the keyword such a model is refused; the attention terms are not defined for it.
    `differential=True`: fine-tune a model with `vit_kwargs.use_differential_transformer` (hvla_train_differential): every
    policy block runs DifferentialAttention forward and backward; the heads of the four lambda vectors and of `subln/weight` train (or
    freeze, `frozen_keys`) like every other head.  Without the keyword such a model is refused; the attention terms and the four noise
    arguments are refused with it.
    `layer_tokens=True`: fine-tune a model with `hypernet_kwargs.share_layer_index=False` (hvla_train_layer_tokens): the
    context encoder runs with its NL layer tokens, every generated leaf is made from the context row of its module's token, and with
    `share_TF_output_head` the blocks' shared heads train (decay, freeze) as ONE tensor each, whose gradient is the sum over the blocks.
    Combines with `language_tokens` and `differential`.  Without the keyword such a model is refused.
    `dropout_rate`, `image_embedding_noise`, `embedding_dropout_rate`, `image_dropout` (all 0 = off, the default; `train_noise_from_config`
    reads them from a reference-shaped config): the four noise sources the reference's loop switches on with train=True
    (hvla_train_noise_set), drawn from a counter-based generator keyed by `noise_seed` -- equal to jax's noise in
    distribution, not in bits.  Every forward_backward that is not forward_only draws afresh (`noise_draw` counts them, micro-batches
    of a gradient accumulation included); a sample's noise depends on its global index rank * batch + row, not on its row;
    `validate()` draws nothing."""

    def __init__(self, model, batch: int, peak_lr: float = 3e-4, weight_decay: float = 0.05, clip: float = 1.0,
                 ema_decay: float = 0.999, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8,
                 train_encoder: bool = False, base_lr: float = 3e-5, base_weight_decay: float = 0.0,
                 weight_decay_strategy: str = "v5", ema_start_step: int = 5000, grad_accumulation_steps: int = 1,
                 accept_baked_position_table: bool = False, frozen_keys=(), attention_entropy: float = 0.0,
                 attention_map_alignment: float = 0.0, num_steps=None, metrics: bool = False, task_names=(), language_tokens: bool = False,
                 dropout_rate: float = 0.0, image_embedding_noise: float = 0.0, embedding_dropout_rate: float = 0.0,
                 image_dropout: float = 0.0, noise_seed: int = 0, differential: bool = False, layer_tokens: bool = False):
        self.attention_entropy, self.attention_map_alignment, self.num_steps = attention_loss_plan(
            attention_entropy, attention_map_alignment, num_steps)
        self.language_tokens = bool(language_tokens)
        self.differential = bool(differential)
        self.noise = dict(policy_dropout=float(dropout_rate), image_embedding_noise=float(image_embedding_noise),
                          context_dropout=float(embedding_dropout_rate), image_dropout=float(image_dropout))
        self.noise_on = any(v != 0.0 for v in self.noise.values())
        self.noise_seed, self.noise_draw = int(noise_seed), 0
        self.layer_tokens = bool(layer_tokens)
        if getattr(model.geometry, "layer_tokens", False) and not self.layer_tokens:
            raise ValueError("fine-tuning a model with hypernet_kwargs.share_layer_index=False is not built; serving is "
                             "(the training kernels run one layer token and one GEMM over the output heads, DESIGN.md §24)")
        if self.layer_tokens and not getattr(model.geometry, "layer_tokens", False):
            raise ValueError("layer_tokens=True needs a model with hypernet_kwargs.share_layer_index=False: this model's context "
                             "encoder has one layer token")
        if getattr(model.geometry, "differential", False) and not self.differential:
            raise ValueError("fine-tuning a model with vit_kwargs.use_differential_transformer is not built; serving is "
                             "(without differential=True the training kernels run no DifferentialAttention, DESIGN.md §23)")
        if self.differential and not getattr(model.geometry, "differential", False):
            raise ValueError("differential=True needs a model with vit_kwargs.use_differential_transformer: this model's policy "
                             "has no DifferentialAttention")
        if self.differential and self.language_tokens:
            raise ValueError("differential=True with language_tokens=True: use_differential_transformer together with "
                             "use_language_token is not built (DESIGN.md §22)")
        if self.differential and (self.attention_entropy > 0 or self.attention_map_alignment > 0):
            raise ValueError("attention_entropy / attention_map_alignment are not defined with differential=True: the module's map is "
                             "the signed A1 - lambda A2, which has no entropy (DESIGN.md §23)")
        if self.differential and self.noise_on:
            raise ValueError("dropout_rate / image_embedding_noise / embedding_dropout_rate / image_dropout with differential=True are "
                             "not built: the noise is restated for the other attention modules only (DESIGN.md §23)")
        if getattr(model.geometry, "lang_in_policy", False) and not self.language_tokens:
            raise ValueError("fine-tuning a model with vit_kwargs.use_language_token is not built: the training kernels run the "
                             "policy without language tokens (serving it is, DESIGN.md §11)")
        if self.language_tokens and not getattr(model.geometry, "lang_in_policy", False):
            raise ValueError("language_tokens=True needs a model with vit_kwargs.use_language_token: this model's policy has no "
                             "language_token_projection")
        if self.language_tokens and (self.attention_entropy > 0 or self.attention_map_alignment > 0):
            raise ValueError("attention_entropy / attention_map_alignment are not defined with language_tokens=True: the reference "
                             "compares the action token's attention over lang_tokens + P keys with a P-wide DINOv2 map "
                             "(scripts/train.py:364-368), which does not broadcast; the entropy term is left out with it")
        import torch
        self.torch, self.model, self.g, self.B = torch, model, model.geometry, batch
        self.train_encoder = bool(train_encoder)
        baked = (model.config or {}).get("position_embeddings_baked_from")
        source = getattr(model, "position_table_source", None)
        # the reference's leaf is the un-resized table: with it at hand it is the parameter, the baked table a derived quantity
        self.position_source = source if self.train_encoder and not accept_baked_position_table else None
        self.source_n = _source_side(self.position_source)
        self._drops_source = self.train_encoder and accept_baked_position_table and source is not None
        if self.train_encoder and baked and source is None and not accept_baked_position_table:
            raise ValueError(
                f"this checkpoint's DINOv2 position table was baked from {baked} to the run-time grid at conversion time "
                "(hypervla/convert.py); the reference trains the ORIGINAL table through interpolate_pos_encoding, so its "
                "gradient and Adam state differ and the result cannot be exported back into a reference-shaped "
                "checkpoint.  This model has no position_table_source (checkpoints converted before the converter kept it): convert "
                "again, or pass accept_baked_position_table=True to train the baked table anyway (INTEGRATION.md).")
        dev = model.device
        self.interp_w = None
        if self.source_n:
            from .convert import position_interp_weights
            self.interp_w = torch.as_tensor(position_interp_weights(self.source_n, self.g.grid)).to(dev).contiguous()
        # create_optimizer(frozen_keys=...): fnmatch patterns over the dotted leaf names (frozen_plan); no match, no mask
        self.frozen_keys = (frozen_keys,) if isinstance(frozen_keys, str) else tuple(frozen_keys)
        plan, self.frozen_buckets = frozen_plan(self.g, self.frozen_keys, self.train_encoder, self.source_n, base_weight_decay)
        self.frozen_count = int(plan.sum())
        self.trainable_count = int(plan.size) - self.frozen_count
        self.frozen = torch.as_tensor(plan).to(dev) if self.frozen_count else None
        self._select()
        n, G, work, n_hyper = model._ctx.train_sizes(batch, self.train_encoder)
        layout, total = train_param_layout(self.g, self.train_encoder, self.source_n)
        assert n == total, (n, total)
        self.n, self.G, self.n_hyper = n, G, n_hyper
        f32 = dict(dtype=torch.float32, device=dev)
        self.params = torch.as_tensor(pack_params(self.g, model.params, self.train_encoder, self.position_source)).to(dev)
        if self.source_n:
            self._derive_slot(layout)
        self.grads = torch.zeros(n, **f32)
        self.mu = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        self.nu = torch.zeros(n, **f32)
        self.ema = self.params.clone()
        self.theta = torch.empty(batch, G, **f32)
        self.dtheta = torch.empty(batch, G, **f32)
        self.work = torch.empty(work, **f32)
        self.loss = torch.zeros(batch, **f32)
        self.actions = torch.zeros(batch, self.g.horizon, self.g.action_dim, **f32)
        self.logits = torch.zeros(batch, self.g.horizon, **f32)
        # hvla_train_attention_losses' metric outputs: ent_b / align_b of the last step
        self.aux_entropy = torch.zeros(batch, **f32) if self.attention_entropy > 0 else None
        self.aux_alignment = torch.zeros(batch, **f32) if self.attention_map_alignment > 0 else None
        self.aux_metrics: Dict[str, "torch.Tensor"] = {}
        self.sqsum = torch.zeros(1, **f32)
        self.weight_decay_strategy = weight_decay_strategy
        self.wd_mask = torch.as_tensor(weight_decay_mask(self.g, weight_decay_strategy, self.train_encoder, self.source_n)).to(dev)
        # the pull towards the pretrained encoder only exists for base_weight_decay > 0 (scripts/train.py:469)
        self.params0 = self.params[n_hyper:].clone() if self.train_encoder and base_weight_decay > 0 else None
        self.accum_k = int(grad_accumulation_steps)
        if self.accum_k < 1:
            raise ValueError("grad_accumulation_steps >= 1")
        self.acc = torch.zeros(n, **f32) if self.accum_k > 1 else None
        self.micro = 0                                  # micro-batches since the last update
        self.buf = self._buffers(self.grads)
        self.buf_acc = self._buffers(self.acc) if self.acc is not None else None
        self.hy = dict(b1=b1, b2=b2, eps=eps, weight_decay=weight_decay, clip=clip, ema_decay=ema_decay,
                       base_weight_decay=base_weight_decay)
        self.peak_lr, self.base_peak_lr, self.step_count = peak_lr, base_lr, 0
        self.ema_start_step = int(ema_start_step)
        self._bucket_setup()
        self.metrics = bool(metrics)
        self.task_names = tuple(task_names)
        if self.task_names and not self.metrics:
            raise ValueError("task_names are the names of info()'s task_loss_<name>: they need metrics=True")
        if len(set(self.task_names)) != len(self.task_names):
            raise ValueError(f"task_names {self.task_names!r} repeat a name")
        self.prev_params = None                         # the snapshot for update_norm; validate() borrows it as its gradient sink
        self._val = None                                # validate()'s outputs and its two hvla_train_buffers, on first use
        if self.metrics:
            self._metrics_setup()

    def _metrics_setup(self):
        """The buffers of hvla_train_metrics: its output vector (NaN until a step fills a slot), its scratch, the snapshot of the
        parameters, and -- frozen encoder -- the sum of squares of the shared DINOv2 leaves that every sample's dict_base_params
        carries (scripts/train.py:384), once in float64 from the model's host tensors."""
        torch, dev = self.torch, self.model.device
        nt = len(self.task_names)
        self.metric_vec = torch.full((_native.HVLA_METRIC_N + 2 * nt,), float("nan"), dtype=torch.float32, device=dev)
        self.metric_reduced = None                      # info(reduce=True) under several ranks: the all-reduced copy
        self.metric_scratch = torch.empty(_native.HVLA_TRAIN_METRICS_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
        self.prev_params = torch.empty(self.n, dtype=torch.float32, device=dev)
        self.task_ids = None
        self.encoder_sqsum = 0.0
        if not self.train_encoder:
            self.encoder_sqsum = float(sum((np.asarray(self.model.params[shared_name(path)], np.float64) ** 2).sum()
                                           for path, _ in encoder_leaves(self.g)))
        self._last_lr = None

    def _metrics_call(self, select):
        """hvla_train_metrics on this step's buffers (always the micro-batch's own `grads`, also under gradient accumulation)."""
        tok, msk, cls, obs, tgt, am, tm = self._keep
        wa_on = "attention_alignment_loss" in self.aux_metrics
        self.model._ctx.train_metrics(
            self.buf, select, self.metric_vec.data_ptr(), self.B, self.train_encoder, self.metric_scratch.data_ptr(),
            prev_params_ptr=self.prev_params.data_ptr(), target_ptr=tgt.data_ptr(), tmask_ptr=tm.data_ptr(), amask_ptr=am.data_ptr(),
            task_ids_ptr=self.task_ids.data_ptr() if self.task_ids is not None else 0, n_tasks=len(self.task_names),
            entropy_ptr=self.aux_entropy.data_ptr() if self.aux_entropy is not None else 0,
            alignment_ptr=self.aux_alignment.data_ptr() if wa_on else 0, encoder_sqsum=self.encoder_sqsum, stream=self.model._stream())

    def _select(self, reference=None, attention=False):
        """What every call into the context starts with, in this order (the mask's length depends on the source); in front of a
        step (`attention`) also the attention terms, whose annealed alignment weight it returns."""
        self._select_language()
        self._select_source()
        self._select_frozen()
        self._select_noise()
        return self._select_attention(reference) if attention else None

    def _select_language(self):
        """Whether this tuner trains the policy with its language prefix (hvla_train_language_tokens; host-side like the others,
        and first: the entries below refuse a use_language_token context without it)."""
        self.model._ctx.train_language_tokens(self.language_tokens)
        self.model._ctx.train_differential(self.differential)
        self.model._ctx.train_layer_tokens(self.layer_tokens)

    def _select_source(self):
        """The context is the model's, shared by every FineTuner on it: each call into it first says which position table this
        one trains (hvla_train_position_source; a host-side setting, nothing is launched)."""
        self.model._ctx.train_position_source(self.source_n, self.interp_w.data_ptr() if self.source_n else 0)

    def _select_frozen(self):
        """... and which elements it leaves alone (hvla_train_frozen: the mask by pointer and the buckets frozen_plan found wholly
        frozen, or NULL; a host-side setting like the one above, after it because the mask's length depends on the source)."""
        if self.frozen is None:
            self.model._ctx.train_frozen(0, 0, 0)
        else:
            self.model._ctx.train_frozen(self.frozen.data_ptr(), self.frozen.numel(), self.frozen_buckets)

    def _select_noise(self):
        """... and which noise it trains with (hvla_train_noise_set, by value: the rates, the seed, this rank's first global sample
        index and the current draw; off for a FineTuner without noise).  In front of train_sizes too: the noisy copies of the tokens
        and the CLS rows live in the workspace."""
        if not self.noise_on:
            self.model._ctx.train_noise(off=True)
            return
        import torch.distributed as dist
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.model._ctx.train_noise(seed=self.noise_seed, sample_offset=rank * self.B, draw=self.noise_draw, **self.noise)

    def _select_attention(self, reference=None):
        """... and which attention terms its loss has (hvla_train_attention_losses; off for a FineTuner without them).  The alignment
        weight is annealed with this tuner's count of applied updates, the reference's `state.step`."""
        wa = alignment_weight(self.attention_map_alignment, self.step_count, self.num_steps)
        self.model._ctx.train_attention_losses(
            self.attention_entropy, wa, reference.data_ptr() if wa > 0 else 0,
            self.aux_entropy.data_ptr() if self.aux_entropy is not None else 0,
            self.aux_alignment.data_ptr() if wa > 0 else 0)
        return wa

    def _derive_slot(self, layout):
        """The baked slot of `params` becomes the device's own resize of the tail (bitwise what every later step and apply
        re-derives), after a check that the source really is the source of the table being served: the two may differ by the
        rounding of two four-tap float32 contractions evaluated in another order, not by more."""
        torch, g = self.torch, self.g
        at = {name: (off, int(np.prod(shape))) for name, off, shape in layout}
        (so, sn), (to, tn) = at[POSITION_LEAF], at[POSITION_SOURCE]
        self.slot, self.tail = slice(so, so + sn), slice(to, to + tn)
        served = self.params[self.slot].clone()
        self.model._ctx.position_interp(self.params[self.tail].data_ptr(), self.source_n, self.interp_w.data_ptr(),
                                        self.params[self.slot].data_ptr(), self.model._stream())
        w1 = float(self.interp_w.abs().sum(dim=0).max())
        bound = 2 * 14 * 2.0 ** -24 * w1 * w1 * float(self.params[self.tail].abs().max())
        worst = float((self.params[self.slot] - served).abs().max())
        if not worst <= bound:
            raise ValueError(
                f"model.position_table_source ({self.source_n} x {self.source_n}) is not the source of the served table "
                f"{POSITION_LEAF}: resized to {g.grid} x {g.grid} it differs from it by {worst:.3e}, the resize's own rounding "
                f"allows {bound:.3e}.  Pass the source these parameters were baked from, or accept_baked_position_table=True "
                "to train the served table itself (INTEGRATION.md)")

    def _bucket_setup(self):
        self.buckets = gradient_buckets(self.g, self.train_encoder, self.source_n)
        ranges = self.model._ctx.train_bucket_ranges(self.train_encoder)
        self._bucket_id = [ranges.index((off, n)) for _, off, n in self.buckets]   # the library's numbering (0 encoder, 1 heads, 2 context)
        self._comm = None

    def _buffers(self, grads):
        return _native.hvla_train_buffers(*[t.data_ptr() if t is not None else None for t in (
            self.params, grads, self.mu, self.nu, self.ema, self.theta, self.dtheta, self.work, self.loss,
            self.actions, self.logits, self.sqsum, self.wd_mask, self.params0)])

    def _hyper(self, lr, forward_only=False, base_lr=None, clip=None, ema=True):
        h = self.hy
        return _native.hvla_train_hyper(lr, h["b1"], h["b2"], h["eps"], h["weight_decay"], h["clip"] if clip is None else clip,
                                        h["ema_decay"] if ema else 0.0,
                                        self.step_count, int(forward_only), lr if base_lr is None else base_lr,
                                        h["base_weight_decay"], int(self.train_encoder))

    def forward_backward(self, instruction_dict, initial_state, tokens_or_images, batch, forward_only=False,
                         reference_attention=None, task_index=None):
        """loss [B] (device) after writing self.grads = d mean(loss) / d params.  The fourth argument is the frozen
        encoder's patch tokens f32 [B, P, E], or -- with train_encoder -- the uint8 observations [B, (1,) H, W, 3].
        `reference_attention` (device or host float32 [B, P]; needed iff attention_map_alignment > 0): the alignment term's target.
        `task_index` (metrics=True): {name: bool [B]} as the reference passes it (scripts/train.py:406, 455-456), names from `task_names`."""
        check_reference_attention(self.attention_map_alignment, reference_attention, self.B, self.g.patches)
        if task_index is not None and not self.metrics:
            raise ValueError("task_index feeds info()'s task_loss_<name>: it needs FineTuner(metrics=True, task_names=...)")
        ids = resolve_task_index(task_index, self.task_names, self.B) if self.metrics and self.task_names else None
        torch, m, g = self.torch, self.model, self.g
        li = instruction_dict["language_instruction"]
        if "token_embedding" not in li:                    # frozen T5 inside the step, as scripts/train.py:407-415
            li = m.encode_instructions(li)
        tok = m._dev(li["token_embedding"], torch.float32)
        msk = m._dev(li["attention_mask"], torch.int64)
        cls = m._dev(np.asarray(initial_state["patch_embeddings"])[:, 0], torch.float32)
        if self.train_encoder:
            img = tokens_or_images
            if not torch.is_tensor(img):
                img = np.asarray(img)
            if img.ndim == 5:
                img = img[:, 0]
            obs = m._dev(img, torch.uint8)
            assert tuple(obs.shape) == (self.B, g.image_size, g.image_size, 3), obs.shape
            tkn_ptr, img_ptr = None, obs.data_ptr()
        else:
            obs = m._dev(tokens_or_images, torch.float32)
            assert tuple(obs.shape) == (self.B, g.patches, g.enc_dim), obs.shape
            tkn_ptr, img_ptr = obs.data_ptr(), None
        tgt = m._dev(np.asarray(batch["action"])[:, 0], torch.float32)
        am = m._dev(np.asarray(batch["action_pad_mask"])[:, 0].astype(np.uint8), torch.uint8)
        tm = m._dev(np.asarray(batch["timestep_pad_mask"])[:, 0].astype(np.uint8), torch.uint8)
        assert tok.shape[0] == self.B
        ref = m._dev(reference_attention, torch.float32) if self.attention_map_alignment > 0 else None
        self._keep = (tok, msk, cls, obs, tgt, am, tm)
        self._keep_reference = ref
        if self.metrics:
            self.task_ids = m._dev(ids, torch.int32) if ids is not None else None
        ptrs = [tok.data_ptr(), msk.data_ptr(), cls.data_ptr(), tkn_ptr, img_ptr, tgt.data_ptr(), tm.data_ptr(), am.data_ptr()]
        if self.noise_on and not forward_only:
            self.noise_draw += 1                           # every differentiated step draws afresh (a forward-only one draws nothing)
        wa = self._select(ref, attention=True)
        m._ctx.train_step(self.buf, ptrs, self.B, self._hyper(0.0, forward_only), m._stream())
        self.aux_metrics = {}
        if self.attention_entropy > 0:
            self.aux_metrics["attention_entropy_loss"] = self.aux_entropy
        if wa > 0:
            self.aux_metrics["attention_alignment_loss"] = self.aux_alignment
        return self.loss

    def all_reduce_gradient(self, single_rank_too: bool = False):
        """`pmean(grads)` of scripts/train.py:460, bucketed: RCCL over xGMI, one all-reduce per gradient bucket, each
        enqueued on a communication stream that waits (on the device, hvla_train_wait_bucket) only for the event
        hvla_train_step recorded when that bucket became final -- the 343 MB DINOv2 bucket is on the links while the
        weight-generation and context-encoder backward still run.  Nothing here blocks the host; the compute stream
        waits for the reductions before the optimizer reads `grads`.  (`single_rank_too`: run the same path in a
        one-rank process group -- the tests' way of exercising the events and streams on a one-GPU box.)"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or single_rank_too)):
            return
        torch, m = self.torch, self.model
        world = dist.get_world_size()
        if self._comm is None:
            self._comm = torch.cuda.Stream(device=m.device)
        cur = torch.cuda.current_stream(m.device)
        works = []
        with torch.cuda.stream(self._comm):
            for i, (_, off, n) in enumerate(self.buckets):
                if self.frozen_buckets >> self._bucket_id[i] & 1:     # wholly frozen (frozen_keys): not computed, nobody reads it
                    continue
                m._ctx.train_wait_bucket(self._bucket_id[i], self._comm.cuda_stream)
                works.append(dist.all_reduce(self.grads[off:off + n], async_op=True))
            for w in works:
                w.wait()                                  # the communication stream waits for the collective
            self.grads /= world                           # ... and scales behind it
        cur.wait_stream(self._comm)

    def apply(self, lr=None, base_lr=None):
        """Gradient all-reduce, then the optimizer: chain(clip_by_global_norm, [MultiSteps](adamw)) and the EMA.  With
        grad_accumulation_steps = k the clipped gradient of every micro-batch goes into a running mean and parameters move
        on every k-th call only (optax.MultiSteps, octo/utils/train_utils.py:420-421); returns True when they moved.
        With metrics=True hvla_train_metrics runs twice round it: everything but update_norm after the all-reduce and before the
        optimizer (the reference logs param_norm of the parameters before the update), then the snapshot of `params`, the optimizer,
        and update_norm = |params - snapshot| (zero on a micro-step that moved nothing)."""
        self.all_reduce_gradient()
        if not self.metrics:
            return self._optimizer(lr, base_lr)
        self._select()
        self._metrics_call(_native.HVLA_METRICS_PRE)
        self.prev_params.copy_(self.params)
        self._last_lr = lr_rsqrt(self.step_count, self.peak_lr) if lr is None else lr
        moved = self._optimizer(lr, base_lr)
        self._metrics_call(_native.HVLA_METRICS_UPDATE)            # (the optimizer left the context's selection as it is)
        return moved

    def _optimizer(self, lr=None, base_lr=None):
        ctx, st = self.model._ctx, self.model._stream()
        self._select()
        if self.accum_k > 1:
            if self.micro == 0:
                self.acc.zero_()
            ctx.train_accumulate(self.buf, self.acc.data_ptr(), 1.0 / self.accum_k, self._hyper(0.0), st)
            self.micro += 1
            if self.micro < self.accum_k:
                return False
            self.micro = 0
        lr = lr_rsqrt(self.step_count, self.peak_lr) if lr is None else lr
        base_lr = lr_rsqrt(self.step_count, self.base_peak_lr) if base_lr is None else base_lr
        update = self.step_count + 1                   # scripts/train.py:679 current_update_step
        ema_on = update > self.ema_start_step
        if self.accum_k > 1:                           # the micro-gradients were clipped one by one
            ctx.train_apply(self.buf_acc, self._hyper(lr, base_lr=base_lr, clip=float("inf"), ema=ema_on), st)
        else:
            ctx.train_apply(self.buf, self._hyper(lr, base_lr=base_lr, ema=ema_on), st)
        if update == self.ema_start_step:              # scripts/train.py:682-688: the EMA starts as a copy
            self.ema.copy_(self.params)
        self.step_count += 1
        return True

    def step(self, instruction_dict, initial_state, images, batch, lr=None, base_lr=None, reference_attention=None, task_index=None):
        check_reference_attention(self.attention_map_alignment, reference_attention, self.B, self.g.patches)
        obs = images if self.train_encoder else self.model.encode_images(images)
        loss = self.forward_backward(instruction_dict, initial_state, obs, batch, reference_attention=reference_attention,
                                     task_index=task_index)
        self.apply(lr, base_lr)
        return loss.mean()

    def info(self, reduce: bool = True) -> Dict[str, object]:
        """The reference's `info` of the last step (scripts/train.py:506-529) under its key names (INFO_KEYS, `task_loss_<name>`):
        0-d device tensors, views into hvla_train_metrics' vector -- nothing synchronises until the caller reads one, and the next
        step overwrites them.  With a process group of more than one rank and `reduce`, the rank-local means and the task sums and
        counts are all-reduced first (reduce_info_vector: one collective, into a copy)."""
        if not self.metrics:
            raise RuntimeError("info() needs FineTuner(metrics=True)")
        import torch.distributed as dist
        vec = self.metric_vec
        if reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            if self.metric_reduced is None:
                self.metric_reduced = self.torch.empty_like(vec)
            self.metric_reduced.copy_(vec)
            vec = reduce_info_vector(self.metric_reduced, len(self.task_names), dist.get_world_size())
        lr = None if self._last_lr is None else self.torch.full((), float(self._last_lr), dtype=self.torch.float32, device=vec.device)
        return info_from_vector(vec, self.task_names, lr, self.attention_entropy > 0, self.attention_map_alignment > 0)

    def _validation_buffers(self):
        """validate()'s own outputs and its two hvla_train_buffers (params / the EMA).  A forward-only hvla_train_step still zeroes the
        vector `grads` points at: that is the snapshot vector of the metrics (free between two apply calls), so `self.grads` keeps
        its bits; a tuner without metrics gets that vector here, on the first validation."""
        if self._val is None:
            torch, dev = self.torch, self.model.device
            f32 = dict(dtype=torch.float32, device=dev)
            if self.prev_params is None:
                self.prev_params = torch.empty(self.n, **f32)
            out = dict(loss=torch.zeros(self.B, **f32), actions=torch.zeros(self.B, self.g.horizon, self.g.action_dim, **f32),
                       logits=torch.zeros(self.B, self.g.horizon, **f32), terms=torch.zeros(3, self.B, **f32))
            bufs = {}
            for ema, vec in ((False, self.params), (True, self.ema)):
                bufs[ema] = _native.hvla_train_buffers(*[t.data_ptr() if t is not None else None for t in (
                    vec, self.prev_params, self.mu, self.nu, None, self.theta, self.dtheta, self.work, out["loss"], out["actions"],
                    out["logits"], self.sqsum, self.wd_mask, self.params0)])
            self._val = (out, bufs)
        return self._val

    def validate(self, instruction_dict, initial_state, images, batch, ema: bool = False) -> Dict[str, object]:
        """The reference's `validation_action_loss` (scripts/train.py:546-583) on one batch: {"mse": 0-d device tensor} =
        mean((predicted - clip(action, -5, 5))^2) * action_dim over every sample, step and dimension, unmasked, the gripper column
        being the thresholded prediction.  A forward-only step on `params`, or with `ema` on their moving average (what the reference
        evaluates, data/simpler/evaluate.py:440-444), then hvla_loss_terms.  Writes no gradient, no optimizer state and no counter,
        and leaves `loss`, `actions`, `logits`, `aux_metrics` and the metrics of the last step alone (the attention terms are off
        for it: they are no part of the mse); `theta` and the workspace are shared with the step, so call it between steps, not
        between forward_backward and apply.  Arguments as `step`."""
        torch, m, g = self.torch, self.model, self.g
        out, bufs = self._validation_buffers()
        li = instruction_dict["language_instruction"]
        if "token_embedding" not in li:
            li = m.encode_instructions(li)
        tok = m._dev(li["token_embedding"], torch.float32)
        msk = m._dev(li["attention_mask"], torch.int64)
        cls = m._dev(np.asarray(initial_state["patch_embeddings"])[:, 0], torch.float32)
        if self.train_encoder:
            img = images if torch.is_tensor(images) else np.asarray(images)
            if img.ndim == 5:
                img = img[:, 0]
            obs = m._dev(img, torch.uint8)
            assert tuple(obs.shape) == (self.B, g.image_size, g.image_size, 3), obs.shape
            tkn_ptr, img_ptr = None, obs.data_ptr()
        else:
            obs = m.encode_images(images)
            assert tuple(obs.shape) == (self.B, g.patches, g.enc_dim), obs.shape
            tkn_ptr, img_ptr = obs.data_ptr(), None
        tgt = m._dev(np.asarray(batch["action"])[:, 0], torch.float32)
        am = m._dev(np.asarray(batch["action_pad_mask"])[:, 0].astype(np.uint8), torch.uint8)
        tm = m._dev(np.asarray(batch["timestep_pad_mask"])[:, 0].astype(np.uint8), torch.uint8)
        assert tok.shape[0] == self.B
        self._select_language()
        self._select_source()
        self._select_frozen()
        self._select_noise()                            # (the plan's offsets are the setting's; a forward-only step draws nothing)
        m._ctx.train_attention_losses()                 # off; the next step selects its own again
        ptrs = [tok.data_ptr(), msk.data_ptr(), cls.data_ptr(), tkn_ptr, img_ptr, tgt.data_ptr(), tm.data_ptr(), am.data_ptr()]
        m._ctx.train_step(bufs[bool(ema)], ptrs, self.B, self._hyper(0.0, True), m._stream())
        t = out["terms"]
        m._ctx.loss_terms(out["actions"].data_ptr(), out["logits"].data_ptr(), tgt.data_ptr(), tm.data_ptr(), am.data_ptr(),
                          t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), self.B, m._stream())
        return {"mse": (t[2].double().mean() / g.horizon).float()}

    def validate_batches(self, batches, ema: bool = False) -> Dict[str, object]:
        """`ValidationCallback`'s average over a validation set: `batches` yields (instruction_dict, initial_state, images, batch);
        the mean of validate()'s metrics over them, accumulated on the device (one tensor per key, read by the caller)."""
        total, count = {}, 0
        for instruction_dict, initial_state, images, batch in batches:
            for k, v in self.validate(instruction_dict, initial_state, images, batch, ema=ema).items():
                total[k] = v.double() if k not in total else total[k] + v.double()
            count += 1
        if not count:
            raise ValueError("validate_batches: no batch")
        return {k: (v / count).float() for k, v in total.items()}

    def publish(self, ema: bool = False, host_copy: bool = True, audit: bool = False):
        """Serve the fine-tuned weights in place (`hvla_train_publish`): the parameters, or with `ema` their moving average
        (the reference evaluates `model.replace(params=ema)`, data/simpler/evaluate.py:440-444), are packed on the device into
        the buffers the model's context serves from, on the model's stream.  The context stays the one it was: its language
        encoder, pooled arenas, `GeneratedWeights` and captured graphs remain valid; weights generated earlier keep their
        values, `create_tasks` / `assign_tasks` from now on use the new ones.  The image encoder is rewritten only when this
        FineTuner trains it.

        `host_copy=True` also replaces `model.params` by the published tensors (encoder leaves that were not trained are
        kept), so that `save_pretrained` writes what is being served.  With `host_copy=False` nothing leaves the device and
        `model.params` / `save_pretrained` raise until a later `publish(host_copy=True)`.
        When the position table is trained through its interpolation (the model has a `position_table_source`), the served table is
        baked on the device from the published vector's source, and `host_copy=True` updates `model.position_table_source` too;
        after training the baked table itself (`accept_baked_position_table=True`) it sets it to None.
        `audit=True` runs `model.audit_operand_range()` afterwards: a trained encoder is where fp16 operands can leave their
        range; it returns that audit's result, otherwise None."""
        m = self.model
        vec = self.ema if ema else self.params
        self._select()
        if self.source_n:                          # the slot the host copy reads is the resize of the tail being published, whatever
            m._ctx.position_interp(vec[self.tail].data_ptr(), self.source_n, self.interp_w.data_ptr(),     # was done to the vector
                                   vec[self.slot].data_ptr(), m._stream())
        m._ctx.train_publish(vec.data_ptr(), self.n, self.train_encoder, m._stream())
        if host_copy:
            new = dict(m._params)
            got = unpack_params(self.g, vec.cpu().numpy(), self.train_encoder, self.source_n)
            if self.source_n:                      # the trained source goes with the table that was baked from it
                got, m.position_table_source = got
            elif self._drops_source:               # the baked table was trained on its own: the source is stale
                m.position_table_source = None
            new.update(got)
            m.params = new
        else:
            m._params_stale = True
        return m.audit_operand_range() if audit else None
