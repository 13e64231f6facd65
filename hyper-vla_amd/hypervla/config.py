"""Static configuration + base-network metadata for the HyperVLA action-prediction path.

The reference keeps every model hyper-parameter in ``config.json`` (hypervla/model.py:152-163) and
derives the generated-leaf metadata in ``HyperVLA.init_base_net`` (hypervla/model.py:370-515).  This
module restates the README run's effective values (README.md:33-61) and the leaf list
the hypernetwork generates: 73 leaves, G = 201 500 parameters per episode for
E = 768.

Nothing here touches the GPU; it is pure host metadata shared by the product path, the tests and
the synthetic generators.
"""
from __future__ import annotations

import copy
import re
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np


# --------------------------------------------------------------------------------------
# Geometry of the path (all sizes are parameters so a tiny config can exercise every branch)
# --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Geometry:
    # frozen image encoder (HF Dinov2, reference: "facebook/dinov2-base", base_vit.py:76)
    image_size: int = 224
    patch: int = 14
    enc_dim: int = 768          # E
    enc_layers: int = 12
    enc_heads: int = 12
    enc_mlp: int = 3072
    # generated policy ("vit_t": README.md:47-50)
    dim: int = 64               # D
    layers: int = 4             # L
    heads: int = 4              # H
    mlp: int = 128              # M
    horizon: int = 4            # action_horizon
    action_dim: int = 7
    tanh_scale: float = 5.0
    max_action: float = 5.0
    clip_target: bool = True    # MixActionHead.loss clips the action target to +-max_action (action_heads.py:499-500)
    # hypernetwork (README.md:33-44)
    ctx_dim: int = 128          # C
    ctx_layers: int = 6
    ctx_heads: int = 4
    ctx_mlp: int = 512
    lang_tokens: int = 32       # T5 max_length (hypervla_pretrain_config.py:302-312)
    lang_dim: int = 768         # T5-base hidden size
    scale_context: bool = True
    # base_net_kwargs.vit_kwargs.use_language_token (base_vit.py:159-166,207-212): the T5 token embeddings, projected to D,
    # lead the policy's sequence [T language | P patches | 1 action]; language queries see only language keys
    lang_in_policy: bool = False
    # base_net_kwargs.vit_kwargs.return_attention_map (transformer.py:172-181): the block's attention is
    # CustomMultiHeadDotProductAttention, which hands the boolean mask to dot_product_attention_weights as `bias=`
    # (multi_head_attetion.py:88-98): 1 is added to every allowed score and nothing is masked
    mask_as_bias: bool = False
    # base_net_kwargs.vit_kwargs.use_differential_transformer (transformer.py:166-171): the block's attention is DifferentialAttention
    # (differential_transformer.py:99-252): per head two softmaxes over the halves of q / k with the mask added to the unscaled scores,
    # (A1 - lambda A2) V, an RMSNorm over the head's values; bias-free projections.  Served, not fine-tuned
    differential: bool = False
    # hypernet_kwargs.share_layer_index=False (model.py:400-436): the context encoder carries one layer token per module of the
    # policy and every generated leaf reads the token of its module.  Served, not fine-tuned
    layer_tokens: bool = False
    # hypernet_kwargs.share_TF_output_head (hypernetwork.py:221-225): one set of output heads serves every policy block, the
    # blocks differ through their tokens alone -- so only with layer_tokens
    shared_block_heads: bool = False

    def __post_init__(self):
        if self.shared_block_heads and not self.layer_tokens:
            raise ValueError("Geometry(shared_block_heads=True, layer_tokens=False): with share_TF_output_head and one shared layer "
                             "token every policy block would receive the same weights")
        if self.differential and self.lang_in_policy:
            raise ValueError("use_differential_transformer together with use_language_token is not built: DifferentialAttention adds "
                             "the mask as a bias, so language queries attend to patch keys and the language prefix is no per-episode "
                             "constant")
        if self.differential and self.mask_as_bias:
            raise ValueError("Geometry(differential=True, mask_as_bias=True): with use_differential_transformer the block never reaches "
                             "the return_attention_map branch (transformer.py:166-172); the one form is differential=True alone")
        if self.mask_as_bias and self.lang_in_policy:
            raise ValueError("return_attention_map together with use_language_token is not built: with the mask added as a bias "
                             "language queries attend to patch keys, so the language prefix is no per-episode constant")

    @property
    def attention_name(self) -> str:   # flax auto-name of the policy blocks' attention module
        if self.differential:
            return "DifferentialAttention_0"
        return "CustomMultiHeadDotProductAttention_0" if self.mask_as_bias else "MultiHeadDotProductAttention_0"

    @property
    def grid(self) -> int:
        return self.image_size // self.patch

    @property
    def patches(self) -> int:      # P
        return self.grid * self.grid

    @property
    def seq(self) -> int:          # S = patches + 1 action token (policy) / + CLS (encoder)
        return self.patches + 1

    @property
    def policy_seq(self) -> int:   # rows of the policy's pos_embedding: [T language if lang_in_policy | P patches | 1 action]
        return self.seq + (self.lang_tokens if self.lang_in_policy else 0)

    @property
    def num_layer_tokens(self) -> int:   # NL: rows of layer_pos_embedding, and of the context embedding [B, NL, C]
        return len(layer_token_modules(self)) if self.layer_tokens else 1

    @property
    def ctx_seq(self) -> int:      # language tokens + initial-image CLS + NL layer tokens
        return self.lang_tokens + 1 + self.num_layer_tokens

    @property
    def head_dim(self) -> int:
        return self.dim // self.heads

    @property
    def patch_in(self) -> int:     # 14*14*3
        return self.patch * self.patch * 3


FULL = Geometry()
# DINOv2-small token width named by BASELINE.json config 2 (policy-only variant)
SMALL_E = Geometry(enc_dim=384, enc_heads=6, enc_mlp=1536)
# Reduced geometry inside the HIP kernels' specialisation (P % 32 == 0, encoder head_dim 64, policy
# 64-d / 4 heads): fast full-tensor GPU parity runs against the live oracle
MID = Geometry(image_size=112, patch=14, enc_dim=128, enc_layers=2, enc_heads=2, enc_mlp=512,
               layers=2, ctx_layers=2, ctx_mlp=256, lang_tokens=12, lang_dim=64)
# A tiny geometry that still walks every code path (used for exhaustive intermediate fixtures)
TINY = Geometry(image_size=56, patch=14, enc_dim=32, enc_layers=2, enc_heads=2, enc_mlp=64,
                dim=16, layers=2, heads=2, mlp=32, ctx_dim=16, ctx_layers=2, ctx_heads=2, ctx_mlp=32,
                lang_tokens=8, lang_dim=24)


# --------------------------------------------------------------------------------------
# Generated-leaf metadata  (reference: init_base_net, hypervla/model.py:370-515)
# --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class T5Geometry:
    """Frozen instruction encoder (``LanguageTokenizer('t5-base')``, data/utils/language_tokenizer.py:9-28;
    octo/model/components/tokenizers.py:186-211): HF ``T5Config`` fields of "t5-base"."""
    vocab: int = 32128
    d_model: int = 768
    d_kv: int = 64
    heads: int = 12
    d_ff: int = 3072
    layers: int = 12
    buckets: int = 32            # relative_attention_num_buckets
    max_distance: int = 128      # relative_attention_max_distance
    eps: float = 1e-6

    @property
    def inner(self) -> int:
        return self.heads * self.d_kv


T5_BASE = T5Geometry()
T5_TINY = T5Geometry(vocab=300, d_model=32, d_kv=8, heads=2, d_ff=64, layers=2)      # pairs with TINY (lang_dim 32)
T5_MID = T5Geometry(vocab=1000, d_model=768, d_kv=64, heads=12, d_ff=3072, layers=2)  # full widths, 2 layers (tests)


def t5_param_shapes(t: T5Geometry) -> Dict[str, Tuple[int, ...]]:
    """FlaxT5EncoderModel parameter tree, '/'-joined (kernels are [in, out])."""
    s: Dict[str, Tuple[int, ...]] = {"shared/embedding": (t.vocab, t.d_model)}
    for i in range(t.layers):
        b = f"encoder/block/{i}/layer/"
        for nm in ("q", "k", "v"):
            s[b + f"0/SelfAttention/{nm}/kernel"] = (t.d_model, t.inner)
        s[b + "0/SelfAttention/o/kernel"] = (t.inner, t.d_model)
        s[b + "0/layer_norm/weight"] = (t.d_model,)
        s[b + "1/DenseReluDense/wi/kernel"] = (t.d_model, t.d_ff)
        s[b + "1/DenseReluDense/wo/kernel"] = (t.d_ff, t.d_model)
        s[b + "1/layer_norm/weight"] = (t.d_model,)
    s["encoder/block/0/layer/0/SelfAttention/relative_attention_bias/embedding"] = (t.buckets, t.heads)
    s["encoder/final_layer_norm/weight"] = (t.d_model,)
    return s


@dataclass(frozen=True)
class Leaf:
    path: Tuple[str, ...]       # base-net pytree path
    shape: Tuple[int, ...]
    offset: int                 # offset into the per-episode flat parameter vector (reference order)

    @property
    def size(self) -> int:
        return int(np.prod(self.shape))

    @property
    def flat_name(self) -> str:     # hypervla/model.py:532-540 (flatten_dict, sep='_')
        return "_".join(self.path)

    @property
    def head_name(self) -> str:     # flax auto-name of the per-leaf Dense: hypernetwork.py:65-67
        return "output_head_" + self.flat_name

    @property
    def shared_head_name(self) -> str:   # share_TF_output_head: the head of this leaf's name in any block (hypernetwork.py:221-225)
        return re.sub(r"encoderblock_\d+", "encoderblock", self.head_name)


def layer_token_modules(g: "Geometry") -> List[Tuple[str, ...]]:
    """THE layer-token table of ``share_layer_index=False`` with ``encoder_type="DINOv2"`` (model.py:418-436): the module each
    token index stands for, as a path prefix of its leaves.  Index 0 is the shared image encoder, which is not generated
    (``layer_token_mask[0] = False``); then the modules of ``encoder/Transformer_0``, the remaining ``encoder`` modules, and
    ``action_head``.  The reference walks dicts that ``jax.tree_map`` rebuilt, whose keys are SORTED AS STRINGS -- the assumption
    `generated_leaves` already rests on -- so ``encoderblock_10`` comes before ``encoderblock_2``.  The table does
    not depend on `g.layer_tokens`: it is what the flag switches on."""
    T = ("encoder", "Transformer_0")
    mods = [("encoder", "image_encoder")]
    mods += [T + (m,) for m in sorted(["encoder_norm"] + [f"encoderblock_{l}" for l in range(g.layers)])]
    mods += [("encoder", m) for m in sorted(["image_embedding_projection", "pos_embedding"] +
                                            (["language_token_projection"] if g.lang_in_policy else []))]
    return mods + [("action_head",)]


def token_of(g: "Geometry", leaf) -> int:
    """The layer-token index a generated leaf (a `Leaf` or its path) reads under ``layer_tokens``: that of the module its path
    begins with.  Never 0."""
    path = tuple(leaf.path if isinstance(leaf, Leaf) else leaf)
    for i, m in enumerate(layer_token_modules(g)):
        if path[:len(m)] == m:
            return i
    raise ValueError(f"leaf {'/'.join(path)} belongs to no module of the layer-token table")


def generated_leaves(g: Geometry) -> List[Leaf]:
    """The 73 HN-generated leaves in jax pytree order (dict keys sorted at every level); 75 with ``lang_in_policy``, which adds
    ``encoder/language_token_projection`` (base_vit.py:162-165) between the image projection and the position embedding.  With
    ``mask_as_bias`` the eight attention leaves of a block are named ``CustomMultiHeadDotProductAttention_0`` and lead the block.
    With ``differential`` a block's attention has nine leaves under ``DifferentialAttention_0``, which leads the block too: four
    bias-free [D, D] projections, the four lambda vectors [D / (2 H)] and ``subln/weight`` [D / H] (differential_transformer.py:139-156):
    77 leaves, G = 200 668 at the README geometry.

    ``shared_modules=("image_encoder",)`` removes the DINOv2 leaves (hypervla/model.py:439-451);
    ``share_layer_index=True`` makes every leaf read context token 0 (model.py:400-402).
    """
    D, M, H, hd, E = g.dim, g.mlp, g.heads, g.head_dim, g.enc_dim
    A = g.horizon * (g.action_dim - 1)
    items: List[Tuple[Tuple[str, ...], Tuple[int, ...]]] = []
    items += [(("action_head", "continuous_head", "bias"), (A,)),
              (("action_head", "continuous_head", "kernel"), (D, A)),
              (("action_head", "discrete_head", "bias"), (g.horizon,)),
              (("action_head", "discrete_head", "kernel"), (D, g.horizon))]
    T = ("encoder", "Transformer_0")
    items += [(T + ("encoder_norm", "bias"), (D,)), (T + ("encoder_norm", "scale"), (D,))]
    for l in range(g.layers):
        B = T + (f"encoderblock_{l}",)
        rest = [(B + ("LayerNorm_0", "bias"), (D,)), (B + ("LayerNorm_0", "scale"), (D,)),
                (B + ("LayerNorm_1", "bias"), (D,)), (B + ("LayerNorm_1", "scale"), (D,)),
                (B + ("MlpBlock_0", "Dense_0", "bias"), (M,)),
                (B + ("MlpBlock_0", "Dense_0", "kernel"), (D, M)),
                (B + ("MlpBlock_0", "Dense_1", "bias"), (D,)),
                (B + ("MlpBlock_0", "Dense_1", "kernel"), (M, D))]
        A_ = B + (g.attention_name,)
        attn = [(A_ + ("key", "bias"), (H, hd)), (A_ + ("key", "kernel"), (D, H, hd)),
                (A_ + ("out", "bias"), (D,)), (A_ + ("out", "kernel"), (H, hd, D)),
                (A_ + ("query", "bias"), (H, hd)), (A_ + ("query", "kernel"), (D, H, hd)),
                (A_ + ("value", "bias"), (H, hd)), (A_ + ("value", "kernel"), (D, H, hd))]
        if g.differential:      # sorted keys again; "DifferentialAttention_0" comes before "LayerNorm_0"
            attn = [(A_ + ("k_proj", "kernel"), (D, D)),
                    (A_ + ("lambda_k1",), (hd // 2,)), (A_ + ("lambda_k2",), (hd // 2,)),
                    (A_ + ("lambda_q1",), (hd // 2,)), (A_ + ("lambda_q2",), (hd // 2,)),
                    (A_ + ("out_proj", "kernel"), (D, D)), (A_ + ("q_proj", "kernel"), (D, D)),
                    (A_ + ("subln", "weight"), (hd,)), (A_ + ("v_proj", "kernel"), (D, D))]
        # sorted keys: "CustomMultiHead..." comes before "LayerNorm_0", "MultiHead..." after "MlpBlock_0"
        items += attn + rest if (g.mask_as_bias or g.differential) else rest + attn
    items += [(("encoder", "image_embedding_projection", "bias"), (D,)),
              (("encoder", "image_embedding_projection", "kernel"), (E, D))]
    if g.lang_in_policy:
        items += [(("encoder", "language_token_projection", "bias"), (D,)),
                  (("encoder", "language_token_projection", "kernel"), (g.lang_dim, D))]
    items += [(("encoder", "pos_embedding"), (1, g.policy_seq, D))]
    leaves, off = [], 0
    for path, shape in items:
        leaves.append(Leaf(path, tuple(shape), off))
        off += int(np.prod(shape))
    return leaves


def total_generated(g: Geometry) -> int:
    lv = generated_leaves(g)
    return lv[-1].offset + lv[-1].size


assert total_generated(FULL) == 201_500 and len(generated_leaves(FULL)) == 73
# use_differential_transformer: per block - 4 biases (4 D) + 4 lambda vectors (4 D / (2 H)) + subln/weight (D / H) = - 208, + 1 leaf
assert total_generated(Geometry(differential=True)) == 200_668 and len(generated_leaves(Geometry(differential=True))) == 77


def pytree_from_theta(g: Geometry, theta, squeeze: bool = False) -> Dict:
    """theta [B, G] (reference leaf order, what `GeneratedWeights.export` returns) -> the reference's nested ``base_params`` dict of
    the generated leaves, each [B, *shape] (``squeeze``: episode 0 alone, [*shape], as the reference's create_tasks squeezes B == 1)."""
    theta = np.asarray(theta)
    G = total_generated(g)
    if theta.ndim != 2 or theta.shape[1] != G:
        raise ValueError(f"theta must be [B, {G}], got {theta.shape}")
    tree: Dict = {}
    for lf in generated_leaves(g):
        v = theta[:, lf.offset:lf.offset + lf.size].reshape((theta.shape[0],) + lf.shape)
        if squeeze:
            v = v[0]
        node = tree
        for key in lf.path[:-1]:
            node = node.setdefault(key, {})
        node[lf.path[-1]] = v
    return tree


def theta_from_pytree(g: Geometry, tree: Dict) -> np.ndarray:
    """The inverse of :func:`pytree_from_theta`: a nested ``base_params`` dict -> float32 [B, G].  Leaves are [B, *shape], or
    [*shape] throughout for one episode.  An ``encoder/image_encoder`` subtree -- the shared DINOv2 leaves the reference broadcasts
    into ``base_params`` (hypernetwork.py:233), of which the device holds one copy -- is ignored.  A missing leaf raises KeyError,
    an unknown one ValueError, a wrong shape ValueError, each naming the leaf's path."""
    leaves = generated_leaves(g)
    known = {lf.path for lf in leaves}

    def walk(node, path):
        for key, v in node.items():
            p = path + (key,)
            if p == ("encoder", "image_encoder"):
                continue
            if isinstance(v, dict):
                walk(v, p)
            elif p not in known:
                raise ValueError(f"unknown leaf {'/'.join(p)}: not one of the {len(leaves)} generated leaves of this geometry")

    walk(tree, ())
    cols, B = [], None
    for lf in leaves:
        node, name = tree, "/".join(lf.path)
        for key in lf.path:
            if not isinstance(node, dict) or key not in node:
                raise KeyError(f"missing leaf {name}")
            node = node[key]
        if isinstance(node, dict):
            raise ValueError(f"leaf {name} is a subtree, expected an array of shape {('B',) + lf.shape}")
        v = np.asarray(node)
        if v.shape == lf.shape and B in (None, 0):
            B, v = 0, v[None]                        # the single-episode form
        elif v.ndim == len(lf.shape) + 1 and v.shape[1:] == lf.shape and B in (None, v.shape[0]) and v.shape[0] >= 1:
            B = v.shape[0]
        else:
            want = lf.shape if B == 0 else (("B" if B is None else B),) + lf.shape
            raise ValueError(f"leaf {name} has shape {v.shape}, expected {want}")
        cols.append(v.reshape(v.shape[0], -1).astype(np.float32, copy=False))
    return np.ascontiguousarray(np.concatenate(cols, 1))


# --------------------------------------------------------------------------------------
# config.json the evaluators read (data/utils/hypervla_interface.py:76-87, model.py:152-163)
# --------------------------------------------------------------------------------------
def default_config(g: Geometry = FULL, dataset_name: str = "bridge_dataset") -> Dict:
    cfg = dict(
        window_size=1,
        dataset_kwargs=dict(
            dataset_kwargs_list=[
                dict(name="bridge_dataset", action_proprio_normalization_type="normal"),
                dict(name="fractal20220817_data", action_proprio_normalization_type="normal"),
                dict(name="libero", action_proprio_normalization_type="normal"),
            ],
            frame_transform_kwargs=dict(resize_size=dict(primary=(g.image_size, g.image_size))),
            batch_size=256,
        ),
        text_processor=dict(kwargs=dict(
            tokenizer_name="t5-base",
            tokenizer_kwargs=dict(max_length=g.lang_tokens, padding="max_length", truncation=True,
                                  return_tensors="np"))),
        hypernet_kwargs=dict(
            encoder_type="transformer", context_embedding_dim=g.ctx_dim,
            context_encoder_kwargs=dict(num_layers=g.ctx_layers, mlp_dim=g.ctx_mlp,
                                        num_attention_heads=g.ctx_heads, dropout_rate=0.0,
                                        attention_dropout_rate=0.0, add_position_embedding=False),
            attend_to_padding=False, task_attend_to_layer=False, embedding_dropout_rate=0.0,
            scale_context_embedding=g.scale_context, output_head_bias=True,
            generation_strategy="block", shared_modules=("image_encoder",),
            include_goal_image=False, use_initial_image=True, use_all_image_tokens=False,
            share_TF_output_head=bool(g.shared_block_heads), init_strategy=0, share_all_params=False,
            share_layer_index=not g.layer_tokens, image_dropout=0.0),
        base_net_kwargs=dict(
            model_type="vit", action_head_type="mix", action_horizon=g.horizon,
            action_dim=g.action_dim,
            vit_kwargs=dict(encoder_type="DINOv2", patch_size=16, hidden_dim=g.dim,
                            num_layers=g.layers, num_heads=g.heads, mlp_dim=g.mlp,
                            dropout_rate=0.0, use_language_token=bool(g.lang_in_policy),
                            fine_tune_pretrained_image_encoder=True, image_embedding_noise=0.0,
                            use_differential_transformer=bool(g.differential), return_attention_map=bool(g.mask_as_bias),
                            add_positional_embedding=True, include_class_token=False),
            action_head_kwargs=dict(token_per_horizon=False, squash_continuous_action=True,
                                    tanh_scaling_factor=g.tanh_scale, clip_target=g.clip_target,
                                    max_action=g.max_action, hidden_dims=())),
        geometry=dict(image_size=g.image_size, patch=g.patch, enc_dim=g.enc_dim,
                      enc_layers=g.enc_layers, enc_heads=g.enc_heads, enc_mlp=g.enc_mlp,
                      lang_tokens=g.lang_tokens, lang_dim=g.lang_dim, layer_tokens=bool(g.layer_tokens)),
    )
    return copy.deepcopy(cfg)


def geometry_from_config(cfg: Dict) -> Geometry:
    """Inverse of :func:`default_config` (rejects branches the path does not build).

    ``use_differential_transformer`` selects ``Geometry.differential``.  A config with both ``use_differential_transformer`` and
    ``return_attention_map`` maps to ``differential=True, mask_as_bias=False``: Encoder1DBlock tests the first flag first
    (transformer.py:166-172), so such a model runs DifferentialAttention and never builds CustomMultiHeadDotProductAttention."""
    b, h = cfg["base_net_kwargs"], cfg["hypernet_kwargs"]
    v, a = b["vit_kwargs"], b["action_head_kwargs"]
    ge = cfg.get("geometry", {})
    if b["model_type"] != "vit" or b["action_head_type"] != "mix" or v["encoder_type"] != "DINOv2":
        raise ValueError("only model_type=vit / encoder_type=DINOv2 / action_head_type=mix is built "
                         "(README.md:45-56); got %r/%r/%r" % (b["model_type"], v["encoder_type"],
                                                              b["action_head_type"]))
    # share_layer_index: `geometry.layer_tokens`, which default_config and convert_checkpoint write, must say the same; a raw
    # reference config has no such key and share_layer_index decides alone
    layer_tokens = not bool(h.get("share_layer_index", False))
    if "layer_tokens" in ge and bool(ge["layer_tokens"]) != layer_tokens:
        raise ValueError(f"hypernet_kwargs.share_layer_index={h.get('share_layer_index')!r} contradicts geometry.layer_tokens="
                         f"{ge['layer_tokens']!r}: geometry.layer_tokens must equal not share_layer_index")
    shared_block_heads = bool(h.get("share_TF_output_head", False))
    if shared_block_heads and not layer_tokens:
        raise ValueError("hypernet_kwargs.share_TF_output_head=True with share_layer_index=True: every policy block would receive "
                         "the same weights")
    for key, want in (("generation_strategy", "block"),
                      ("use_initial_image", True), ("use_all_image_tokens", False),
                      ("attend_to_padding", False), ("task_attend_to_layer", False)):
        if h.get(key) != want:
            raise ValueError(f"hypernet_kwargs.{key}={h.get(key)!r} is outside the built path "
                             f"(README.md:33-44 uses {want!r})")
    if a.get("token_per_horizon") or a.get("hidden_dims"):
        raise ValueError("token_per_horizon / hidden_dims action heads are not built")
    lang_in_policy = bool(v.get("use_language_token", False))
    differential = bool(v.get("use_differential_transformer", False))
    mask_as_bias = bool(v.get("return_attention_map", False)) and not differential
    if differential and lang_in_policy:
        raise ValueError("base_net_kwargs.vit_kwargs.use_differential_transformer together with use_language_token is not built: "
                         "DifferentialAttention adds the mask as a bias (differential_transformer.py:219-221), so language queries "
                         "attend to patch keys and the language prefix is no per-episode constant")
    if mask_as_bias and lang_in_policy:
        raise ValueError("base_net_kwargs.vit_kwargs.return_attention_map together with use_language_token is not built: "
                         "CustomMultiHeadDotProductAttention adds the mask as a bias (multi_head_attetion.py:88-98), so language "
                         "queries attend to patch keys and the language prefix is no per-episode constant")
    for key, want in (("include_class_token", False), ("add_positional_embedding", True)):
        if bool(v.get(key, want)) != want:
            raise ValueError(f"base_net_kwargs.vit_kwargs.{key}={v.get(key)!r} is outside the built path (only {want!r} is built)")
    if b.get("action_token_num", 1) != 1 or v.get("action_token_num", 1) != 1:
        raise ValueError("action_token_num != 1 is not built: the policy kernels run exactly one action token")
    if lang_in_policy and ge.get("lang_tokens", 32) > 32:
        raise ValueError(f"use_language_token with lang_tokens={ge.get('lang_tokens')} is not built: the language prefix must fit "
                         "one 32-key tile of the policy kernel")
    if not a.get("squash_continuous_action", True):
        raise ValueError("squash_continuous_action=False is not built: the mix head kernels apply tanh(x / s) * max_action "
                         "(action_heads.py:469-470)")
    ce = h["context_encoder_kwargs"]
    return Geometry(
        image_size=ge.get("image_size", 224), patch=ge.get("patch", 14),
        enc_dim=ge.get("enc_dim", 768), enc_layers=ge.get("enc_layers", 12),
        enc_heads=ge.get("enc_heads", 12), enc_mlp=ge.get("enc_mlp", 3072),
        dim=v["hidden_dim"], layers=v["num_layers"], heads=v["num_heads"], mlp=v["mlp_dim"],
        horizon=b["action_horizon"], action_dim=b["action_dim"],
        tanh_scale=a.get("tanh_scaling_factor", 5.0), max_action=a.get("max_action", 5.0),
        clip_target=bool(a.get("clip_target", True)),                  # action_heads.py:408 default True
        ctx_dim=h["context_embedding_dim"], ctx_layers=ce["num_layers"],
        ctx_heads=ce["num_attention_heads"], ctx_mlp=ce["mlp_dim"],
        lang_tokens=ge.get("lang_tokens", 32), lang_dim=ge.get("lang_dim", 768),
        scale_context=bool(h.get("scale_context_embedding", False)), lang_in_policy=lang_in_policy, mask_as_bias=mask_as_bias,
        differential=differential, layer_tokens=layer_tokens, shared_block_heads=shared_block_heads)


# --------------------------------------------------------------------------------------
# Shared (not generated) leaves: the DINOv2 image encoder inside the base net
# (transformers FlaxDinov2Module param tree).  In the HN checkpoint each is a
# flat vector named "encoder_image_encoder_<path joined by _>" (hypernetwork.py:88-97).
# --------------------------------------------------------------------------------------
def encoder_leaves(g: Geometry) -> List[Tuple[Tuple[str, ...], Tuple[int, ...]]]:
    E, F, p = g.enc_dim, g.enc_mlp, g.patch
    out: List[Tuple[Tuple[str, ...], Tuple[int, ...]]] = [
        (("embeddings", "cls_token"), (1, 1, E)),
        (("embeddings", "mask_token"), (1, E)),
        (("embeddings", "patch_embeddings", "projection", "bias"), (E,)),
        (("embeddings", "patch_embeddings", "projection", "kernel"), (p, p, 3, E)),
        # baked to the run-time grid at conversion time (never interpolated on device)
        (("embeddings", "position_embeddings"), (1, g.patches + 1, E)),
    ]
    for i in range(g.enc_layers):
        L = ("encoder", "layer", str(i))
        for nm in ("key", "query", "value"):
            out += [(L + ("attention", "attention", nm, "bias"), (E,)),
                    (L + ("attention", "attention", nm, "kernel"), (E, E))]
        out += [(L + ("attention", "output", "dense", "bias"), (E,)),
                (L + ("attention", "output", "dense", "kernel"), (E, E)),
                (L + ("layer_scale1", "lambda1"), (E,)),
                (L + ("layer_scale2", "lambda1"), (E,)),
                (L + ("mlp", "fc1", "bias"), (F,)), (L + ("mlp", "fc1", "kernel"), (E, F)),
                (L + ("mlp", "fc2", "bias"), (E,)), (L + ("mlp", "fc2", "kernel"), (F, E)),
                (L + ("norm1", "bias"), (E,)), (L + ("norm1", "scale"), (E,)),
                (L + ("norm2", "bias"), (E,)), (L + ("norm2", "scale"), (E,))]
    out += [(("layernorm", "bias"), (E,)), (("layernorm", "scale"), (E,))]
    return out


def shared_name(path: Tuple[str, ...]) -> str:
    return "encoder_image_encoder_" + "_".join(path)


def hypernet_param_shapes(g: Geometry) -> Dict[str, Tuple[int, ...]]:
    """Every tensor of the HN checkpoint, keyed by '/'-joined flax path."""
    C, Hc, hc = g.ctx_dim, g.ctx_heads, g.ctx_dim // g.ctx_heads
    s: Dict[str, Tuple[int, ...]] = {
        "task_token_projection/kernel": (g.lang_dim, C), "task_token_projection/bias": (C,),
        "initial_image_projection/kernel": (g.enc_dim, C), "initial_image_projection/bias": (C,),
        "task_pos_embedding": (1, g.lang_tokens, C),
        "initial_image_pos_embedding": (1, 1, C),
        "layer_pos_embedding": (1, g.num_layer_tokens, C),
    }
    for l in range(g.ctx_layers):
        b = f"Transformer_0/encoderblock_{l}/"
        for ln in ("LayerNorm_0", "LayerNorm_1"):
            s[b + ln + "/scale"] = (C,)
            s[b + ln + "/bias"] = (C,)
        a = b + "MultiHeadDotProductAttention_0/"
        for nm in ("query", "key", "value"):
            s[a + nm + "/kernel"] = (C, Hc, hc)
            s[a + nm + "/bias"] = (Hc, hc)
        s[a + "out/kernel"] = (Hc, hc, C)
        s[a + "out/bias"] = (C,)
        s[b + "MlpBlock_0/Dense_0/kernel"] = (C, g.ctx_mlp)
        s[b + "MlpBlock_0/Dense_0/bias"] = (g.ctx_mlp,)
        s[b + "MlpBlock_0/Dense_1/kernel"] = (g.ctx_mlp, C)
        s[b + "MlpBlock_0/Dense_1/bias"] = (C,)
    s["Transformer_0/encoder_norm/scale"] = (C,)
    s["Transformer_0/encoder_norm/bias"] = (C,)
    for lf in generated_leaves(g):       # shared_block_heads: the blocks' leaves of one name collapse onto one head
        head = lf.shared_head_name if g.shared_block_heads else lf.head_name
        s[head + "/kernel"] = (C, lf.size)
        s[head + "/bias"] = (lf.size,)
    for path, shape in encoder_leaves(g):
        s[shared_name(path)] = (int(np.prod(shape)),)
    return s
