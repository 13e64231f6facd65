"""Float64 restatement of the generated policy with ``vit_kwargs.use_language_token`` (test infrastructure, like oracle/).

Built from the unchanged pieces of ``oracle/hvla_ref_np.py`` (``dense``, ``transformer`` with an explicit mask,
``generate_base_params`` over the extended leaf list, ``context_embedding``, ``dinov2``).  What the option adds
(reference ``hypervla/components/base_vit.py:159-227``):
  * :159-166  the T5 token embeddings [T, lang_dim] -- every position, padding included: nothing masks them in the base
    net -- through ``Dense(D)`` named ``language_token_projection``, prepended to the patch tokens;
  * :182-204  one zero action token appended, ``pos_embedding`` of T + P + 1 rows added;
  * :207-214  the mask: language queries see only language keys, no query but the action token's sees the action key.
With the flag off every function here is ``oracle.hvla_ref_np``'s operation for operation (same bits).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from oracle import hvla_ref_np as R

F = np.float64


def policy_mask(T: int, P: int, lang: bool) -> np.ndarray:
    """[1, 1, S, S] attention mask of the policy's sequence [T language | P patches | 1 action] (base_vit.py:207-214)."""
    if not lang:
        return R.policy_mask(1, P + 1)
    S = T + P + 1
    m = np.ones((1, 1, S, S), bool)
    m[:, :, :T, T:] = False                      # :211-212 language tokens only attend to themselves
    m[:, :, :-1, -1:] = False                    # :213-214 language and image tokens do not attend to the action token
    return m


def embed(bp: Dict[str, np.ndarray], g, patch_tokens, lang_tokens) -> np.ndarray:
    """The policy's input sequence [S, D] of one episode (base_vit.py:130-204)."""
    pfx = "encoder_"
    x = R.dense(patch_tokens, bp[pfx + "image_embedding_projection_kernel"], bp[pfx + "image_embedding_projection_bias"])
    if g.lang_in_policy:
        t = R.dense(np.asarray(lang_tokens, F), bp[pfx + "language_token_projection_kernel"],
                    bp[pfx + "language_token_projection_bias"])
        x = np.concatenate([t, x], axis=0)
    x = np.concatenate([x, np.zeros((1, g.dim), F)], axis=0)
    return x + np.asarray(bp[pfx + "pos_embedding"], F)[0]


def policy_one(bp: Dict[str, np.ndarray], g, patch_tokens, lang_tokens=None, sink: Optional[dict] = None):
    """One episode: (actions [horizon, action_dim], gripper logits [horizon], action embedding [D])."""
    x = embed(bp, g, patch_tokens, lang_tokens)[None]
    mask = policy_mask(g.lang_tokens, g.patches, g.lang_in_policy)
    tp = {R._slash(k[len("encoder_"):]): v for k, v in bp.items() if k.startswith("encoder_Transformer_0_")}
    if sink is not None:
        sink["pol/x0"] = x[0]
    x = R.transformer(x, mask, tp, "Transformer_0/", g.layers, g.heads, sink, "pol/")
    emb = x[0, -1]                                                   # base_vit.py:226
    cont = R.dense(emb, bp["action_head_continuous_head_kernel"], bp["action_head_continuous_head_bias"])
    logit = R.dense(emb, bp["action_head_discrete_head_kernel"], bp["action_head_discrete_head_bias"])
    cont = cont.reshape(g.horizon, g.action_dim - 1)                 # action_heads.py:460-463
    cont = np.tanh(cont / g.tanh_scale) * g.max_action               # :469-470
    grip = (logit >= 0.0).astype(F)                                  # :536
    return np.concatenate([cont, grip[:, None]], axis=-1), logit, emb


def policy(base_params, g, patch_tokens, lang_tokens=None, sinks=None):
    """Batched: base_params {flat leaf: [B, ...]}, patch_tokens [B, P, E], lang_tokens [B, T, lang_dim] (flag on)."""
    acts, logits, embs = [], [], []
    for b in range(patch_tokens.shape[0]):
        bp = {k: np.asarray(v[b], F) for k, v in base_params.items()}
        s = sinks[b] if sinks is not None else None
        a, l, e = policy_one(bp, g, np.asarray(patch_tokens[b], F), None if lang_tokens is None else lang_tokens[b], s)
        acts.append(a), logits.append(l), embs.append(e)
    return np.stack(acts), np.stack(logits), np.stack(embs)


def create_tasks(hp, g, instruction_dict, initial_state):
    """HyperVLA.create_tasks (hypervla/model.py:35-83): generated leaves {flat name: [B, ...]} incl. the language projection."""
    from hypervla.config import generated_leaves
    bp, _ = R.create_tasks(hp, g, generated_leaves(g), instruction_dict, initial_state)
    return bp


def sample_actions(hp, g, enc_shapes, base_params, images_u8, lang_tokens):
    """images u8 [B, H, W, 3] -> (actions, logits, DINOv2 patch tokens [B, P, E])."""
    imgs = np.asarray(images_u8)
    if imgs.ndim == 5:
        imgs = imgs[:, 0]
    tokens = R.dinov2(hp, g, enc_shapes, R.normalize_images(imgs))[:, 1:]
    a, l, _ = policy(base_params, g, tokens, lang_tokens)
    return a, l, tokens


def head_attention(base_params, g, patch_tokens, lang_tokens) -> np.ndarray:
    """[B, layers, heads, T + P]: the action token's attention over every other token, `attention_weights[0][b, :, -1, :-1]`
    (data/utils/hypervla_interface.py:213-215)."""
    B = patch_tokens.shape[0]
    sinks = [dict() for _ in range(B)]
    policy(base_params, g, patch_tokens, lang_tokens, sinks)
    key = "pol/Transformer_0/encoderblock_{}/MultiHeadDotProductAttention_0/attention_weights"
    return np.stack([np.stack([s[key.format(l)][0, :, -1, :-1] for l in range(g.layers)]) for s in sinks])


def language_kv(bp: Dict[str, np.ndarray], g, patch_tokens, lang_tokens):
    """K and V [layers, T, heads, head_dim] of the language tokens of one episode, every layer (what the prefix holds)."""
    sink: dict = {}
    policy_one(bp, g, np.asarray(patch_tokens, F), lang_tokens, sink)
    T = g.lang_tokens
    ks, vs = [], []
    x = sink["pol/x0"]
    for l in range(g.layers):
        b = f"encoder_Transformer_0_encoderblock_{l}_"
        h = R.layer_norm(x, bp[b + "LayerNorm_0_scale"], bp[b + "LayerNorm_0_bias"])[:T]
        a = b + "MultiHeadDotProductAttention_0_"
        ks.append(np.einsum("sd,dhk->shk", h, bp[a + "key_kernel"]) + bp[a + "key_bias"])
        vs.append(np.einsum("sd,dhk->shk", h, bp[a + "value_kernel"]) + bp[a + "value_bias"])
        x = sink[f"pol/Transformer_0/encoderblock_{l}/out"][0]
    return np.stack(ks), np.stack(vs)
