"""Float64 restatement of the generated policy with ``vit_kwargs.use_differential_transformer`` (test infrastructure, like oracle/).

With the flag every ``Encoder1DBlock`` of the policy runs ``DifferentialAttention(embed_dim=D, num_heads=H, depth=l)`` on
``LayerNorm_0(x)`` with ``attn_mask=`` the boolean mask of base_vit.py:209-214 (hypervla/components/transformer.py:166-171,
hypervla/components/differential_transformer.py:99-252).  q / k / v / out are bias-free ``Dense(D)``; q and k are split into
2 H heads of hd = D / (2 H), head h of the module taking q / k heads 2 h (part 1) and 2 h + 1 (part 2) and the 2 hd features
[2 hd h, 2 hd (h + 1)) of v; the scores are unscaled, the mask is ADDED (True -> 1.0: a patch query sees the action key one
logit below the others), A = softmax(q1 k1) - lambda softmax(q2 k2), the head's A V goes through an RMSNorm(2 hd, eps 1e-5)
with one weight for all heads and is scaled by 1 - lambda_init(l); lambda = exp(sum lambda_q1 lambda_k1)
- exp(sum lambda_q2 lambda_k2) + lambda_init(l), lambda_init(l) = 0.8 - 0.6 exp(-0.3 l).

``mode`` selects the attention of the same network:
    "literal"   DifferentialAttention.__call__ line by line (its reshapes, einsum strings, + attn_mask, subln on [b h t, 2 hd])
    "restated"  the same in head / part indexing (what the kernel computes)
    "plain"     the model WITHOUT the flag on the same tensors (masked softmax over 2 hd features, 1 / sqrt(2 hd), no lambda, no
                RMSNorm, no biases), to tell the models apart
``dtype``: numpy float64 (the reference) or float32 (the conditioning check: every operation in float32).
"""
from __future__ import annotations

import math

import numpy as np

from oracle import hvla_ref_np as onp

F = np.float64


def lambda_init_fn(depth):
    return 0.8 - 0.6 * math.exp(-0.3 * depth)                         # differential_transformer.py:75-79


def mask_matrix(S: int) -> np.ndarray:
    """base_vit.py:209-214: True = allowed; patch rows against the action key are False."""
    m = np.ones((S, S), bool)
    m[:-1, -1] = False
    return m


class _Ops:
    """dense / layer_norm / gelu_tanh of oracle.hvla_ref_np in float64, the same formulas in `dtype` otherwise."""

    def __init__(self, dtype):
        self.t = dtype
        self.f64 = dtype == np.float64

    def a(self, x):
        return np.asarray(x, self.t)

    def dense(self, x, k, b=None):
        if self.f64:
            return onp.dense(x, k, 0.0 if b is None else b)
        y = self.a(x) @ self.a(k)
        return y if b is None else y + self.a(b)

    def layer_norm(self, x, s, b):
        if self.f64:
            return onp.layer_norm(x, s, b)
        x = self.a(x)
        mean = x.mean(-1, keepdims=True, dtype=self.t)
        var = np.maximum(self.t(0.0), (x * x).mean(-1, keepdims=True, dtype=self.t) - mean * mean)
        return (x - mean) / np.sqrt(var + self.t(1e-6)) * self.a(s) + self.a(b)

    def gelu_tanh(self, x):
        if self.f64:
            return onp.gelu_tanh(x)
        t = self.t
        return t(0.5) * x * (t(1.0) + np.tanh(t(math.sqrt(2.0 / math.pi)) * (x + t(0.044715) * x * x * x)))


def _softmax(s):
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


def lambda_full(bp, pa, l, t=F):
    """differential_transformer.py:227-229 for layer l of one episode."""
    lq1, lk1, lq2, lk2 = (np.asarray(bp[pa + n], t) for n in ("lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2"))
    return np.exp(np.sum(lq1 * lk1)) - np.exp(np.sum(lq2 * lk2)) + t(lambda_init_fn(l))


def _attn_literal(h, bp, pa, g, l, ops):
    """DifferentialAttention.__call__ (differential_transformer.py:183-252), x = h[None]."""
    t = ops.t
    x = h[None]
    embed_dim, num_heads = g.dim, g.heads
    num_kv_heads, n_rep = num_heads, 1
    head_dim = embed_dim // (2 * num_heads)
    bsz, tgt_len, _ = x.shape
    src_len = tgt_len
    q = ops.dense(x, bp[pa + "q_proj_kernel"])
    k = ops.dense(x, bp[pa + "k_proj_kernel"])
    v = ops.dense(x, bp[pa + "v_proj_kernel"])
    q = q.reshape(bsz, tgt_len, 2 * num_heads, head_dim)
    k = k.reshape(bsz, src_len, 2 * num_kv_heads, head_dim)
    v = v.reshape(bsz, src_len, num_kv_heads, 2 * head_dim)
    q = q.reshape(bsz, tgt_len, num_heads, 2, head_dim)
    q1 = q[:, :, :, 0, :]
    q2 = q[:, :, :, 1, :]
    k = k.reshape(bsz, src_len, num_kv_heads, 2, head_dim)
    k1 = k[:, :, :, 0, :]
    k2 = k[:, :, :, 1, :]
    assert n_rep == 1
    q1k1 = np.einsum("bthd,bshd->bhts", q1, k1)
    q2k2 = np.einsum("bthd,bshd->bhts", q2, k2)
    attn_mask = mask_matrix(tgt_len)[None, None]                      # [1, 1, S, S] bool (transformer.py:171)
    q1k1 = q1k1 + attn_mask.astype(t)                                 # bool + float: True -> 1.0
    q2k2 = q2k2 + attn_mask.astype(t)
    A1 = _softmax(q1k1)
    A2 = _softmax(q2k2)
    lambda_init = t(lambda_init_fn(l))
    lambda_1 = np.exp(np.sum(ops.a(bp[pa + "lambda_q1"]) * ops.a(bp[pa + "lambda_k1"])))
    lambda_2 = np.exp(np.sum(ops.a(bp[pa + "lambda_q2"]) * ops.a(bp[pa + "lambda_k2"])))
    lambda_full_ = lambda_1 - lambda_2 + lambda_init
    A = A1 - lambda_full_ * A2
    v = v.transpose(0, 2, 1, 3)
    attn = np.einsum("bhts,bhsd->bhtd", A, v)
    attn_reshaped = attn.reshape(bsz * num_heads * tgt_len, 2 * head_dim)
    normed = attn_reshaped / np.sqrt(np.mean(attn_reshaped ** 2, axis=-1, keepdims=True, dtype=t) + t(1e-5))   # RMSNorm(eps=self.eps)
    attn_normed = normed * ops.a(bp[pa + "subln_weight"])
    attn_normed = attn_normed.reshape(bsz, num_heads, tgt_len, 2 * head_dim)
    attn_normed = attn_normed * (t(1.0) - lambda_init)
    attn_out = attn_normed.transpose(0, 2, 1, 3).reshape(bsz, tgt_len, embed_dim)
    return ops.dense(attn_out, bp[pa + "out_proj_kernel"])[0]


def _attn_restated(h, bp, pa, g, l, ops):
    """Head / part indexing: feature 2 hd h + hd c + d of q, k is head h, part c; v and the output use feature 2 hd h + d."""
    t = ops.t
    S, D, H = h.shape[0], g.dim, g.heads
    hd = D // (2 * H)
    q = ops.dense(h, bp[pa + "q_proj_kernel"]).reshape(S, H, 2, hd)
    k = ops.dense(h, bp[pa + "k_proj_kernel"]).reshape(S, H, 2, hd)
    v = ops.dense(h, bp[pa + "v_proj_kernel"]).reshape(S, H, 2 * hd)
    M = mask_matrix(S).astype(t)
    lam, linit = lambda_full(bp, pa, l, t), t(lambda_init_fn(l))
    w = ops.a(bp[pa + "subln_weight"])
    out = np.empty((S, H, 2 * hd), t)
    for hh in range(H):
        A = [_softmax(q[:, hh, c] @ k[:, hh, c].T + M) for c in range(2)]
        o = (A[0] - lam * A[1]) @ v[:, hh]
        o = o / np.sqrt((o * o).mean(-1, keepdims=True, dtype=t) + t(1e-5))
        out[:, hh] = o * w * (t(1.0) - linit)
    return ops.dense(out.reshape(S, D), bp[pa + "out_proj_kernel"])


def _attn_plain(h, bp, pa, g, l, ops):
    """nn.MultiHeadDotProductAttention on the same four kernels (H heads of 2 hd, the mask applied), zero biases."""
    t = ops.t
    S, D, H = h.shape[0], g.dim, g.heads
    hd = D // H
    q = ops.dense(h, bp[pa + "q_proj_kernel"]).reshape(S, H, hd)
    k = ops.dense(h, bp[pa + "k_proj_kernel"]).reshape(S, H, hd)
    v = ops.dense(h, bp[pa + "v_proj_kernel"]).reshape(S, H, hd)
    s = np.einsum("qhd,khd->hqk", q, k) / t(math.sqrt(hd))
    s = np.where(mask_matrix(S)[None], s, -np.inf)
    o = np.einsum("hqk,khd->qhd", _softmax(s), v)
    return ops.dense(o.reshape(S, D), bp[pa + "out_proj_kernel"])


_ATTN = {"literal": _attn_literal, "restated": _attn_restated, "plain": _attn_plain}


def _policy_one(bp, g, patch_tokens, mode, ops):
    D = g.dim
    x = ops.dense(ops.a(patch_tokens), bp["encoder_image_embedding_projection_kernel"], bp["encoder_image_embedding_projection_bias"])
    x = np.concatenate([x, np.zeros((1, D), ops.t)], 0) + ops.a(bp["encoder_pos_embedding"])[0]
    for l in range(g.layers):
        pb = f"encoder_Transformer_0_encoderblock_{l}_"
        pa = pb + g.attention_name + "_"
        h = ops.layer_norm(x, bp[pb + "LayerNorm_0_scale"], bp[pb + "LayerNorm_0_bias"])
        x = x + _ATTN[mode](h, bp, pa, g, l, ops)
        y = ops.layer_norm(x, bp[pb + "LayerNorm_1_scale"], bp[pb + "LayerNorm_1_bias"])
        y = ops.gelu_tanh(ops.dense(y, bp[pb + "MlpBlock_0_Dense_0_kernel"], bp[pb + "MlpBlock_0_Dense_0_bias"]))
        x = x + ops.dense(y, bp[pb + "MlpBlock_0_Dense_1_kernel"], bp[pb + "MlpBlock_0_Dense_1_bias"])
    x = ops.layer_norm(x, bp["encoder_Transformer_0_encoder_norm_scale"], bp["encoder_Transformer_0_encoder_norm_bias"])
    emb = x[-1]
    cont = ops.dense(emb, bp["action_head_continuous_head_kernel"], bp["action_head_continuous_head_bias"])
    logit = ops.dense(emb, bp["action_head_discrete_head_kernel"], bp["action_head_discrete_head_bias"])
    cont = np.tanh(cont.reshape(g.horizon, g.action_dim - 1) / ops.t(g.tanh_scale)) * ops.t(g.max_action)
    act = np.concatenate([cont, (logit >= 0.0).astype(ops.t)[:, None]], -1)
    return act, logit


def policy(base_params, g, patch_tokens, mode="restated", dtype=F):
    """Batched episodes with their own weights: (actions [B, Hz, ad], logits [B, Hz])."""
    ops = _Ops(dtype)
    acts, logits = [], []
    for b in range(np.asarray(patch_tokens).shape[0]):
        bp = {k: np.asarray(v[b], dtype) for k, v in base_params.items()}
        a, l = _policy_one(bp, g, np.asarray(patch_tokens[b], dtype), mode, ops)
        acts.append(a), logits.append(l)
    return np.stack(acts), np.stack(logits)


def lambdas(base_params, g):
    """lambda of every episode and layer, [B, L] float64."""
    B = next(iter(base_params.values())).shape[0]
    out = np.empty((B, g.layers), F)
    for b in range(B):
        for l in range(g.layers):
            pa = f"encoder_Transformer_0_encoderblock_{l}_{g.attention_name}_"
            out[b, l] = lambda_full({k: np.asarray(v[b], F) for k, v in base_params.items() if k.startswith(pa)}, pa, l)
    return out


def lambda_scaled(params, x=5.0):
    """The checkpoint with every lambda output head (kernel and bias) x `x`: the generated lambda vectors x `x`, their products x^2."""
    return {k: (v * np.float32(x)).astype(np.float32) if k.startswith("output_head_") and "_lambda_" in k else v
            for k, v in params.items()}


def create_tasks(hp, g, instruction_dict, initial_state):
    from hypervla.config import generated_leaves
    return onp.create_tasks(hp, g, generated_leaves(g), instruction_dict, initial_state)[0]


def sample_actions(hp, g, enc_shapes, base_params, images_u8, mode="restated"):
    """images [B, 1, H, W, 3] uint8 -> (actions, logits, tokens)."""
    imgs = np.asarray(images_u8)
    if imgs.ndim == 5:
        imgs = imgs[:, 0]
    tokens = onp.dinov2(hp, g, enc_shapes, onp.normalize_images(imgs))[:, 1:]
    return policy(base_params, g, tokens, mode) + (tokens,)
