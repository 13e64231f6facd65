"""Float64 restatement of the generated policy with ``vit_kwargs.return_attention_map`` (test infrastructure, like oracle/).

With the flag every ``Encoder1DBlock`` of the policy runs ``CustomMultiHeadDotProductAttention``
(hypervla/components/transformer.py:172-181), which hands the boolean mask of base_vit.py:209-214 to
``nn.dot_product_attention_weights`` as ``bias=mask`` (hypervla/components/multi_head_attetion.py:88-98): flax scales the query
by 1/sqrt(hd), forms the scores, ADDS the bias (True -> 1.0, False -> 0.0) and takes the softmax over all S keys.  Nothing is
masked: a patch query attends to the action token's key, one logit below every other key; the action row gets + 1 on every key,
which its softmax ignores.  The attention leaves are named ``CustomMultiHeadDotProductAttention_0`` (``Geometry.attention_name``).

``mode`` selects the attention of the same network, on the geometry's own leaf names:
    "bias"     the restatement: scores + M, M = 1 except M[q < P][k = P] = 0
    "literal"  dot_product_attention_weights(bias=mask) line by line (query / sqrt(depth), einsum, + bias, softmax)
    "masked"   -inf where the mask is False: the model WITHOUT the flag (what oracle/ computes), for comparisons
numpy (`policy`, `sample_actions`, `head_attention`) and torch (`PolicyBiasRef`, `train_loss_and_grads`) forms.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import hvla_ref_np as onp
from oracle import hvla_ref_torch as ot

import attention_loss_ref as AR

F = np.float64


def mask_matrix(S: int) -> np.ndarray:
    """base_vit.py:209-214 as floats: 1 = allowed, 0 = not (patch rows against the action key)."""
    m = np.ones((S, S), F)
    m[:-1, -1] = 0.0
    return m


# ---------------------------------------------------------------------------------------------- numpy
def _weights(q, k, mode):
    """q, k [S, H, hd] -> attention weights [H, S, S]."""
    S, H, hd = q.shape
    M = mask_matrix(S)
    if mode == "literal":                                             # flax.linen.attention.dot_product_attention_weights
        depth = q.shape[-1]
        query = q / np.sqrt(depth).astype(F)
        attn_weights = np.einsum("qhd,khd->hqk", query, k)
        bias = M.astype(bool)[None]                                   # the mask, handed over as bias=
        attn_weights = attn_weights + bias                            # bool + float: True -> 1.0
        attn_weights = attn_weights - attn_weights.max(-1, keepdims=True)
        e = np.exp(attn_weights)
        return e / e.sum(-1, keepdims=True)
    s = np.einsum("qhd,khd->hqk", q, k) / math.sqrt(hd)
    if mode == "bias":
        s = s + M[None]
    elif mode == "masked":
        s = np.where(M[None] != 0, s, -np.inf)
    else:
        raise ValueError(mode)
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


def _policy_one(bp, g, patch_tokens, mode="bias", below=None):
    """One episode; bp leaves carry no batch dim.  Returns (actions, logits, [per-layer weights [H, S, S]], [per-layer block inputs]).
    `below`: per-layer block inputs to use INSTEAD of the running residual (holds the layers below equal between two modes)."""
    D, H, hd = g.dim, g.heads, g.head_dim
    x = onp.dense(patch_tokens, bp["encoder_image_embedding_projection_kernel"], bp["encoder_image_embedding_projection_bias"])
    x = np.concatenate([x, np.zeros((1, D), F)], 0) + np.asarray(bp["encoder_pos_embedding"], F)[0]
    maps, inputs = [], []
    for l in range(g.layers):
        if below is not None:
            x = below[l]
        inputs.append(x)
        pb = f"encoder_Transformer_0_encoderblock_{l}_"
        pa = pb + g.attention_name + "_"
        h = onp.layer_norm(x, bp[pb + "LayerNorm_0_scale"], bp[pb + "LayerNorm_0_bias"])
        q = np.einsum("sd,dhk->shk", h, np.asarray(bp[pa + "query_kernel"], F)) + np.asarray(bp[pa + "query_bias"], F)
        k = np.einsum("sd,dhk->shk", h, np.asarray(bp[pa + "key_kernel"], F)) + np.asarray(bp[pa + "key_bias"], F)
        v = np.einsum("sd,dhk->shk", h, np.asarray(bp[pa + "value_kernel"], F)) + np.asarray(bp[pa + "value_bias"], F)
        w = _weights(q, k, mode)
        maps.append(w)
        o = np.einsum("hqk,khd->qhd", w, v)
        x = x + np.einsum("qhd,hdo->qo", o, np.asarray(bp[pa + "out_kernel"], F)) + np.asarray(bp[pa + "out_bias"], F)
        y = onp.layer_norm(x, bp[pb + "LayerNorm_1_scale"], bp[pb + "LayerNorm_1_bias"])
        y = onp.gelu_tanh(onp.dense(y, bp[pb + "MlpBlock_0_Dense_0_kernel"], bp[pb + "MlpBlock_0_Dense_0_bias"]))
        x = x + onp.dense(y, bp[pb + "MlpBlock_0_Dense_1_kernel"], bp[pb + "MlpBlock_0_Dense_1_bias"])
    x = onp.layer_norm(x, bp["encoder_Transformer_0_encoder_norm_scale"], bp["encoder_Transformer_0_encoder_norm_bias"])
    emb = x[-1]
    cont = onp.dense(emb, bp["action_head_continuous_head_kernel"], bp["action_head_continuous_head_bias"])
    logit = onp.dense(emb, bp["action_head_discrete_head_kernel"], bp["action_head_discrete_head_bias"])
    cont = np.tanh(cont.reshape(g.horizon, g.action_dim - 1) / g.tanh_scale) * g.max_action
    act = np.concatenate([cont, (logit >= 0.0).astype(F)[:, None]], -1)
    return act, logit, maps, inputs


def policy(base_params, g, patch_tokens, mode="bias"):
    """Batched episodes with their own weights: (actions [B, Hz, ad], logits [B, Hz], head maps [B, L, H, P]) -- the maps are
    `attention_weights[0, :, -1, :-1]` of every layer (hypervla_interface.py:213-215)."""
    acts, logits, heads = [], [], []
    for b in range(np.asarray(patch_tokens).shape[0]):
        bp = {k: np.asarray(v[b], F) for k, v in base_params.items()}
        a, l, maps, _ = _policy_one(bp, g, np.asarray(patch_tokens[b], F), mode)
        acts.append(a), logits.append(l), heads.append(np.stack([m[:, -1, :-1] for m in maps]))
    return np.stack(acts), np.stack(logits), np.stack(heads)


def create_tasks(hp, g, instruction_dict, initial_state):
    from hypervla.config import generated_leaves
    return onp.create_tasks(hp, g, generated_leaves(g), instruction_dict, initial_state)[0]


def sample_actions(hp, g, enc_shapes, base_params, images_u8, mode="bias"):
    """images [B, 1, H, W, 3] uint8 -> (actions, logits, head maps, tokens)."""
    imgs = np.asarray(images_u8)
    if imgs.ndim == 5:
        imgs = imgs[:, 0]
    tokens = onp.dinov2(hp, g, enc_shapes, onp.normalize_images(imgs))[:, 1:]
    return policy(base_params, g, tokens, mode) + (tokens,)


def to_masked_names(base_params, g):
    """The same leaves under the names of the model without the flag (what oracle/ reads)."""
    return {k.replace(g.attention_name, "MultiHeadDotProductAttention_0"): v for k, v in base_params.items()}


# ---------------------------------------------------------------------------------------------- torch
class PolicyBiasRef(ot.PolicyRef):
    """``attention_loss_ref.PolicyAttnRef`` with the attention of `mode`: (actions, logits, last block's map [B, H, S, S])."""

    def __init__(self, g, leaves, mode="bias"):
        super().__init__(g, leaves)
        self.mode = mode

    def __call__(self, theta, tokens, quant=None):
        assert quant is None
        g = self.g
        B, P, E = tokens.shape
        D, H, hd = g.dim, g.heads, g.head_dim
        lf = lambda n: self.leaf(theta, n)
        x = torch.bmm(tokens, lf("encoder_image_embedding_projection_kernel")) + lf("encoder_image_embedding_projection_bias")[:, None]
        x = torch.cat([x, torch.zeros(B, 1, D, dtype=x.dtype)], 1) + lf("encoder_pos_embedding")[:, 0]
        S = P + 1
        M = torch.as_tensor(mask_matrix(S)).to(x.dtype)

        def ln(x, pre):
            s, b = lf(pre + "_scale")[:, None], lf(pre + "_bias")[:, None]
            return Fn.layer_norm(x, (D,), None, None, eps=1e-6) * s + b

        attn = None
        for l in range(g.layers):
            pb = f"encoder_Transformer_0_encoderblock_{l}_"
            pa = pb + g.attention_name + "_"
            h = ln(x, pb + "LayerNorm_0")
            q = torch.bmm(h, lf(pa + "query_kernel").reshape(B, D, D)) + lf(pa + "query_bias").reshape(B, 1, D)
            k = torch.bmm(h, lf(pa + "key_kernel").reshape(B, D, D)) + lf(pa + "key_bias").reshape(B, 1, D)
            v = torch.bmm(h, lf(pa + "value_kernel").reshape(B, D, D)) + lf(pa + "value_bias").reshape(B, 1, D)
            q, k, v = (t.reshape(B, S, H, hd).transpose(1, 2) for t in (q, k, v))
            scores = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
            if self.mode == "bias":
                scores = scores + M
            else:
                assert self.mode == "masked"
                scores = scores.masked_fill(M == 0, float("-inf"))
            attn = torch.softmax(scores, dim=-1)
            o = (attn @ v).transpose(1, 2).reshape(B, S, D)
            x = x + torch.bmm(o, lf(pa + "out_kernel").reshape(B, D, D)) + lf(pa + "out_bias")[:, None]
            y = ln(x, pb + "LayerNorm_1")
            y = Fn.gelu(torch.bmm(y, lf(pb + "MlpBlock_0_Dense_0_kernel")) + lf(pb + "MlpBlock_0_Dense_0_bias")[:, None], approximate="tanh")
            x = x + torch.bmm(y, lf(pb + "MlpBlock_0_Dense_1_kernel")) + lf(pb + "MlpBlock_0_Dense_1_bias")[:, None]
        x = ln(x, "encoder_Transformer_0_encoder_norm")
        emb = x[:, -1:]
        cont = torch.bmm(emb, lf("action_head_continuous_head_kernel"))[:, 0] + lf("action_head_continuous_head_bias")
        logit = torch.bmm(emb, lf("action_head_discrete_head_kernel"))[:, 0] + lf("action_head_discrete_head_bias")
        cont = torch.tanh(cont.reshape(B, g.horizon, g.action_dim - 1) / g.tanh_scale) * g.max_action
        act = torch.cat([cont, (logit >= 0).to(cont.dtype)[..., None]], -1)
        return act, logit, attn


def train_loss_and_grads(params, g, leaves, instruction_dict, initial_state, tokens, batch, w_ent=0.0, w_align=0.0,
                         reference_map=None, mode="bias", dtype=torch.float64, images=None, enc_shapes=None, clip_target=None):
    """``attention_loss_ref.train_loss_and_grads_aux`` on this policy: (per-sample loss [B] including the weighted terms, ent [B],
    align [B] (zeros without a map), {leaf: d mean_b loss_b / d leaf}).  With `images` the DINOv2 encoder is in the graph."""
    hn = ot.HyperNetRef(params, g, leaves, dtype)
    names = sorted(hn.p)
    for k in names:
        hn.p[k] = hn.p[k].clone().requires_grad_(True)
    hn.w_cat = torch.cat([hn.p[l.head_name + "/kernel"] for l in leaves], dim=1)
    hn.b_cat = torch.cat([hn.p[l.head_name + "/bias"] for l in leaves], dim=0)
    li = instruction_dict["language_instruction"]
    ctx = hn.context(li["token_embedding"], li["attention_mask"], np.asarray(initial_state["patch_embeddings"])[:, 0])
    theta = hn.generate(ctx)
    enc = None
    if images is not None:
        enc = ot.build_hf_dinov2(params, g, enc_shapes, dtype).train(False)
        for q in enc.parameters():
            q.requires_grad_(True)
        x = torch.as_tensor(np.asarray(images)).to(dtype)
        if x.ndim == 5:
            x = x[:, 0]
        x = (x / 255.0 - ot._MEAN.to(dtype)) / ot._STD.to(dtype)
        tok_t = enc(pixel_values=x.permute(0, 3, 1, 2).contiguous()).last_hidden_state[:, 1:]
    else:
        tok_t = torch.as_tensor(np.asarray(tokens)).to(dtype)
    act, logit, attn = PolicyBiasRef(g, leaves, mode)(theta, tok_t)
    if clip_target is None:
        clip_target = bool(getattr(g, "clip_target", True))
    per, _ = ot.mix_loss(g, act[..., :-1], logit, batch["action"], batch["timestep_pad_mask"], batch["action_pad_mask"],
                         clip_target=clip_target)
    ent, align = AR.attention_terms(attn, reference_map if w_align else None)
    if align is None:
        align = torch.zeros_like(ent)
    per = per + w_ent * ent + w_align * align
    loss = per.mean()
    wrt = [hn.p[k] for k in names]
    enc_named = list(enc.named_parameters()) if enc is not None else []
    grads = torch.autograd.grad(loss, wrt + [q for _, q in enc_named], allow_unused=True)
    out = {k: (gr.detach() if gr is not None else torch.zeros_like(hn.p[k])) for k, gr in zip(names, grads)}
    if enc is not None:
        hf = {n: (gr.detach() if gr is not None else torch.zeros_like(q)) for (n, q), gr in zip(enc_named, grads[len(wrt):])}
        out.update(ot._hf_grads_to_flax(hf, g))
    return per.detach(), ent.detach(), align.detach(), out
