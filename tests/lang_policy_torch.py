"""Float64 torch restatement of the generated policy with ``vit_kwargs.use_language_token``, for autograd (test infrastructure, like
oracle/): the gradient oracle of the fine-tune step with ``FineTuner(language_tokens=True)``.

``LangPolicyRef`` has the structure of ``oracle.hvla_ref_torch.PolicyRef`` (a batch of episodes that each carry their own weights,
batched matmuls in the role of jax.vmap) with what the option adds, as tests/lang_policy_ref.py states it in numpy
(reference ``hypervla/components/base_vit.py:159-166, 182-214``): every T5 position through ``language_token_projection`` in front of
the patch tokens, ``pos_embedding`` of T + P + 1 rows, and the mask -- language queries see only language keys, no query but the
action token's sees the action key.  ``train_loss_and_grads`` composes it with ``HyperNetRef``, ``mix_loss`` and (encoder trained)
``build_hf_dinov2`` exactly as ``oracle.hvla_ref_torch.train_loss_and_grads`` composes ``PolicyRef``.  ``GEOMETRIES`` names the
language geometries the GPU tests and the CPU extent trace (tools/train_lang_extent_trace.hip) share.
"""
import dataclasses

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import hvla_ref_torch as ot

# name: (changes to MID with lang_in_policy=True, B).  P = 64, D = 64, two policy layers, lang_dim 64 unless changed.
GEOMETRIES = {
    "T12": (dict(), 4),                                       # Sx = 77 -> row stride 80
    "T2": (dict(lang_tokens=2), 4),                           # Sx = 67: the shortest prefix, K = 2 in dWl
    "T3": (dict(lang_tokens=3), 4),                           # Sx = 68: a row stride with no padding behind the row
    "T32": (dict(lang_tokens=32), 4),                         # Sx = 97: the longest prefix
    "T32-P256": (dict(lang_tokens=32, image_size=224), 2),    # Sx = 289: more than one 128-row tile per episode
}


def geometry(name):
    from hypervla.config import MID
    changes, B = GEOMETRIES[name]
    return dataclasses.replace(MID, lang_in_policy=True, **changes), B


def policy_keep(T, P):
    """bool [S, S], True = attend (base_vit.py:209-214)."""
    S = T + P + 1
    keep = torch.ones(S, S, dtype=torch.bool)
    keep[:T, T:] = False
    keep[:-1, -1] = False
    return keep


class LangPolicyRef(ot.PolicyRef):
    """ViT.__call__ with use_language_token + MixActionHead for theta [B, G], tokens [B, P, E], lang_tokens [B, T, lang_dim]."""

    def __call__(self, theta, tokens, lang_tokens):
        g = self.g
        B, P, E = tokens.shape
        T = lang_tokens.shape[1]
        D, H, hd = g.dim, g.heads, g.head_dim
        lf = lambda n: self.leaf(theta, n)
        x = torch.bmm(tokens, lf("encoder_image_embedding_projection_kernel")) + lf("encoder_image_embedding_projection_bias")[:, None]
        t = torch.bmm(lang_tokens, lf("encoder_language_token_projection_kernel")) + lf("encoder_language_token_projection_bias")[:, None]
        x = torch.cat([t, x, torch.zeros(B, 1, D, dtype=x.dtype)], 1) + lf("encoder_pos_embedding")[:, 0]
        S = T + P + 1
        keep = policy_keep(T, P)

        def ln(x, pre):
            s, b = lf(pre + "_scale")[:, None], lf(pre + "_bias")[:, None]
            return Fn.layer_norm(x, (D,), None, None, eps=1e-6) * s + b

        for l in range(g.layers):
            pb = f"encoder_Transformer_0_encoderblock_{l}_"
            pa = pb + "MultiHeadDotProductAttention_0_"
            h = ln(x, pb + "LayerNorm_0")
            q = torch.bmm(h, lf(pa + "query_kernel").reshape(B, D, D)) + lf(pa + "query_bias").reshape(B, 1, D)
            k = torch.bmm(h, lf(pa + "key_kernel").reshape(B, D, D)) + lf(pa + "key_bias").reshape(B, 1, D)
            v = torch.bmm(h, lf(pa + "value_kernel").reshape(B, D, D)) + lf(pa + "value_bias").reshape(B, 1, D)
            q, k, v = (u.reshape(B, S, H, hd).transpose(1, 2) for u in (q, k, v))
            o = Fn.scaled_dot_product_attention(q, k, v, attn_mask=keep)
            o = o.transpose(1, 2).reshape(B, S, D)
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
        return act, logit, emb[:, 0]


def train_loss_and_grads(params, g, leaves, instruction_dict, initial_state, tokens, batch, images=None, enc_shapes=None):
    """(per-sample loss [B], mean loss, {leaf: gradient}) in float64 by autograd through hypernetwork -> theta -> LangPolicyRef ->
    mix loss; with `images` (and `enc_shapes`) through transformers' Dinov2Model too, its gradients under the checkpoint's names.
    The instruction's token embeddings feed the context encoder AND the policy; nothing is differentiated with respect to them."""
    dtype = torch.float64
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
    lang = torch.as_tensor(np.asarray(li["token_embedding"])).to(dtype)
    act, logit, _ = LangPolicyRef(g, leaves)(theta, tok_t, lang)
    per, loss = ot.mix_loss(g, act[..., :-1], logit, batch["action"], batch["timestep_pad_mask"], batch["action_pad_mask"],
                            clip_target=bool(getattr(g, "clip_target", True)))
    wrt = [hn.p[k] for k in names]
    enc_named = list(enc.named_parameters()) if enc is not None else []
    grads = torch.autograd.grad(loss, wrt + [q for _, q in enc_named], allow_unused=True)
    out = {k: (gr.detach() if gr is not None else torch.zeros_like(hn.p[k])) for k, gr in zip(names, grads)}
    if enc is not None:
        hf = {n: (gr.detach() if gr is not None else torch.zeros_like(q)) for (n, q), gr in zip(enc_named, grads[len(wrt):])}
        out.update(ot._hf_grads_to_flax(hf, g))
    return per.detach(), loss.detach(), out
