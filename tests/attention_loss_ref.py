"""Float64 restatement of the fine-tune loss with the reference's two attention terms (test infrastructure, like oracle/).

``oracle.hvla_ref_torch.PolicyRef`` runs its attention through ``scaled_dot_product_attention`` and exposes no
probabilities, so the generated policy is restated here with an explicit masked softmax that also returns the LAST block's map
[B, H, S, S] -- what the reference's base net hands to ``sample_loss_fn`` (hypervla/components/transformer.py:248-262).
``HyperNetRef``, ``mix_loss`` and ``build_hf_dinov2`` are the oracle's, unchanged.  The two terms (scripts/train.py:348-373),
per sample, on the action token's row of that map:

    ent_b   = mean_h ( -sum_k p[h, -1, k] log(p[h, -1, k] + 1e-8) )
    align_b = mean_{k < P} ( mean_h p[h, -1, k] - r_b[k] )^2               r_b: DINOv2's CLS row, mean over heads, a constant
    loss    = mean_b ( mix_loss_b + w_ent ent_b + w_align align_b )        w_align: already annealed
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import hvla_ref_torch as ot

EPS = 1e-8


class PolicyAttnRef(ot.PolicyRef):
    """``PolicyRef.__call__`` operation for operation, the attention written out: (actions, logits, last block's map)."""

    def __call__(self, theta, tokens, quant=None):
        assert quant is None
        g = self.g
        B, P, E = tokens.shape
        D, H, hd = g.dim, g.heads, g.head_dim
        lf = lambda n: self.leaf(theta, n)
        x = torch.bmm(tokens, lf("encoder_image_embedding_projection_kernel")) + lf("encoder_image_embedding_projection_bias")[:, None]
        x = torch.cat([x, torch.zeros(B, 1, D, dtype=x.dtype)], 1) + lf("encoder_pos_embedding")[:, 0]
        S = P + 1
        keep = torch.ones(S, S, dtype=torch.bool)
        keep[:-1, -1] = False                                         # base_vit.py:209-214: only the action token sees the action key

        def ln(x, pre):
            s, b = lf(pre + "_scale")[:, None], lf(pre + "_bias")[:, None]
            return Fn.layer_norm(x, (D,), None, None, eps=1e-6) * s + b

        attn = None
        for l in range(g.layers):
            pb = f"encoder_Transformer_0_encoderblock_{l}_"
            pa = pb + "MultiHeadDotProductAttention_0_"
            h = ln(x, pb + "LayerNorm_0")
            q = torch.bmm(h, lf(pa + "query_kernel").reshape(B, D, D)) + lf(pa + "query_bias").reshape(B, 1, D)
            k = torch.bmm(h, lf(pa + "key_kernel").reshape(B, D, D)) + lf(pa + "key_bias").reshape(B, 1, D)
            v = torch.bmm(h, lf(pa + "value_kernel").reshape(B, D, D)) + lf(pa + "value_bias").reshape(B, 1, D)
            q, k, v = (t.reshape(B, S, H, hd).transpose(1, 2) for t in (q, k, v))
            scores = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
            attn = torch.softmax(scores.masked_fill(~keep, float("-inf")), dim=-1)      # [B, H, S, S]
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


def attention_terms(attn, reference_map=None):
    """(ent [B], align [B] or None) of a map [B, H, S, S] (torch): scripts/train.py:350-372 per sample."""
    p = attn[:, :, -1]                                                # [B, H, S]: the action token's row
    ent = (-(p * torch.log(p + EPS)).sum(-1)).mean(1)
    if reference_map is None:
        return ent, None
    r = torch.as_tensor(np.asarray(reference_map)).to(attn.dtype)
    return ent, ((p[:, :, :-1].mean(1) - r) ** 2).mean(-1)


def dterms_dp(p, w_ent, w_align, r):
    """The analytic gradient the kernel adds to dp: d(w_ent ent + w_align align) / dp[h][k] for ONE sample; p [H, S], r [P] (numpy)."""
    H, S = p.shape
    P = S - 1
    g = (w_ent / H) * (-np.log(p + EPS) - p / (p + EPS))
    if w_align:
        m = p.mean(0)
        g[:, :P] += w_align * 2.0 * (m[:P] - r) / (P * H)
    return g


def train_loss_and_grads_aux(params, g, leaves, instruction_dict, initial_state, tokens, batch, w_ent=0.0, w_align=0.0,
                             reference_map=None, dtype=torch.float64, images=None, enc_shapes=None, clip_target=None):
    """``oracle.hvla_ref_torch.train_loss_and_grads`` with the two terms: (per-sample loss [B] INCLUDING the weighted terms,
    ent [B], align [B] (zeros without a map), {leaf: d mean_b loss_b / d leaf}).  With `images` the DINOv2 encoder is in the graph."""
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
    act, logit, attn = PolicyAttnRef(g, leaves)(theta, tok_t)
    if clip_target is None:
        clip_target = bool(getattr(g, "clip_target", True))
    per, _ = ot.mix_loss(g, act[..., :-1], logit, batch["action"], batch["timestep_pad_mask"], batch["action_pad_mask"],
                         clip_target=clip_target)
    ent, align = attention_terms(attn, reference_map if w_align else None)
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


def synthetic_reference_map(B: int, P: int, seed: int = 5) -> np.ndarray:
    """A stand-in for DINOv2's CLS row, mean over heads: positive, peaked on a few patches, summing to less than 1 (the CLS key
    keeps some of the mass) -- f32 [B, P]."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, P + 1)) * 1.5
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True))[:, 1:].astype(np.float32)
