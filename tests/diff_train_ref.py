"""Torch float64 autograd restatement of the generated policy with ``vit_kwargs.use_differential_transformer`` (test infrastructure,
like oracle/): the gradient oracle of FineTuner(differential=True).

``diff_attention`` is ``tests/diff_attention_ref._attn_restated`` in torch, batched over episodes that each carry their own leaves
(hypervla/components/differential_transformer.py:99-252).  ``PolicyDiffRef`` is ``oracle.hvla_ref_torch.PolicyRef`` with it in every
block, in the manner of ``mask_bias_ref.PolicyBiasRef``; ``train_loss_and_grads`` is the oracle's function of that name on it.

``mode`` selects the attention of the same network on the same leaves:
    "diff"         DifferentialAttention
    "lambda_init"  the same with lambda frozen at lambda_init(l): the four lambda vectors do not enter
    "plain"        nn.MultiHeadDotProductAttention on the four kernels (masked softmax over 2 hd features, 1 / sqrt(2 hd), no RMSNorm)
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import hvla_ref_torch as ot

from diff_attention_ref import lambda_init_fn, mask_matrix


def diff_attention(h, wq, wk, wv, wo, lq1, lk1, lq2, lk2, sw, depth, H, mode="diff"):
    """h [B, S, D]; wq, wk, wv, wo [B, D, D]; lq1 .. lk2 [B, D / (2 H)]; sw [B, D / H] -> out_proj(subln((A1 - lambda A2) V)) [B, S, D]."""
    B, S, D = h.shape
    hd = D // (2 * H)
    q = torch.bmm(h, wq).reshape(B, S, H, 2, hd)
    k = torch.bmm(h, wk).reshape(B, S, H, 2, hd)
    v = torch.bmm(h, wv).reshape(B, S, H, 2 * hd).transpose(1, 2)                 # [B, H, S, 2 hd]
    if mode == "plain":
        keep = torch.as_tensor(mask_matrix(S))
        s = torch.einsum("bqhd,bkhd->bhqk", q.reshape(B, S, H, 2 * hd), k.reshape(B, S, H, 2 * hd)) / math.sqrt(2 * hd)
        o = torch.softmax(s.masked_fill(~keep, float("-inf")), -1) @ v
        return torch.bmm(o.transpose(1, 2).reshape(B, S, D), wo)
    M = torch.as_tensor(mask_matrix(S)).to(h.dtype)                                 # bool + float: True -> 1.0
    A = [torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q[:, :, :, c], k[:, :, :, c]) + M, -1) for c in range(2)]
    linit = lambda_init_fn(depth)
    if mode == "lambda_init":
        lam = torch.full((B,), linit, dtype=h.dtype)
    else:
        assert mode == "diff", mode
        lam = torch.exp((lq1 * lk1).sum(-1)) - torch.exp((lq2 * lk2).sum(-1)) + linit
    o = (A[0] - lam[:, None, None, None] * A[1]) @ v                                # [B, H, S, 2 hd]
    o = o * torch.rsqrt((o * o).mean(-1, keepdim=True) + 1e-5) * sw[:, None, None, :] * (1.0 - linit)
    return torch.bmm(o.transpose(1, 2).reshape(B, S, D), wo)


class PolicyDiffRef(ot.PolicyRef):
    """``oracle.hvla_ref_torch.PolicyRef`` with the attention of `mode` in every block: (actions, logits, lambda [B, L])."""

    def __init__(self, g, leaves, mode="diff"):
        super().__init__(g, leaves)
        self.mode = mode

    def __call__(self, theta, tokens, quant=None):
        assert quant is None
        g = self.g
        B, P, E = tokens.shape
        D, H = g.dim, g.heads
        lf = lambda n: self.leaf(theta, n)
        x = torch.bmm(tokens, lf("encoder_image_embedding_projection_kernel")) + lf("encoder_image_embedding_projection_bias")[:, None]
        x = torch.cat([x, torch.zeros(B, 1, D, dtype=x.dtype)], 1) + lf("encoder_pos_embedding")[:, 0]

        def ln(x, pre):
            s, b = lf(pre + "_scale")[:, None], lf(pre + "_bias")[:, None]
            return Fn.layer_norm(x, (D,), None, None, eps=1e-6) * s + b

        lams = []
        for l in range(g.layers):
            pb = f"encoder_Transformer_0_encoderblock_{l}_"
            pa = pb + g.attention_name + "_"
            h = ln(x, pb + "LayerNorm_0")
            lam4 = [lf(pa + n) for n in ("lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2")]
            lams.append(torch.exp((lam4[0] * lam4[1]).sum(-1)) - torch.exp((lam4[2] * lam4[3]).sum(-1)) + lambda_init_fn(l))
            x = x + diff_attention(h, lf(pa + "q_proj_kernel"), lf(pa + "k_proj_kernel"), lf(pa + "v_proj_kernel"),
                                   lf(pa + "out_proj_kernel"), *lam4, lf(pa + "subln_weight"), l, H, self.mode)
            y = ln(x, pb + "LayerNorm_1")
            y = Fn.gelu(torch.bmm(y, lf(pb + "MlpBlock_0_Dense_0_kernel")) + lf(pb + "MlpBlock_0_Dense_0_bias")[:, None], approximate="tanh")
            x = x + torch.bmm(y, lf(pb + "MlpBlock_0_Dense_1_kernel")) + lf(pb + "MlpBlock_0_Dense_1_bias")[:, None]
        x = ln(x, "encoder_Transformer_0_encoder_norm")
        emb = x[:, -1:]
        cont = torch.bmm(emb, lf("action_head_continuous_head_kernel"))[:, 0] + lf("action_head_continuous_head_bias")
        logit = torch.bmm(emb, lf("action_head_discrete_head_kernel"))[:, 0] + lf("action_head_discrete_head_bias")
        cont = torch.tanh(cont.reshape(B, g.horizon, g.action_dim - 1) / g.tanh_scale) * g.max_action
        act = torch.cat([cont, (logit >= 0).to(cont.dtype)[..., None]], -1)
        return act, logit, torch.stack(lams, 1)


def forward(params, g, leaves, instruction_dict, initial_state, tokens, mode="diff", dtype=torch.float64):
    """(actions [B, Hz, ad], logits [B, Hz], lambda [B, L]) from given tokens, no gradient."""
    with torch.no_grad():
        hn = ot.HyperNetRef(params, g, leaves, dtype)
        li = instruction_dict["language_instruction"]
        ctx = hn.context(li["token_embedding"], li["attention_mask"], np.asarray(initial_state["patch_embeddings"])[:, 0])
        return PolicyDiffRef(g, leaves, mode)(hn.generate(ctx), torch.as_tensor(np.asarray(tokens)).to(dtype))


def train_loss_and_grads(params, g, leaves, instruction_dict, initial_state, tokens, batch, mode="diff", dtype=torch.float64,
                         images=None, enc_shapes=None, clip_target=None):
    """``oracle.hvla_ref_torch.train_loss_and_grads`` on this policy: (per-sample loss [B], {leaf: d mean_b loss_b / d leaf},
    lambda [B, L]).  With `images` (and `enc_shapes`) the DINOv2 encoder is in the graph and its leaves are in the dict; otherwise
    the encoder is frozen and `tokens` are given."""
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
    act, logit, lam = PolicyDiffRef(g, leaves, mode)(theta, tok_t)
    if clip_target is None:
        clip_target = bool(getattr(g, "clip_target", True))
    per, loss = ot.mix_loss(g, act[..., :-1], logit, batch["action"], batch["timestep_pad_mask"], batch["action_pad_mask"],
                            clip_target=clip_target)
    wrt = [hn.p[k] for k in names]
    enc_named = list(enc.named_parameters()) if enc is not None else []
    grads = torch.autograd.grad(loss, wrt + [q for _, q in enc_named], allow_unused=True)
    out = {k: (gr.detach() if gr is not None else torch.zeros_like(hn.p[k])) for k, gr in zip(names, grads)}
    if enc is not None:
        hf = {n: (gr.detach() if gr is not None else torch.zeros_like(q)) for (n, q), gr in zip(enc_named, grads[len(wrt):])}
        out.update(ot._hf_grads_to_flax(hf, g))
    return per.detach(), out, lam.detach()


# ---------------------------------------------------------------------------------------------- the GPU cases' inputs
# One table for tests/test_gpu_diff_train.py (which runs the device) and tests/test_diff_train_host.py (which checks the conditions
# on the reference alone and measures the float32 floor): name -> (geometry name, B, train_encoder, batch seed).
CASES = {"mid": ("MID", 4, False, 2), "full": ("FULL", 2, False, 0), "mid_enc": ("MID", 2, True, 0)}
LAMBDA_X = 5.0                                          # diff_attention_ref.lambda_scaled: DESIGN.md §22's figure
TARGET_X = 0.1                                          # continuous targets x 0.1, as tests/test_gpu_mask_as_bias.py: smaller losses
LOSS_RTOL, LOSS_ATOL, LEAF_TOL = 3e-4, 3e-5, 2e-3       # train_parity's loss bounds, §20's fine-tune leaf bound


def case_geometry(name):
    import dataclasses
    from hypervla import config
    return dataclasses.replace(getattr(config, CASES[name][0]), differential=True)


def case_params(g):
    """The synthetic checkpoint with every lambda head x LAMBDA_X."""
    from hypervla import synthetic as syn
    import diff_attention_ref as DR
    return DR.lambda_scaled(syn.synthetic_params(g), LAMBDA_X)


def case_inputs(name):
    """(g, B, train_encoder, params, ins, st, x, batch): x = tokens [B, P, E] (encoder frozen) or uint8 images (trained)."""
    from hypervla import synthetic as syn
    _, B, enc, seed = CASES[name]
    g = case_geometry(name)
    params = case_params(g)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    batch = syn.synthetic_action_batch(B, g, seed)
    batch["action"][..., :-1] *= TARGET_X
    x = syn.synthetic_images(B, g) if enc else np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    return g, B, enc, params, ins, st, x, batch


def case_reference(name, mode="diff", dtype=torch.float64):
    """train_loss_and_grads on a case's inputs: (per, grads, lambda)."""
    from hypervla.config import encoder_leaves, generated_leaves
    g, B, enc, params, ins, st, x, batch = case_inputs(name)
    if enc:
        return train_loss_and_grads(params, g, generated_leaves(g), ins, st, None, batch, mode, dtype, images=x,
                                    enc_shapes=dict(encoder_leaves(g)))
    p = {k: v for k, v in params.items() if not k.startswith("encoder_image_encoder_")}
    return train_loss_and_grads(p, g, generated_leaves(g), ins, st, x, batch, mode, dtype)
