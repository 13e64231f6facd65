"""Torch float64 autograd restatement of the hypernetwork with one layer token per policy module (``Geometry.layer_tokens``;
test infrastructure, like oracle/): the gradient oracle of FineTuner(layer_tokens=True).

It is ``tests/layer_tokens_ref.py`` restated in torch on top of ``oracle.hvla_ref_torch``: ``LayerTokenHyperNet`` is the oracle's
``HyperNetRef`` -- its Transformer block, its projections -- with NL layer rows, their mask, the final norm over the last NL rows
and every leaf generated from the context row of its module's token through its own (or, with ``shared_block_heads``, the blocks'
shared) output head.  The token table and the head names come from ``hypervla.config`` (``token_of``, ``Leaf.shared_head_name``), the
mask from ``layer_tokens_ref.context_mask``: each is held in one place.  The policy is the oracle's, ``lang_policy_torch``'s under
``use_language_token`` or ``diff_train_ref``'s under ``use_differential_transformer``.

``train_loss_and_grads`` has the signature and the result of ``oracle.hvla_ref_torch.train_loss_and_grads``, so
``tests/train_parity.py``'s metrics apply to it."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as Fn

from hypervla.config import layer_token_modules, token_of
from oracle import hvla_ref_torch as ot

import layer_tokens_ref as LR


class LayerTokenHyperNet(ot.HyperNetRef):
    def __init__(self, params, g, leaves, dtype=torch.float64):
        # (not the base constructor: it fuses the heads under `head_name`, which a shared head does not have)
        self.g, self.leaves, self.dt = g, leaves, dtype
        self.p = {k: ot._t(v, dtype) for k, v in params.items() if not k.startswith("encoder_image_encoder_")}

    def context(self, token_embedding, attention_mask, init_cls, quant=None):
        """ctx [B, NL, C] (hypernetwork.py:104-197, dropout 0)."""
        g, p = self.g, self.p
        tok = ot._t(token_embedding, self.dt)
        B, T, _ = tok.shape
        NL = len(layer_token_modules(g))
        x_lang = ot._mm(tok, p["task_token_projection/kernel"], quant) + p["task_token_projection/bias"] + p["task_pos_embedding"]
        x_img = ot._mm(ot._t(init_cls, self.dt).reshape(B, 1, -1), p["initial_image_projection/kernel"], quant) \
            + p["initial_image_projection/bias"] + p["initial_image_pos_embedding"]
        assert tuple(p["layer_pos_embedding"].shape) == (1, NL, g.ctx_dim)
        x = torch.cat([x_lang, x_img, p["layer_pos_embedding"].expand(B, NL, -1)], 1)
        keep = torch.as_tensor(LR.context_mask(attention_mask, np.ones(B, bool), LR.layer_token_mask(g)))
        for l in range(g.ctx_layers):
            x = self._block(x, keep, l, g.ctx_heads, quant)
        x = Fn.layer_norm(x, (g.ctx_dim,), p["Transformer_0/encoder_norm/scale"], p["Transformer_0/encoder_norm/bias"], eps=1e-6)
        ctx = x[:, -NL:]
        return ctx / math.sqrt(g.ctx_dim) if g.scale_context else ctx

    def generate(self, ctx, quant=None):
        """theta [B, G] in reference leaf order: leaf p = Dense_p(ctx[:, token(p)])."""
        out = []
        for lf in self.leaves:
            head = LR.head_of(self.g, lf)
            out.append(ot._mm(ctx[:, token_of(self.g, lf)], self.p[head + "/kernel"], quant) + self.p[head + "/bias"])
        return torch.cat(out, 1)


def forward(params, g, leaves, instruction_dict, initial_state, dtype=torch.float64):
    """(ctx [B, NL, C], theta [B, G]) without gradients: what layer_tokens_ref.create_tasks returns as its last two."""
    with torch.no_grad():
        hn = LayerTokenHyperNet(params, g, leaves, dtype)
        li = instruction_dict["language_instruction"]
        ctx = hn.context(li["token_embedding"], li["attention_mask"], np.asarray(initial_state["patch_embeddings"])[:, 0])
        return ctx, hn.generate(ctx)


def _policy(g, leaves, theta, tok_t, lang):
    if getattr(g, "differential", False):
        import diff_train_ref as DT
        act, logit, _ = DT.PolicyDiffRef(g, leaves)(theta, tok_t)
    elif getattr(g, "lang_in_policy", False):
        import lang_policy_torch as LT
        act, logit, _ = LT.LangPolicyRef(g, leaves)(theta, tok_t, lang)
    else:
        act, logit, _ = ot.PolicyRef(g, leaves)(theta, tok_t)
    return act, logit


def train_loss_and_grads(params, g, leaves, instruction_dict, initial_state, tokens, batch, dtype=torch.float64,
                         images=None, enc_shapes=None, clip_target=None, keep_theta=None):
    """(per-sample loss [B], mean loss, {leaf: d mean_b loss_b / d leaf}) by autograd through the layer-token hypernetwork -> theta ->
    per-sample policy -> mix loss.  A shared head appears once, under its ``encoderblock`` name; its gradient is the sum over the
    blocks.  `keep_theta` (a dict, optional) receives theta, d loss / d theta and d loss / d ctx."""
    hn = LayerTokenHyperNet(params, g, leaves, dtype)
    names = sorted(hn.p)
    for k in names:
        hn.p[k] = hn.p[k].clone().requires_grad_(True)
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
    act, logit = _policy(g, leaves, theta, tok_t, lang)
    if clip_target is None:
        clip_target = bool(getattr(g, "clip_target", True))
    per, loss = ot.mix_loss(g, act[..., :-1], logit, batch["action"], batch["timestep_pad_mask"], batch["action_pad_mask"],
                            clip_target=clip_target)
    wrt = [hn.p[k] for k in names]
    enc_named = list(enc.named_parameters()) if enc is not None else []
    extra = [theta, ctx] if keep_theta is not None else []
    grads = torch.autograd.grad(loss, wrt + [q for _, q in enc_named] + extra, allow_unused=True)
    out = {k: (gr.detach() if gr is not None else torch.zeros_like(hn.p[k])) for k, gr in zip(names, grads)}
    if enc is not None:
        hf = {n: (gr.detach() if gr is not None else torch.zeros_like(q))
              for (n, q), gr in zip(enc_named, grads[len(wrt):len(wrt) + len(enc_named)])}
        out.update(ot._hf_grads_to_flax(hf, g))
    if keep_theta is not None:
        keep_theta.update(theta=theta.detach(), dtheta=grads[-2].detach(), dctx=grads[-1].detach())
    return per.detach(), loss.detach(), out
