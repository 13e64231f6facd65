"""Float64 torch restatement of the fine-tune step under hvla_train_noise_set (test infrastructure, like oracle/): the gradient
oracle of tests/test_gpu_train_noise.py.

``NoisyPolicyRef`` restates ``oracle.hvla_ref_torch.PolicyRef.__call__`` (and, with language tokens, tests/lang_policy_torch.py's
``LangPolicyRef.__call__``) with the dropout multipliers of hypervla.train's numpy generator at the four policy sites
(reference base_vit.py:204-205, transformer.py:67,74,192).  ``train_loss_and_grads`` feeds ``HyperNetRef.context`` / ``generate``
(imported, not edited) the masked CLS row (hypernetwork.py:119-122), masks the context embedding between the two
(hypernetwork.py:193-195), and gives the policy ``tokens + sigma z`` with z from the float64 Box-Muller (base_vit.py:123-127).
A multiplier is 1 / keep_prob in float64 on the float32 keep_prob = 1 - rate the device divides by.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

from hypervla import train as T
from lang_policy_torch import policy_keep
from oracle import hvla_ref_torch as ot


class Noise:
    """One hvla_train_noise setting; `mult(kind, layer, shape)` / `normals(shape)` -> float64 [B, *shape] for rows sample_offset + b."""

    def __init__(self, B, policy_dropout=0.0, image_embedding_noise=0.0, context_dropout=0.0, image_dropout=0.0, seed=0,
                 sample_offset=0, draw=0):
        self.B, self.seed, self.offset, self.draw = B, seed, sample_offset, draw
        self.sigma = float(image_embedding_noise)
        self.rate = {T.NOISE_POLICY_INPUT: policy_dropout, T.NOISE_ATTN_OUT: policy_dropout, T.NOISE_MLP_HIDDEN: policy_dropout,
                     T.NOISE_MLP_OUT: policy_dropout, T.NOISE_CONTEXT: context_dropout, T.NOISE_IMAGE_CLS: image_dropout}

    def mult(self, kind, layer, shape):
        rate, n = self.rate[kind], int(np.prod(shape))
        if rate == 0.0:
            return torch.ones((self.B,) + tuple(shape), dtype=torch.float64)
        kp = float(np.float32(1.0) - np.float32(rate))
        rows = [T.noise_multipliers(rate, self.seed, T.noise_site(kind, layer), self.offset + b, self.draw, n) > 0 for b in range(self.B)]
        return torch.as_tensor(np.stack(rows).astype(np.float64) / kp).reshape((self.B,) + tuple(shape))

    def normals(self, shape):
        n = int(np.prod(shape))
        rows = [T.noise_normals(self.seed, T.noise_site(T.NOISE_TOKENS), self.offset + b, self.draw, n) for b in range(self.B)]
        return torch.as_tensor(np.stack(rows)).reshape((self.B,) + tuple(shape))


class NoisyPolicyRef(ot.PolicyRef):
    """PolicyRef.__call__ / LangPolicyRef.__call__ (`lang_tokens` [B, T, lang_dim] or None) with the policy's dropout."""

    def __call__(self, theta, tokens, nz, lang_tokens=None):
        g = self.g
        B, P, E = tokens.shape
        T_ = 0 if lang_tokens is None else lang_tokens.shape[1]
        D, H, hd, M = g.dim, g.heads, g.head_dim, g.mlp
        lf = lambda n: self.leaf(theta, n)
        x = torch.bmm(tokens, lf("encoder_image_embedding_projection_kernel")) + lf("encoder_image_embedding_projection_bias")[:, None]
        if T_:
            t = torch.bmm(lang_tokens, lf("encoder_language_token_projection_kernel")) + lf("encoder_language_token_projection_bias")[:, None]
            x = torch.cat([t, x], 1)
        x = torch.cat([x, torch.zeros(B, 1, D, dtype=x.dtype)], 1) + lf("encoder_pos_embedding")[:, 0]
        S = T_ + P + 1
        x = x * nz.mult(T.NOISE_POLICY_INPUT, 0, (S, D))
        keep = policy_keep(T_, P)

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
            y = torch.bmm(o, lf(pa + "out_kernel").reshape(B, D, D)) + lf(pa + "out_bias")[:, None]
            x = x + y * nz.mult(T.NOISE_ATTN_OUT, l, (S, D))
            y = ln(x, pb + "LayerNorm_1")
            y = Fn.gelu(torch.bmm(y, lf(pb + "MlpBlock_0_Dense_0_kernel")) + lf(pb + "MlpBlock_0_Dense_0_bias")[:, None], approximate="tanh")
            y = y * nz.mult(T.NOISE_MLP_HIDDEN, l, (S, M))
            y = torch.bmm(y, lf(pb + "MlpBlock_0_Dense_1_kernel")) + lf(pb + "MlpBlock_0_Dense_1_bias")[:, None]
            x = x + y * nz.mult(T.NOISE_MLP_OUT, l, (S, D))
        x = ln(x, "encoder_Transformer_0_encoder_norm")
        emb = x[:, -1:]
        cont = torch.bmm(emb, lf("action_head_continuous_head_kernel"))[:, 0] + lf("action_head_continuous_head_bias")
        logit = torch.bmm(emb, lf("action_head_discrete_head_kernel"))[:, 0] + lf("action_head_discrete_head_bias")
        cont = torch.tanh(cont.reshape(B, g.horizon, g.action_dim - 1) / g.tanh_scale) * g.max_action
        act = torch.cat([cont, (logit >= 0).to(cont.dtype)[..., None]], -1)
        return act, logit, emb[:, 0]


def train_loss_and_grads(params, g, leaves, instruction_dict, initial_state, tokens, batch, nz, images=None, enc_shapes=None):
    """(per-sample loss [B], mean loss, {leaf: gradient}) in float64, composed as oracle.hvla_ref_torch.train_loss_and_grads composes
    the noise-free step.  `nz`: Noise.  A use_language_token geometry gets the instruction's token embeddings as the policy's prefix."""
    dtype = torch.float64
    hn = ot.HyperNetRef(params, g, leaves, dtype)
    names = sorted(hn.p)
    for k in names:
        hn.p[k] = hn.p[k].clone().requires_grad_(True)
    hn.w_cat = torch.cat([hn.p[l.head_name + "/kernel"] for l in leaves], dim=1)
    hn.b_cat = torch.cat([hn.p[l.head_name + "/bias"] for l in leaves], dim=0)
    li = instruction_dict["language_instruction"]
    cls = torch.as_tensor(np.asarray(initial_state["patch_embeddings"])[:, 0]).to(dtype) * nz.mult(T.NOISE_IMAGE_CLS, 0, (g.enc_dim,))
    ctx = hn.context(li["token_embedding"], li["attention_mask"], cls)
    ctx = ctx * nz.mult(T.NOISE_CONTEXT, 0, (g.ctx_dim,))
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
    if nz.sigma > 0:
        tok_t = tok_t + float(np.float32(nz.sigma)) * nz.normals((g.patches, g.enc_dim))
    lang = torch.as_tensor(np.asarray(li["token_embedding"])).to(dtype) if getattr(g, "lang_in_policy", False) else None
    act, logit, _ = NoisyPolicyRef(g, leaves)(theta, tok_t, nz, lang)
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
