"""Float64 restatement of the hypernetwork with one layer token per policy module (hypernet_kwargs.share_layer_index=False,
`Geometry.layer_tokens`): HyperNetwork.generate_context_embedding and __call__ of the reference
(hypervla/components/hypernetwork.py:99-233) with the token table of HyperVLA.init_base_net (hypervla/model.py:393-436).

The dense layer, the Transformer and the LayerNorm are the oracle's (oracle/hvla_ref_np.py, which restates transformer.py); what the
oracle does not have -- NL layer tokens, their mask, the routing of every leaf to its token and the shared-head name rule -- is
stated here.  The token table itself comes from hypervla.config.layer_token_modules / token_of: it is held in one place."""
import numpy as np

from hypervla.config import generated_leaves, layer_token_modules, token_of
from oracle.hvla_ref_np import dense, layer_norm, transformer  # noqa: F401  (layer_norm: re-exported for the tests)

F = np.float64


def layer_token_mask(g):
    """model.py:399-436: False for the shared image encoder's token (index 0), True for every generated module."""
    return np.array([m != ("encoder", "image_encoder") for m in layer_token_modules(g)], bool)


def context_mask(attention_mask, lang_pad_mask, token_mask):
    """[B, 1, S, S], S = T + 1 + NL (hypernetwork.py:149-181 with attend_to_padding=False, task_attend_to_layer=False):
    language columns = attention mask & pad mask (:154-157), the image column all true (:161-163), layer column j =
    layer_token_mask[j] (:171-173) with the rows that are no layer queries cleared (:176-177)."""
    am = np.asarray(attention_mask).astype(bool)
    B, T = am.shape
    tm = np.asarray(token_mask, bool)
    NL = tm.shape[0]
    S = T + 1 + NL
    m = np.zeros((B, 1, S, S), bool)
    m[:, :, :, :T] = (am & np.asarray(lang_pad_mask).astype(bool)[:, None])[:, None, None, :]
    m[:, :, :, T] = True
    m[:, :, :, T + 1:] = tm[None, None, None, :]
    m[:, :, :S - NL, T + 1:] = False
    return m


def context_embedding(hp, g, token_embedding, attention_mask, init_cls, lang_pad_mask=None):
    """ctx [B, NL, C] (hypernetwork.py:104-197, dropout 0)."""
    tok = np.asarray(token_embedding, F)
    B = tok.shape[0]
    NL = len(layer_token_modules(g))
    if lang_pad_mask is None:
        lang_pad_mask = np.ones(B, bool)                                                     # model.py:69
    t = dense(tok, hp["task_token_projection/kernel"], hp["task_token_projection/bias"])
    t = t + np.asarray(hp["task_pos_embedding"], F)                                          # :112-115
    cls = np.asarray(init_cls, F).reshape(B, 1, -1)                                          # :126
    i = dense(cls, hp["initial_image_projection/kernel"], hp["initial_image_projection/bias"])
    i = i + np.asarray(hp["initial_image_pos_embedding"], F)                                 # :127
    pos = np.asarray(hp["layer_pos_embedding"], F)
    assert pos.shape == (1, NL, g.ctx_dim), pos.shape
    layer = np.zeros((B, NL, g.ctx_dim), F) + pos                                            # :144-145
    x = np.concatenate([t, i, layer], axis=1)                                                # :128,147
    mask = context_mask(attention_mask, lang_pad_mask, layer_token_mask(g))
    out = transformer(x, mask, hp, "Transformer_0/", g.ctx_layers, g.ctx_heads)
    ctx = out[:, -NL:]                                                                       # :188
    if g.scale_context:
        ctx = ctx / np.sqrt(g.ctx_dim)                                                       # :191-192
    return ctx


def head_of(g, lf):
    """The output head of a leaf: its own, or with share_TF_output_head the one named with encoderblock_<l> -> encoderblock
    (hypernetwork.py:221-225)."""
    return lf.shared_head_name if g.shared_block_heads else lf.head_name


def generate_base_params(hp, g, ctx):
    """Leaf p = Dense_p(ctx[:, token(p)]) (hypernetwork.py:205-217); {flat_name: [B, *shape]}."""
    out = {}
    for lf in generated_leaves(g):
        c = ctx[:, token_of(g, lf)]
        v = dense(c, hp[head_of(g, lf) + "/kernel"], hp[head_of(g, lf) + "/bias"])
        out[lf.flat_name] = v.reshape((c.shape[0],) + tuple(lf.shape))
    return out


def create_tasks(hp, g, instruction_dict, initial_state):
    """(base_params {flat_name: [B, *shape]}, ctx [B, NL, C], theta [B, G] in reference leaf order)."""
    li = instruction_dict["language_instruction"]
    ctx = context_embedding(hp, g, li["token_embedding"], li["attention_mask"], np.asarray(initial_state["patch_embeddings"])[:, 0])
    bp = generate_base_params(hp, g, ctx)
    theta = np.concatenate([bp[l.flat_name].reshape(ctx.shape[0], -1) for l in generated_leaves(g)], 1)
    return bp, ctx, theta
