// train_layout.h — flat layout of the trainable parameter vector (hvla_train_*).  No HIP types: train.hip, api.hip, the layout of
// the serving buffers (serving_layout.h) and its CPU check (tests/native/publish_map_check.cpp) share this one text.
#pragma once
#include <stdint.h>

#include "layout.h"

namespace hvla {

// The leaves of ONE transformer block, as offsets into whatever holds it: the context encoder's blocks in the hypernetwork's
// part of the vector, DINOv2's blocks in the shared part, the generated policy's blocks in a row of theta -- and, in the serving
// tables (serving_layout.h), the same members as offsets into the serving buffers.  ls1 / ls2 (LayerScale): DINOv2 only, else -1.
struct BlockLeaves { long ln0_s, ln0_b, wq, bq, wk, bk, wv, bv, wo, bo, ln1_s, ln1_b, w1, b1, w2, b2, ls1, ls2; };

// What a DifferentialAttention block (Geom::differential) has besides q_proj / k_proj / v_proj / out_proj, which take
// wq / wk / wv / wo above with bq = bk = bv = bo = -1: the four lambda vectors [D / (2 H)] and subln/weight [D / H], in a row of theta.
struct DiffLeaves { long lq1, lk1, lq2, lk2, sw; };

// flat layout of the trainable hypernetwork parameters (float32 elements)
// `total` = the hypernetwork's own parameters; the shared DINOv2 leaves follow at [total, total + enc_total) when the
// image encoder is trained too (`fine_tune_pretrained_image_encoder=True`), in hypervla.config.encoder_leaves order.
// wp .. bd and pol[]: the generated policy's leaves in a row of theta [G] (generated_leaves order, by flax name).
struct TrainLayout {
  long w_tok, b_tok, w_img, b_img, pos_tok, pos_img, pos_layer, norm_s, norm_b, wcat, bcat, total, G;
  BlockLeaves layer[CTX_MAX_LAYERS];
  long e_cls, e_mask, e_pb, e_pk, e_pos, e_lnb, e_lns, enc_total;
  BlockLeaves enc[ENC_MAX_LAYERS];
  long wp, bp, pos, ns, nb, wc, bc, wd, bd;
  BlockLeaves pol[TRAIN_MAX_POLICY_LAYERS];
  bool policy_ok;          // every policy leaf above was found by its name (false beyond TRAIN_MAX_POLICY_LAYERS, which the serving
                           // tables may be built for: they do not read the policy's offsets)
  long wl, bl;             // encoder_language_token_projection_{kernel,bias} in a row of theta (use_language_token; else -1).  L.pos then
                           // spans g.pos_rows() = T + P + 1 rows
  DiffLeaves dif[TRAIN_MAX_POLICY_LAYERS];   // use_differential_transformer: the five leaves a block has besides its four kernels (else all -1)
};

// nullptr, or why the training path (hvla_train_*) does not serve a geometry hvla_create accepted (HVLA_E_SHAPE with this text).
// The first two answers are the default: hvla_train_differential(ctx, 1) / hvla_train_language_tokens(ctx, 1) lift them for that
// context (train_entry, api.hip)
inline const char* train_refusal(const Geom& g) {
  if (g.layer_tokens) return "the training path does not build hypernet_kwargs.share_layer_index=False (one layer token per policy module): serving is";
  if (g.differential) return "the training path does not build use_differential_transformer (DifferentialAttention): serving is";
  if (g.lang_in_policy) return "the training path does not build use_language_token";
  if (g.ctx_layers > CTX_MAX_LAYERS || g.L > TRAIN_MAX_POLICY_LAYERS || g.enc_layers > ENC_MAX_LAYERS) return "too many layers for the training path";
  return nullptr;
}
// ... and the same question for a context whose caller asked for the language prefix (language_tokens): what else stands against it
inline const char* train_refusal(const Geom& g, bool language_tokens) {
  if (!language_tokens || !g.lang_in_policy) return train_refusal(g);
  Geom plain = g;
  plain.lang_in_policy = 0;
  return train_refusal(plain);
}
// ... and for a context whose caller asked for DifferentialAttention's backward (differential; hvla_train_differential)
inline const char* train_refusal(const Geom& g, bool language_tokens, bool differential) {
  if (!differential || !g.differential) return train_refusal(g, language_tokens);
  Geom plain = g;
  plain.differential = 0;
  return train_refusal(plain, language_tokens);
}
inline TrainLayout make_train_layout(const Geom& g) {
  TrainLayout L{};
  long o = 0;
  auto add = [&](long& slot, long n) { slot = o; o += n; };
  const int C = g.C, F = g.ctx_mlp;
  add(L.w_tok, (long)g.lang_dim * C); add(L.b_tok, C); add(L.w_img, (long)g.E * C); add(L.b_img, C);
  add(L.pos_tok, (long)g.T * C); add(L.pos_img, C); add(L.pos_layer, C);
  for (int l = 0; l < g.ctx_layers; ++l) {
    BlockLeaves& c = L.layer[l];
    add(c.ln0_s, C); add(c.ln0_b, C); add(c.ln1_s, C); add(c.ln1_b, C);
    add(c.wq, (long)C * C); add(c.bq, C); add(c.wk, (long)C * C); add(c.bk, C); add(c.wv, (long)C * C); add(c.bv, C);
    add(c.wo, (long)C * C); add(c.bo, C); add(c.w1, (long)C * F); add(c.b1, F); add(c.w2, (long)F * C); add(c.b2, C);
    c.ls1 = c.ls2 = -1;
  }
  add(L.norm_s, C); add(L.norm_b, C);
  const std::vector<LeafInfo> leaves = generated_leaves(g);
  L.G = leaves.back().offset + leaves.back().size;
  add(L.wcat, (long)C * L.G); add(L.bcat, L.G);
  L.total = o;
  // shared DINOv2 leaves, hypervla.config.encoder_leaves order, offsets relative to L.total
  o = 0;
  const long E = g.E, Fe = g.enc_mlp, Se = g.P() + 1;
  add(L.e_cls, E); add(L.e_mask, E); add(L.e_pb, E); add(L.e_pk, (long)g.patch * g.patch * 3 * E); add(L.e_pos, Se * E);
  for (int l = 0; l < g.enc_layers; ++l) {
    BlockLeaves& y = L.enc[l];
    add(y.bk, E); add(y.wk, E * E); add(y.bq, E); add(y.wq, E * E); add(y.bv, E); add(y.wv, E * E); add(y.bo, E); add(y.wo, E * E);
    add(y.ls1, E); add(y.ls2, E); add(y.b1, Fe); add(y.w1, E * Fe); add(y.b2, E); add(y.w2, Fe * E);
    add(y.ln0_b, E); add(y.ln0_s, E); add(y.ln1_b, E); add(y.ln1_s, E);
  }
  add(L.e_lnb, E); add(L.e_lns, E);
  L.enc_total = o;
  // the generated policy, each leaf by its flax name
  L.policy_ok = g.L <= TRAIN_MAX_POLICY_LAYERS;
  auto f = [&](const std::string& n) {
    for (const LeafInfo& l : leaves) if (l.flat == n) return (long)l.offset;
    L.policy_ok = false;
    return -1L;
  };
  L.bc = f("action_head_continuous_head_bias"); L.wc = f("action_head_continuous_head_kernel");
  L.bd = f("action_head_discrete_head_bias"); L.wd = f("action_head_discrete_head_kernel");
  L.nb = f("encoder_Transformer_0_encoder_norm_bias"); L.ns = f("encoder_Transformer_0_encoder_norm_scale");
  L.bp = f("encoder_image_embedding_projection_bias"); L.wp = f("encoder_image_embedding_projection_kernel");
  L.pos = f("encoder_pos_embedding");
  L.wl = g.lang_in_policy ? f("encoder_language_token_projection_kernel") : -1;
  L.bl = g.lang_in_policy ? f("encoder_language_token_projection_bias") : -1;
  for (int l = 0; l < g.L && l < TRAIN_MAX_POLICY_LAYERS; ++l) {
    const std::string B = "encoder_Transformer_0_encoderblock_" + std::to_string(l) + "_", A = B + g.attention_name();
    BlockLeaves& y = L.pol[l];
    y.ln0_b = f(B + "LayerNorm_0_bias"); y.ln0_s = f(B + "LayerNorm_0_scale"); y.ln1_b = f(B + "LayerNorm_1_bias"); y.ln1_s = f(B + "LayerNorm_1_scale");
    y.b1 = f(B + "MlpBlock_0_Dense_0_bias"); y.w1 = f(B + "MlpBlock_0_Dense_0_kernel");
    y.b2 = f(B + "MlpBlock_0_Dense_1_bias"); y.w2 = f(B + "MlpBlock_0_Dense_1_kernel");
    DiffLeaves& d = L.dif[l];
    d.lq1 = d.lk1 = d.lq2 = d.lk2 = d.sw = -1;
    if (g.differential) {      // four bias-free Dense(D) and five vectors (differential_transformer.py:139-156)
      y.wk = f(A + "k_proj_kernel"); y.wo = f(A + "out_proj_kernel"); y.wq = f(A + "q_proj_kernel"); y.wv = f(A + "v_proj_kernel");
      y.bk = y.bo = y.bq = y.bv = -1;
      d.lk1 = f(A + "lambda_k1"); d.lk2 = f(A + "lambda_k2"); d.lq1 = f(A + "lambda_q1"); d.lq2 = f(A + "lambda_q2");
      d.sw = f(A + "subln_weight");
    } else {
      y.bk = f(A + "key_bias"); y.wk = f(A + "key_kernel"); y.bo = f(A + "out_bias"); y.wo = f(A + "out_kernel");
      y.bq = f(A + "query_bias"); y.wq = f(A + "query_kernel"); y.bv = f(A + "value_bias"); y.wv = f(A + "value_kernel");
    }
    y.ls1 = y.ls2 = -1;
  }
  return L;
}

}  // namespace hvla
