// train_layout.h — flat layout of the trainable parameter vector (hvla_train_*).  No HIP types: train.hip, api.hip, the layout of
// the serving buffers (serving_layout.h) and its CPU check (tests/native/publish_map_check.cpp) share this one text.
// With Geom::layer_tokens pos_layer has NL rows, the heads are [C][Gh] / [Gh] with Gh <= G (shared block heads are ONE
// tensor), and the run table says which context token and which head columns a range of theta columns reads; the tiles of the three
// grouped weight-generation products (train.h bgemm_groups) are cut from that table here, so that a CPU check sees what the device gets.
#pragma once
#include <stdint.h>

#include <utility>

#include "layout.h"

namespace hvla {

// The leaves of ONE transformer block, as offsets into whatever holds it: the context encoder's blocks in the hypernetwork's
// part of the vector, DINOv2's blocks in the shared part, the generated policy's blocks in a row of theta -- and, in the serving
// tables (serving_layout.h), the same members as offsets into the serving buffers.  ls1 / ls2 (LayerScale): DINOv2 only, else -1.
struct BlockLeaves { long ln0_s, ln0_b, wq, bq, wk, bk, wv, bv, wo, bo, ln1_s, ln1_b, w1, b1, w2, b2, ls1, ls2; };

// What a DifferentialAttention block (Geom::differential) has besides q_proj / k_proj / v_proj / out_proj, which take
// wq / wk / wv / wo above with bq = bk = bv = bo = -1: the four lambda vectors [D / (2 H)] and subln/weight [D / H], in a row of theta.
struct DiffLeaves { long lq1, lk1, lq2, lk2, sw; };

// One maximal run of theta columns [tcol, tcol + width) that reads ONE context token and the contiguous head columns
// [hcol, hcol + width): with layer tokens one per generated module (NL - 1 in all), in generated_leaves order -- action_head,
// encoder_norm, the blocks, the projections, pos_embedding.  With shared_block_heads the L blocks' runs have one hcol.
struct TokenRun { long tcol, width, hcol; int token; };
constexpr int TRAIN_MAX_RUNS = TRAIN_MAX_POLICY_LAYERS + 5;     // NL - 1 at TRAIN_MAX_POLICY_LAYERS with use_language_token

// One workgroup column of a grouped product (bgemm_groups, train.h): element offsets added to the launch's A, B, C and bias, the
// tile's column origin n0 inside an operand of N columns (blockIdx.z adds whole tiles), and its K range [k0, k1) (k1 = 0: the launch's K).  A tile never
// spans two runs; a run's last tile is a partial tile (n0 + tile > N).
struct BGTile { long a, b, c, bias; int n0, N, k0, k1; };

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
  // layer_tokens (else NL = 1, Gh = G, nruns = 0): pos_layer is [NL][C], wcat [C][Gh], bcat [Gh]
  int NL, nruns;
  long Gh;
  TokenRun run[TRAIN_MAX_RUNS];
};

// nullptr, or why the training path (hvla_train_*) does not serve a geometry hvla_create accepted (HVLA_E_SHAPE with this text).
// The first three answers are the default: hvla_train_layer_tokens(ctx, 1) / hvla_train_differential(ctx, 1) /
// hvla_train_language_tokens(ctx, 1) lift them for that context (train_entry, api.hip)
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
// ... and for a context whose caller asked for the layer tokens (layer_tokens; hvla_train_layer_tokens)
inline const char* train_refusal(const Geom& g, bool language_tokens, bool differential, bool layer_tokens) {
  if (!layer_tokens || !g.layer_tokens) return train_refusal(g, language_tokens, differential);
  Geom plain = g;
  plain.layer_tokens = plain.shared_block_heads = 0;
  return train_refusal(plain, language_tokens, differential);
}
inline TrainLayout make_train_layout(const Geom& g) {
  TrainLayout L{};
  long o = 0;
  auto add = [&](long& slot, long n) { slot = o; o += n; };
  const int C = g.C, F = g.ctx_mlp;
  add(L.w_tok, (long)g.lang_dim * C); add(L.b_tok, C); add(L.w_img, (long)g.E * C); add(L.b_img, C);
  add(L.pos_tok, (long)g.T * C); add(L.pos_img, C); add(L.pos_layer, (long)g.NL() * C);
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
  L.NL = g.NL(); L.nruns = 0; L.Gh = L.G;
  bool runs_ok = true;
  if (g.layer_tokens) {      // the run table, from layer_token_of and output_head_of alone: the string order of encoderblock_10 falls out of them
    std::vector<std::pair<std::string, long>> heads;
    long hc = 0;
    for (const LeafInfo& l : leaves) {
      const int token = layer_token_of(g, l.flat);
      const std::string head = output_head_of(g, l.flat);
      long h = -1;
      for (const auto& e : heads) if (e.first == head) h = e.second;
      if (h < 0) { h = hc; heads.push_back({head, h}); hc += l.size; }
      TokenRun* r = L.nruns ? &L.run[L.nruns - 1] : nullptr;
      if (r && r->token == token && r->tcol + r->width == l.offset && r->hcol + r->width == h) { r->width += l.size; continue; }
      if (L.nruns == TRAIN_MAX_RUNS) { runs_ok = false; break; }       // beyond TRAIN_MAX_POLICY_LAYERS: train_refusal's answer
      L.run[L.nruns++] = TokenRun{(long)l.offset, (long)l.size, h, token};
    }
    L.Gh = hc;
  }
  add(L.wcat, (long)C * L.Gh); add(L.bcat, L.Gh);
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
  L.policy_ok = g.L <= TRAIN_MAX_POLICY_LAYERS && runs_ok;
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

// The tiles of the three grouped products of a layer-token layout, `tile` columns wide (64 / 128), in run order:
//   kind 0  theta[:, run] = ctx[:, token] W_h[:, hcols] + b_h[hcols]     A = ctx [B][NL C], B = W_h [C][Gh], C = theta [B][G], bias = b_h
//   kind 1  dW_h[:, hcols] += ctx[:, token]^T dtheta[:, run]              A = ctx (transposed), B = dtheta [B][G], C = dW_h [C][Gh]
//   kind 2  dctx[:, token] = dtheta[:, run] W_h[:, hcols]^T               A = dtheta, B = W_h (transposed), C = dctx [B][NL C]; split-K: one
//           entry per K chunk of `tile` = kchunk (a multiple of 32) columns of a run, N = C whole (blockIdx.z walks it)
// K of kinds 0 / 1 (C, B) is the launch's: k1 = 0 stands for BG::K, so no table depends on the batch.
inline std::vector<BGTile> group_tiles(const Geom& g, const TrainLayout& L, int kind, int tile) {
  std::vector<BGTile> v;
  for (int i = 0; i < L.nruns; ++i) {
    const TokenRun& r = L.run[i];
    const long tok = (long)r.token * g.C;
    for (long n0 = 0; n0 < r.width; n0 += tile) {
      if (kind == 0) v.push_back(BGTile{tok, r.hcol, r.tcol, r.hcol, (int)n0, (int)r.width, 0, 0});
      else if (kind == 1) v.push_back(BGTile{tok, r.tcol, r.hcol, 0, (int)n0, (int)r.width, 0, 0});
      else v.push_back(BGTile{r.tcol, r.hcol, tok, 0, 0, g.C, (int)n0, (int)(n0 + tile < r.width ? n0 + tile : r.width)});
    }
  }
  return v;
}
// the K chunk of kind 2: about 512 workgroups per tile of the output (bgemm()'s want_split), whole 32-float k steps, at least 128
inline int group_kchunk(const TrainLayout& L) {
  const long k = ((L.G + 511) / 512 + 31) / 32 * 32;
  return (int)(k < 128 ? 128 : k);
}
// float4 staging of the grouped products: every origin and width a multiple of 4 floats
inline bool group_vec_ok(const Geom& g, const TrainLayout& L) {
  bool ok = g.C % 4 == 0 && L.G % 4 == 0 && L.Gh % 4 == 0;
  for (int i = 0; i < L.nruns; ++i) ok = ok && L.run[i].tcol % 4 == 0 && L.run[i].width % 4 == 0 && L.run[i].hcol % 4 == 0;
  return ok;
}

}  // namespace hvla
