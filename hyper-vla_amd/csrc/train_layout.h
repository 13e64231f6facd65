// train_layout.h — flat layout of the trainable parameter vector (hvla_train_*).  No HIP types: train.hip, api.hip, the layout of
// the serving buffers (serving_layout.h) and its CPU check (tests/native/publish_map_check.cpp) share this one text.
#pragma once
#include <stdint.h>

#include "layout.h"

namespace hvla {

// flat layout of the trainable hypernetwork parameters (float32 elements)
// `total` = the hypernetwork's own parameters; the shared DINOv2 leaves follow at [total, total + enc_total) when the
// image encoder is trained too (`fine_tune_pretrained_image_encoder=True`), in hypervla.config.encoder_leaves order.
struct TrainLayout {
  long w_tok, b_tok, w_img, b_img, pos_tok, pos_img, pos_layer, norm_s, norm_b, wcat, bcat, total, G;
  struct CL { long ln0_s, ln0_b, ln1_s, ln1_b, wq, bq, wk, bk, wv, bv, wo, bo, w1, b1, w2, b2; } layer[8];
  long e_cls, e_mask, e_pb, e_pk, e_pos, e_lnb, e_lns, enc_total;
  struct EL { long kb, kk, qb, qk, vb, vk, ob, ok, ls1, ls2, f1b, f1k, f2b, f2k, n1b, n1s, n2b, n2s; } enc[24];
};
inline TrainLayout make_train_layout(const Geom& g) {
  TrainLayout L{};
  long o = 0;
  auto add = [&](long& slot, long n) { slot = o; o += n; };
  const int C = g.C, F = g.ctx_mlp;
  add(L.w_tok, (long)g.lang_dim * C); add(L.b_tok, C); add(L.w_img, (long)g.E * C); add(L.b_img, C);
  add(L.pos_tok, (long)g.T * C); add(L.pos_img, C); add(L.pos_layer, C);
  for (int l = 0; l < g.ctx_layers; ++l) {
    TrainLayout::CL& c = L.layer[l];
    add(c.ln0_s, C); add(c.ln0_b, C); add(c.ln1_s, C); add(c.ln1_b, C);
    add(c.wq, (long)C * C); add(c.bq, C); add(c.wk, (long)C * C); add(c.bk, C); add(c.wv, (long)C * C); add(c.bv, C);
    add(c.wo, (long)C * C); add(c.bo, C); add(c.w1, (long)C * F); add(c.b1, F); add(c.w2, (long)F * C); add(c.b2, C);
  }
  add(L.norm_s, C); add(L.norm_b, C);
  L.G = generated_leaves(g).back().offset + generated_leaves(g).back().size;
  add(L.wcat, (long)C * L.G); add(L.bcat, L.G);
  L.total = o;
  // shared DINOv2 leaves, hypervla.config.encoder_leaves order, offsets relative to L.total
  o = 0;
  const long E = g.E, Fe = g.enc_mlp, Se = g.P() + 1;
  add(L.e_cls, E); add(L.e_mask, E); add(L.e_pb, E); add(L.e_pk, (long)g.patch * g.patch * 3 * E); add(L.e_pos, Se * E);
  for (int l = 0; l < g.enc_layers; ++l) {
    TrainLayout::EL& y = L.enc[l];
    add(y.kb, E); add(y.kk, E * E); add(y.qb, E); add(y.qk, E * E); add(y.vb, E); add(y.vk, E * E); add(y.ob, E); add(y.ok, E * E);
    add(y.ls1, E); add(y.ls2, E); add(y.f1b, Fe); add(y.f1k, E * Fe); add(y.f2b, E); add(y.f2k, Fe * E);
    add(y.n1b, E); add(y.n1s, E); add(y.n2b, E); add(y.n2s, E);
  }
  add(L.e_lnb, E); add(L.e_lns, E);
  L.enc_total = o;
  return L;
}

}  // namespace hvla
