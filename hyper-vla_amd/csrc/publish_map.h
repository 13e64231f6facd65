// publish_map.h — the index maps of hvla_train_publish (publish.hip): where every element of the flat training vector
// (train_layout.h) goes in the device buffers hvla_load_weights fills (api.hip).  No HIP types: the kernels and the CPU check
// (tests/native/publish_map_check.cpp, which runs the same tables against pack.h and a transcription of the load order) share
// this text.  Every table is a plain struct that a kernel takes by value: the publish allocates and uploads nothing.
//
// The training vector and the load order are both regular per layer, so a table holds the segments of layer 0 plus one source
// and one destination stride; a segment with per_layer == 0 exists once.
#pragma once
#include <stdint.h>

#include "layout.h"
#include "pack.h"
#include "train_layout.h"

namespace hvla {
namespace pubmap {

constexpr int MAX_SEGS = 32;
struct CopySeg { int64_t src, dst; int32_t n, per_layer; };
// f32 copies dst[seg.dst + l * dst_stride + i] = params[seg.src + l * src_stride + i], i < n, l < (per_layer ? layers : 1)
struct CopyTable {
  int32_t nseg, layers;
  int64_t src_stride, dst_stride, dst_total;
  CopySeg seg[MAX_SEGS];
};

inline void add_seg(CopyTable& t, int64_t& o, int64_t src, int64_t n, int per_layer, int64_t pad) {
  t.seg[t.nseg++] = CopySeg{src, o, (int32_t)n, per_layer};
  o += (n + pad - 1) / pad * pad;
}

// context encoder -> hn_f32: every tensor padded to 4 floats, in the order hvla_load_weights pushes them (not the training
// order: the final norm comes before the blocks, LayerNorm_1 after the attention)
inline CopyTable ctx_table(const Geom& g, const TrainLayout& L) {
  CopyTable t{};
  int64_t o = 0;
  const int64_t C = g.C, F = g.ctx_mlp;
  auto add = [&](int64_t src, int64_t n, int pl) { add_seg(t, o, src, n, pl, 4); };
  add(L.w_tok, g.lang_dim * C, 0); add(L.b_tok, C, 0); add(L.w_img, g.E * C, 0); add(L.b_img, C, 0);
  add(L.pos_tok, g.T * C, 0); add(L.pos_img, C, 0); add(L.pos_layer, C, 0); add(L.norm_s, C, 0); add(L.norm_b, C, 0);
  const int64_t layer0 = o;
  t.layers = g.ctx_layers;
  if (g.ctx_layers > 0) {
    const TrainLayout::CL& c = L.layer[0];
    add(c.ln0_s, C, 1); add(c.ln0_b, C, 1);
    add(c.wq, C * C, 1); add(c.bq, C, 1); add(c.wk, C * C, 1); add(c.bk, C, 1); add(c.wv, C * C, 1); add(c.bv, C, 1);
    add(c.wo, C * C, 1); add(c.bo, C, 1);
    add(c.ln1_s, C, 1); add(c.ln1_b, C, 1);
    add(c.w1, C * F, 1); add(c.b1, F, 1); add(c.w2, F * C, 1); add(c.b2, C, 1);
    t.src_stride = g.ctx_layers > 1 ? L.layer[1].ln0_s - L.layer[0].ln0_s : 0;
  }
  t.dst_stride = o - layer0;
  t.dst_total = layer0 + t.dst_stride * g.ctx_layers;
  return t;
}

// image encoder.  16-bit planes enc16 / encd16 (`off16` order): patch embedding [E][Kp], then per layer qkv [3E][E], out [E][E],
// fc1 [Fe][E], fc2 [E][Fe].  f32 vectors encf32 (`offf` order): patch bias [E], position table [S][E], final norm scale, bias,
// then per layer q / k / v bias, out bias, fc1 bias, fc2 bias, norm1 scale / bias, norm2 scale / bias, layer scales 1 / 2.
struct EncMat { int64_t src, dst; int32_t K, N, tile0; };   // [K][N] f32 at params + src -> [N][K] 16-bit at dst; tile0: its first 64 x 64 tile
constexpr int ENC_MATS = 6;
constexpr int TR_TILE = 64;
struct EncMap {
  CopyTable vec;
  EncMat mat[ENC_MATS];            // layer 0, in destination order: query, key, value, out, fc1, fc2
  int32_t tiles_per_layer, layers;
  int64_t mat_src_stride, mat_dst_stride, n16;
  int64_t src_cls, src_pb, src_pk, src_pos;     // training-vector offsets of the embedding leaves
  int64_t f_bpatch, f_pos;                      // encf32 offsets of the patch bias and the position table
  int32_t E, S, Kp, Kreal;
};

inline EncMap enc_map(const Geom& g, const TrainLayout& L) {
  EncMap m{};
  const int64_t E = g.E, Fe = g.enc_mlp, S = g.S(), b = L.total;
  m.E = g.E; m.S = g.S(); m.Kreal = g.patch * g.patch * 3; m.Kp = 2 * ((m.Kreal + 63) / 64 * 64);
  m.layers = g.enc_layers;
  m.src_cls = b + L.e_cls; m.src_pb = b + L.e_pb; m.src_pk = b + L.e_pk; m.src_pos = b + L.e_pos;
  int64_t of = 0;
  auto addf = [&](int64_t src, int64_t n, int pl) { add_seg(m.vec, of, src, n, pl, 1); };
  m.f_bpatch = of; of += E;
  m.f_pos = of; of += S * E;
  addf(b + L.e_lns, E, 0); addf(b + L.e_lnb, E, 0);
  const int64_t f_layer0 = of, o16_layer0 = E * m.Kp;
  m.vec.layers = g.enc_layers;
  if (g.enc_layers > 0) {
    const TrainLayout::EL& y = L.enc[0];
    addf(b + y.qb, E, 1); addf(b + y.kb, E, 1); addf(b + y.vb, E, 1); addf(b + y.ob, E, 1); addf(b + y.f1b, Fe, 1); addf(b + y.f2b, E, 1);
    addf(b + y.n1s, E, 1); addf(b + y.n1b, E, 1); addf(b + y.n2s, E, 1); addf(b + y.n2b, E, 1); addf(b + y.ls1, E, 1); addf(b + y.ls2, E, 1);
    m.vec.src_stride = m.mat_src_stride = g.enc_layers > 1 ? L.enc[1].kb - L.enc[0].kb : 0;
    int64_t o16 = o16_layer0;
    int32_t tile = 0;
    auto addm = [&](int i, int64_t src, int K, int N) {
      m.mat[i] = EncMat{b + src, o16, K, N, tile};
      o16 += (int64_t)K * N;
      tile += (K / TR_TILE) * (N / TR_TILE);
    };
    addm(0, y.qk, g.E, g.E); addm(1, y.kk, g.E, g.E); addm(2, y.vk, g.E, g.E); addm(3, y.ok, g.E, g.E);
    addm(4, y.f1k, g.E, g.enc_mlp); addm(5, y.f2k, g.enc_mlp, g.E);
    m.tiles_per_layer = tile;
    m.mat_dst_stride = o16 - o16_layer0;
  }
  m.vec.dst_stride = of - f_layer0;
  m.vec.dst_total = f_layer0 + m.vec.dst_stride * g.enc_layers;
  m.n16 = o16_layer0 + m.mat_dst_stride * g.enc_layers;
  return m;
}

// ---- element formulas (device and host) ----------------------------------------------------------------------------------

// one element of a transposing pack: the 16-bit weight and what the rounding dropped, x 4096 (pack::pack_matrix_t)
HVLA_HD inline void round_pair(float w, bool bf, uint16_t& w16, uint16_t& d16) {
  w16 = pack::to16(w, bf);
  d16 = pack::to16((w - pack::from16(w16, bf)) * 4096.f, bf);
}
// one element of W_cat: hi = bf16(w), lo = bf16(w - hi) (pack::pack_wcat)
HVLA_HD inline void split_pair(float w, uint16_t& hi, uint16_t& lo) {
  hi = pack::f2bf(w);
  lo = pack::f2bf(w - pack::bf2f(hi));
}
// column tau of a 32-column tile sits in fragment lane rho (+ 32 for the upper eight k of a k-step): the inverse of
// tau = 16 ((rho >> 2) & 1) + (rho & 3) + 4 (rho >> 3) in pack::pack_wcat
HVLA_HD inline int rho_of_tau(int tau) { return (tau & 3) + 4 * (tau >> 4) + 8 * ((tau >> 2) & 3); }

// output channel nn of the patch embedding: row nn of [E][hi Kp/2 | lo Kp/2] and its bias, the arithmetic of hvla_load_weights
// (the rescale 256 / (255 std) in double, rounded to f32 once; the bias accumulated in double, ascending k).  `pk` [Kreal][E]
HVLA_HD inline float patch_channel(const float* pk, float pb, int E, int nn, int Kreal, int Kp, bool bf, uint16_t* row) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  // (selected, not indexed: a table indexed by k % 3 would sit in the kernel's private segment)
  const int Kp1 = Kp / 2;
  double bacc = pb;
  for (int k = 0; k < Kp1; ++k) {
    uint16_t hi = 0, lo = 0;
    if (k < Kreal) {
      const int c = k % 3;
      const double mean = c == 0 ? 0.485 : c == 1 ? 0.456 : 0.406, sd = c == 0 ? 0.229 : c == 1 ? 0.224 : 0.225;
      const double wk = pk[(size_t)k * E + nn];
      const float w = (float)(wk * 256.0 / (255.0 * sd));
      hi = pack::to16(w, bf);
      lo = pack::to16(w - pack::from16(hi, bf), bf);
      bacc += wk * (128.0 / 255.0 - mean) / sd;
    }
    row[k] = hi;
    row[Kp1 + k] = lo;
  }
  return (float)bacc;
}

}  // namespace pubmap
}  // namespace hvla
