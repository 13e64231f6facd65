// serving_layout.h — the one description of the device buffers that hold the served weights: hn_f32 (context encoder), enc16 /
// encd16 (image-encoder matrices and their rounding residues) and encf32 (image-encoder vectors).  served_ctx / served_enc name
// every served tensor once, in the order it lies in its buffer.  hvla_load_weights (api.hip) packs checkpoint tensors through
// them (pack_serving, below), hvla_train_publish (publish.hip) derives from them the tables its kernels take by value, and
// tests/native/publish_map_check.cpp runs both on the CPU.  W_cat / b_cat are laid out by layout.h's perm.  No HIP types.
#pragma once
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "layout.h"
#include "pack.h"
#include "train_layout.h"

namespace hvla {
namespace serving {

enum Pack {
  PAD4,         // hn_f32: f32 copy, padded to 4 floats
  COPY,         // encf32: f32 copy
  TRANSPOSE,    // enc16 / encd16: [K][N] f32 -> [N][K] 16-bit weight and residue (pack::round_pair)
  PATCH,        // enc16: the patch embedding [Kreal][E] -> [E][Kp] (pack::patch_channel) ...
  PATCH_BIAS,   // ... and encf32: the bias that comes out of the same arithmetic
  POS,          // encf32: the position table, the CLS token added into row 0
  CLS,          // no buffer: read by POS
  UNSERVED      // no buffer: a checkpoint must hold it, nothing reads it
};
// `src`: the tensor's offset in the flat training vector (the shared DINOv2 leaves follow the hypernetwork's own parameters).
// The checkpoint name is prefix + leaf, or prefix + layer + sep + leaf for a per-layer tensor (layer >= 0).
struct Tensor { const char *prefix, *sep, *leaf; int layer; int64_t n, src; Pack pack; int K; };
inline std::string checkpoint_name(const Tensor& t) {
  return t.layer < 0 ? std::string(t.prefix) + t.leaf : t.prefix + std::to_string(t.layer) + t.sep + t.leaf;
}

inline int patch_kreal(const Geom& g) { return g.patch * g.patch * 3; }
inline int patch_kp(const Geom& g) { return 2 * ((patch_kreal(g) + 63) / 64 * 64); }     // [W_hi | W_lo] along K (encoder.hip)

// elements of hn_f32 / enc16 (= encd16) / encf32
struct Extent { int64_t hn, n16, nf; };

// Where every tensor lies: `at` has TrainLayout's members, holding offsets in the destination buffer where `L` holds offsets in
// the training vector.  A member names the tensor wherever one is needed: api.hip sets the kernels' pointers from `at` by member.
using Offsets = TrainLayout;

// One running offset per buffer; f(tensor, destination offset) for every tensor in turn.  `in` says which names and which part of
// the training vector the next tensors have.
template <class F>
struct Walk {
  const Geom& g;
  F& f;
  Extent e{0, 0, 0};
  const char *prefix = "", *sep = "";
  int layer = -1;
  int64_t base = 0;
  void in(const char* p, const char* s, int l, int64_t b) { prefix = p; sep = s; layer = l; base = b; }
  void operator()(const char* leaf, int64_t n, int64_t src, long& at, Pack pack, int64_t K = 0) {
    int64_t none = -1;
    int64_t& o = pack == PAD4 ? e.hn : pack == TRANSPOSE || pack == PATCH ? e.n16 : pack == CLS || pack == UNSERVED ? none : e.nf;
    at = (long)o;
    f(Tensor{prefix, sep, leaf, layer, n, base + src, pack, (int)K}, o);
    o += pack == PAD4 ? (n + 3) / 4 * 4 : pack == PATCH ? (int64_t)g.E * patch_kp(g) : n;
  }
};

// context encoder -> hn_f32 (not the training order: the final norm comes before the blocks, LayerNorm_1 after the attention)
template <class F>
inline Extent served_ctx(const Geom& g, const TrainLayout& L, Offsets& at, F&& f) {
  Walk<F> put{g, f};
  const int64_t C = g.C, Fc = g.ctx_mlp;
#define HVLA_ATT "MultiHeadDotProductAttention_0/"
  put("task_token_projection/kernel", g.lang_dim * C, L.w_tok, at.w_tok, PAD4); put("task_token_projection/bias", C, L.b_tok, at.b_tok, PAD4);
  put("initial_image_projection/kernel", g.E * C, L.w_img, at.w_img, PAD4); put("initial_image_projection/bias", C, L.b_img, at.b_img, PAD4);
  put("task_pos_embedding", g.T * C, L.pos_tok, at.pos_tok, PAD4); put("initial_image_pos_embedding", C, L.pos_img, at.pos_img, PAD4);
  put("layer_pos_embedding", g.NL() * C, L.pos_layer, at.pos_layer, PAD4);     // (1, NL, C): the training vector holds the NL rows too
  put("Transformer_0/encoder_norm/scale", C, L.norm_s, at.norm_s, PAD4); put("Transformer_0/encoder_norm/bias", C, L.norm_b, at.norm_b, PAD4);
  for (int l = 0; l < g.ctx_layers; ++l) {
    const BlockLeaves& s = L.layer[l];
    BlockLeaves& d = at.layer[l];
    put.in("Transformer_0/encoderblock_", "/", l, 0);
    put("LayerNorm_0/scale", C, s.ln0_s, d.ln0_s, PAD4); put("LayerNorm_0/bias", C, s.ln0_b, d.ln0_b, PAD4);
    put(HVLA_ATT "query/kernel", C * C, s.wq, d.wq, PAD4); put(HVLA_ATT "query/bias", C, s.bq, d.bq, PAD4);
    put(HVLA_ATT "key/kernel", C * C, s.wk, d.wk, PAD4); put(HVLA_ATT "key/bias", C, s.bk, d.bk, PAD4);
    put(HVLA_ATT "value/kernel", C * C, s.wv, d.wv, PAD4); put(HVLA_ATT "value/bias", C, s.bv, d.bv, PAD4);
    put(HVLA_ATT "out/kernel", C * C, s.wo, d.wo, PAD4); put(HVLA_ATT "out/bias", C, s.bo, d.bo, PAD4);
    put("LayerNorm_1/scale", C, s.ln1_s, d.ln1_s, PAD4); put("LayerNorm_1/bias", C, s.ln1_b, d.ln1_b, PAD4);
    put("MlpBlock_0/Dense_0/kernel", C * Fc, s.w1, d.w1, PAD4); put("MlpBlock_0/Dense_0/bias", Fc, s.b1, d.b1, PAD4);
    put("MlpBlock_0/Dense_1/kernel", Fc * C, s.w2, d.w2, PAD4); put("MlpBlock_0/Dense_1/bias", C, s.b2, d.b2, PAD4);
  }
#undef HVLA_ATT
  return put.e;
}

// image encoder.  enc16 / encd16: patch embedding [E][Kp], then per layer query, key, value (one [3E][E] to the kernels), out
// [E][E], fc1 [Fe][E], fc2 [E][Fe].  encf32: patch bias [E], position table [S][E], final norm scale, bias, then per layer q / k /
// v bias (one [3E]), out bias, fc1 bias, fc2 bias, norm1 scale / bias, norm2 scale / bias, layer scales 1 / 2.  The CLS token
// precedes the position table that reads it, the patch kernel its bias.
template <class F>
inline Extent served_enc(const Geom& g, const TrainLayout& L, Offsets& at, F&& f) {
  Walk<F> put{g, f};
  const int64_t E = g.E, Fe = g.enc_mlp, Kreal = patch_kreal(g);
  put.in("encoder_image_encoder_", "", -1, L.total);
  put("embeddings_cls_token", E, L.e_cls, at.e_cls, CLS); put("embeddings_mask_token", E, L.e_mask, at.e_mask, UNSERVED);
  put("embeddings_patch_embeddings_projection_kernel", Kreal * E, L.e_pk, at.e_pk, PATCH, Kreal);
  put("embeddings_patch_embeddings_projection_bias", E, L.e_pb, at.e_pb, PATCH_BIAS);
  put("embeddings_position_embeddings", g.S() * E, L.e_pos, at.e_pos, POS);
  put("layernorm_scale", E, L.e_lns, at.e_lns, COPY); put("layernorm_bias", E, L.e_lnb, at.e_lnb, COPY);
  for (int l = 0; l < g.enc_layers; ++l) {
    const BlockLeaves& s = L.enc[l];
    BlockLeaves& d = at.enc[l];
    put.in("encoder_image_encoder_encoder_layer_", "_", l, L.total);
    put("attention_attention_query_kernel", E * E, s.wq, d.wq, TRANSPOSE, E); put("attention_attention_query_bias", E, s.bq, d.bq, COPY);
    put("attention_attention_key_kernel", E * E, s.wk, d.wk, TRANSPOSE, E); put("attention_attention_key_bias", E, s.bk, d.bk, COPY);
    put("attention_attention_value_kernel", E * E, s.wv, d.wv, TRANSPOSE, E); put("attention_attention_value_bias", E, s.bv, d.bv, COPY);
    put("attention_output_dense_kernel", E * E, s.wo, d.wo, TRANSPOSE, E); put("attention_output_dense_bias", E, s.bo, d.bo, COPY);
    put("mlp_fc1_kernel", E * Fe, s.w1, d.w1, TRANSPOSE, E); put("mlp_fc1_bias", Fe, s.b1, d.b1, COPY);
    put("mlp_fc2_kernel", Fe * E, s.w2, d.w2, TRANSPOSE, Fe); put("mlp_fc2_bias", E, s.b2, d.b2, COPY);
    put("norm1_scale", E, s.ln0_s, d.ln0_s, COPY); put("norm1_bias", E, s.ln0_b, d.ln0_b, COPY);
    put("norm2_scale", E, s.ln1_s, d.ln1_s, COPY); put("norm2_bias", E, s.ln1_b, d.ln1_b, COPY);
    put("layer_scale1_lambda1", E, s.ls1, d.ls1, COPY); put("layer_scale2_lambda1", E, s.ls2, d.ls2, COPY);
  }
  return put.e;
}

// ---- the tables the publish kernels take by value: the publish allocates and uploads nothing --------------------------------
// The training vector and the buffers are both regular per layer, so a table holds the segments of layer 0 plus one source and
// one destination stride; a segment with per_layer == 0 exists once.

constexpr int MAX_SEGS = 32;
struct CopySeg { int64_t src, dst; int32_t n, per_layer; };
// f32 copies dst[seg.dst + l * dst_stride + i] = params[seg.src + l * src_stride + i], i < n, l < (per_layer ? layers : 1)
struct CopyTable {
  int32_t nseg, layers;
  int64_t src_stride, dst_stride, dst_total;
  CopySeg seg[MAX_SEGS];
};
inline void add_seg(CopyTable& t, const Tensor& s, int64_t dst) {
  if (s.layer <= 0) t.seg[t.nseg++] = CopySeg{s.src, dst, (int32_t)s.n, s.layer == 0};
}

inline CopyTable ctx_table(const Geom& g, const TrainLayout& L) {
  CopyTable t{};
  Offsets at{};
  t.dst_total = served_ctx(g, L, at, [&](const Tensor& s, int64_t dst) { add_seg(t, s, dst); }).hn;
  t.layers = g.ctx_layers;
  t.src_stride = g.ctx_layers > 1 ? L.layer[1].ln0_s - L.layer[0].ln0_s : 0;
  t.dst_stride = g.ctx_layers > 0 ? (t.dst_total - at.layer[0].ln0_s) / g.ctx_layers : 0;
  return t;
}

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
  Offsets at{};
  int nmat = 0;
  const Extent e = served_enc(g, L, at, [&](const Tensor& s, int64_t dst) {
    if (s.pack == COPY) add_seg(m.vec, s, dst);
    if (s.pack == CLS) m.src_cls = s.src;
    if (s.pack == PATCH) m.src_pk = s.src;
    if (s.pack == PATCH_BIAS) { m.src_pb = s.src; m.f_bpatch = dst; }
    if (s.pack == POS) { m.src_pos = s.src; m.f_pos = dst; }
    if (s.pack == TRANSPOSE && s.layer == 0) {
      const int32_t N = (int32_t)(s.n / s.K);
      m.mat[nmat++] = EncMat{s.src, dst, s.K, N, m.tiles_per_layer};
      m.tiles_per_layer += (s.K / TR_TILE) * (N / TR_TILE);
    }
  });
  m.E = g.E; m.S = g.S(); m.Kreal = patch_kreal(g); m.Kp = patch_kp(g);
  m.layers = m.vec.layers = g.enc_layers;
  m.n16 = e.n16;
  m.vec.dst_total = e.nf;
  if (g.enc_layers > 0) {
    m.vec.src_stride = m.mat_src_stride = g.enc_layers > 1 ? L.enc[1].bk - L.enc[0].bk : 0;
    m.vec.dst_stride = (e.nf - at.enc[0].bq) / g.enc_layers;
    m.mat_dst_stride = (e.n16 - at.enc[0].wq) / g.enc_layers;
  }
  return m;
}

// ---- the host packer: checkpoint tensors -> the host images of the buffers --------------------------------------------------

struct HostImages {
  std::vector<float> hn, encf;
  std::vector<uint16_t> enc16, encd16;
  std::vector<LeafInfo> leaves;             // pack::pack_wcat's inputs: the generated leaves, their kernels and biases
  std::vector<const float*> lk, lb;
  Offsets at;                               // where every tensor lies in its buffer
  std::string missing;                      // "<name> (absent)" / "<name> (wrong size)" of the first tensor that failed
};

// lookup(name) -> (data, numel), data == nullptr for a tensor the checkpoint does not hold.  Every tensor is looked up; if one is
// absent or of another size, `missing` names the first and nothing else of `out` is written.
template <class Lookup>
inline bool pack_serving(const Geom& g, bool bf, Lookup&& lookup, HostImages& out) {
  std::string missing;
  auto get = [&](const std::string& name, int64_t numel) -> const float* {
    const std::pair<const float*, int64_t> t = lookup(name);
    if (t.first && t.second == numel) return t.first;
    if (missing.empty()) missing = name + (t.first ? " (wrong size)" : " (absent)");
    return nullptr;
  };
  struct Job { Tensor t; int64_t dst; const float* p; };
  std::vector<Job> jobs;
  auto collect = [&](const Tensor& t, int64_t dst) { jobs.push_back(Job{t, dst, get(checkpoint_name(t), t.n)}); };
  const TrainLayout L = make_train_layout(g);
  Offsets at{};
  const int64_t nhn = served_ctx(g, L, at, collect).hn;
  std::vector<LeafInfo> leaves = generated_leaves(g);
  std::vector<const float*> lk(leaves.size()), lb(leaves.size());
  for (size_t i = 0; i < leaves.size(); ++i) {
    const std::string head = output_head_of(g, leaves[i].flat);     // shared_block_heads: the blocks' leaves of one name read one tensor
    lk[i] = get(head + "/kernel", (int64_t)g.C * leaves[i].size);
    lb[i] = get(head + "/bias", leaves[i].size);
  }
  const Extent e = served_enc(g, L, at, collect);
  out.missing = missing;
  if (!missing.empty()) return false;
  out.at = at;
  out.leaves.swap(leaves); out.lk.swap(lk); out.lb.swap(lb);
  out.hn.assign(nhn, 0.f); out.encf.assign(e.nf, 0.f);
  out.enc16.assign(e.n16, 0); out.encd16.assign(e.n16, 0);
  const int E = g.E, Kp = patch_kp(g);
  const float *cls = nullptr, *pk = nullptr;
  uint16_t* patch16 = nullptr;
  for (const Job& j : jobs) {
    const Tensor& t = j.t;
    float* f = t.pack == PAD4 ? out.hn.data() : out.encf.data();       // the f32 buffer of the kinds that have one
    switch (t.pack) {
      case PAD4: case COPY: memcpy(f + j.dst, j.p, t.n * 4); break;
      case TRANSPOSE: pack::pack_matrix_t(j.p, t.K, (int)(t.n / t.K), bf, &out.enc16[j.dst], &out.encd16[j.dst]); break;
      case CLS: cls = j.p; break;
      case PATCH: pk = j.p; patch16 = &out.enc16[j.dst]; break;
      case PATCH_BIAS:
        for (int n = 0; n < E; ++n) f[j.dst + n] = pack::patch_channel(pk, j.p[n], E, n, patch_kreal(g), Kp, bf, patch16 + (size_t)n * Kp);
        break;
      case POS: for (int64_t i = 0; i < t.n; ++i) f[j.dst + i] = j.p[i] + (i < E ? cls[i] : 0.f); break;
      case UNSERVED: break;
    }
  }
  return true;
}

}  // namespace serving
}  // namespace hvla
