// layout.h — how one episode's generated parameters are laid out in the device weight arena, and
// the map back to the reference's pytree order (hypervla/model.py:370-515).
//
// The hypernetwork's 73 output heads are one GEMM  theta[B, G] = ctx[B, C] @ W_cat[C, G] + b_cat
// (share_layer_index=True => every head reads context token 0, hypernetwork.py:205-217; with share_layer_index=False the A row of
// a position is the context row of its leaf's layer token, pack.h's segment list).  Because
// the columns of W_cat can be permuted freely at load time, the GEMM writes each parameter straight
// to the place the policy kernel reads it from:
//
//   matrix region  Wh/Wl[B][Gm]  bf16 hi / lo planes (x = hi + lo), in MFMA A-fragment order:
//                  fragment f = 64 lanes x 8 elements; lane (row = l & 31, half = l >> 5) holds
//                  W[k(step, half, j)][n = 32 * mtile + row], j = 0..7 (the K order of each GEMM is the
//                  order in which the kernel produces the matching B fragments, see policy.hip)
//   vector region  Vf[B][Gv]     f32 biases / LayerNorm / position embedding, in accumulator
//                  ("C-layout") order: [tile][half][r] <-> feature 32 * tile + crow(r, half)
//
// perm[pos] is the reference flat index (leaf offset + C-order index in the flax leaf) of packed
// position pos in [0, Gm + Gv), or -1 for padding.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace hvla {

// layer counts the fixed-size tables are built for: hvla_create refuses more context / image-encoder layers (accept.h), the
// training path more policy layers as well (train_layout.h)
constexpr int CTX_MAX_LAYERS = 8;               // CtxParams::layer, TrainLayout::layer
constexpr int ENC_MAX_LAYERS = 24;              // EncWeights::layer, TrainLayout::enc
constexpr int TRAIN_MAX_POLICY_LAYERS = 16;     // TrainLayout::pol

struct Geom {
  int image_size, patch, E, enc_layers, enc_heads, enc_mlp;
  int D, L, H, M, horizon, action_dim;
  float tanh_scale, max_action;
  int C, ctx_layers, ctx_heads, ctx_mlp, T, lang_dim, scale_context;
  int clip_target = 1;       // MixActionHead.loss: clip the action target to +-max_action (action_heads.py:499-500)
  int lang_in_policy = 0;    // vit_kwargs.use_language_token (base_vit.py:159-166,207-212): [T language | P patches | 1 action]
  int mask_as_bias = 0;      // vit_kwargs.return_attention_map (transformer.py:172-181, multi_head_attetion.py:88-98): the blocks' attention is
                             // CustomMultiHeadDotProductAttention_0, which adds the 0 / 1 mask to the scores instead of masking
  int differential = 0;      // vit_kwargs.use_differential_transformer (transformer.py:166-171, differential_transformer.py:99-252): the blocks'
                             // attention is DifferentialAttention_0 -- two softmaxes over the halves of each head's q / k, A1 - lambda A2,
                             // an RMSNorm per head; no q / k / v / out bias.  Not with either flag above
  int layer_tokens = 0;      // hypernet_kwargs.share_layer_index=False (model.py:400-436): NL() layer tokens in the context encoder, every generated
                             // leaf reads the token of its module (layer_token_of, below).  Fine-tuned behind
                             // hvla_train_layer_tokens (train_layout.h's run table)
  int shared_block_heads = 0;   // hypernet_kwargs.share_TF_output_head (hypernetwork.py:221-225): one output head per leaf name for all policy
                             // blocks; only with layer_tokens
  // rows of layer_pos_embedding and of the context embedding: the shared image encoder, encoder_norm, L blocks, the image projection,
  // (the language projection,) the position table and the action head -- or the one token every head reads
  int NL() const { return layer_tokens ? L + 5 + (lang_in_policy ? 1 : 0) : 1; }
  int ctx_row() const { return NL() * C; }     // floats of one episode's context wherever it is carried
  const char* attention_name() const {
    return differential ? "DifferentialAttention_0_" : (mask_as_bias ? "CustomMultiHeadDotProductAttention_0_" : "MultiHeadDotProductAttention_0_");
  }
  int grid() const { return image_size / patch; }
  int P() const { return grid() * grid(); }
  int S() const { return P() + 1; }
  int hd() const { return D / H; }
  int A() const { return horizon * (action_dim - 1); }
  int pos_rows() const { return S() + (lang_in_policy ? T : 0); }   // rows of the policy's pos_embedding
};

// one generated leaf in reference (jax pytree) order
struct LeafInfo {
  std::string flat;          // "encoder_Transformer_0_encoderblock_0_LayerNorm_0_bias"
  std::vector<int> shape;
  int64_t offset, size;
};

inline std::vector<LeafInfo> generated_leaves(const Geom& g) {
  std::vector<LeafInfo> v;
  int64_t off = 0;
  auto add = [&](const std::string& name, std::vector<int> shape) {
    int64_t n = 1;
    for (int s : shape) n *= s;
    v.push_back({name, shape, off, n});
    off += n;
  };
  const int D = g.D, M = g.M, H = g.H, hd = g.hd();
  add("action_head_continuous_head_bias", {g.A()});
  add("action_head_continuous_head_kernel", {D, g.A()});
  add("action_head_discrete_head_bias", {g.horizon});
  add("action_head_discrete_head_kernel", {D, g.horizon});
  const std::string T = "encoder_Transformer_0_";
  add(T + "encoder_norm_bias", {D});
  add(T + "encoder_norm_scale", {D});
  for (int l = 0; l < g.L; ++l) {
    const std::string B = T + "encoderblock_" + std::to_string(l) + "_";
    auto rest = [&] {
      add(B + "LayerNorm_0_bias", {D});
      add(B + "LayerNorm_0_scale", {D});
      add(B + "LayerNorm_1_bias", {D});
      add(B + "LayerNorm_1_scale", {D});
      add(B + "MlpBlock_0_Dense_0_bias", {M});
      add(B + "MlpBlock_0_Dense_0_kernel", {D, M});
      add(B + "MlpBlock_0_Dense_1_bias", {D});
      add(B + "MlpBlock_0_Dense_1_kernel", {M, D});
    };
    if (g.differential) {                 // sorted keys: "DifferentialAttention_0" leads the block; hd / 2 = D / (2 H) per softmax
      const std::string A = B + g.attention_name();
      add(A + "k_proj_kernel", {D, D});
      add(A + "lambda_k1", {hd / 2});
      add(A + "lambda_k2", {hd / 2});
      add(A + "lambda_q1", {hd / 2});
      add(A + "lambda_q2", {hd / 2});
      add(A + "out_proj_kernel", {D, D});
      add(A + "q_proj_kernel", {D, D});
      add(A + "subln_weight", {hd});
      add(A + "v_proj_kernel", {D, D});
      rest();
      continue;
    }
    if (!g.mask_as_bias) rest();          // sorted keys: "CustomMultiHead..." leads the block, "MultiHead..." ends it
    const std::string A = B + g.attention_name();
    add(A + "key_bias", {H, hd});
    add(A + "key_kernel", {D, H, hd});
    add(A + "out_bias", {D});
    add(A + "out_kernel", {H, hd, D});
    add(A + "query_bias", {H, hd});
    add(A + "query_kernel", {D, H, hd});
    add(A + "value_bias", {H, hd});
    add(A + "value_kernel", {D, H, hd});
    if (g.mask_as_bias) rest();
  }
  add("encoder_image_embedding_projection_bias", {D});
  add("encoder_image_embedding_projection_kernel", {g.E, D});
  if (g.lang_in_policy) {
    add("encoder_language_token_projection_bias", {D});
    add("encoder_language_token_projection_kernel", {g.lang_dim, D});
  }
  add("encoder_pos_embedding", {1, g.pos_rows(), D});
  return v;
}

// share_layer_index=False: the layer token a generated leaf reads (model.py:418-436, restated in hypervla.config.layer_token_modules,
// which tests/test_layer_tokens_host.py holds this function to).  Token 0 is the shared image encoder (never returned); then the
// modules of encoder/Transformer_0 in the key-sorted order jax.tree_map rebuilds a dict in -- "encoder_norm", then "encoderblock_<l>"
// as STRINGS, so encoderblock_10 precedes encoderblock_2 --, then image_embedding_projection, (language_token_projection,)
// pos_embedding, and action_head last.  -1: no leaf of this geometry.
inline int layer_token_of(const Geom& g, const std::string& flat) {
  auto starts = [&](const std::string& p) { return flat.compare(0, p.size(), p) == 0; };
  const std::string T = "encoder_Transformer_0_";
  if (starts("action_head_")) return g.NL() - 1;
  if (starts(T + "encoder_norm_")) return 1;
  if (starts(T + "encoderblock_")) {
    const size_t a = T.size() + 13, e = flat.find('_', a);
    if (e == std::string::npos) return -1;
    const std::string own = flat.substr(a, e - a);
    int rank = 0, found = 0;
    for (int l = 0; l < g.L; ++l) {
      const std::string other = std::to_string(l);
      if (other == own) found = 1;
      else if (other < own) ++rank;
    }
    return found ? 2 + rank : -1;
  }
  if (starts("encoder_image_embedding_projection_")) return 2 + g.L;
  if (g.lang_in_policy && starts("encoder_language_token_projection_")) return 3 + g.L;
  if (starts("encoder_pos_embedding")) return 3 + g.L + (g.lang_in_policy ? 1 : 0);
  return -1;
}
// share_TF_output_head: the output head of a leaf, "encoderblock_<l>" -> "encoderblock" (hypernetwork.py:221-225)
inline std::string output_head_of(const Geom& g, const std::string& flat) {
  const std::string B = "encoder_Transformer_0_encoderblock_";
  if (!g.shared_block_heads || flat.compare(0, B.size(), B) != 0) return "output_head_" + flat;
  const size_t e = flat.find('_', B.size());
  return "output_head_" + B.substr(0, B.size() - 1) + (e == std::string::npos ? "" : flat.substr(e));
}

// Offsets the policy kernel uses (all in elements; frag offsets are multiples of 512).
struct PolicyLayout {
  int Gm, Gv;              // padded sizes of the matrix / vector regions (per episode)
  int G;                   // reference parameter count
  // matrix region (bf16 elements)
  int m_proj;              // [D/32 mtile][E/16 kstep] frags
  int m_layer0, m_layer_stride;   // per layer: qkv, out, fc1, fc2
  int m_qkv, m_out, m_fc1, m_fc2;  // offsets inside a layer
  int m_head;
  // vector region (f32 elements)
  int v_proj_bias, v_pos, v_layer0, v_layer_stride;
  int v_ln0_s, v_ln0_b, v_qkv_b, v_out_b, v_ln1_s, v_ln1_b, v_fc1_b, v_fc2_b;  // inside a layer
  int v_norm_s, v_norm_b, v_head_b;
};

// use_differential_transformer: the floats a layer's vector block grows by, behind v_fc2_b's D floats (offsets inside a layer, natural
// order): lambda_q1 | lambda_k1 | lambda_q2 | lambda_k2 (hd / 2 each), then subln's weight (hd).  Kept out of PolicyLayout, which the
// policy kernels take by value: with the flag off every kernel argument is the one of the model without it.
inline int diff_layer_floats(const Geom& g) { return g.differential ? 4 * (g.hd() / 2) + g.hd() : 0; }
inline int diff_v_lambda(const PolicyLayout& p, int D) { return p.v_fc2_b + D; }
inline int diff_v_subln(const PolicyLayout& p, int D, int hd) { return p.v_fc2_b + D + 4 * (hd / 2); }

inline int crow_h(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// K order of B fragments made from 32-row accumulator tiles (guide §3 "accumulator tile as the next
// MFMA's operand"): element j of lane-half h in k-step ks is feature
//   32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3)
inline int kphi(int ks, int half, int j) {
  return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * half + (j & 3);
}
// K order of the image-projection GEMM: each lane loads 16 consecutive floats of its token row per
// pair of k-steps:  32 * (ks >> 1) + 16 * h + 8 * (ks & 1) + j
inline int kproj(int ks, int half, int j) { return 32 * (ks >> 1) + 16 * half + 8 * (ks & 1) + j; }

// use_language_token: where the language leaves sit.  Kept out of PolicyLayout, which policy_kernel takes by value:
// with the flag off the arena and every kernel argument are those of the model without it.
//   m_lkv     the episode's language K / V prefix, written by lang_prefix_kernel once per episode, read by policy_kernel_lang
//             (policy.hip): right behind the head's fragments, for layer l and head pair ph 2048 elements at m_lkv + (2 l + ph) 2048
//             of the hi plane (head 2 ph) and of the lo plane (head 2 ph + 1), each [K hi 1 KiB | K lo 1 KiB | V^T 2 KiB] -- the
//             8 KiB of one staged weight tile.  Not generated: perm -1 (the weight generation writes zeros there first)
//   m_lproj   language_token_projection kernel [lang_dim, D], [D/32 mtile][lang_dim/16 kstep] frags in the projection's kproj order
//   v_lproj_b its bias, C-layout (D floats)
//   v_lpos    pos_embedding rows [0, T), one C-layout row of D floats each; PolicyLayout::v_pos then holds rows [T, T + P + 1),
//             so the policy kernel's patch / action rows need no change
constexpr int LANG_PAIR_BYTES = 8192;
struct LangLayout {
  int on = 0;
  int m_lkv = 0, m_lproj = 0, v_lproj_b = 0, v_lpos = 0;
};

struct PackedLayout {
  PolicyLayout pl;
  LangLayout ll;
  std::vector<int32_t> perm;   // [Gm + Gv] -> reference flat index or -1
};

// Every offset of PolicyLayout / LangLayout except G (which needs the leaf list): sizes alone, no allocation, so that the
// acceptance predicate (accept.h) can ask how many per-layer floats the policy kernel keeps in LDS without building perm.
inline void policy_offsets(const Geom& g, PolicyLayout& p, LangLayout& ll) {
  const int D = g.D, M = g.M, H = g.H, E = g.E, S = g.S();
  const int TD = D / 32, TM = M / 32;
  p.G = 0;
  // ---- matrix region offsets
  int m = 0;
  p.m_proj = m;  m += TD * (E / 16) * 512;
  p.m_qkv = 0;
  p.m_out = p.m_qkv + (3 * D / 32) * (D / 16) * 512;
  p.m_fc1 = p.m_out + H * TD * 512;
  p.m_fc2 = p.m_fc1 + TM * (D / 16) * 512;
  p.m_layer_stride = p.m_fc2 + TM * TD * 2 * 512;
  p.m_layer0 = m;  m += g.L * p.m_layer_stride;
  p.m_head = m;  m += (D / 16) * 512;
  ll.on = g.lang_in_policy ? 1 : 0;
  if (ll.on) {
    ll.m_lkv = m;  m += g.L * 2 * (LANG_PAIR_BYTES / 4);             // (policy_body.inc derives it as m_head + 4 frags)
    ll.m_lproj = m;  m += TD * (g.lang_dim / 16) * 512;
  }
  p.Gm = m;
  // ---- vector region offsets
  int v = 0;
  p.v_proj_bias = v;  v += D;
  p.v_pos = v;  v += S * D;
  if (ll.on) {
    ll.v_lproj_b = v;  v += D;
    ll.v_lpos = v;  v += g.T * D;
  }
  p.v_ln0_s = 0;  p.v_ln0_b = D;  p.v_qkv_b = 2 * D;  p.v_out_b = 5 * D;
  p.v_ln1_s = 6 * D;  p.v_ln1_b = 7 * D;  p.v_fc1_b = 8 * D;  p.v_fc2_b = 8 * D + M;
  p.v_layer_stride = 9 * D + M + diff_layer_floats(g);
  p.v_layer0 = v;  v += g.L * p.v_layer_stride;
  p.v_norm_s = v;  v += D;
  p.v_norm_b = v;  v += D;
  p.v_head_b = v;  v += 32;
  p.Gv = (v + 31) / 32 * 32;
}

inline PackedLayout build_layout(const Geom& g) {
  PackedLayout out;
  PolicyLayout& p = out.pl;
  LangLayout& ll = out.ll;
  policy_offsets(g, p, ll);
  const int D = g.D, M = g.M, H = g.H, hd = g.hd(), E = g.E, S = g.S();
  const int TD = D / 32, TM = M / 32;
  auto leaves = generated_leaves(g);
  auto find = [&](const std::string& n) -> const LeafInfo& {
    for (auto& l : leaves)
      if (l.flat == n) return l;
    static LeafInfo none;
    return none;
  };
  p.G = (int)(leaves.back().offset + leaves.back().size);

  out.perm.assign((size_t)p.Gm + p.Gv, -1);
  int32_t* pm = out.perm.data();
  int32_t* pv = out.perm.data() + p.Gm;

  // A-fragment writer: W^T rows n (32 per mtile), k given by korder(ks, half, j); ref(k, n) gives the
  // reference flat index or -1.
  auto put_frag = [&](int base, int frag, int mtile, int ks, int (*korder)(int, int, int), int kbase,
                      auto ref) {
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) {
        int n = 32 * mtile + (lane & 31);
        int k = kbase + korder(ks, lane >> 5, j);
        pm[base + frag * 512 + lane * 8 + j] = ref(k, n);
      }
  };
  auto cvec = [&](int base, int ntiles, auto ref) {   // C-layout vector [tile][half][r]
    for (int t = 0; t < ntiles; ++t)
      for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 16; ++r) pv[base + (t * 2 + h) * 16 + r] = ref(32 * t + crow_h(r, h));
  };

  {  // image_embedding_projection: kernel [E, D]
    const LeafInfo& K = find("encoder_image_embedding_projection_kernel");
    const LeafInfo& Bv = find("encoder_image_embedding_projection_bias");
    int f = 0;
    for (int mt = 0; mt < TD; ++mt)
      for (int ks = 0; ks < E / 16; ++ks, ++f)
        put_frag(p.m_proj, f, mt, ks, kproj, 0, [&](int k, int n) { return (int32_t)(K.offset + (int64_t)k * D + n); });
    cvec(p.v_proj_bias, TD, [&](int n) { return (int32_t)(Bv.offset + n); });
    const LeafInfo& Pe = find("encoder_pos_embedding");
    const int t0 = ll.on ? g.T : 0;                       // patch / action rows follow the language rows
    for (int t = 0; t < S; ++t)
      cvec(p.v_pos + t * D, TD, [&](int n) { return (int32_t)(Pe.offset + (int64_t)(t0 + t) * D + n); });
    if (ll.on) {
      for (int t = 0; t < g.T; ++t)
        cvec(ll.v_lpos + t * D, TD, [&](int n) { return (int32_t)(Pe.offset + (int64_t)t * D + n); });
      const LeafInfo& Kl = find("encoder_language_token_projection_kernel");
      const LeafInfo& Bl = find("encoder_language_token_projection_bias");
      const int El = g.lang_dim;
      int fl = 0;
      for (int mt = 0; mt < TD; ++mt)
        for (int ks = 0; ks < El / 16; ++ks, ++fl)
          put_frag(ll.m_lproj, fl, mt, ks, kproj, 0, [&](int k, int n) { return (int32_t)(Kl.offset + (int64_t)k * D + n); });
      cvec(ll.v_lproj_b, TD, [&](int n) { return (int32_t)(Bl.offset + n); });
    }
  }
  for (int l = 0; l < g.L; ++l) {
    const std::string Bn = "encoder_Transformer_0_encoderblock_" + std::to_string(l) + "_";
    const std::string An = Bn + g.attention_name();
    const int mb = p.m_layer0 + l * p.m_layer_stride, vb = p.v_layer0 + l * p.v_layer_stride;
    // fused QKV: rows n in [0,D) = query (head-major h*hd+d == flax [D,H,hd] flattened), [D,2D) key,
    // [2D,3D) value
    // (differential: q_proj / k_proj / v_proj [D, D], the same index arithmetic; no bias leaves, their slots stay padding = zeros)
    const bool df = g.differential != 0;
    const LeafInfo* W[3] = {&find(An + (df ? "q_proj_kernel" : "query_kernel")), &find(An + (df ? "k_proj_kernel" : "key_kernel")),
                            &find(An + (df ? "v_proj_kernel" : "value_kernel"))};
    const LeafInfo* Bq[3] = {&find(An + "query_bias"), &find(An + "key_bias"), &find(An + "value_bias")};
    int f = 0;
    for (int mt = 0; mt < 3 * D / 32; ++mt)
      for (int ks = 0; ks < D / 16; ++ks, ++f)
        put_frag(mb + p.m_qkv, f, mt, ks, kphi, 0, [&](int k, int n) {
          return (int32_t)(W[n / D]->offset + (int64_t)k * D + (n % D));
        });
    if (!df) cvec(vb + p.v_qkv_b, 3 * D / 32, [&](int n) { return (int32_t)(Bq[n / D]->offset + (n % D)); });
    // out projection: flax kernel [H, hd, D]; per head one k-step of hd = 16, K order kphi(ks=0)
    const LeafInfo& Wo = find(An + (df ? "out_proj_kernel" : "out_kernel"));
    f = 0;
    for (int hh = 0; hh < H; ++hh)
      for (int mt = 0; mt < TD; ++mt, ++f)
        put_frag(mb + p.m_out, f, mt, 0, kphi, 0, [&](int k, int n) {
          return (int32_t)(Wo.offset + ((int64_t)hh * hd + k) * D + n);
        });
    if (!df) cvec(vb + p.v_out_b, TD, [&](int n) { return (int32_t)(find(An + "out_bias").offset + n); });
    if (df) {
      const char* lam[4] = {"lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2"};
      for (int i = 0; i < 4; ++i)
        for (int d = 0; d < hd / 2; ++d) pv[vb + diff_v_lambda(p, D) + i * (hd / 2) + d] = (int32_t)(find(An + lam[i]).offset + d);
      for (int d = 0; d < hd; ++d) pv[vb + diff_v_subln(p, D, hd) + d] = (int32_t)(find(An + "subln_weight").offset + d);
    }
    cvec(vb + p.v_ln0_s, TD, [&](int n) { return (int32_t)(find(Bn + "LayerNorm_0_scale").offset + n); });
    cvec(vb + p.v_ln0_b, TD, [&](int n) { return (int32_t)(find(Bn + "LayerNorm_0_bias").offset + n); });
    cvec(vb + p.v_ln1_s, TD, [&](int n) { return (int32_t)(find(Bn + "LayerNorm_1_scale").offset + n); });
    cvec(vb + p.v_ln1_b, TD, [&](int n) { return (int32_t)(find(Bn + "LayerNorm_1_bias").offset + n); });
    // fc1: kernel [D, M]
    const LeafInfo& W1 = find(Bn + "MlpBlock_0_Dense_0_kernel");
    f = 0;
    for (int mt = 0; mt < TM; ++mt)
      for (int ks = 0; ks < D / 16; ++ks, ++f)
        put_frag(mb + p.m_fc1, f, mt, ks, kphi, 0, [&](int k, int n) { return (int32_t)(W1.offset + (int64_t)k * M + n); });
    cvec(vb + p.v_fc1_b, TM, [&](int n) { return (int32_t)(find(Bn + "MlpBlock_0_Dense_0_bias").offset + n); });
    // fc2: kernel [M, D]; consumed per hidden tile t: [t][mt][s]
    const LeafInfo& W2 = find(Bn + "MlpBlock_0_Dense_1_kernel");
    f = 0;
    for (int t = 0; t < TM; ++t)
      for (int mt = 0; mt < TD; ++mt)
        for (int s = 0; s < 2; ++s, ++f)
          put_frag(mb + p.m_fc2, f, mt, s, kphi, 32 * t, [&](int k, int n) { return (int32_t)(W2.offset + (int64_t)k * D + n); });
    cvec(vb + p.v_fc2_b, TD, [&](int n) { return (int32_t)(find(Bn + "MlpBlock_0_Dense_1_bias").offset + n); });
  }
  cvec(p.v_norm_s, TD, [&](int n) { return (int32_t)(find("encoder_Transformer_0_encoder_norm_scale").offset + n); });
  cvec(p.v_norm_b, TD, [&](int n) { return (int32_t)(find("encoder_Transformer_0_encoder_norm_bias").offset + n); });
  {  // mix head: rows [0, A) continuous_head, [A, A + horizon) discrete_head, rest padding
    const LeafInfo& Wc = find("action_head_continuous_head_kernel");
    const LeafInfo& Wd = find("action_head_discrete_head_kernel");
    const LeafInfo& Bc = find("action_head_continuous_head_bias");
    const LeafInfo& Bd = find("action_head_discrete_head_bias");
    const int A = g.A(), Hz = g.horizon;
    for (int ks = 0; ks < D / 16; ++ks)
      put_frag(p.m_head, ks, 0, ks, kphi, 0, [&](int k, int n) -> int32_t {
        if (n < A) return (int32_t)(Wc.offset + (int64_t)k * A + n);
        if (n < A + Hz) return (int32_t)(Wd.offset + (int64_t)k * Hz + (n - A));
        return -1;
      });
    cvec(p.v_head_b, 1, [&](int n) -> int32_t {
      if (n < A) return (int32_t)(Bc.offset + n);
      if (n < A + Hz) return (int32_t)(Bd.offset + (n - A));
      return -1;
    });
  }
  return out;
}

}  // namespace hvla
