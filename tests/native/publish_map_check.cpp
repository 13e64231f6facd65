// CPU-only check of the serving buffers' layout (csrc/serving_layout.h) under AddressSanitizer and UndefinedBehaviorSanitizer.
// Built and run by tests/test_publish_host.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wextra -Werror -I hyper-vla_amd/csrc ...
// At MID and README geometry a flat training vector of distinct values goes three ways:
//   reference: the leaves cut out of the vector (what unpack_params does), through pack::pack_wcat, pack::pack_matrix_t and a
//              transcription of the order in which hvla_load_weights laid out the context encoder and the image encoder before
//              serving_layout.h existed.  It is frozen: the pin that the one layout text moved no byte, and the witness that does
//              not run that text;
//   emulation: what the publish kernels do -- the tables of serving_layout.h and pack.h's element formulas, applied element by
//              element with a counter per destination;
//   packer:    what hvla_load_weights does -- serving::pack_serving itself, fed the same leaves by checkpoint name.
// Every buffer must agree byte for byte, every destination element must be written exactly once, and the offsets the packer
// returns must be where the reference holds each tensor and tile every buffer.  At MID geometry the packer's refusals too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "serving_layout.h"

using namespace hvla;
using namespace hvla::pack;
using namespace hvla::serving;

#define REQUIRE(c, ...) do { if (!(c)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

// distinct, both signs, 2^-25 .. 4: fp16 subnormals, values that round to zero, and (low bits clear) exact ties
static float value(size_t i) {
  const uint32_t m = (uint32_t)(i >> 1);
  const uint32_t u = ((uint32_t)(i & 1) << 31) | (0x33000000u + m * 4u + m % 3u);
  float f;
  memcpy(&f, &u, 4);
  return f;
}

template <typename T>
static int same(const std::vector<T>& a, const std::vector<T>& b, const char* g, const char* what) {
  REQUIRE(a.size() == b.size(), "%s: %s has %zu elements, the reference %zu", g, what, a.size(), b.size());
  if (memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0) return 0;
  for (size_t i = 0; i < a.size(); ++i)
    if (memcmp(&a[i], &b[i], sizeof(T)) != 0) REQUIRE(false, "%s: %s differs at element %zu", g, what, i);
  return 0;
}
static int once(const std::vector<uint8_t>& cnt, size_t from, const char* g, const char* what) {
  for (size_t i = 0; i < cnt.size(); ++i)
    REQUIRE(cnt[i] == (i >= from ? 1 : 0), "%s: %s element %zu written %d times", g, what, i, (int)cnt[i]);
  return 0;
}

// the kernels' table-driven copy
static void apply(const CopyTable& t, const float* params, std::vector<float>& dst, std::vector<uint8_t>& cnt) {
  for (int s = 0; s < t.nseg; ++s)
    for (int l = 0; l < (t.seg[s].per_layer ? t.layers : 1); ++l)
      for (int i = 0; i < t.seg[s].n; ++i) {
        const size_t o = (size_t)(t.seg[s].dst + l * t.dst_stride + i);
        dst.at(o) = params[t.seg[s].src + l * t.src_stride + i];
        ++cnt.at(o);
      }
}

// ---- a checkpoint: every leaf by its name, cut out of the training vector (what unpack_params hands to load_weights).  The names
// are written out here, not taken from serving_layout.h
struct Checkpoint {
  std::map<std::string, std::pair<const float*, int64_t>> t;
  std::vector<std::vector<float>> own;                 // the generated leaves' kernels: [C][size] cut out of W_cat [C][G]
  std::pair<const float*, int64_t> operator()(const std::string& name) const {
    auto it = t.find(name);
    return it == t.end() ? std::pair<const float*, int64_t>{nullptr, 0} : it->second;
  }
};
static Checkpoint cut_checkpoint(const Geom& g, const TrainLayout& L, const float* P) {
  Checkpoint ck;
  const int64_t C = g.C, F = g.ctx_mlp, E = g.E, Fe = g.enc_mlp;
  auto add = [&](const std::string& name, long off, int64_t n) { ck.t[name] = {P + off, n}; };
  add("task_token_projection/kernel", L.w_tok, g.lang_dim * C); add("task_token_projection/bias", L.b_tok, C);
  add("initial_image_projection/kernel", L.w_img, E * C); add("initial_image_projection/bias", L.b_img, C);
  add("task_pos_embedding", L.pos_tok, g.T * C); add("initial_image_pos_embedding", L.pos_img, C); add("layer_pos_embedding", L.pos_layer, C);
  for (int l = 0; l < g.ctx_layers; ++l) {
    const BlockLeaves& c = L.layer[l];
    const std::string b = "Transformer_0/encoderblock_" + std::to_string(l) + "/", a = b + "MultiHeadDotProductAttention_0/";
    add(b + "LayerNorm_0/scale", c.ln0_s, C); add(b + "LayerNorm_0/bias", c.ln0_b, C);
    add(b + "LayerNorm_1/scale", c.ln1_s, C); add(b + "LayerNorm_1/bias", c.ln1_b, C);
    add(a + "query/kernel", c.wq, C * C); add(a + "query/bias", c.bq, C); add(a + "key/kernel", c.wk, C * C); add(a + "key/bias", c.bk, C);
    add(a + "value/kernel", c.wv, C * C); add(a + "value/bias", c.bv, C); add(a + "out/kernel", c.wo, C * C); add(a + "out/bias", c.bo, C);
    add(b + "MlpBlock_0/Dense_0/kernel", c.w1, C * F); add(b + "MlpBlock_0/Dense_0/bias", c.b1, F);
    add(b + "MlpBlock_0/Dense_1/kernel", c.w2, F * C); add(b + "MlpBlock_0/Dense_1/bias", c.b2, C);
  }
  add("Transformer_0/encoder_norm/scale", L.norm_s, C); add("Transformer_0/encoder_norm/bias", L.norm_b, C);
  const auto leaves = generated_leaves(g);
  ck.own.resize(leaves.size());
  for (size_t i = 0; i < leaves.size(); ++i) {
    ck.own[i].resize((size_t)C * leaves[i].size);
    for (int k = 0; k < C; ++k) memcpy(&ck.own[i][(size_t)k * leaves[i].size], P + L.wcat + (long)k * L.G + leaves[i].offset, leaves[i].size * 4);
    ck.t["output_head_" + leaves[i].flat + "/kernel"] = {ck.own[i].data(), C * leaves[i].size};
    add("output_head_" + leaves[i].flat + "/bias", L.bcat + leaves[i].offset, leaves[i].size);
  }
  const std::string ep = "encoder_image_encoder_";
  const long X = L.total;
  add(ep + "embeddings_cls_token", X + L.e_cls, E); add(ep + "embeddings_mask_token", X + L.e_mask, E);
  add(ep + "embeddings_patch_embeddings_projection_bias", X + L.e_pb, E);
  add(ep + "embeddings_patch_embeddings_projection_kernel", X + L.e_pk, (int64_t)g.patch * g.patch * 3 * E);
  add(ep + "embeddings_position_embeddings", X + L.e_pos, g.S() * E);
  for (int l = 0; l < g.enc_layers; ++l) {
    const BlockLeaves& y = L.enc[l];
    const std::string b = ep + "encoder_layer_" + std::to_string(l) + "_", a = b + "attention_attention_";
    add(a + "key_bias", X + y.bk, E); add(a + "key_kernel", X + y.wk, E * E); add(a + "query_bias", X + y.bq, E); add(a + "query_kernel", X + y.wq, E * E);
    add(a + "value_bias", X + y.bv, E); add(a + "value_kernel", X + y.wv, E * E);
    add(b + "attention_output_dense_bias", X + y.bo, E); add(b + "attention_output_dense_kernel", X + y.wo, E * E);
    add(b + "layer_scale1_lambda1", X + y.ls1, E); add(b + "layer_scale2_lambda1", X + y.ls2, E);
    add(b + "mlp_fc1_bias", X + y.b1, Fe); add(b + "mlp_fc1_kernel", X + y.w1, E * Fe); add(b + "mlp_fc2_bias", X + y.b2, E); add(b + "mlp_fc2_kernel", X + y.w2, Fe * E);
    add(b + "norm1_bias", X + y.ln0_b, E); add(b + "norm1_scale", X + y.ln0_s, E); add(b + "norm2_bias", X + y.ln1_b, E); add(b + "norm2_scale", X + y.ln1_s, E);
  }
  add(ep + "layernorm_bias", X + L.e_lnb, E); add(ep + "layernorm_scale", X + L.e_lns, E);
  return ck;
}

// what the enumeration hands its visitor: a tensor and where it goes
struct Placed { Tensor t; int64_t dst; };

// the packer's offsets carry TrainLayout's member names: member m of `at` must be where the enumeration put the tensor that
// lies at member m of the training layout
static int members_agree(const Geom& g, const TrainLayout& L, const Offsets& at, const std::vector<Placed>& all, const char* name) {
  std::map<int64_t, int64_t> where;                    // training-vector offset -> destination offset
  for (const Placed& p : all) REQUIRE(where.emplace(p.t.src, p.dst).second, "%s: two tensors at training offset %lld", name, (long long)p.t.src);
#define AT(src, dst, m) REQUIRE(where.count(src.m + base) && where[src.m + base] == dst.m, "%s: the returned offset of %s", name, #m)
  long base = 0;
  AT(L, at, w_tok); AT(L, at, b_tok); AT(L, at, w_img); AT(L, at, b_img); AT(L, at, pos_tok); AT(L, at, pos_img); AT(L, at, pos_layer);
  AT(L, at, norm_s); AT(L, at, norm_b);
  for (int l = 0; l < g.ctx_layers; ++l) {
    const BlockLeaves &s = L.layer[l], &d = at.layer[l];
    AT(s, d, ln0_s); AT(s, d, ln0_b); AT(s, d, ln1_s); AT(s, d, ln1_b); AT(s, d, wq); AT(s, d, bq); AT(s, d, wk); AT(s, d, bk);
    AT(s, d, wv); AT(s, d, bv); AT(s, d, wo); AT(s, d, bo); AT(s, d, w1); AT(s, d, b1); AT(s, d, w2); AT(s, d, b2);
  }
  base = L.total;
  AT(L, at, e_cls); AT(L, at, e_mask); AT(L, at, e_pb); AT(L, at, e_pk); AT(L, at, e_pos); AT(L, at, e_lnb); AT(L, at, e_lns);
  for (int l = 0; l < g.enc_layers; ++l) {
    const BlockLeaves &s = L.enc[l], &d = at.enc[l];
    AT(s, d, bk); AT(s, d, wk); AT(s, d, bq); AT(s, d, wq); AT(s, d, bv); AT(s, d, wv); AT(s, d, bo); AT(s, d, wo); AT(s, d, ls1); AT(s, d, ls2);
    AT(s, d, b1); AT(s, d, w1); AT(s, d, b2); AT(s, d, w2); AT(s, d, ln0_b); AT(s, d, ln0_s); AT(s, d, ln1_b); AT(s, d, ln1_s);
  }
#undef AT
  return 0;
}

// the packer's refusals: the first tensor (in the enumeration's order) that is absent or of another size is named, and nothing
// of the output is written
static int refusals(const Geom& g) {
  const TrainLayout L = make_train_layout(g);
  std::vector<float> v((size_t)(L.total + L.enc_total), 0.25f);
  const Checkpoint full = cut_checkpoint(g, L, v.data());
  const std::string ep = "encoder_image_encoder_", head = "output_head_" + generated_leaves(g)[3].flat + "/kernel";
  auto refused = [&](const Checkpoint& ck, const std::string& want) -> int {
    HostImages H;
    H.hn.assign(3, 7.f); H.encf.assign(3, 7.f); H.enc16.assign(3, 7); H.encd16.assign(3, 7); H.lk.assign(3, nullptr); H.lb.assign(3, nullptr);
    H.at.w_tok = H.at.enc[1].wq = 77;
    REQUIRE(!pack_serving(g, false, ck, H), "the packer accepted a checkpoint without %s", want.c_str());
    REQUIRE(H.missing == want, "the packer names '%s', not '%s'", H.missing.c_str(), want.c_str());
    REQUIRE(H.hn == std::vector<float>(3, 7.f) && H.encf == H.hn && H.enc16 == std::vector<uint16_t>(3, 7) && H.encd16 == H.enc16 &&
            H.lk.size() == 3 && H.lb.size() == 3 && H.leaves.empty() && H.at.w_tok == 77 && H.at.enc[1].wq == 77,
            "the packer wrote before it refused %s", want.c_str());
    return 0;
  };
  // one tensor of every pack kind, one that backs nothing, a generated leaf, and per-layer tensors of a layer > 0
  const std::string one[] = {"task_pos_embedding", ep + "layernorm_scale", ep + "encoder_layer_0_mlp_fc2_kernel",
                             ep + "embeddings_patch_embeddings_projection_kernel", ep + "embeddings_patch_embeddings_projection_bias",
                             ep + "embeddings_position_embeddings", ep + "embeddings_cls_token", ep + "embeddings_mask_token", head,
                             "Transformer_0/encoderblock_1/MlpBlock_0/Dense_0/bias", ep + "encoder_layer_1_norm2_bias",
                             ep + "encoder_layer_1_attention_attention_value_kernel"};
  for (const std::string& n : one) {
    REQUIRE(full.t.count(n), "no tensor %s in the checkpoint", n.c_str());
    Checkpoint ck = full;
    ck.t.erase(n);
    if (refused(ck, n + " (absent)")) return 1;
    for (int d = -1; d <= 1; d += 2) {
      ck = full;
      ck.t[n].second += d;
      if (refused(ck, n + " (wrong size)")) return 1;
    }
  }
  // two at once: the context encoder comes before the generated leaves, those before the image encoder; inside a layer the
  // buffer order decides
  const std::string two[][2] = {{"Transformer_0/encoderblock_1/LayerNorm_1/bias", head},
                                {head, ep + "embeddings_cls_token"},
                                {ep + "encoder_layer_1_attention_attention_query_bias", ep + "encoder_layer_1_attention_attention_key_kernel"},
                                {ep + "encoder_layer_0_norm2_scale", ep + "encoder_layer_1_attention_attention_query_kernel"}};
  for (const auto& pr : two) {
    Checkpoint ck = full;
    REQUIRE(ck.t.erase(pr[0]) && ck.t.count(pr[1]), "no tensors %s / %s in the checkpoint", pr[0].c_str(), pr[1].c_str());
    ck.t[pr[1]].second += 1;
    if (refused(ck, pr[0] + " (absent)")) return 1;
  }
  printf("MID geometry: the packer names the first absent or wrong-sized tensor and writes nothing\n");
  return 0;
}

static int check(const Geom& g, const char* name, bool bf) {
  const TrainLayout L = make_train_layout(g);
  const size_t n = (size_t)(L.total + L.enc_total);
  std::vector<float> v(n);                           // exact size: an index past the vector is an ASAN report
  for (size_t i = 0; i < n; ++i) v[i] = value(i);
  const float* P = v.data();
  const int C = g.C, F = g.ctx_mlp, E = g.E, Fe = g.enc_mlp, S = g.S(), T = g.T;

  // ------------------------------------------------------------ the real host packer, and the enumeration it runs
  const Checkpoint ck = cut_checkpoint(g, L, P);
  HostImages H;
  REQUIRE(pack_serving(g, bf, ck, H), "%s: the packer misses %s", name, H.missing.c_str());
  std::vector<Placed> in_ctx, in_enc, all;
  Offsets at{};
  const int64_t hn_total = served_ctx(g, L, at, [&](const Tensor& t, int64_t dst) { in_ctx.push_back({t, dst}); }).hn;
  const Extent enc_total = served_enc(g, L, at, [&](const Tensor& t, int64_t dst) { in_enc.push_back({t, dst}); });
  REQUIRE(memcmp(&at, &H.at, sizeof at) == 0, "%s: the packer returns other offsets than the enumeration", name);
  all = in_ctx;
  all.insert(all.end(), in_enc.begin(), in_enc.end());
  if (members_agree(g, L, H.at, all, name)) return 1;

  // ------------------------------------------------------------ context encoder: hvla_load_weights' push order
  {
    std::vector<float> ref;
    auto push = [&](long off, int64_t numel) {
      const size_t o = ref.size();
      ref.resize(o + ((numel + 3) / 4) * 4, 0.f);
      memcpy(ref.data() + o, P + off, numel * 4);
    };
    push(L.w_tok, (int64_t)g.lang_dim * C); push(L.b_tok, C); push(L.w_img, (int64_t)E * C); push(L.b_img, C);
    push(L.pos_tok, (int64_t)T * C); push(L.pos_img, C); push(L.pos_layer, C); push(L.norm_s, C); push(L.norm_b, C);
    for (int l = 0; l < g.ctx_layers; ++l) {
      const BlockLeaves& c = L.layer[l];
      push(c.ln0_s, C); push(c.ln0_b, C);
      push(c.wq, (int64_t)C * C); push(c.bq, C); push(c.wk, (int64_t)C * C); push(c.bk, C); push(c.wv, (int64_t)C * C); push(c.bv, C);
      push(c.wo, (int64_t)C * C); push(c.bo, C);
      push(c.ln1_s, C); push(c.ln1_b, C);
      push(c.w1, (int64_t)C * F); push(c.b1, F); push(c.w2, (int64_t)F * C); push(c.b2, C);
    }
    const CopyTable t = ctx_table(g, L);
    REQUIRE(t.nseg <= MAX_SEGS && (size_t)t.dst_total == ref.size(), "%s: context table covers %lld of %zu floats", name,
            (long long)t.dst_total, ref.size());
    std::vector<float> got(ref.size(), 0.f);
    std::vector<uint8_t> cnt(ref.size(), 0);
    apply(t, P, got, cnt);
    if (same(got, ref, name, "hn_f32") || once(cnt, 0, name, "hn_f32")) return 1;     // (no tensor of these geometries needs padding)
    if (same(H.hn, ref, name, "the packer's hn_f32")) return 1;
    int64_t o = 0;                                     // every tensor where the transcription has it, one behind the other
    for (const Placed& p : in_ctx) {
      REQUIRE(p.t.pack == PAD4 && p.dst == o, "%s: %s at %lld of hn_f32, behind a tensor that ends at %lld", name, checkpoint_name(p.t).c_str(),
              (long long)p.dst, (long long)o);
      o += (p.t.n + 3) / 4 * 4;
      REQUIRE((size_t)o <= ref.size() && memcmp(&ref[p.dst], P + p.t.src, p.t.n * 4) == 0, "%s: the transcription has %s elsewhere", name,
              checkpoint_name(p.t).c_str());
    }
    REQUIRE((size_t)o == ref.size() && hn_total == o, "%s: the enumeration fills %lld of %zu floats of hn_f32", name, (long long)o, ref.size());
  }

  // ------------------------------------------------------------ W_cat / b_cat: pack::pack_wcat on the leaves cut from the vector
  {
    const PackedLayout lay = build_layout(g);
    const int Gtot = lay.pl.Gm + lay.pl.Gv, ntiles = Gtot / 32, KS = C / 16;
    const long G = L.G;
    auto leaves = generated_leaves(g);
    std::vector<std::vector<float>> K(leaves.size());
    std::vector<const float*> lk(leaves.size()), lb(leaves.size());
    for (size_t i = 0; i < leaves.size(); ++i) {
      K[i].resize((size_t)C * leaves[i].size);
      for (int k = 0; k < C; ++k) memcpy(&K[i][(size_t)k * leaves[i].size], P + L.wcat + (long)k * G + leaves[i].offset, leaves[i].size * 4);
      lk[i] = K[i].data();
      lb[i] = P + L.bcat + leaves[i].offset;
    }
    std::vector<uint16_t> hi, lo;
    std::vector<float> bc;
    pack::pack_wcat(lay, leaves, lk, lb, C, hi, lo, bc);
    REQUIRE(H.leaves.size() == leaves.size() && H.lk.size() == lk.size() && H.lb.size() == lb.size(), "%s: the packer's leaves", name);
    for (size_t i = 0; i < leaves.size(); ++i)         // the packer hands pack_wcat the same leaves: the same planes come out
      REQUIRE(H.leaves[i].flat == leaves[i].flat && H.leaves[i].offset == leaves[i].offset && H.leaves[i].size == leaves[i].size &&
              memcmp(H.lk[i], lk[i], K[i].size() * 4) == 0 && memcmp(H.lb[i], lb[i], leaves[i].size * 4) == 0,
              "%s: the packer's inputs to pack_wcat differ at leaf %zu", name, i);
    std::vector<uint16_t> ghi(hi.size(), 0xffff), glo(hi.size(), 0xffff);
    std::vector<float> gbc(bc.size(), -1.f);
    std::vector<uint8_t> cnt(hi.size(), 0), cntb(bc.size(), 0);
    const float* wcat = P + L.wcat;
    for (int pt = 0; pt < ntiles; ++pt)
      for (int tau = 0; tau < 32; ++tau) {
        const int ref = lay.perm[(size_t)pt * 32 + tau];
        gbc[(size_t)pt * 32 + tau] = ref >= 0 ? P[L.bcat + ref] : 0.f;
        ++cntb[(size_t)pt * 32 + tau];
        for (int ks = 0; ks < KS; ++ks)
          for (int r = 0; r < 16; ++r) {
            const float w = ref >= 0 ? wcat[(size_t)(16 * ks + r) * G + ref] : 0.f;
            const size_t o = (((size_t)pt * KS + ks) * 64 + rho_of_tau(tau) + 32 * (r >> 3)) * 8 + (r & 7);
            split_pair(w, ghi.at(o), glo.at(o));
            ++cnt[o];
          }
      }
    if (same(ghi, hi, name, "wcat_hi") || same(glo, lo, name, "wcat_lo") || same(gbc, bc, name, "b_cat")) return 1;
    if (once(cnt, 0, name, "wcat") || once(cntb, 0, name, "b_cat")) return 1;
  }

  // ------------------------------------------------------------ image encoder: hvla_load_weights' off16 / offf order
  {
    const float* X = P + L.total;
    const int p = g.patch, Kreal = p * p * 3, Kp = 2 * ((Kreal + 63) / 64 * 64), Kp1 = Kp / 2;
    const size_t per_layer16 = (size_t)3 * E * E + (size_t)E * E + (size_t)2 * E * Fe;
    std::vector<uint16_t> w16((size_t)E * Kp + per_layer16 * g.enc_layers), d16(w16.size(), 0);
    const size_t per_layerf = (size_t)3 * E + E + Fe + E + 6 * (size_t)E;
    std::vector<float> wf((size_t)E + (size_t)S * E + 2 * (size_t)E + per_layerf * g.enc_layers);
    size_t o16 = 0, of = 0, cur16 = 0, curf = 0;
    auto mark16 = [&](size_t k) { cur16 = o16; o16 += k; };
    auto markf = [&](size_t k) { curf = of; of += k; };
    const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
    const float *e_pk = X + L.e_pk, *e_pb = X + L.e_pb, *e_pos = X + L.e_pos, *e_cls = X + L.e_cls;
    mark16((size_t)E * Kp);
    markf(E);
    for (int nn = 0; nn < E; ++nn) {
      double bacc = e_pb[nn];
      for (int k = 0; k < Kp1; ++k) {
        uint16_t hi = 0, lo = 0;
        if (k < Kreal) {
          const int c = k % 3;
          const double wk = e_pk[(size_t)k * E + nn];
          const float w = (float)(wk * 256.0 / (255.0 * sd[c]));
          hi = pack::to16(w, bf);
          lo = pack::to16(w - pack::from16(hi, bf), bf);
          bacc += wk * (128.0 / 255.0 - mean[c]) / sd[c];
        }
        w16[cur16 + (size_t)nn * Kp + k] = hi;
        w16[cur16 + (size_t)nn * Kp + Kp1 + k] = lo;
      }
      wf[curf + nn] = (float)bacc;
    }
    markf((size_t)S * E);
    for (size_t i = 0; i < (size_t)S * E; ++i) wf[curf + i] = e_pos[i] + (i < (size_t)E ? e_cls[i] : 0.f);
    markf(E); memcpy(&wf[curf], X + L.e_lns, E * 4);
    markf(E); memcpy(&wf[curf], X + L.e_lnb, E * 4);
    auto tr = [&](long src, int K, int N, size_t dst) { pack::pack_matrix_t(X + src, K, N, bf, &w16[dst], &d16[dst]); };
    for (int i = 0; i < g.enc_layers; ++i) {
      const BlockLeaves& s = L.enc[i];
      mark16((size_t)3 * E * E);
      tr(s.wq, E, E, cur16); tr(s.wk, E, E, cur16 + (size_t)E * E); tr(s.wv, E, E, cur16 + (size_t)2 * E * E);
      mark16((size_t)E * E); tr(s.wo, E, E, cur16);
      mark16((size_t)E * Fe); tr(s.w1, E, Fe, cur16);
      mark16((size_t)Fe * E); tr(s.w2, Fe, E, cur16);
      markf(3 * E);
      memcpy(&wf[curf], X + s.bq, E * 4); memcpy(&wf[curf + E], X + s.bk, E * 4); memcpy(&wf[curf + 2 * E], X + s.bv, E * 4);
      markf(E); memcpy(&wf[curf], X + s.bo, E * 4);
      markf(Fe); memcpy(&wf[curf], X + s.b1, Fe * 4);
      markf(E); memcpy(&wf[curf], X + s.b2, E * 4);
      const long six[6] = {s.ln0_s, s.ln0_b, s.ln1_s, s.ln1_b, s.ls1, s.ls2};
      for (int q = 0; q < 6; ++q) { markf(E); memcpy(&wf[curf], X + six[q], E * 4); }
    }
    REQUIRE(o16 == w16.size() && of == wf.size(), "%s: the transcription does not fill its own buffers", name);

    const EncMap m = enc_map(g, L);
    REQUIRE(m.vec.nseg <= MAX_SEGS && (size_t)m.n16 == w16.size() && (size_t)m.vec.dst_total == wf.size() && m.Kp == Kp && m.Kreal == Kreal,
            "%s: encoder map sizes", name);
    std::vector<uint16_t> g16(w16.size(), 0xffff), gd16(w16.size(), 0);
    std::vector<float> gf(wf.size(), -1.f);
    std::vector<uint8_t> c16(w16.size(), 0), cd16(w16.size(), 0), cf(wf.size(), 0);
    apply(m.vec, P, gf, cf);
    for (int i = 0; i < m.S * m.E; ++i) {                                              // publish_pos_kernel
      gf.at(m.f_pos + i) = P[m.src_pos + i] + (i < m.E ? P[m.src_cls + i] : 0.f);
      ++cf[m.f_pos + i];
    }
    for (int nn = 0; nn < m.E; ++nn) {                                                 // publish_patch_kernel
      gf.at(m.f_bpatch + nn) = patch_channel(P + m.src_pk, P[m.src_pb + nn], m.E, nn, m.Kreal, m.Kp, bf, &g16.at((size_t)nn * m.Kp));
      ++cf[m.f_bpatch + nn];
      for (int k = 0; k < m.Kp; ++k) ++c16[(size_t)nn * m.Kp + k];
    }
    int tiles = 0;
    for (int l = 0; l < m.layers; ++l)                                                 // publish_transpose_kernel, tile by tile
      for (int i = 0; i < ENC_MATS; ++i) {
        const EncMat& e = m.mat[i];
        REQUIRE(e.K % TR_TILE == 0 && e.N % TR_TILE == 0, "%s: matrix %d is no multiple of the tile", name, i);
        if (l == 0) { REQUIRE(e.tile0 == tiles, "%s: tile0 of matrix %d", name, i); tiles += (e.K / TR_TILE) * (e.N / TR_TILE); }
        const float* src = P + e.src + l * m.mat_src_stride;
        const size_t dst = (size_t)(e.dst + l * m.mat_dst_stride);
        for (int k = 0; k < e.K; ++k)
          for (int nn = 0; nn < e.N; ++nn) {
            const size_t o = dst + (size_t)nn * e.K + k;
            round_pair(src[(size_t)k * e.N + nn], bf, g16.at(o), gd16.at(o));
            ++c16[o]; ++cd16[o];
          }
      }
    REQUIRE(m.layers == 0 || tiles == m.tiles_per_layer, "%s: tiles per layer", name);
    if (same(g16, w16, name, "enc16") || same(gd16, d16, name, "encd16") || same(gf, wf, name, "encf32")) return 1;
    if (once(c16, 0, name, "enc16") || once(cd16, (size_t)E * Kp, name, "encd16") || once(cf, 0, name, "encf32")) return 1;
    if (same(H.enc16, w16, name, "the packer's enc16") || same(H.encd16, d16, name, "the packer's encd16") ||
        same(H.encf, wf, name, "the packer's encf32"))
      return 1;
    int64_t at16 = 0, atf = 0;                         // every tensor where the transcription has it, one behind the other in its buffer
    for (const Placed& p : in_enc) {
      const Tensor& t = p.t;
      const std::string nm = checkpoint_name(t);
      if (t.pack == CLS || t.pack == UNSERVED) { REQUIRE(p.dst == -1, "%s: %s has a place", name, nm.c_str()); continue; }
      const bool is16 = t.pack == TRANSPOSE || t.pack == PATCH;
      int64_t& o = is16 ? at16 : atf;
      REQUIRE(p.dst == o, "%s: %s at %lld, behind a tensor that ends at %lld", name, nm.c_str(), (long long)p.dst, (long long)o);
      o += t.pack == PATCH ? (int64_t)E * Kp : t.n;
      REQUIRE((size_t)o <= (is16 ? w16.size() : wf.size()), "%s: %s ends past its buffer", name, nm.c_str());
      if (t.pack == COPY) REQUIRE(memcmp(&wf[p.dst], P + t.src, t.n * 4) == 0, "%s: the transcription has %s elsewhere", name, nm.c_str());
      if (t.pack == TRANSPOSE) {                       // its four corners: [K][N] -> [N][K]
        const int K = t.K, N = (int)(t.n / t.K);
        const int kn[4][2] = {{0, 0}, {K - 1, 0}, {0, N - 1}, {K - 1, N - 1}};
        for (const auto& c : kn) {
          uint16_t w, d;
          round_pair(P[t.src + (int64_t)c[0] * N + c[1]], bf, w, d);
          REQUIRE(w16[p.dst + (int64_t)c[1] * K + c[0]] == w && d16[p.dst + (int64_t)c[1] * K + c[0]] == d,
                  "%s: the transcription has %s elsewhere", name, nm.c_str());
        }
      }
      if (t.pack == PATCH) REQUIRE(p.dst == 0 && t.src == L.total + L.e_pk && t.K == Kreal, "%s: the patch embedding", name);
      if (t.pack == PATCH_BIAS) REQUIRE(p.dst == 0 && t.src == L.total + L.e_pb, "%s: the patch bias", name);
      if (t.pack == POS) REQUIRE(p.dst == E && t.src == L.total + L.e_pos && t.n == (int64_t)S * E, "%s: the position table", name);
    }
    REQUIRE((size_t)at16 == w16.size() && (size_t)atf == wf.size() && enc_total.n16 == at16 && enc_total.nf == atf,
            "%s: the enumeration fills %lld of %zu and %lld of %zu elements", name, (long long)at16, w16.size(), (long long)atf, wf.size());
  }
  printf("%s (%s): %zu training values, every buffer byte for byte, every element once\n", name, bf ? "bf16" : "f16", n);
  return 0;
}

int main() {
  for (int tau = 0; tau < 32; ++tau) {
    const int rho = rho_of_tau(tau);
    REQUIRE(16 * ((rho >> 2) & 1) + (rho & 3) + 4 * (rho >> 3) == tau, "rho_of_tau(%d)", tau);
  }
  Geom mid{112, 14, 128, 2, 2, 512, 64, 2, 4, 128, 4, 7, 5.f, 5.f, 128, 2, 4, 256, 12, 64, 1};
  Geom full{224, 14, 768, 12, 12, 3072, 64, 4, 4, 128, 4, 7, 5.f, 5.f, 128, 6, 4, 512, 32, 768, 1};
  if (check(mid, "MID geometry", false) || check(mid, "MID geometry", true)) return 1;
  if (check(full, "README geometry", false)) return 1;
  if (refusals(mid)) return 1;
  printf("OK\n");
  return 0;
}
