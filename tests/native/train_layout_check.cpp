// CPU-only check of csrc/train_layout.h (the flat training vector and the generated policy's leaves in a row of theta).  Built and
// run by tests/test_host_sanitizers.py with g++ -fsanitize=address,undefined.  Over the TINY, MID and README geometries and the
// layer-count edges: every policy member is the offset of the generated leaf of its flax name (written out here), no member is -1
// but the LayerScale of blocks that have none, the members tile [0, total), [0, enc_total) and [0, G) without gap or overlap, and
// the predicate refuses one layer more than the tables hold before make_train_layout is reached.  Prints `name offset` for every
// member of the MID and README vectors under hypervla.train.train_param_layout's names: the pytest compares the two.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "train_layout.h"

using namespace hvla;

#define REQUIRE(c, ...) do { if (!(c)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static Geom mid() { return Geom{112, 14, 128, 2, 2, 512, 64, 2, 4, 128, 4, 7, 5.f, 5.f, 128, 2, 4, 256, 12, 64, 1}; }
static Geom tiny() { return Geom{56, 14, 32, 2, 2, 64, 16, 2, 2, 32, 4, 7, 5.f, 5.f, 16, 2, 2, 32, 8, 24, 1}; }
static Geom readme() { return Geom{224, 14, 768, 12, 12, 3072, 64, 4, 4, 128, 4, 7, 5.f, 5.f, 128, 6, 4, 512, 32, 768, 1}; }

struct Member { std::string name; long offset, size; };

// the 16 (+ 2) leaves of one block of width D and MLP width F, under the names of the three checkpoints
enum Flavour { CTX, DINO, POLICY };
static void block_members(std::vector<Member>& v, const BlockLeaves& y, Flavour fl, int l, long D, long F) {
  const std::string n = std::to_string(l);
  if (fl == DINO) {
    const std::string b = "encoder_image_encoder_encoder_layer_" + n + "_", a = b + "attention_attention_";
    v.push_back({a + "key_bias", y.bk, D}); v.push_back({a + "key_kernel", y.wk, D * D}); v.push_back({a + "query_bias", y.bq, D});
    v.push_back({a + "query_kernel", y.wq, D * D}); v.push_back({a + "value_bias", y.bv, D}); v.push_back({a + "value_kernel", y.wv, D * D});
    v.push_back({b + "attention_output_dense_bias", y.bo, D}); v.push_back({b + "attention_output_dense_kernel", y.wo, D * D});
    v.push_back({b + "layer_scale1_lambda1", y.ls1, D}); v.push_back({b + "layer_scale2_lambda1", y.ls2, D});
    v.push_back({b + "mlp_fc1_bias", y.b1, F}); v.push_back({b + "mlp_fc1_kernel", y.w1, D * F}); v.push_back({b + "mlp_fc2_bias", y.b2, D});
    v.push_back({b + "mlp_fc2_kernel", y.w2, F * D}); v.push_back({b + "norm1_bias", y.ln0_b, D}); v.push_back({b + "norm1_scale", y.ln0_s, D});
    v.push_back({b + "norm2_bias", y.ln1_b, D}); v.push_back({b + "norm2_scale", y.ln1_s, D});
    return;
  }
  const char* sep = fl == CTX ? "/" : "_";
  const std::string b = std::string(fl == CTX ? "Transformer_0/encoderblock_" : "encoder_Transformer_0_encoderblock_") + n + sep;
  const std::string a = b + "MultiHeadDotProductAttention_0" + sep;
  auto nm = [&](const std::string& p, const char* x, const char* leaf) { return p + x + sep + leaf; };
  v.push_back({nm(b, "LayerNorm_0", "scale"), y.ln0_s, D}); v.push_back({nm(b, "LayerNorm_0", "bias"), y.ln0_b, D});
  v.push_back({nm(b, "LayerNorm_1", "scale"), y.ln1_s, D}); v.push_back({nm(b, "LayerNorm_1", "bias"), y.ln1_b, D});
  v.push_back({nm(a, "query", "kernel"), y.wq, D * D}); v.push_back({nm(a, "query", "bias"), y.bq, D});
  v.push_back({nm(a, "key", "kernel"), y.wk, D * D}); v.push_back({nm(a, "key", "bias"), y.bk, D});
  v.push_back({nm(a, "value", "kernel"), y.wv, D * D}); v.push_back({nm(a, "value", "bias"), y.bv, D});
  v.push_back({nm(a, "out", "kernel"), y.wo, D * D}); v.push_back({nm(a, "out", "bias"), y.bo, D});
  v.push_back({nm(b, "MlpBlock_0", fl == CTX ? "Dense_0/kernel" : "Dense_0_kernel"), y.w1, D * F});
  v.push_back({nm(b, "MlpBlock_0", fl == CTX ? "Dense_0/bias" : "Dense_0_bias"), y.b1, F});
  v.push_back({nm(b, "MlpBlock_0", fl == CTX ? "Dense_1/kernel" : "Dense_1_kernel"), y.w2, F * D});
  v.push_back({nm(b, "MlpBlock_0", fl == CTX ? "Dense_1/bias" : "Dense_1_bias"), y.b2, D});
}

// the members tile [0, end): sorted by offset, each starts where the one before ended
static int tiles(std::vector<Member> v, long end, const char* what) {
  std::sort(v.begin(), v.end(), [](const Member& a, const Member& b) { return a.offset < b.offset; });
  long at = 0;
  for (const Member& m : v) {
    REQUIRE(m.offset >= 0, "%s: %s is %ld", what, m.name.c_str(), m.offset);
    REQUIRE(m.offset == at, "%s: %s at %ld, the one before ends at %ld", what, m.name.c_str(), m.offset, at);
    at += m.size;
  }
  REQUIRE(at == end, "%s: the members end at %ld, the vector at %ld", what, at, end);
  return 0;
}

static int check(const Geom& g, const char* name, bool print) {
  REQUIRE(train_refusal(g) == nullptr, "%s: refused: %s", name, train_refusal(g));
  const TrainLayout L = make_train_layout(g);
  REQUIRE(L.policy_ok, "%s: a policy leaf was not found", name);
  const long C = g.C, E = g.E, D = g.D;
  // ---- the hypernetwork's part
  std::vector<Member> hyper = {{"task_token_projection/kernel", L.w_tok, (long)g.lang_dim * C}, {"task_token_projection/bias", L.b_tok, C},
                               {"initial_image_projection/kernel", L.w_img, E * C}, {"initial_image_projection/bias", L.b_img, C},
                               {"task_pos_embedding", L.pos_tok, (long)g.T * C}, {"initial_image_pos_embedding", L.pos_img, C},
                               {"layer_pos_embedding", L.pos_layer, C}, {"Transformer_0/encoder_norm/scale", L.norm_s, C},
                               {"Transformer_0/encoder_norm/bias", L.norm_b, C}, {"W_cat", L.wcat, C * L.G}, {"b_cat", L.bcat, L.G}};
  for (int l = 0; l < g.ctx_layers; ++l) {
    block_members(hyper, L.layer[l], CTX, l, C, g.ctx_mlp);
    REQUIRE(L.layer[l].ls1 == -1 && L.layer[l].ls2 == -1, "%s: context block %d has a LayerScale offset", name, l);
  }
  if (tiles(hyper, L.total, name)) return 1;
  // ---- the shared DINOv2 leaves
  const long Se = g.P() + 1;
  std::vector<Member> enc = {{"encoder_image_encoder_embeddings_cls_token", L.e_cls, E}, {"encoder_image_encoder_embeddings_mask_token", L.e_mask, E},
                             {"encoder_image_encoder_embeddings_patch_embeddings_projection_bias", L.e_pb, E},
                             {"encoder_image_encoder_embeddings_patch_embeddings_projection_kernel", L.e_pk, (long)g.patch * g.patch * 3 * E},
                             {"encoder_image_encoder_embeddings_position_embeddings", L.e_pos, Se * E},
                             {"encoder_image_encoder_layernorm_bias", L.e_lnb, E}, {"encoder_image_encoder_layernorm_scale", L.e_lns, E}};
  for (int l = 0; l < g.enc_layers; ++l) block_members(enc, L.enc[l], DINO, l, E, g.enc_mlp);
  if (tiles(enc, L.enc_total, name)) return 1;
  // ---- the generated policy in a row of theta: every member is the generated leaf of its flax name
  std::vector<Member> pol = {{"action_head_continuous_head_bias", L.bc, g.A()}, {"action_head_continuous_head_kernel", L.wc, D * g.A()},
                             {"action_head_discrete_head_bias", L.bd, g.horizon}, {"action_head_discrete_head_kernel", L.wd, D * g.horizon},
                             {"encoder_Transformer_0_encoder_norm_bias", L.nb, D}, {"encoder_Transformer_0_encoder_norm_scale", L.ns, D},
                             {"encoder_image_embedding_projection_bias", L.bp, D}, {"encoder_image_embedding_projection_kernel", L.wp, E * D},
                             {"encoder_pos_embedding", L.pos, (long)g.pos_rows() * D}};
  for (int l = 0; l < g.L; ++l) {
    block_members(pol, L.pol[l], POLICY, l, D, g.M);
    REQUIRE(L.pol[l].ls1 == -1 && L.pol[l].ls2 == -1, "%s: policy block %d has a LayerScale offset", name, l);
  }
  std::map<std::string, LeafInfo> leaf;
  const std::vector<LeafInfo> leaves = generated_leaves(g);
  for (const LeafInfo& l : leaves) leaf[l.flat] = l;
  REQUIRE(pol.size() == leaves.size(), "%s: %zu policy members, %zu generated leaves", name, pol.size(), leaves.size());
  for (const Member& m : pol) {
    REQUIRE(leaf.count(m.name), "%s: no generated leaf %s", name, m.name.c_str());
    REQUIRE(leaf[m.name].offset == m.offset && leaf[m.name].size == m.size, "%s: %s at %ld (%ld elements), the leaf at %lld (%lld)", name,
            m.name.c_str(), m.offset, m.size, (long long)leaf[m.name].offset, (long long)leaf[m.name].size);
  }
  if (tiles(pol, L.G, name)) return 1;
  if (print) {
    printf("## %s %ld\n", name, L.total + L.enc_total);
    for (const Member& m : hyper) printf("%s %ld\n", m.name.c_str(), m.offset);
    for (const Member& m : enc) printf("%s %ld\n", m.name.c_str(), L.total + m.offset);
  }
  return 0;
}

static int refused(Geom g, const char* what, const char* text) {
  const char* why = train_refusal(g);      // what every hvla_train_* entry asks before it builds the layout
  REQUIRE(why && strstr(why, text), "%s: %s", what, why ? why : "not refused");
  return 0;
}

int main() {
  if (check(tiny(), "TINY", false) || check(mid(), "MID", true) || check(readme(), "README", true)) return 1;
  Geom g = mid();
  g.ctx_layers = 0; if (check(g, "ctx_layers 0", false)) return 1;
  g.ctx_layers = CTX_MAX_LAYERS; if (check(g, "ctx_layers 8", false)) return 1;
  g = mid(); g.enc_layers = 0; if (check(g, "enc_layers 0", false)) return 1;
  g.enc_layers = ENC_MAX_LAYERS; if (check(g, "enc_layers 24", false)) return 1;
  g = mid(); g.L = 1; if (check(g, "L 1", false)) return 1;
  g.L = TRAIN_MAX_POLICY_LAYERS; if (check(g, "L 16", false)) return 1;
  g = readme(); g.ctx_layers = CTX_MAX_LAYERS; g.enc_layers = ENC_MAX_LAYERS; g.L = TRAIN_MAX_POLICY_LAYERS;
  if (check(g, "README, every table full", false)) return 1;
  static_assert(CTX_MAX_LAYERS == 8 && ENC_MAX_LAYERS == 24 && TRAIN_MAX_POLICY_LAYERS == 16, "the limits of include/hvla.h");
  g = mid(); g.L = 17; if (refused(g, "L 17", "too many layers")) return 1;
  g = mid(); g.ctx_layers = 9; if (refused(g, "ctx_layers 9", "too many layers")) return 1;
  g = mid(); g.enc_layers = 25; if (refused(g, "enc_layers 25", "too many layers")) return 1;
  g = mid(); g.lang_in_policy = 1; if (refused(g, "use_language_token", "use_language_token")) return 1;
  printf("OK\n");
  return 0;
}
