// CPU-only check of csrc/train_layout.h for use_language_token geometries (hvla_train_language_tokens), beside
// tests/native/train_layout_check.cpp.  Built and run by tests/test_lang_train_host.py with g++ -fsanitize=address,undefined.  With the
// option: TrainLayout::wl / bl are the offsets of the generated leaves encoder_language_token_projection_{kernel,bias}, L.pos spans
// pos_rows() = T + P + 1 rows, every policy member tiles [0, G) together with the two, and the refusal is lifted only for a caller
// that asked.  Without it: wl == bl == -1 and the members in front of W_cat are where they are with the option (the option only
// lengthens a row of theta).  Prints `## name n_params G wl bl pos` per geometry: the pytest compares them with
// hypervla.train.train_param_layout and hypervla.config.generated_leaves.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "train_layout.h"

using namespace hvla;

#define REQUIRE(c, ...) do { if (!(c)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static Geom mid() { return Geom{112, 14, 128, 2, 2, 512, 64, 2, 4, 128, 4, 7, 5.f, 5.f, 128, 2, 4, 256, 12, 64, 1}; }
static Geom readme() { return Geom{224, 14, 768, 12, 12, 3072, 64, 4, 4, 128, 4, 7, 5.f, 5.f, 128, 6, 4, 512, 32, 768, 1}; }

struct Member { std::string name; long offset, size; };

static int check(Geom g, const char* name) {
  g.lang_in_policy = 1;
  REQUIRE(train_refusal(g) && strstr(train_refusal(g), "use_language_token"), "%s: not refused by default", name);
  REQUIRE(train_refusal(g, false) && strstr(train_refusal(g, false), "use_language_token"), "%s: not refused with the setting off", name);
  REQUIRE(train_refusal(g, true) == nullptr, "%s: refused although asked for: %s", name, train_refusal(g, true));
  const TrainLayout L = make_train_layout(g);
  REQUIRE(L.policy_ok, "%s: a policy leaf was not found", name);
  const std::vector<LeafInfo> leaves = generated_leaves(g);
  auto leaf = [&](const std::string& n) -> const LeafInfo* {
    for (const LeafInfo& l : leaves) if (l.flat == n) return &l;
    return nullptr;
  };
  const long D = g.D, E = g.E;
  const LeafInfo *kl = leaf("encoder_language_token_projection_kernel"), *bl = leaf("encoder_language_token_projection_bias"),
                 *pos = leaf("encoder_pos_embedding");
  REQUIRE(kl && bl && pos, "%s: the generated leaves lack a language leaf", name);
  REQUIRE(L.wl == kl->offset && kl->size == (long)g.lang_dim * D, "%s: wl %ld, the leaf at %lld (%lld)", name, L.wl, (long long)kl->offset, (long long)kl->size);
  REQUIRE(L.bl == bl->offset && bl->size == D, "%s: bl %ld, the leaf at %lld (%lld)", name, L.bl, (long long)bl->offset, (long long)bl->size);
  REQUIRE(g.pos_rows() == g.T + g.P() + 1, "%s: pos_rows %d", name, g.pos_rows());
  REQUIRE(L.pos == pos->offset && pos->size == (long)g.pos_rows() * D, "%s: pos %ld, the leaf at %lld (%lld)", name, L.pos, (long long)pos->offset, (long long)pos->size);
  // every policy member, the two new ones among them, tiles a row of theta
  std::vector<Member> pol = {{"bc", L.bc, g.A()}, {"wc", L.wc, D * g.A()}, {"bd", L.bd, g.horizon}, {"wd", L.wd, D * g.horizon}, {"nb", L.nb, D},
                             {"ns", L.ns, D}, {"bp", L.bp, D}, {"wp", L.wp, E * D}, {"bl", L.bl, D}, {"wl", L.wl, (long)g.lang_dim * D},
                             {"pos", L.pos, (long)g.pos_rows() * D}};
  for (int l = 0; l < g.L; ++l) {
    const BlockLeaves& y = L.pol[l];
    const long F = g.M;
    const Member blk[] = {{"ln0_s", y.ln0_s, D}, {"ln0_b", y.ln0_b, D}, {"ln1_s", y.ln1_s, D}, {"ln1_b", y.ln1_b, D}, {"wq", y.wq, D * D}, {"bq", y.bq, D},
                          {"wk", y.wk, D * D}, {"bk", y.bk, D}, {"wv", y.wv, D * D}, {"bv", y.bv, D}, {"wo", y.wo, D * D}, {"bo", y.bo, D},
                          {"w1", y.w1, D * F}, {"b1", y.b1, F}, {"w2", y.w2, F * D}, {"b2", y.b2, D}};
    for (const Member& m : blk) pol.push_back({"pol[" + std::to_string(l) + "]." + m.name, m.offset, m.size});
    REQUIRE(y.ls1 == -1 && y.ls2 == -1, "%s: policy block %d has a LayerScale offset", name, l);
  }
  REQUIRE(pol.size() == leaves.size(), "%s: %zu policy members, %zu generated leaves", name, pol.size(), leaves.size());
  std::sort(pol.begin(), pol.end(), [](const Member& a, const Member& b) { return a.offset < b.offset; });
  long at = 0;
  for (const Member& m : pol) {
    REQUIRE(m.offset == at, "%s: %s at %ld, the one before ends at %ld", name, m.name.c_str(), m.offset, at);
    at += m.size;
  }
  REQUIRE(at == L.G, "%s: the policy members end at %ld, a row of theta at %ld", name, at, L.G);
  // the same geometry without the option
  Geom off = g;
  off.lang_in_policy = 0;
  const TrainLayout L0 = make_train_layout(off);
  REQUIRE(L0.policy_ok && L0.wl == -1 && L0.bl == -1, "%s without the option: wl %ld bl %ld", name, L0.wl, L0.bl);
  REQUIRE(off.pos_rows() == off.S() && L0.G + (long)(g.lang_dim + 1 + g.T) * D == L.G, "%s: G %ld without, %ld with the option", name, L0.G, L.G);
  REQUIRE(L0.wcat == L.wcat && L0.norm_b == L.norm_b && L0.w_tok == L.w_tok && L0.enc_total == L.enc_total && L0.e_pos == L.e_pos,
          "%s: the option moved a member in front of W_cat or among the encoder leaves", name);
  REQUIRE(L0.wp == L.wp && L0.bp == L.bp && L0.pol[g.L - 1].wv == L.pol[g.L - 1].wv && L0.pos == L.pos - (long)(g.lang_dim + 1) * D,
          "%s: the option moved a policy leaf in front of the language leaves", name);
  printf("## %s %ld %ld %ld %ld %ld\n", name, L.total + L.enc_total, L.G, L.wl, L.bl, L.pos);
  return 0;
}

int main() {
  Geom g = mid();
  if (check(g, "T12")) return 1;
  g.T = 2; if (check(g, "T2")) return 1;
  g.T = 3; if (check(g, "T3")) return 1;
  g.T = 32; if (check(g, "T32")) return 1;
  g.image_size = 224; if (check(g, "T32-P256")) return 1;
  if (check(readme(), "README")) return 1;
  g = mid(); g.lang_in_policy = 1; g.L = TRAIN_MAX_POLICY_LAYERS + 1;
  REQUIRE(train_refusal(g, true) && strstr(train_refusal(g, true), "too many layers"), "L 17 with the option: not refused for its layers");
  printf("OK\n");
  return 0;
}
