// CPU-only check of the training layout of share_layer_index=False models (csrc/train_layout.h: the run table, Gh, train_refusal's
// four-argument form, group_tiles).  Built and run by tests/test_layer_tokens_train_host.py with
// g++ -fsanitize=address,undefined.  For every geometry below it requires that
//   - train_refusal answers as the table in main() says for every combination of the three switches;
//   - the layout has NL - 1 runs, contiguous in theta, tiling [0, G); their head columns tile [0, Gh) once without shared heads and
//     the block range L times with them; no run reads token 0; pos_layer holds NL C floats and wcat / bcat C Gh / Gh;
//   - every tile of the three grouped products stays inside its run, its operands and its output: walked element range by element
//     range against the sizes of ctx [B][NL C], W_h [C][Gh], b_h [Gh], theta / dtheta [B][G], dctx [B][NL C]; the tiles of a kind
//     cover every (run column) / (run K index) exactly once.
// It prints "RUN <case> <tcol> <width> <hcol> <token>" and "LAYOUT <case> NL G Gh total pos_layer wcat bcat" for the test to compare
// with hypervla.train.token_runs / train_param_layout.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "train_layout.h"

using namespace hvla;

#define REQUIRE(c, ...) do { if (!(c)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static Geom mid() {
  Geom g{112, 14, 128, 2, 2, 512, 64, 2, 4, 128, 4, 7, 5.f, 5.f, 128, 2, 4, 256, 12, 64, 1};
  return g;
}
static Geom readme() {
  Geom g = mid();
  g.image_size = 224; g.E = 768; g.enc_layers = 12; g.enc_heads = 12; g.enc_mlp = 3072; g.L = 4; g.ctx_layers = 6; g.ctx_mlp = 512; g.T = 32; g.lang_dim = 768;
  return g;
}

static int check_tiles(const char* name, const Geom& g, const TrainLayout& L) {
  const long C = g.C, NLC = (long)L.NL * C, G = L.G, Gh = L.Gh;
  for (int tile : {64, 128}) {
    for (int kind = 0; kind < 2; ++kind) {
      std::vector<int> seen(G, 0);
      for (const BGTile& t : group_tiles(g, L, kind, tile)) {
        REQUIRE(t.k0 == 0 && t.k1 == 0 && t.n0 % tile == 0 && t.n0 < t.N, "%s kind %d: tile %d of %d", name, kind, t.n0, t.N);
        const long n1 = t.n0 + tile < t.N ? t.n0 + tile : t.N;
        const long theta0 = kind == 0 ? t.c : t.b, head0 = kind == 0 ? t.b : t.c;
        REQUIRE(t.a % C == 0 && t.a >= C && t.a + C <= NLC, "%s kind %d: context row at %ld", name, kind, t.a);       // a whole row, never token 0's
        REQUIRE(theta0 >= 0 && theta0 + n1 <= G && head0 >= 0 && head0 + n1 <= Gh, "%s kind %d: columns %ld / %ld + %ld", name, kind, theta0, head0, n1);
        if (kind == 0) REQUIRE(t.bias == t.b, "%s: bias and kernel columns differ", name);
        int run = -1;
        for (int r = 0; r < L.nruns; ++r)
          if (theta0 == L.run[r].tcol) run = r;
        REQUIRE(run >= 0 && t.N == L.run[run].width && head0 == L.run[run].hcol && t.a == (long)L.run[run].token * C, "%s kind %d: a tile of no run", name, kind);
        for (long n = t.n0; n < n1; ++n) ++seen[theta0 + n];
      }
      for (long c = 0; c < G; ++c) REQUIRE(seen[c] == 1, "%s kind %d tile %d: theta column %ld in %d tiles", name, kind, tile, c, seen[c]);
    }
  }
  const int kc = group_kchunk(L);
  REQUIRE(kc % 32 == 0 && kc >= 128, "%s: K chunk %d", name, kc);
  std::vector<int> seen(G, 0);
  for (const BGTile& t : group_tiles(g, L, 2, kc)) {
    REQUIRE(t.n0 == 0 && t.N == g.C && t.k0 % 32 == 0 && t.k0 < t.k1 && t.k1 - t.k0 <= kc, "%s dctx: chunk [%d, %d)", name, t.k0, t.k1);
    REQUIRE(t.c % C == 0 && t.c >= C && t.c + C <= NLC, "%s dctx: output row at %ld", name, t.c);
    REQUIRE(t.a >= 0 && t.a + t.k1 <= G && t.b >= 0 && t.b + t.k1 <= Gh, "%s dctx: K range past an operand", name);
    int run = -1;
    for (int r = 0; r < L.nruns; ++r)
      if (t.a == L.run[r].tcol) run = r;
    REQUIRE(run >= 0 && t.k1 <= L.run[run].width && t.b == L.run[run].hcol && t.c == (long)L.run[run].token * C, "%s dctx: a chunk of no run", name);
    for (long k = t.k0; k < t.k1; ++k) ++seen[t.a + k];
  }
  for (long c = 0; c < G; ++c) REQUIRE(seen[c] == 1, "%s dctx: theta column %ld in %d chunks", name, c, seen[c]);
  return 0;
}

static int check(const char* name, Geom g, bool shared) {
  g.layer_tokens = 1; g.shared_block_heads = shared ? 1 : 0;
  const TrainLayout L = make_train_layout(g);
  REQUIRE(L.policy_ok, "%s: policy leaves", name);
  REQUIRE(L.NL == g.NL() && L.nruns == L.NL - 1, "%s: %d runs for %d tokens", name, L.nruns, L.NL);
  long at = 0, block = 0;
  std::vector<int> head(L.Gh, 0);
  for (int r = 0; r < L.nruns; ++r) {
    const TokenRun& t = L.run[r];
    REQUIRE(t.tcol == at && t.width > 0, "%s: run %d starts at %ld, not %ld", name, r, t.tcol, at);
    REQUIRE(t.token >= 1 && t.token < L.NL, "%s: run %d reads token %d", name, r, t.token);
    REQUIRE(t.hcol >= 0 && t.hcol + t.width <= L.Gh, "%s: run %d head columns", name, r);
    for (long c = 0; c < t.width; ++c) ++head[t.hcol + c];
    at += t.width;
    if (r == 2) block = t.width;                  // action_head, encoder_norm, then the blocks
    printf("RUN %s %ld %ld %ld %d\n", name, t.tcol, t.width, t.hcol, t.token);
  }
  REQUIRE(at == L.G, "%s: the runs end at %ld of %ld", name, at, L.G);
  REQUIRE(L.Gh == (shared ? L.G - (long)(g.L - 1) * block : L.G), "%s: Gh %ld", name, L.Gh);
  for (long c = 0; c < L.Gh; ++c) {
    const bool in_block = c >= L.run[2].hcol && c < L.run[2].hcol + block;
    REQUIRE(head[c] == (shared && in_block ? g.L : 1), "%s: head column %ld read by %d runs", name, c, head[c]);
  }
  REQUIRE(L.norm_s - L.pos_layer >= (long)L.NL * g.C && L.bcat - L.wcat == (long)g.C * L.Gh && L.total - L.bcat == L.Gh, "%s: extents", name);
  printf("LAYOUT %s %d %ld %ld %ld %ld %ld %ld\n", name, L.NL, L.G, L.Gh, L.total, L.pos_layer, L.wcat, L.bcat);
  return check_tiles(name, g, L);
}

int main() {
  // ---- the refusal matrix: (language, differential, layer tokens, shared heads) x the three switches
  for (int geo = 0; geo < 16; ++geo) {
    Geom g = mid();
    g.lang_in_policy = geo & 1; g.differential = (geo >> 1) & 1; g.layer_tokens = (geo >> 2) & 1; g.shared_block_heads = (geo >> 3) & 1;
    if (g.shared_block_heads && !g.layer_tokens) continue;
    for (int sw = 0; sw < 8; ++sw) {
      const bool lang = sw & 1, diff = (sw >> 1) & 1, lt = (sw >> 2) & 1;
      const char* why = train_refusal(g, lang, diff, lt);
      // the first flavour the caller did not ask for, in train_refusal(g)'s order: layer tokens, differential, language
      const char* want = g.layer_tokens && !lt ? "share_layer_index" : g.differential && !diff ? "use_differential_transformer" : g.lang_in_policy && !lang ? "use_language_token" : nullptr;
      REQUIRE((why == nullptr) == (want == nullptr), "geometry %d switches %d: %s", geo, sw, why ? why : "accepted");
      if (want) REQUIRE(strstr(why, want) != nullptr, "geometry %d switches %d: '%s' does not name %s", geo, sw, why, want);
      if (!lt) REQUIRE(why == train_refusal(g, lang, diff), "geometry %d switches %d: the three-argument form answers otherwise", geo, sw);
    }
    printf("REFUSAL %d ok\n", geo);
  }
  {
    Geom g = mid();
    g.layer_tokens = 1; g.L = TRAIN_MAX_POLICY_LAYERS + 1;
    REQUIRE(train_refusal(g, true, true, true) && strstr(train_refusal(g, true, true, true), "too many layers"), "17 policy layers");
    g.L = TRAIN_MAX_POLICY_LAYERS; g.lang_in_policy = 1;
    REQUIRE(!train_refusal(g, true, true, true) && make_train_layout(g).policy_ok && make_train_layout(g).nruns == TRAIN_MAX_RUNS, "16 policy layers with language tokens");
    Geom plain = mid();
    const TrainLayout P = make_train_layout(plain);
    REQUIRE(P.NL == 1 && P.nruns == 0 && P.Gh == P.G && P.norm_s - P.pos_layer >= plain.C, "a model without layer tokens");
  }
  for (int shared = 0; shared < 2; ++shared) {
    const std::string s = shared ? "-shared" : "";
    Geom lang = mid(), diff = mid(), l11 = mid(), s48 = mid();
    lang.lang_in_policy = 1; diff.differential = 1; l11.L = 11; s48.L = 4; s48.T = 38;
    if (check(("MID" + s).c_str(), mid(), shared) || check(("README" + s).c_str(), readme(), shared) || check(("LANG" + s).c_str(), lang, shared) ||
        check(("DIFF" + s).c_str(), diff, shared) || check(("L11" + s).c_str(), l11, shared) || check(("S48" + s).c_str(), s48, shared))
      return 1;
  }
  printf("OK\n");
  return 0;
}
