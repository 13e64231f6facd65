// CPU-only check of csrc/accept.h (the geometries hvla_create serves).  Built and run by tests/test_host_sanitizers.py with
// g++ -fsanitize=address,undefined.  Walks the predicate over a grid of configs -- from four accepted bases (the MID and README
// geometries, with and without use_language_token), every PAIR of fields through every pair of edge values: lower edge, upper edge,
// one step outside each, zero, negative, INT_MAX -- and requires that the verdict arrives without a runtime error (UBSan aborts on
// a division by zero or a signed overflow), that a zero divisor is HVLA_E_SHAPE, and that everything ACCEPTED meets the launch-side
// preconditions of the kernels, computed by the functions the launchers themselves call.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "accept.h"

using namespace hvla;

#define REQUIRE(c, ...) do { if (!(c)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static hvla_config base_mid() {
  hvla_config c;
  memset(&c, 0, sizeof c);
  c.struct_size = sizeof c;
  c.image_size = 112; c.patch = 14; c.enc_dim = 128; c.enc_layers = 2; c.enc_heads = 2; c.enc_mlp = 512;
  c.dim = 64; c.layers = 2; c.heads = 4; c.mlp = 128; c.horizon = 4; c.action_dim = 7; c.tanh_scale = 5.f; c.max_action = 5.f;
  c.ctx_dim = 128; c.ctx_layers = 2; c.ctx_heads = 4; c.ctx_mlp = 256; c.lang_tokens = 12; c.lang_dim = 64; c.scale_context = 1;
  c.max_batch = 8; c.enc_dtype = HVLA_ENC_F16; c.streams = 1; c.clip_target = 1;
  return c;
}
static hvla_config base_full() {
  hvla_config c = base_mid();
  c.image_size = 224; c.enc_dim = 768; c.enc_layers = 12; c.enc_heads = 12; c.enc_mlp = 3072;
  c.layers = 4; c.ctx_layers = 6; c.ctx_mlp = 512; c.lang_tokens = 32; c.lang_dim = 768;
  return c;
}

struct Field {
  const char* name;
  int32_t hvla_config::*member;
  std::vector<int> values;
};
static const std::vector<Field>& fields() {
  static const std::vector<Field> f = {
      {"image_size", &hvla_config::image_size, {0, -14, 14, 32, 84, 112, 128, 224, 226, 448, INT_MAX}},
      {"patch", &hvla_config::patch, {0, -1, 1, 4, 7, 8, 14, 16, 28, INT_MAX}},
      {"enc_dim", &hvla_config::enc_dim, {0, -128, 64, 128, 192, 256, 640, 1024, 1152, INT_MAX}},
      {"enc_layers", &hvla_config::enc_layers, {-1, 0, 1, 24, 25, INT_MAX}},
      {"enc_heads", &hvla_config::enc_heads, {0, -2, 1, 2, 4, 10, 12, 16, 17, INT_MAX}},
      {"enc_mlp", &hvla_config::enc_mlp, {0, -128, 64, 128, 192, 3072, 4096, INT_MAX}},
      {"dim", &hvla_config::dim, {0, 32, 64, 128, INT_MAX}},
      {"layers", &hvla_config::layers, {-1, 0, 1, 4, 5, 7, 8, 9, 64, INT_MAX}},
      {"heads", &hvla_config::heads, {0, 2, 4, 8, INT_MAX}},
      {"mlp", &hvla_config::mlp, {0, -32, 16, 32, 48, 128, 160, 256, 288, 768, 800, 1024, INT_MAX - 30, INT_MAX}},
      {"horizon", &hvla_config::horizon, {0, -1, 1, 4, 8, 16, 32, 33, 65536, INT_MAX}},
      {"action_dim", &hvla_config::action_dim, {0, -1, 1, 2, 4, 7, 8, 9, 32, 33, 65536, INT_MAX}},
      {"ctx_dim", &hvla_config::ctx_dim, {0, -32, 16, 32, 64, 96, 128, 256, INT_MAX}},
      {"ctx_layers", &hvla_config::ctx_layers, {-1, 0, 1, 8, 9, INT_MAX}},
      {"ctx_heads", &hvla_config::ctx_heads, {0, -1, 1, 2, 3, 4, 8, 16, 32, 64, 128, INT_MAX}},
      {"ctx_mlp", &hvla_config::ctx_mlp, {0, -16, 8, 16, 24, 48, 512, 1008, 1024, 4096, INT_MAX - 14, INT_MAX}},
      {"lang_tokens", &hvla_config::lang_tokens, {0, -1, 1, 2, 15, 32, 33, 38, 39, INT_MAX - 1, INT_MAX}},
      {"lang_dim", &hvla_config::lang_dim, {0, -4, 2, 4, 20, 22, 64, 392, 768, INT_MAX - 3}},
      {"max_batch", &hvla_config::max_batch, {0, -1, 1, INT_MAX}},
      {"enc_dtype", &hvla_config::enc_dtype, {-1, 0, 1, 2}},
      {"streams", &hvla_config::streams, {-1, 0, 1, 2, 3}},
  };
  return f;
}

static long n_configs = 0, n_accepted = 0;

// the launch-side preconditions of an accepted geometry
static int check_accepted(const hvla_config& c, int lang) {
#define CFG "image %d patch %d enc %d/%d/%d/%d policy %d/%d/%d/%d act %dx%d ctx %d/%d/%d/%d lang %dx%d (in policy %d)", c.image_size, c.patch, \
            c.enc_dim, c.enc_layers, c.enc_heads, c.enc_mlp, c.dim, c.layers, c.heads, c.mlp, c.horizon, c.action_dim, c.ctx_dim,             \
            c.ctx_layers, c.ctx_heads, c.ctx_mlp, c.lang_tokens, c.lang_dim, lang
  REQUIRE(c.patch > 0 && c.image_size > 0 && c.image_size % c.patch == 0, CFG);
  const int grid = c.image_size / c.patch, P = grid * grid, NW = P / 32;
  REQUIRE(P == 64 || P == 256, CFG);                               // policy_kernel<2> / <8>; an image tile of the encoder's aligned GEMMs
  REQUIRE(c.dim == 64 && c.heads == 4 && c.layers >= 1 && c.mlp >= 32 && c.mlp % 32 == 0, CFG);
  REQUIRE(c.horizon >= 1 && c.action_dim >= 2 && c.horizon * c.action_dim <= 32, CFG);      // the head's one 32-row tile
  REQUIRE(c.enc_heads > 0 && c.enc_dim == 64 * c.enc_heads && c.enc_dim % 128 == 0 && c.enc_dim <= 1024 && c.enc_mlp % 128 == 0 && c.enc_mlp > 0, CFG);
  REQUIRE(c.enc_layers >= 0 && c.enc_layers <= ENC_MAX_LAYERS && c.ctx_layers >= 0 && c.ctx_layers <= CTX_MAX_LAYERS, CFG);
  REQUIRE(c.ctx_heads > 0 && c.ctx_dim % c.ctx_heads == 0, CFG);
  const int hc = c.ctx_dim / c.ctx_heads;
  REQUIRE(hc % 4 == 0 && hc >= 4, CFG);                            // the score loop's k-steps of four features
  REQUIRE(c.ctx_dim % 16 == 0 && CTX_THREADS % c.ctx_dim == 0 && c.ctx_mlp % 16 == 0 && c.ctx_mlp > 0, CFG);   // column tiles; the CLS projection's parts
  REQUIRE(c.lang_tokens >= 2 && c.lang_tokens + 2 <= 48 && c.lang_dim % 4 == 0 && c.lang_dim > 0, CFG);       // three 16-key tiles, 16-byte token loads
  REQUIRE(ctx_encoder_lds_bytes(c.lang_tokens, c.ctx_dim, c.ctx_mlp, c.enc_dim) <= LDS_LIMIT, CFG);
  // the staged token chunk and the CLS row + partial sums fit the third buffer
  const size_t big = ctx_big_elems(c.lang_tokens, c.ctx_dim, c.ctx_mlp, c.enc_dim);
  REQUIRE(big >= (size_t)c.lang_tokens * 132 && big >= (size_t)c.enc_dim + CTX_THREADS &&
          big >= (size_t)(c.lang_tokens + 2) * (3 * c.ctx_dim + 4) && big >= (size_t)(c.lang_tokens + 2) * (c.ctx_mlp + 4), CFG);
  // the policy kernel, in the form the context will launch and in the other one's formula when that one is a geometry too
  PolicyLayout pl{};
  LangLayout ll;
  policy_offsets(geom_of(c, lang), pl, ll);
  REQUIRE(pl.Gv > pl.v_layer0 && pl.v_layer0 % 4 == 0 && pl.Gv % 4 == 0, CFG);
  REQUIRE(policy_lds_bytes(NW, lang != 0, pl.Gv - pl.v_layer0) <= LDS_LIMIT, CFG);
  REQUIRE(policy_lds_bytes_of(c, lang) == policy_lds_bytes(NW, lang != 0, pl.Gv - pl.v_layer0), CFG);
  if (lang) {
    REQUIRE(c.lang_tokens <= 32 && c.lang_dim % 64 == 0, CFG);
    REQUIRE(accept_geometry(c, 0) == HVLA_OK, CFG);                // the language form needs more LDS, never less
    REQUIRE(policy_lds_bytes_of(c, 0) <= policy_lds_bytes_of(c, 1), CFG);
  }
  const EncSizes z{1, P, P + 1, c.enc_dim, c.enc_mlp, c.enc_heads, c.patch, c.enc_layers, 256, 2, true, true, false};
  REQUIRE(plan_call(z).ok, CFG);
  return 0;
}

static int visit(const hvla_config& c, int lang) {
  ++n_configs;
  const int v = accept_geometry(c, lang);
  REQUIRE(v == HVLA_OK || v == HVLA_E_SHAPE || v == HVLA_E_DTYPE, "verdict %d", v);
  if (c.heads == 0 || c.patch == 0 || c.enc_heads == 0 || c.ctx_heads == 0)
    REQUIRE(v != HVLA_OK && (v == HVLA_E_SHAPE || (c.enc_dtype != HVLA_ENC_F16 && c.enc_dtype != HVLA_ENC_BF16)), "zero divisor accepted");
  if (c.enc_dtype != HVLA_ENC_F16 && c.enc_dtype != HVLA_ENC_BF16) REQUIRE(v == HVLA_E_DTYPE, "dtype %d: verdict %d", c.enc_dtype, v);
  if (v != HVLA_OK) return 0;
  ++n_accepted;
  return check_accepted(c, lang);
}

struct Pin {
  const char* what;
  hvla_config c;
  int lang, want;
};
template <typename F> static hvla_config with(hvla_config c, F f) { f(c); return c; }

int main() {
  const hvla_config bases[2] = {base_mid(), base_full()};
  for (const hvla_config& b : bases)
    for (int lang = 0; lang < 2; ++lang) {
      REQUIRE(accept_geometry(b, lang) == HVLA_OK, "a base geometry is refused");
      if (visit(b, lang)) return 1;
      const std::vector<Field>& F = fields();
      for (size_t i = 0; i < F.size(); ++i)
        for (size_t j = i + 1; j < F.size(); ++j)
          for (int vi : F[i].values)
            for (int vj : F[j].values) {
              hvla_config c = b;
              c.*(F[i].member) = vi;
              c.*(F[j].member) = vj;
              if (visit(c, lang)) { printf("  at %s = %d, %s = %d, lang %d\n", F[i].name, vi, F[j].name, vj, lang); return 1; }
            }
    }
  // an out-of-range language flag
  REQUIRE(accept_geometry(base_mid(), 2) == HVLA_E_SHAPE && accept_geometry(base_mid(), -1) == HVLA_E_SHAPE, "language flag");

  // ---- the edges by name: the verdict of each is part of the contract
  const hvla_config M = base_mid(), Fl = base_full();
  const Pin pins[] = {
      {"zero heads", with(M, [](hvla_config& c) { c.heads = 0; }), 0, HVLA_E_SHAPE},
      {"zero patch", with(M, [](hvla_config& c) { c.patch = 0; }), 0, HVLA_E_SHAPE},
      {"zero enc_heads", with(M, [](hvla_config& c) { c.enc_heads = 0; }), 0, HVLA_E_SHAPE},
      {"zero ctx_heads", with(M, [](hvla_config& c) { c.ctx_heads = 0; }), 0, HVLA_E_SHAPE},
      {"horizon 0", with(M, [](hvla_config& c) { c.horizon = 0; }), 0, HVLA_E_SHAPE},
      {"action_dim 1", with(M, [](hvla_config& c) { c.action_dim = 1; c.horizon = 4; }), 0, HVLA_E_SHAPE},
      {"negative encoder widths", with(M, [](hvla_config& c) { c.enc_dim = -128; c.enc_heads = -2; }), 0, HVLA_E_SHAPE},
      {"negative layers", with(M, [](hvla_config& c) { c.enc_layers = -1; }), 0, HVLA_E_SHAPE},
      {"negative ctx layers", with(M, [](hvla_config& c) { c.ctx_layers = -1; }), 0, HVLA_E_SHAPE},
      {"32 head rows", with(M, [](hvla_config& c) { c.horizon = 4; c.action_dim = 8; }), 0, HVLA_OK},
      {"33 head rows", with(M, [](hvla_config& c) { c.horizon = 3; c.action_dim = 11; }), 0, HVLA_E_SHAPE},
      {"horizon 16 x 2", with(M, [](hvla_config& c) { c.horizon = 16; c.action_dim = 2; }), 0, HVLA_OK},
      {"overflowing head rows", with(M, [](hvla_config& c) { c.horizon = 65536; c.action_dim = 65536; }), 0, HVLA_E_SHAPE},
      {"mlp 32", with(M, [](hvla_config& c) { c.mlp = 32; }), 0, HVLA_OK},
      {"mlp 48", with(M, [](hvla_config& c) { c.mlp = 48; }), 0, HVLA_E_SHAPE},
      {"mlp 160 x 3 layers", with(Fl, [](hvla_config& c) { c.mlp = 160; c.layers = 3; }), 0, HVLA_OK},
      // the policy kernel's LDS at P = 256 (NW = 8): 5632 floats are left for layers x (576 + mlp) + 160
      {"P 256: 7 layers at mlp 128", with(Fl, [](hvla_config& c) { c.layers = 7; }), 0, HVLA_OK},
      {"P 256: 8 layers at mlp 128", with(Fl, [](hvla_config& c) { c.layers = 8; }), 0, HVLA_E_SHAPE},
      {"P 256: mlp 768 at 4 layers", with(Fl, [](hvla_config& c) { c.mlp = 768; }), 0, HVLA_OK},
      {"P 256: mlp 800 at 4 layers", with(Fl, [](hvla_config& c) { c.mlp = 800; }), 0, HVLA_E_SHAPE},
      {"P 256: mlp 1024 at 4 layers", with(Fl, [](hvla_config& c) { c.mlp = 1024; }), 0, HVLA_E_SHAPE},
      // ... with the language prefix's 8 KiB: 3584 floats
      {"P 256, language: 4 layers at mlp 128", with(Fl, [](hvla_config& c) { c.layers = 4; }), 1, HVLA_OK},
      {"P 256, language: 5 layers at mlp 128", with(Fl, [](hvla_config& c) { c.layers = 5; }), 1, HVLA_E_SHAPE},
      {"P 256, language: mlp 256 at 4 layers", with(Fl, [](hvla_config& c) { c.mlp = 256; }), 1, HVLA_OK},
      {"P 256, language: mlp 288 at 4 layers", with(Fl, [](hvla_config& c) { c.mlp = 288; }), 1, HVLA_E_SHAPE},
      {"language: 33 tokens", with(Fl, [](hvla_config& c) { c.lang_tokens = 33; }), 1, HVLA_E_SHAPE},
      {"language: lang_dim 96", with(Fl, [](hvla_config& c) { c.lang_dim = 96; }), 1, HVLA_E_SHAPE},
      {"language: 2 tokens", with(Fl, [](hvla_config& c) { c.lang_tokens = 2; }), 1, HVLA_OK},
      // context encoder
      {"context head width 4", with(M, [](hvla_config& c) { c.ctx_dim = 32; c.ctx_heads = 8; c.ctx_mlp = 16; }), 0, HVLA_OK},
      {"context head width 2", with(M, [](hvla_config& c) { c.ctx_dim = 32; c.ctx_heads = 16; }), 0, HVLA_E_SHAPE},
      {"context head width 2 at 64", with(M, [](hvla_config& c) { c.ctx_dim = 64; c.ctx_heads = 32; }), 0, HVLA_E_SHAPE},
      {"context head width 1", with(M, [](hvla_config& c) { c.ctx_dim = 128; c.ctx_heads = 128; }), 0, HVLA_E_SHAPE},
      {"context one head of 128", with(M, [](hvla_config& c) { c.ctx_heads = 1; }), 0, HVLA_OK},
      {"ctx_dim 96", with(M, [](hvla_config& c) { c.ctx_dim = 96; }), 0, HVLA_E_SHAPE},
      {"1 token", with(M, [](hvla_config& c) { c.lang_tokens = 1; }), 0, HVLA_E_SHAPE},
      {"2 tokens", with(M, [](hvla_config& c) { c.lang_tokens = 2; }), 0, HVLA_OK},
      {"38 tokens of 20", with(M, [](hvla_config& c) { c.lang_tokens = 38; c.lang_dim = 20; }), 0, HVLA_OK},
      {"39 tokens", with(M, [](hvla_config& c) { c.lang_tokens = 39; }), 0, HVLA_E_SHAPE},
      {"lang_dim 22", with(M, [](hvla_config& c) { c.lang_dim = 22; }), 0, HVLA_E_SHAPE},
      {"ctx_mlp 1008 at 38 tokens", with(M, [](hvla_config& c) { c.lang_tokens = 38; c.ctx_mlp = 1008; }), 0, HVLA_E_SHAPE},
      // encoder
      {"enc_dim 1024", with(Fl, [](hvla_config& c) { c.enc_dim = 1024; c.enc_heads = 16; c.enc_mlp = 1152; }), 0, HVLA_OK},
      {"enc_dim 1152", with(Fl, [](hvla_config& c) { c.enc_dim = 1152; c.enc_heads = 18; }), 0, HVLA_E_SHAPE},
      {"36 patches", with(M, [](hvla_config& c) { c.image_size = 84; }), 0, HVLA_E_SHAPE},
      {"32 x 32 image of 4 x 4 patches", with(M, [](hvla_config& c) { c.image_size = 32; c.patch = 4; }), 0, HVLA_OK},
      {"no encoder layers", with(M, [](hvla_config& c) { c.enc_layers = 0; }), 0, HVLA_OK},
      {"no context layers", with(M, [](hvla_config& c) { c.ctx_layers = 0; }), 0, HVLA_OK},
      {"dtype", with(M, [](hvla_config& c) { c.enc_dtype = 2; }), 0, HVLA_E_DTYPE},
      {"three streams", with(M, [](hvla_config& c) { c.streams = 3; }), 0, HVLA_E_SHAPE},
  };
  for (const Pin& p : pins) {
    const int v = accept_geometry(p.c, p.lang);
    REQUIRE(v == p.want, "%s: verdict %d, expected %d", p.what, v, p.want);
    if (visit(p.c, p.lang)) return 1;
  }
  // the two limits above come from the layout, not from this file: the largest accepted layer count / mlp are exactly where the
  // shared LDS function crosses 160 KiB
  for (int lang = 0; lang < 2; ++lang) {
    hvla_config c = Fl;
    int lmax = 0, mmax = 0;
    for (c.layers = 1; c.layers <= 64; ++c.layers)
      if (accept_geometry(c, lang) == HVLA_OK) lmax = c.layers;
    c.layers = 4;
    for (c.mlp = 32; c.mlp <= 4096; c.mlp += 32)
      if (accept_geometry(c, lang) == HVLA_OK) mmax = c.mlp;
    c = Fl; c.layers = lmax;
    REQUIRE(policy_lds_bytes_of(c, lang) <= LDS_LIMIT, "layers");
    c.layers = lmax + 1;
    REQUIRE(policy_lds_bytes_of(c, lang) > LDS_LIMIT, "layers + 1");
    c = Fl; c.mlp = mmax;
    REQUIRE(policy_lds_bytes_of(c, lang) <= LDS_LIMIT, "mlp");
    c.mlp = mmax + 32;
    REQUIRE(policy_lds_bytes_of(c, lang) > LDS_LIMIT, "mlp + 32");
    printf("P = 256, use_language_token %d: layers <= %d at mlp 128, mlp <= %d at 4 layers\n", lang, lmax, mmax);
    REQUIRE(lmax == (lang ? 4 : 7) && mmax == (lang ? 256 : 768), "limits moved: layers %d mlp %d", lmax, mmax);
  }
  printf("%ld configs, %ld accepted\n", n_configs, n_accepted);
  REQUIRE(n_configs > 3000 && n_accepted > 300, "the grid is too thin");
  printf("OK\n");
  return 0;
}
