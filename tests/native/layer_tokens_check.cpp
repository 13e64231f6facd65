// CPU-only check of the host side of share_layer_index=False (csrc/layout.h layer_token_of / output_head_of, csrc/pack.h
// TokenSegments, csrc/accept.h).  Built and run by tests/test_layer_tokens_host.py with g++ -fsanitize=address,undefined.
// For every geometry below it packs W_cat from kernels whose every element is a non-zero function of (head, k, column), builds the
// segment list and requires that
//   - every non-padding position is in exactly one segment of its tile, a padding position in none, and no segment has token 0;
//   - a tile has exactly as many segments as distinct tokens;
//   - in a segment's fragment block the lanes of its own positions hold split_pair of the position's own head column (with
//     shared_block_heads: the shared head's), non-zero in the hi plane, and every other lane is zero in both planes;
//   - accept_geometry answers HVLA_OK at 48 context rows, HVLA_E_SHAPE at 49 and when the LDS formula with the rows exceeds 160 KiB.
// It prints "SEGMENTS <case> ..." with the number of tiles that hold more than one token, and "TOKEN <case> <flat leaf name> <token>" for the test to compare with hypervla.config.token_of.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "accept.h"
#include "pack.h"

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

static float value(int head, int k, int64_t col) { return 0.25f * (1 + head % 7) + 0.001f * k + 0.01f * (float)(col % 13); }

static int check(const char* name, const hvla_config& c, int lang, int shared, bool print, int diff = 0) {
  REQUIRE(accept_geometry(c, lang, diff, 1) == HVLA_OK, "%s is not accepted", name);
  Geom g = geom_of(c, lang, diff);
  g.layer_tokens = 1;
  g.shared_block_heads = shared;
  const PackedLayout lay = build_layout(g);
  const std::vector<LeafInfo> leaves = generated_leaves(g);
  const int C = g.C, KS = C / 16, NL = g.NL();
  REQUIRE(NL == g.L + 5 + lang && g.T + 1 + NL <= CTX_MAX_ROWS, "%s: NL %d", name, NL);
  // one kernel / bias per output head; with shared_block_heads the blocks' leaves of one name share theirs
  std::map<std::string, int> head_id;
  std::vector<std::vector<float>> hk, hb;
  std::vector<int> head_of_leaf(leaves.size());
  std::vector<const float*> lk(leaves.size()), lb(leaves.size());
  for (size_t i = 0; i < leaves.size(); ++i) {
    const std::string h = output_head_of(g, leaves[i].flat);
    REQUIRE(h.compare(0, 12, "output_head_") == 0, "%s", h.c_str());
    if (!head_id.count(h)) {
      const int id = (int)hk.size();
      head_id[h] = id;
      hk.emplace_back((size_t)C * leaves[i].size);
      hb.emplace_back((size_t)leaves[i].size);
      for (int k = 0; k < C; ++k)
        for (int64_t n = 0; n < leaves[i].size; ++n) hk[id][(size_t)k * leaves[i].size + n] = value(id, k, n);
      for (int64_t n = 0; n < leaves[i].size; ++n) hb[id][n] = -value(id, 0, n);
    }
    head_of_leaf[i] = head_id[h];
    REQUIRE((int64_t)hb[head_of_leaf[i]].size() == leaves[i].size, "%s: shared head of another size", leaves[i].flat.c_str());
    const int t = layer_token_of(g, leaves[i].flat);
    REQUIRE(t >= 1 && t < NL, "%s: token %d of %s", name, t, leaves[i].flat.c_str());
    if (print) printf("TOKEN %s %s %d\n", name, leaves[i].flat.c_str(), t);
  }
  REQUIRE((int)head_id.size() == (int)leaves.size() - (shared ? (g.L - 1) * (diff ? 17 : 16) : 0), "%s: %zu heads", name, head_id.size());
  for (size_t i = 0; i < leaves.size(); ++i) { lk[i] = hk[head_of_leaf[i]].data(); lb[i] = hb[head_of_leaf[i]].data(); }
  std::vector<uint16_t> hi, lo, shi, slo;
  std::vector<float> bc;
  pack::pack_wcat(lay, leaves, lk, lb, C, hi, lo, bc);
  const pack::TokenSegments s = pack::build_segments(g, lay, leaves);
  pack::pack_segments(s, C, hi, lo, shi, slo);
  const int Gtot = lay.pl.Gm + lay.pl.Gv, ntiles = Gtot / 32, nseg = (int)s.token.size();
  REQUIRE((int)s.tile_segs.size() == 2 * ntiles && (int)s.pos_token.size() == Gtot && (int)s.tile.size() == nseg, "%s: sizes", name);
  REQUIRE(shi.size() == (size_t)nseg * KS * 512 && slo.size() == shi.size(), "%s: block sizes", name);
  std::vector<int32_t> leaf_of(lay.pl.G);
  for (size_t i = 0; i < leaves.size(); ++i)
    for (int64_t j = 0; j < leaves[i].size; ++j) leaf_of[leaves[i].offset + j] = (int32_t)i;
  int next = 0, multi = 0, most = 0;
  for (int pt = 0; pt < ntiles; ++pt) {
    const int first = s.tile_segs[2 * pt], count = s.tile_segs[2 * pt + 1];
    REQUIRE(first == next && count >= 0 && first + count <= nseg, "%s: tile %d segments [%d, +%d)", name, pt, first, count);
    next = first + count;
    std::set<int> distinct;
    for (int i = 0; i < 32; ++i) {
      const int pos = pt * 32 + i, ref = lay.perm[pos], t = s.pos_token[pos];
      REQUIRE((ref < 0) == (t < 0), "%s: position %d", name, pos);
      if (t >= 0) {
        REQUIRE(t == layer_token_of(g, leaves[leaf_of[ref]].flat), "%s: position %d token", name, pos);
        distinct.insert(t);
      }
      int in = 0;
      for (int q = first; q < first + count; ++q) in += s.token[q] == t;
      REQUIRE(in == (t >= 0 ? 1 : 0), "%s: position %d is in %d segments of its tile", name, pos, in);
    }
    REQUIRE(count == (int)distinct.size(), "%s: tile %d has %d segments for %zu tokens", name, pt, count, distinct.size());
    multi += count > 1;
    most = count > most ? count : most;
    for (int q = first; q < first + count; ++q) {
      REQUIRE(s.tile[q] == pt && s.token[q] >= 1 && s.token[q] < NL, "%s: segment %d", name, q);
      for (int lane = 0; lane < 64; ++lane) {
        const int pos = pt * 32 + pack::tau_of_rho(lane & 31), ref = lay.perm[pos];
        const bool own = s.pos_token[pos] == s.token[q];
        for (int ks = 0; ks < KS; ++ks)
          for (int j = 0; j < 8; ++j) {
            const size_t o = (((size_t)q * KS + ks) * 64 + lane) * 8 + j;
            uint16_t wh = 0, wl = 0;
            if (own) {
              const int li = leaf_of[ref];
              pack::split_pair(value(head_of_leaf[li], 16 * ks + 8 * (lane >> 5) + j, ref - leaves[li].offset), wh, wl);
              REQUIRE(wh != 0, "%s: a zero test value", name);
            }
            REQUIRE(shi[o] == wh && slo[o] == wl, "%s: segment %d lane %d ks %d j %d: %04x %04x, expected %04x %04x", name, q, lane, ks,
                    j, shi[o], slo[o], wh, wl);
          }
      }
    }
  }
  REQUIRE(next == nseg, "%s: %d of %d segments belong to a tile", name, next, nseg);
  for (int pos = 0; pos < Gtot; ++pos)
    if (lay.perm[pos] >= 0) {
      const int li = leaf_of[lay.perm[pos]];
      REQUIRE(bc[pos] == hb[head_of_leaf[li]][lay.perm[pos] - leaves[li].offset], "%s: bias of position %d", name, pos);
    }
  printf("SEGMENTS %s tiles %d segments %d multi %d most %d NL %d\n", name, ntiles, nseg, multi, most, NL);
  return 0;
}

int main() {
  const hvla_config mid = base_mid(), full = base_full();
  if (check("MID", mid, 0, 0, true)) return 1;
  if (check("MID_shared", mid, 0, 1, false)) return 1;
  if (check("README", full, 0, 0, false)) return 1;
  if (check("README_shared", full, 0, 1, false)) return 1;
  {  // the largest accepted policies: 7 layers at mlp 128; 4 layers at mlp 768 with 38 language tokens, 38 + 1 + 9 = 48 rows
    hvla_config c = mid;
    c.image_size = 224; c.layers = 7;
    if (check("L7", c, 0, 0, false)) return 1;
    c.layers = 4; c.mlp = 768; c.lang_tokens = 38;
    if (check("M768_S48", c, 0, 1, false)) return 1;
    REQUIRE(accept_geometry(c, 0, 0, 1) == HVLA_OK, "48 rows refused");
    c.layers = 5; c.mlp = 128;
    REQUIRE(accept_geometry(c, 0, 0, 0) == HVLA_OK && accept_geometry(c, 0, 0, 1) == HVLA_E_SHAPE, "49 rows: not refused by the rows alone");
    c.layers = 4; c.lang_tokens = 39;
    REQUIRE(accept_geometry(c, 0, 0, 1) == HVLA_E_SHAPE, "39 language tokens");
  }
  {  // use_language_token: one token more, between the image projection and the position table
    hvla_config c = mid;
    c.lang_dim = 64;
    if (check("MID_lang", c, 1, 0, true)) return 1;
  }
  {  // use_differential_transformer: a block's vectors are 48 floats longer, so the blocks' vector runs start on odd multiples of 16 and
     // a tile holds the end of one block and the start of the next -- the tiles with two segments
    if (check("MID_diff", mid, 0, 0, true, 1)) return 1;
    if (check("README_diff_shared", full, 0, 1, false, 1)) return 1;
  }
  {  // an 11-layer policy's table alone (encoderblock_10 sorts before encoderblock_2); its arena is not packed
    hvla_config c = mid;
    c.layers = 11;
    Geom g = geom_of(c, 0);
    g.layer_tokens = 1;
    for (const LeafInfo& l : generated_leaves(g)) printf("TOKEN L11 %s %d\n", l.flat.c_str(), layer_token_of(g, l.flat));
  }
  {  // the LDS formula with the rows: a context MLP that fits with one layer token and not with NL
    hvla_config c = full;
    int found = 0;
    for (int f = 512; f <= 4096 && !found; f += 16) {
      c.ctx_mlp = f;
      const int NL = c.layers + 5;
      const bool fits1 = ctx_encoder_lds_bytes(c.lang_tokens, c.ctx_dim, f, c.enc_dim) <= LDS_LIMIT;
      const bool fitsN = ctx_encoder_lds_bytes(c.lang_tokens, c.ctx_dim, f, c.enc_dim, NL - 1) <= LDS_LIMIT;
      REQUIRE((accept_geometry(c, 0, 0, 0) == HVLA_OK) == fits1 && (accept_geometry(c, 0, 0, 1) == HVLA_OK) == fitsN, "ctx_mlp %d", f);
      found = fits1 && !fitsN;
    }
    REQUIRE(found, "no context MLP width separates the two LDS formulas");
  }
  REQUIRE(accept_geometry(mid, 0, 0, 2) == HVLA_E_SHAPE && accept_geometry(mid, 0, 0, -1) == HVLA_E_SHAPE, "layer_tokens outside {0, 1}");
  printf("OK\n");
  return 0;
}
