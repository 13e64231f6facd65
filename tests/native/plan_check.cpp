// CPU-only check of csrc/plan.h (the launch plan of run_encoder and the XCD tile order of the small GEMM kernels).  Built and run
// by tests/test_host_sanitizers.py with g++ -fsanitize=address,undefined; argv[1] = tests/native/encoder_plan_trace.txt, the
// launches of the dispatch that plan.h replaced (recorded on the CPU from run_encoder with its launch macro turned into a logger);
// argv[2] = tests/native/encoder_workspace_trace.txt, the workspace sizes and slice offsets of the expressions WorkspacePlan replaced.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "plan.h"

using namespace hvla;

#define REQUIRE(c, ...) do { if (!(c)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static const char* kernel_name(int k) {
  static const char* const gemm[] = {
#define HVLA_X(id, ...) #id,
      HVLA_GEMM_KERNELS(HVLA_X)
#undef HVLA_X
  };
  static const char* const other[] = {"IM2COL", "LN_GROUP", "LN_MEAN", "COLMEAN", "LN_FINAL"};
  return k >= IM2COL ? other[k - IM2COL] : gemm[k];
}
static const char* const attn_name[NUM_ATTN_KERNELS] = {"ATT", "ATT_U", "ATT_MAP"};

// One encode as run_encoder issues it: a line per launch (kernel id, grid, block, LDS bytes, category; the lnx_* numbers of a
// persistent fused-LayerNorm launch).  Returns the number of launches (the two memsets count), -1 when the call is refused;
// `bad` counts launches whose LDS size or kernel id is out of range.
struct Walk {
  std::string out;
  int n = 0, bad = 0;
  void line(const Launch& l, const char* name, const GemmPlan* g = nullptr) {
    char buf[160];
    int k = snprintf(buf, sizeof buf, "%s %u", name, l.grid);
    if (l.grid_y != 1) k += snprintf(buf + k, sizeof buf - k, "x%u", l.grid_y);
    k += snprintf(buf + k, sizeof buf - k, " %u %zu %d", l.block, l.lds, l.cat);
    if (g && g->lnx_G) k += snprintf(buf + k, sizeof buf - k, " lnx %d %d %d %d %d", g->lnx_G, g->lnx_rows_aligned, g->lnx_rounds_div, g->lnx_rows_xcd, g->lnx_rcp);
    out += buf;
    out += '\n';
    ++n;
    if (l.lds > LDS_LIMIT || l.grid == 0 || l.block == 0 || l.block > 1024) ++bad;
  }
  void other(const Launch& l) { line(l, kernel_name(l.kernel)); }
  void gemm(const GemmPlan& g) {
    for (const Launch* l : {&g.small, &g.main}) {
      if (!*l) continue;
      if (l->kernel >= NUM_GEMM_KERNELS) ++bad;
      line(*l, kernel_name(l->kernel), l == &g.main ? &g : nullptr);
    }
    if (!g.main) ++bad;
  }
  bool norm(const EncSizes& z, int Nnext, int scratch_cols) {
    const NormPlan n = plan_norm(z, Nnext, scratch_cols);
    other(n.group);
    if (n.mean) other(n.mean);
    return n.fold;
  }
  int encode(const EncSizes& z) {
    const CallPlan c = plan_call(z);
    if (!c.ok) { out += "REFUSED\n"; return -1; }
    const int E = z.E, F = z.F;
    if (c.cnt_bytes) {
      out += "MEMSET " + std::to_string(c.cnt_bytes) + "\nMEMSET " + std::to_string(c.part_bytes) + "\n";
      n += 2;
    }
    other(c.im2col);
    GemmPlan g = plan_gemm(z, EPI_PATCH, E, c.Kp, 0, z.layers > 0, false);
    gemm(g);
    bool ln_fused = g.ln_fused;
    for (int l = 0; l < z.layers; ++l) {
      bool fold = !ln_fused && norm(z, 3 * E, F);
      gemm(plan_gemm(z, EPI_QKV, 3 * E, E, 2, false, fold));
      if (c.attention.kernel < 0 || c.attention.kernel >= NUM_ATTN_KERNELS) ++bad;
      line(c.attention, attn_name[c.attention.kernel]);
      g = plan_gemm(z, EPI_RES, E, E, 4, true, false);
      gemm(g);
      fold = !g.ln_fused && norm(z, F, 3 * E);
      g = plan_gemm(z, EPI_GELU, F, E, 5, false, fold);
      gemm(g);
      if (!g.aligned && c.colmean) other(c.colmean);
      g = plan_gemm(z, EPI_RES, E, F, 6, l + 1 < z.layers, false);
      gemm(g);
      ln_fused = g.ln_fused;
    }
    other(c.final_norm);
    return n;
  }
};
static int launches(const EncSizes& z) { Walk w; const int n = w.encode(z); return w.bad ? -2 : n; }

struct Geo { const char* name; int image, patch, E, F, H; };
static const Geo README = {"readme", 224, 14, 768, 3072, 12}, DINOV2S = {"dinov2s", 224, 14, 384, 1536, 6};
static EncSizes sizes(const Geo& g, int B, int layers, int ncu = 256, bool comp = true, bool ln_ws = true) {
  const int grid = g.image / g.patch, P = grid * grid;
  return EncSizes{B, P, P + 1, g.E, g.F, g.H, g.patch, layers, ncu, 2, comp, ln_ws, false};
}

// gemm256p_kernel's tile_origin_x restated: with the plan's five lnx_* numbers, the ncu workgroups of a persistent fused-LayerNorm
// launch cover every tile once in nbm * nbn / ncu rounds, and the nbn column tiles of an image either run in ONE round (on nbn
// workgroups of one XCD label) or one after the other on one workgroup (all but the last `later`)
static bool lnx_covers(const GemmPlan& p, int ncu) {
  const int nbm = p.nbm, nbn = p.nbn, R = nbm * nbn / ncu;
  if (nbm * nbn % ncu || ncu % 8) return false;
  std::vector<int> round_of(nbm * nbn, -1), wg_of(nbm * nbn, -1);
  for (int b = 0; b < ncu; ++b)
    for (int rnd = 0; rnd < R; ++rnd) {
      const int xcd = b & 7, w = b >> 3, wq = (w * p.lnx_rcp) >> 16, rq = (rnd * p.lnx_rcp) >> 16;
      int row, col;
      if (wq < p.lnx_G) { row = rnd * p.lnx_G + wq; col = w - wq * nbn; }
      else { row = p.lnx_rows_aligned + (w - p.lnx_G * nbn) * p.lnx_rounds_div + rq; col = rnd - rq * nbn; }
      const int tm = xcd * p.lnx_rows_xcd + row;
      if (tm < 0 || tm >= nbm || col < 0 || col >= nbn || round_of[tm * nbn + col] >= 0) return false;
      round_of[tm * nbn + col] = rnd;
      wg_of[tm * nbn + col] = b;
    }
  for (int tm = 0; tm < nbm; ++tm) {
    bool one_round = true, one_wg = true;
    for (int c = 0; c < nbn; ++c) {
      if (round_of[tm * nbn + c] < 0) return false;
      one_round &= round_of[tm * nbn + c] == round_of[tm * nbn] && (wg_of[tm * nbn + c] & 7) == (wg_of[tm * nbn] & 7);
      one_wg &= wg_of[tm * nbn + c] == wg_of[tm * nbn] && round_of[tm * nbn + c] == round_of[tm * nbn] + c;
    }
    if (!one_round && !one_wg) return false;
  }
  return true;
}

// ---- the encoder workspace (WorkspacePlan): what run_encoder touches in buffer `buf` for nb images, in bytes from the slice's start
static size_t ws_touched(const Geo& g, int buf, int nb) {
  const EncSizes z = sizes(g, nb, 2);
  const CallPlan c = plan_call(z);
  const size_t n = (size_t)nb, S = (size_t)z.S, E = (size_t)z.E, F = (size_t)z.F, im2col = (size_t)z.P * c.Kp;
  switch (buf) {
    case WS_X: return n * S * E * 4;
    case WS_H: return n * S * E * 2;
    case WS_QKV: return n * S * 3 * E * 2;
    case WS_G: return n * (im2col > S * F ? im2col : S * F) * 2;        // P * Kp im2col elements, then S * F hidden elements
    case WS_CORR: return n * 2 * (3 * E > F ? 3 * E : F) * 4;
    case WS_ABAR: return n * 2 * (E > F ? E : F) * 2;
    case WS_LN_CNT: return c.cnt_bytes > lnx_cnt_bytes(nb) ? c.cnt_bytes : lnx_cnt_bytes(nb);   // (cleared at B >= 8 only: held at every nb)
    default: return c.part_bytes > lnx_part_bytes(nb, z.E) ? c.part_bytes : lnx_part_bytes(nb, z.E);
  }
}
// the halves [0, b0) and [b0, B) of a step in a context of w.max_batch >= B episodes: every slice starts on 16 bytes, the first ends
// before the second begins, the second inside the allocation.  Returns the first buffer that fails, -1 when all hold.
static int ws_halves_fail(const WorkspacePlan& w, const Geo& g, int B, int b0) {
  for (int buf = 0; buf < NUM_WS; ++buf) {
    if (w.offset(buf, 0) != 0 || w.offset(buf, b0) % 16 != 0) return buf;
    if (b0 > 0 && ws_touched(g, buf, b0) > w.offset(buf, b0)) return buf;
    if (B > b0 && w.offset(buf, b0) + ws_touched(g, buf, B - b0) > w.bytes(buf)) return buf;
  }
  return -1;
}
static bool read_file(const char* path, std::string& into) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  char buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) into.append(buf, k);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  // xcd_run: a bijection of [0, nwg) for every grid size, XCD x (= block id % 8) owning ONE contiguous run of tile indices
  for (int nwg = 1; nwg <= 4100; ++nwg) {
    std::vector<int> seen(nwg, 0), lo(8, nwg), hi(8, -1), cnt(8, 0);
    for (int b = 0; b < nwg; ++b) {
      const int t = xcd_run(b, nwg);
      REQUIRE(t >= 0 && t < nwg, "nwg %d: block %d -> tile %d", nwg, b, t);
      ++seen[t];
      const int x = b % 8;
      if (t < lo[x]) lo[x] = t;
      if (t > hi[x]) hi[x] = t;
      ++cnt[x];
    }
    for (int t = 0; t < nwg; ++t) REQUIRE(seen[t] == 1, "nwg %d: tile %d taken %d times", nwg, t, seen[t]);
    for (int x = 0; x < 8; ++x)
      if (cnt[x]) REQUIRE(hi[x] - lo[x] + 1 == cnt[x], "nwg %d: XCD %d owns %d tiles spread over [%d, %d]", nwg, x, cnt[x], lo[x], hi[x]);
  }
  // the small-row launch at B = 256 (RT = 4 CLS + 8 mean-row tiles per column tile): a 64-column slice of W or dW is read by
  // the row tiles of one problem of one column tile -- on at most two XCDs (one where the runs are whole columns: fc1, out / fc2)
  const int RT = 12, ncols[3] = {36, 48, 12};
  for (int nc : ncols) {
    const int nwg = RT * nc;
    std::vector<unsigned> xcds(2 * nc, 0);
    for (int b = 0; b < nwg; ++b) {
      const int t = xcd_run(b, nwg), bn = t / RT, bm = t % RT;
      xcds[2 * bn + (bm >= 4)] |= 1u << (b % 8);
    }
    int worst = 0;
    for (unsigned m : xcds) { const int c = __builtin_popcount(m); if (c > worst) worst = c; }
    REQUIRE(worst <= 2, "%d column tiles: a slice is read on %d XCDs", nc, worst);
    if ((nwg / 8) % RT == 0) REQUIRE(worst == 1, "%d column tiles: whole columns per XCD, yet a slice is on %d XCDs", nc, worst);
  }
  // non-temporal 16-bit outputs: 32-bit BYTE offsets.  fc1 at S = 257, F = 3072, 2-byte elements
  const size_t S = 257, F = 3072;
  REQUIRE(big_output(256 * S, F, 2) && nt16_addressable(256 * S, F, 2), "B = 256 takes the non-temporal form");
  REQUIRE(!big_output(16 * S, F, 2), "B = 16 does not (25 MB)");
  REQUIRE(nt16_addressable(2720 * S, F, 2), "B = 2720: %zu bytes", 2720 * S * F * 2);
  REQUIRE(!nt16_addressable(2721 * S, F, 2), "B = 2721: %zu bytes wrap a 32-bit byte offset", 2721 * S * F * 2);
  REQUIRE(!nt16_addressable((size_t)1 << 16, (size_t)1 << 15, 2), "exactly 4 GiB");
  REQUIRE(nt16_addressable(((size_t)1 << 16) - 1, (size_t)1 << 15, 2), "one row below 4 GiB");
  // ---- the launch counts the committed profiles pin (README geometry, 12 layers, compensation on, 256 CUs; the recorded totals
  // are one higher: the policy's launch)
  REQUIRE(launches(sizes(README, 1, 12)) == 99, "B = 1: %d launches (profiles/r6_bench_b1.json: 100 per step)", launches(sizes(README, 1, 12)));
  REQUIRE(launches(sizes(README, 4, 12)) == 123, "B = 4: %d launches (r6_bench_b4.json: 124)", launches(sizes(README, 4, 12)));
  for (int B : {8, 256, 1024}) REQUIRE(launches(sizes(README, B, 12)) == 113, "B = %d: %d launches (r6_bench_b256.json, r6_bench_b1024.json: 114)", B, launches(sizes(README, B, 12)));
  REQUIRE(launches(sizes(DINOV2S, 256, 12)) == 113, "DINOv2-small, B = 256: %d launches (r6_bench_b256_dinov2_small.json: 114)", launches(sizes(DINOV2S, 256, 12)));
  // ---- form boundaries
  const int E = README.E, Fm = README.F;
  {
    const GemmPlan lo = plan_gemm(sizes(README, 7, 12), EPI_QKV, 3 * E, E, 2, false, false), hi = plan_gemm(sizes(README, 8, 12), EPI_QKV, 3 * E, E, 2, false, false);
    REQUIRE(!lo.aligned && lo.fused_bias && lo.main.kernel == G64C_QKV && !lo.small, "2047 rows: 64 x 64 tiles, bias rows inside");
    REQUIRE(hi.aligned && !hi.fused_bias && hi.main.kernel == G256_QKV && hi.small.kernel == G64_QKV && hi.nbm == 8 && hi.tile_row0 == 1 && hi.tile_stride == 257,
            "2048 rows: image-aligned tiles behind the CLS / mean-row launch");
    REQUIRE(plan_norm(sizes(README, 1, 12), 3 * E, Fm).fold && plan_gemm(sizes(README, 1, 12), EPI_QKV, 3 * E, E, 2, false, true).main.kernel == G64CF_QKV, "B = 1: QKV folds the LayerNorm's partials");
    const NormPlan n2 = plan_norm(sizes(README, 2, 12), 3 * E, Fm);
    REQUIRE(n2.partial && !n2.fold && n2.mean.kernel == LN_MEAN, "B = 2: QKV is more than one round, the mean rows get their launch");
  }
  const int ncus[4] = {256, 304, 64, 250};
  for (int ncu : ncus)
    for (int B = 1; B <= 7; ++B) {
      const GemmPlan p = plan_gemm(sizes(README, B, 12, ncu), EPI_RES, E, E, 4, true, false);
      const int nb64 = (B * 257 + 63) / 64 * (E / 64);
      REQUIRE((p.main.kernel == G64C32) == (2 * nb64 <= ncu) && (int)p.main.grid == (2 * nb64 <= ncu ? 2 * nb64 : nb64), "B = %d, %d CUs: 64 x 32 tiles exactly below half of the chip", B, ncu);
    }
  for (int ncu : ncus) {
    int persistent = 0;
    for (int B = 8; B <= 2432; ++B) {
      const GemmPlan p = plan_gemm(sizes(README, B, 12, ncu), EPI_RES, E, E, 4, true, false);
      REQUIRE(p.ln_fused && p.nbn == 3 && p.nbm == B, "B = %d: the out-projection runs norm2 in its epilogue", B);
      if (p.main.kernel == G256LN_RES_P || p.main.kernel == G256LNNT_RES_P) {
        ++persistent;
        REQUIRE((int)p.main.grid == ncu && lnx_covers(p, ncu), "B = %d, %d CUs: persistent, yet an image's column tiles do not share a round", B, ncu);
      } else {
        REQUIRE((int)p.main.grid == B * 3 && p.lnx_G == 0, "B = %d, %d CUs: one workgroup per tile", B, ncu);
      }
    }
    // (three column tiles, 32 / 38 / 8 workgroups per XCD label: two left over, so the rounds must be a multiple of three)
    REQUIRE(persistent == (ncu % 8 ? 0 : 2432 / ncu), "%d CUs: %d persistent batches", ncu, persistent);
  }
  {
    const GemmPlan p = plan_gemm(sizes(README, 1024, 12), EPI_RES, E, E, 4, true, false);   // 3072 tiles on 256 CUs: 12 rounds
    REQUIRE(p.main.kernel == G256LNNT_RES_P && p.lnx_G == 10 && p.lnx_rows_aligned == 120 && p.lnx_rounds_div == 4 && p.lnx_rows_xcd == 128 && p.lnx_rcp == 21846, "B = 1024: lnx numbers");
    REQUIRE(p.lnx_rows_aligned + (256 / 8 - p.lnx_G * 3) * p.lnx_rounds_div == p.lnx_rows_xcd, "B = 1024: the groups' and the left-over workgroups' images add up");
  }
  // tests/test_gpu_geometry_contract.py runs the persistent fused LayerNorm once per column-tile count: on 256 CUs these three
  // (width, batch) pairs take it in the patch embedding and in both residual GEMMs, and the same widths at B = 9 do not
  for (const Geo& g : {Geo{"e1024", 224, 14, 1024, 2048, 16}, Geo{"e512", 224, 14, 512, 1024, 8}, Geo{"e256", 224, 14, 256, 512, 4}}) {
    const int nbn = g.E / 256, B = 256 / nbn;
    const EncSizes z = sizes(g, B, 1), nine = sizes(g, 9, 1);
    const GemmPlan pe = plan_gemm(z, EPI_PATCH, g.E, plan_call(z).Kp, 0, true, false), out = plan_gemm(z, EPI_RES, g.E, g.E, 4, true, false),
                   fc2 = plan_gemm(z, EPI_RES, g.E, g.F, 6, true, false);
    REQUIRE(pe.main.kernel == G256LN_PATCH_P && out.main.kernel == G256LN_RES_P && fc2.main.kernel == G256LN_RES_P, "E = %d, B = %d: persistent fused LayerNorm", g.E, B);
    for (const GemmPlan* p : {&pe, &out, &fc2})
      REQUIRE(p->ln_fused && p->nbn == nbn && p->nbm == B && (int)p->main.grid == 256 && lnx_covers(*p, 256), "E = %d, B = %d: %d column tiles of an image in one round", g.E, B, nbn);
    REQUIRE(plan_gemm(nine, EPI_PATCH, g.E, plan_call(nine).Kp, 0, true, false).main.kernel == G256LN_PATCH &&
            plan_gemm(nine, EPI_RES, g.E, g.E, 4, true, false).main.kernel == G256LN_RES, "E = %d, B = 9: one workgroup per tile", g.E);
  }
  REQUIRE(plan_gemm(sizes(README, 2720, 12), EPI_GELU, Fm, E, 5, false, false).main.kernel == G256NT_GELU, "B = 2720: fc1 stores non-temporally");
  REQUIRE(plan_gemm(sizes(README, 2721, 12), EPI_GELU, Fm, E, 5, false, false).main.kernel == G256_GELU, "B = 2721: fc1's output is 4 GiB, the plain form");
  {
    int B = 1;
    while ((size_t)B * 257 * Fm < ((size_t)1 << 32)) ++B;                        // 5441
    REQUIRE(B == 5441 && plan_call(sizes(README, B - 1, 12)).ok && !plan_call(sizes(README, B, 12)).ok && launches(sizes(README, B, 12)) == -1, "refused from B = %d on", B);
  }
  // ---- the sweep: every planned LDS size within the limit, every kernel id inside its table, and the launches those of the recorded trace
  std::string want;
  if (argc > 1) REQUIRE(read_file(argv[1], want), "cannot open %s", argv[1]);
  const Geo geos[4] = {README, DINOV2S, {"mid", 112, 14, 128, 512, 2}, {"wide64", 112, 14, 768, 3072, 12}};
  const int Bs[14] = {1, 2, 4, 7, 8, 9, 64, 255, 256, 257, 1024, 2048, 2720, 2721};
  size_t at = 0;
  for (const Geo& g : geos)
    for (int B : Bs)
      for (int ncu : ncus)
        for (int comp = 1; comp >= 0; --comp)
          for (int lnws = 1; lnws >= 0; --lnws) {
            if (ncu != 256 && !(comp && lnws)) continue;       // the other CU counts with everything on only: keeps the file small
            Walk w;
            char head[96];
            snprintf(head, sizeof head, "# %s B %d ncu %d comp %d lnws %d\n", g.name, B, ncu, comp, lnws);
            w.out = head;
            const int n = w.encode(sizes(g, B, 2, ncu, comp != 0, lnws != 0));
            REQUIRE(w.bad == 0, "%s: %d launches out of range", head, w.bad);
            if (n >= 0) w.out += "= " + std::to_string(n) + "\n";
            if (argc > 1) {
              REQUIRE(want.compare(at, w.out.size(), w.out) == 0, "%sthe plan:\n%srecorded (from byte %zu):\n%s", head, w.out.c_str(), at, want.substr(at, w.out.size()).c_str());
              at += w.out.size();
            }
          }
  REQUIRE(argc > 1 && at == want.size() && at > 0, "usage: plan_check encoder_plan_trace.txt (%zu of %zu bytes matched)", at, want.size());
  // ---- the encoder workspace: sizes and slice offsets are those recorded from the expressions WorkspacePlan replaced (argv[2]: the
  // allocations of hvla_create, the slices of encode_range), and over the same sweep the halves of a two-stream step are disjoint,
  // aligned and inside the allocation for everything run_encoder touches
  std::string ws_want, ws_got;
  REQUIRE(argc > 2 && read_file(argv[2], ws_want), "usage: plan_check encoder_plan_trace.txt encoder_workspace_trace.txt");
  const Geo ws_geos[5] = {{"tiny", 56, 14, 32, 64, 2}, geos[2], README, DINOV2S, {"e1024", 224, 14, 1024, 4096, 16}};
  const int max_batches[9] = {1, 2, 5, 63, 64, 65, 96, 256, 1024};
  for (const Geo& g : ws_geos)
    for (int max_batch : max_batches) {
      const EncSizes z = sizes(g, 1, 2);
      const int Kp = plan_call(z).Kp;
      const WorkspacePlan w(z.P, z.S, z.E, z.F, Kp, max_batch);
      char line[256];
      int k = snprintf(line, sizeof line, "# %s max_batch %d\nalloc", g.name, max_batch);
      for (int buf = 0; buf < NUM_WS; ++buf) k += snprintf(line + k, sizeof line - k, " %zu", w.bytes(buf));
      ws_got += line;
      ws_got += '\n';
      const int Bs2[7] = {0, 64, 65, 66, 67, 96, max_batch};
      for (int i = 0; i < 7; ++i) {
        const int B = Bs2[i], b0 = B / 2;
        if (B > max_batch || (i == 6 && (B == 96 || (B >= 64 && B <= 67)))) continue;
        k = snprintf(line, sizeof line, "B %d b0 %d:", B, b0);
        for (int buf = 0; buf < NUM_WS; ++buf) k += snprintf(line + k, sizeof line - k, " %zu", w.offset(buf, b0));
        ws_got += line;
        ws_got += '\n';
        const int fail = ws_halves_fail(w, g, B, b0);
        REQUIRE(fail < 0, "%s, max_batch %d, halves [0, %d) and [%d, %d): buffer %d", g.name, max_batch, b0, b0, B, fail);
        // the whole context as one call, too
        REQUIRE(ws_halves_fail(w, g, max_batch, 0) < 0, "%s: %d episodes do not fit their own allocation", g.name, max_batch);
        // the slices of g were once cut by S * F alone: at MID (P * Kp = 81920 > S * F = 33280) the first half's im2col rows then
        // ran into the second half's (tests/test_gpu_parity.py::test_two_stream_step_with_a_narrow_mlp) -- this check refuses that cut
        if (!strcmp(g.name, "mid") && b0 > 0) {
          WorkspacePlan narrow = w;
          narrow.per[WS_G] = (size_t)z.S * z.F * 2;
          REQUIRE(ws_halves_fail(narrow, g, B, b0) == WS_G, "mid, halves at %d: g cut by S * F alone passes", b0);
        }
      }
    }
  REQUIRE(ws_got == ws_want, "the workspace table (%zu bytes) is not the recorded one (%zu bytes):\n%s", ws_got.size(), ws_want.size(), ws_got.c_str());
  printf("OK\n");
  return 0;
}
