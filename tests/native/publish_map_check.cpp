// CPU-only check of the index maps of hvla_train_publish (csrc/publish_map.h) under AddressSanitizer and UndefinedBehaviorSanitizer.
// Built and run by tests/test_publish_host.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wextra -Werror -I hyper-vla_amd/csrc ...
// At MID and README geometry a flat training vector of distinct values goes two ways:
//   reference: the leaves cut out of the vector (what unpack_params does), through pack::pack_wcat, pack::pack_matrix_t and a
//              transcription of the order in which hvla_load_weights lays out the context encoder and the image encoder;
//   emulation: what the publish kernels do -- the tables of publish_map.h and its element formulas, applied element by element
//              with a counter per destination.
// Every buffer must agree byte for byte and every destination element must be written exactly once.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "publish_map.h"

using namespace hvla;
using namespace hvla::pubmap;

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

static int check(const Geom& g, const char* name, bool bf) {
  const TrainLayout L = make_train_layout(g);
  const size_t n = (size_t)(L.total + L.enc_total);
  std::vector<float> v(n);                           // exact size: an index past the vector is an ASAN report
  for (size_t i = 0; i < n; ++i) v[i] = value(i);
  const float* P = v.data();
  const int C = g.C, F = g.ctx_mlp, E = g.E, Fe = g.enc_mlp, S = g.S(), T = g.T;

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
      const TrainLayout::CL& c = L.layer[l];
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
      const TrainLayout::EL& s = L.enc[i];
      mark16((size_t)3 * E * E);
      tr(s.qk, E, E, cur16); tr(s.kk, E, E, cur16 + (size_t)E * E); tr(s.vk, E, E, cur16 + (size_t)2 * E * E);
      mark16((size_t)E * E); tr(s.ok, E, E, cur16);
      mark16((size_t)E * Fe); tr(s.f1k, E, Fe, cur16);
      mark16((size_t)Fe * E); tr(s.f2k, Fe, E, cur16);
      markf(3 * E);
      memcpy(&wf[curf], X + s.qb, E * 4); memcpy(&wf[curf + E], X + s.kb, E * 4); memcpy(&wf[curf + 2 * E], X + s.vb, E * 4);
      markf(E); memcpy(&wf[curf], X + s.ob, E * 4);
      markf(Fe); memcpy(&wf[curf], X + s.f1b, Fe * 4);
      markf(E); memcpy(&wf[curf], X + s.f2b, E * 4);
      const long six[6] = {s.n1s, s.n1b, s.n2s, s.n2b, s.ls1, s.ls2};
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
  printf("OK\n");
  return 0;
}
