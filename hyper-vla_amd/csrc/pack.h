// pack.h — the element formulas of the serving buffers and the host packing of W_cat and the encoder matrices (no HIP types: the
// programs of tests/native/ run it under -fsanitize=address,undefined on the CPU).  Every formula exists once: the host packer
// (serving_layout.h) and publish.hip run this text.  HVLA_PACK_HD is `__host__ __device__` under hipcc, empty for a host compiler.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "layout.h"

#if defined(__HIPCC__)
#define HVLA_PACK_HD __host__ __device__
#else
#define HVLA_PACK_HD
#endif

namespace hvla {
namespace pack {

HVLA_PACK_HD inline uint16_t f2bf(float f) {          // round-to-nearest-even, NaN preserved
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
HVLA_PACK_HD inline float bf2f(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// IEEE binary16, round-to-nearest-even, subnormals kept, overflow to infinity (== the hardware conversion)
HVLA_PACK_HD inline uint16_t f2h(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (u > 0x7f800000u ? 0x200u : 0u));   // inf / NaN
  if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                       // rounds to >= 65520: inf
  if (u < 0x38800000u) {                                                                         // below 2^-14: subnormal
    if (u < 0x33000000u) return (uint16_t)sign;                                                  // below 2^-25: zero
    const int shift = 126 - (int)(u >> 23);                          // 14 .. 24
    const uint32_t mant = (u & 0x7fffffu) | 0x800000u;
    const uint32_t q = mant >> shift, rem = mant & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    return (uint16_t)(sign | (q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u)));
  }
  const uint32_t v = u - 0x38000000u;                                // rebias 127 -> 15
  return (uint16_t)(sign | ((v + 0xfffu + ((v >> 13) & 1u)) >> 13));
}
HVLA_PACK_HD inline float h2f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  uint32_t u;
  if (e == 0) {
    if (m == 0) u = sign;
    else {
      int s = 0;
      uint32_t mm = m;
      while (!(mm & 0x400u)) mm <<= 1, ++s;
      u = sign | ((uint32_t)(113 - s) << 23) | ((mm & 0x3ffu) << 13);
    }
  } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
  else u = sign | ((e + 112u) << 23) | (m << 13);
  float f;
  memcpy(&f, &u, 4);
  return f;
}
HVLA_PACK_HD inline uint16_t to16(float f, bool bf) { return bf ? f2bf(f) : f2h(f); }
HVLA_PACK_HD inline float from16(uint16_t h, bool bf) { return bf ? bf2f(h) : h2f(h); }

// one element of a transposing pack: the 16-bit weight and what the rounding dropped, x 4096 (stays in the normal range of fp16)
HVLA_PACK_HD inline void round_pair(float w, bool bf, uint16_t& w16, uint16_t& d16) {
  w16 = to16(w, bf);
  d16 = to16((w - from16(w16, bf)) * 4096.f, bf);
}
// one element of W_cat: hi = bf16(w), lo = bf16(w - hi)
HVLA_PACK_HD inline void split_pair(float w, uint16_t& hi, uint16_t& lo) {
  hi = f2bf(w);
  lo = f2bf(w - bf2f(hi));
}
// fragment lane rho (+ 32 for the upper eight k of a k-step) holds column tau of its 32-column tile, and the inverse
HVLA_PACK_HD inline int tau_of_rho(int rho) { return 16 * ((rho >> 2) & 1) + (rho & 3) + 4 * (rho >> 3); }
HVLA_PACK_HD inline int rho_of_tau(int tau) { return (tau & 3) + 4 * (tau >> 4) + 8 * ((tau >> 2) & 3); }

// output channel nn of the patch embedding: row nn of [E][hi Kp/2 | lo Kp/2] and its bias.  `pk` [Kreal][E].
// ((p/255 - mean)/std) . w  ==  (p - 128) . w' / 256 + const with w' = 256 w / (255 std): x256 keeps small weights in the 16-bit
// normal range.  The rescale is done in double and rounded to f32 once; the bias is accumulated in double, ascending k.
HVLA_PACK_HD inline float patch_channel(const float* pk, float pb, int E, int nn, int Kreal, int Kp, bool bf, uint16_t* row) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  // (selected, not indexed: a table indexed by k % 3 would sit in the kernel's private segment)
  const int Kp1 = Kp / 2;
  double bacc = pb;
  for (int k = 0; k < Kp1; ++k) {
    uint16_t hi = 0, lo = 0;
    if (k < Kreal) {
      const int c = k % 3;
      const double mean = c == 0 ? 0.485 : c == 1 ? 0.456 : 0.406, sd = c == 0 ? 0.229 : c == 1 ? 0.224 : 0.225;
      const double wk = pk[(size_t)k * E + nn];
      const float w = (float)(wk * 256.0 / (255.0 * sd));
      hi = to16(w, bf);
      lo = to16(w - from16(hi, bf), bf);
      bacc += wk * (128.0 / 255.0 - mean) / sd;
    }
    row[k] = hi;
    row[Kp1 + k] = lo;
  }
  return (float)bacc;
}

// W_cat^T as MFMA A fragments (layout.h): tile pt, k-step ks, lane (rho = l & 31, hk = l >> 5), j; hi / lo bf16 planes, and
// b_cat in packed order.  lk[i] / lb[i]: kernel [C][size_i] / bias [size_i] of generated leaf i.
inline void pack_wcat(const PackedLayout& lay, const std::vector<LeafInfo>& leaves, const std::vector<const float*>& lk,
                      const std::vector<const float*>& lb, int C, std::vector<uint16_t>& hi, std::vector<uint16_t>& lo,
                      std::vector<float>& bc) {
  const PolicyLayout& pl = lay.pl;
  const int Gtot = pl.Gm + pl.Gv, ntiles = Gtot / 32, KS = C / 16;
  std::vector<int32_t> leaf_of(pl.G);
  for (size_t i = 0; i < leaves.size(); ++i)
    for (int64_t j = 0; j < leaves[i].size; ++j) leaf_of[leaves[i].offset + j] = (int32_t)i;
  hi.assign((size_t)ntiles * KS * 512, 0);
  lo.assign(hi.size(), 0);
  bc.assign(Gtot, 0.f);
  const int32_t* perm = lay.perm.data();
  for (int pos = 0; pos < Gtot; ++pos)
    if (perm[pos] >= 0) {
      const int ref = perm[pos], li = leaf_of[ref];
      bc[pos] = lb[li][ref - leaves[li].offset];
    }
  for (int pt = 0; pt < ntiles; ++pt)
    for (int lane = 0; lane < 64; ++lane) {
      const int rho = lane & 31, hk = lane >> 5;
      const int ref = perm[pt * 32 + tau_of_rho(rho)];
      const float* col = nullptr;
      int64_t n_leaf = 0;
      if (ref >= 0) {
        const int li = leaf_of[ref];
        col = lk[li] + (ref - leaves[li].offset);
        n_leaf = leaves[li].size;
      }
      for (int ks = 0; ks < KS; ++ks)
        for (int j = 0; j < 8; ++j) {
          const int k = 16 * ks + 8 * hk + j;
          const size_t o = ((size_t)(pt * KS + ks) * 64 + lane) * 8 + j;
          split_pair(col ? col[(int64_t)k * n_leaf] : 0.f, hi[o], lo[o]);
        }
    }
}

// share_layer_index=False: the A row of a packed position is the context row of its leaf's layer token (layout.h layer_token_of).
// The arena order is the policy kernel's, so a 32-position tile may hold positions of several tokens -- the vector region packs
// encoder_norm, the per-layer vectors, the head bias and the position table side by side.  A tile is therefore cut into SEGMENTS, one
// per distinct token among its positions, in order of first appearance; a padding position (perm -1) has no token and a tile of
// padding alone no segment.  Each segment has its own W_cat^T fragment block (hi and lo, [KS][64 lanes][8] as pack_wcat's) in which
// the rows of positions of another token, or of padding, are zero: summed over a tile's segments, every position meets its own
// column exactly once and exact zeros otherwise (hypernet.hip weightgen_tokens_body).
struct TokenSegments {
  std::vector<int32_t> token;         // [nseg] the layer token of segment s
  std::vector<int32_t> tile;          // [nseg] its tile
  std::vector<int32_t> tile_segs;     // [ntiles][2]: first segment, count
  std::vector<int32_t> pos_token;     // [Gm + Gv] the token of every position, -1 for padding
};
inline TokenSegments build_segments(const Geom& g, const PackedLayout& lay, const std::vector<LeafInfo>& leaves) {
  const PolicyLayout& pl = lay.pl;
  const int Gtot = pl.Gm + pl.Gv, ntiles = Gtot / 32;
  std::vector<int32_t> tok_of_ref(pl.G, -1);
  for (const LeafInfo& l : leaves) {
    const int t = layer_token_of(g, l.flat);
    for (int64_t j = 0; j < l.size; ++j) tok_of_ref[l.offset + j] = t;
  }
  TokenSegments s;
  s.pos_token.assign(Gtot, -1);
  s.tile_segs.assign((size_t)ntiles * 2, 0);
  for (int pos = 0; pos < Gtot; ++pos)
    if (lay.perm[pos] >= 0) s.pos_token[pos] = tok_of_ref[lay.perm[pos]];
  for (int pt = 0; pt < ntiles; ++pt) {
    const int first = (int)s.token.size();
    for (int i = 0; i < 32; ++i) {
      const int t = s.pos_token[pt * 32 + i];
      bool seen = t < 0;
      for (int q = first; q < (int)s.token.size() && !seen; ++q) seen = s.token[q] == t;
      if (!seen) { s.token.push_back(t); s.tile.push_back(pt); }
    }
    s.tile_segs[2 * pt] = first;
    s.tile_segs[2 * pt + 1] = (int)s.token.size() - first;
  }
  return s;
}
// the segments' fragment blocks from pack_wcat's planes: block s is tile s.tile[s] with the lanes of other tokens' positions zeroed
inline void pack_segments(const TokenSegments& s, int C, const std::vector<uint16_t>& hi, const std::vector<uint16_t>& lo,
                          std::vector<uint16_t>& shi, std::vector<uint16_t>& slo) {
  const int KS = C / 16;
  shi.assign(s.token.size() * KS * 512, 0);
  slo.assign(shi.size(), 0);
  for (size_t q = 0; q < s.token.size(); ++q)
    for (int lane = 0; lane < 64; ++lane) {
      if (s.pos_token[s.tile[q] * 32 + tau_of_rho(lane & 31)] != s.token[q]) continue;
      for (int ks = 0; ks < KS; ++ks) {
        const size_t src = ((size_t)(s.tile[q] * KS + ks) * 64 + lane) * 8, dst = ((q * KS + ks) * 64 + lane) * 8;
        memcpy(&shi[dst], &hi[src], 16);
        memcpy(&slo[dst], &lo[src], 16);
      }
    }
}

// flax [K][N] -> [N][K] 16-bit, and the rounding residues for the per-image compensation of the encoder GEMMs (encoder.hip
// corr_kernel)
inline void pack_matrix_t(const float* src, int K, int N, bool bf, uint16_t* w16, uint16_t* d16) {
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) round_pair(src[(size_t)k * N + n], bf, w16[(size_t)n * K + k], d16[(size_t)n * K + k]);
}

}  // namespace pack
}  // namespace hvla
