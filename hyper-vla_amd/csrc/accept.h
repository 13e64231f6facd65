// accept.h -- which geometries hvla_create serves (no HIP types): ONE predicate from (hvla_config, use_language_token) to
// HVLA_OK / HVLA_E_SHAPE / HVLA_E_DTYPE, and next to it the two dynamic-LDS descriptions it refuses by.  The launchers
// (launch_ctx_encoder in hypernet.hip, launch_policy_nw in policy.hip) size their launches with the same functions, so a geometry
// the predicate lets through cannot fail its first launch for LDS.  A CPU test walks the predicate over every edge of the contract
// and checks the launch-side preconditions of everything it accepts (tests/native/accept_check.cpp, built with g++ under ASan /
// UBSan by tests/test_host_sanitizers.py).
//
// What the hand-written kernels are specialised for (anything else is refused, never emulated):
//   policy     dim == 64, heads == 4, mlp % 32 == 0, mlp >= 32, layers >= 1, 1 <= horizon, 2 <= action_dim,
//              horizon * action_dim <= 32 (one 32-row head tile), and the per-layer vectors fit the policy kernel's LDS
//              (policy_lds_bytes <= 160 KiB: at P = 256 layers <= 7 at mlp = 128, mlp <= 768 at layers = 4)
//   encoder    enc_dim % 128 == 0, 128 <= enc_dim <= 1024, enc_mlp % 128 == 0, enc_mlp >= 128, head width 64,
//              0 <= enc_layers <= ENC_MAX_LAYERS, image_size % patch == 0, P = (image_size / patch)^2 in {256, 64}
//   context    ctx_dim in {128, 64, 32}, ctx_dim % ctx_heads == 0 with a head width that is a multiple of 4 (the score loop's
//              k-steps of the f32 MFMA), ctx_mlp % 16 == 0, 0 <= ctx_layers <= CTX_MAX_LAYERS, 2 <= lang_tokens <= 38,
//              lang_dim % 4 == 0, and the working set fits the context encoder's LDS (ctx_encoder_lds_bytes <= 160 KiB)
//   use_language_token   additionally lang_tokens <= 32 (one 32-key tile) and lang_dim % 64 == 0
//   share_layer_index=False   lang_tokens + 1 + NL <= 48 rows (NL = layers + 5, + 1 with use_language_token), the LDS formula with that many
//   use_differential_transformer   not with use_language_token; the per-layer vectors are 48 floats longer and the policy kernel keeps
//              a second table of action-row partials, both inside the same 160 KiB
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hvla.h"
#include "layout.h"
#include "plan.h"

namespace hvla {

// (CTX_MAX_LAYERS, ENC_MAX_LAYERS: layout.h)
// Two kernel constants the LDS formulas below depend on.  They are DEFINED here so that the formulas stand in a header without HIP
// types; what each is for is told where it is used (hypernet.hip, policy.hip).
constexpr int CTX_THREADS = 1024;     // ctx_encoder_kernel's workgroup: 16 waves
constexpr int PRING = 4;              // policy_kernel's ring of staged weight tiles, 8 KiB each

// ---- context encoder: floats of its third LDS buffer (q | k | v or the MLP hidden rows; the staged token chunk; the CLS row and
// the partial sums of its projection), and the dynamic LDS of ctx_encoder_kernel for T task tokens, width C, MLP width F, image width E
// (extra_rows: the layer tokens beyond the first, NL - 1 under share_layer_index=False)
inline size_t ctx_big_elems(int T, int C, int F, int E, int extra_rows = 0) {
  const int S = T + 2 + extra_rows;
  const int ldq = 3 * C + 4, ldf = F + 4;
  int bigld = ldq > ldf ? ldq : ldf;
  if (bigld < 132) bigld = 132;
  size_t big_elems = (size_t)S * bigld;
  if (big_elems < (size_t)E + CTX_THREADS) big_elems = (size_t)E + CTX_THREADS;
  return big_elems;
}
inline size_t ctx_encoder_lds_bytes(int T, int C, int F, int E, int extra_rows = 0) {
  return ((size_t)2 * (T + 2 + extra_rows) * (C + 4) + ctx_big_elems(T, C, F, E, extra_rows) + 64) * sizeof(float);   // x, h, big, the key mask
}
constexpr int CTX_MAX_ROWS = 48;      // three 16-row MFMA tiles: the context kernels' sequence limit

// ---- generated policy: the dynamic LDS of policy_kernel<NW> (NW = P / 32 waves) and of its language-token form, THE description:
// policy_lds_bytes takes its total from it and the kernel body (policy_body.inc) is held to it by static_asserts.  What each buffer
// holds is told where the kernel uses it.  Byte offsets from the start of the dynamic LDS, in the order of the buffers.
struct PolicyLds {
  int nhr;          // heads resident in K / V^T at a time
  int np;           // rows of the action row's partial table per head: <= 8 waves (+ the language prefix) + the own key
  int spx;          // keys of the attention-map export: the patches (+ the prefix tile)
  int act_floats;   // the action token's scratch: xa .. ga [384] | part [2][np][20] (differential: [2][2][np][20], one table per softmax) | pbuf [NW][32] | pexp [2][spx] | qkv1 [96] | hpriv [NW][64]
  int act_bytes;    // ... rounded up to 1 KiB; the scratch sits at offset 0
  int ring;         // [PRING][8 KiB] staged weight tiles
  int kh, kl;       // [nhr][P / 32][2][32][8] bf16 each
  int vt;           // [nhr][hi d 0-15 | lo d 0-15][P + 8] fp16
  int pre;          // [LANG_PAIR_BYTES] the resident head pair's language prefix (lang only: else empty)
  int park;         // [NW][4 KiB] phase A's attention outputs
  int vlds;         // [layer_vec_floats] f32, to the end
};
constexpr PolicyLds policy_lds(int NW, bool lang, bool diff = false) {
  const int SP = NW * 32, VLD = SP + 8;
  PolicyLds d{};
  d.nhr = 2;
  d.np = lang ? 10 : 9;
  d.spx = SP + (lang ? 32 : 0);
  d.act_floats = 384 + 2 * (diff ? 2 : 1) * d.np * 20 + NW * 32 + 2 * d.spx + 96 + NW * 64;
  d.act_bytes = (d.act_floats * 4 + 1023) & ~1023;
  d.ring = d.act_bytes;
  d.kh = d.ring + PRING * 8192;
  d.kl = d.kh + d.nhr * SP * 16 * 2;
  d.vt = d.kl + d.nhr * SP * 16 * 2;
  d.pre = d.vt + d.nhr * 32 * VLD * 2;
  d.park = d.pre + (lang ? LANG_PAIR_BYTES : 0);
  d.vlds = d.park + NW * 4096;
  return d;
}
// layer_vec_floats = PolicyLayout::Gv - v_layer0, the per-layer vectors + encoder_norm + head bias the kernel copies to LDS once.
inline size_t policy_lds_bytes(int NW, bool lang, int layer_vec_floats, bool diff = false) {
  return (size_t)policy_lds(NW, lang, diff).vlds + (size_t)layer_vec_floats * sizeof(float);
}

inline Geom geom_of(const hvla_config& c, int lang, int diff = 0) {
  Geom g = Geom{c.image_size, c.patch, c.enc_dim, c.enc_layers, c.enc_heads, c.enc_mlp,
              c.dim, c.layers, c.heads, c.mlp, c.horizon, c.action_dim, c.tanh_scale, c.max_action,
              c.ctx_dim, c.ctx_layers, c.ctx_heads, c.ctx_mlp, c.lang_tokens, c.lang_dim, c.scale_context,
              c.clip_target != 0, lang};
  g.differential = diff;
  return g;
}

// the policy kernel's LDS for an ACCEPTED width set (dim 64, mlp % 32 == 0, small layer count: the offsets are ints)
inline size_t policy_lds_bytes_of(const hvla_config& c, int lang, int diff = 0) {
  PolicyLayout pl{};
  LangLayout ll;
  policy_offsets(geom_of(c, lang, diff), pl, ll);
  const int grid = c.image_size / c.patch;
  return policy_lds_bytes(grid * grid / 32, lang != 0, pl.Gv - pl.v_layer0, diff != 0);
}

// HVLA_OK, or why hvla_create refuses the geometry.  Every divisor is checked before it divides and every product is formed in 64
// bits: the verdict arrives for ANY field values.  (struct_size and the options' struct_size are the caller's.)
// diff: use_differential_transformer (a longer per-layer vector block and a second partial table in the policy kernel's LDS); not with lang
// layer_tokens: share_layer_index=False -- NL = layers + 5 (+ 1 with lang) layer tokens; the sequence lang_tokens + 1 + NL must fit
// CTX_MAX_ROWS and the LDS working set is sized with it
inline int accept_geometry(const hvla_config& c, int lang, int diff = 0, int layer_tokens = 0) {
  if (layer_tokens != 0 && layer_tokens != 1) return HVLA_E_SHAPE;
  if (c.enc_dtype != HVLA_ENC_F16 && c.enc_dtype != HVLA_ENC_BF16) return HVLA_E_DTYPE;
  if (lang != 0 && lang != 1) return HVLA_E_SHAPE;
  if ((diff != 0 && diff != 1) || (diff && lang)) return HVLA_E_SHAPE;
  if (c.max_batch < 1 || c.streams < 0 || c.streams > 2) return HVLA_E_SHAPE;
  // generated policy
  if (c.dim != 64 || c.heads != 4 || c.mlp < 32 || c.mlp % 32 != 0 || c.layers < 1) return HVLA_E_SHAPE;
  if (c.horizon < 1 || c.action_dim < 2 || (int64_t)c.horizon * c.action_dim > 32) return HVLA_E_SHAPE;
  // image encoder
  if (c.enc_dim < 128 || c.enc_dim > 1024 || c.enc_dim % 128 != 0 || c.enc_mlp < 128 || c.enc_mlp % 128 != 0) return HVLA_E_SHAPE;
  if (c.enc_heads < 1 || c.enc_dim % c.enc_heads != 0 || c.enc_dim / c.enc_heads != 64) return HVLA_E_SHAPE;
  if (c.enc_layers < 0 || c.enc_layers > ENC_MAX_LAYERS) return HVLA_E_SHAPE;
  if (c.patch < 1 || c.image_size < 1 || c.image_size % c.patch != 0) return HVLA_E_SHAPE;
  const int64_t grid = c.image_size / c.patch, P = grid * grid;
  if (P != 256 && P != 64) return HVLA_E_SHAPE;     // (32 patches are no square: no policy_kernel<1> is built)
  // context encoder
  if (c.ctx_dim != 128 && c.ctx_dim != 64 && c.ctx_dim != 32) return HVLA_E_SHAPE;
  if (c.ctx_heads < 1 || c.ctx_dim % c.ctx_heads != 0 || (c.ctx_dim / c.ctx_heads) % 4 != 0) return HVLA_E_SHAPE;
  if (c.ctx_mlp < 16 || c.ctx_mlp % 16 != 0 || c.ctx_layers < 0 || c.ctx_layers > CTX_MAX_LAYERS) return HVLA_E_SHAPE;
  if (c.lang_tokens < 2 || c.lang_tokens > 38 || c.lang_dim < 4 || c.lang_dim % 4 != 0) return HVLA_E_SHAPE;
  // use_language_token: the language prefix is one 32-key tile of the policy kernel, its projection runs in k-steps of 64
  if (lang && (c.lang_tokens > 32 || c.lang_dim % 64 != 0)) return HVLA_E_SHAPE;
  // the context encoder keeps its token block, q / k / v and the MLP hidden rows in LDS, the policy kernel its per-layer vectors:
  // a geometry that does not fit is refused here, not at the first hvla_generate / hvla_step
  int extra_rows = 0;
  if (layer_tokens) {
    const int64_t nl = (int64_t)c.layers + 5 + (lang ? 1 : 0);
    if ((int64_t)c.lang_tokens + 1 + nl > CTX_MAX_ROWS) return HVLA_E_SHAPE;
    extra_rows = (int)nl - 1;
  }
  if (ctx_encoder_lds_bytes(c.lang_tokens, c.ctx_dim, c.ctx_mlp, c.enc_dim, extra_rows) > LDS_LIMIT) return HVLA_E_SHAPE;
  if ((int64_t)c.layers * (9 * 64 + (int64_t)c.mlp) * (int64_t)sizeof(float) > (int64_t)LDS_LIMIT) return HVLA_E_SHAPE;   // (keeps the offsets in int)
  if (policy_lds_bytes_of(c, lang, diff) > LDS_LIMIT) return HVLA_E_SHAPE;
  return HVLA_OK;
}

}  // namespace hvla
