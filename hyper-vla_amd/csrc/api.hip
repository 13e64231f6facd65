// api.hip — the C ABI of libhvla (include/hvla.h): context, weight packing, launch sequencing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hvla.h"
#include "common.h"
#include "kernels.h"
#include "layout.h"
#include "pack.h"
#include "serving_layout.h"
#include "t5.h"
#include "train.h"

using namespace hvla;

namespace {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) {
    if (p) { (void)hipFree(p); p = nullptr; }
    bytes = n;
    return n ? hipMalloc(&p, n) : hipSuccess;
  }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

using hvla::pack::bf2f;
using hvla::pack::f2bf;
using hvla::pack::f2h;

}  // namespace

struct hvla_weights {
  int B = 0;
  int Gm = 0, Gv = 0, C = 0;     // the row sizes it was allocated for (C: the floats of a context row, NL * ctx_dim): an arena of another geometry is refused where rows are written whole
  DevBuf wh, wl, vf, ctx, ring, count;
  DevBuf slot_count;             // int32 [B]: the episode pool's per-row ensemble counters (hvla_ensemble_slots)
};

struct hvla_post {               // per-slot post-processing state (hvla_post_*, postprocess.hip)
  int B = 0, H = 0;
  DevBuf ring;                   // f64 [B][H][H][HVLA_POST_DIM]
  DevBuf state;                  // PostSlot [B]
};

struct TrainState {               // what the hvla_train_* entries keep per context
  TrainLayout L{};                // the layout of the context's geometry, built by the first entry that train_refusal lets through
  bool have_layout = false;
  bool timer = false;             // this context switched its device's GEMM timer on (hvla_train_profile): hvla_destroy gives the events back
  TrainOptions sel;               // what the setters selected, all the caller's device memory: hvla_train_position_source (ps.n == 0: the baked
                                  // table is the parameter), hvla_train_frozen (mask and wholly frozen buckets), hvla_train_attention_losses
  int64_t frozen_n = 0;           // the mask's length, one of the two of hvla_train_sizes when it was set ...
  bool frozen_enc = false;        //   ... namely the one of this train_encoder value
  bool language_tokens = false;   // hvla_train_language_tokens: the entries serve this use_language_token context
  bool differential = false;      // hvla_train_differential: the entries serve this differential_attention context
  bool layer_tokens = false;      // hvla_train_layer_tokens: the entries serve this layer_tokens context ...
  DevBuf tiles;                   //   ... with the tile tables of its three grouped products (sel.groups points into them), built with the layout
  bool noise_set = false;         // hvla_train_noise_set holds a setting (sel.noise, by value; all rates 0 is a setting too)
  hipEvent_t ev_bucket[3] = {nullptr, nullptr, nullptr};   // hvla_train_step: gradient buckets final (created on first use)
  bool bucket_recorded[3] = {false, false, false};
};

struct hvla_ctx {
  hvla_config cfg{};
  Geom g{};
  int device = 0;
  std::string err;
  bool loaded = false;
  PackedLayout lay;
  int Kp = 0;
  // device weights
  DevBuf hn_f32;                 // context-encoder parameters, natural flax layout
  CtxParams ctxp{};
  DevBuf wcat_hi, wcat_lo, bcat, perm;
  DevBuf seg_token, tile_segs;   // layer_tokens: wcat_hi / wcat_lo then hold one fragment block per segment (pack.h TokenSegments)
  DevBuf seg_tile, pos_token, pos_head;   //   ... and what hvla_train_publish gathers them by: a segment's tile, a position's token and head column
  int nseg = 0;
  DevBuf enc16, encd16, encf32;  // encoder matrices (16-bit), their rounding residues x 4096 (16-bit) and vectors (f32)
  EncWeights encw{};
  // workspaces (sized for cfg.max_batch)
  DevBuf ctx_hi, ctx_lo, ctx_f32, tokens, flags;
  WorkspacePlan wsp;             // the encoder's workspace (plan.h): sizes of ws[] and where an episode's slice of each begins
  DevBuf ws[NUM_WS];
  uint32_t ln_spin = 800;        // EncWorkspace::ln_spin (8 us); hvla_debug_lnx_spin of the bench library changes it
#ifdef HVLA_BENCH_HOOKS
  int enc_stop = 0;              // EncWorkspace::stop_after (hvla_debug_encode_stop)
#endif
  Profiler prof;
  float *amap_dino = nullptr, *amap_head = nullptr;     // hvla_set_attention_outputs: caller-owned device buffers (opt-in)
  // cfg.streams == 2: helper stream and fork / join events of hvla_step
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // weight arenas handed back with hvla_weights_free wait here for the next hvla_generate of the same batch size: after
  // the first episode batch hvla_generate does not allocate (include/hvla.h: it can then be captured / does not sync)
  std::vector<hvla_weights*> arena_pool;
  std::mutex pool_mu;                        // hvla_weights_free can arrive from another thread (Python's GC) than hvla_generate
  static constexpr size_t ARENA_POOL_MAX = 4;
  TrainState train;
  ~hvla_ctx() {
    for (hvla_weights* w : arena_pool) delete w;
    for (hipEvent_t e : train.ev_bucket)
      if (e) (void)hipEventDestroy(e);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (side) (void)hipStreamDestroy(side);
  }
  // observation preprocessing (hvla_preprocess): span tables of the last (H, W) and scratch
  int rs_H = 0, rs_W = 0, rs_row_span = 0, rs_col_span = 0;
  DevBuf rs_tab, rs_rows, rs_img, rs_pad;
  // optional frozen T5 instruction encoder (hvla_t5_load)
  bool t5_loaded = false;
  T5Dims t5d{};
  T5Weights t5w{};
  DevBuf t5_f32, t5_work;
  int t5_max_batch = 0;
};

#define FAIL(ctx, code, ...)                       \
  do {                                             \
    char _b[512];                                  \
    snprintf(_b, sizeof _b, __VA_ARGS__);          \
    (ctx)->err = _b;                               \
    return (code);                                 \
  } while (0)
#define HIPCHK(ctx, call)                                                               \
  do {                                                                                  \
    hipError_t _e = (call);                                                             \
    if (_e != hipSuccess) FAIL(ctx, HVLA_E_HIP, "%s: %s", #call, hipGetErrorString(_e)); \
  } while (0)

extern "C" {

// why this thread's last hvla_create_with_v2 refused, where it had a text (there is no ctx to hold it); else null
static thread_local const char* create_refusal = nullptr;

const char* hvla_last_error(const hvla_ctx* ctx) { return ctx ? ctx->err.c_str() : (create_refusal ? create_refusal : "null ctx"); }

int hvla_create(const hvla_config* c, int device, hvla_ctx** out) { return hvla_create_with(c, nullptr, device, out); }

int hvla_create_with(const hvla_config* c, const hvla_policy_options* opts, int device, hvla_ctx** out) {
  if (!c || !out) return HVLA_E_SHAPE;
  *out = nullptr;
  create_refusal = nullptr;
  if (opts && opts->struct_size != sizeof(hvla_policy_options)) return HVLA_E_SHAPE;   // hvla_config's rule for the options: never read past the caller's struct
  const hvla_policy_options_v2 v2{sizeof(hvla_policy_options_v2), opts ? opts->use_language_token : 0, 0};
  return hvla_create_with_v2(c, opts ? &v2 : nullptr, device, out);
}

int hvla_create_with_v2(const hvla_config* c, const hvla_policy_options_v2* opts, int device, hvla_ctx** out) {
  if (!c || !out) return HVLA_E_SHAPE;
  *out = nullptr;
  create_refusal = nullptr;
  if (opts && opts->struct_size != sizeof(hvla_policy_options_v2)) return HVLA_E_SHAPE;   // the same rule for the options
  const hvla_policy_options_v3 v3{sizeof(hvla_policy_options_v3), opts ? opts->use_language_token : 0,
                                  opts ? opts->attention_mask_as_bias : 0, 0};
  return hvla_create_with_v3(c, opts ? &v3 : nullptr, device, out);
}

int hvla_create_with_v3(const hvla_config* c, const hvla_policy_options_v3* opts, int device, hvla_ctx** out) {
  if (!c || !out) return HVLA_E_SHAPE;
  *out = nullptr;
  create_refusal = nullptr;
  if (opts && opts->struct_size != sizeof(hvla_policy_options_v3)) return HVLA_E_SHAPE;   // the same rule for the options
  const hvla_policy_options_v4 v4{sizeof(hvla_policy_options_v4), opts ? opts->use_language_token : 0, opts ? opts->attention_mask_as_bias : 0,
                                  opts ? opts->differential_attention : 0, 0, 0};
  return hvla_create_with_v4(c, opts ? &v4 : nullptr, device, out);
}

int hvla_create_with_v4(const hvla_config* c, const hvla_policy_options_v4* opts, int device, hvla_ctx** out) {
  if (!c || !out) return HVLA_E_SHAPE;
  *out = nullptr;
  create_refusal = nullptr;
  if (c->struct_size != sizeof(hvla_config)) return HVLA_E_SHAPE;   // the caller's header is not this library's: never read past its struct
  if (opts && opts->struct_size != sizeof(hvla_policy_options_v4)) return HVLA_E_SHAPE;   // the same rule for the options
  const int ltok = opts ? opts->layer_tokens : 0, shared = opts ? opts->shared_block_heads : 0;
  if ((ltok != 0 && ltok != 1) || (shared != 0 && shared != 1)) return HVLA_E_SHAPE;
  if (shared && !ltok) {
    create_refusal = "shared_block_heads without layer_tokens: with share_TF_output_head and one shared layer token every policy block "
                     "would receive the same weights";
    return HVLA_E_SHAPE;
  }
  const int lang = opts ? opts->use_language_token : 0;
  if (lang != 0 && lang != 1) return HVLA_E_SHAPE;
  const int mab = opts ? opts->attention_mask_as_bias : 0;
  if (mab != 0 && mab != 1) return HVLA_E_SHAPE;
  const int diff = opts ? opts->differential_attention : 0;
  if (diff != 0 && diff != 1) return HVLA_E_SHAPE;
  if (mab && lang) {
    create_refusal = "attention_mask_as_bias with use_language_token is not built: with the mask added as a bias language queries "
                     "attend to patch keys, so the language prefix is no per-episode constant";
    return HVLA_E_SHAPE;
  }
  if (diff && lang) {
    create_refusal = "differential_attention with use_language_token is not built: DifferentialAttention adds the mask as a bias, so "
                     "language queries attend to patch keys and the language prefix is no per-episode constant";
    return HVLA_E_SHAPE;
  }
  if (diff && mab) {
    create_refusal = "differential_attention with attention_mask_as_bias: with both vit_kwargs set the reference runs "
                     "DifferentialAttention (transformer.py:166-172), which is differential_attention alone";
    return HVLA_E_SHAPE;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return HVLA_E_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HVLA_E_DEVICE;
  if (!strstr(prop.gcnArchName, "gfx950")) return HVLA_E_DEVICE;   // CDNA4 only: no fallback path
  std::unique_ptr<hvla_ctx> ctx(new hvla_ctx);
  ctx->cfg = *c;
  ctx->device = device;
  Geom& g = ctx->g;
  // what the hand-written kernels are specialised for (anything else is refused, never emulated): the predicate of accept.h,
  // which also refuses a context encoder or a policy that does not fit its kernel's LDS here, not at the first hvla_generate / hvla_step
  if (const int verdict = accept_geometry(*c, lang, diff, ltok)) return verdict;
  g = geom_of(*c, lang, diff);
  g.mask_as_bias = mab;
  g.layer_tokens = ltok;
  g.shared_block_heads = shared;
  const int P = g.P();
  if (hipSetDevice(device) != hipSuccess) return HVLA_E_DEVICE;
  ctx->lay = build_layout(g);
  ctx->Kp = serving::patch_kp(g);
  {  // the packed order must be a bijection onto the reference parameter vector
    std::vector<uint8_t> seen(ctx->lay.pl.G, 0);
    for (int32_t r : ctx->lay.perm)
      if (r >= 0) {
        if (r >= ctx->lay.pl.G || seen[r]) return HVLA_E_STATE;
        seen[r] = 1;
      }
    for (uint8_t s : seen)
      if (!s) return HVLA_E_STATE;
  }
  const size_t Bm = c->max_batch;
  ctx->wsp = WorkspacePlan(P, g.S(), g.E, g.enc_mlp, ctx->Kp, c->max_batch);
  hipError_t e = hipSuccess;
  auto A = [&](DevBuf& b, size_t n) { if (e == hipSuccess) e = b.alloc(n); };
  A(ctx->ctx_hi, Bm * g.ctx_row() * 2); A(ctx->ctx_lo, Bm * g.ctx_row() * 2); A(ctx->ctx_f32, Bm * g.ctx_row() * 4);   // [Bm][NL][C]
  A(ctx->tokens, Bm * P * g.E * 4); A(ctx->flags, 64 * sizeof(int));
  for (int i = 0; i < NUM_WS; ++i) A(ctx->ws[i], ctx->wsp.bytes(i));
  if (e != hipSuccess) return HVLA_E_ARENA_FULL;
  if (hipMemset(ctx->ws[WS_LN_CNT].p, 0, ctx->ws[WS_LN_CNT].bytes) != hipSuccess) return HVLA_E_HIP;
  // the packed order on the device: a property of the geometry, so hvla_weights_import can run before any weights are loaded
  if (ctx->perm.alloc(ctx->lay.perm.size() * 4) != hipSuccess) return HVLA_E_ARENA_FULL;
  if (hipMemcpy(ctx->perm.p, ctx->lay.perm.data(), ctx->lay.perm.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return HVLA_E_HIP;
  if (c->streams == 2) {
    if (hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess)
      return HVLA_E_HIP;
  }
  *out = ctx.release();
  return HVLA_OK;
}

void hvla_destroy(hvla_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->train.timer) train_gemm_timer_release();
  delete ctx;
}

int64_t hvla_num_generated(const hvla_ctx* ctx) { return ctx ? ctx->lay.pl.G : 0; }
int32_t hvla_num_layer_tokens(const hvla_ctx* ctx) { return ctx ? ctx->g.NL() : 0; }

int hvla_load_weights(hvla_ctx* ctx, const hvla_tensor_desc* t, int32_t n) {
  if (!ctx) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const Geom& g = ctx->g;
  std::map<std::string, const hvla_tensor_desc*> m;
  for (int i = 0; i < n; ++i) {
    if (!t[i].name || !t[i].data) FAIL(ctx, HVLA_E_WEIGHTS, "tensor %d has null name/data", i);
    m[t[i].name] = &t[i];
  }
  // ---- pack on the host: the order, the names and the arithmetic are serving_layout.h's
  serving::HostImages h;
  auto lookup = [&](const std::string& name) {
    auto it = m.find(name);
    using R = std::pair<const float*, int64_t>;
    return it == m.end() ? R{nullptr, 0} : R{it->second->data, it->second->numel};
  };
  if (!serving::pack_serving(g, ctx->cfg.enc_dtype == HVLA_ENC_BF16, lookup, h))
    FAIL(ctx, HVLA_E_WEIGHTS, "checkpoint tensor %s", h.missing.c_str());
  // W_cat^T fragments (layout.h): tile pt, k-step ks, lane (rho = l & 31, hk = l >> 5), j
  std::vector<uint16_t> hi, lo;
  std::vector<float> bc;
  pack::pack_wcat(ctx->lay, h.leaves, h.lk, h.lb, g.C, hi, lo, bc);
  pack::TokenSegments segs;
  if (g.layer_tokens) {      // one fragment block per (tile, token) segment instead of one per tile (pack.h)
    segs = pack::build_segments(g, ctx->lay, h.leaves);
    std::vector<uint16_t> shi, slo;
    pack::pack_segments(segs, g.C, hi, lo, shi, slo);
    hi.swap(shi); lo.swap(slo);
  }

  // ---- upload
  auto up = [&](DevBuf& b, const void* src, size_t bytes) {
    const hipError_t e = b.alloc(bytes);
    return e != hipSuccess ? e : hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
  };
  HIPCHK(ctx, up(ctx->hn_f32, h.hn.data(), h.hn.size() * 4));
  HIPCHK(ctx, up(ctx->wcat_hi, hi.data(), hi.size() * 2));
  HIPCHK(ctx, up(ctx->wcat_lo, lo.data(), lo.size() * 2));
  HIPCHK(ctx, up(ctx->bcat, bc.data(), bc.size() * 4));
  if (g.layer_tokens) {
    HIPCHK(ctx, up(ctx->seg_token, segs.token.data(), segs.token.size() * 4));
    HIPCHK(ctx, up(ctx->tile_segs, segs.tile_segs.data(), segs.tile_segs.size() * 4));
    // publish.hip's maps: the head column of every packed position, through the training layout's run table
    const TrainLayout L = make_train_layout(g);
    std::vector<int32_t> pos_head(segs.pos_token.size(), -1);
    if (L.policy_ok)
      for (size_t pos = 0; pos < pos_head.size(); ++pos) {
        const int32_t ref = ctx->lay.perm[pos];
        for (int r = 0; r < L.nruns && ref >= 0; ++r)
          if (ref >= L.run[r].tcol && ref < L.run[r].tcol + L.run[r].width) pos_head[pos] = (int32_t)(L.run[r].hcol + (ref - L.run[r].tcol));
      }
    HIPCHK(ctx, up(ctx->seg_tile, segs.tile.data(), segs.tile.size() * 4));
    HIPCHK(ctx, up(ctx->pos_token, segs.pos_token.data(), segs.pos_token.size() * 4));
    HIPCHK(ctx, up(ctx->pos_head, pos_head.data(), pos_head.size() * 4));
    ctx->nseg = (int)segs.token.size();
  }
  HIPCHK(ctx, up(ctx->enc16, h.enc16.data(), h.enc16.size() * 2));
  HIPCHK(ctx, up(ctx->encd16, h.encd16.data(), h.encd16.size() * 2));
  HIPCHK(ctx, up(ctx->encf32, h.encf.data(), h.encf.size() * 4));

  // ---- the kernels' pointers, each from the offset of the tensor it names (q / k / v lie one behind the other: one pointer)
  const serving::Offsets& at = h.at;
  const float* hn = ctx->hn_f32.as<float>();
  CtxParams& cp = ctx->ctxp;
  cp = CtxParams{};
  cp.T = g.T; cp.C = g.C; cp.F = g.ctx_mlp; cp.heads = g.ctx_heads; cp.layers = g.ctx_layers; cp.lang_dim = g.lang_dim; cp.E = g.E;
  cp.scale_context = g.scale_context;
#define HN(to, from, f) to.f = hn + from.f           // the context encoder's pointers carry the names of TrainLayout's members
  HN(cp, at, w_tok); HN(cp, at, b_tok); HN(cp, at, w_img); HN(cp, at, b_img); HN(cp, at, pos_tok); HN(cp, at, pos_img);
  HN(cp, at, pos_layer); HN(cp, at, norm_s); HN(cp, at, norm_b);
  for (int l = 0; l < g.ctx_layers; ++l) {
    const BlockLeaves& o = at.layer[l];
    CtxLayer& c = cp.layer[l];
    HN(c, o, ln0_s); HN(c, o, ln0_b); HN(c, o, wq); HN(c, o, bq); HN(c, o, wk); HN(c, o, bk); HN(c, o, wv); HN(c, o, bv);
    HN(c, o, wo); HN(c, o, bo); HN(c, o, ln1_s); HN(c, o, ln1_b); HN(c, o, w1); HN(c, o, b1); HN(c, o, w2); HN(c, o, b2);
  }
#undef HN
  const uint16_t *e16 = ctx->enc16.as<uint16_t>(), *dd = ctx->encd16.as<uint16_t>();
  const float* df = ctx->encf32.as<float>();
  EncWeights& w = ctx->encw;
  w.w_patch = e16 + at.e_pk; w.b_patch = df + at.e_pb; w.pos = df + at.e_pos; w.lnf_s = df + at.e_lns; w.lnf_b = df + at.e_lnb;
  for (int i = 0; i < g.enc_layers; ++i) {
    const BlockLeaves& o = at.enc[i];
    EncLayerW& L = w.layer[i];
    L.wqkv = e16 + o.wq; L.wo = e16 + o.wo; L.w1 = e16 + o.w1; L.w2 = e16 + o.w2;
    L.dqkv = dd + o.wq; L.dwo = dd + o.wo; L.dw1 = dd + o.w1; L.dw2 = dd + o.w2;
    L.bqkv = df + o.bq; L.bo = df + o.bo; L.b1 = df + o.b1; L.b2 = df + o.b2;
    L.ln1_s = df + o.ln0_s; L.ln1_b = df + o.ln0_b; L.ln2_s = df + o.ln1_s; L.ln2_b = df + o.ln1_b; L.ls1 = df + o.ls1; L.ls2 = df + o.ls2;
  }
  HIPCHK(ctx, hipDeviceSynchronize());
  ctx->loaded = true;
  return HVLA_OK;
}

// What the count argument of a serving entry counts: a batch of the context (and of the arena, if the entry has one), call rows
// mapped to slots of a pool, or nothing.  `workspace`: the entry runs the context's weights in its max_batch-sized workspace --
// all but the ensemble entries, which touch the arena alone and ask neither for loaded weights nor for max_batch.
struct ServeCount {
  enum Kind { NONE, BATCH, SLOTS } kind;
  bool workspace;
  int32_t n;
  const hvla_weights* w;
  const int32_t* slots;
};
static ServeCount batch_of(int32_t B, const hvla_weights* w = nullptr) { return {ServeCount::BATCH, true, B, w, nullptr}; }
static ServeCount slots_of(const hvla_weights* w, const int32_t* slots, int32_t K, bool workspace = true) {
  return {ServeCount::SLOTS, workspace, K, w, slots};
}
static ServeCount arena_only() { return {ServeCount::NONE, false, 0, nullptr, nullptr}; }

// The head of every serving entry, in the order each of them used to check by hand: the handles (ctx, and `handles`: the entry's arena
// or out pointer) -> HVLA_E_STATE, the weights loaded, the count, the entry's other must-not-be-null pointers (`args`), the device.
// Hands the stream back.
static int serve_entry(hvla_ctx* ctx, bool handles, const ServeCount& c, bool args, void* stream, hipStream_t& st) {
  if (!ctx || !handles) return HVLA_E_STATE;
  if (c.workspace && !ctx->loaded) FAIL(ctx, HVLA_E_STATE, "called before hvla_load_weights");
  const int32_t Bm = ctx->cfg.max_batch;
  if (c.kind == ServeCount::BATCH) {
    if (c.n < 1 || c.n > Bm) FAIL(ctx, HVLA_E_SHAPE, "batch %d outside [1, %d]", c.n, Bm);
    if (c.w && c.n != c.w->B) FAIL(ctx, HVLA_E_SHAPE, "batch %d != arena batch %d", c.n, c.w->B);
  } else if (c.kind == ServeCount::SLOTS) {
    if (!c.slots) FAIL(ctx, HVLA_E_SHAPE, "null slot map");
    const int32_t cap = c.workspace && Bm < c.w->B ? Bm : c.w->B;
    if (c.n < 1 || c.n > cap) FAIL(ctx, HVLA_E_SHAPE, "%d slots outside [1, %d] (a pool of %d slots, max_batch %d)", c.n, cap, c.w->B, Bm);
  }
  if (!args) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  st = reinterpret_cast<hipStream_t>(stream);
  return HVLA_OK;
}

// an arena of B episodes: one handed back by hvla_weights_free if the ctx holds one of that size, else a new allocation
static int take_arena(hvla_ctx* ctx, int32_t B, std::unique_ptr<hvla_weights>& w) {
  const PolicyLayout& pl = ctx->lay.pl;
  const Geom& g = ctx->g;
  {
    std::lock_guard<std::mutex> lk(ctx->pool_mu);
    for (size_t i = 0; i < ctx->arena_pool.size(); ++i)        // an arena of this batch size handed back earlier
      if (ctx->arena_pool[i]->B == B) {
        w.reset(ctx->arena_pool[i]);
        ctx->arena_pool.erase(ctx->arena_pool.begin() + i);
        return HVLA_OK;
      }
  }
  w.reset(new hvla_weights);
  w->B = B;
  w->Gm = pl.Gm; w->Gv = pl.Gv; w->C = g.ctx_row();
  hipError_t e = hipSuccess;
  auto A = [&](DevBuf& b, size_t n) { if (e == hipSuccess) e = b.alloc(n); };
  auto all = [&]() {
    A(w->wh, (size_t)B * pl.Gm * 2); A(w->wl, (size_t)B * pl.Gm * 2); A(w->vf, (size_t)B * pl.Gv * 4);
    A(w->ctx, (size_t)B * g.ctx_row() * 4);
    A(w->ring, (size_t)g.horizon * B * g.horizon * g.action_dim * 4); A(w->count, 16); A(w->slot_count, (size_t)B * 4);
  };
  all();
  if (e != hipSuccess) {
    {
      std::lock_guard<std::mutex> lk(ctx->pool_mu);
      for (hvla_weights* q : ctx->arena_pool) delete q;      // give the pooled arenas back to the device and retry once
      ctx->arena_pool.clear();
    }
    e = hipSuccess;
    all();
  }
  if (e != hipSuccess) FAIL(ctx, HVLA_E_ARENA_FULL, "weight arena for %d episodes: %s", B, hipGetErrorString(e));
  return HVLA_OK;
}

// use_language_token: K episodes' language tokens (tok [K, T, lang_dim]) through the policy once, into the language prefix of their
// arena rows (slots[k], or k) (lang_prefix_kernel); nothing to do without the option
static int lang_prefix(hvla_ctx* ctx, hvla_weights* w, const float* tok, int K, const int32_t* slots, hipStream_t st) {
  const LangLayout& ll = ctx->lay.ll;
  if (!ll.on) return HVLA_OK;
  const Geom& g = ctx->g;
  LangPrefixParams lp{ctx->lay.pl, ll.m_lproj, ll.m_lkv, ll.v_lproj_b, ll.v_lpos, w->wh.as<__bf16>(), w->wl.as<__bf16>(),
                      w->vf.as<float>(), tok, slots, w->B, g.T, g.lang_dim, g.L, g.M};
  ++ctx->prof.nlaunch;
  HIPCHK(ctx, launch_lang_prefix(lp, K, st));
  return HVLA_OK;
}

// K tasks through context encoder -> weight generation -> language prefix into arena w.  slots null (hvla_generate): into rows
// 0 .. K-1, the f32 context rows straight into the arena.  Else (the episode pool) into rows slots[k]: the unchanged context encoder
// writes workspace rows 0 .. K-1, and pool_assign moves the f32 rows to their slots and zeroes those slots' ensemble counters.
static int generate_body(hvla_ctx* ctx, hvla_weights* w, const int32_t* slots, int K, const float* tok, const int64_t* mask,
                         const float* cls, hipStream_t st) {
  const PolicyLayout& pl = ctx->lay.pl;
  const Geom& g = ctx->g;
  CtxParams cp = ctx->ctxp;
  cp.tok = tok; cp.attn_mask = mask; cp.cls = cls;
  cp.ctx = slots ? ctx->ctx_f32.as<float>() : w->ctx.as<float>(); cp.ctx_hi = ctx->ctx_hi.as<__bf16>(); cp.ctx_lo = ctx->ctx_lo.as<__bf16>();
  HIPCHK(ctx, launch_ctx_encoder(cp, K, st, g.layer_tokens ? g.NL() : 0));
  WeightGenParams wp{ctx->wcat_hi.as<__bf16>(), ctx->wcat_lo.as<__bf16>(), ctx->bcat.as<float>(),
                     ctx->ctx_hi.as<__bf16>(), ctx->ctx_lo.as<__bf16>(), w->wh.as<__bf16>(), w->wl.as<__bf16>(),
                     w->vf.as<float>(), K, pl.Gm, pl.Gv, (pl.Gm + pl.Gv) / 32};
  if (g.layer_tokens) {
    const WeightGenTokensParams tp{wp, ctx->seg_token.as<int32_t>(), ctx->tile_segs.as<int32_t>()};
    HIPCHK(ctx, launch_weightgen_tokens(tp, g.C, st, slots, w->B));
  } else {
    HIPCHK(ctx, launch_weightgen(wp, g.C, st, slots, w->B));
  }
  if (slots)
    HIPCHK(ctx, launch_pool_assign(ctx->ctx_f32.as<float>(), w->ctx.as<float>(), w->slot_count.as<int>(), slots, K, g.ctx_row(), w->B, st));
  return lang_prefix(ctx, w, tok, K, slots, st);
}

int hvla_generate(hvla_ctx* ctx, const float* tok, const int64_t* mask, const float* cls, int32_t B,
                  hvla_weights** out, void* stream) {
  if (ctx && out) *out = nullptr;
  hipStream_t st;
  if (int r = serve_entry(ctx, out != nullptr, batch_of(B), tok && mask && cls, stream, st)) return r;
  std::unique_ptr<hvla_weights> w;
  if (int r = take_arena(ctx, B, w)) return r;
  HIPCHK(ctx, hipMemsetAsync(w->count.p, 0, 16, st));
  HIPCHK(ctx, hipMemsetAsync(w->slot_count.p, 0, w->slot_count.bytes, st));   // (the arena may have served as an episode pool)
  if (int r = generate_body(ctx, w.get(), nullptr, B, tok, mask, cls, st)) return r;
  *out = w.release();
  return HVLA_OK;
}

int hvla_weights_free(hvla_ctx* ctx, hvla_weights* w) {
  if (!w) return HVLA_OK;
  if (!ctx) { delete w; return HVLA_OK; }
  (void)hipSetDevice(ctx->device);
  // hipFree waited for the device; a pooled arena must give the same guarantee before another stream's hvla_generate
  // writes into it (this call has no stream of its own: frees happen at episode resets, not in the step loop)
  (void)hipDeviceSynchronize();
  std::lock_guard<std::mutex> lk(ctx->pool_mu);
  if (ctx->arena_pool.size() < hvla_ctx::ARENA_POOL_MAX) ctx->arena_pool.push_back(w);
  else delete w;
  return HVLA_OK;
}

int hvla_release_pooled_arenas(hvla_ctx* ctx) {
  if (!ctx) return HVLA_E_STATE;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  std::lock_guard<std::mutex> lk(ctx->pool_mu);
  for (hvla_weights* q : ctx->arena_pool) delete q;
  ctx->arena_pool.clear();
  return HVLA_OK;
}

int32_t hvla_weights_batch(const hvla_weights* w) { return w ? w->B : 0; }

int hvla_weights_export(hvla_ctx* ctx, const hvla_weights* w, float* theta, float* context, void* stream) {
  if (!ctx || !w) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const PolicyLayout& pl = ctx->lay.pl;
  if (theta)
    HIPCHK(ctx, launch_export_theta(w->wh.as<__bf16>(), w->wl.as<__bf16>(), w->vf.as<float>(), ctx->perm.as<int32_t>(),
                                    pl.Gm, pl.Gv, pl.G, w->B, theta, st));
  if (context)
    HIPCHK(ctx, hipMemcpyAsync(context, w->ctx.p, (size_t)w->B * ctx->g.ctx_row() * 4, hipMemcpyDeviceToDevice, st));
  return HVLA_OK;
}

// episodes [b0, b0 + nb) of the batch: every per-episode buffer is offset, the workspace slices are those of the context's table
// (disjoint for the two halves of a two-stream step).  audit (hvla_encode_audit's test instrumentation): the call then runs outside
// the profiler and the launch count, and exports no attention map.
static int encode_range(hvla_ctx* ctx, const uint8_t* images, float* out, int b0, int nb, bool keep_cls, hipStream_t st,
                        uint32_t* audit = nullptr) {
  const Geom& g = ctx->g;
  auto at = [&](int buf) { return static_cast<char*>(ctx->ws[buf].p) + ctx->wsp.offset(buf, b0); };
  EncWorkspace ws{reinterpret_cast<float*>(at(WS_X)), at(WS_H), at(WS_QKV), at(WS_G), reinterpret_cast<float*>(at(WS_CORR)), at(WS_ABAR)};
  if (ctx->amap_dino && !audit) ws.amap = ctx->amap_dino + (size_t)b0 * g.enc_layers * g.enc_heads * g.P();
  ws.ln_cnt = reinterpret_cast<uint32_t*>(at(WS_LN_CNT));
  ws.ln_part = reinterpret_cast<float*>(at(WS_LN_PART));
  ws.ln_spin = ctx->ln_spin;
#ifdef HVLA_BENCH_HOOKS
  if (!audit) ws.stop_after = ctx->enc_stop;
#endif
  const size_t img = (size_t)g.image_size * g.image_size * 3, per = (keep_cls ? (size_t)g.S() : (size_t)g.P()) * g.E;
  HIPCHK(ctx, launch_encoder(g, ctx->cfg.enc_dtype, ctx->encw, ws, images + (size_t)b0 * img, out + (size_t)b0 * per, nb, st,
                             audit ? nullptr : &ctx->prof, keep_cls, audit));
  return HVLA_OK;
}

int hvla_encode(hvla_ctx* ctx, const uint8_t* images, float* tokens, int32_t B, void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, true, batch_of(B), images && tokens, stream, st)) return r;
  return encode_range(ctx, images, tokens, 0, B, false, st);
}

int hvla_encode_hidden(hvla_ctx* ctx, const uint8_t* images, float* hidden, int32_t B, void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, true, batch_of(B), images && hidden, stream, st)) return r;
  return encode_range(ctx, images, hidden, 0, B, true, st);
}

// test instrumentation: the encoder with a range audit of every 16-bit MFMA operand it writes (LayerNorm outputs, q / k /
// v, attention outputs, GELU outputs; all layers).  maxabs f32 [4], nonfinite i32 [4]: HOST pointers.
int hvla_encode_audit(hvla_ctx* ctx, const uint8_t* images, int32_t B, float* maxabs, int32_t* nonfinite, void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, true, batch_of(B), images && maxabs && nonfinite, stream, st)) return r;
  uint32_t* slots = reinterpret_cast<uint32_t*>(ctx->flags.p);
  HIPCHK(ctx, hipMemsetAsync(slots, 0, 8 * sizeof(uint32_t), st));
  if (int r = encode_range(ctx, images, ctx->tokens.as<float>(), 0, B, false, st, slots)) return r;
  uint32_t h[8];
  HIPCHK(ctx, hipMemcpyAsync(h, slots, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (int i = 0; i < 4; ++i) {
    memcpy(&maxabs[i], &h[2 * i], 4);
    nonfinite[i] = (int32_t)h[2 * i + 1];
  }
  return HVLA_OK;
}

// slots (episode pool): call row b takes its weights from arena row slots[b]; the arena pointers then stay at row 0 and the
// slot map moves with b0 instead
static int policy_range(hvla_ctx* ctx, const hvla_weights* w, const float* tokens, float* actions, float* logits, int b0,
                        int nb, hipStream_t st, const int32_t* slots = nullptr) {
  const Geom& g = ctx->g;
  const PolicyLayout& pl = ctx->lay.pl;
  const size_t wb = slots ? 0 : (size_t)b0;
  PolicyParams p{pl, w->wh.as<__bf16>() + wb * pl.Gm, w->wl.as<__bf16>() + wb * pl.Gm,
                 w->vf.as<float>() + wb * pl.Gv, tokens + (size_t)b0 * g.P() * g.E,
                 actions + (size_t)b0 * g.horizon * g.action_dim, logits ? logits + (size_t)b0 * g.horizon : nullptr,
                 nb, g.E, g.P(), g.L, g.M, g.horizon, g.action_dim, g.tanh_scale, g.max_action};
  const LangLayout& ll = ctx->lay.ll;
  const int lang_T = ll.on ? g.T : 0;                           // use_language_token: the head map has lang_T + P keys
  if (ctx->amap_head && g.differential) FAIL(ctx, HVLA_E_SHAPE, "no attention-map export with differential_attention");   // (hvla_set_attention_outputs refuses it)
  if (ctx->amap_head) p.amap = ctx->amap_head + (size_t)b0 * g.L * g.H * (g.P() + lang_T);
  ctx->prof.begin(HVLA_PROF_POLICY, st);
  ++ctx->prof.nlaunch;
  HIPCHK(ctx, launch_policy(p, st, lang_T, slots ? slots + b0 : nullptr, w->B, g.mask_as_bias != 0, g.differential != 0));
  ctx->prof.end(HVLA_PROF_POLICY, st);
  return HVLA_OK;
}

int hvla_policy(hvla_ctx* ctx, const hvla_weights* w, const float* tokens, float* actions, float* logits, int32_t B,
                void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, w != nullptr, batch_of(B, w), tokens && actions, stream, st)) return r;
  return policy_range(ctx, w, tokens, actions, logits, 0, B, st);
}

int hvla_set_attention_outputs(hvla_ctx* ctx, float* dino_cls_attention, float* head_attention) {
  if (!ctx) return HVLA_E_STATE;
  if (head_attention && ctx->g.differential)
    FAIL(ctx, HVLA_E_SHAPE, "head_attention with differential_attention: DifferentialAttention sows no attention weights "
         "(transformer.py:166-171), there is no map of the action token to export");
  ctx->amap_dino = dino_cls_attention;
  ctx->amap_head = head_attention;
  return HVLA_OK;
}

// One step of n call rows on arena w: its episodes 0 .. n-1 (slots null), or call row b on the weights of arena row slots[b].
static int step_body(hvla_ctx* ctx, const hvla_weights* w, const int32_t* slots, int n, const uint8_t* images, float* actions,
                     float* logits, hipStream_t st) {
  float* tokens = ctx->tokens.as<float>();
  if (!ctx->side || n < 64) {
    if (int r = encode_range(ctx, images, tokens, 0, n, false, st)) return r;
    return policy_range(ctx, w, tokens, actions, logits, 0, n, st, slots);
  }
  // two halves on two streams: while one half is in an HBM-bound kernel (LayerNorm, a residual epilogue, attention
  // staging) or in the ragged end of a grid, the other half's GEMM has the matrix cores.  Episodes are independent and
  // every kernel is batch-invariant, so the bytes are those of the single-stream step.
  const int b0 = n / 2;
  HIPCHK(ctx, hipEventRecord(ctx->ev_fork, st));
  HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
  if (int r = encode_range(ctx, images, tokens, 0, b0, false, st)) return r;
  if (int r = encode_range(ctx, images, tokens, b0, n - b0, false, ctx->side)) return r;
  if (int r = policy_range(ctx, w, tokens, actions, logits, 0, b0, st, slots)) return r;
  if (int r = policy_range(ctx, w, tokens, actions, logits, b0, n - b0, ctx->side, slots)) return r;
  HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->side));
  HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_join, 0));
  return HVLA_OK;
}

int hvla_step(hvla_ctx* ctx, const hvla_weights* w, const uint8_t* images, float* actions, float* logits, int32_t B,
              void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, w != nullptr, batch_of(B, w), images && actions, stream, st)) return r;
  return step_body(ctx, w, nullptr, B, images, actions, logits, st);
}

int hvla_ensemble_reset(hvla_ctx* ctx, hvla_weights* w, void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, w != nullptr, arena_only(), true, stream, st)) return r;
  HIPCHK(ctx, hipMemsetAsync(w->count.p, 0, 16, st));
  HIPCHK(ctx, hipMemsetAsync(w->slot_count.p, 0, w->slot_count.bytes, st));
  return HVLA_OK;
}

// slots null: the arena's B episodes on its one counter; else K call rows on the counters of their slots
static int ensemble_body(hvla_ctx* ctx, hvla_weights* w, const int32_t* slots, int K, const float* actions, const float* mean,
                         const float* std, const uint8_t* mask, float* out, hipStream_t st) {
  ++ctx->prof.nlaunch;
  HIPCHK(ctx, launch_ensemble(actions, w->ring.as<float>(), slots ? w->slot_count.as<int>() : w->count.as<int>(), mean, std, mask, out,
                              w->B, ctx->g.horizon, ctx->g.action_dim, st, slots, K));
  return HVLA_OK;
}

int hvla_ensemble(hvla_ctx* ctx, hvla_weights* w, const float* actions, const float* mean, const float* std,
                  const uint8_t* mask, float* out, void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, w != nullptr, arena_only(), actions && mean && std && mask && out, stream, st)) return r;
  return ensemble_body(ctx, w, nullptr, 0, actions, mean, std, mask, out, st);
}

// ------------------------------------------------------------------ episode pool (include/hvla.h)
int hvla_weights_alloc(hvla_ctx* ctx, int32_t B, hvla_weights** out, void* stream) {
  if (ctx && out) *out = nullptr;
  hipStream_t st;
  if (int r = serve_entry(ctx, out != nullptr, batch_of(B), true, stream, st)) return r;
  std::unique_ptr<hvla_weights> w;
  if (int r = take_arena(ctx, B, w)) return r;
  // empty slots: zero weights step to finite actions, zero counters start a fresh ensemble
  for (DevBuf* b : {&w->wh, &w->wl, &w->vf, &w->ctx, &w->ring, &w->count, &w->slot_count})
    HIPCHK(ctx, hipMemsetAsync(b->p, 0, b->bytes, st));
  *out = w.release();
  return HVLA_OK;
}

int hvla_generate_slots(hvla_ctx* ctx, hvla_weights* w, const int32_t* slots, int32_t K, const float* tok, const int64_t* mask,
                        const float* cls, void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, w != nullptr, slots_of(w, slots, K), tok && mask && cls, stream, st)) return r;
  return generate_body(ctx, w, slots, K, tok, mask, cls, st);
}

int hvla_step_slots(hvla_ctx* ctx, const hvla_weights* w, const int32_t* slots, int32_t K, const uint8_t* images, float* actions,
                    float* logits, void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, w != nullptr, slots_of(w, slots, K), images && actions, stream, st)) return r;
  return step_body(ctx, w, slots, K, images, actions, logits, st);
}

int hvla_ensemble_slots(hvla_ctx* ctx, hvla_weights* w, const int32_t* slots, int32_t K, const float* actions, const float* mean,
                        const float* std, const uint8_t* mask, float* out, void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, w != nullptr, slots_of(w, slots, K, false), actions && mean && std && mask && out, stream, st)) return r;
  return ensemble_body(ctx, w, slots, K, actions, mean, std, mask, out, st);
}

// ------------------------------------------------------------------ weight arenas as values (include/hvla.h)
// None of these asks for loaded weights: the permutation is the geometry's, and the language prefix reads the arena and the tokens only.
static ServeCount arena_batch_of(int32_t B) { return {ServeCount::BATCH, false, B, nullptr, nullptr}; }

// rows are written whole, so the arena must have this context's row sizes (an arena of another context with the same geometry is fine)
static int arena_fits(hvla_ctx* ctx, const hvla_weights* w, const char* what) {
  const PolicyLayout& pl = ctx->lay.pl;
  if (w->Gm != pl.Gm || w->Gv != pl.Gv || w->C != ctx->g.ctx_row())
    FAIL(ctx, HVLA_E_SHAPE, "the %s arena belongs to another geometry (rows of %d + %d weights and %d context floats, this context's have %d + %d and %d)",
         what, w->Gm, w->Gv, w->C, pl.Gm, pl.Gv, ctx->g.ctx_row());
  return HVLA_OK;
}

// what an import refuses before it touches an arena: no theta, or tokens that do not go with the context's use_language_token
static int import_args(hvla_ctx* ctx, int K, const float* theta, const float* tok) {
  if (!theta) FAIL(ctx, HVLA_E_SHAPE, "null theta: the import needs the [%d, %d] parameter rows", K, ctx->lay.pl.G);
  if (ctx->lay.ll.on && !tok)
    FAIL(ctx, HVLA_E_SHAPE, "a use_language_token context imports with the episodes' token embeddings [%d, %d, %d]: none given", K,
         ctx->g.T, ctx->g.lang_dim);
  if (!ctx->lay.ll.on && tok) FAIL(ctx, HVLA_E_SHAPE, "token embeddings given to a context without use_language_token");
  return HVLA_OK;
}

// theta [K, G] (+ context, + tokens) into rows slots[k] (null: rows k) of w: import_theta_kernel, then the language prefix of those rows
static int import_body(hvla_ctx* ctx, hvla_weights* w, const int32_t* slots, int K, const float* theta, const float* context,
                       const float* tok, hipStream_t st) {
  const PolicyLayout& pl = ctx->lay.pl;
  ++ctx->prof.nlaunch;
  HIPCHK(ctx, launch_import_theta(theta, context, ctx->perm.as<int32_t>(), slots, w->wh.as<__bf16>(), w->wl.as<__bf16>(),
                                  w->vf.as<float>(), w->ctx.as<float>(), w->slot_count.as<int>(), pl.Gm, pl.Gv, pl.G, ctx->g.ctx_row(), K, w->B,
                                  st));
  return lang_prefix(ctx, w, tok, K, slots, st);
}

int hvla_weights_import(hvla_ctx* ctx, const float* theta, const float* context, const float* tok, int32_t B, hvla_weights** out,
                        void* stream) {
  if (ctx && out) *out = nullptr;
  hipStream_t st;
  if (int r = serve_entry(ctx, out != nullptr, arena_batch_of(B), true, stream, st)) return r;
  if (int r = import_args(ctx, B, theta, tok)) return r;
  std::unique_ptr<hvla_weights> w;
  if (int r = take_arena(ctx, B, w)) return r;
  HIPCHK(ctx, hipMemsetAsync(w->count.p, 0, 16, st));      // (the per-row counters are the kernel's)
  if (int r = import_body(ctx, w.get(), nullptr, B, theta, context, tok, st)) return r;
  *out = w.release();
  return HVLA_OK;
}

int hvla_weights_import_slots(hvla_ctx* ctx, hvla_weights* w, const int32_t* slots, int32_t K, const float* theta,
                              const float* context, const float* tok, void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, w != nullptr, slots_of(w, slots, K, false), true, stream, st)) return r;
  if (int r = import_args(ctx, K, theta, tok)) return r;
  if (int r = arena_fits(ctx, w, "destination")) return r;
  return import_body(ctx, w, slots, K, theta, context, tok, st);
}

int hvla_weights_copy_slots(hvla_ctx* ctx, hvla_weights* dst, const int32_t* dst_slots, const hvla_weights* src,
                            const int32_t* src_slots, int32_t K, void* stream) {
  hipStream_t st;
  if (int r = serve_entry(ctx, dst != nullptr && src != nullptr, slots_of(dst, dst_slots, K, false), true, stream, st)) return r;
  if (!src_slots) FAIL(ctx, HVLA_E_SHAPE, "null source slot map");
  if (K > src->B) FAIL(ctx, HVLA_E_SHAPE, "%d slots outside [1, %d] (the source arena has %d rows)", K, src->B, src->B);
  if (int r = arena_fits(ctx, dst, "destination")) return r;
  if (int r = arena_fits(ctx, src, "source")) return r;
  ++ctx->prof.nlaunch;
  HIPCHK(ctx, launch_copy_rows(src->wh.p, src->wl.p, src->vf.p, src->ctx.p, dst->wh.p, dst->wl.p, dst->vf.p, dst->ctx.p,
                               dst->slot_count.as<int>(), src_slots, dst_slots, dst->Gm, dst->Gv, dst->C, K, src->B, dst->B, st));
  return HVLA_OK;
}

// ------------------------------------------------------------------ post-processing of pool slots (include/hvla.h)
int hvla_post_create(hvla_ctx* ctx, int32_t B, hvla_post** out, void* stream) {
  if (!ctx || !out) return HVLA_E_STATE;
  *out = nullptr;
  const Geom& g = ctx->g;
  if (g.action_dim != HVLA_POST_DIM) FAIL(ctx, HVLA_E_SHAPE, "post-processing needs action_dim %d, the ctx has %d", HVLA_POST_DIM, g.action_dim);
  if (g.horizon < 1 || g.horizon > POST_MAX_HORIZON) FAIL(ctx, HVLA_E_SHAPE, "horizon %d outside [1, %d]", g.horizon, POST_MAX_HORIZON);
  if (B < 1 || B > ctx->cfg.max_batch) FAIL(ctx, HVLA_E_SHAPE, "%d post-processing slots outside [1, %d]", B, ctx->cfg.max_batch);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  std::unique_ptr<hvla_post> p(new hvla_post);
  p->B = B;
  p->H = g.horizon;
  HIPCHK(ctx, p->ring.alloc((size_t)B * g.horizon * g.horizon * HVLA_POST_DIM * sizeof(double)));
  HIPCHK(ctx, p->state.alloc((size_t)B * sizeof(PostSlot)));
  HIPCHK(ctx, hipMemsetAsync(p->ring.p, 0, p->ring.bytes, st));
  HIPCHK(ctx, hipMemsetAsync(p->state.p, 0, p->state.bytes, st));
  *out = p.release();
  return HVLA_OK;
}

int hvla_post_free(hvla_ctx* ctx, hvla_post* p) {
  if (!p) return HVLA_OK;
  if (ctx) (void)hipSetDevice(ctx->device);
  delete p;                                                  // hipFree waits for the device
  return HVLA_OK;
}

int hvla_post_assign(hvla_ctx* ctx, hvla_post* p, const int32_t* slots, int32_t K, const int32_t* rows, const uint8_t* ensemble,
                     void* stream) {
  if (!ctx || !p) return HVLA_E_STATE;
  if (!slots || !rows || !ensemble) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  if (K < 1 || K > p->B) FAIL(ctx, HVLA_E_SHAPE, "%d slots outside [1, %d]", K, p->B);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ++ctx->prof.nlaunch;
  HIPCHK(ctx, launch_post_assign(p->state.as<PostSlot>(), slots, K, p->B, rows, ensemble, reinterpret_cast<hipStream_t>(stream)));
  return HVLA_OK;
}

int hvla_post_step(hvla_ctx* ctx, hvla_post* p, const int32_t* slots, int32_t K, const float* actions, const hvla_post_row* table,
                   int32_t n_rows, double* raw_out, double* env_out, void* stream) {
  if (!ctx || !p) return HVLA_E_STATE;
  if (!slots || !actions || !table || !env_out) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  if (K < 1 || K > p->B) FAIL(ctx, HVLA_E_SHAPE, "%d slots outside [1, %d]", K, p->B);
  if (n_rows < 1) FAIL(ctx, HVLA_E_SHAPE, "empty post-processing table");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ++ctx->prof.nlaunch;
  HIPCHK(ctx, launch_post_step(actions, slots, K, p->B, p->H, p->ring.as<double>(), p->state.as<PostSlot>(), table, n_rows, raw_out,
                               env_out, reinterpret_cast<hipStream_t>(stream)));
  return HVLA_OK;
}

int hvla_loss(hvla_ctx* ctx, const float* actions, const float* logits, const float* target, const uint8_t* tmask,
              const uint8_t* amask, float* loss, int32_t B, void* stream) {
  if (!ctx) return HVLA_E_STATE;
  if (B < 1) FAIL(ctx, HVLA_E_SHAPE, "batch %d", B);
  if (!actions || !logits || !target || !tmask || !amask || !loss) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, launch_loss(actions, logits, target, tmask, amask, loss, B, ctx->g.horizon, ctx->g.action_dim,
                          ctx->g.max_action, ctx->g.clip_target != 0, reinterpret_cast<hipStream_t>(stream)));
  return HVLA_OK;
}

int hvla_loss_terms(hvla_ctx* ctx, const float* actions, const float* logits, const float* target, const uint8_t* tmask,
                    const uint8_t* amask, float* continuous, float* gripper, float* sqerr, int32_t B, void* stream) {
  if (!ctx) return HVLA_E_STATE;
  if (B < 1) FAIL(ctx, HVLA_E_SHAPE, "batch %d", B);
  if (!actions || !logits || !target || !tmask || !amask || !continuous || !gripper || !sqerr) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, launch_loss_terms(actions, logits, target, tmask, amask, continuous, gripper, sqerr, nullptr, B, ctx->g.horizon,
                                ctx->g.action_dim, ctx->g.max_action, ctx->g.clip_target != 0, reinterpret_cast<hipStream_t>(stream)));
  return HVLA_OK;
}

// the selection as an entry with this train_encoder value sees it: the position source is off unless the encoder is trained
static TrainOptions train_options(const hvla_ctx* ctx, bool train_encoder) {
  TrainOptions o = ctx->train.sel;
  if (!train_encoder) o.ps = PosSource();
  return o;
}

// the mask set by hvla_train_frozen must be the one of this call's train_encoder value and of the vector's present length (the
// position source may have changed since): checked before anything is launched, so that no kernel indexes it past its end
static int frozen_fits(hvla_ctx* ctx, bool train_encoder) {
  const TrainState& t = ctx->train;
  if (!t.sel.frozen) return HVLA_OK;
  const int64_t n = train_vector_elems(t.L, t.sel.ps, train_encoder);
  if (t.frozen_enc != train_encoder || t.frozen_n != n)
    FAIL(ctx, HVLA_E_STATE, "the frozen mask was set for train_encoder = %d and %lld elements, this call has train_encoder = %d and %lld: "
         "call hvla_train_frozen first", (int)t.frozen_enc, (long long)t.frozen_n, (int)train_encoder, (long long)n);
  return HVLA_OK;
}

// The head of every hvla_train_* entry, before it looks at its other arguments: the null checks (`args`: the entry's other
// must-not-be-null pointers), whether the training path serves the geometry at all, the device, the layout (built once per
// context) and, for the entries that read the frozen mask (frozen_for = their train_encoder value, else -1), that the mask fits.
static int train_entry(hvla_ctx* ctx, bool args = true, int frozen_for = -1) {
  if (!ctx || !args) return HVLA_E_STATE;
  TrainState& t = ctx->train;
  if (const char* why = train_refusal(ctx->g, t.language_tokens, t.differential, t.layer_tokens)) FAIL(ctx, HVLA_E_SHAPE, "%s", why);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (!t.have_layout) { t.L = make_train_layout(ctx->g); t.have_layout = true; }
  if (!t.L.policy_ok) FAIL(ctx, HVLA_E_STATE, "the generated policy has no leaf of a name the training path reads");
  if (ctx->g.layer_tokens && !t.tiles.p) {      // once per context: the tables do not depend on the batch
    std::vector<BGTile> host;
    (void)token_groups(ctx->g, t.L, nullptr, host);
    HIPCHK(ctx, t.tiles.alloc(host.size() * sizeof(BGTile)));
    HIPCHK(ctx, hipMemcpy(t.tiles.p, host.data(), host.size() * sizeof(BGTile), hipMemcpyHostToDevice));
    t.sel.groups = token_groups(ctx->g, t.L, t.tiles.as<BGTile>(), host);
  }
  return frozen_for < 0 ? HVLA_OK : frozen_fits(ctx, frozen_for != 0);
}

int hvla_train_sizes(hvla_ctx* ctx, int32_t B, int32_t train_encoder, int64_t out[4]) {
  if (int rc = train_entry(ctx, out != nullptr)) return rc;
  if (B < 1) FAIL(ctx, HVLA_E_SHAPE, "batch %d", B);
  const TrainLayout& L = ctx->train.L;
  out[0] = train_vector_elems(L, ctx->train.sel.ps, train_encoder != 0); out[1] = L.G;
  out[2] = (int64_t)train_workspace_floats(ctx->g, B, train_encoder != 0, ctx->train.sel.noise); out[3] = L.total;
  return HVLA_OK;
}

int hvla_train_context_rows(hvla_ctx* ctx, int32_t B, int32_t train_encoder, int64_t out[3]) {
  if (int rc = train_entry(ctx, out != nullptr)) return rc;
  if (B < 1) FAIL(ctx, HVLA_E_SHAPE, "batch %d", B);
  long o[3];
  train_context_rows(ctx->g, B, train_encoder != 0, ctx->train.sel.noise, o);
  out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
  return HVLA_OK;
}

static int position_args(hvla_ctx* ctx, const void* a, int32_t n, const void* w, const void* b) {
  if (!a || !w || !b) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  if (n < 2 || n > 1024) FAIL(ctx, HVLA_E_SHAPE, "source grid %d outside [2, 1024]", n);
  if (((uintptr_t)a | (uintptr_t)b) % 16 != 0) FAIL(ctx, HVLA_E_SHAPE, "tables must be 16-byte aligned");
  const int grid = ctx->g.image_size / ctx->g.patch;
  if (grid * grid != ctx->g.P() || ctx->g.E % 4 != 0) FAIL(ctx, HVLA_E_SHAPE, "the context's patch grid is not square");
  return HVLA_OK;
}

int hvla_position_interp(hvla_ctx* ctx, const float* src, int32_t n, const float* w, float* dst, void* stream) {
  if (!ctx) return HVLA_E_STATE;
  if (int rc = position_args(ctx, src, n, w, dst)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, launch_position_interp(src, n, w, dst, ctx->g.image_size / ctx->g.patch, ctx->g.E, reinterpret_cast<hipStream_t>(stream)));
  return HVLA_OK;
}

int hvla_position_interp_adjoint(hvla_ctx* ctx, const float* ddst, int32_t n, const float* w, float* dsrc, void* stream) {
  if (!ctx) return HVLA_E_STATE;
  if (int rc = position_args(ctx, ddst, n, w, dsrc)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, launch_position_adjoint(ddst, n, w, dsrc, ctx->g.image_size / ctx->g.patch, ctx->g.E, reinterpret_cast<hipStream_t>(stream)));
  return HVLA_OK;
}

int hvla_train_position_source(hvla_ctx* ctx, int32_t n, const float* w) {
  if (!ctx) return HVLA_E_STATE;
  if (n == 0) { ctx->train.sel.ps = PosSource(); return HVLA_OK; }
  if (int rc = train_entry(ctx)) return rc;
  if (!w) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  if (n < 2 || n > 1024) FAIL(ctx, HVLA_E_SHAPE, "source grid %d outside [2, 1024]", n);
  const TrainLayout& L = ctx->train.L;
  // the kernels move 16 bytes at a time: the slot and the tail must start on a multiple of 4 elements of the flat vector
  if ((L.total + L.e_pos) % 4 != 0 || (L.total + L.enc_total) % 4 != 0 || ctx->g.E % 4 != 0)
    FAIL(ctx, HVLA_E_SHAPE, "the position table is not 16-byte aligned in this geometry's training vector");
  ctx->train.sel.ps = PosSource{n, w, ctx->g.image_size / ctx->g.patch, ctx->g.E};
  return HVLA_OK;
}

int hvla_train_frozen(hvla_ctx* ctx, const uint8_t* frozen, int64_t n_params, int32_t frozen_buckets) {
  if (!ctx) return HVLA_E_STATE;
  TrainState& t = ctx->train;
  if (!frozen) { t.sel.frozen = nullptr; t.sel.frozen_buckets = 0; t.frozen_n = 0; t.frozen_enc = false; return HVLA_OK; }
  if (int rc = train_entry(ctx)) return rc;
  const int64_t n_hyper = t.L.total, n_enc = train_vector_elems(t.L, t.sel.ps, true);
  if (n_params != n_hyper && n_params != n_enc)
    FAIL(ctx, HVLA_E_SHAPE, "frozen mask of %lld elements: the training vector has %lld (frozen encoder) or %lld (trained encoder)",
         (long long)n_params, (long long)n_hyper, (long long)n_enc);
  const bool enc = n_params == n_enc;
  if (frozen_buckets & ~7) FAIL(ctx, HVLA_E_SHAPE, "frozen_buckets 0x%x: buckets are 0, 1, 2", (unsigned)frozen_buckets);
  if (enc && (frozen_buckets & 1)) FAIL(ctx, HVLA_E_SHAPE, "the whole image encoder frozen is train_encoder == 0");
  t.sel.frozen = frozen; t.sel.frozen_buckets = frozen_buckets; t.frozen_n = n_params; t.frozen_enc = enc;
  return HVLA_OK;
}

int hvla_train_attention_losses(hvla_ctx* ctx, const hvla_train_attention* opts) {
  if (!ctx) return HVLA_E_STATE;
  if (!opts) { ctx->train.sel.aux = AttnAux(); return HVLA_OK; }
  if (int rc = train_entry(ctx)) return rc;
  if (ctx->g.lang_in_policy) FAIL(ctx, HVLA_E_SHAPE, "the attention terms are not defined with use_language_token: the action row has T + P keys, the reference map P");
  if (ctx->g.differential && (opts->entropy_weight != 0.f || opts->alignment_weight != 0.f))
    FAIL(ctx, HVLA_E_SHAPE, "the attention terms are not defined with differential_attention: the module's map is the signed A1 - lambda A2, which has no entropy");
  if (opts->struct_size != sizeof(hvla_train_attention)) FAIL(ctx, HVLA_E_SHAPE, "hvla_train_attention.struct_size %u: this library's is %zu", opts->struct_size, sizeof(hvla_train_attention));
  const float we = opts->entropy_weight, wa = opts->alignment_weight;
  if (!std::isfinite(we) || !std::isfinite(wa) || we < 0.f || wa < 0.f) FAIL(ctx, HVLA_E_SHAPE, "attention loss weights (%g, %g) must be finite and >= 0", (double)we, (double)wa);
  if (wa > 0.f && !opts->reference_map) FAIL(ctx, HVLA_E_SHAPE, "alignment_weight %g > 0 needs reference_map [B, P]", (double)wa);
  ctx->train.sel.aux = AttnAux{we, wa, opts->reference_map, opts->entropy, opts->alignment};
  return HVLA_OK;
}

int hvla_train_language_tokens(hvla_ctx* ctx, int32_t on) {
  if (!ctx) return HVLA_E_STATE;
  if (on == 0) { ctx->train.language_tokens = false; return HVLA_OK; }
  if (on != 1) FAIL(ctx, HVLA_E_SHAPE, "hvla_train_language_tokens(%d): 0 or 1", on);
  if (!ctx->g.lang_in_policy) FAIL(ctx, HVLA_E_SHAPE, "hvla_train_language_tokens(1) on a context created without use_language_token");
  ctx->train.language_tokens = true;
  return HVLA_OK;
}

int hvla_train_differential(hvla_ctx* ctx, int32_t on) {
  if (!ctx) return HVLA_E_STATE;
  if (on == 0) { ctx->train.differential = false; return HVLA_OK; }
  if (on != 1) FAIL(ctx, HVLA_E_SHAPE, "hvla_train_differential(%d): 0 or 1", on);
  if (!ctx->g.differential) FAIL(ctx, HVLA_E_SHAPE, "hvla_train_differential(1) on a context created without differential_attention");
  ctx->train.differential = true;
  return HVLA_OK;
}

int hvla_train_layer_tokens(hvla_ctx* ctx, int32_t on) {
  if (!ctx) return HVLA_E_STATE;
  if (on == 0) { ctx->train.layer_tokens = false; return HVLA_OK; }
  if (on != 1) FAIL(ctx, HVLA_E_SHAPE, "hvla_train_layer_tokens(%d): 0 or 1", on);
  ctx->train.layer_tokens = ctx->g.layer_tokens != 0;      // on a context without layer tokens: HVLA_OK and nothing changes
  return HVLA_OK;
}

int hvla_train_noise_set(hvla_ctx* ctx, const hvla_train_noise* opts) {
  if (!ctx) return HVLA_E_STATE;
  if (!opts) { ctx->train.sel.noise = TrainNoise(); ctx->train.noise_set = false; return HVLA_OK; }
  if (int rc = train_entry(ctx)) return rc;
  if (opts->struct_size != sizeof(hvla_train_noise)) FAIL(ctx, HVLA_E_SHAPE, "hvla_train_noise.struct_size %u: this library's is %zu", opts->struct_size, sizeof(hvla_train_noise));
  const float rates[3] = {opts->policy_dropout, opts->context_dropout, opts->image_dropout};
  for (float r : rates)
    if (!std::isfinite(r) || r < 0.f || r >= 1.f) FAIL(ctx, HVLA_E_SHAPE, "dropout rate %g outside [0, 1)", (double)r);
  const float sg = opts->image_embedding_noise;
  if (!std::isfinite(sg) || sg < 0.f) FAIL(ctx, HVLA_E_SHAPE, "image_embedding_noise %g must be finite and >= 0", (double)sg);
  const Geom& g = ctx->g;      // one Philox block is four consecutive elements of a row (accept.h admits no other widths)
  if (g.differential && (rates[0] != 0.f || rates[1] != 0.f || rates[2] != 0.f || sg != 0.f))
    FAIL(ctx, HVLA_E_SHAPE, "hvla_train_noise with differential_attention is not built: the noise is restated for the other attention modules only");
  if (g.D % 4 != 0 || g.M % 4 != 0 || g.E % 4 != 0 || g.C % 4 != 0) FAIL(ctx, HVLA_E_SHAPE, "a noise site's width is no multiple of 4");
  TrainNoise nz;
  nz.policy_dropout = rates[0]; nz.sigma = sg; nz.context_dropout = rates[1]; nz.image_dropout = rates[2];
  nz.key.k0 = (uint32_t)opts->seed; nz.key.k1 = (uint32_t)(opts->seed >> 32);
  nz.key.draw = opts->draw; nz.key.sample0 = (long)opts->sample_offset;
  ctx->train.sel.noise = nz;
  ctx->train.noise_set = true;
  return HVLA_OK;
}

int hvla_train_noise_probe(hvla_ctx* ctx, uint32_t site, int64_t sample_id, int64_t n, float* out, void* stream) {
  if (int rc = train_entry(ctx)) return rc;
  if (!ctx->train.noise_set) FAIL(ctx, HVLA_E_STATE, "hvla_train_noise_probe without a hvla_train_noise_set setting");
  const uint32_t kind = site & 0xffu;
  if (kind < 1 || kind > 7) FAIL(ctx, HVLA_E_SHAPE, "site 0x%x: kinds are 1..7", site);
  if (!out || n < 1 || n > (1 << 24)) FAIL(ctx, HVLA_E_SHAPE, "n %lld outside [1, 2^24] or null out", (long long)n);
  const TrainNoise& nz = ctx->train.sel.noise;
  NoiseKey key = nz.key;
  key.site = site; key.sample0 = (long)sample_id;
  const float rate = kind <= NOISE_MLP_OUT ? nz.policy_dropout : kind == NOISE_CONTEXT ? nz.context_dropout : kind == NOISE_IMAGE_CLS ? nz.image_dropout : 0.f;
  HIPCHK(ctx, train_noise_probe(key, rate, kind == NOISE_TOKENS, n, out, reinterpret_cast<hipStream_t>(stream)));
  return HVLA_OK;
}

static TrainBuffers to_tb(const hvla_train_buffers* b) {
  return TrainBuffers{b->params, b->grads, reinterpret_cast<__bf16*>(b->mu), b->nu, b->ema, b->theta, b->dtheta, b->work,
                      b->loss, b->actions, b->logits, b->sqsum, b->wd_mask, b->params0};
}
static TrainHyper to_hp(const hvla_train_hyper* hy) {
  return TrainHyper{hy->lr, hy->b1, hy->b2, hy->eps, hy->weight_decay, hy->clip, hy->ema_decay, hy->step, hy->forward_only,
                    hy->base_lr, hy->base_weight_decay};
}

int hvla_train_step(hvla_ctx* ctx, const hvla_train_buffers* buf, const float* tok, const int64_t* mask, const float* cls,
                    const float* tokens, const uint8_t* images, const float* target, const uint8_t* tmask,
                    const uint8_t* amask, int32_t B, const hvla_train_hyper* hy, void* stream) {
  if (int rc = train_entry(ctx, buf && hy, images != nullptr)) return rc;
  if (B < 1) FAIL(ctx, HVLA_E_SHAPE, "batch %d", B);
  if (!buf->params || !buf->grads || !buf->theta || !buf->dtheta || !buf->work || !buf->loss || !tok || !mask || !cls ||
      !target || !tmask || !amask)
    FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  if ((tokens != nullptr) == (images != nullptr)) FAIL(ctx, HVLA_E_SHAPE, "pass exactly one of tokens (frozen encoder) / images (trained encoder)");
  if ((images != nullptr) != (hy->train_encoder != 0)) FAIL(ctx, HVLA_E_STATE, "hyper.train_encoder does not match the inputs");
  TrainState& t = ctx->train;
  if (!hy->forward_only && ((t.sel.noise.sigma > 0.f && tokens && (uintptr_t)tokens % 16 != 0) || (t.sel.noise.image_dropout > 0.f && (uintptr_t)cls % 16 != 0)))
    FAIL(ctx, HVLA_E_SHAPE, "under hvla_train_noise tokens and cls are read 16 bytes at a time: they must be 16-byte aligned");
  TrainInputs in{tok, mask, cls, tokens, images, target, tmask, amask};
  const TrainHyper hp = to_hp(hy);
  for (hipEvent_t& e : t.ev_bucket)
    if (!e) HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(ctx, train_step(ctx->g, t.L, to_tb(buf), in, B, hp, reinterpret_cast<hipStream_t>(stream), hp.forward_only ? nullptr : t.ev_bucket,
                         train_options(ctx, images != nullptr)));
  // ONE pending backward per ctx: the bucket events belong to the last hvla_train_step that ran a backward pass, and
  // hvla_train_wait_bucket refers to that step.  A forward-only step (evaluation between a step and its apply) records
  // nothing and leaves the pending step's events alone.
  if (!hp.forward_only) {
    t.bucket_recorded[0] = images != nullptr;
    t.bucket_recorded[1] = t.bucket_recorded[2] = true;
  }
  return HVLA_OK;
}

int hvla_train_bucket_ranges(hvla_ctx* ctx, int32_t train_encoder, int64_t out[6]) {
  if (int rc = train_entry(ctx, out != nullptr)) return rc;
  const TrainLayout& L = ctx->train.L;
  out[0] = L.total; out[1] = train_vector_elems(L, ctx->train.sel.ps, train_encoder != 0) - L.total;     // the shared DINOv2 leaves (+ the position source)
  out[2] = L.wcat; out[3] = L.total - L.wcat;                     // the output heads (W_cat, b_cat)
  out[4] = 0; out[5] = L.wcat;                                    // the context encoder
  return HVLA_OK;
}

int hvla_train_wait_bucket(hvla_ctx* ctx, int32_t bucket, void* stream) {
  if (!ctx) return HVLA_E_STATE;
  if (bucket < 0 || bucket > 2) FAIL(ctx, HVLA_E_SHAPE, "bucket %d outside [0, 2]", bucket);
  if (!ctx->train.bucket_recorded[bucket]) FAIL(ctx, HVLA_E_STATE, "bucket %d was not produced by the last hvla_train_step", bucket);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), ctx->train.ev_bucket[bucket], 0));
  return HVLA_OK;
}

int hvla_train_profile(hvla_ctx* ctx, int32_t on) {
  if (!ctx) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const bool first = on && !ctx->train.timer;
  train_gemm_timer(on != 0, first);
  if (on) ctx->train.timer = true;
  return HVLA_OK;
}

int hvla_train_profile_read(hvla_ctx* ctx, float* gemm_ms, double* gemm_flops, int32_t* launches) {
  if (!ctx || !gemm_ms || !gemm_flops || !launches) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int n = 0;
  HIPCHK(ctx, train_gemm_timer_read(gemm_ms, gemm_flops, &n));
  *launches = n;
  return HVLA_OK;
}

int hvla_train_apply(hvla_ctx* ctx, const hvla_train_buffers* buf, const hvla_train_hyper* hy, void* stream) {
  if (int rc = train_entry(ctx, buf && hy, hy && hy->train_encoder != 0)) return rc;
  if (!buf->params || !buf->grads || !buf->mu || !buf->nu || !buf->sqsum) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  HIPCHK(ctx, train_apply(ctx->train.L, to_tb(buf), to_hp(hy), hy->train_encoder != 0, reinterpret_cast<hipStream_t>(stream),
                          train_options(ctx, hy->train_encoder != 0)));
  return HVLA_OK;
}

int hvla_train_accumulate(hvla_ctx* ctx, const hvla_train_buffers* buf, float* acc, float inv_k, const hvla_train_hyper* hy,
                          void* stream) {
  if (int rc = train_entry(ctx, buf && hy, hy && hy->train_encoder != 0)) return rc;
  if (!buf->grads || !buf->sqsum || !acc) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  HIPCHK(ctx, train_accumulate(ctx->train.L, to_tb(buf), acc, inv_k, to_hp(hy), hy->train_encoder != 0, reinterpret_cast<hipStream_t>(stream),
                               train_options(ctx, hy->train_encoder != 0)));
  return HVLA_OK;
}

int hvla_train_metrics(hvla_ctx* ctx, const hvla_train_buffers* buf, const hvla_train_metrics_in* in, float* out, int32_t B,
                       int32_t train_encoder, void* stream) {
  if (int rc = train_entry(ctx, buf && in, train_encoder != 0)) return rc;
  if (in->struct_size != sizeof(hvla_train_metrics_in))
    FAIL(ctx, HVLA_E_SHAPE, "hvla_train_metrics_in.struct_size %u: this library's is %zu", in->struct_size, sizeof(hvla_train_metrics_in));
  if (!in->scratch || !out) FAIL(ctx, HVLA_E_SHAPE, "null scratch or out");
  if (!buf->params || !buf->grads) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  if (B < 1 || B > HVLA_TRAIN_METRICS_MAX_BATCH) FAIL(ctx, HVLA_E_SHAPE, "batch %d outside [1, %d]", B, HVLA_TRAIN_METRICS_MAX_BATCH);
  if (!(in->select & (HVLA_METRICS_PRE | HVLA_METRICS_UPDATE)) || (in->select & ~(HVLA_METRICS_PRE | HVLA_METRICS_UPDATE)))
    FAIL(ctx, HVLA_E_SHAPE, "select 0x%x: HVLA_METRICS_PRE | HVLA_METRICS_UPDATE", in->select);
  if ((in->select & HVLA_METRICS_UPDATE) && !in->prev_params) FAIL(ctx, HVLA_E_SHAPE, "HVLA_METRICS_UPDATE needs prev_params");
  if (in->n_tasks < 0) FAIL(ctx, HVLA_E_SHAPE, "n_tasks %d", in->n_tasks);
  if (in->task_ids && in->n_tasks == 0) FAIL(ctx, HVLA_E_SHAPE, "task_ids given with n_tasks == 0");
  if ((uintptr_t)in->scratch % 16 != 0) FAIL(ctx, HVLA_E_SHAPE, "scratch must be 16-byte aligned");
  HIPCHK(ctx, train_metrics(ctx->g, ctx->train.L, to_tb(buf), *in, out, B, train_encoder != 0, reinterpret_cast<hipStream_t>(stream),
                            train_options(ctx, train_encoder != 0)));
  return HVLA_OK;
}

int hvla_train_publish(hvla_ctx* ctx, const float* params, int64_t n_params, int32_t train_encoder, void* stream) {
  if (int rc = train_entry(ctx)) return rc;
  if (!ctx->loaded) FAIL(ctx, HVLA_E_STATE, "hvla_train_publish before hvla_load_weights");
  if (!params) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  const Geom& g = ctx->g;
  const TrainLayout& L = ctx->train.L;
  const PosSource ps = train_options(ctx, train_encoder != 0).ps;
  const int64_t want = train_vector_elems(L, ps, train_encoder != 0);
  if (n_params != want) FAIL(ctx, HVLA_E_SHAPE, "n_params %lld, the training vector has %lld", (long long)n_params, (long long)want);
  if (ps.n > 0 && (serving::enc_map(g, L).f_pos % 4 != 0 || (uintptr_t)params % 16 != 0))
    FAIL(ctx, HVLA_E_SHAPE, "the position table is not 16-byte aligned");
  // (the transposing kernel's whole 64 x 64 tiles: hvla_create admits encoder widths in multiples of 128 only)
  const PolicyLayout& pl = ctx->lay.pl;
  const int Gtot = pl.Gm + pl.Gv;
  PublishArgs a{g, params, ctx->hn_f32.as<float>(), ctx->perm.as<int32_t>(), ctx->wcat_hi.as<uint16_t>(), ctx->wcat_lo.as<uint16_t>(),
                ctx->bcat.as<float>(), Gtot, ctx->enc16.as<uint16_t>(), ctx->encd16.as<uint16_t>(), ctx->encf32.as<float>(),
                ctx->cfg.enc_dtype == HVLA_ENC_BF16, train_encoder != 0};
  if (g.layer_tokens) {
    a.pos_head = ctx->pos_head.as<int32_t>(); a.pos_token = ctx->pos_token.as<int32_t>();
    a.seg_tile = ctx->seg_tile.as<int32_t>(); a.seg_token = ctx->seg_token.as<int32_t>(); a.nseg = ctx->nseg;
  }
  ctx->prof.nlaunch += train_encoder ? 6 : 2;
  HIPCHK(ctx, launch_publish(a, reinterpret_cast<hipStream_t>(stream)));
  if (ps.n > 0) {      // the served table is the resize of the vector's SOURCE table, by the kernel the step resizes with
    ctx->prof.nlaunch += 2;
    HIPCHK(ctx, launch_position_serve(params + L.total + L.enc_total, ps.n, ps.w, params + L.total + L.e_cls,
                                      ctx->encf32.as<float>() + serving::enc_map(g, L).f_pos, ps.grid, ps.E, reinterpret_cast<hipStream_t>(stream)));
  }
  return HVLA_OK;
}

int hvla_preprocess(hvla_ctx* ctx, const uint8_t* frames, int32_t B, int32_t H, int32_t W, int32_t flags, uint8_t* images,
                    void* stream) {
  if (!ctx) return HVLA_E_STATE;
  if (B < 1 || H < 2 || W < 2 || H > 8192 || W > 8192) FAIL(ctx, HVLA_E_SHAPE, "frames [%d, %d, %d, 3]", B, H, W);
  if (!frames || !images) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  if (flags & ~3) FAIL(ctx, HVLA_E_SHAPE, "flags %d (1 = crop, 2 = padded resize)", flags);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int S = ctx->g.image_size;
  const bool crop = flags & HVLA_PREPROCESS_CROP, pad = flags & HVLA_PREPROCESS_PAD;
  const int LH = pad ? 256 : H, LW = pad ? 320 : W;           // what the lanczos3 stage sees (hypervla_interface.py:90-95)
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (LH != ctx->rs_H || LW != ctx->rs_W) {                    // new source shape: rebuild the span tables
    std::vector<int> rs, rc, cs, cc;
    std::vector<float> rw, cw;
    build_resize_spans(LH, S, rs, rc, rw, ctx->rs_row_span);
    build_resize_spans(LW, S, cs, cc, cw, ctx->rs_col_span);
    std::vector<float> host;                                    // [row start | row count | col start | col count] as ints, then weights
    host.resize((size_t)4 * S + rw.size() + cw.size());
    memcpy(host.data(), rs.data(), (size_t)S * 4); memcpy(host.data() + S, rc.data(), (size_t)S * 4);
    memcpy(host.data() + 2 * S, cs.data(), (size_t)S * 4); memcpy(host.data() + 3 * S, cc.data(), (size_t)S * 4);
    memcpy(host.data() + 4 * S, rw.data(), rw.size() * 4); memcpy(host.data() + 4 * S + rw.size(), cw.data(), cw.size() * 4);
    HIPCHK(ctx, hipStreamSynchronize(st));                      // a previous call may still read the old tables
    HIPCHK(ctx, ctx->rs_tab.alloc(host.size() * 4));
    HIPCHK(ctx, hipMemcpy(ctx->rs_tab.p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    ctx->rs_H = LH; ctx->rs_W = LW;
  }
  const size_t need_rows = (size_t)B * S * LW * 3 * 4, need_img = (size_t)B * S * S * 3 * 4;
  const size_t need_pad = pad ? (size_t)B * LH * LW * 3 * 4 : 0;
  if (ctx->rs_rows.bytes < need_rows || ctx->rs_img.bytes < need_img || ctx->rs_pad.bytes < need_pad) {
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (ctx->rs_rows.bytes < need_rows) HIPCHK(ctx, ctx->rs_rows.alloc(need_rows));
    if (ctx->rs_img.bytes < need_img) HIPCHK(ctx, ctx->rs_img.alloc(need_img));
    if (ctx->rs_pad.bytes < need_pad) HIPCHK(ctx, ctx->rs_pad.alloc(need_pad));
  }
  const int* ti = ctx->rs_tab.as<int>();
  const float* tw = ctx->rs_tab.as<float>() + 4 * S;
  HIPCHK(ctx, launch_resize(frames, images, ctx->rs_rows.as<float>(), ctx->rs_img.as<float>(), ti, ti + S, tw,
                            ctx->rs_row_span, ti + 2 * S, ti + 3 * S, tw + (size_t)S * ctx->rs_row_span, ctx->rs_col_span, B, LH,
                            LW, S, crop, st, pad ? ctx->rs_pad.as<float>() : nullptr, H, W));
  return HVLA_OK;
}

// bucket of relative position rel = key - query, bidirectional (transformers `_relative_position_bucket`; the log is
// evaluated in float32 as both the torch and the flax model do)
static int t5_bucket(int rel, int buckets, int max_distance) {
  const int nb = buckets / 2, max_exact = nb / 2;
  int out = rel > 0 ? nb : 0;
  const int n = rel < 0 ? -rel : rel;
  if (n < max_exact) return out + n;
  const float v = logf((float)n / (float)max_exact) / (float)log((double)max_distance / (double)max_exact) * (float)(nb - max_exact);
  int large = max_exact + (int)v;
  if (large > nb - 1) large = nb - 1;
  return out + large;
}

int hvla_t5_load(hvla_ctx* ctx, const hvla_t5_config* c, const hvla_tensor_desc* t, int32_t n) {
  if (!ctx || !c) return HVLA_E_STATE;
  if (c->layers < 1 || c->layers > 24 || c->heads < 1 || c->d_model < 1 || c->d_kv < 1 || c->d_ff < 1 || c->vocab < 1 ||
      c->buckets < 4 || c->buckets % 2 || c->max_tokens < 1 || c->max_batch < 1)
    FAIL(ctx, HVLA_E_SHAPE, "bad T5 configuration");
  if (c->d_model != ctx->g.lang_dim) FAIL(ctx, HVLA_E_SHAPE, "T5 d_model %d != lang_dim %d of the hypernetwork", c->d_model, ctx->g.lang_dim);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::map<std::string, const hvla_tensor_desc*> m;
  for (int i = 0; i < n; ++i) {
    if (!t[i].name || !t[i].data) FAIL(ctx, HVLA_E_WEIGHTS, "tensor %d has null name/data", i);
    std::string nm = t[i].name;
    if (nm.rfind("hf_model/", 0) == 0) nm = nm.substr(9);          // the reference nests the HF module under `hf_model`
    m[nm] = &t[i];
  }
  const int D = c->d_model, I = c->heads * c->d_kv, F = c->d_ff, TM = c->max_tokens;
  std::vector<float> host;
  std::vector<std::pair<const float**, size_t>> fix;
  std::string bad;
  auto push = [&](const float** slot, const std::string& name, int64_t numel) {
    auto it = m.find(name);
    if (it == m.end() || it->second->numel != numel) {
      if (bad.empty()) bad = name + (it == m.end() ? " (absent)" : " (wrong size)");
      return;
    }
    const size_t off = (host.size() + 3) / 4 * 4;
    host.resize(off + numel);
    memcpy(host.data() + off, it->second->data, (size_t)numel * 4);
    fix.emplace_back(slot, off);
  };
  T5Weights w{};
  w.max_tokens = TM;
  push(&w.shared, "shared/embedding", (int64_t)c->vocab * D);
  push(&w.final_ln, "encoder/final_layer_norm/weight", D);
  for (int l = 0; l < c->layers; ++l) {
    const std::string b = "encoder/block/" + std::to_string(l) + "/layer/";
    T5LayerW& L = w.layer[l];
    push(&L.ln0, b + "0/layer_norm/weight", D);
    push(&L.wq, b + "0/SelfAttention/q/kernel", (int64_t)D * I);
    push(&L.wk, b + "0/SelfAttention/k/kernel", (int64_t)D * I);
    push(&L.wv, b + "0/SelfAttention/v/kernel", (int64_t)D * I);
    push(&L.wo, b + "0/SelfAttention/o/kernel", (int64_t)I * D);
    push(&L.ln1, b + "1/layer_norm/weight", D);
    push(&L.wi, b + "1/DenseReluDense/wi/kernel", (int64_t)D * F);
    push(&L.wo2, b + "1/DenseReluDense/wo/kernel", (int64_t)F * D);
  }
  // relative-position bias table [heads][2 TM - 1] from the first block's bucket embedding [buckets][heads]
  {
    auto it = m.find("encoder/block/0/layer/0/SelfAttention/relative_attention_bias/embedding");
    if (it == m.end() || it->second->numel != (int64_t)c->buckets * c->heads) {
      if (bad.empty()) bad = "encoder/block/0/layer/0/SelfAttention/relative_attention_bias/embedding";
    } else {
      const float* emb = it->second->data;
      const size_t off = (host.size() + 3) / 4 * 4;
      host.resize(off + (size_t)c->heads * (2 * TM - 1));
      for (int h = 0; h < c->heads; ++h)
        for (int r = -(TM - 1); r <= TM - 1; ++r)
          host[off + (size_t)h * (2 * TM - 1) + (r + TM - 1)] = emb[(size_t)t5_bucket(r, c->buckets, c->max_distance) * c->heads + h];
      fix.emplace_back(&w.relbias, off);
    }
  }
  if (!bad.empty()) FAIL(ctx, HVLA_E_WEIGHTS, "T5 tensor %s", bad.c_str());
  HIPCHK(ctx, ctx->t5_f32.alloc(host.size() * 4));
  HIPCHK(ctx, hipMemcpy(ctx->t5_f32.p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
  for (auto& f : fix) *f.first = ctx->t5_f32.as<float>() + f.second;
  ctx->t5d = T5Dims{c->vocab, D, c->d_kv, c->heads, F, c->layers, c->buckets, c->max_distance, c->eps};
  ctx->t5w = w;
  ctx->t5_max_batch = c->max_batch;
  HIPCHK(ctx, ctx->t5_work.alloc(t5_workspace_floats(ctx->t5d, c->max_batch, TM) * 4));
  ctx->t5_loaded = true;
  return HVLA_OK;
}

int hvla_t5_encode(hvla_ctx* ctx, const int64_t* input_ids, const int64_t* attention_mask, float* token_embedding, int32_t B,
                   int32_t T, void* stream) {
  if (!ctx) return HVLA_E_STATE;
  if (!ctx->t5_loaded) FAIL(ctx, HVLA_E_STATE, "hvla_t5_load has not been called");
  if (B < 1 || B > ctx->t5_max_batch || T < 1 || T > ctx->t5w.max_tokens)
    FAIL(ctx, HVLA_E_SHAPE, "batch %d / tokens %d outside [1, %d] x [1, %d]", B, T, ctx->t5_max_batch, ctx->t5w.max_tokens);
  if (!input_ids || !attention_mask || !token_embedding) FAIL(ctx, HVLA_E_SHAPE, "null pointer");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, t5_encode(ctx->t5d, ctx->t5w, ctx->t5_work.as<float>(), input_ids, attention_mask, token_embedding, B, T,
                        reinterpret_cast<hipStream_t>(stream)));
  return HVLA_OK;
}

int hvla_profile(hvla_ctx* ctx, int32_t mode) {
  if (!ctx) return HVLA_E_STATE;
  if (mode < 0 || mode > 2) FAIL(ctx, HVLA_E_SHAPE, "profile mode %d", mode);
  ctx->prof.mode = mode;
  return HVLA_OK;
}

int hvla_profile_select(hvla_ctx* ctx, uint32_t category_mask) {
  if (!ctx) return HVLA_E_STATE;
  if (category_mask == 0 || (category_mask >> HVLA_PROF_N) != 0) FAIL(ctx, HVLA_E_SHAPE, "profile category mask 0x%x", category_mask);
  ctx->prof.select = category_mask;
  return HVLA_OK;
}

int hvla_profile_read(hvla_ctx* ctx, float* ms, int32_t* launches) {
  if (!ctx || !ms || !launches) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (int i = 0; i < HVLA_PROF_N; ++i) ms[i] = 0.f, launches[i] = 0;
  Profiler& p = ctx->prof;
  for (size_t i = 0; i < p.used; ++i) {
    HIPCHK(ctx, hipEventSynchronize(p.stop[i]));
    float t = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&t, p.start[i], p.stop[i]));
    ms[p.cat[i]] += t;
    launches[p.cat[i]] += 1;
  }
  p.used = 0;
  return HVLA_OK;
}

#ifdef HVLA_BENCH_HOOKS
// diagnostics (libhvla_bench.so only; not part of include/hvla.h): one encoder GEMM shape on the ctx's workspace
int hvla_debug_gemm(hvla_ctx* ctx, int M, int N, int K, int epi, int variant, int iters, float* ms) {
  if (!ctx || !ctx->loaded) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const void* A = ctx->ws[K > ctx->g.E ? WS_G : WS_H].p;
  void* out = ctx->ws[epi == 3 ? WS_X : (epi == 1 ? WS_QKV : WS_G)].p;
  if (epi == 2 && K > ctx->g.E) return HVLA_E_SHAPE;
  const EncLayerW& L = ctx->encw.layer[0];
  const void* W = epi == 1 ? L.wqkv : (epi == 2 ? L.w1 : (K > ctx->g.E ? L.w2 : L.wo));
  const float* bias = epi == 1 ? L.bqkv : (epi == 2 ? L.b1 : L.b2);
  HIPCHK(ctx, debug_gemm(A, W, bias, L.ls1, out, M, N, K, epi, variant, iters, ms, nullptr));
  return HVLA_OK;
}

// diagnostics (not part of include/hvla.h): time one shape of the fine-tune path's batched GEMM on caller buffers
int hvla_debug_bgemm(const float* A, const float* B, float* C, int M, int N, int K, int ta, int tb, int nb, int accumulate,
                     int iters, float* ms) {
  const int lda = ta ? M : K, ldb = tb ? K : N;
  BG g{A, B, C, nullptr, M, N, K, lda, ldb, N, (long)M * K, 0, (long)N * K, 0, (long)M * N, 0, 0, 1, 1.f, accumulate, 1, accumulate != 0};
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  for (int i = 0; i < 3; ++i) bgemm(nullptr, ta != 0, tb != 0, g, nb);
  (void)hipEventRecord(e0, nullptr);
  for (int i = 0; i < iters; ++i) bgemm(nullptr, ta != 0, tb != 0, g, nb);
  (void)hipEventRecord(e1, nullptr);
  (void)hipEventSynchronize(e1);
  (void)hipEventElapsedTime(ms, e0, e1);
  *ms /= iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return hipGetLastError() == hipSuccess ? HVLA_OK : HVLA_E_HIP;
}

// ONE launch of the fine-tune path's batched GEMM with every field of the descriptor in the caller's hands (tools/bgemm_check.py,
// tests/test_gpu_train_gemm.py): a plain-C mirror of BG (train.h) plus the operand orders and the outer batch count.  Null stream,
// synchronised; returns the HIP status (0 = hipSuccess).  chosen[4] = what bgemm_launch selected: tile rows (64 / 128 / 256), float4
// staging, the effective ksplit, and 1 for bgemm_kernel (hvla_debug_train_gemm_exact).
struct hvla_bgemm_desc {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  int32_t M, N, K, lda, ldb, ldc;
  int64_t sA0, sA1, sB0, sB1, sC0, sC1, sBias0, sBias1;
  int32_t nb1;
  float alpha;
  int32_t accumulate, ksplit, allow_split, a_padded;
  int32_t ta, tb, nb0;
};
int hvla_debug_bgemm_once(const hvla_bgemm_desc* d, int32_t* chosen) {
  if (!d || !chosen || d->nb0 < 1 || d->nb1 < 1 || d->ksplit < 1 || d->M < 1 || d->N < 1 || d->K < 1) return (int)hipErrorInvalidValue;
  BG g{d->A, d->B, d->C, d->bias, d->M, d->N, d->K, d->lda, d->ldb, d->ldc, (long)d->sA0, (long)d->sA1, (long)d->sB0, (long)d->sB1,
       (long)d->sC0, (long)d->sC1, (long)d->sBias0, d->nb1, d->alpha, d->accumulate, d->ksplit, d->allow_split, d->a_padded, (long)d->sBias1};
  (void)hipGetLastError();
  bgemm(nullptr, d->ta != 0, d->tb != 0, g, d->nb0);
  hipError_t e = hipGetLastError();
  const hipError_t s = hipDeviceSynchronize();
  if (e == hipSuccess) e = s;
  const BgemmChoice& c = last_bgemm_choice();
  chosen[0] = c.tile, chosen[1] = c.vec, chosen[2] = c.ksplit, chosen[3] = c.exact;
  return (int)e;
}

// phase time stamps of attention_kernel for workgroups `wgs[i]` (8 stamps each), on the ctx's workspace (contents irrelevant)
int hvla_debug_attention_stamps(hvla_ctx* ctx, int32_t B, const int32_t* wgs, int32_t nwg, unsigned long long* out) {
  if (!ctx || !out || !wgs) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const Geom& g = ctx->g;
  DevBuf st;
  HIPCHK(ctx, st.alloc((size_t)8 * 8));
  for (int i = 0; i < nwg; ++i) {
    HIPCHK(ctx, hipMemset(st.p, 0, 64));
    for (int rep = 0; rep < 2; ++rep)
      HIPCHK(ctx, debug_attention_stamps(ctx->ws[WS_QKV].p, ctx->ws[WS_H].p, ctx->ws[WS_ABAR].p, B, g.S(), g.E, g.enc_heads, wgs[i], st.as<unsigned long long>(), nullptr));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(out + (size_t)i * 8, st.p, 64, hipMemcpyDeviceToHost));
  }
  return HVLA_OK;
}

// phase time stamps of the policy kernel (episode 0, wave 0; shader clock): 27 values at the README geometry, policy.hip HVLA_STAMP
int hvla_debug_policy_stamps(hvla_ctx* ctx, const hvla_weights* w, const float* tokens, float* actions, float* logits, int32_t B,
                             unsigned long long* out, int32_t n) {
  if (!ctx || !w || !out) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const Geom& g = ctx->g;
  const PolicyLayout& pl = ctx->lay.pl;
  DevBuf st;
  HIPCHK(ctx, st.alloc((size_t)n * 8));
  HIPCHK(ctx, hipMemset(st.p, 0, (size_t)n * 8));
  PolicyParams p{pl, w->wh.as<__bf16>(), w->wl.as<__bf16>(), w->vf.as<float>(), tokens, actions, logits,
                 B, g.E, g.P(), g.L, g.M, g.horizon, g.action_dim, g.tanh_scale, g.max_action};
  p.stamps = st.as<unsigned long long>();
  for (int i = 0; i < 3; ++i) HIPCHK(ctx, launch_policy(p, nullptr, 0, nullptr, 0, false, g.differential != 0));   // (a differential context's layout is its flavour's alone)
  HIPCHK(ctx, hipDeviceSynchronize());
  HIPCHK(ctx, hipMemcpy(out, st.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return HVLA_OK;
}

// the fine-tune GEMM on the exact-f32 matrix instruction (bitwise fmaf chains) instead of split-bf16: a debugging aid for
// gradient comparisons, so it is a call in the bench library and not an environment switch of the product
int hvla_debug_train_gemm_exact(int on) {
  set_train_gemm_exact(on != 0);
  return HVLA_OK;
}
// shader-clock stamps of the last context-encoder launch (workgroup 0): see hypernet.hip CTX_STAMP
int hvla_debug_ctx_stamps(unsigned long long* out) { return debug_ctx_stamps(out) == hipSuccess ? HVLA_OK : HVLA_E_HIP; }
// device pointer and size of one encoder workspace buffer (tools/ read intermediates back with hipMemcpy):
// `which` is plan.h's WsBuf: 0 x (f32 residual stream), 1 h (16-bit LayerNorm / attention output), 2 qkv, 3 g (MLP hidden), 4 corr,
// 5 abar, 6 ln_cnt, 7 ln_part
int hvla_debug_workspace(hvla_ctx* ctx, int which, void** ptr, size_t* bytes) {
  if (!ctx || !ptr || !bytes) return HVLA_E_STATE;
  if (which < 0 || which >= NUM_WS) return HVLA_E_SHAPE;
  *ptr = ctx->ws[which].p;
  *bytes = ctx->ws[which].bytes;
  return HVLA_OK;
}
int hvla_debug_lnx_stats(hvla_ctx* ctx, unsigned long long* out, int reset) {
  if (!ctx) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, debug_lnx_stats(out, reset));
  return HVLA_OK;
}
// hvla_encode then returns behind its n-th dense product (QKV, out, fc1, fc2 of layer 0 = 1 .. 4, ...; 0 = the whole encoder): the
// workspace is read back (hvla_debug_workspace) as that product's consumers would find it -- tests of the mean rows and the corr table
int hvla_debug_encode_stop(hvla_ctx* ctx, int32_t n) {
  if (!ctx || n < 0) return HVLA_E_STATE;
  ctx->enc_stop = n;
  return HVLA_OK;
}
// how long a column tile of a residual GEMM waits for the image's other tiles (ticks of 10 ns; the product's value is 800).  0 = nobody
// waits: every tile but an image's last arriver is normalised from memory -- the test that the two routes give the same bytes
int hvla_debug_lnx_spin(hvla_ctx* ctx, uint32_t ticks) {
  if (!ctx) return HVLA_E_STATE;
  ctx->ln_spin = ticks;
  return HVLA_OK;
}
#endif  // HVLA_BENCH_HOOKS

int64_t hvla_launches(hvla_ctx* ctx) {
  if (!ctx) return 0;
  const int64_t n = (int64_t)ctx->prof.nlaunch;
  ctx->prof.nlaunch = 0;
  return n;
}

int hvla_box_probe(hvla_ctx* ctx, float out[3], void* stream) {
  if (!ctx || !out) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf sink, ticks;
  int ncu = 256;
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device);
  if (sink.alloc((size_t)ncu * 512 * sizeof(float)) != hipSuccess || ticks.alloc(64) != hipSuccess) FAIL(ctx, HVLA_E_ARENA_FULL, "box probe buffers");
  HIPCHK(ctx, run_box_probe(sink.as<float>(), ticks.as<unsigned long long>(), out, reinterpret_cast<hipStream_t>(stream)));
  return HVLA_OK;
}

int hvla_selftest(hvla_ctx* ctx, void* stream) {
  if (!ctx) return HVLA_E_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(ctx, hipMemsetAsync(ctx->flags.p, 0, 64 * sizeof(int), st));
  HIPCHK(ctx, launch_selftest(ctx->flags.as<int>(), st));
  int h[64];
  HIPCHK(ctx, hipMemcpyAsync(h, ctx->flags.p, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (int i = 0; i < 8; ++i)
    if (h[i]) FAIL(ctx, HVLA_E_STATE, "MFMA layout probe %d failed (%d mismatches)", i, h[i]);
  return HVLA_OK;
}

}  // extern "C"
