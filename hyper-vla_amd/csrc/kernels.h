// kernels.h — parameter blocks + launchers shared between the kernel files and api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/hvla.h"
#include "accept.h"
#include "layout.h"

namespace hvla {

// ---------------------------------------------------------------- hypernetwork
struct CtxLayer {
  const float *ln0_s, *ln0_b, *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo, *ln1_s, *ln1_b, *w1, *b1, *w2, *b2;
};
struct CtxParams {
  int T, C, F, heads, layers, lang_dim, E, scale_context;
  int big_elems;             // floats in the kernel's third LDS buffer (set by launch_ctx_encoder)
  const float* tok;          // [B, T, lang_dim]
  const int64_t* attn_mask;  // [B, T]
  const float* cls;          // [B, E]
  const float *w_tok, *b_tok, *w_img, *b_img, *pos_tok, *pos_img, *pos_layer, *norm_s, *norm_b;
  CtxLayer layer[CTX_MAX_LAYERS];
  float* ctx;                // [B, C]
  __bf16 *ctx_hi, *ctx_lo;   // [B, C]
};
// share_layer_index=False (ctx_encoder_kernel_tokens): NL layer tokens, T + 1 + NL <= CTX_MAX_ROWS rows; of `enc`, pos_layer is then
// [NL, C], ctx [B, NL, C] and ctx_hi / ctx_lo token-major [NL, B, C].  (A struct of its own: ctx_encoder_kernel's arguments stay as they are.)
struct CtxTokensParams {
  CtxParams enc;
  int NL;
};
struct WeightGenParams {
  const __bf16 *wcat_hi, *wcat_lo;   // [ntiles][KS][64 lanes][8]
  const float* bcat;                 // [Gm + Gv]
  const __bf16 *ctx_hi, *ctx_lo;     // [B, C]
  __bf16 *wh, *wl;                   // [B, Gm]
  float* vf;                         // [B, Gv]
  int B, Gm, Gv, ntiles;
};
// share_layer_index=False (pack.h TokenSegments): gen.wcat_hi / wcat_lo are the segments' fragment blocks [nseg][KS][64 lanes][8],
// gen.ctx_hi / ctx_lo the token-major planes [NL][B][C]
struct WeightGenTokensParams {
  WeightGenParams gen;
  const int32_t* seg_token;          // [nseg] the layer token of a segment
  const int32_t* tile_segs;          // [ntiles][2] first segment, count
};
hipError_t launch_ctx_encoder(const CtxParams& p, int B, hipStream_t st, int NL = 0);     // NL > 0: ctx_encoder_kernel_tokens
hipError_t launch_weightgen_tokens(const WeightGenTokensParams& q, int C, hipStream_t st, const int32_t* slot = nullptr, int rows = 0);
// (ctx_encoder_lds_bytes, the dynamic LDS of ctx_encoder_kernel for a geometry -- <= 160 KiB or refused at create -- is accept.h's)
// episode pool, `slot` not null: weightgen_kernel's output row of input episode r is arena row slot[r] of an arena of
// `rows`; launch_pool_assign puts the K new context rows (f32 workspace rows 0 .. K-1) at arena rows slot[k] and zeroes those rows'
// ensemble counters.  Slot entries outside [0, rows) are skipped by both.
hipError_t launch_weightgen(const WeightGenParams& p, int C, hipStream_t st, const int32_t* slot = nullptr, int rows = 0);
hipError_t launch_pool_assign(const float* ctx_rows, float* ctx, int* count, const int32_t* slot, int K, int C, int rows,
                              hipStream_t st);
hipError_t launch_export_theta(const __bf16* wh, const __bf16* wl, const float* vf, const int32_t* perm,
                               int Gm, int Gv, int G, int B, float* theta, hipStream_t st);
// weight arenas as values (weights_io.hip).  launch_import_theta: the export's inverse, theta [K, G] (+ context [K, C],
// or null: zeros) into arena rows slot[k] (slot null: rows k) of an arena of `rows`, those rows' ensemble counters zeroed.
// launch_copy_rows: rows src_slot[k] of one arena into rows dst_slot[k] of another, bytewise, the destination counters zeroed.  Slot
// entries outside their arena are skipped, as above.
hipError_t launch_import_theta(const float* theta, const float* context, const int32_t* perm, const int32_t* slot, __bf16* wh,
                               __bf16* wl, float* vf, float* ctx, int* count, int Gm, int Gv, int G, int C, int K, int rows,
                               hipStream_t st);
hipError_t launch_copy_rows(const void* swh, const void* swl, const void* svf, const void* sctx, void* dwh, void* dwl, void* dvf,
                            void* dctx, int* count, const int32_t* src_slot, const int32_t* dst_slot, int Gm, int Gv, int C, int K,
                            int srows, int drows, hipStream_t st);

// ---------------------------------------------------------------- image encoder (DINOv2)
struct EncLayerW {
  const void *wqkv, *wo, *w1, *w2;               // 16-bit [N][K] (K contiguous)
  const void *dqkv, *dwo, *dw1, *dw2;            // 16-bit [N][K]: (W - the 16-bit W above) x 4096, the rounding the corr table compensates
  const float *bqkv, *bo, *b1, *b2;              // f32
  const float *ln1_s, *ln1_b, *ln2_s, *ln2_b, *ls1, *ls2;
};
struct EncWeights {
  const void* w_patch;        // 16-bit [E][Kp] (normalisation folded in)
  const float* b_patch;       // [E] (bias - sum W mean/std)
  const float* pos;           // [S, E] position embeddings (row 0 already has cls_token added)
  const float *lnf_s, *lnf_b;
  EncLayerW layer[ENC_MAX_LAYERS];
};
struct EncWorkspace {
  float* x;        // [B*S, E] residual stream f32
  void* h;         // [B*S, E] 16-bit LN output / attention output
  void* qkv;       // [B*S, 3E] 16-bit
  void* g;         // [B*S, F] 16-bit MLP hidden; also holds the im2col matrix [B*P, Kp]
  float* corr;     // [B, 2, max(3E, F)] bias rows of the current GEMM per image half (bias + mean row of that half . dW)
  void* abar;      // [B, 2, max(E, F)] 16-bit mean rows (upper / lower half of the image) of the current GEMM's activation operand
  float* amap = nullptr;   // nullable: [B, enc_layers, enc_heads, P] attention of the CLS query over the patch keys (opt-in export)
  uint32_t* ln_cnt = nullptr;   // nullable: [B rounded up to 4] arrival words of the LayerNorms fused into the residual GEMMs (encoder.hip GemmArgs::ln_cnt)
  float* ln_part = nullptr;     // nullable: [B][<= 4][256] 16-byte entries, the per-row (sum, sum of squares) of every column tile (GemmArgs::ln_part); either null = LayerNorm as its own launch
  uint32_t ln_spin = 800;       // how long a column tile waits for the image's other tiles before it leaves its share to the last arriver: ticks of 10 ns
#ifdef HVLA_BENCH_HOOKS
  int stop_after = 0;           // libhvla_bench.so (hvla_debug_encode_stop): return behind the n-th dense product of the call (QKV, out, fc1, fc2 of
                                // layer 0 = 1 .. 4, ...), so that a test can read the workspace as that product's consumers would find it
#endif
};
// optional live timing: a pool of hipEvent pairs tagged with a category (include/hvla.h HVLA_PROF_*)
struct Profiler {
  int mode = 0;                       // 0 off, 1 the selected categories only, 2 all
  uint32_t select = 1u << 5;          // mode 1: bit c = category c (hvla_profile_select; default the fc1 GEMM)
  std::vector<hipEvent_t> start, stop;
  std::vector<int> cat;
  size_t used = 0;
  uint64_t nlaunch = 0;               // kernel launches since the last hvla_launches() (counted in run_encoder / hvla_policy / hvla_ensemble)
  bool want(int c) const { return c >= 0 && (mode == 2 || (mode == 1 && ((select >> c) & 1u))); }
  void begin(int c, hipStream_t st) {
    if (!want(c)) return;
    if (used == start.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      start.push_back(a), stop.push_back(b), cat.push_back(c);
    }
    cat[used] = c;
    (void)hipEventRecord(start[used], st);
  }
  void end(int c, hipStream_t st) {
    if (!want(c) || used >= start.size()) return;
    (void)hipEventRecord(stop[used], st);
    ++used;
  }
};
hipError_t launch_encoder(const Geom& g, int dtype, const EncWeights& w, const EncWorkspace& ws,
                          const uint8_t* images, float* tokens, int B, hipStream_t st, Profiler* prof,
                          bool keep_cls = false,    // keep_cls: tokens = f32 [B, S, E] last_hidden_state
                          uint32_t* audit = nullptr);   // [4 sites][2]: max |16-bit operand| (float bits), non-finite count

#ifdef HVLA_BENCH_HOOKS
hipError_t debug_gemm(const void* A, const void* W, const float* bias, const float* aux, void* out, int M, int N,
                      int K, int epi, int variant, int iters, float* ms, hipStream_t st);
hipError_t debug_lnx_stats(unsigned long long* out, int reset);   // [8][256]: fused-LayerNorm counters per workgroup id (encoder.hip g_lnx_dbg)
hipError_t debug_ctx_stamps(unsigned long long* out);   // [64] shader-clock stamps of the last context-encoder launch
hipError_t debug_attention_stamps(const void* qkv, void* o, void* omean, int B, int S, int E, int H, int wg, unsigned long long* stamps,
                                  hipStream_t st);
#endif

// ---------------------------------------------------------------- observation preprocessing (resize.hip)
void build_resize_spans(int in_size, int out_size, std::vector<int>& start, std::vector<int>& count, std::vector<float>& w,
                        int& maxspan);
hipError_t launch_resize(const uint8_t* src, uint8_t* dst, float* tmp_rows, float* tmp_img, const int* row_start,
                         const int* row_count, const float* row_w, int row_span, const int* col_start, const int* col_count,
                         const float* col_w, int col_span, int B, int H, int W, int S, int crop, hipStream_t st,
                         float* padded = nullptr, int src_h = 0, int src_w = 0);   // padded: f32 [B][H][W][3] scratch of resize_with_pad

// ---------------------------------------------------------------- generated policy
struct PolicyParams {
  PolicyLayout pl;
  const __bf16 *wh, *wl;     // [B, Gm]
  const float* vf;           // [B, Gv]
  const float* tokens;       // [B, P, E]
  float* actions;            // [B, horizon, action_dim]
  float* logits;             // [B, horizon] or null
  int B, E, P, L, M, horizon, action_dim;
  float tanh_scale, max_action;
  float* amap = nullptr;     // [B, L, heads, P] or null: attention of the action token over the patch keys, every layer
#ifdef HVLA_BENCH_HOOKS
  unsigned long long* stamps = nullptr;   // libhvla_bench.so: shader-clock time stamps of episode 0 / wave 0 at the phase boundaries
#endif
};
// lang_T > 0: use_language_token (policy_kernel_lang): the arena rows hold the language prefix lang_prefix_kernel
// wrote (LangLayout::m_lkv), lang_T is the number of language tokens; p.amap is then [B, L, heads, lang_T + P]
// episode pool, `slots` not null: workgroup b takes its weights from arena row slots[b] (p.wh / wl / vf point at row 0 of an arena of
// `rows` episodes); tokens, actions, logits and attention rows stay call rows.  Entries outside [0, rows) are skipped.
// mask_as_bias: return_attention_map (policy_kernel_bias): the mask is added to the scores, patch queries attend to
// the action token's key one logit below the others; not together with lang_T > 0
hipError_t launch_policy(const PolicyParams& p, hipStream_t st, int lang_T = 0, const int32_t* slots = nullptr, int rows = 0,
                         bool mask_as_bias = false, bool differential = false);
// differential: use_differential_transformer (policy_kernel_diff); p.pl is then the layout of a Geom with the flag
// (a longer per-layer vector block); not together with lang_T > 0 or mask_as_bias, and p.amap must be null
// use_language_token: the language tokens of K episodes through the policy once (lang_prefix_kernel): K / V of every layer into
// the episodes' arena rows (LangLayout::m_lkv)
struct LangPrefixParams {
  PolicyLayout pl;
  int m_lproj, m_lkv, v_lproj_b, v_lpos;   // LangLayout
  __bf16 *wh, *wl;                   // arena row 0 [rows, Gm]
  const float* vf;                   // [rows, Gv]
  const float* tok;                  // [K, T, lang_dim] (hvla_generate's token_embedding)
  const int32_t* slots;              // [K] arena row of episode k, or null: row k
  int rows, T, lang_dim, L, M;
};
hipError_t launch_lang_prefix(const LangPrefixParams& p, int K, hipStream_t st);

// ---------------------------------------------------------------- caller-side device helpers
// episode pool, `slots` not null: count [B] one counter per arena row; call row k of K is arena row slots[k].  Else count [1], B call rows.
hipError_t launch_ensemble(const float* actions, float* ring, int* count, const float* mean, const float* std, const uint8_t* mask,
                           float* out, int B, int horizon, int action_dim, hipStream_t st, const int32_t* slots = nullptr, int K = 0);

// episode pool post-processing (postprocess.hip, include/hvla.h hvla_post_*): the caller-side state of one slot's episode
// (InferenceWrapper's ensemble counter and gripper fields), next to a ring of its last `horizon` un-normalised predictions
constexpr int POST_MAX_HORIZON = 16;          // the ensemble weights 1 / n come from a table of this many entries
constexpr int POST_STICKY_REPEATS = 15;       // google_robot's sticky_gripper_num_repeat (hypervla_interface.py:49-53)
struct PostSlot {
  double prev_grip;                           // previous_gripper_action (valid when has_prev)
  double sticky_value;                        // sticky_gripper_action
  int32_t calls;                              // postprocess calls since the slot was assigned
  int32_t row;                                // row of the caller's hvla_post_row table
  int32_t ensemble, has_prev, sticky_on, repeat;
};
hipError_t launch_post_assign(PostSlot* state, const int32_t* slots, int K, int B, const int32_t* rows, const uint8_t* ensemble,
                              hipStream_t st);
hipError_t launch_post_step(const float* actions, const int32_t* slots, int K, int B, int H, double* ring, PostSlot* state,
                            const hvla_post_row* table, int n_rows, double* raw_out, double* env_out, hipStream_t st);

hipError_t launch_loss(const float* actions, const float* logits, const float* target, const uint8_t* tmask,
                       const uint8_t* amask, float* loss, int B, int horizon, int action_dim, float max_action,
                       bool clip_target, hipStream_t st);

// ---------------------------------------------------------------- training metrics (metrics.hip, include/hvla.h hvla_loss_terms;
// train_metrics, the body of hvla_train_metrics, is declared in train.h next to the structures it reads)
// continuous / gripper f32 [B]; sqerr f32 [B] and sqerr64 f64 [B] nullable (the same f64 sum, rounded or not)
hipError_t launch_loss_terms(const float* actions, const float* logits, const float* target, const uint8_t* tmask, const uint8_t* amask,
                             float* continuous, float* gripper, float* sqerr, double* sqerr64, int B, int horizon, int action_dim,
                             float max_action, bool clip_target, hipStream_t st);

// ---------------------------------------------------------------- publish (publish.hip, include/hvla.h hvla_train_publish)
// the flat training vector `params` into the serving buffers; the encoder's three only with train_encoder
struct PublishArgs {
  Geom g;
  const float* params;
  float* hn;
  const int32_t* perm;
  uint16_t *wcat_hi, *wcat_lo;
  float* bcat;
  int Gtot;                     // Gm + Gv, packed positions
  uint16_t *enc16, *encd16;
  float* encf32;
  int bf, train_encoder;
  // layer_tokens: wcat_hi / wcat_lo hold one fragment block per segment (pack.h TokenSegments).  Per packed position its
  // head column in the training vector's W_h (-1: padding) and its token; per segment its tile and its token (device, from the load)
  const int32_t *pos_head = nullptr, *pos_token = nullptr, *seg_tile = nullptr, *seg_token = nullptr;
  int nseg = 0;
};
hipError_t launch_publish(const PublishArgs& a, hipStream_t st);

// ---------------------------------------------------------------- position table (position.hip, include/hvla.h hvla_position_*)
// src [1 + n n, E] -> dst [1 + grid grid, E] through the resize whose per-axis weight matrix is w [n, grid] (device), and the
// adjoint ddst -> dsrc of that map.  E % 4 == 0, every pointer 16-byte aligned.
hipError_t launch_position_interp(const float* src, int n, const float* w, float* dst, int grid, int E, hipStream_t st);
// the serving buffer's table: `table` [1 + grid grid, E] = resize of src, then the class token added into row 0 as the loader does
hipError_t launch_position_serve(const float* src, int n, const float* w, const float* cls, float* table, int grid, int E, hipStream_t st);
hipError_t launch_position_adjoint(const float* ddst, int n, const float* w, float* dsrc, int grid, int E, hipStream_t st);

// ---------------------------------------------------------------- self test
hipError_t launch_selftest(int* fail_flags, hipStream_t st);
hipError_t run_box_probe(float* sink, unsigned long long* ticks, float out[3], hipStream_t st);   // selftest.hip: sustained clock / MFMA rate of this box

}  // namespace hvla
