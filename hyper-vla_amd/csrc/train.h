// train.h — fine-tune step structures (train.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/hvla.h"
#include "layout.h"
#include "noise.h"
#include "train_layout.h"

namespace hvla {

// generic batched f32 GEMM on the matrix cores (split-bf16, f32-class accuracy; train_gemm.hip):
//   C[b0,b1] (+)= alpha * op(A)[b0,b1] * op(B)[b0,b1] (+ bias[b0][n]),  batch = blockIdx.z = b0 * nb1 + b1
struct BG {
  const float* A;
  const float* B;
  float* C;
  const float* bias;          // nullable, indexed [n], batch stride sBias0
  int M, N, K, lda, ldb, ldc;
  long sA0, sA1, sB0, sB1, sC0, sC1, sBias0;
  int nb1;                    // batch = blockIdx.z = b0 * nb1 + b1
  float alpha;
  int accumulate;             // 0 store, 1 C += (one writer per element), 2 atomic C += (batches share C)
  int ksplit = 1;             // > 1: K is cut into ksplit chunks over blockIdx.z, reduced with atomics (accumulate != 0)
  int allow_split = 0;        // 1: the launcher may choose ksplit > 1 itself (deep-K gradient products; result then
                              //    depends on the order of the atomic adds in its last bits)
  int a_padded = 0;           // 1: every row of A is followed by zeros up to a multiple of 4 elements inside lda (the attention
                              //    matrices, row stride S rounded up): float4 staging may run over the row's end
  long sBias1 = 0;            // bias stride of the inner batch index b1
};
void bgemm(hipStream_t st, bool ta, bool tb, BG g, int nb0);
// The grouped form: ONE launch whose workgroup column blockIdx.x takes its operand origins, its column origin and
// width and its K range from tiles[blockIdx.x] (device memory; train_layout.h group_tiles).  g gives the bases, M, the leading
// dimensions, alpha, the bias base (nullable) and accumulate (0 store, 1 +=, 2 atomic +=), K for a tile without a K range of its own; g.N, the
// strides and ksplit are not read.  grid = (ntiles, ceil(M / tile), nz); tile = 64 / 128 square; vec_ok: every origin of the table is a multiple of 4 floats.
// `flops`: the product's f32-equivalent work for the launch timer.  The same staging, hi / lo split, three-MFMA core and store
// modes as bgemm()'s kernel, in a kernel of its own.
void bgemm_groups(hipStream_t st, bool ta, bool tb, BG g, const BGTile* tiles, int ntiles, int tile, int nz, bool vec_ok, double flops);
// One operand of a product: its base, leading dimension and the strides of the outer (b0) and inner (b1) batch index.  T = float
// converts to T = const float and not back: only an Out names a C.
template <class T> struct Operand {
  T* p; int ld; long s0, s1;
  Operand(T* p_, int ld_, long s0_ = 0, long s1_ = 0) : p(p_), ld(ld_), s0(s0_), s1(s1_) {}
  template <class U> Operand(const Operand<U>& o) : p(o.p), ld(o.ld), s0(o.s0), s1(o.s1) {}
};
using In = Operand<const float>;
using Out = Operand<float>;
// the shapes the step's operands have, by name:
// one matrix for every batch -- shared weights, or [nb][S][ld] activations with the batch folded into M
template <class T> Operand<T> mat(T* p, int ld) { return {p, ld}; }
// [nb][n][ld]: n rows a sample (a product may use fewer: the first T of a context block's Sc rows)
template <class T> Operand<T> per_sample(T* p, int n, int ld) { return {p, ld, (long)n * ld}; }
// a matrix per episode at any stride (a generated leaf in its row of theta: stride G)
template <class T> Operand<T> per_episode(T* p, int ld, long stride) { return {p, ld, stride}; }
// matrices `step` apart as the inner batch b1 (q, k, v in one product), the same for every b0
template <class T> Operand<T> inner_batch(T* p, int ld, long step) { return {p, ld, 0, step}; }
// head b1 of an activation [nb][S][D]: columns [b1 w, b1 w + w), w = hd (w = hd / 2: the 2 H sub-heads of DifferentialAttention)
template <class T> Operand<T> head_slice(T* x, int S, int D, int w) { return {x, D, (long)S * D, w}; }
// The S x S attention matrices have row stride Sp = S rounded up to 4 floats, zeros behind every row (written by the softmax kernels):
// as A operands (a_padded) they are staged with float4 loads like everything else (S = 257: the all-dword staging these four
// products per layer were left with cost 3.6 ms per step).  A block keeps Hn = H tables a sample, 2 H under DifferentialAttention.
inline int score_stride(int S) { return (S + 3) & ~3; }
inline long score_floats(long H, long S, bool differential = false) { return (differential ? 2 * H : H) * S * score_stride((int)S); }
// the score tables [nb][Hn][S][Sp], table b1 of sample b0
template <class T> Operand<T> score_table(T* p, int Hn, int S) { return {p, score_stride(S), score_floats(Hn, S), (long)S * score_stride(S)}; }
// what a product does with C
enum class Store {
  Set,          // C = ...
  Add,          // C += ..., one writer per element
  Atomic,       // atomic C += ...: batches share C
  AddSplitK,    // C += ..., and the launcher may cut K into chunks reduced with atomics (BG::allow_split)
};
// C[b0, b1] = / += alpha op(A)[b0, b1] op(B)[b0, b1], op(A) M x K and op(B) K x N, nb1 inner batches; bgemm()'s nb0 gives the outer count
inline BG product(In A, In B, Out C, int M, int N, int K, Store store = Store::Set, float alpha = 1.f, int nb1 = 1) {
  BG g{A.p, B.p, C.p, nullptr};
  g.M = M; g.N = N; g.K = K; g.lda = A.ld; g.ldb = B.ld; g.ldc = C.ld;
  g.sA0 = A.s0; g.sA1 = A.s1; g.sB0 = B.s0; g.sB1 = B.s1; g.sC0 = C.s0; g.sC1 = C.s1; g.sBias0 = 0;
  g.nb1 = nb1; g.alpha = alpha;
  g.accumulate = store == Store::Set ? 0 : store == Store::Atomic ? 2 : 1;
  g.allow_split = store == Store::AddSplitK;
  return g;
}
// ... + bias[b0, b1][n] (nullable)
inline BG with_bias(BG g, const float* bias, long s0 = 0, long s1 = 0) { g.bias = bias; g.sBias0 = s0; g.sBias1 = s1; return g; }
// ... whose A is score tables: zeros up to a multiple of 4 floats behind every row
inline BG a_padded(BG g) { g.a_padded = 1; return g; }
void train_gemm_timer(bool on, bool first_use_by_this_context);                  // hvla_train_profile (the current device's timer; counts its users)
void train_gemm_timer_release();                                                 // hvla_destroy of a context that used it: the events go with the last user
hipError_t train_gemm_timer_read(float* ms, double* flops, int* launches);      // since the last read

#ifdef HVLA_BENCH_HOOKS
void set_train_gemm_exact(bool on);
// what the last bgemm() launch of this process chose (hvla_debug_bgemm_once reports it; tools/bgemm_check.py): tile = 64 / 128 / 256 rows
// (256 x 128, else square), vec = float4 staging, ksplit = the K chunks on blockIdx.z, exact = bgemm_kernel (f32 instruction; tile 64)
struct BgemmChoice { int tile, vec, ksplit, exact; };
const BgemmChoice& last_bgemm_choice();
#endif
// The reference's train=True noise (hvla_train_noise; noise.h).  Off (the default, and every rate 0): train_step
// launches exactly what it launches without this struct and the workspace has today's size.  On: one element-wise launch per site
// and pass whose rate is positive; the policy's two residual GEMMs then write the branch into t.y and dropout_fwd_kernel adds it to
// the residual.  The context encoder's and DINOv2's blocks draw nothing, and neither does a forward_only step.  Workspace: the
// noisy copy of the frozen encoder's tokens (sigma > 0) and the masked copy of the CLS rows (image_dropout > 0) are taken behind
// everything else, so every other offset is what it is without noise; the size is asked for AFTER the setting is made.
struct TrainNoise {
  float policy_dropout = 0.f, sigma = 0.f, context_dropout = 0.f, image_dropout = 0.f;
  NoiseKey key;                       // seed, draw, sample_offset (site is filled in per launch)
  bool on() const { return policy_dropout > 0.f || sigma > 0.f || context_dropout > 0.f || image_dropout > 0.f; }
};
size_t train_workspace_floats(const Geom& g, int B, bool train_encoder, const TrainNoise& nz = TrainNoise());
// hvla_train_context_rows: where a step of this batch size leaves ctx and dctx [B][NL][C] in `work` (offsets in floats), and their length
void train_context_rows(const Geom& g, int B, bool train_encoder, const TrainNoise& nz, long out[3]);
// hvla_train_noise_probe: out[i] = the multiplier of element i of a dropout site (rate > 0: 0 or 1 / keep_prob) or, with
// normal, the i-th normal of the site, for the sample whose global index is key.sample0
hipError_t train_noise_probe(const NoiseKey& key, float rate, bool normal, long n, float* out, hipStream_t st);

struct TrainBuffers {        // all device memory, owned by the caller
  float* params;             // [total]
  float* grads;              // [total]
  __bf16* mu;                // [total]  AdamW first moment (optax mu_dtype = bfloat16)
  float* nu;                 // [total]
  float* ema;                // [total] or null
  float* theta;              // [B, G]
  float* dtheta;             // [B, G]
  float* work;               // [train_workspace_floats]
  float* loss;               // [B]
  float* actions;            // [B, horizon, action_dim] or null
  float* logits;             // [B, horizon] or null
  float* sqsum;              // [1]
  const uint8_t* wd_mask;    // [total (+ enc_total)] 1 where decoupled weight decay applies: built by the host from the
                             //     selected weight_decay_strategy (hypervla/train.py), flat parameter order
  const float* params0;      // [enc_total (+ source tail)] pretrained encoder weights for the delta decay (train.py:465-471) or null
};
struct TrainInputs {
  const float* tok;          // [B, T, lang_dim]
  const int64_t* attn_mask;  // [B, T]
  const float* cls;          // [B, E]
  const float* tokens;       // [B, P, E]  frozen-encoder patch tokens (hvla_encode); null when `images` is given
  const uint8_t* images;     // [B, H, W, 3] -> the encoder runs (and is differentiated) inside the step
  const float* target;       // [B, horizon, action_dim]
  const uint8_t* tmask;      // [B]
  const uint8_t* amask;      // [B, horizon, action_dim]
};
struct TrainHyper {
  float lr, b1, b2, eps, weight_decay, clip, ema_decay;
  int step, forward_only;
  float base_lr, base_weight_decay;      // optimizer group of the shared (DINOv2) leaves, train_utils.py:411-419
};
// The DINOv2 position table trained through its interpolation (hvla_train_position_source; position.hip).  n == 0: off, and every
// entry below launches exactly what it launches without this struct.  On (trained encoder only): the flat vector is
// [hypernetwork | encoder leaves | source table (1 + n n) E]; the baked table's slot among the encoder leaves (TrainLayout::e_pos)
// stays where it is as a derived quantity -- resized from the tail before the encoder reads it, its gradient carried to the tail
// by the adjoint and then zeroed.
struct PosSource {
  int n = 0;                 // side of the source grid
  const float* w = nullptr;  // [n, grid] per-axis resize weights (device, owned by the caller)
  int grid = 0, E = 0;       // the context's
  long tail() const { return n ? (long)(1 + (long)n * n) * E : 0; }
};
// bucket_done (nullable, [3]): events recorded on `st` when a contiguous range of `grads` is final -- [0] the shared DINOv2
// leaves [total, total + enc_total) after the image encoder's backward (trained encoder only), [1] the output heads
// [wcat, total) after the weight-generation backward, [2] the context encoder [0, wcat) at the end -- so that the caller's
// all-reduce of a bucket runs under the rest of the backward pass.
// frozen_buckets / frozen (hvla_train_frozen; 0 / nullptr: off, and exactly the launches without them): bit 1 leaves out dW_cat and
// db_cat, bit 2 dctx and the context encoder's backward -- the skipped ranges of `grads` stay zero, all three events are still
// recorded; `frozen` [n] (device, 1 = frozen) takes its elements out of the global norm and out of AdamW's loads and stores.
// The attention terms of the reference's sample_loss_fn (hvla_train_attention_losses; scripts/train.py:348-373), both on the action
// token's attention row of the last policy layer: loss_b += w_ent ent_b + w_align align_b.  Off (both weights 0, the default):
// train_step launches exactly what it launches without this struct.  On: attention_aux_kernel once behind head_loss_kernel (also
// forward-only) and once inside the last policy layer's backward; no workspace.
struct AttnAux {
  float w_ent = 0.f, w_align = 0.f;   // w_align: the effective, already annealed weight
  const float* ref = nullptr;         // [B, P] DINOv2's last-layer CLS attention over the patches, mean over heads (device; read iff w_align > 0)
  float* ent = nullptr;               // [B] out, nullable: ent_b
  float* align = nullptr;             // [B] out, nullable: align_b (written iff w_align > 0)
  bool on() const { return w_ent > 0.f || w_align > 0.f; }
};
// hvla_train_layer_tokens: the tile tables of the three grouped weight-generation products in device memory, built
// once per context from the layout's run table (api.hip; train_layout.h group_tiles).  fwd / dw: 64- and 128-column tiles [0] / [1]
struct TokenGroups {
  const BGTile *fwd[2] = {nullptr, nullptr}, *dw[2] = {nullptr, nullptr}, *dctx = nullptr;
  int ntiles[2] = {0, 0}, ndctx = 0;
  bool vec_ok = false;
};
// the five tables back to back in `host` (what the caller uploads to `base`), and the selection that points into `base`
inline TokenGroups token_groups(const Geom& g, const TrainLayout& L, const BGTile* base, std::vector<BGTile>& host) {
  TokenGroups t;
  host.clear();
  auto put = [&](int kind, int tile, int& count) {
    const std::vector<BGTile> v = group_tiles(g, L, kind, tile);
    const BGTile* at = base + host.size();
    host.insert(host.end(), v.begin(), v.end());
    count = (int)v.size();
    return at;
  };
  int n = 0;
  t.fwd[0] = put(0, 64, t.ntiles[0]); t.fwd[1] = put(0, 128, t.ntiles[1]);
  t.dw[0] = put(1, 64, n); t.dw[1] = put(1, 128, n);
  t.dctx = put(2, group_kchunk(L), t.ndctx);
  t.vec_ok = group_vec_ok(g, L);
  return t;
}
// what the hvla_train_* setters selected, in one struct for the three entries below (default: everything off)
struct TrainOptions {
  PosSource ps;                       // hvla_train_position_source (trained encoder only)
  const uint8_t* frozen = nullptr;    // hvla_train_frozen: the mask of train_apply / train_accumulate ...
  int frozen_buckets = 0;             //   ... and the buckets train_step leaves out
  AttnAux aux;                        // hvla_train_attention_losses
  TrainNoise noise;                   // hvla_train_noise_set
  TokenGroups groups;                 // hvla_train_layer_tokens (read under Geom::layer_tokens only)
};
// vector length of params / grads / mu / nu: the shared leaves and the position table's source follow the hypernetwork's when
// the image encoder is trained
inline long train_vector_elems(const TrainLayout& L, const PosSource& ps, bool train_encoder) {
  return L.total + (train_encoder ? L.enc_total + ps.tail() : 0);
}
hipError_t train_step(const Geom& g, const TrainLayout& L, const TrainBuffers& tb, const TrainInputs& in, int B,
                      const TrainHyper& hp, hipStream_t st, hipEvent_t* bucket_done, const TrainOptions& opt);
hipError_t train_apply(const TrainLayout& L, const TrainBuffers& tb, const TrainHyper& hp, bool train_encoder, hipStream_t st,
                       const TrainOptions& opt);
hipError_t train_accumulate(const TrainLayout& L, const TrainBuffers& tb, float* acc, float inv_k, const TrainHyper& hp,
                            bool train_encoder, hipStream_t st, const TrainOptions& opt);
// hvla_train_metrics (metrics.hip): launches of its own, none of the three entries above changes by it.  Reads tb and `in`, writes
// `out` and in.scratch only.  opt.ps / opt.frozen as for train_apply.
hipError_t train_metrics(const Geom& g, const TrainLayout& L, const TrainBuffers& tb, const hvla_train_metrics_in& in, float* out, int B,
                         bool train_encoder, hipStream_t st, const TrainOptions& opt);

}  // namespace hvla
