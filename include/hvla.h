/*
 * hvla.h — C ABI of libhvla: the MI355X-native HyperVLA action-prediction path.
 *
 * Drop-in boundary.  Each entry point names the reference interface it replaces
 * (paths relative to the reference repository).  The reference is pure Python/JAX and has no FFI
 * of its own; a maintainer binds this library with ctypes from hypervla/model.py (the stub is in
 * INTEGRATION.md; the binding this repo ships is hyper-vla_amd/hypervla/_native.py).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / HIP types in signatures (`stream` is a hipStream_t
 *     passed as void*; NULL = the device's default stream).
 *   - every data pointer of generate/encode/policy/step/export is a DEVICE pointer owned by the
 *     caller; hvla_load_weights takes HOST pointers.
 *   - every call returns HVLA_OK (0) or a negative HVLA_E_* code; no C++ exception crosses the
 *     boundary; hvla_last_error(ctx) gives the message of the last failing call on that ctx.
 *   - a ctx is bound to one device; calls on one ctx are not re-entrant; different ctxs are
 *     independent.  After hvla_load_weights, encode/policy/step do not allocate, do not
 *     synchronise and launch only on `stream`, so a step can be captured into a hipGraph.
 *     hvla_generate allocates its weight arena only when the ctx holds no arena of that batch size
 *     handed back by hvla_weights_free (the first episode batch of a size; afterwards it only
 *     launches on `stream`); hvla_weights_free waits for the device, as hipFree would.
 */
#ifndef HVLA_H_
#define HVLA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HVLA_OK 0
#define HVLA_E_SHAPE (-1)      /* batch / geometry outside what the ctx was created for        */
#define HVLA_E_DTYPE (-2)      /* unsupported operand type selector                            */
#define HVLA_E_DEVICE (-3)     /* bad device ordinal, or not a gfx950 device                   */
#define HVLA_E_ARENA_FULL (-4) /* device allocation for a weight arena / workspace failed      */
#define HVLA_E_HIP (-5)        /* a HIP runtime call failed (message has the hipError string)  */
#define HVLA_E_WEIGHTS (-6)    /* missing / mis-sized / unknown named tensor                   */
#define HVLA_E_STATE (-7)      /* call order violated (e.g. step before load_weights)          */

#define HVLA_ENC_F16 0  /* encoder MFMA operands fp16 (default: meets the 1e-3 action tolerance) */
#define HVLA_ENC_BF16 1 /* encoder MFMA operands bf16 (same rate, ~7x larger action error)       */

typedef struct hvla_ctx hvla_ctx;
typedef struct hvla_weights hvla_weights; /* per-batch generated-weight arena (opaque)          */

/* Geometry of the path == the values the reference reads from config.json
 * (hypervla/model.py:152-163,197-200; README.md:33-61).                                        */
typedef struct hvla_config {
  uint32_t struct_size;                      /* = sizeof(hvla_config) of the header the caller was built against: hvla_create
                                                returns HVLA_E_SHAPE when it is not this library's (the struct is passed by pointer
                                                and grows at its end; a binder built against another header is refused, never
                                                read past its end)                                                      */
  int32_t image_size, patch;                 /* 224, 14.  (image_size / patch)^2 must be 256 or 64 patches (the whole list of what
                                                hvla_create serves: csrc/accept.h; anything else is HVLA_E_SHAPE)               */
  int32_t enc_dim, enc_layers, enc_heads, enc_mlp; /* DINOv2-base: 768, 12, 12, 3072            */
  int32_t dim, layers, heads, mlp;           /* generated vit_t: 64, 4, 4, 128.  dim == 64, heads == 4, mlp % 32 == 0, layers >= 1, and
                                                the per-layer vectors -- layers x (576 + mlp) + 160 floats -- must fit the policy kernel's
                                                LDS (at 256 patches 5632 floats, 3584 with use_language_token): HVLA_E_SHAPE otherwise  */
  int32_t horizon, action_dim;               /* 4, 7.  horizon >= 1, action_dim >= 2, horizon * action_dim <= 32                */
  float tanh_scale, max_action;              /* 5, 5 (action_heads.py:469-470)                  */
  int32_t ctx_dim, ctx_layers, ctx_heads, ctx_mlp; /* hypernet: 128, 6, 4, 512.  ctx_dim 128, 64 or 32; ctx_dim / ctx_heads a multiple
                                                of 4 (the score loop's k-steps); ctx_mlp % 16 == 0 (the f32 MFMA's column
                                                tiles), and the context encoder's LDS working set -- (lang_tokens + 2) rows
                                                (lang_tokens + 1 + NL with layer_tokens, hvla_policy_options_v4) of
                                                max(3 ctx_dim, ctx_mlp) + 2 ctx_dim floats -- must fit 160 KiB: hvla_create
                                                returns HVLA_E_SHAPE otherwise                                          */
  int32_t lang_tokens, lang_dim;             /* 32, 768                                         */
  int32_t scale_context;                     /* hypernetwork.py:191-192                         */
  int32_t max_batch;                         /* workspace is sized for this many episodes       */
  int32_t enc_dtype;                         /* HVLA_ENC_F16 | HVLA_ENC_BF16                    */
  int32_t streams;                           /* 1 (default, 0 = 1) or 2: hvla_step runs the two halves of a batch of
                                                >= 64 episodes on two streams, forked from / joined to the caller's  */
  int32_t clip_target;                       /* action_head_kwargs.clip_target (action_heads.py:408,499-500): the loss clips
                                                the action target to +-max_action iff non-zero                        */
} hvla_config;

/* One named float32 tensor of the hypernetwork checkpoint, HOST memory, reference naming
 * (SURVEY.md §5.4): "task_token_projection/kernel", "Transformer_0/encoderblock_3/LayerNorm_0/scale",
 * "output_head_<flat leaf>/kernel", flat shared vectors "encoder_image_encoder_<path>", ...      */
typedef struct hvla_tensor_desc {
  const char* name;
  const float* data;
  int64_t numel;
} hvla_tensor_desc;

/* Replaces: HyperVLA.load_pretrained's model construction (hypervla/model.py:197-208).          */
int hvla_create(const hvla_config* cfg, int device, hvla_ctx** out);

/* Model options outside hvla_config (whose size is part of the ABI).  Follows hvla_config's rule: struct_size must be
 * sizeof(hvla_policy_options) of this header, or hvla_create_with returns HVLA_E_SHAPE before reading anything else.
 *   use_language_token  base_net_kwargs.vit_kwargs.use_language_token (base_vit.py:159-166,207-212): the token embeddings
 *                       given to hvla_generate, projected by the generated language_token_projection, lead the policy's
 *                       sequence [lang_tokens language | P patches | 1 action]; language queries see only language keys.
 *                       Needs lang_tokens <= 32 and lang_dim % 64 == 0.  hvla_generate / hvla_generate_slots then also run
 *                       the language tokens through the policy once per episode and keep their K / V of every layer beside
 *                       the episode's weights; the training entry points refuse such a ctx until
 *                       hvla_train_language_tokens(ctx, 1) asks for the policy with its language prefix.              */
typedef struct hvla_policy_options {
  uint32_t struct_size;                      /* = sizeof(hvla_policy_options)                                           */
  int32_t use_language_token;                /* 0 (default) or 1                                                        */
} hvla_policy_options;

/* hvla_create with options; opts == NULL is hvla_create (the same ctx, byte for byte).                               */
int hvla_create_with(const hvla_config* cfg, const hvla_policy_options* opts, int device, hvla_ctx** out);

/* hvla_policy_options with one more field.  The size of hvla_policy_options is part of the ABI (its exact-size rule refuses any
 * other), so the field travels in a struct and an entry of its own; the same rule holds here for sizeof(hvla_policy_options_v2).
 *   use_language_token      as above
 *   attention_mask_as_bias  base_net_kwargs.vit_kwargs.return_attention_map (hypervla/components/transformer.py:172-181): the
 *                       policy blocks' attention is CustomMultiHeadDotProductAttention, which hands the boolean mask of
 *                       base_vit.py:209-214 to dot_product_attention_weights as `bias=` (multi_head_attetion.py:88-98): the
 *                       mask's 1 / 0 is ADDED to the scaled scores and nothing is masked, so a patch query also attends to the
 *                       action token's key, one logit below every other key; the action row is the masked model's formula.
 *                       The generated leaves of the attention are then named `..._CustomMultiHeadDotProductAttention_0_...`
 *                       and lead their block in the parameter order (hvla_load_weights, hvla_weights_import / _export, the
 *                       training vector).  Served, fine-tuned and published like any other context.  Not
 *                       built together with use_language_token (language queries would attend to patch keys, so the language
 *                       prefix would be no per-episode constant): HVLA_E_SHAPE, hvla_last_error(NULL) says why.            */
typedef struct hvla_policy_options_v2 {
  uint32_t struct_size;                      /* = sizeof(hvla_policy_options_v2)                                        */
  int32_t use_language_token;                /* 0 (default) or 1                                                        */
  int32_t attention_mask_as_bias;            /* 0 (default) or 1                                                        */
} hvla_policy_options_v2;

/* hvla_create_with for hvla_policy_options_v2: opts == NULL, or attention_mask_as_bias 0, is hvla_create_with of the same
 * use_language_token (the same ctx, byte for byte).  A refusal leaves *out NULL; where it has more to say than its code,
 * hvla_last_error(NULL) returns the text until this thread's next hvla_create / hvla_create_with / hvla_create_with_v2.  */
int hvla_create_with_v2(const hvla_config* cfg, const hvla_policy_options_v2* opts, int device, hvla_ctx** out);

/* hvla_policy_options_v2 with one more field, by the same rule (struct_size must be sizeof(hvla_policy_options_v3)).
 *   differential_attention  base_net_kwargs.vit_kwargs.use_differential_transformer (hypervla/components/transformer.py:166-171):
 *                       the policy blocks' attention is DifferentialAttention (differential_transformer.py:99-252).  Each of
 *                       the `heads` heads splits its dim / heads q and k features into two halves; each half has its own
 *                       softmax over all P + 1 keys, unscaled, with the mask of base_vit.py:209-214 ADDED to the scores (as under
 *                       attention_mask_as_bias); the head's output is (A1 - lambda A2) V with lambda = exp(lambda_q1 . lambda_k1)
 *                       - exp(lambda_q2 . lambda_k2) + lambda_init(layer), RMS-normalised over the head's dim / heads values
 *                       (eps 1e-5), times subln's weight and 1 - lambda_init(layer).  The generated leaves of the attention are
 *                       `..._DifferentialAttention_0_{k_proj_kernel, lambda_k1, lambda_k2, lambda_q1, lambda_q2, out_proj_kernel,
 *                       q_proj_kernel, subln_weight, v_proj_kernel}` (no biases) and lead their block in the parameter order.
 *                       Until hvla_train_differential(ctx, 1) asks for its backward pass every
 *                       hvla_train_* entry that reads the geometry, hvla_train_publish included, returns HVLA_E_SHAPE with
 *                       a text; so does hvla_set_attention_outputs with a head_attention buffer (the reference sows no
 *                       attention weights in this branch); dino_cls_attention alone is accepted.  Not built together with use_language_token or attention_mask_as_bias (with both
 *                       vit_kwargs set the reference runs DifferentialAttention: pass differential_attention alone):
 *                       HVLA_E_SHAPE, hvla_last_error(NULL) says why.                                                       */
typedef struct hvla_policy_options_v3 {
  uint32_t struct_size;                      /* = sizeof(hvla_policy_options_v3)                                        */
  int32_t use_language_token;                /* 0 (default) or 1                                                        */
  int32_t attention_mask_as_bias;            /* 0 (default) or 1                                                        */
  int32_t differential_attention;            /* 0 (default) or 1                                                        */
} hvla_policy_options_v3;

/* hvla_create_with_v2 for hvla_policy_options_v3: opts == NULL, or differential_attention 0, is hvla_create_with_v2 of the other
 * two fields (the same ctx, byte for byte).  Refusals as for hvla_create_with_v2.                                          */
int hvla_create_with_v3(const hvla_config* cfg, const hvla_policy_options_v3* opts, int device, hvla_ctx** out);

/* hvla_policy_options_v3 with two more fields, by the same rule (struct_size must be sizeof(hvla_policy_options_v4)).
 *   layer_tokens        hypernet_kwargs.share_layer_index=False (hypervla/model.py:400-436, the reference config's default): the
 *                       context encoder's sequence ends in NL = layers + 5 (+ 1 with use_language_token) learned layer tokens, one
 *                       per module of the policy in key-sorted order -- 0 the shared image encoder (attended by nobody), then
 *                       encoder_norm, encoderblock_<l> as strings (encoderblock_10 before encoderblock_2), image_embedding_
 *                       projection, (language_token_projection,) pos_embedding, action_head -- a layer key is attended by the
 *                       layer queries alone (hypernetwork.py:149-181), and every generated leaf is the output head of its name
 *                       applied to the context row of its module's token (hypernetwork.py:199-217).  Shapes that
 *                       change: "layer_pos_embedding" is (1, NL, ctx_dim) in hvla_load_weights; the context of an episode is
 *                       [NL, ctx_dim] wherever it is carried (hvla_weights_export / _import / _import_slots, pool slots, copies).
 *                       Needs lang_tokens + 1 + NL <= 48 and the context encoder's LDS working set with that many rows within
 *                       160 KiB.  Served only: every hvla_train_* entry returns HVLA_E_SHAPE with a text naming share_layer_index.
 *   shared_block_heads  hypernet_kwargs.share_TF_output_head (hypernetwork.py:221-225): the leaves of all policy blocks with one
 *                       name are generated by ONE output head, "output_head_encoder_Transformer_0_encoderblock_<rest>" in
 *                       hvla_load_weights, and differ through their tokens alone.  Only with layer_tokens: HVLA_E_SHAPE otherwise,
 *                       hvla_last_error(NULL) says why.                                                                         */
typedef struct hvla_policy_options_v4 {
  uint32_t struct_size;                      /* = sizeof(hvla_policy_options_v4)                                        */
  int32_t use_language_token;                /* 0 (default) or 1                                                        */
  int32_t attention_mask_as_bias;            /* 0 (default) or 1                                                        */
  int32_t differential_attention;            /* 0 (default) or 1                                                        */
  int32_t layer_tokens;                      /* 0 (default) or 1                                                        */
  int32_t shared_block_heads;                /* 0 (default) or 1                                                        */
} hvla_policy_options_v4;

/* hvla_create_with_v3 for hvla_policy_options_v4: opts == NULL, or both new fields 0, is hvla_create_with_v3 of the other three
 * (the same ctx, byte for byte).  Refusals as for hvla_create_with_v2.                                                      */
int hvla_create_with_v4(const hvla_config* cfg, const hvla_policy_options_v4* opts, int device, hvla_ctx** out);
/* NL, the layer tokens of the context (1 unless created with layer_tokens): an episode's context is [NL, ctx_dim].  NULL ctx: 0.  */
int32_t hvla_num_layer_tokens(const hvla_ctx* ctx);
void hvla_destroy(hvla_ctx* ctx);
const char* hvla_last_error(const hvla_ctx* ctx);

/* Replaces: orbax restore of HN params + `.replace(params=EMA)` (hypervla/model.py:210-214,
 * data/simpler/evaluate.py:438-444).  Packs every tensor into its device layout.
 * With layer_tokens "layer_pos_embedding" has NL * ctx_dim elements; with shared_block_heads the policy blocks' output heads are the
 * shared ones, "output_head_encoder_Transformer_0_encoderblock_<rest>/{kernel,bias}" (hvla_policy_options_v4).
 * Must be given every tensor of the checkpoint in one call; may be called again to swap weights. */
int hvla_load_weights(hvla_ctx* ctx, const hvla_tensor_desc* tensors, int32_t n);

/* Number of generated parameters per episode (G = 201500 for the README geometry).              */
int64_t hvla_num_generated(const hvla_ctx* ctx);

/* Replaces: HyperVLA.create_tasks -> HyperNetwork.__call__ (hypervla/model.py:35-83,
 * hypervla/components/hypernetwork.py:99-233) for B episodes at once.
 *   token_embedding f32 [B, lang_tokens, lang_dim]; attention_mask i64 [B, lang_tokens];
 *   initial_cls f32 [B, enc_dim]  (= initial_state["patch_embeddings"][:, 0]).
 * On success *out owns a device arena with B episodes' policy weights.                          */
int hvla_generate(hvla_ctx* ctx, const float* token_embedding, const int64_t* attention_mask,
                  const float* initial_cls, int32_t B, hvla_weights** out, void* stream);
int hvla_weights_free(hvla_ctx* ctx, hvla_weights* w);
/* hvla_weights_free parks up to 4 arenas per ctx for the next hvla_generate of the same batch size (0.8 MB per episode at the
 * README geometry: ~0.8 GB stay resident after batches of 256).  This gives them back to the device (waits for the device).
 * The pool is locked: hvla_weights_free / hvla_release_pooled_arenas may be called from another thread than hvla_generate
 * (a garbage collector), everything else on a ctx stays single-threaded.                                                   */
int hvla_release_pooled_arenas(hvla_ctx* ctx);
int32_t hvla_weights_batch(const hvla_weights* w);

/* Reference-order views for the caller / parity tests (the reference returns these from
 * create_tasks as `base_params` and the context embedding).  theta f32 [B, G] in pytree leaf
 * order; context f32 [B, ctx_dim], with layer_tokens [B, NL, ctx_dim]
 * (NL = hvla_num_layer_tokens).  Either pointer may be NULL.                                    */
int hvla_weights_export(hvla_ctx* ctx, const hvla_weights* w, float* theta, float* context,
                        void* stream);

/* Replaces: ViT.__call__'s DINOv2 branch up to `last_hidden_state[:, 1:]`
 * (hypervla/components/base_vit.py:109-122).  images u8 [B, H, W, 3] -> tokens f32 [B, P, E].   */
int hvla_encode(hvla_ctx* ctx, const uint8_t* images, float* tokens, int32_t B, void* stream);

/* Replaces: the evaluators' `DINO_encode_image(initial_image).last_hidden_state`, the source of
 * initial_state["patch_embeddings"] whose CLS row conditions the hypernetwork
 * (data/simpler/evaluate.py:155-163,264-274; data/libero/evaluate.py:175; scripts/train.py:417-419), run with the
 * DINOv2 weights loaded into this ctx.  images u8 [B, H, W, 3] -> hidden f32 [B, 1 + P, E] (row 0 = CLS).   */
int hvla_encode_hidden(hvla_ctx* ctx, const uint8_t* images, float* hidden, int32_t B, void* stream);

/* Replaces: the rest of BaseNetwork.predict_action with per-episode weights
 * (base_vit.py:130-227, transformer.py:127-262, action_heads.py:431-472,524-538).
 *   tokens f32 [B, P, E] -> actions f32 [B, horizon, action_dim]; gripper_logits f32 [B, horizon]
 *   (nullable; the threshold `logit >= 0` is what column action_dim-1 of `actions` holds).     */
int hvla_policy(hvla_ctx* ctx, const hvla_weights* w, const float* tokens, float* actions,
                float* gripper_logits, int32_t B, void* stream);

/* Replaces: the `intermediates` that sample_actions returns next to the actions (hypervla/model.py:126-137: every attention
 * map, sown at hypervla/components/base_vit.py:117-118 and by flax's attention modules), as far as a caller of the path
 * reads them: InferenceWrapper(save_attention_map=True) keeps exactly two slices
 * (data/utils/hypervla_interface.py:208-217), which the evaluators pickle (data/simpler/evaluate.py:358-378):
 *   dino_cls_attention f32 [B, enc_layers, enc_heads, P]  DINOv2: attention of the CLS query over the P patch keys
 *                                                          (`DINO_attention_map[0][layer][b, :, 0, 1:]`)
 *   head_attention     f32 [B, layers, heads, P]          generated policy: attention of the action token over the P patch
 *                                                          keys (`attention_weights[0][b, :, -1, :-1]`); with
 *                                                          use_language_token [B, layers, heads, lang_tokens + P]: the
 *                                                          language keys first, as the reference's sequence has them
 * Opt-in: the DEVICE buffers registered here (either may be NULL) are written by every following hvla_encode /
 * hvla_policy / hvla_step on this ctx until the call is repeated with NULLs; rows are the episodes of that call.   */
int hvla_set_attention_outputs(hvla_ctx* ctx, float* dino_cls_attention, float* head_attention);

/* Replaces: HyperVLA.sample_actions (hypervla/model.py:85-137): hvla_encode + hvla_policy through
 * the ctx's own token workspace.  B must equal hvla_weights_batch(w).                           */
int hvla_step(hvla_ctx* ctx, const hvla_weights* w, const uint8_t* images, float* actions,
              float* gripper_logits, int32_t B, void* stream);

/* Replaces: the un-normalise + temporal ensemble of InferenceWrapper.step for a batch of
 * episodes (data/utils/hypervla_interface.py:219-253, data/utils/action_ensemble.py:15-27,
 * temperature 0).  Keeps a device ring of the last `horizon` predictions inside `w`.
 *   actions f32 [B, horizon, action_dim] (as written by hvla_policy/step);
 *   mean/std f32 [action_dim], mask u8 [action_dim] (device); out f32 [B, action_dim].
 * The un-normalisation is the affine map a * std + mean on the masked columns.  NormalizationType.NORMAL (:219-230) passes
 * the dataset's mean / std; NormalizationType.BOUNDS (:231-242), (a + 1) (p99 - p01 + 1e-8) / 2 + p01, is the same map with
 * std = (p99 - p01 + 1e-8) / 2 and mean = p01 + std (hypervla.interface.device_unnormalization builds either pair).  */
int hvla_ensemble_reset(hvla_ctx* ctx, hvla_weights* w, void* stream);
int hvla_ensemble(hvla_ctx* ctx, hvla_weights* w, const float* actions, const float* mean,
                  const float* std, const uint8_t* mask, float* out, void* stream);

/* Episode pool: episodes join and leave a running batch (no reference counterpart: the reference runs one episode at a time;
 * hypervla.evaluate.BatchEvaluator.run_episodes drives it).  An arena of B slots; slot s is row s of wh / wl / vf / ctx and of
 * the ensemble ring, and has an ensemble counter of its own.  `slots` is a DEVICE int32 [K] map owned by the caller, K distinct
 * entries in [0, B) (hypervla.pool.check_slots refuses anything else before a map reaches the device); the kernels skip an entry
 * outside [0, B): no load, no store.  Every slot is bit-batch-invariant: a slot's weights, actions and ensemble are bitwise those
 * of the same episode run alone through hvla_generate / hvla_step, whatever else shares the pool or the call.  Apart from
 * hvla_weights_alloc none of these calls allocates or synchronises the host: a pooled step loop can be captured in a hipGraph.
 * hvla_weights_free / hvla_weights_export / hvla_weights_batch take a pool like any arena.
 *
 * hvla_weights_alloc: an arena of B (1 <= B <= max_batch) EMPTY slots (taken from the ctx's freed arenas when one of that size
 * is parked, else allocated): weights and context zero-filled -- stepping a slot that was never assigned is defined and gives
 * finite actions -- and every ensemble counter zero.                                                                         */
int hvla_weights_alloc(hvla_ctx* ctx, int32_t B, hvla_weights** out, void* stream);
/* hvla_generate for K (1 <= K <= min(B, max_batch)) new tasks into slots[0 .. K-1] of w: inputs as hvla_generate's for K
 * episodes.  Writes only those rows of the weights and the context and zeroes those slots' ensemble counters; the rows are
 * bitwise what hvla_generate gives the same tasks.  (With layer_tokens a context row is [NL, ctx_dim], here as everywhere.)           */
int hvla_generate_slots(hvla_ctx* ctx, hvla_weights* w, const int32_t* slots, int32_t K, const float* token_embedding,
                        const int64_t* attention_mask, const float* initial_cls, void* stream);
/* hvla_step for K frames, frame k with the weights of slot slots[k]: images u8 [K, H, W, 3] -> actions f32 [K, horizon,
 * action_dim], gripper_logits f32 [K, horizon] (nullable).  Attention outputs (hvla_set_attention_outputs) have K rows, one per
 * call row.  With hvla_config.streams == 2 and K >= 64 the two halves run on two streams, as hvla_step's.                    */
int hvla_step_slots(hvla_ctx* ctx, const hvla_weights* w, const int32_t* slots, int32_t K, const uint8_t* images,
                    float* actions, float* gripper_logits, void* stream);
/* hvla_ensemble per slot: actions row k (f32 [K, horizon, action_dim]) is the prediction of slot slots[k], out f32 [K, action_dim]
 * its un-normalised ensembled action; each slot counts its own calls since hvla_generate_slots assigned it (or since
 * hvla_weights_alloc / hvla_generate / hvla_ensemble_reset).  A slot's ring rows are those hvla_ensemble uses for that row: an
 * arena is ensembled either through hvla_ensemble or through hvla_ensemble_slots, not both.                                  */
int hvla_ensemble_slots(hvla_ctx* ctx, hvla_weights* w, const int32_t* slots, int32_t K, const float* actions,
                        const float* mean, const float* std, const uint8_t* mask, float* out, void* stream);

/* Weight arenas as values: the way IN that hvla_weights_export is the way out of.  The reference's create_tasks
 * returns a plain `base_params` pytree and sample_actions(base_params=...) runs any pytree of that shape (hypervla/model.py:35-137): a
 * policy kept on disk, the mean of two tasks' policies, a perturbed leaf, one the hypernetwork never produced.  hypervla.model
 * import_tasks / assign_base_params / copy_tasks / load_tasks drive these.  theta is a DEVICE f32 [K, G] in reference leaf order
 * (G = hvla_num_generated; what hvla_weights_export writes), context a device f32 [K, ctx_dim] -- [K, NL, ctx_dim] for a context
 * created with layer_tokens, NL = hvla_num_layer_tokens -- or NULL (zeros: the policy does not read
 * it), token_embedding a device f32 [K, lang_tokens, lang_dim], required iff the context was created with use_language_token (the
 * rows' language prefix is then written from it, as hvla_generate does) and refused otherwise.  Matrix elements are split into
 * hi = bf16(x), lo = bf16(x - hi) exactly as the weight generation splits its f32 results; vector elements are stored as given;
 * padding is zero.  Hence hvla_weights_export after an import returns theta bit for bit on the vector leaves and float(hi) + float(lo)
 * on the matrix leaves, and returns an exported theta unchanged -- but the two HALVES of an exported element are not always those
 * of the arena it came from (0.1 % of elements differ), so a policy re-imported from an export steps close to the original, not
 * bitwise equal: hvla_weights_copy_slots is the bitwise path.  Every imported or copied slot is bit-batch-invariant: it steps as the
 * same row imported alone, and a copied row as its source.  None of these calls needs hvla_load_weights to have run; apart from
 * hvla_weights_import taking an arena (as hvla_generate does: from the ctx's freed arenas when one of that size is parked) none
 * allocates or synchronises the host, so a pooled loop that imports or copies can be captured in a hipGraph.  HVLA_E_STATE: a NULL
 * handle; HVLA_E_SHAPE: NULL theta, tokens missing or given without the option, a count outside its range, an arena allocated for
 * another geometry -- nothing is written then.
 *
 * hvla_weights_import: B (1 <= B <= max_batch) rows of theta into a new arena of B episodes, ensemble counters zero.              */
int hvla_weights_import(hvla_ctx* ctx, const float* theta, const float* context, const float* token_embedding, int32_t B,
                        hvla_weights** out, void* stream);
/* Row k of theta (and of context / token_embedding) into slot slots[k] of w, K in [1, B]; slot maps follow the episode pool's rules.
 * Writes only those rows and zeroes those slots' ensemble counters; every other slot keeps its bytes.                           */
int hvla_weights_import_slots(hvla_ctx* ctx, hvla_weights* w, const int32_t* slots, int32_t K, const float* theta,
                              const float* context, const float* token_embedding, void* stream);
/* Slot src_slots[k] of src into slot dst_slots[k] of dst, K in [1, min(B of dst, B of src)]: weights (with the language prefix) and
 * context byte for byte, the destination's ensemble counter zero; a pair with either entry out of range is skipped.  src and dst may
 * be the same arena only if no slot is in both maps (hypervla.model.copy_tasks checks; the kernel does not).                     */
int hvla_weights_copy_slots(hvla_ctx* ctx, hvla_weights* dst, const int32_t* dst_slots, const hvla_weights* src,
                            const int32_t* src_slots, int32_t K, void* stream);

/* Episode pool post-processing: replaces InferenceWrapper.postprocess (data/utils/hypervla_interface.py:219-304: un-normalisation
 * :219-242, temporal ensemble :250-253 == data/utils/action_ensemble.py:15-27 with temperature 0, euler -> axis-angle :261-267,
 * gripper rules :269-299) for every running episode of a pool at once; hypervla.postprocess.DevicePostprocessor drives it and
 * hypervla.evaluate.BatchEvaluator(postprocess="device") steps its simulators with the result.  A hvla_post holds B slots of
 * caller-side state next to (not inside) an arena: a ring of the last `horizon` un-normalised predictions (f64 [B][horizon]
 * [horizon][7]), a call counter, a table row, an ensemble flag and the sticky-gripper state.  Slot maps follow the episode pool's
 * rules (distinct entries; entries outside [0, B) are skipped).  Only hvla_post_create allocates and only hvla_post_free waits for
 * the device: a pooled loop of hvla_preprocess -> hvla_step_slots -> hvla_post_step can be captured in a hipGraph.
 *
 * The caller owns the table: one hvla_post_row per (policy setup, dataset statistics) pair, in device memory.
 *   HVLA_NORM_NORMAL: p0 = mean, p1 = std;          value = where(mask, a * std + mean, a)
 *   HVLA_NORM_BOUNDS: p0 = p01,  p1 = p99 - p01 + 1e-8 evaluated as the host evaluates it (in the statistics' own dtype);
 *                                                   value = where(mask, (a + 1) * p1 / 2 + p01, a)
 * Arithmetic: f64 in the host's operation order and without contraction, so raw_action and the env action's translation are
 * bitwise numpy's; the rotation (cos / sin / atan2 of the device library) is within 1 ulp after its f32 rounding; the gripper is
 * exact.  A row with a normalisation or setup code not listed here gives NaN outputs and leaves its slot's state alone.          */
#define HVLA_POST_DIM 7             /* action width of every policy setup: xyz, roll pitch yaw, gripper                         */
#define HVLA_NORM_NORMAL 0
#define HVLA_NORM_BOUNDS 1
#define HVLA_SETUP_LIBERO 0         /* gripper 2 g - 1                                                                           */
#define HVLA_SETUP_WIDOWX_BRIDGE 1  /* gripper 2 (g > 0.5) - 1                                                                   */
#define HVLA_SETUP_GOOGLE_ROBOT 2   /* relative gripper action held for 15 calls once |previous - g| > 0.5 (sticky gripper)      */
typedef struct hvla_post hvla_post;
typedef struct hvla_post_row {
  int32_t normalization;            /* HVLA_NORM_*                                                                               */
  int32_t setup;                    /* HVLA_SETUP_*                                                                              */
  double p0[HVLA_POST_DIM], p1[HVLA_POST_DIM];
  uint8_t mask[HVLA_POST_DIM];      /* 1: un-normalise this column                                                              */
} hvla_post_row;
/* B (1 <= B <= max_batch) slots, zeroed: a slot that was never assigned steps with table row 0 and no ensemble.  HVLA_E_SHAPE when
 * the ctx's action_dim is not 7 or its horizon exceeds 16.                                                                     */
int hvla_post_create(hvla_ctx* ctx, int32_t B, hvla_post** out, void* stream);
int hvla_post_free(hvla_ctx* ctx, hvla_post* p);
/* InferenceWrapper.reset (:140-160) of slots[0 .. K-1]: slot slots[k] starts a fresh episode with table row rows[k] and the
 * temporal ensemble on iff ensemble[k] != 0.  rows i32 [K], ensemble u8 [K]: device.  Other slots keep their state.            */
int hvla_post_assign(hvla_ctx* ctx, hvla_post* p, const int32_t* slots, int32_t K, const int32_t* rows, const uint8_t* ensemble,
                     void* stream);
/* One postprocess call for each of K slots: actions f32 [K, horizon, 7] (row k the prediction of slot slots[k], as written by
 * hvla_step_slots); table: n_rows hvla_post_row (device); raw_out f64 [K, 7] (nullable) = raw_action; env_out f64 [K, 7] = the env
 * action: translation f64, rotation and gripper f32 values.  A slot whose row is outside [0, n_rows) is skipped.  Slots left out
 * of the map keep their state.                                                                                                  */
int hvla_post_step(hvla_ctx* ctx, hvla_post* p, const int32_t* slots, int32_t K, const float* actions, const hvla_post_row* table,
                   int32_t n_rows, double* raw_out, double* env_out, void* stream);

/* Replaces: MixActionHead.loss evaluated per sample (vmap of sample_loss_fn) on the policy's outputs
 * (hypervla/components/action_heads.py:474-522, scripts/train.py:326-346): the forward half of the
 * fine-tune step.  actions / logits as written by hvla_policy / hvla_step; target f32 [B, horizon,
 * action_dim] (clipped to +-max_action inside iff hvla_config.clip_target); timestep_mask u8 [B];
 * action_mask u8 [B, horizon, action_dim]; loss f32 [B] = 6 * masked-MSE + masked sigmoid-BCE.     */
int hvla_loss(hvla_ctx* ctx, const float* actions, const float* gripper_logits, const float* target,
              const uint8_t* timestep_mask, const uint8_t* action_mask, float* loss, int32_t B,
              void* stream);

/* Replaces: one fine-tune step of the hypernetwork (scripts/train.py:405-542 `train_step_pmap` without the
 * frozen T5 / initial-image encoders that feed it; octo/utils/train_utils.py:295-443 `create_optimizer`):
 * forward + backward of mean_b MixLoss(policy(theta_b(params), tokens_b), action_b), then (hvla_train_apply)
 * clip-by-global-norm -> AdamW with bf16 first moment and the v5 weight-decay mask -> EMA.  The image encoder is
 * either frozen (`fine_tune_pretrained_image_encoder=False`, the config default: `tokens` come from hvla_encode) or
 * trained (README.md:55; its leaves form the "shared" optimizer group at base_lr / base_weight_decay).  Between the
 * two calls the caller all-reduces `grads` over ranks (RCCL; scripts/train.py:460 `pmean`).
 * Every buffer is DEVICE memory owned by the caller; the flat parameter order is make_train_layout()
 * (csrc/train_layout.h) == hypervla.train.train_param_layout(); sizes from hvla_train_sizes.  Every hvla_train_*
 * entry first asks whether the training path serves the context's geometry: use_language_token without
 * hvla_train_language_tokens(ctx, 1), differential_attention without hvla_train_differential(ctx, 1), more than 8 context, 16 policy or 24 image-encoder layers are HVLA_E_SHAPE before any
 * other argument is looked at.                                                                           */
typedef struct hvla_train_buffers {
  float* params;           /* [n_params]                                                     */
  float* grads;            /* [n_params]  written by hvla_train_step                          */
  void* mu;                /* [n_params]  bf16 first moment                                   */
  float* nu;               /* [n_params]                                                     */
  float* ema;              /* [n_params] or NULL                                              */
  float* theta;            /* [B, G]                                                         */
  float* dtheta;           /* [B, G]                                                         */
  float* work;             /* [workspace_floats]                                              */
  float* loss;             /* [B] per-sample loss                                             */
  float* actions;          /* [B, horizon, action_dim] or NULL                                */
  float* logits;           /* [B, horizon] or NULL                                            */
  float* sqsum;            /* [1] scratch for the global gradient norm                        */
  const uint8_t* wd_mask;  /* [n_params] 1 where decoupled weight decay applies (the caller builds  */
                           /*   the mask of its weight_decay_strategy, train_utils.py:330-375)     */
  const float* params0;    /* [n_encoder] pretrained encoder weights (delta decay) or NULL     */
} hvla_train_buffers;
typedef struct hvla_train_hyper {
  float lr, b1, b2, eps, weight_decay, clip, ema_decay;
  int32_t step, forward_only;
  float base_lr, base_weight_decay; /* optimizer group of the shared DINOv2 leaves               */
  int32_t train_encoder;            /* base_vit.py:67 fine_tune_pretrained_image_encoder        */
} hvla_train_hyper;
/* out = { n_params, G, workspace_floats, n_hypernet }.  With train_encoder the shared DINOv2 leaves
 * (hypervla.config.encoder_leaves order) occupy params[n_hypernet, n_params).                     */
int hvla_train_sizes(hvla_ctx* ctx, int32_t B, int32_t train_encoder, int64_t out[4]);
/* Exactly one of `tokens` (f32 [B, P, E] from hvla_encode: frozen encoder) and `images` (u8 [B, H, W, 3]:
 * DINOv2 runs in f32 inside the step and receives gradients, README.md:55) is non-NULL.          */
int hvla_train_step(hvla_ctx* ctx, const hvla_train_buffers* buf, const float* token_embedding,
                    const int64_t* attention_mask, const float* initial_cls, const float* tokens,
                    const uint8_t* images, const float* target, const uint8_t* timestep_mask,
                    const uint8_t* action_mask, int32_t B, const hvla_train_hyper* hyper, void* stream);
int hvla_train_apply(hvla_ctx* ctx, const hvla_train_buffers* buf, const hvla_train_hyper* hyper, void* stream);
/* Replaces: the point where scripts/train.py:460 `jax.lax.pmean(grads, "batch")` lets XLA overlap the gradient
 * all-reduce with the backward pass.  hvla_train_step finishes `grads` in three contiguous buckets, in this order:
 *   0  the shared DINOv2 leaves  [n_hyper, n_hyper + n_encoder)   (trained encoder only; after the image encoder's backward)
 *   1  the output heads          [offset of W_cat, n_hyper)       (after the weight-generation backward)
 *   2  the context encoder       [0, offset of W_cat)             (end of the step)
 * hvla_train_bucket_ranges writes (offset, length) of buckets 0, 1, 2 into out[6] (length 0 = not produced);
 * hvla_train_wait_bucket makes `stream` (the caller's communication stream) wait until bucket `bucket` of the LAST
 * hvla_train_step is final, without blocking the host: the caller then enqueues its all-reduce of that range there.     */
int hvla_train_bucket_ranges(hvla_ctx* ctx, int32_t train_encoder, int64_t out[6]);
int hvla_train_wait_bucket(hvla_ctx* ctx, int32_t bucket, void* stream);
/* Measurement only (bench.py --finetune `roofline`): while on, every batched GEMM launch of hvla_train_step (the split-bf16
 * kernel that carries ~80 % of the step: forward, input-gradient and weight-gradient products) is bracketed by HIP events on the
 * launch stream.  hvla_train_profile_read returns, since the last read, the summed milliseconds of those launches, their
 * f32-equivalent work (2 M N K each; three bf16 matrix instructions per product on the hardware) and their number.           */
int hvla_train_profile(hvla_ctx* ctx, int32_t on);
int hvla_train_profile_read(hvla_ctx* ctx, float* gemm_ms, double* gemm_flops, int32_t* launches);
/* Replaces: one micro-step of optax.MultiSteps under the reference's chain(clip_by_global_norm, MultiSteps(adamw))
 * (octo/utils/train_utils.py:420-426, grad_accumulation_steps > 1): acc += clip_by_global_norm(buf->grads) * inv_k.
 * After k micro-steps the caller runs hvla_train_apply with `grads` pointing at acc and hyper.clip = +inf.        */
int hvla_train_accumulate(hvla_ctx* ctx, const hvla_train_buffers* buf, float* acc, float inv_k,
                          const hvla_train_hyper* hyper, void* stream);
/* Replaces: `model.replace(params=ema)` between fine-tuning and evaluation (data/simpler/evaluate.py:440-444), without the
 * host: `params` (DEVICE, f32 [n_params] in the flat training order; the parameters and the EMA are both such vectors) is
 * packed in place into every device buffer hvla_load_weights fills -- the context encoder, the W_cat hi / lo fragment planes
 * and b_cat, and with train_encoder != 0 the image encoder's 16-bit matrices, rounding residues and f32 vectors (enc_dtype
 * honoured).  The bytes are those hvla_load_weights writes for the same tensors; with train_encoder == 0 the image encoder's
 * buffers are not touched.  Allocates nothing, does not synchronise with the host, launches only on `stream`; no buffer address
 * changes, so the context's arenas, pools and captured graphs stay valid and read the new weights from their next launch on.
 * Weights generated earlier (hvla_generate) keep their values: they were generated already.  Ordering against work of this
 * context on OTHER streams (a step in flight, a second stream of cfg.streams == 2 is joined by hvla_step itself) is the
 * caller's.  Refused before any launch: not loaded -> HVLA_E_STATE; n_params != hvla_train_sizes(...)[0] for that flag, NULL
 * params, or a use_language_token geometry without hvla_train_language_tokens(ctx, 1) -> HVLA_E_SHAPE.  With it the columns of
 * the two language heads go through the same permutation as every other head's, and create_tasks / assign_tasks after the
 * publish build weights and language prefix from them.                                                                       */
int hvla_train_publish(hvla_ctx* ctx, const float* params, int64_t n_params, int32_t train_encoder, void* stream);

/* Replaces: FlaxDinov2Embeddings.interpolate_pos_encoding, which resizes HF's n x n DINOv2 position table to
 * the run-time grid inside every forward pass, and its transpose under jax.grad: the reference trains the n x n table.
 * hvla_position_interp: src f32 [1 + n n, E] -> dst f32 [1 + P, E], the context's grid and width (dst has no other geometry).  Row 0
 * is copied.  w f32 [n, grid] is the per-axis weight matrix of hypervla.convert._scale_and_translate_weights(n, grid,
 * (grid + 0.1) / n), computed on the host by that function and uploaded by the caller: the library restates no formula.  Height
 * axis first, then width, each in f32 with ascending taps, as convert.bake_position_embeddings; n == grid copies the table.
 * hvla_position_interp_adjoint: dsrc f32 [1 + n n, E] = A^T ddst f32 [1 + P, E] as a gather in ascending (i, j): no atomics,
 * bit-reproducible.  All pointers DEVICE, 16-byte aligned.  HVLA_E_SHAPE: a NULL or misaligned pointer, n < 2.                */
int hvla_position_interp(hvla_ctx* ctx, const float* src, int32_t n, const float* w, float* dst, void* stream);
int hvla_position_interp_adjoint(hvla_ctx* ctx, const float* ddst, int32_t n, const float* w, float* dsrc, void* stream);
/* Train the position table through its interpolation (n >= 2; n == 0 turns it off again, the state of a new context).  w as
 * above, kept by POINTER and owned by the caller for as long as the source is on.  Off, or with train_encoder == 0, every
 * hvla_train_* entry does exactly what it did.  On, with train_encoder != 0:
 *   - the flat vector is [hypernetwork | encoder leaves | source table (1 + n n) E]: hvla_train_sizes reports it, bucket 0 of
 *     hvla_train_bucket_ranges grows by the tail, params0 and wd_mask cover it.  The baked table's slot among the encoder leaves
 *     stays where it is, as a derived quantity;
 *   - hvla_train_step resizes tail -> slot in `params` before the encoder runs, carries the slot's gradient to the tail with the
 *     adjoint after the encoder's backward and zeroes the slot's gradient, all before bucket 0's event;
 *   - hvla_train_apply / hvla_train_accumulate take the norm and the shared group's AdamW over the tail too, then re-derive
 *     the slot of `params` (and of `ema` when the EMA is on) from its tail;
 *   - hvla_train_publish bakes the served position table from the tail of the vector it is given, with the same kernel (the
 *     vector's own slot is not read for it and, like the rest of the vector, not written).                                  */
int hvla_train_position_source(hvla_ctx* ctx, int32_t n, const float* w);
/* Replaces: `create_optimizer(frozen_keys=...)` (octo/utils/train_utils.py:242-292 freeze_weights, applied at :428-439): fnmatch
 * patterns over the parameter tree, wrapped round the whole chain as multi_transform({"trainable": tx, "frozen": set_to_zero()}).
 * The caller resolves the patterns (hypervla.train.frozen_plan) into `frozen`, DEVICE uint8 [n_params], 1 = frozen, kept by
 * POINTER and owned by the caller while set; NULL turns it off again (n_params and frozen_buckets are then ignored), the state of
 * a new context, in which every hvla_train_* entry launches exactly what it launched.  A host-side setting: nothing is launched,
 * hvla_train_buffers / hvla_train_hyper keep their layout.  Set:
 *   - hvla_train_apply / hvla_train_accumulate take the global norm over the trainable elements only (the reference's clip sits
 *     inside the trainable transform); sqsum[0] is that sum.  AdamW, in both groups, neither loads nor stores a frozen element of
 *     params / mu / nu / ema (nor its grads / params0): they keep their bits;
 *   - frozen_buckets: bit b = bucket b of hvla_train_bucket_ranges is frozen as a whole, the caller's declaration.  A bucket
 *     declared frozen is not computed: bit 1 leaves out dW_cat and db_cat, bit 2 everything behind bucket 1's event and the
 *     product dctx = dtheta W_cat^T before it; its range of `grads` stays zero.  All events are recorded where they always are
 *     (hvla_train_wait_bucket keeps working).  If the mask disagrees with the declaration, the bucket's elements see zero
 *     gradients; nothing is read out of bounds either way.  Frozen elements of a computed bucket get their gradients in `grads`;
 *     the optimizer ignores them.
 * HVLA_E_SHAPE at set time: n_params is not hvla_train_sizes(...)[0] for one of the two train_encoder values under the current
 * position source (the value it matches is remembered); bits outside 0..2; bit 0 with the trained encoder's length (that is
 * train_encoder == 0).  HVLA_E_STATE from hvla_train_step (forward-only too), hvla_train_apply and hvla_train_accumulate, before
 * any launch, while a mask is set for the other train_encoder value than hyper->train_encoder (or the position source changed
 * the vector's length since).                                                                                                */
int hvla_train_frozen(hvla_ctx* ctx, const uint8_t* frozen, int64_t n_params, int32_t frozen_buckets);
/* Replaces: the two attention terms of `sample_loss_fn` (scripts/train.py:348-373, config.auxiliary_loss.attention_entropy and
 * .attention_map_alignment), added to every sample's loss after MixActionHead.loss -- so neither the timestep nor the action mask
 * touches them.  Both read the action token's attention row of the LAST policy layer (transformer.py:248-262 returns that block's
 * map): p[h][k], the softmax of query S-1 of head h over all S = P + 1 keys (the row is unmasked).  Per sample b:
 *   ent_b   = 1/H sum_h ( -sum_{k<S} p[h][k] log(p[h][k] + 1e-8) )
 *   m[k]    = 1/H sum_h p[h][k];   align_b = 1/P sum_{k<P} (m[k] - reference_map[b][k])^2
 *   loss_b  = mix_loss_b + entropy_weight ent_b + alignment_weight align_b
 * reference_map is a constant (the reference stops the gradient): DINOv2's last-layer CLS attention over the patches, mean over
 * heads, of the PRETRAINED encoder (scripts/train.py:432-438).  alignment_weight is the effective weight: the caller applies the
 * annealing (1 - step / num_steps) on the host.  The gradient of mean_b loss_b flows through the attention row into everything the
 * step differentiates (with train_encoder != 0 into the shared DINOv2 leaves too, through the policy's keys).
 * A host-side setting kept on the context, like hvla_train_frozen: nothing is launched, pointers are kept by POINTER and stay the
 * caller's while set, hvla_train_buffers / hvla_train_hyper keep their layout and hvla_train_sizes its values (no workspace).
 * While a weight is > 0, hvla_train_step launches one small kernel behind the loss (forward_only too: buf->loss includes the
 * terms, entropy / alignment receive ent_b / align_b -- alignment only while alignment_weight > 0) and once more inside the last
 * policy layer's backward; all sums in a fixed order, no atomics.  With both weights 0, or after opts == NULL (the state of a new
 * context), hvla_train_step launches exactly what it launched.
 * HVLA_E_SHAPE, before anything is stored (the previous setting stays in force): struct_size != sizeof(hvla_train_attention), a
 * negative or non-finite weight, alignment_weight > 0 with a NULL reference_map, a use_language_token context -- whatever
 * hvla_train_language_tokens says: the reference's alignment term compares the action row over lang_tokens + P keys with a P-wide
 * map (scripts/train.py:364-368), which has no defined value, and the entropy term is left out with it.                      */
typedef struct hvla_train_attention {
  uint32_t struct_size;
  float entropy_weight;         /* auxiliary_loss.attention_entropy                                   */
  float alignment_weight;       /* (1 - step/num_steps) * auxiliary_loss.attention_map_alignment      */
  const float* reference_map;   /* device f32 [B, P]; needed iff alignment_weight > 0                  */
  float* entropy;               /* device f32 [B] out, or NULL                                        */
  float* alignment;             /* device f32 [B] out, or NULL                                        */
} hvla_train_attention;
int hvla_train_attention_losses(hvla_ctx* ctx, const hvla_train_attention* opts);   /* NULL: off */
/* Fine-tune a use_language_token context (scripts/train.py:326-346 binds whatever dict_base_params the hypernetwork produced;
 * base_vit.py:159-166,207-214 prepends and masks the projected instruction tokens in training as in inference).  A host-side
 * setting kept on the context, like hvla_train_frozen: nothing is launched, nothing allocated.  on == 0 (always HVLA_OK) is the
 * state of a new context: every hvla_train_* entry refuses a use_language_token context with HVLA_E_SHAPE.  on == 1: they serve
 * it (hvla_train_attention_losses excepted).  The policy then runs on lang_tokens + P + 1 rows per episode: rows [0, lang_tokens)
 * are hvla_train_step's token_embedding through the generated language_token_projection (padded positions included, as in the
 * reference), the mask is the serving path's, head and loss read the last row; the vector holds the two heads' columns in W_cat /
 * b_cat and hvla_train_sizes reports the longer workspace.  Nothing flows into token_embedding (T5 is frozen).
 * The gradient of the generated policy's key biases, zero under any attention mask, is left at exact zeros in `grads` (the
 * heads output_head_*_key_bias): with few language keys the column sum that forms it carried only operand rounding.
 * HVLA_E_SHAPE: on == 1 on a context created without use_language_token; any other value.  NULL ctx: HVLA_E_STATE.           */
int hvla_train_language_tokens(hvla_ctx* ctx, int32_t on);
/* Fine-tune a differential_attention context (hvla_create_with_v3; hypervla/components/differential_transformer.py:99-252 runs in
 * the reference's training loop as it does in inference).  The exact counterpart of hvla_train_language_tokens: a host-side
 * setting kept on the context, nothing launched, nothing allocated.  on == 0 (always HVLA_OK) is the state of a new context: every
 * hvla_train_* entry refuses a differential_attention context with HVLA_E_SHAPE.  on == 1: they serve it.  Every policy block
 * then runs DifferentialAttention forward and backward in f32: the four bias-free projections, the two
 * unscaled softmaxes per head with the mask added, lambda from the episode's own four vectors and the layer's depth, the RMSNorm
 * over a head's 16 values; the gradients of lambda_q1 / k1 / q2 / k2 and subln/weight land in the episode's dtheta row and flow
 * through the output heads like every other leaf, reduced in a fixed order (no floating-point atomics: a sample's loss and dtheta
 * row do not depend on the batch around it).  hvla_train_sizes reports the longer workspace; hvla_train_publish serves the
 * trained vector into the running context.  Refused with HVLA_E_SHAPE and a text on such a context: hvla_train_attention_losses
 * with a weight != 0 (the module's map A1 - lambda A2 is signed: no entropy) and hvla_train_noise_set with a rate or sigma != 0.
 * HVLA_E_SHAPE: on == 1 on a context created without differential_attention; any other value.  NULL ctx: HVLA_E_STATE.       */
int hvla_train_differential(hvla_ctx* ctx, int32_t on);
/* Fine-tune a layer_tokens context (hvla_create_with_v4; hypernet_kwargs.share_layer_index=False, the default of the reference's
 * pretraining config, with or without share_TF_output_head).  A host-side setting kept on the context like the two above.
 * on == 0 (always HVLA_OK) is the state of a new context: every hvla_train_* entry refuses a layer_tokens context with
 * HVLA_E_SHAPE.  on == 1: they serve it.  The training vector then holds layer_pos_embedding as NL rows and
 * the output heads as [C][Gh] / [Gh], Gh <= G (with shared_block_heads the blocks' leaves of one name are one tensor); the context
 * encoder runs forward and backward on T + 1 + NL rows; the weight generation and its two gradients are one grouped launch each,
 * whose tile tables the context keeps in device memory (allocated by the first entry that follows).  hvla_train_sizes reports the
 * longer vector and workspace; hvla_train_publish serves the trained vector into the running context (the heads into the
 * per-token segment blocks).  On a context created without layer_tokens on == 1 is HVLA_OK and changes nothing.
 * HVLA_E_SHAPE: any other value of `on`.  NULL ctx: HVLA_E_STATE.                                                                 */
int hvla_train_layer_tokens(hvla_ctx* ctx, int32_t on);
/* Test instrumentation, like hvla_train_noise_probe: where hvla_train_step at this batch size and train_encoder value (under the
 * current noise setting) leaves the context embedding and its gradient in buffers.work.  out[0], out[1]: the offsets in floats of
 * ctx and d loss / d ctx, each [B][NL][ctx_dim] (NL = hvla_num_layer_tokens); out[2]: their length B NL ctx_dim.  d ctx is what the
 * weight-generation backward wrote (rows of a token no leaf reads are zero); with the context encoder's bucket frozen it is not
 * written.  Errors as hvla_train_sizes.                                                                                           */
int hvla_train_context_rows(hvla_ctx* ctx, int32_t B, int32_t train_encoder, int64_t out[3]);
/* Replaces: the four noise sources the reference's training loop switches on by running the model with train=True --
 * vit_kwargs.dropout_rate (base_vit.py:205; transformer.py:67,74,192), vit_kwargs.image_embedding_noise (base_vit.py:123-127),
 * hypernet_kwargs.embedding_dropout_rate (hypernetwork.py:193-195) and hypernet_kwargs.image_dropout (hypernetwork.py:119-122).
 * Deviation: the random bits are not jax's threefry bits; the noise is EQUAL IN DISTRIBUTION to the reference's, not bit-equal.
 * It comes from a counter-based generator with no state and no stored masks (csrc/noise.h): Philox4x32-10 with key = seed and
 * counter = (element >> 2, sample_offset + b, site, draw), element e taking word e & 3 of its block; the backward pass regenerates
 * what the forward pass drew, and hypervla.train.philox4x32 restates it on the host bit for bit.
 *   dropout: keep iff (word >> 8) >= ceil(rate 2^24); y = x / (1.0f - rate) where kept, else 0 (flax divides)
 *   normals: Box-Muller on the word pairs (w0, w1), (w2, w3): u1 = ((w >> 8) + 1) 2^-24, u2 = (w' >> 8) 2^-24,
 *            z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2)
 * site = kind | layer << 8, element index row-major over the per-sample shape:
 *   1 policy input after + pos_embedding [S, dim] (S includes the language prefix)      policy_dropout
 *   2 layer l: attention branch behind out-projection and bias [S, dim]                  policy_dropout
 *   3 layer l: behind the GELU [S, mlp]                                                  policy_dropout
 *   4 layer l: MLP output in front of the residual add [S, dim]                          policy_dropout
 *   5 DINOv2 tokens in front of image_embedding_projection, tokens + sigma z [P, enc_dim]  image_embedding_noise
 *   6 context embedding behind the scale_context division [ctx_dim]                      context_dropout
 *   7 the initial image's CLS row in front of initial_image_projection [enc_dim]         image_dropout
 * The context encoder's and DINOv2's blocks draw nothing (context_encoder_kwargs.dropout_rate, attention-probability dropout and
 * hypernet_kwargs.final_dropout_rate are not built); a forward_only hvla_train_step draws nothing; the serving entries draw nothing.
 * A sample's noise depends on its GLOBAL index sample_offset + b (low 32 bits), never on its row or on what shares the batch.
 * `draw` is the caller's: bump it before every hvla_train_step, or two steps draw the same masks.  A captured graph replays the
 * `draw` (and seed and offset) it was captured with: the values are kernel arguments.
 * A host-side setting kept BY VALUE on the context, like hvla_train_frozen: nothing is launched.  A site whose rate is 0 launches
 * nothing; with every rate 0, or after opts == NULL (the state of a new context), hvla_train_step launches exactly what it
 * launched and hvla_train_sizes returns what it returned.  While image_embedding_noise > 0 with a frozen encoder, or image_dropout
 * > 0, the step keeps a noisy copy in the workspace and hvla_train_sizes reports the larger size: make the setting BEFORE asking
 * for sizes.  The step then reads `tokens` / `cls` 16 bytes at a time: a pointer that is not 16-byte aligned is HVLA_E_SHAPE.
 * While policy_dropout > 0 the gradient of the generated policy's key biases, zero under any mask, is left at exact zeros in
 * `grads`, as under hvla_train_language_tokens.
 * HVLA_E_SHAPE, with nothing stored and the previous setting in force: struct_size != sizeof(hvla_train_noise); a dropout rate
 * outside [0, 1) or non-finite; a negative or non-finite image_embedding_noise.  NULL ctx: HVLA_E_STATE.                      */
typedef struct hvla_train_noise {
  uint32_t struct_size;
  float policy_dropout;         /* vit_kwargs.dropout_rate                                             */
  float image_embedding_noise;  /* vit_kwargs.image_embedding_noise (sigma)                            */
  float context_dropout;        /* hypernet_kwargs.embedding_dropout_rate                              */
  float image_dropout;          /* hypernet_kwargs.image_dropout                                       */
  uint64_t seed;
  int64_t sample_offset;        /* global index of row 0 (rank * B under data parallelism)             */
  uint32_t draw;                /* the caller bumps it before every hvla_train_step                    */
} hvla_train_noise;
int hvla_train_noise_set(hvla_ctx* ctx, const hvla_train_noise* opts);   /* NULL: off, the state of a new context */

/* Replaces: the `metrics` of MixActionHead.loss (hypervla/components/action_heads.py:517-521: `continuous_loss`, `gripper_loss`) per
 * sample, and the numerator of `validation_action_loss` (scripts/train.py:578-581).  Arguments as hvla_loss (actions / gripper_logits
 * as hvla_train_step, hvla_policy or hvla_step wrote them); all outputs device f32 [B]:
 *   continuous[b] = (action_dim - 1) * masked-MSE,  gripper[b] = masked sigmoid-BCE  -- the two terms whose sum hvla_loss and
 *                   hvla_train_step store (same expressions: the 1e-5 floor on the mask means, the target clipped to +-max_action
 *                   iff hvla_config.clip_target, log1p(exp(-|z|))), summed in the order of the step's own loss kernel;
 *   sqerr[b]      = sum_{h,a} (actions - clip(target, -5, 5))^2 over every step and dimension, NO mask, the gripper column being the
 *                   0 / 1 threshold `actions` holds; the clip is the literal +-5 of scripts/train.py:580, not max_action.  Accumulated
 *                   in f64, rounded once.  `mse` of the reference = mean_b sqerr[b] / horizon (its `.mean() * action_dim`).
 * No allocation, no host synchronisation, bit-reproducible.  HVLA_E_SHAPE: B < 1, a NULL pointer.                                   */
int hvla_loss_terms(hvla_ctx* ctx, const float* actions, const float* gripper_logits, const float* target,
                    const uint8_t* timestep_mask, const uint8_t* action_mask, float* continuous, float* gripper, float* sqerr,
                    int32_t B, void* stream);

/* Replaces: the `info` dict of `train_step_pmap` (scripts/train.py:494-529: training_loss, grad_norm, update_norm, param_norm, the
 * per-sample `metrics` of sample_loss_fn :346-384 averaged, `task_loss_<name>` :455-456,522-525) and `param_norm_callable`
 * (octo/utils/train_utils.py:437-441), computed on the device from the buffers of the step -- nothing is copied to the host.
 * out (device f32 [HVLA_METRIC_N + 2 n_tasks]), one HVLA_METRIC_* index per slot:
 *   the rank-local block [0, HVLA_METRIC_LOCAL_N): means over the B samples of this rank --
 *     TRAINING_LOSS = mean buf->loss;  CONTINUOUS_LOSS, GRIPPER_LOSS = means of hvla_loss_terms' terms on buf->actions / buf->logits;
 *     MSE = mean_b sqerr[b] / horizon;  BASE_PARAMS_NORM = mean_b sqrt(sum theta_b^2 + enc_sq), enc_sq the sum of squares of the shared
 *     DINOv2 leaves every sample's dict_base_params carries (scripts/train.py:384): with train_encoder taken from buf->params (the
 *     position table as its source while hvla_train_position_source is on, else as the baked table), else `encoder_sqsum`;
 *     ATTENTION_ENTROPY, ATTENTION_ALIGNMENT = means of `entropy` / `alignment`;
 *   then n_tasks sums  sum_b loss[b] [task_ids[b] == t]  and n_tasks counts (the reference divides after its psum; an id outside
 *     [0, n_tasks) is counted nowhere, the episode pool's skip rule);
 *   then the replicated block (equal on every rank after the gradient all-reduce), at HVLA_METRIC_<NAME> + 2 n_tasks:
 *     GRAD_NORM  = |buf->grads|, EVERY element as it stands (optax.global_norm(grads) of the averaged gradient, before the clip):
 *                  frozen elements of a computed bucket included.  Deviation: a bucket DECLARED frozen (hvla_train_frozen) was not
 *                  computed and contributes zeros, where the reference's norm includes its gradient.  The baked position slot's
 *                  gradient is zero by construction.  buf->sqsum[0], the clip's own sum, is f32 with atomics and over trainable
 *                  elements only: it differs from GRAD_NORM^2 by that rounding (and by the frozen elements);
 *     PARAM_NORM = |buf->params| without the elements whose frozen byte is set (param_norm_callable zeroes frozen leaves) and, while
 *                  the position source is on, without the baked slot (a derived quantity; the source tail is the parameter);
 *     UPDATE_NORM = |buf->params - prev_params| without the baked slot: optax.global_norm(updates), delta decay included; zero on a
 *                  micro-step of gradient accumulation that moved nothing.
 * select: HVLA_METRICS_PRE fills everything but UPDATE_NORM (call it after the gradient all-reduce and before hvla_train_apply: the
 * reference logs param_norm of the parameters before the update); HVLA_METRICS_UPDATE fills UPDATE_NORM (after hvla_train_apply, with
 * prev_params the snapshot taken before it).  A slot that is not selected, or whose inputs are NULL (target / masks / buf->actions /
 * buf->logits for the three loss terms, buf->theta, entropy, alignment, task_ids), is not written.
 * Every sum runs in a fixed order without atomics, in f64, rounded to f32 once: `out` is a function of the data alone and each value
 * within one f32 rounding of the exact one.  Allocates nothing, does not synchronise with the host, launches on `stream` only,
 * writes only `out` and `scratch` (HVLA_TRAIN_METRICS_SCRATCH_DOUBLES doubles, contents undefined between calls); may be captured.
 * Follows the hvla_train_* rules: the geometry refusal first, the position source and the frozen mask held on the context are
 * honoured, HVLA_E_STATE while the mask was set for the other train_encoder value.  HVLA_E_SHAPE before any launch: struct_size !=
 * sizeof(hvla_train_metrics_in), NULL scratch or out, NULL buf->params or buf->grads, B outside [1, HVLA_TRAIN_METRICS_MAX_BATCH],
 * select without a bit of HVLA_METRICS_PRE | HVLA_METRICS_UPDATE or with another, UPDATE without prev_params, n_tasks < 0, task_ids
 * given with n_tasks == 0, a scratch that is not 16-byte aligned.                                                                  */
#define HVLA_METRICS_PRE 1u
#define HVLA_METRICS_UPDATE 2u
#define HVLA_METRIC_TRAINING_LOSS 0
#define HVLA_METRIC_CONTINUOUS_LOSS 1
#define HVLA_METRIC_GRIPPER_LOSS 2
#define HVLA_METRIC_MSE 3
#define HVLA_METRIC_BASE_PARAMS_NORM 4
#define HVLA_METRIC_ATTENTION_ENTROPY 5
#define HVLA_METRIC_ATTENTION_ALIGNMENT 6
#define HVLA_METRIC_LOCAL_N 7              /* the rank-local block; task sums at [7, 7 + n_tasks), counts behind them      */
#define HVLA_METRIC_GRAD_NORM 7            /* + 2 n_tasks                                                                  */
#define HVLA_METRIC_PARAM_NORM 8           /* + 2 n_tasks                                                                  */
#define HVLA_METRIC_UPDATE_NORM 9          /* + 2 n_tasks                                                                  */
#define HVLA_METRIC_N 10
#define HVLA_TRAIN_METRICS_WORKGROUPS 1024 /* the norm pass's grid, whatever n_params is                                   */
#define HVLA_TRAIN_METRICS_MAX_BATCH 4096
/* partial sums 4 x WORKGROUPS | 8 totals | row sums, squared errors and the two loss terms, MAX_BATCH each                    */
#define HVLA_TRAIN_METRICS_SCRATCH_DOUBLES (4 * HVLA_TRAIN_METRICS_WORKGROUPS + 8 + 3 * HVLA_TRAIN_METRICS_MAX_BATCH)
typedef struct hvla_train_metrics_in {
  uint32_t struct_size;            /* = sizeof(hvla_train_metrics_in): the exact-size rule of hvla_policy_options         */
  uint32_t select;                 /* HVLA_METRICS_PRE | HVLA_METRICS_UPDATE                                               */
  const float* prev_params;        /* device f32 [n_params]: params before hvla_train_apply; needed for UPDATE             */
  const float* target;             /* as given to hvla_train_step, or NULL                                                 */
  const uint8_t* timestep_mask;
  const uint8_t* action_mask;
  const int32_t* task_ids;         /* device i32 [B] in [0, n_tasks), or NULL                                              */
  int32_t n_tasks;
  const float* entropy;            /* device f32 [B]: hvla_train_attention_losses' outputs, or NULL                        */
  const float* alignment;
  double encoder_sqsum;            /* frozen encoder: sum of squares of the shared DINOv2 leaves; ignored with train_encoder */
  double* scratch;                 /* device, HVLA_TRAIN_METRICS_SCRATCH_DOUBLES doubles, 16-byte aligned                  */
} hvla_train_metrics_in;
int hvla_train_metrics(hvla_ctx* ctx, const hvla_train_buffers* buf, const hvla_train_metrics_in* in, float* out, int32_t B,
                       int32_t train_encoder, void* stream);

/* Replaces: InferenceWrapper._resize_image (data/utils/hypervla_interface.py:89-121): optionally
 * tf.image.resize_with_pad(image, 256, 320) (bilinear, zero padding; `padded_resize`), then
 * tf.image.resize(lanczos3, antialias=True) to image_size x image_size, optionally the centred sqrt(0.9)
 * tf.image.crop_and_resize (bilinear), then round / clip / uint8.  frames u8 [B, H, W, 3] (device) ->
 * images u8 [B, image_size, image_size, 3] (device), the input of hvla_step / hvla_encode_hidden.
 * flags: HVLA_PREPROCESS_CROP | HVLA_PREPROCESS_PAD.                                                              */
#define HVLA_PREPROCESS_CROP 1
#define HVLA_PREPROCESS_PAD 2
int hvla_preprocess(hvla_ctx* ctx, const uint8_t* frames, int32_t B, int32_t H, int32_t W, int32_t flags, uint8_t* images,
                    void* stream);

/* Replaces: the frozen instruction encoder `LanguageTokenizer('t5-base')` that produces
 * task["language_instruction"]["token_embedding"] (octo/model/components/tokenizers.py:186-211;
 * data/utils/language_tokenizer.py:9-28; scripts/train.py:407-415 runs it inside every training step):
 * FlaxT5EncoderModel(config).module(input_ids, attention_mask).last_hidden_state.  Optional: load once, then
 * input_ids / attention_mask i64 [B, T] (device) -> token_embedding f32 [B, T, d_model] (device), ready for
 * hvla_generate.  Tensors are named as in the flax tree ('/'-joined, kernels [in, out]; an `hf_model/` prefix is
 * accepted); d_model must equal the hypernetwork's lang_dim.  Tokenisation (SentencePiece) stays on the host.      */
typedef struct hvla_t5_config {
  int32_t vocab, d_model, d_kv, heads, d_ff, layers, buckets, max_distance;
  float eps;
  int32_t max_tokens, max_batch;
} hvla_t5_config;
int hvla_t5_load(hvla_ctx* ctx, const hvla_t5_config* cfg, const hvla_tensor_desc* tensors, int32_t n);
int hvla_t5_encode(hvla_ctx* ctx, const int64_t* input_ids, const int64_t* attention_mask, float* token_embedding,
                   int32_t B, int32_t T, void* stream);

/* Live per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 *   mode 0: off (default);  1: only the selected categories (hvla_profile_select; the encoder fc1 GEMM unless told otherwise);  2: every category.
 * hvla_profile_read synchronises the recorded events, adds their durations per category into
 * ms[HVLA_PROF_N] / launches[HVLA_PROF_N], and clears the event pool.                            */
#define HVLA_PROF_PATCH 0   /* im2col + patch-embedding GEMM + CLS rows */
#define HVLA_PROF_LN 1      /* encoder LayerNorms                       */
#define HVLA_PROF_QKV 2     /* encoder QKV GEMM                         */
#define HVLA_PROF_ATTN 3    /* encoder attention                        */
#define HVLA_PROF_OUT 4     /* encoder out-projection GEMM (+residual)  */
#define HVLA_PROF_FC1 5     /* encoder fc1 GEMM (+erf GELU)             */
#define HVLA_PROF_FC2 6     /* encoder fc2 GEMM (+residual)             */
#define HVLA_PROF_POLICY 7  /* generated-policy megakernel              */
#define HVLA_PROF_COMP 8    /* encoder: the small launches in front of each big GEMM -- mean rows of its activation operand and the 2 B
                               latency-bound rows (B CLS rows + B rows that compensate the weight rounding)                      */
#define HVLA_PROF_N 9
int hvla_profile(hvla_ctx* ctx, int32_t mode);
int hvla_profile_read(hvla_ctx* ctx, float* ms, int32_t* launches);
/* Which categories mode 1 times: bit c = HVLA_PROF_c (default 1 << HVLA_PROF_FC1).  bench.py first reads a mode-2 pass, then selects
 * the categories of the kernel symbol with the largest share of the step (round 6: out + fc2 run one instantiation) for the events
 * inside its timed region.  A mask with a bit at or above HVLA_PROF_N, or zero, is HVLA_E_SHAPE.                                   */
int hvla_profile_select(hvla_ctx* ctx, uint32_t category_mask);

/* Measurement only (bench.py).  hvla_launches: kernel launches (and memset nodes) the ctx has enqueued since the last call
 * -- hvla_encode / hvla_policy / hvla_step / hvla_ensemble count themselves -- so that "launches per step" is what the library
 * did, not a restatement of its host logic.  hvla_box_probe: what THIS device sustains right now, in a probe kernel of its own
 * (never inside a product kernel): out[0] = shader clock in MHz under a chip-wide matrix-core loop (shader-clock ticks per tick of
 * the constant 100 MHz clock), out[1] = that loop's TFLOP/s (dense fp16 v_mfma_f32_32x32x16, eight waves per CU), out[2] = its
 * duration in ms.  The boxes of a pool differ by several per cent: a step time is read against these.                        */
int64_t hvla_launches(hvla_ctx* ctx);
int hvla_box_probe(hvla_ctx* ctx, float out[3], void* stream);

/* Test instrumentation: hvla_encode with a range audit of every 16-bit MFMA operand the encoder writes, over all layers:
 * site 0 LayerNorm outputs, 1 stored q / k / v, 2 attention outputs, 3 GELU outputs.  maxabs f32 [4] = largest finite
 * |value| per site, nonfinite i32 [4] = number of inf / NaN values (an fp16 overflow shows up here).  HOST pointers.    */
int hvla_encode_audit(hvla_ctx* ctx, const uint8_t* images, int32_t B, float* maxabs, int32_t* nonfinite, void* stream);
/* Test instrumentation: what hvla_train_step draws under the current hvla_train_noise_set setting (seed, draw, rates) for the sample
 * whose global index is sample_id, at `site` = kind | layer << 8: out (DEVICE f32 [n]) receives the multipliers of elements [0, n)
 * of a dropout site (0 or 1 / keep_prob; all 1 / 1 when the site's rate is 0) or, for kind 5, the n normals z (not sigma z).
 * HVLA_E_STATE without a setting; HVLA_E_SHAPE for a kind outside 1..7, n outside [1, 2^24] or a NULL out.                         */
int hvla_train_noise_probe(hvla_ctx* ctx, uint32_t site, int64_t sample_id, int64_t n, float* out, void* stream);

/* Primitive self-check used by tests: runs the MFMA fragment-layout probes on the ctx's device
 * and returns HVLA_OK only if every probe matches its exact integer expectation.                */
int hvla_selftest(hvla_ctx* ctx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HVLA_H_ */
