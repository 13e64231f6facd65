// train_trace_driver.h -- what the two CPU drivers of csrc/train.hip's -DHVLA_TRAIN_TRACE seam share (tools/train_launch_trace.hip,
// tools/train_extent_trace.hip): the fake buffers, the two base geometries, one traced point and the recorded sweep.
#pragma once
#include <cstdio>
#include <vector>

#include "train.h"

namespace hvla {
void* train_trace_buffer(const char* name);
void train_trace_plan(const Geom& g, int B, bool train_encoder, const TrainNoise& nz);
}
using namespace hvla;

template <class T> static T* buf(const char* name) { return static_cast<T*>(train_trace_buffer(name)); }

static Geom mid() {      // the MID geometry of the tests
  Geom g{112, 14, 128, 2, 2, 512, 64, 2, 4, 128, 4, 7, 5.f, 5.f, 128, 2, 4, 256, 12, 64, 1};
  return g;
}
static Geom readme2() {  // the README widths with two encoder layers
  Geom g = mid();
  g.image_size = 224; g.E = 768; g.enc_heads = 12; g.enc_mlp = 3072; g.L = 4; g.ctx_layers = 6; g.ctx_mlp = 512; g.T = 32; g.lang_dim = 768;
  return g;
}

struct Point {
  const char* geom; Geom g; int B;
  int enc;               // 0 encoder frozen, 1 trained, 2 trained with a position source (n = 16)
  int forward_only, frozen_buckets, frozen_mask;
  int aux;               // 0 off, 1 entropy only, 2 both
  float ema_decay, base_wd;
  int noise = 0;         // 1: hvla_train_noise with all four knobs on (the title then ends in noise=1)
};

// plan: also print the size of every buffer a launch may point into and the workspace plan (train_trace_plan), and stop behind
// train_step -- what tests/test_train_workspace_extents.py reads.  Without it: the lines of tests/native/train_step_trace.txt.
static int run(const Point& p, bool plan = false) {
  const Geom& g = p.g;
  printf("# %s L=%d ctx_layers=%d enc_layers=%d B=%d enc=%d forward_only=%d frozen_buckets=%d frozen=%d aux=%d ema=%g base_wd=%g%s\n", p.geom, g.L,
         g.ctx_layers, g.enc_layers, p.B, p.enc, p.forward_only, p.frozen_buckets, p.frozen_mask, p.aux, (double)p.ema_decay, (double)p.base_wd,
         p.noise ? " noise=1" : "");
  const bool enc = p.enc != 0;
  TrainOptions opt;
  if (p.noise) {
    opt.noise.policy_dropout = opt.noise.context_dropout = opt.noise.image_dropout = 0.25f;
    opt.noise.sigma = 0.1f;
    opt.noise.key.k0 = 7; opt.noise.key.draw = 3; opt.noise.key.sample0 = 8;
  }
  printf("workspace %zu\n", train_workspace_floats(g, p.B, enc, opt.noise));
  TrainBuffers tb{buf<float>("params"), buf<float>("grads"), buf<__bf16>("mu"), buf<float>("nu"), buf<float>("ema"), buf<float>("theta"),
                  buf<float>("dtheta"), buf<float>("work"), buf<float>("loss"), buf<float>("actions"), buf<float>("logits"), buf<float>("sqsum"),
                  buf<uint8_t>("wd_mask"), enc ? buf<float>("params0") : nullptr};
  TrainInputs in{buf<float>("tok"), buf<int64_t>("attn_mask"), buf<float>("cls"), enc ? nullptr : buf<float>("tokens"),
                 enc ? buf<uint8_t>("images") : nullptr, buf<float>("target"), buf<uint8_t>("tmask"), buf<uint8_t>("amask")};
  TrainHyper hp{1e-3f, 0.9f, 0.999f, 1e-8f, 0.01f, 1.f, p.ema_decay, 3, p.forward_only, 1e-4f, p.base_wd};
  if (p.enc == 2) { opt.ps.n = 16; opt.ps.w = buf<float>("pos_w"); opt.ps.grid = g.grid(); opt.ps.E = g.E; }
  AttnAux& aux = opt.aux;
  if (p.aux >= 1) { aux.w_ent = 0.25f; aux.ent = buf<float>("aux_ent"); }
  if (p.aux >= 2) { aux.w_align = 0.5f; aux.ref = buf<float>("aux_ref"); aux.align = buf<float>("aux_align"); }
  opt.frozen_buckets = p.frozen_buckets;
  opt.frozen = p.frozen_mask ? buf<uint8_t>("frozen") : nullptr;
  hipEvent_t ev[3];
  for (int i = 0; i < 3; ++i) ev[i] = reinterpret_cast<hipEvent_t>(buf<char>("event") + i);
  hipStream_t st = reinterpret_cast<hipStream_t>(buf<char>("st"));
  if (train_refusal(g, true, true, true)) { printf("refused: %s\n", train_refusal(g, true, true, true)); return 1; }     // (a use_language_token, differential or layer_tokens point is one that asked)
  const TrainLayout L = make_train_layout(g);
  if (!L.policy_ok) { printf("a policy leaf was not found\n"); return 1; }
  std::vector<BGTile> tiles;
  if (g.layer_tokens) opt.groups = token_groups(g, L, buf<BGTile>("tiles"), tiles);
  if (plan) {
    const long n = train_vector_elems(L, opt.ps, enc);
    printf("size params %ld\nsize grads %ld\nsize theta %ld\nsize dtheta %ld\n", n, n, (long)p.B * L.G, (long)p.B * L.G);
    printf("size tok %ld\nsize cls %ld\nsize tokens %ld\n", (long)p.B * g.T * g.lang_dim, (long)p.B * g.E, enc ? 0L : (long)p.B * g.P() * g.E);
    if (g.layer_tokens) printf("size tiles %zu\n", tiles.size());
    train_trace_plan(g, p.B, enc, opt.noise);
  }
  printf("step\n");
  (void)train_step(g, L, tb, in, p.B, hp, st, p.forward_only ? nullptr : ev, opt);
  if (p.forward_only || plan) return 0;
  printf("accumulate\n");
  (void)train_accumulate(L, tb, buf<float>("acc"), 0.5f, hp, enc, st, opt);
  printf("apply\n");
  (void)train_apply(L, tb, hp, enc, st, opt);
  return 0;
}

// the sweep tests/native/train_step_trace.txt was recorded over
static const std::vector<Point>& recorded_sweep() {
  static const std::vector<Point> sweep = [] {
    Geom l16 = mid(), l1 = mid();
    l16.L = 16; l16.ctx_layers = 0;
    l1.L = 1; l1.ctx_layers = 8;
    return std::vector<Point>{
        // geometry          B  enc fwd fb mask aux ema    base_wd
        {"MID", mid(), 1, 2, 0, 0, 0, 2, 0.999f, 0.05f},
        {"MID", mid(), 5, 0, 0, 2, 1, 0, 0.f, 0.f},
        {"MID", mid(), 32, 1, 0, 0, 1, 1, 0.f, 0.05f},
        {"MID", mid(), 32, 2, 1, 0, 0, 2, 0.f, 0.f},
        {"README2", readme2(), 2, 0, 0, 4, 1, 0, 0.999f, 0.f},
        {"README2", readme2(), 8, 1, 0, 6, 1, 0, 0.f, 0.f},
        {"README2", readme2(), 32, 2, 0, 4, 0, 1, 0.999f, 0.05f},
        // the layer-count edges, forward only (a block's backward is the same text for every layer; the per-layer offsets are
        // tests/native/train_layout_check.cpp's)
        {"MID-L16", l16, 1, 0, 1, 0, 0, 2, 0.f, 0.f},
        {"MID-L1", l1, 5, 0, 1, 0, 0, 0, 0.f, 0.f},
    };
  }();
  return sweep;
}
