// train_extent_trace.hip -- CPU only, like tools/train_launch_trace.hip: the fine-tune step's launches at the EDGES of the accepted
// set (csrc/accept.h minus train_refusal), each with the workspace plan in front of it, so that a host check can hold every GEMM
// operand, copy and memset to the plan's buffers (tests/test_train_workspace_extents.py).  Build and run:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -DHVLA_TRAIN_TRACE -I hyper-vla_amd/csrc tools/train_extent_trace.hip hyper-vla_amd/csrc/train.hip -o train_extent_trace
//
// Per point: the `#` line, `workspace <floats>`, `size <buffer> <elements>` for the buffers whose length the layout gives,
// `plan <name> <offset> <floats>` per buffer of make_plan, `step`, then the step's lines.  The cases are those of
// tests/test_gpu_train_geometry.py (same names), each with the encoder frozen and trained, at its GPU batch size and at B = 1;
// MID, the README widths and the recorded sweep of tests/native/train_step_trace.txt are the controls.
#include <vector>

#include "train_trace_driver.h"

static Geom full1() {    // the README widths with one layer of each kind
  Geom g = readme2();
  g.enc_layers = g.L = g.ctx_layers = 1;
  return g;
}
static Geom readme() {
  Geom g = readme2();
  g.enc_layers = 12;
  return g;
}

struct Case { const char* name; Geom g; int B; };

int main() {
  std::vector<Case> cases;
  auto add = [&](const char* name, Geom base, int B, auto change) { change(base); cases.push_back({name, base, B}); };
  add("MID", mid(), 4, [](Geom&) {});
  add("README", readme(), 2, [](Geom&) {});
  // encoder frozen on the GPU
  add("P1", mid(), 5, [](Geom& g) { g.M = 32; });
  add("P2", mid(), 5, [](Geom& g) { g.M = 160; g.L = 3; });
  add("P3", mid(), 5, [](Geom& g) { g.horizon = 1; });
  add("P4", mid(), 5, [](Geom& g) { g.horizon = 4; g.action_dim = 8; });
  add("P5", mid(), 5, [](Geom& g) { g.horizon = 16; g.action_dim = 2; g.ctx_layers = 0; });
  add("P6", full1(), 2, [](Geom& g) { g.M = 32; });
  add("C1", mid(), 5, [](Geom& g) { g.T = 2; });
  add("C1n", mid(), 5, [](Geom& g) { g.T = 2; g.C = 32; g.ctx_heads = 8; g.ctx_mlp = 16; });
  add("C2", mid(), 5, [](Geom& g) { g.T = 38; g.lang_dim = 20; });
  add("C3", mid(), 5, [](Geom& g) { g.T = 15; g.ctx_mlp = 48; });
  add("C4", mid(), 5, [](Geom& g) { g.C = 128; g.ctx_heads = 1; });
  add("C5", mid(), 5, [](Geom& g) { g.lang_dim = 392; });
  // encoder trained on the GPU
  add("E1", mid(), 5, [](Geom& g) { g.E = 256; g.enc_heads = 4; g.enc_mlp = 128; });
  add("E1-B128", mid(), 128, [](Geom& g) { g.E = 256; g.enc_heads = 4; g.enc_mlp = 128; });
  add("E2", mid(), 3, [](Geom& g) { g.E = 640; g.enc_heads = 10; g.enc_mlp = 384; });
  add("E3", mid(), 5, [](Geom& g) { g.patch = 4; g.image_size = 32; });
  add("E4", mid(), 3, [](Geom& g) { g.patch = 16; g.image_size = 128; });
  add("E5", full1(), 2, [](Geom& g) { g.patch = 7; g.image_size = 112; });
  add("E6", full1(), 2, [](Geom& g) { g.E = 1024; g.enc_heads = 16; g.enc_mlp = 128; });
  add("E7", full1(), 3, [](Geom& g) { g.E = 128; g.enc_heads = 2; g.enc_mlp = 128; g.enc_layers = 2; });
  add("E8", full1(), 2, [](Geom& g) { g.enc_layers = 0; });
  add("E9", full1(), 9, [](Geom& g) { g.E = 256; g.enc_heads = 4; g.enc_mlp = 640; });
  for (const Case& c : cases)
    for (int enc = 0; enc < 2; ++enc)
      for (int B : {c.B, 1}) {
        if (B == 1 && c.B == 1) continue;
        if (run(Point{c.name, c.g, B, enc, 0, 0, 0, 0, 0.f, 0.f}, true)) return 1;
      }
  for (const Point& p : recorded_sweep())
    if (run(p, true)) return 1;
  // hvla_train_noise with all four knobs on at MID, encoder frozen and trained (tests/test_train_noise_host.py): the residual
  // branches go through t.y, the token and CLS copies sit behind the rest of the plan
  for (int enc = 0; enc < 2; ++enc)
    if (run(Point{"MID", mid(), 4, enc, 0, 0, 0, 0, 0.f, 0.f, 1}, true)) return 1;
  return 0;
}
