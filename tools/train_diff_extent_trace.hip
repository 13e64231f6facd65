// train_diff_extent_trace.hip -- CPU only, beside tools/train_bias_extent_trace.hip: the fine-tune step's launches and workspace plan
// for use_differential_transformer geometries (Geom::differential), whose policy blocks have nine attention leaves
// without biases, 2 H softmax tables per block, and the buffers DifferentialAttention's backward keeps (pa, oraw, t.dP, t.t2).
// tests/test_diff_train_host.py holds every operand to the plan's buffers with the rules of tests/test_train_workspace_extents.py.
// Build and run:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -DHVLA_TRAIN_TRACE -I hyper-vla_amd/csrc tools/train_diff_extent_trace.hip hyper-vla_amd/csrc/train.hip -o train_diff_extent_trace
//
// The cases are those of tests/test_gpu_diff_train.py: MID at B = 4 and B = 1, the README widths at B = 2, each with the encoder
// frozen and trained.  The last two points are flag-OFF: MID at B = 4, frozen and trained, under the title and with the arguments
// tools/train_extent_trace.hip gives them, so that a test can hold the two outputs equal line for line.
#include <vector>

#include "train_trace_driver.h"

struct Case { const char* name; Geom g; int B; };

int main() {
  std::vector<Case> cases;
  auto add = [&](const char* name, Geom base, int B) { base.differential = 1; cases.push_back({name, base, B}); };
  add("MID-diff", mid(), 4);
  add("MID-diff", mid(), 1);
  add("README2-diff", readme2(), 2);
  for (const Case& c : cases)
    for (int enc = 0; enc < 2; ++enc)
      if (run(Point{c.name, c.g, c.B, enc, 0, 0, 0, 0, 0.f, 0.f}, true)) return 1;
  for (int enc = 0; enc < 2; ++enc)
    if (run(Point{"MID", mid(), 4, enc, 0, 0, 0, 0, 0.f, 0.f}, true)) return 1;
  return 0;
}
