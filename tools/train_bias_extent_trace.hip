// train_bias_extent_trace.hip -- CPU only, beside tools/train_lang_extent_trace.hip: the fine-tune step's launches and workspace plan
// for return_attention_map geometries (Geom::mask_as_bias), whose generated leaves lie in another order in a row of
// theta and whose policy blocks run softmax_bias_fwd_kernel.  tests/test_mask_as_bias_host.py holds every operand to the plan's
// buffers with the rules of tests/test_train_workspace_extents.py.  Build and run:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -DHVLA_TRAIN_TRACE -I hyper-vla_amd/csrc tools/train_bias_extent_trace.hip hyper-vla_amd/csrc/train.hip -o train_bias_extent_trace
//
// The cases are those of tests/test_gpu_mask_as_bias.py: MID at B = 4 (plain and with both attention terms) and B = 2, the README
// widths at B = 2, each with the encoder frozen and trained, at its batch and at B = 1.
#include <vector>

#include "train_trace_driver.h"

struct Case { const char* name; Geom g; int B; int aux; };

int main() {
  std::vector<Case> cases;
  auto add = [&](const char* name, Geom base, int B, int aux) { base.mask_as_bias = 1; cases.push_back({name, base, B, aux}); };
  add("MID-bias", mid(), 4, 0);
  add("MID-bias-aux", mid(), 4, 2);
  add("MID-bias-B2", mid(), 2, 0);
  add("README2-bias", readme2(), 2, 0);
  for (const Case& c : cases)
    for (int enc = 0; enc < 2; ++enc)
      for (int B : {c.B, 1})
        if (run(Point{c.name, c.g, B, enc, 0, 0, 0, c.aux, 0.f, 0.f}, true)) return 1;
  return 0;
}
