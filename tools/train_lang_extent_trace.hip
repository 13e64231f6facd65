// train_lang_extent_trace.hip -- CPU only, beside tools/train_extent_trace.hip: the fine-tune step's launches and workspace plan for
// use_language_token geometries (hvla_train_language_tokens), where the policy runs on T + P + 1 rows per episode.
// tests/test_lang_train_host.py holds every operand to the plan's buffers with the rules of tests/test_train_workspace_extents.py: a
// policy buffer still sized by P + 1 rows is an operand that leaves its buffer, which a parity run can pass by luck.  Build and run:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -DHVLA_TRAIN_TRACE -I hyper-vla_amd/csrc tools/train_lang_extent_trace.hip hyper-vla_amd/csrc/train.hip -o train_lang_extent_trace
//
// The cases are those of tests/lang_policy_torch.py::GEOMETRIES (same names), each with the encoder frozen and trained, at its GPU
// batch size and at B = 1, and the README widths with the option at the batch of the recorded speed figure.
#include <vector>

#include "train_trace_driver.h"

struct Case { const char* name; Geom g; int B; };

int main() {
  std::vector<Case> cases;
  auto add = [&](const char* name, Geom base, int B, auto change) { base.lang_in_policy = 1; change(base); cases.push_back({name, base, B}); };
  add("T12", mid(), 4, [](Geom&) {});
  add("T2", mid(), 4, [](Geom& g) { g.T = 2; });
  add("T3", mid(), 4, [](Geom& g) { g.T = 3; });
  add("T32", mid(), 4, [](Geom& g) { g.T = 32; });
  add("T32-P256", mid(), 2, [](Geom& g) { g.T = 32; g.image_size = 224; });
  add("README2-lang", readme2(), 32, [](Geom&) {});
  for (const Case& c : cases)
    for (int enc = 0; enc < 2; ++enc)
      for (int B : {c.B, 1})
        if (run(Point{c.name, c.g, B, enc, 0, 0, 0, 0, 0.f, 0.f}, true)) return 1;
  return 0;
}
