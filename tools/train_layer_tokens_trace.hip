// train_layer_tokens_trace.hip -- CPU only, beside tools/train_diff_extent_trace.hip: the fine-tune step's launches and workspace plan
// for share_layer_index=False geometries (Geom::layer_tokens), whose context encoder runs on T + 1 + NL rows and whose
// weight generation is three grouped launches (bgemm_groups) over the layout's run table.  tests/test_layer_tokens_train_host.py
// holds the layer-token lines of its output to tests/native/train_layer_tokens_trace.txt byte for byte and every operand to the plan's buffers with the rules
// of tests/test_train_workspace_extents.py.  Build and run:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -DHVLA_TRAIN_TRACE -I hyper-vla_amd/csrc tools/train_layer_tokens_trace.hip hyper-vla_amd/csrc/train.hip -o train_layer_tokens_trace
//
// The points: MID at B = 1 and 5 with own and with shared heads; the sequence edge T + 1 + NL = 48 (four policy layers, 38 language
// tokens) at B = 3, encoder frozen and trained; use_language_token and differential at B = 2; the README widths at B = 2; MID at
// B = 128 (the 128-column tile tables).  The last two points are flag-OFF: MID at B = 4, frozen and trained, under the title and with
// the arguments tools/train_extent_trace.hip gives them.
#include <vector>

#include "train_trace_driver.h"

struct Case { const char* name; Geom g; int B; int enc; };

int main() {
  std::vector<Case> cases;
  auto add = [&](const char* name, Geom base, int B, int enc, bool shared, auto change) {
    base.layer_tokens = 1; base.shared_block_heads = shared ? 1 : 0;
    change(base);
    cases.push_back({name, base, B, enc});
  };
  for (int B : {1, 5}) {
    add("MID-lt", mid(), B, 0, false, [](Geom&) {});
    add("MID-lt-shared", mid(), B, 0, true, [](Geom&) {});
  }
  for (int enc = 0; enc < 2; ++enc) add("S48-lt", mid(), 3, enc, false, [](Geom& g) { g.L = 4; g.T = 38; });
  add("LANG-lt", mid(), 2, 0, true, [](Geom& g) { g.lang_in_policy = 1; });
  add("DIFF-lt-shared", mid(), 2, 0, true, [](Geom& g) { g.differential = 1; });
  add("README2-lt", readme2(), 2, 0, false, [](Geom&) {});
  add("MID-lt-shared", mid(), 128, 0, true, [](Geom&) {});
  for (const Case& c : cases)
    if (run(Point{c.name, c.g, c.B, c.enc, 0, 0, 0, 0, 0.f, 0.f}, true)) return 1;
  for (int enc = 0; enc < 2; ++enc)
    if (run(Point{"MID", mid(), 4, enc, 0, 0, 0, 0, 0.f, 0.f}, true)) return 1;
  return 0;
}
