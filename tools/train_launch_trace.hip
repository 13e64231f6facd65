// train_launch_trace.hip -- CPU only: prints what the fine-tune step enqueues, launch for launch and argument for argument, over a
// sweep of geometries, batch sizes and options.  csrc/train.hip built with -DHVLA_TRAIN_TRACE prints instead of launching
// (tools/train_launch_trace.h), so this runs without a GPU, on fake pointers that host code never dereferences.  Build and run:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -DHVLA_TRAIN_TRACE -I hyper-vla_amd/csrc tools/train_launch_trace.hip hyper-vla_amd/csrc/train.hip -o train_launch_trace
//
// tests/native/train_step_trace.txt is its output, recorded from the sequencing before the block-leaf table;
// tests/test_train_launch_trace.py builds it from the tree and compares byte for byte.  A change that moves a launch on purpose
// regenerates the file and says so.  The points and the driver of one point: tools/train_trace_driver.h.
#include "train_trace_driver.h"

int main() {
  for (const Point& p : recorded_sweep())
    if (run(p)) return 1;
  return 0;
}
