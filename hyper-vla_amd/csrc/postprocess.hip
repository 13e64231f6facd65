// postprocess.hip — InferenceWrapper.postprocess per pool slot on the device (include/hvla.h hvla_post_*):
// un-normalisation, temporal ensemble, euler -> axis-angle and the gripper rules of each slot's policy setup
// (data/utils/hypervla_interface.py:219-299, data/utils/action_ensemble.py:15-27 with temperature 0).
//
// Arithmetic contract: f64 in the host's operation order, so raw_action and the translation are bitwise what numpy computes.
// That holds only WITHOUT floating-point contraction: HIP's default fuses `a * std + mean` and every `acc + w * x` of the ensemble
// into v_fma_f64, which numpy never does.  Every function of this file therefore starts with `#pragma clang fp contract(off)`
// (tests/test_postprocess_host.py checks the kernel's ISA for v_fma_f64 / v_fmac_f64).  The rotation calls cos / sin / atan2 /
// sqrt and divides, whose library forms use fma internally: it lives in post_axangle, kept out of line so that the kernel's own
// body stays fma-free; its result is rounded to f32, where it agrees with the host to within 1 ulp.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "../../include/hvla.h"
#include "kernels.h"

namespace hvla {

namespace {

// 1.0 / n for the ensemble weights (ActionEnsembler: ones(n) / n): folded by the compiler, correctly rounded as numpy's
// division, so the kernel itself divides nothing.
__constant__ double kPostInv[POST_MAX_HORIZON + 1] = {0.0,       1.0 / 1,  1.0 / 2,  1.0 / 3,  1.0 / 4,  1.0 / 5,
                                                      1.0 / 6,   1.0 / 7,  1.0 / 8,  1.0 / 9,  1.0 / 10, 1.0 / 11,
                                                      1.0 / 12,  1.0 / 13, 1.0 / 14, 1.0 / 15, 1.0 / 16};

struct Rot3 {
  float x, y, z;
};

// hypervla.interface.euler2axangle (transforms3d's quaternion route) followed by `ax * angle`, rounded to f32.
__device__ __attribute__((noinline)) Rot3 post_axangle(double ai, double aj, double ak) {
#pragma clang fp contract(off)
  const double ci = cos(ai / 2.0), si = sin(ai / 2.0);
  const double cj = cos(aj / 2.0), sj = sin(aj / 2.0);
  const double ck = cos(ak / 2.0), sk = sin(ak / 2.0);
  double w = cj * ci * ck + sj * si * sk;
  double x = cj * si * ck - sj * ci * sk;
  double y = cj * si * sk + sj * ci * ck;
  double z = cj * ci * sk - sj * si * ck;
  const double n = sqrt(w * w + x * x + y * y + z * z);
  if (n < 1e-8) return {0.f, 0.f, 0.f};                     // axis (1, 0, 0), angle 0
  w = w / n; x = x / n; y = y / n; z = z / n;
  const double v = sqrt(x * x + y * y + z * z);
  if (v < DBL_EPSILON * 3.0) return {0.f, 0.f, 0.f};
  const double angle = 2.0 * atan2(v, w);
  return {(float)(x / v * angle), (float)(y / v * angle), (float)(z / v * angle)};
}

// InferenceWrapper.unnormalize for column c (the mask picks the un-normalised value or the raw one)
__device__ __forceinline__ double post_unnormalize(float a32, const hvla_post_row& t, int c) {
#pragma clang fp contract(off)
  const double a = (double)a32;
  if (!t.mask[c]) return a;
  if (t.normalization == HVLA_NORM_BOUNDS) return (a + 1.0) * t.p1[c] / 2.0 + t.p0[c];   // p1 = p99 - p01 + 1e-8
  return a * t.p1[c] + t.p0[c];                                                          // p0 = mean, p1 = std
}

// One thread per call row k, arena slot b = slots[k] (distinct, so the slot's state is updated in place).  Entries outside
// [0, B), and slots whose table row is outside [0, n_rows), are skipped: no load of their state past the check, no store.
__global__ void post_slots_kernel(const float* __restrict__ actions, const int32_t* __restrict__ slots, int K, int B, int H,
                                  double* __restrict__ ring, PostSlot* __restrict__ state, const hvla_post_row* __restrict__ table,
                                  int n_rows, double* __restrict__ raw_out, double* __restrict__ env_out) {
#pragma clang fp contract(off)
  constexpr int D = HVLA_POST_DIM;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int b = slots[k];
  if (b < 0 || b >= B) return;
  PostSlot s = state[b];
  if (s.row < 0 || s.row >= n_rows) return;
  const hvla_post_row& t = table[s.row];
  const bool known = (t.normalization == HVLA_NORM_NORMAL || t.normalization == HVLA_NORM_BOUNDS) &&
                     (t.setup == HVLA_SETUP_LIBERO || t.setup == HVLA_SETUP_WIDOWX_BRIDGE || t.setup == HVLA_SETUP_GOOGLE_ROBOT);
  if (!known) {                                             // a table the library does not know: NaN, state untouched
#pragma unroll
    for (int c = 0; c < D; ++c) {
      if (raw_out) raw_out[(size_t)k * D + c] = __builtin_nan("");
      env_out[(size_t)k * D + c] = __builtin_nan("");
    }
    return;
  }
  const float* a = actions + (size_t)k * H * D;
  double raw[D];
  if (s.ensemble) {
    // ring [H calls][H rows][D] of slot b: the un-normalised prediction of call c sits at c % H
    double* rg = ring + (size_t)b * H * H * D;
    double* cur = rg + (size_t)(s.calls % H) * H * D;
    for (int h = 0; h < H; ++h)
#pragma unroll
      for (int c = 0; c < D; ++c) cur[h * D + c] = post_unnormalize(a[h * D + c], t, c);
    const int n = s.calls + 1 < H ? s.calls + 1 : H;
    const double wt = kPostInv[n];
    const int first = s.calls - (n - 1);                    // the oldest stored call: ensemble term idx = 0
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double acc = 0.0;                                     // Python's sum(): 0 + w * pred_0[n - 1] + ... + w * pred_{n-1}[0]
      for (int idx = 0; idx < n; ++idx)
        acc = acc + wt * rg[(size_t)((first + idx) % H) * H * D + (n - 1 - idx) * D + c];
      raw[c] = acc;
    }
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) raw[c] = post_unnormalize(a[c], t, c);
  }
  const Rot3 rot = post_axangle(raw[3], raw[4], raw[5]);
  const double g = raw[D - 1];
  double grip;
  if (t.setup == HVLA_SETUP_GOOGLE_ROBOT) {                 // the sticky gripper (hypervla_interface.py:269-292)
    double rel = s.has_prev ? s.prev_grip - g : 0.0;
    s.prev_grip = g;
    s.has_prev = 1;
    if (fabs(rel) > 0.5 && !s.sticky_on) {
      s.sticky_on = 1;
      s.sticky_value = rel;
    }
    if (s.sticky_on) {
      s.repeat += 1;
      rel = s.sticky_value;
    }
    if (s.repeat == POST_STICKY_REPEATS) {
      s.sticky_on = 0;
      s.repeat = 0;
      s.sticky_value = 0.0;
    }
    grip = rel;
  } else if (t.setup == HVLA_SETUP_WIDOWX_BRIDGE) {
    grip = 2.0 * (g > 0.5 ? 1.0 : 0.0) - 1.0;
  } else {
    grip = 2.0 * g - 1.0;
  }
  s.calls += 1;
  state[b] = s;
#pragma unroll
  for (int c = 0; c < D; ++c)
    if (raw_out) raw_out[(size_t)k * D + c] = raw[c];
  double* e = env_out + (size_t)k * D;
  e[0] = raw[0]; e[1] = raw[1]; e[2] = raw[2];
  e[3] = (double)rot.x; e[4] = (double)rot.y; e[5] = (double)rot.z;
  e[6] = (double)(float)grip;
}

// InferenceWrapper.reset of the caller-side state: fresh ensemble, no previous gripper action, sticky off.
__global__ void post_assign_kernel(PostSlot* __restrict__ state, const int32_t* __restrict__ slots, int K, int B,
                                   const int32_t* __restrict__ rows, const uint8_t* __restrict__ ensemble) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int b = slots[k];
  if (b < 0 || b >= B) return;
  PostSlot s{};
  s.row = rows[k];
  s.ensemble = ensemble[k] != 0;
  state[b] = s;
}

}  // namespace

hipError_t launch_post_assign(PostSlot* state, const int32_t* slots, int K, int B, const int32_t* rows, const uint8_t* ensemble,
                              hipStream_t st) {
  hipLaunchKernelGGL(post_assign_kernel, dim3((K + 63) / 64), dim3(64), 0, st, state, slots, K, B, rows, ensemble);
  return hipGetLastError();
}

hipError_t launch_post_step(const float* actions, const int32_t* slots, int K, int B, int H, double* ring, PostSlot* state,
                            const hvla_post_row* table, int n_rows, double* raw_out, double* env_out, hipStream_t st) {
  if (H < 1 || H > POST_MAX_HORIZON) return hipErrorInvalidValue;
  hipLaunchKernelGGL(post_slots_kernel, dim3((K + 63) / 64), dim3(64), 0, st, actions, slots, K, B, H, ring, state, table, n_rows,
                     raw_out, env_out);
  return hipGetLastError();
}

}  // namespace hvla
