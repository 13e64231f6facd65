// position.hip — DINOv2's position table through its interpolation (include/hvla.h hvla_position_interp / _adjoint).
//
// The reference keeps HF's n x n table as the trainable leaf and resizes it to the run-time grid inside every forward pass
// (FlaxDinov2Embeddings.interpolate_pos_encoding: jax.image.scale_and_translate, bicubic, no antialiasing).  The resize is the
// separable linear map  dst[1 + i grid + j] = sum_w ( sum_h src[1 + h n + w] W[h][i] ) W[w][j]  with ONE weight matrix W [n, grid]
// for both axes; the caller computes W with the converter's own numpy function (hypervla/convert.py) and uploads it, so nothing of
// the formula is restated here.  Row 0 (the class row) is copied.
//
//   interp   one thread per (destination row, 4 columns): the height axis is contracted first, then the width axis, each in f32
//            with the taps in ascending order, products rounded before they are added (no fused multiply-add, no contraction of
//            the two stages into one sum) -- the order of convert.bake_position_embeddings
//   adjoint  dsrc = A^T ddst as a GATHER: one thread per (source row, 4 columns) sums the outputs that row feeds, in ascending
//            (i, j); no atomics, bit-reproducible
//
// Both are bound by latency (0.8 MB and 4.2 MB of traffic at n = 37, grid = 16, E = 768): 16-byte accesses along E, no LDS, no
// matrix cores.  A thread finds the taps of its row by scanning its row / column of W for the first and the last non-zero weight
// (the non-zero taps of a resize are contiguous; a zero weight inside the range contributes +-0 to the sum).
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace hvla {

// first and last index k in [0, len) with w[k * stride] != 0 (lo > hi: none)
__device__ __forceinline__ void tap_range(const float* __restrict__ w, int len, int stride, int& lo, int& hi) {
  lo = len;
  hi = -1;
  for (int k = 0; k < len; ++k)
    if (w[(long)k * stride] != 0.f) {
      if (lo == len) lo = k;
      hi = k;
    }
}

__global__ void __launch_bounds__(256) position_interp_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                              float* __restrict__ dst, int n, int grid, int e4) {
#pragma clang fp contract(off)
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (1 + grid * grid) * e4) return;
  const int row = idx / e4, c = idx - row * e4;
  const f32x4* __restrict__ s = reinterpret_cast<const f32x4*>(src);
  f32x4* __restrict__ d = reinterpret_cast<f32x4*>(dst);
  if (row == 0 || n == grid) {                       // the class row; n == grid: the table is returned untouched
    d[idx] = s[idx];
    return;
  }
  const int i = (row - 1) / grid, j = (row - 1) - i * grid;
  int h0, h1, w0, w1;
  tap_range(w + i, n, grid, h0, h1);                 // column i of W: the source rows of output row i
  tap_range(w + j, n, grid, w0, w1);                 // column j of W: the source columns of output column j
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int x = w0; x <= w1; ++x) {
    f32x4 t = {0.f, 0.f, 0.f, 0.f};                  // the height contraction of source column x
    for (int y = h0; y <= h1; ++y) {
      const float wy = w[(long)y * grid + i];
      const f32x4 v = s[(long)(1 + y * n + x) * e4 + c];
      t[0] = t[0] + v[0] * wy; t[1] = t[1] + v[1] * wy; t[2] = t[2] + v[2] * wy; t[3] = t[3] + v[3] * wy;
    }
    const float wx = w[(long)x * grid + j];
    acc[0] = acc[0] + t[0] * wx; acc[1] = acc[1] + t[1] * wx; acc[2] = acc[2] + t[2] * wx; acc[3] = acc[3] + t[3] * wx;
  }
  d[idx] = acc;
}

__global__ void __launch_bounds__(256) position_adjoint_kernel(const float* __restrict__ ddst, const float* __restrict__ w,
                                                               float* __restrict__ dsrc, int n, int grid, int e4) {
#pragma clang fp contract(off)
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (1 + n * n) * e4) return;
  const int row = idx / e4, c = idx - row * e4;
  const f32x4* __restrict__ g = reinterpret_cast<const f32x4*>(ddst);
  f32x4* __restrict__ o = reinterpret_cast<f32x4*>(dsrc);
  if (row == 0 || n == grid) {
    o[idx] = g[idx];
    return;
  }
  const int y = (row - 1) / n, x = (row - 1) - y * n;
  int i0, i1, j0, j1;
  tap_range(w + (long)y * grid, grid, 1, i0, i1);    // row y of W: the output rows source row y feeds
  tap_range(w + (long)x * grid, grid, 1, j0, j1);    // row x of W: the output columns source column x feeds
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int i = i0; i <= i1; ++i) {
    const float wy = w[(long)y * grid + i];
    for (int j = j0; j <= j1; ++j) {
      const float ww = wy * w[(long)x * grid + j];
      const f32x4 v = g[(long)(1 + i * grid + j) * e4 + c];
      acc[0] = acc[0] + v[0] * ww; acc[1] = acc[1] + v[1] * ww; acc[2] = acc[2] + v[2] * ww; acc[3] = acc[3] + v[3] * ww;
    }
  }
  o[idx] = acc;
}

// the serving buffer holds the table with the class token added into row 0 (serving_layout.h, Pack POS): the loader's expression,
// element for element, in place behind the resize
__global__ void __launch_bounds__(256) position_serve_kernel(float* table, const float* __restrict__ cls, int E, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) table[i] = table[i] + (i < E ? cls[i] : 0.f);
}

hipError_t launch_position_interp(const float* src, int n, const float* w, float* dst, int grid, int E, hipStream_t st) {
  const int e4 = E / 4, total = (1 + grid * grid) * e4;
  hipLaunchKernelGGL(position_interp_kernel, dim3((total + 255) / 256), dim3(256), 0, st, src, w, dst, n, grid, e4);
  return hipGetLastError();
}

hipError_t launch_position_serve(const float* src, int n, const float* w, const float* cls, float* table, int grid, int E, hipStream_t st) {
  hipError_t e = launch_position_interp(src, n, w, table, grid, E, st);
  if (e != hipSuccess) return e;
  const int total = (1 + grid * grid) * E;
  hipLaunchKernelGGL(position_serve_kernel, dim3((total + 255) / 256), dim3(256), 0, st, table, cls, E, total);
  return hipGetLastError();
}

hipError_t launch_position_adjoint(const float* ddst, int n, const float* w, float* dsrc, int grid, int E, hipStream_t st) {
  const int e4 = E / 4, total = (1 + n * n) * e4;
  hipLaunchKernelGGL(position_adjoint_kernel, dim3((total + 255) / 256), dim3(256), 0, st, ddst, w, dsrc, n, grid, e4);
  return hipGetLastError();
}

}  // namespace hvla
