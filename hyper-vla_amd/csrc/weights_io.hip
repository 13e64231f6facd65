// weights_io.hip — weight arenas as values: a reference-order theta into arena rows (the inverse of
// export_theta_kernel, hypernet.hip) and arena rows from one arena to another.  Both are index maps bound by memory traffic; the
// arena side of every access is 16 bytes per lane, lanes consecutive.
#include "common.h"
#include "kernels.h"

namespace hvla {

typedef __attribute__((ext_vector_type(4))) int32_t i32x4;

// theta[k][ref] or zero for padding / the language prefix region (perm -1), which the weight generation zeroes too
__device__ __forceinline__ float theta_at(const float* __restrict__ th, int ref) { return ref >= 0 ? th[ref] : 0.f; }

// grid (column chunks, K), as the export's.  Row k of theta [K, G] -> arena row slot[k] (slot null: row k); an entry outside [0, rows)
// touches nothing (pool_assign_kernel's rule).  An item is 16 bytes of one plane:
//   matrix region  8 consecutive positions -- one lane's share of a 1 KiB fragment: their 8 perm entries as two 16-byte loads, 8
//                  gathered theta values, split1 (common.h: the halves the weight generation gives the same f32 value), one bf16x8
//                  store to wh and one to wl
//   vector region  4 consecutive positions: one 16-byte perm load, 4 gathered values, one f32x4 store
// Gm is a multiple of 512 and Gv of 32 (layout.h), so every vector access is aligned and no item straddles the two regions.
// The workgroups of chunk 0 also write the row's context (`context` [K, C], or zeros) and zero its ensemble counter.
__global__ __launch_bounds__(256) void import_theta_kernel(const float* __restrict__ theta, const float* __restrict__ context,
                                                           const int32_t* __restrict__ perm, const int32_t* __restrict__ slot,
                                                           __bf16* __restrict__ wh, __bf16* __restrict__ wl, float* __restrict__ vf,
                                                           float* __restrict__ ctx, int* __restrict__ count, int Gm, int Gv, int G,
                                                           int C, int rows) {
  const int k = blockIdx.y;
  const int row = slot ? slot[k] : k;
  if (row < 0 || row >= rows) return;
  const float* th = theta + (size_t)k * G;
  const int nm = Gm / 8, nv = Gv / 4;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nm + nv; i += gridDim.x * blockDim.x) {
    if (i < nm) {
      const i32x4 r0 = *reinterpret_cast<const i32x4*>(perm + (size_t)i * 8);
      const i32x4 r1 = *reinterpret_cast<const i32x4*>(perm + (size_t)i * 8 + 4);
      const float v[8] = {theta_at(th, r0[0]), theta_at(th, r0[1]), theta_at(th, r0[2]), theta_at(th, r0[3]),
                          theta_at(th, r1[0]), theta_at(th, r1[1]), theta_at(th, r1[2]), theta_at(th, r1[3])};
      const Split8 s = split8(v);
      *reinterpret_cast<bf16x8*>(wh + (size_t)row * Gm + (size_t)i * 8) = s.hi;
      *reinterpret_cast<bf16x8*>(wl + (size_t)row * Gm + (size_t)i * 8) = s.lo;
    } else {
      const int j = i - nm;
      const i32x4 r = *reinterpret_cast<const i32x4*>(perm + (size_t)Gm + (size_t)j * 4);
      const f32x4 v = {theta_at(th, r[0]), theta_at(th, r[1]), theta_at(th, r[2]), theta_at(th, r[3])};
      *reinterpret_cast<f32x4*>(vf + (size_t)row * Gv + (size_t)j * 4) = v;
    }
  }
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) ctx[(size_t)row * C + c] = context ? context[(size_t)k * C + c] : 0.f;
    if (threadIdx.x == 0) count[row] = 0;
  }
}

// grid (chunks, K).  Row src_slot[k] of one arena (`srows` rows) -> row dst_slot[k] of another (`drows` rows), byte for byte in 16-byte
// units: wh, wl (the language prefix included: it lies inside the matrix planes), vf and ctx; the destination's ensemble counter to
// zero.  A pair with either entry out of range touches nothing.  The same arena on both sides needs disjoint maps (the host checks).
__global__ __launch_bounds__(256) void copy_rows_kernel(const u32x4* __restrict__ swh, const u32x4* __restrict__ swl,
                                                        const u32x4* __restrict__ svf, const u32x4* __restrict__ sctx,
                                                        u32x4* __restrict__ dwh, u32x4* __restrict__ dwl, u32x4* __restrict__ dvf,
                                                        u32x4* __restrict__ dctx, int* __restrict__ count,
                                                        const int32_t* __restrict__ src_slot, const int32_t* __restrict__ dst_slot,
                                                        int Gm, int Gv, int C, int srows, int drows) {
  const int k = blockIdx.y;
  const int s = src_slot[k], d = dst_slot[k];
  if (s < 0 || s >= srows || d < 0 || d >= drows) return;
  const int nm = Gm / 8, nv = Gv / 4, nc = C / 4;         // 16-byte units per row of a matrix plane, of vf and of ctx
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * nm + nv + nc; i += gridDim.x * blockDim.x) {
    if (i < nm)
      dwh[(size_t)d * nm + i] = swh[(size_t)s * nm + i];
    else if (i < 2 * nm)
      dwl[(size_t)d * nm + (i - nm)] = swl[(size_t)s * nm + (i - nm)];
    else if (i < 2 * nm + nv)
      dvf[(size_t)d * nv + (i - 2 * nm)] = svf[(size_t)s * nv + (i - 2 * nm)];
    else
      dctx[(size_t)d * nc + (i - 2 * nm - nv)] = sctx[(size_t)s * nc + (i - 2 * nm - nv)];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) count[d] = 0;
}

// ---- launchers -----------------------------------------------------------------------------------
static int chunks_of(int items) {
  const int n = (items + 255) / 256;
  return n < 1 ? 1 : n > 128 ? 128 : n;                    // the export's 128 column chunks at most; the kernels stride over the rest
}

hipError_t launch_import_theta(const float* theta, const float* context, const int32_t* perm, const int32_t* slot, __bf16* wh,
                               __bf16* wl, float* vf, float* ctx, int* count, int Gm, int Gv, int G, int C, int K, int rows,
                               hipStream_t st) {
  if (Gm % 8 || Gv % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(import_theta_kernel, dim3(chunks_of(Gm / 8 + Gv / 4), K), dim3(256), 0, st, theta, context, perm, slot, wh, wl,
                     vf, ctx, count, Gm, Gv, G, C, rows);
  return hipGetLastError();
}

hipError_t launch_copy_rows(const void* swh, const void* swl, const void* svf, const void* sctx, void* dwh, void* dwl, void* dvf,
                            void* dctx, int* count, const int32_t* src_slot, const int32_t* dst_slot, int Gm, int Gv, int C, int K,
                            int srows, int drows, hipStream_t st) {
  if (Gm % 8 || Gv % 4 || C % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(copy_rows_kernel, dim3(chunks_of(Gm / 4 + Gv / 4 + C / 4), K), dim3(256), 0, st,
                     static_cast<const u32x4*>(swh), static_cast<const u32x4*>(swl), static_cast<const u32x4*>(svf),
                     static_cast<const u32x4*>(sctx), static_cast<u32x4*>(dwh), static_cast<u32x4*>(dwl), static_cast<u32x4*>(dvf),
                     static_cast<u32x4*>(dctx), count, src_slot, dst_slot, Gm, Gv, C, srows, drows);
  return hipGetLastError();
}

}  // namespace hvla
