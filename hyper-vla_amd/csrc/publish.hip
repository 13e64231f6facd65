// publish.hip — hvla_train_publish: the flat training vector (parameters or EMA) into the serving buffers, on the device.
//
// Everything here is an index permutation with a rounding, bound by memory traffic; no matrix core is involved.  The index maps
// come from the enumeration of serving_layout.h that hvla_load_weights packs by, the roundings are the functions of pack.h that it
// calls: the bytes are the loader's (tests/native/publish_map_check.cpp runs both on the CPU against a frozen copy of the earlier
// loader; tests/test_gpu_publish.py compares the device buffers' effect bit for bit against a freshly loaded model).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "serving_layout.h"

namespace hvla {

using namespace serving;
using namespace pack;

// ---- f32 copies driven by a table (context encoder -> hn_f32, encoder vectors -> encf32) ----
// grid (x, segment, layer); a segment that exists once is written by layer 0's blocks only
__global__ void __launch_bounds__(256) publish_copy_kernel(const float* __restrict__ params, float* __restrict__ dst, CopyTable t) {
  const CopySeg s = t.seg[blockIdx.y];
  const int l = blockIdx.z;
  if (!s.per_layer && l > 0) return;
  const float* __restrict__ src = params + s.src + (int64_t)l * t.src_stride;
  float* __restrict__ out = dst + s.dst + (int64_t)l * t.dst_stride;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < s.n; i += gridDim.x * blockDim.x) out[i] = src[i];
}

// ---- position table: the CLS token is added into row 0 ----
__global__ void __launch_bounds__(256) publish_pos_kernel(const float* __restrict__ pos, const float* __restrict__ cls,
                                                          float* __restrict__ out, int E, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = pos[i] + (i < E ? cls[i] : 0.f);
}

// ---- patch embedding: one thread per output channel (the bias is a serial double sum in ascending k) ----
__global__ void __launch_bounds__(64) publish_patch_kernel(const float* __restrict__ pk, const float* __restrict__ pb,
                                                           uint16_t* __restrict__ w16, float* __restrict__ bias, int E, int Kreal,
                                                           int Kp, int bf) {
  const int nn = blockIdx.x * blockDim.x + threadIdx.x;
  if (nn >= E) return;
  bias[nn] = patch_channel(pk, pb[nn], E, nn, Kreal, Kp, bf != 0, w16 + (size_t)nn * Kp);
}

// ---- transposing pack: [K][N] f32 -> [N][K] 16-bit weight and residue planes ----
// One workgroup per 64 x 64 tile, through LDS.  The tile is stored [k][n] with a pitch of 65 floats.
//   in : a wave reads 64 consecutive n of one row k (256 B) and stores them to 64 consecutive words: no two lanes of a 32-lane
//        group share a bank, under the 32-bank rule of ds_write_b32 or against all 64 banks.
//   out: a 32-lane group is 16 k-pairs p x 2 rows n; a lane reads words (2p + j) 65 + n, bank (2p + j + n) mod 32 -- sixteen even
//        offsets plus the parity of n: 32 different banks.  Each lane packs k = 2p, 2p + 1 into one 32-bit store, so 16 lanes
//        write 64 contiguous bytes of a row of the output and the lane's second pair (p + 16) completes the 128-byte line.
// blockIdx.x runs over the tiles of one layer's six matrices (EncMat::tile0), blockIdx.y over the layers.
constexpr int TR_PITCH = TR_TILE + 1;
__global__ void __launch_bounds__(256) publish_transpose_kernel(const float* __restrict__ params, uint16_t* __restrict__ w16,
                                                                uint16_t* __restrict__ d16, EncMap m, int bf) {
  __shared__ float tile[TR_TILE * TR_PITCH];
  int mi = 0;
#pragma unroll
  for (int i = 1; i < ENC_MATS; ++i)
    if ((int)blockIdx.x >= m.mat[i].tile0) mi = i;
  // (selected field by field: indexing the by-value table with a run-time index would put it in the private segment)
  int64_t src0 = m.mat[0].src, dst0 = m.mat[0].dst;
  int K = m.mat[0].K, N = m.mat[0].N, t0 = 0;
#pragma unroll
  for (int i = 1; i < ENC_MATS; ++i)
    if (mi == i) { src0 = m.mat[i].src; dst0 = m.mat[i].dst; K = m.mat[i].K; N = m.mat[i].N; t0 = m.mat[i].tile0; }
  const int layer = blockIdx.y, t = blockIdx.x - t0, ntn = N / TR_TILE;
  const int k0 = (t / ntn) * TR_TILE, n0 = (t % ntn) * TR_TILE;
  const float* __restrict__ src = params + src0 + (int64_t)layer * m.mat_src_stride;
  const int64_t dst = dst0 + (int64_t)layer * m.mat_dst_stride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 4
  for (int r = wave; r < TR_TILE; r += 4) tile[r * TR_PITCH + lane] = src[(size_t)(k0 + r) * N + n0 + lane];
  __syncthreads();
  const int p = threadIdx.x & 15, nl = threadIdx.x >> 4;      // 16 rows n per pass
#pragma unroll
  for (int pass = 0; pass < TR_TILE / 16; ++pass) {
    const int n = pass * 16 + nl;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = 2 * (p + 16 * h);
      uint16_t wa, da, wb, db;
      round_pair(tile[k * TR_PITCH + n], bf != 0, wa, da);
      round_pair(tile[(k + 1) * TR_PITCH + n], bf != 0, wb, db);
      const size_t o = (size_t)dst + (size_t)(n0 + n) * K + k0 + k;     // even: K, k0 and k are
      *reinterpret_cast<uint32_t*>(w16 + o) = (uint32_t)wa | ((uint32_t)wb << 16);
      *reinterpret_cast<uint32_t*>(d16 + o) = (uint32_t)da | ((uint32_t)db << 16);
    }
  }
}

// ---- W_cat fragments and b_cat ----
// One workgroup takes WC_RUN = 16 consecutive 32-column tiles: 512 packed positions, one whole fragment of the matrix region, whose
// source columns are 32 consecutive features of 16 rows of a generated leaf -- whole 128-byte lines of each of the C rows of W_cat.
// Thread t holds packed columns t and t + 256.  Per k-step (16 rows of W_cat) it gathers its 2 x 16 values, splits them into the hi / lo
// bf16 planes and stores them where the fragment wants them: column tau of a tile is lane rho_of_tau(tau), rows 0-7 of the k-step its
// eight elements in lane rho, rows 8-15 in lane rho + 32 -- two 16-byte LDS stores per plane.  The staged k-step is then 16 tiles x
// 1 KiB per plane, each a contiguous run of the output (element ((pt KS + ks) 64 + lane) 8 + j), written 16 bytes per thread.
// perm < 0 (padding): zeros, as the host packer leaves them.
constexpr int WC_RUN = 16;
// The k-step loop of both W_cat kernels: this thread's two columns gather column ref[c] of wcat [16 KS][ld] (ref < 0: zeros) into LDS
// slot[c]; the staged k-step goes out as fragment blocks blk0 .. blk0 + WC_RUN - 1, those below nblk.
__device__ __forceinline__ void wcat_ksteps(const float* __restrict__ wcat, int ld, const int (&ref)[2], const int (&slot)[2], int blk0,
                                            int nblk, int KS, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
  __shared__ uint4 stage[2][WC_RUN * 64];          // [plane][block][lane]: 8 bf16 each
  const int tid = threadIdx.x;
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float w[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) w[r] = ref[c] >= 0 ? wcat[(size_t)(16 * ks + r) * ld + ref[c]] : 0.f;
#pragma unroll
      for (int hk = 0; hk < 2; ++hk) {
        uint32_t h[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint16_t h0, l0, h1, l1;
          split_pair(w[8 * hk + 2 * j], h0, l0);
          split_pair(w[8 * hk + 2 * j + 1], h1, l1);
          h[j] = (uint32_t)h0 | ((uint32_t)h1 << 16);
          l[j] = (uint32_t)l0 | ((uint32_t)l1 << 16);
        }
        stage[0][slot[c] + 32 * hk] = make_uint4(h[0], h[1], h[2], h[3]);
        stage[1][slot[c] + 32 * hk] = make_uint4(l[0], l[1], l[2], l[3]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = tid; i < WC_RUN * 64; i += 256) {
      const int blk = blk0 + (i >> 6);
      if (blk < nblk) {
        const size_t o = ((size_t)blk * KS + ks) * 64 + (i & 63);      // in 16-byte units
        reinterpret_cast<uint4*>(hi)[o] = stage[0][i];
        reinterpret_cast<uint4*>(lo)[o] = stage[1][i];
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) publish_wcat_kernel(const float* __restrict__ wcat, const float* __restrict__ bsrc,
                                                           const int32_t* __restrict__ perm, uint16_t* __restrict__ hi,
                                                           uint16_t* __restrict__ lo, float* __restrict__ bc, int G, int ntiles, int KS) {
  const int pt0 = blockIdx.x * WC_RUN;
  const int tid = threadIdx.x;
  int ref[2], slot[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col = tid + 256 * c, tl = col >> 5, tau = col & 31;
    const bool live = pt0 + tl < ntiles;
    ref[c] = live ? perm[(size_t)pt0 * 32 + col] : -1;
    slot[c] = tl * 64 + rho_of_tau(tau);
    if (live) bc[(size_t)pt0 * 32 + col] = ref[c] >= 0 ? bsrc[ref[c]] : 0.f;
  }
  wcat_ksteps(wcat, G, ref, slot, pt0, ntiles, KS, hi, lo);
}

// ---- the same for a layer-token model: one fragment block per SEGMENT (pack.h TokenSegments) ----
// A workgroup takes WC_RUN consecutive segments.  Column tau of segment q is position 32 tile(q) + tau; it is live iff the position's
// token is the segment's, and then gathers column pos_head[position] of W_h [C][Gh] -- with shared block heads the L blocks' positions
// of one leaf read one column.  Positions of another token, or of padding, are zero rows, as pack_segments leaves them; the split is
// publish_wcat_kernel's.  b_cat in packed order is written by the one segment a position is live in (padding keeps the load's zero).
__global__ void __launch_bounds__(256) publish_wcat_segments_kernel(const float* __restrict__ wcat, const float* __restrict__ bsrc,
                                                                    const int32_t* __restrict__ pos_head, const int32_t* __restrict__ pos_token,
                                                                    const int32_t* __restrict__ seg_tile, const int32_t* __restrict__ seg_token,
                                                                    uint16_t* __restrict__ hi, uint16_t* __restrict__ lo, float* __restrict__ bc,
                                                                    int Gh, int nseg, int KS) {
  const int q0 = blockIdx.x * WC_RUN;
  const int tid = threadIdx.x;
  int ref[2], slot[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col = tid + 256 * c, sl = col >> 5, tau = col & 31;
    ref[c] = -1;
    slot[c] = sl * 64 + rho_of_tau(tau);
    if (q0 + sl < nseg) {
      const int pos = seg_tile[q0 + sl] * 32 + tau;
      if (pos_token[pos] == seg_token[q0 + sl]) {
        ref[c] = pos_head[pos];
        bc[pos] = bsrc[ref[c]];
      }
    }
  }
  wcat_ksteps(wcat, Gh, ref, slot, q0, nseg, KS, hi, lo);
}

hipError_t launch_publish(const PublishArgs& a, hipStream_t st) {
  const TrainLayout L = make_train_layout(a.g);
  const CopyTable ct = ctx_table(a.g, L);
  const int ctx_layers = ct.layers > 0 ? ct.layers : 1;
  hipLaunchKernelGGL(publish_copy_kernel, dim3(16, ct.nseg, ctx_layers), dim3(256), 0, st, a.params, a.hn, ct);
  const int Gtot = a.Gtot, ntiles = Gtot / 32;
  if (a.g.layer_tokens)
    hipLaunchKernelGGL(publish_wcat_segments_kernel, dim3((a.nseg + WC_RUN - 1) / WC_RUN), dim3(256), 0, st, a.params + L.wcat, a.params + L.bcat,
                       a.pos_head, a.pos_token, a.seg_tile, a.seg_token, a.wcat_hi, a.wcat_lo, a.bcat, (int)L.Gh, a.nseg, a.g.C / 16);
  else
    hipLaunchKernelGGL(publish_wcat_kernel, dim3((ntiles + WC_RUN - 1) / WC_RUN), dim3(256), 0, st, a.params + L.wcat, a.params + L.bcat,
                       a.perm, a.wcat_hi, a.wcat_lo, a.bcat, (int)L.G, ntiles, a.g.C / 16);
  if (a.train_encoder) {
    const EncMap m = enc_map(a.g, L);
    const int enc_layers = m.layers > 0 ? m.layers : 1;
    hipLaunchKernelGGL(publish_copy_kernel, dim3(2, m.vec.nseg, enc_layers), dim3(256), 0, st, a.params, a.encf32, m.vec);
    const int npos = m.S * m.E;
    hipLaunchKernelGGL(publish_pos_kernel, dim3((npos + 1023) / 1024), dim3(256), 0, st, a.params + m.src_pos, a.params + m.src_cls,
                       a.encf32 + m.f_pos, m.E, npos);
    hipLaunchKernelGGL(publish_patch_kernel, dim3((m.E + 63) / 64), dim3(64), 0, st, a.params + m.src_pk, a.params + m.src_pb, a.enc16,
                       a.encf32 + m.f_bpatch, m.E, m.Kreal, m.Kp, a.bf);
    if (m.layers > 0)
      hipLaunchKernelGGL(publish_transpose_kernel, dim3(m.tiles_per_layer, m.layers), dim3(256), 0, st, a.params, a.enc16, a.encd16, m,
                         a.bf);
  }
  return hipGetLastError();
}

}  // namespace hvla
