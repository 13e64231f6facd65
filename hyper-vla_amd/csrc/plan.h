// plan.h -- everything run_encoder decides from sizes alone (no HIP types): which kernel instantiation runs for every dense product,
// its grid and LDS size, whether a LayerNorm or mean-row launch follows, the attention launch, the memsets.  encoder.hip fills
// pointers and launches what the plan says; a CPU test drives the same functions at sizes no test batch reaches and compares them,
// launch for launch, with a trace recorded from the dispatch they replaced (tests/native/plan_check.cpp, built with g++ under
// ASan / UBSan by tests/test_host_sanitizers.py).  Also the tile and stage constants host and kernels share, and the tile-order
// arithmetic of the 64 x 64 and 128 x 128 GEMM kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define HVLA_HD __host__ __device__ __forceinline__
#else
#define HVLA_HD inline
#endif

namespace hvla {

// Workgroups are dealt round-robin over the chip's 8 XCDs (block b runs on XCD b % 8), each with an L2 of its own.  xcd_run maps
// the block id to a linear tile index such that XCD x owns the x-th of 8 CONTIGUOUS runs of tile indices (the first nwg % 8 runs one
// longer): a bijection of [0, nwg) for every nwg >= 1.  Tiles that share an operand panel are made neighbours in the linear order,
// so the panel crosses the fabric once per XCD that a run boundary puts it on (at most two) instead of once per L2.
HVLA_HD int xcd_run(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

// A GEMM output of 96 MB or more is not found in L2 / the memory-side cache by the kernel that reads it next: the 16-bit outputs
// of QKV / fc1 are then stored non-temporally and the f32 residual rows read non-temporally (gemm256p_kernel<..., NT>).
HVLA_HD bool big_output(size_t rows, size_t cols, size_t elem_bytes) { return rows * cols * elem_bytes >= ((size_t)96 << 20); }

// The non-temporal 16-bit stores of the QKV / GELU epilogues are buffer stores with ONE 32-bit BYTE offset per lane (the rows as
// scalar offsets): an output of 4 GiB or more cannot be addressed that way and takes the flat-store form (element offsets, good to
// 2^32 ELEMENTS, which run_encoder checks for every batch).  fc1 at S = 257, F = 3072: from B = 2721 on.
HVLA_HD bool nt16_addressable(size_t rows, size_t cols, size_t elem_bytes) { return rows * cols * elem_bytes < ((size_t)1 << 32); }

// ------------------------------------------------------------------------------------------------ tile and stage constants
// (what each kernel does with them is told at the kernel, encoder.hip)
enum { EPI_PATCH = 0, EPI_QKV = 1, EPI_GELU = 2, EPI_RES = 3, EPI_CORR = 4 };   // CORR: out f32 = bias + acc / 4096 (gemm64_kernel's second problem)
constexpr int GBM = 128, GBN = 128, GBK = 64, GLD = 72;   // gemm_kernel; GLD: padded LDS row (halves) = 144 B
constexpr int SBM = 64, SBN = 64, SNS = 6, SST = 16384;   // gemm64_kernel: stages (6, or 4 for two workgroups per CU) x 16 KB
constexpr int SNSC = 5, SSTC = 28672;   // gemm64c_kernel: stages x (A 8 KB | W 8 KB | dW 8 KB | mean rows 4 KB)
constexpr int SSTF = 24576;             // ... FOLD: a stage is A | W | dW, the mean rows of all K-tiles sit behind the stages
constexpr size_t gemm64c_fold_lds(int K) { return (size_t)SNSC * SSTF + (size_t)(K / 64) * 2048; }
constexpr int SNS32 = 7, SST32 = 20480; // gemm64c32_kernel
constexpr int HBM_ = 256, HBN_ = 256;   // gemm256p_kernel
constexpr size_t P256_LDS = 131072;     // ... its LDS: 2 buffers x (A 32 KB | W 32 KB)
constexpr int LNW = 16;                 // waves of a LayerNorm workgroup
constexpr int LNG = 8;                  // row groups per image of layernorm_group_kernel = partial column sums per image: [half][fq]
constexpr int APS = 68;                 // attention: floats per partial of the last query: max, sum, 2 unused, O[64] (16-byte aligned)
constexpr int AVLD = 64;                // attention: V row stride (halves): 128 B, 64-B halves swapped on rows with bit 1 set
constexpr int G64_MAXM = 2047;          // rows up to which a GEMM is cut into 64x64 tiles (pure latency below that)
constexpr size_t LDS_LIMIT = 160 * 1024;   // the dynamic-LDS limit every kernel of the tables is raised to
constexpr int CAT_COMP = 8;             // HVLA_PROF_COMP
// attention_kernel's LDS: K and V [KT * 32][AVLD], the last query, its KT partials, per-wave column sums (+ the exported row)
constexpr size_t attention_lds(int KT, size_t elem, bool amap) {
  return (size_t)KT * 32 * 2 * AVLD * elem + (size_t)KT * APS * sizeof(float) + 64 * elem + (size_t)(KT - 1) * 64 * sizeof(float) +
         (amap ? (size_t)(KT * 32 + 32) * sizeof(float) : 0);
}

// ------------------------------------------------------------------------------------------------ kernel ids
// Every GEMM instantiation of the encoder, ONCE: X(id, kernel).  encoder.hip expands the list into its table id -> void (*)(GemmArgs)
// (attribute loop, launches, debug_gemm), this file into the ids, the CPU test into their names.  Inside a family the order is
// epilogue-major, PERSIST last, so that the plan picks an id by arithmetic (the static_asserts below).
#define HVLA_GEMM_KERNELS(X) \
  X(G128_PATCH, gemm_kernel<Op, EPI_PATCH>) X(G128_QKV, gemm_kernel<Op, EPI_QKV>) X(G128_GELU, gemm_kernel<Op, EPI_GELU>) \
  X(G128_RES, gemm_kernel<Op, EPI_RES>) \
  X(G64_PATCH, gemm64_kernel<Op, EPI_PATCH>) X(G64_QKV, gemm64_kernel<Op, EPI_QKV>) X(G64_GELU, gemm64_kernel<Op, EPI_GELU>) \
  X(G64_RES, gemm64_kernel<Op, EPI_RES>) X(G64_CORR, gemm64_kernel<Op, EPI_CORR>) \
  X(G64S4_QKV, gemm64_kernel<Op, EPI_QKV, 4>) X(G64S4_GELU, gemm64_kernel<Op, EPI_GELU, 4>) X(G64S4_RES, gemm64_kernel<Op, EPI_RES, 4>) \
  X(G64C_QKV, gemm64c_kernel<Op, EPI_QKV>) X(G64C_GELU, gemm64c_kernel<Op, EPI_GELU>) X(G64C_RES, gemm64c_kernel<Op, EPI_RES>) \
  X(G64CF_QKV, gemm64c_kernel<Op, EPI_QKV, true>) X(G64CF_GELU, gemm64c_kernel<Op, EPI_GELU, true>) X(G64C32, gemm64c32_kernel<Op>) \
  X(G256_PATCH, gemm256p_kernel<Op, EPI_PATCH, false>) X(G256_PATCH_P, gemm256p_kernel<Op, EPI_PATCH, true>) \
  X(G256_QKV, gemm256p_kernel<Op, EPI_QKV, false>) X(G256_QKV_P, gemm256p_kernel<Op, EPI_QKV, true>) \
  X(G256_GELU, gemm256p_kernel<Op, EPI_GELU, false>) X(G256_GELU_P, gemm256p_kernel<Op, EPI_GELU, true>) \
  X(G256_RES, gemm256p_kernel<Op, EPI_RES, false>) X(G256_RES_P, gemm256p_kernel<Op, EPI_RES, true>) \
  X(G256NT_QKV, gemm256p_kernel<Op, EPI_QKV, false, false, true>) X(G256NT_QKV_P, gemm256p_kernel<Op, EPI_QKV, true, false, true>) \
  X(G256NT_GELU, gemm256p_kernel<Op, EPI_GELU, false, false, true>) X(G256NT_GELU_P, gemm256p_kernel<Op, EPI_GELU, true, false, true>) \
  X(G256NT_RES, gemm256p_kernel<Op, EPI_RES, false, false, true>) X(G256NT_RES_P, gemm256p_kernel<Op, EPI_RES, true, false, true>) \
  X(G256LN_PATCH, gemm256p_kernel<Op, EPI_PATCH, false, true>) X(G256LN_PATCH_P, gemm256p_kernel<Op, EPI_PATCH, true, true>) \
  X(G256LN_RES, gemm256p_kernel<Op, EPI_RES, false, true>) X(G256LN_RES_P, gemm256p_kernel<Op, EPI_RES, true, true>) \
  X(G256LNNT_RES, gemm256p_kernel<Op, EPI_RES, false, true, true>) X(G256LNNT_RES_P, gemm256p_kernel<Op, EPI_RES, true, true, true>)
enum GemmKernel : int {
#define HVLA_X(id, ...) id,
  HVLA_GEMM_KERNELS(HVLA_X)
#undef HVLA_X
  NUM_GEMM_KERNELS
};
static_assert(G128_PATCH + EPI_RES == G128_RES && G64_PATCH + EPI_CORR == G64_CORR && G64S4_QKV - EPI_QKV + EPI_RES == G64S4_RES, "");
static_assert(G64C_QKV - EPI_QKV + EPI_RES == G64C_RES && G64CF_QKV - EPI_QKV + EPI_GELU == G64CF_GELU, "");
static_assert(G256_PATCH + 2 * EPI_RES + 1 == G256_RES_P && G256NT_QKV + 2 * (EPI_RES - EPI_QKV) + 1 == G256NT_RES_P, "");
static_assert(G256LN_PATCH + 1 == G256LN_PATCH_P && G256LN_RES + 1 == G256LN_RES_P && G256LNNT_RES + 1 == G256LNNT_RES_P, "");
// the attention instantiations (encoder.hip's second table) and the launches that have one instantiation each (named in traces only)
enum AttnKernel : int { ATT, ATT_U, ATT_MAP, NUM_ATTN_KERNELS };   // rolled | unrolled (S = 257) | also exports the CLS query's attention row
enum OtherKernel : int { IM2COL = 100, LN_GROUP, LN_MEAN, COLMEAN, LN_FINAL };

// ------------------------------------------------------------------------------------------------ the plan
struct Launch {
  int kernel = -1;                 // < 0: no launch
  unsigned grid = 0, grid_y = 1, block = 0;
  size_t lds = 0;
  int cat = -1;                    // profiler category that brackets it (include/hvla.h HVLA_PROF_*; < 0: none)
  explicit operator bool() const { return kernel >= 0; }
};
struct EncSizes {                  // what an encoder call is decided from
  int B, P, S, E, F, H, patch, layers;
  int ncu;
  size_t elem;                     // bytes of a 16-bit operand element
  bool comp, ln_ws, amap;          // weight-rounding compensation on | the fused LayerNorms' workspace exists | attention-map export
  int M() const { return B * S; }
};
HVLA_HD int ceil_div(int a, int b) { return (a + b - 1) / b; }

// What the fused LayerNorms keep in the workspace, sized by the limits above: an image has at most LNX_MAX_E / HBN_ column tiles,
// a tile leaves one 16-byte entry {sum, tag, sum of squares, tag} per row, every image has one 4-byte arrival word, and the words
// of a call are cleared (and a half batch's words begin) in multiples of 16 bytes.
constexpr int LNX_MAX_E = 1024;                          // can_fuse_ln's width limit
constexpr int LNX_TILES = LNX_MAX_E / HBN_;              // column tiles per image the workspace has room for
constexpr int LNX_ENTRY_BYTES = 16, LNX_CNT_ALIGN = 16;
static_assert(LNX_TILES == 4 && LNX_MAX_E % HBN_ == 0, "");
inline size_t lnx_cnt_bytes(int nb) { return ((size_t)nb * sizeof(uint32_t) + LNX_CNT_ALIGN - 1) / LNX_CNT_ALIGN * LNX_CNT_ALIGN; }
inline size_t lnx_part_bytes(int nb, int E) { return (size_t)nb * ((E + HBN_ - 1) / HBN_) * HBM_ * LNX_ENTRY_BYTES; }

// small batch: does the GEMM [M][K] x [N][K] run as gemm64c_kernel (bias rows computed inside)?
// (S >= 9: a block's 64 rows then belong to at most 8 images = the 16 rows of the kernels' bias-row tile)
inline bool small_fused(const EncSizes& z, int N, int K) {
  return z.comp && z.M() <= G64_MAXM && (size_t)z.M() * K < (1ull << 31) && (size_t)N * K < (1ull << 31) && N % SBN == 0 && K % 64 == 0 && z.S >= 9;
}
// may a residual / patch GEMM on image-aligned tiles run the LayerNorm behind it inside its epilogue (LNX)?
inline bool can_fuse_ln(const EncSizes& z) { return z.ln_ws && (size_t)z.M() * z.E * 4 < (1ull << 32) && z.E <= LNX_MAX_E; }
// the persistent form of an LNX launch keeps the nbn column tiles of an image in one round (tile_origin_x): the counts must divide
inline bool lnx_persistent(int ncu, int nbm, int nbn) {
  const int nt = nbm * nbn;
  if (ncu % 8 || nt % ncu || nbm % 8) return false;
  const int Wx = ncu / 8, odd = Wx % nbn, R = nt / ncu;
  return Wx >= nbn && (odd == 0 || R % nbn == 0);
}

struct GemmPlan {
  Launch small;                    // in front, HVLA_PROF_COMP: the B CLS rows (+ the 2 B mean rows -> corr) when `aligned`, else the corr-only table
  Launch main;
  bool aligned = false;            // image-aligned 256-row tiles: tile_row0 / tile_stride / nbm hold, a GELU epilogue wrote the mean rows itself
  bool fused_bias = false;         // gemm64c forms: the bias rows are computed inside (abar2 / dW2 / M2 of the MAIN launch)
  bool fold = false;               // ... from the partials the LayerNorm in front left (FOLD)
  bool ln_fused = false;           // the LayerNorm behind this GEMM runs inside its epilogue
  int tile_row0 = 0, tile_stride = 256, nbm = 0, nbn = 0;
  int lnx_G = 0, lnx_rows_aligned = 0, lnx_rounds_div = 0, lnx_rows_xcd = 0, lnx_rcp = 0;   // GemmArgs::lnx_* (persistent LNX only)
};
// the LNX launch of an image-aligned GEMM: base = the non-persistent instantiation
inline void plan_lnx(const EncSizes& z, GemmPlan& p, int base) {
  const bool persist = lnx_persistent(z.ncu, p.nbm, p.nbn);
  p.main.kernel = base + persist;
  p.main.grid = persist ? z.ncu : p.nbm * p.nbn;
  p.ln_fused = true;
  if (persist) {
    const int Wx = z.ncu / 8, R = p.nbm * p.nbn / z.ncu;
    p.lnx_G = Wx / p.nbn; p.lnx_rows_aligned = R * p.lnx_G; p.lnx_rounds_div = R / p.nbn; p.lnx_rows_xcd = p.nbm / 8;
    p.lnx_rcp = (65536 + p.nbn - 1) / p.nbn;
  }
}
// One dense product of the encoder, [rows][K] x [N][K]: the patch embedding (epi = EPI_PATCH: B * P rows, K = Kp) or a layer GEMM
// (B * S rows).  ln_follows: a LayerNorm reads the output next (RES; PATCH: layers > 0); ln_partial: the LayerNorm in front left its
// partial sums to this launch (plan_norm's fold).
//  * images of 256 patches, more than 2047 rows, N % 64 == 0, N >= 256: ONE gemm64_kernel launch for the 2 B latency-bound rows (the
//    B CLS rows, stride S, plain bias; the 2 B mean rows against dW -> corr), then gemm256p_kernel over image-aligned tiles (tile row
//    b = rows b*S + 1 .. b*S + 256) with corr as its bias rows.  (N % 256 != 0, DINOv2-small: the last tile column is 64, 128 or 192
//    wide, the rest of its MFMAs wasted -- still twice as fast as the 128 x 128 register-staged kernel.)
//  * up to 2047 rows with compensation: gemm64c_kernel, bias rows inside;
//  * otherwise a corr-only gemm64_kernel launch, then gemm64_kernel (<= 2047 rows) or gemm_kernel (128x128 tiles), bias row looked up per row.
// The patch embedding has no CLS rows and no mean rows (no small launch), no non-temporal form, and its tile rows are images only
// when P = 256 (LNX only then).
inline GemmPlan plan_gemm(const EncSizes& z, int epi, int N, int K, int cat, bool ln_follows, bool ln_partial) {
  GemmPlan p;
  const int B = z.B, ncu = z.ncu, M = epi == EPI_PATCH ? B * z.P : z.M();
  const bool fits32 = (size_t)M * K < (1ull << 31) && (epi == EPI_PATCH || (size_t)N * K < (1ull << 31));
  p.main.block = 256;
  p.main.cat = cat;
  p.nbn = ceil_div(N, HBN_);
  p.aligned = N % SBN == 0 && N >= HBN_ && M > G64_MAXM && fits32 &&
              (epi == EPI_PATCH ? M % HBM_ == 0 : z.P == HBM_ && K >= 128 && K % 64 == 0);
  if (p.aligned) {
    p.main.block = 512;
    p.main.lds = P256_LDS;
    if (epi == EPI_PATCH) {
      p.nbm = M / HBM_; p.tile_row0 = 0; p.tile_stride = HBM_;
      if (z.P == HBM_ && can_fuse_ln(z) && ln_follows) { plan_lnx(z, p, G256LN_PATCH); return p; }   // a tile row is an image: norm1 of layer 0 inside the epilogue
    } else {
      int nblocks = ceil_div(B, SBM) * (N / SBN);
      if (z.comp) nblocks += ceil_div(2 * B, SBM) * (N / SBN);       // two mean rows per image
      // (a three-stage form, three workgroups per CU for the launches above 512 blocks, was tried: run-to-run different
      // tokens in ~4 % of the episodes of a 1024-episode batch, whichever order the reads and the DMA issue are in, while
      // the four- and six-stage forms are clean -- not understood, not used: profiles/r3_experiments_not_kept.txt)
      const bool two_per_cu = nblocks > ncu;
      p.small = Launch{two_per_cu ? G64S4_QKV - EPI_QKV + epi : G64_PATCH + epi, (unsigned)nblocks, 1, 256, (size_t)(two_per_cu ? 4 : SNS) * SST, CAT_COMP};
      p.nbm = B; p.tile_row0 = 1; p.tile_stride = z.S;
      // a big batch: the 16-bit output goes past L2, the f32 residual rows are read past it (see the epilogue)
      if (epi == EPI_RES && ln_follows && can_fuse_ln(z)) {
        plan_lnx(z, p, big_output(M, N, sizeof(float)) ? G256LNNT_RES : G256LN_RES);
        return p;
      }
      // (the 16-bit NT stores carry 32-bit BYTE offsets: an output of 4 GiB or more takes the plain form -- ADVICE r5)
      if (big_output(M, N, epi == EPI_RES ? sizeof(float) : z.elem) && (epi == EPI_RES || nt16_addressable(M, N, z.elem))) {
        const bool persist = (B * p.nbn) % ncu == 0;
        p.main.kernel = G256NT_QKV + 2 * (epi - EPI_QKV) + persist;
        p.main.grid = persist ? ncu : B * p.nbn;
        return p;
      }
    }
    const bool persist = (p.nbm * p.nbn) % ncu == 0;
    p.main.kernel = G256_PATCH + 2 * epi + persist;
    p.main.grid = persist ? ncu : p.nbm * p.nbn;
    return p;
  }
  if (epi != EPI_PATCH && small_fused(z, N, K)) {            // (no launch of its own for the bias rows: nothing is timed as HVLA_PROF_COMP)
    const int nb64 = ceil_div(M, SBM) * (N / SBN);
    p.fused_bias = true;
    if (epi != EPI_RES && ln_partial) {
      p.fold = true;
      p.main.kernel = G64CF_QKV - EPI_QKV + epi; p.main.grid = nb64; p.main.lds = gemm64c_fold_lds(K);
    } else if (epi == EPI_RES && 2 * nb64 <= ncu) {          // less than half of the chip: 64 x 32 tiles on twice as many CUs
      p.main.kernel = G64C32; p.main.grid = 2 * nb64; p.main.lds = (size_t)SNS32 * SST32;
    } else {
      p.main.kernel = G64C_QKV - EPI_QKV + epi; p.main.grid = nb64; p.main.lds = (size_t)SNSC * SSTC;
    }
    return p;
  }
  if (epi != EPI_PATCH && z.comp)                            // the same gemm64_body<EPI_CORR> arithmetic as the fused launch above
    p.small = Launch{G64_CORR, (unsigned)(ceil_div(2 * B, SBM) * (N / SBN)), 1, 256, (size_t)SNS * SST, CAT_COMP};
  if (M <= G64_MAXM && fits32 && N % SBN == 0 && (epi == EPI_PATCH || K % 64 == 0)) {
    p.main.kernel = G64_PATCH + epi; p.main.grid = ceil_div(M, SBM) * (N / SBN); p.main.lds = (size_t)SNS * SST;
  } else {
    p.main.kernel = G128_PATCH + epi; p.main.grid = ceil_div(M, GBM) * (N / GBN); p.main.lds = (size_t)2 * (GBM + GBN) * GLD * z.elem;
  }
  return p;
}

// norm1 / norm2 as launches of their own (+ the column sums of the output).  Nnext: width of the GEMM that reads the output.
// scratch_cols: a 16-bit [M][scratch_cols] workspace buffer is free from this launch until its consumer GEMM has ENDED, for the partial
// column sums [B][LNG][E] f32 -- if it has room.
// (one launch with the image's last workgroup to arrive -- ticket by atomicAdd behind a __threadfence -- adding the
// partials was tried: 14.0 us against 5.2 + 4.7 for the two launches, profiles/r3_experiments_not_kept.txt)
// fold, B = 1: every workgroup of the consumer GEMM adds the partials up itself (gemm64c_kernel, FOLD) -- while that GEMM is ONE round
// of workgroups (round 4, same box: B = 1 1.250 against 1.270 ms per step with the separate launch; B = 4 1.93 against 1.85).
struct NormPlan {
  Launch group, mean;              // layernorm_group_kernel | layernorm_mean_kernel (only when the partials are written and not folded)
  bool partial = false, fold = false;
};
inline NormPlan plan_norm(const EncSizes& z, int Nnext, int scratch_cols) {
  NormPlan n;
  n.group = Launch{LN_GROUP, LNG, (unsigned)z.B, LNW * 64, (size_t)(z.P / 8) * z.E * sizeof(float), 1};
  n.partial = z.comp && (size_t)LNG * z.E * sizeof(float) <= (size_t)z.S * scratch_cols * z.elem;
  n.fold = n.partial && small_fused(z, Nnext, z.E) && gemm64c_fold_lds(z.E) <= LDS_LIMIT && ceil_div(z.M(), SBM) * (Nnext / SBN) <= z.ncu;
  if (n.partial && !n.fold) n.mean = Launch{LN_MEAN, 2u * z.B, 1, 256, 0, 1};
  return n;
}

// one workgroup per (image, head), one wavefront per 32-query block
inline Launch plan_attention(int B, int S, int H, size_t elem, bool amap) {
  const int KT = (S + 31) / 32;                            // S = 32 * (KT - 1) + 1
  // (unrolled, the attention-map instantiation spills: it stays rolled)
  return Launch{amap ? ATT_MAP : KT == 9 ? ATT_U : ATT, (unsigned)(B * H), 1, (unsigned)(KT - 1) * 64, attention_lds(KT, elem, amap), 3};
}

// what a call decides once
struct CallPlan {
  bool ok = false;                 // false: refused (the GEMM epilogues address their outputs with 32-bit element offsets)
  int Kp = 0;                      // K of the patch GEMM: [a | a] x [W_hi | W_lo]
  size_t cnt_bytes = 0, part_bytes = 0;   // the fused LayerNorms' arrival words / entry tags are cleared first (0: no memsets)
  Launch im2col, attention, colmean, final_norm;   // (colmean: the mean rows of fc1's output when its epilogue did not write them)
};
inline CallPlan plan_call(const EncSizes& z) {
  CallPlan c;
  const int M = z.M();
  c.ok = (size_t)M * (size_t)(z.F > 3 * z.E ? z.F : 3 * z.E) < (1ull << 32);
  if (!c.ok) return c;
  c.Kp = 2 * ((z.patch * z.patch * 3 + 63) / 64 * 64);
  if (can_fuse_ln(z) && z.P == HBM_ && M > G64_MAXM) {
    c.cnt_bytes = lnx_cnt_bytes(z.B);
    c.part_bytes = lnx_part_bytes(z.B, z.E);
  }
  const size_t chunks = ((size_t)z.B * z.P * (c.Kp / 16) + 255) / 256;
  c.im2col = Launch{IM2COL, (unsigned)(chunks > 8192 ? 8192 : chunks), 1, 256, 0, 0};
  c.attention = plan_attention(z.B, z.S, z.H, z.elem, z.amap);
  if (z.comp) c.colmean = Launch{COLMEAN, (unsigned)ceil_div(z.F, 256), (unsigned)z.B, 256, 0, -1};
  c.final_norm = Launch{LN_FINAL, (unsigned)ceil_div(M, 4), 1, 256, 0, 1};
  return c;
}

// ------------------------------------------------------------------------------------------------ the workspace
// The eight buffers an encoder call works in (EncWorkspace, kernels.h), ONCE: how large each is for a context of max_batch episodes
// and where the slice of the episodes from b0 on begins.  hvla_create allocates by it and encode_range cuts by it, so the slices of
// the two halves of a two-stream step are disjoint, and each holds what run_encoder touches for its episodes, wherever the CPU test
// says so (plan_check.cpp: a sweep against the sizes and offsets recorded from the expressions this replaced).
enum WsBuf : int { WS_X, WS_H, WS_QKV, WS_G, WS_CORR, WS_ABAR, WS_LN_CNT, WS_LN_PART, NUM_WS };
struct WorkspacePlan {
  size_t max_batch = 0;
  size_t per[NUM_WS] = {};         // bytes per episode (ln_cnt: its 4-byte word; slices of it begin on LNX_CNT_ALIGN)
  WorkspacePlan() = default;
  WorkspacePlan(int P, int S, int E, int F, int Kp, int max_batch_) : max_batch((size_t)max_batch_) {
    const size_t s = (size_t)S, e = (size_t)E, f = (size_t)F, elem = 2, im2col = (size_t)P * Kp;   // (16-bit operands of either dtype)
    per[WS_X] = s * e * sizeof(float);                        // [S][E] f32 residual stream
    per[WS_H] = s * e * elem;                                 // [S][E]
    per[WS_QKV] = s * 3 * e * elem;                           // [S][3E]
    per[WS_G] = (s * f > im2col ? s * f : im2col) * elem;     // the MLP hidden rows [S][F] and, before them, the im2col rows [P][Kp]
    per[WS_CORR] = 2 * (f > 3 * e ? f : 3 * e) * sizeof(float);   // two bias rows per image (upper / lower half) of the widest GEMM
    per[WS_ABAR] = 2 * (f > e ? f : e) * elem;                // two mean rows per image of the widest activation operand
    per[WS_LN_CNT] = sizeof(uint32_t);
    per[WS_LN_PART] = (size_t)LNX_TILES * HBM_ * LNX_ENTRY_BYTES;
  }
  // (ln_cnt: each half of a two-stream step clears a multiple of LNX_CNT_ALIGN bytes from an aligned start, and 64 bytes to spare)
  size_t bytes(int buf) const { return buf == WS_LN_CNT ? (max_batch + 4) * per[buf] + 64 : max_batch * per[buf]; }
  size_t offset(int buf, int b0) const { return buf == WS_LN_CNT ? lnx_cnt_bytes(b0) : (size_t)b0 * per[buf]; }
};

}  // namespace hvla
