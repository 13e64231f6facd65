// train_gemm.hip — the batched GEMM of the fine-tune step and of t5.hip (train.h: bgemm() and its per-device timer): the split-bf16
// kernel on the bf16 matrix cores, the exact-f32 kernel behind libhvla_bench.so's switch, the tile chooser and the launch timer.
// The -DHVLA_TRAIN_TRACE builds of train.hip do not compile this file: tools/train_launch_trace.h defines the bgemm() they link.
#include <cstdint>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "train.h"

namespace hvla {

// ------------------------------------------------------------------------------------------------
// generic batched GEMM  C[b0,b1] (+)= alpha * op(A)[b0,b1] * op(B)[b0,b1] (+ bias[b0][n])
// ------------------------------------------------------------------------------------------------

// 64x64 output tile per workgroup, 4 waves x (32x32) on the exact-f32 matrix instruction
// v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain, guide §3): lane l supplies A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31], so both operands are conflict-free row reads of the k-major LDS tiles.
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void bgemm_kernel(BG g) {
  __shared__ float As[16][64];
  __shared__ float Bs[16][64];
  const int zb = blockIdx.z / g.ksplit, kc = blockIdx.z % g.ksplit;
  const int b0 = zb / g.nb1, b1 = zb % g.nb1;
  const int kchunk = ((g.K + g.ksplit - 1) / g.ksplit + 15) & ~15;
  const int kbeg = kc * kchunk, kend = kbeg + kchunk < g.K ? kbeg + kchunk : g.K;
  const float* A = g.A + b0 * g.sA0 + b1 * g.sA1;
  const float* B = g.B + b0 * g.sB0 + b1 * g.sB1;
  float* C = g.C + b0 * g.sC0 + b1 * g.sC1;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave >> 1, wn = wave & 1, col = lane & 31, half = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = kbeg; k0 < kend; k0 += 16) {
    for (int i = threadIdx.x; i < 64 * 16; i += 256) {
      int mm, kk;
      if (TA) { mm = i & 63; kk = i >> 6; } else { kk = i & 15; mm = i >> 4; }
      const int m = m0 + mm, k = k0 + kk;
      float v = 0.f;
      if (m < g.M && k < kend) v = TA ? A[(long)k * g.lda + m] : A[(long)m * g.lda + k];
      As[kk][mm] = v;
    }
    for (int i = threadIdx.x; i < 64 * 16; i += 256) {
      int nn, kk;
      if (TB) { kk = i & 15; nn = i >> 4; } else { nn = i & 63; kk = i >> 6; }
      const int n = n0 + nn, k = k0 + kk;
      float v = 0.f;
      if (n < g.N && k < kend) v = TB ? B[(long)n * g.ldb + k] : B[(long)k * g.ldb + n];
      Bs[kk][nn] = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + half][wm * 32 + col], Bs[kk + half][wn * 32 + col], acc, 0, 0, 0);
    __syncthreads();
  }
  const float* bias = g.bias ? g.bias + b0 * g.sBias0 + b1 * g.sBias1 : nullptr;
  const int n = n0 + wn * 32 + col;
  if (n >= g.N) return;
  const float bn = bias && kc == 0 ? bias[n] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + crow(r, half);
    if (m >= g.M) continue;
    const float v = g.alpha * acc[r] + bn;
    float* c = C + (long)m * g.ldc + n;
    if (g.accumulate == 2 || g.ksplit > 1) unsafeAtomicAdd(c, v);          // several batches reduce into one C
    else *c = g.accumulate ? *c + v : v;
  }
}

// ------------------------------------------------------------------------------------------------
// The same product on the bf16 matrix cores at f32-class accuracy: every f32 operand element is split while it is
// staged into LDS, x = hi + lo (two bf16, 16 mantissa bits together), and each 16-deep k chunk costs three
// v_mfma_f32_32x32x16_bf16 (lo*hi + hi*lo + hi*hi; the dropped lo*lo term is 2^-16 relative) -- about 5x the f32
// instruction's rate.  Operands are staged without transposition whatever their layout in memory (see stage_load).
// 4 waves as 2 x 2, BM x BN in {128 x 128, 64 x 64}, k steps of 32 with three steps of global loads in flight.
// ------------------------------------------------------------------------------------------------
// Staging of one BR x 32 operand tile (f32 in memory -> hi / lo bf16 planes in LDS), two flavours:
//   T = false  source is k-contiguous (rows of 32 floats): LDS image [row][32] with XOR-swizzled 16-byte chunks; fragments by ds_read_b128
//   T = true   source is row-contiguous (memory [k][row]): LDS image [k][BR + 32], no transposition while staging;
//              the fragment's k-in-lane order comes from ds_read_b64_tr_b16 (two per plane and k chunk)
// Either way a thread moves float4's along the contiguous dimension (scalar fallback for unaligned / edge pieces).
// Loads are branch-free so that the compiler keeps counted s_waitcnt vmcnt: VEC = one float4 per piece (host guarantees
// 16-byte alignment and that pieces never straddle the K / row edge), else 4 dwords.
// Out-of-range pieces are read from this block of zeros: selecting the ADDRESS keeps the load free of any instruction that
// consumes its result (a `v = ok ? v : 0` after the load would make the wave wait for the data right there and undo the
// prefetch).
__device__ __attribute__((aligned(16))) float hvla_zero_piece[4] = {0.f, 0.f, 0.f, 0.f};

// The loads are written as inline asm so that the compiler does not track them: it would otherwise place its own
// (conservative, often vmcnt(0)) waits wherever it schedules the consumers and drain the younger stages with them.  The
// kernel waits for exactly one stage with a constant s_waitcnt vmcnt and pins the consumers behind it with tie().
// One stage of one operand in registers: P pieces of 4 consecutive elements, as float4 tuples (VEC) or as 4P scalars.
// Each register is written by exactly one asm load and first touched again by tie() after the wait -- never copied in
// between (the hardware does not interlock a VGPR read against a load still in flight).
template <int P, bool VEC> struct StageRegs;
template <int P> struct StageRegs<P, true> {
  f32x4 v[P];
  __device__ __forceinline__ float get(int j, int c) const { return v[j][c]; }
};
template <int P> struct StageRegs<P, false> {
  float f[4 * P];
  __device__ __forceinline__ float get(int j, int c) const { return f[4 * j + c]; }
};
#define HVLA_T(x) "+v"(x)
__device__ __forceinline__ void tie(StageRegs<4, true>& r) { asm volatile("" : HVLA_T(r.v[0]), HVLA_T(r.v[1]), HVLA_T(r.v[2]), HVLA_T(r.v[3])::"memory"); }
__device__ __forceinline__ void tie(StageRegs<2, true>& r) { asm volatile("" : HVLA_T(r.v[0]), HVLA_T(r.v[1])::"memory"); }
__device__ __forceinline__ void tie(StageRegs<2, false>& r) {
  asm volatile("" : HVLA_T(r.f[0]), HVLA_T(r.f[1]), HVLA_T(r.f[2]), HVLA_T(r.f[3]), HVLA_T(r.f[4]), HVLA_T(r.f[5]), HVLA_T(r.f[6]), HVLA_T(r.f[7])::"memory");
}
__device__ __forceinline__ void tie(StageRegs<4, false>& r) {
  asm volatile("" : HVLA_T(r.f[0]), HVLA_T(r.f[1]), HVLA_T(r.f[2]), HVLA_T(r.f[3]), HVLA_T(r.f[4]), HVLA_T(r.f[5]), HVLA_T(r.f[6]), HVLA_T(r.f[7]),
               HVLA_T(r.f[8]), HVLA_T(r.f[9]), HVLA_T(r.f[10]), HVLA_T(r.f[11]), HVLA_T(r.f[12]), HVLA_T(r.f[13]), HVLA_T(r.f[14]), HVLA_T(r.f[15])::"memory");
}
#undef HVLA_T

template <bool T, int BR, bool VEC, int NTH = 256>
__device__ __forceinline__ void stage_load(const float* __restrict__ P, int ld, int r0, int R, int k0, int kend,
                                           StageRegs<BR * 8 / NTH, VEC>& out) {
#pragma unroll
  for (int j = 0; j < BR * 8 / NTH; ++j) {
    const int idx = threadIdx.x + j * NTH;
    const int r = r0 + (T ? (idx % (BR / 4)) * 4 : idx >> 3), k = k0 + (T ? idx / (BR / 4) : (idx & 7) * 4);
    const bool ok = r < R && k < kend;
    const float* p = P + (T ? (long)k * ld + r : (long)r * ld + k);     // the 4 elements of a piece are adjacent in memory
    if constexpr (VEC) {
      const float* q = ok ? p : hvla_zero_piece;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(out.v[j]) : "v"(q) : "memory");
    } else {
      const int lim = T ? R - r : kend - k;               // valid elements in this piece (<= 0: none)
      const float* z = hvla_zero_piece;
      const float *q0 = ok ? p : z, *q1 = ok && lim > 1 ? p + 1 : z, *q2 = ok && lim > 2 ? p + 2 : z, *q3 = ok && lim > 3 ? p + 3 : z;
      asm volatile("global_load_dword %0, %1, off" : "=v"(out.f[4 * j + 0]) : "v"(q0) : "memory");
      asm volatile("global_load_dword %0, %1, off" : "=v"(out.f[4 * j + 1]) : "v"(q1) : "memory");
      asm volatile("global_load_dword %0, %1, off" : "=v"(out.f[4 * j + 2]) : "v"(q2) : "memory");
      asm volatile("global_load_dword %0, %1, off" : "=v"(out.f[4 * j + 3]) : "v"(q3) : "memory");
    }
  }
}
template <bool T, int BR, bool VEC, int NTH = 256>
__device__ __forceinline__ void stage_store(__bf16* __restrict__ hi, __bf16* __restrict__ lo, const StageRegs<BR * 8 / NTH, VEC>& in) {
#pragma unroll
  for (int j = 0; j < BR * 8 / NTH; ++j) {
    const int idx = threadIdx.x + j * NTH;
    const int o = T ? (idx / (BR / 4)) * (BR + 32) + (idx % (BR / 4)) * 4
                    : (idx >> 3) * 32 + ((((idx & 7) >> 1) ^ ((idx >> 4) & 3)) << 3) + (idx & 1) * 4;   // row = idx >> 3, see load_frag
    bf16x4 h, l;
    __bf16 a, b;
    split1(in.get(j, 0), a, b); h[0] = a; l[0] = b;
    split1(in.get(j, 1), a, b); h[1] = a; l[1] = b;
    split1(in.get(j, 2), a, b); h[2] = a; l[2] = b;
    split1(in.get(j, 3), a, b); h[3] = a; l[3] = b;
    *reinterpret_cast<bf16x4*>(hi + o) = h;
    *reinterpret_cast<bf16x4*>(lo + o) = l;
  }
}
typedef short hvla_tr4 __attribute__((__vector_size__(4 * sizeof(short))));
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* p0, const __bf16* p1) {   // p1 = 4 k rows below p0
  const hvla_tr4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) hvla_tr4*)p0);
  const hvla_tr4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) hvla_tr4*)p1);
  typedef short s8 __attribute__((ext_vector_type(8)));
  const s8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, v);
}
// fragment of the 32-row block starting at row rb, k chunk kk (0 / 16): lane l holds row rb + (l & 31), k = kk + 8 (l >> 5) + 0..7
template <bool T, int BR>
__device__ __forceinline__ Split8 load_frag(const __bf16* hi, const __bf16* lo, int rb, int kk, int lane) {
  Split8 f;
  if (!T) {
    // 64-byte rows, the 16-byte chunk index XORed with (row >> 1) & 3: the 8-byte stores of a half-wave (4 rows) and the
    // 16-byte reads of 8 consecutive rows both spread over all 64 banks (the padded [row][40] image had 2-way store conflicts)
    const int row = rb + (lane & 31);
    const int o = row * 32 + ((((kk >> 3) + (lane >> 5)) ^ ((row >> 1) & 3)) << 3);
    f.hi = *reinterpret_cast<const bf16x8*>(hi + o);
    f.lo = *reinterpret_cast<const bf16x8*>(lo + o);
  } else {
    // 16-lane group g = lane >> 4 covers rows rb + 16 (g & 1) .. + 15 at k half (g >> 1); lane 4q + p of the group
    // addresses LDS row (k) q, columns 4p .. 4p + 3 and receives its own column of the four rows
    constexpr int LDT = BR + 32;
    const int i = lane & 15, q = i >> 2, pp = i & 3;
    const int o = (kk + 8 * (lane >> 5) + q) * LDT + rb + 16 * ((lane >> 4) & 1) + 4 * pp;
    f.hi = tr_frag(hi + o, hi + o + 4 * LDT);
    f.lo = tr_frag(lo + o, lo + o + 4 * LDT);
  }
  return f;
}

// BM = 256 (with BN = 128): EIGHT waves as 4 x 2, the same 64 x 64 per wave -- for problems whose 128 x 128 grid is between one and
// two workgroups per CU (N = 768 at 8 224 rows: 390 tiles, 134 CUs with two and 122 with one; as 256 x 128 it is 198 tiles, one
// round, and a thread splits 24 instead of 32 values per k step).
template <bool TA, bool TB, int BM, int BN, bool VEC>
__global__ __launch_bounds__(BM == 256 ? 512 : 256, BM == 256 ? 1 : 2) void bgemm3_kernel(BG g) {
  constexpr int NTH = BM == 256 ? 512 : 256;               // threads
  constexpr int WM = BM == 256 ? 64 : BM / 2, WN = BN / 2, IM = WM / 32, IN = WN / 32;
  constexpr bool SA = TA, SB = !TB;                       // staging flavour: row-contiguous source?
  constexpr int NA = SA ? 32 * (BM + 32) : BM * 32, NB = SB ? 32 * (BN + 32) : BN * 32;
  // k steps of global loads in flight (register stages): three float4 stages, or two when every piece is 4 dwords
  // (the 6-bit vmcnt could not count three of those)
  constexpr int NST = VEC ? 3 : 2;
  constexpr int PA = BM * 8 / NTH, PB = BN * 8 / NTH;     // float4 pieces per thread and stage
  constexpr int LPS = (PA + PB) * (VEC ? 1 : 4);          // load instructions per stage
  __shared__ __attribute__((aligned(16))) __bf16 Ah[NA], Al[NA], Bh[NB], Bl[NB];
  const int zb = blockIdx.z / g.ksplit, kc = blockIdx.z % g.ksplit;
  const int b0 = zb / g.nb1, b1 = zb % g.nb1;
  const int kchunk = ((g.K + g.ksplit - 1) / g.ksplit + 31) & ~31;
  const int kbeg = kc * kchunk, kend = kbeg + kchunk < g.K ? kbeg + kchunk : g.K;
  const float* A = g.A + b0 * g.sA0 + b1 * g.sA1;
  const float* B = g.B + b0 * g.sB0 + b1 * g.sB1;
  float* C = g.C + b0 * g.sC0 + b1 * g.sC1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave >> 1, wn = wave & 1, col = lane & 31, half = lane >> 5;
  f32x16 acc[IM][IN];
#pragma unroll
  for (int a = 0; a < IM; ++a)
#pragma unroll
    for (int b = 0; b < IN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  StageRegs<PA, VEC> ra[NST];
  StageRegs<PB, VEC> rb[NST];
#pragma unroll
  for (int s2 = 0; s2 < NST; ++s2) {                      // steps past kend read the block of zeros
    stage_load<SA, BM, VEC, NTH>(A, g.lda, m0, g.M, kbeg + 32 * s2, kend, ra[s2]);
    stage_load<SB, BN, VEC, NTH>(B, g.ldb, n0, g.N, kbeg + 32 * s2, kend, rb[s2]);
  }
  // Whole groups of NST steps (a step past kend multiplies staged zeros), every step issues its refill: the number of
  // loads in flight is the same at every wait, so the wait for the oldest stage is the constant vmcnt((NST - 1) * LPS).
  for (int k0 = kbeg; k0 < kend; k0 += 32 * NST) {
#pragma unroll
    for (int s2 = 0; s2 < NST; ++s2) {
      const int kcur = k0 + 32 * s2;
      // raw barriers: a __syncthreads() would also drain the younger register stages' global loads (vmcnt(0))
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // the previous step's fragment reads are done
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 1) * LPS) : "memory");     // the oldest stage has landed
      tie(ra[s2]);
      tie(rb[s2]);
      stage_store<SA, BM, VEC, NTH>(Ah, Al, ra[s2]);
      stage_store<SB, BN, VEC, NTH>(Bh, Bl, rb[s2]);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // the LDS image is complete
      // refill this register stage NST steps ahead
      stage_load<SA, BM, VEC, NTH>(A, g.lda, m0, g.M, kcur + 32 * NST, kend, ra[s2]);
      stage_load<SB, BN, VEC, NTH>(B, g.ldb, n0, g.N, kcur + 32 * NST, kend, rb[s2]);
#pragma unroll
      for (int kk = 0; kk < 32; kk += 16) {
        Split8 fa[IM], fb[IN];
#pragma unroll
        for (int a = 0; a < IM; ++a) fa[a] = load_frag<SA, BM>(Ah, Al, wm * WM + a * 32, kk, lane);
#pragma unroll
        for (int b = 0; b < IN; ++b) fb[b] = load_frag<SB, BN>(Bh, Bl, wn * WN + b * 32, kk, lane);
#pragma unroll
        for (int a = 0; a < IM; ++a)
#pragma unroll
          for (int b = 0; b < IN; ++b) {
            acc[a][b] = mma32_x3(fa[a], fb[b], acc[a][b]);
          }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the refills past kend (zeros) are still in flight
  const float* bias = g.bias && kc == 0 ? g.bias + b0 * g.sBias0 + b1 * g.sBias1 : nullptr;
  // Straight-line epilogue per (full tile?, store mode): with per-element `m < M` branches and a run-time mode inside the
  // loops the compiler drains the memory counter in every predicated block, i.e. one store round trip after the other.
  auto store = [&](auto fullc, auto modec) {
    constexpr bool FULL = decltype(fullc)::value;
    constexpr int MODE = decltype(modec)::value;    // 0 store, 1 read-modify-write, 2 atomic add
#pragma unroll
    for (int b = 0; b < IN; ++b) {
      const int n = n0 + wn * WN + b * 32 + col;
      if (!FULL && n >= g.N) continue;
      const float bn = bias ? bias[n] : 0.f;
#pragma unroll
      for (int a = 0; a < IM; ++a) {
        float old[16];
        if constexpr (MODE == 1) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * WM + a * 32 + crow(r, half);
            old[r] = (FULL || m < g.M) ? C[(long)m * g.ldc + n] : 0.f;
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * WM + a * 32 + crow(r, half);
          if (!FULL && m >= g.M) continue;
          const float v = g.alpha * acc[a][b][r] + bn;
          float* c = C + (long)m * g.ldc + n;
          if constexpr (MODE == 2) unsafeAtomicAdd(c, v);
          else if constexpr (MODE == 1) *c = old[r] + v;
          else *c = v;
        }
      }
    }
  };
  using Yes = std::integral_constant<bool, true>;
  using No = std::integral_constant<bool, false>;
  using M0 = std::integral_constant<int, 0>;
  using M1 = std::integral_constant<int, 1>;
  using M2 = std::integral_constant<int, 2>;
  const bool full = m0 + BM <= g.M && n0 + BN <= g.N;
  const int mode = (g.accumulate == 2 || g.ksplit > 1) ? 2 : (g.accumulate ? 1 : 0);
  if (full) {
    if (mode == 2) store(Yes{}, M2{}); else if (mode == 1) store(Yes{}, M1{}); else store(Yes{}, M0{});
  } else {
    if (mode == 2) store(No{}, M2{}); else if (mode == 1) store(No{}, M1{}); else store(No{}, M0{});
  }
}

template <int BM, int BN, bool VEC>
static void launch_bgemm3(hipStream_t st, bool ta, bool tb, const BG& g, dim3 grid) {
  constexpr int NTH = BM == 256 ? 512 : 256;
  if (!ta && !tb) hipLaunchKernelGGL((bgemm3_kernel<false, false, BM, BN, VEC>), grid, dim3(NTH), 0, st, g);
  else if (!ta && tb) hipLaunchKernelGGL((bgemm3_kernel<false, true, BM, BN, VEC>), grid, dim3(NTH), 0, st, g);
  else if (ta && !tb) hipLaunchKernelGGL((bgemm3_kernel<true, false, BM, BN, VEC>), grid, dim3(NTH), 0, st, g);
  else hipLaunchKernelGGL((bgemm3_kernel<true, true, BM, BN, VEC>), grid, dim3(NTH), 0, st, g);
}

// the exact-f32 matrix instruction (bitwise fmaf chains) instead of the split-bf16 path: libhvla_bench.so only
// (hvla_debug_train_gemm_exact); the product library has no switch that changes its arithmetic
#ifdef HVLA_BENCH_HOOKS
static bool g_train_gemm_exact = false;
void set_train_gemm_exact(bool on) { g_train_gemm_exact = on; }
static bool train_gemm_exact() { return g_train_gemm_exact; }
static BgemmChoice g_bgemm_choice{0, 0, 0, 0};
const BgemmChoice& last_bgemm_choice() { return g_bgemm_choice; }
#define HVLA_BGEMM_CHOSE(tile, vec, ks, ex) (g_bgemm_choice = BgemmChoice{tile, vec, ks, ex})
#else
static constexpr bool train_gemm_exact() { return false; }
#define HVLA_BGEMM_CHOSE(tile, vec, ks, ex) ((void)0)
#endif

// Optional live timing of the batched GEMM launches (hvla_train_profile: bench.py --finetune's `roofline` block): HIP events on
// the launch stream around every bgemm() call and the f32-equivalent work of the call (2 M N K per batch entry; the split-bf16
// kernel spends three matrix instructions per product).  Off by default.  One timer per DEVICE (a context belongs to one device and
// the API entry points make it current before they launch; ADVICE r4: a process-wide timer mixed the contexts of two devices and
// never gave its events back): events are created on that device, destroyed by train_gemm_timer_release() from hvla_destroy, and a
// launch into a stream that is being captured is not timed (events recorded inside a capture cannot be read).  Not thread-safe
// (one training stream per device).
namespace {
struct GemmTimer {
  bool on = false;
  int users = 0;                      // contexts on this device that switched the timer on and are still alive (the events
                                      // go back when the LAST of them is destroyed, not when any of them is)
  std::vector<hipEvent_t> a, b;
  size_t used = 0;
  double flops = 0.0;
};
GemmTimer g_gemm_timer[64];
int g_gemm_timers_on = 0;             // devices whose timer is on: bgemm() asks for the current device only when this is not zero
GemmTimer* gemm_timer_here() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  return &g_gemm_timer[dev];
}
}  // namespace
void train_gemm_timer(bool on, bool first_use_by_this_context) {
  GemmTimer* t = gemm_timer_here();
  if (!t) return;
  if (first_use_by_this_context) ++t->users;
  if (t->on != on) g_gemm_timers_on += on ? 1 : -1;
  t->on = on;
}
void train_gemm_timer_release() {
  GemmTimer* t = gemm_timer_here();
  if (!t || t->users <= 0 || --t->users > 0) return;      // another live context of this device still uses the timer
  if (t->on) --g_gemm_timers_on;
  for (hipEvent_t e : t->a) (void)hipEventDestroy(e);
  for (hipEvent_t e : t->b) (void)hipEventDestroy(e);
  t->a.clear(), t->b.clear();
  t->used = 0, t->flops = 0.0, t->on = false;
}
hipError_t train_gemm_timer_read(float* ms, double* flops, int* launches) {
  *ms = 0.f; *flops = 0.0; *launches = 0;
  GemmTimer* tp = gemm_timer_here();
  if (!tp) return hipErrorInvalidDevice;
  GemmTimer& t = *tp;
  *flops = t.flops; *launches = (int)t.used;
  for (size_t i = 0; i < t.used; ++i) {
    hipError_t e = hipEventSynchronize(t.b[i]);
    if (e != hipSuccess) return e;
    float x = 0.f;
    if ((e = hipEventElapsedTime(&x, t.a[i], t.b[i])) != hipSuccess) return e;
    *ms += x;
  }
  t.used = 0; t.flops = 0.0;
  return hipSuccess;
}
static void bgemm_launch(hipStream_t st, bool ta, bool tb, BG g, int nb0);
void bgemm(hipStream_t st, bool ta, bool tb, BG g, int nb0) {
  if (g_gemm_timers_on == 0) { bgemm_launch(st, ta, tb, g, nb0); return; }
  GemmTimer* tp = gemm_timer_here();
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (!tp || !tp->on || hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { bgemm_launch(st, ta, tb, g, nb0); return; }
  GemmTimer& t = *tp;
  if (t.used == t.a.size()) {
    hipEvent_t x, y;
    if (hipEventCreate(&x) != hipSuccess) { bgemm_launch(st, ta, tb, g, nb0); return; }
    if (hipEventCreate(&y) != hipSuccess) { (void)hipEventDestroy(x); bgemm_launch(st, ta, tb, g, nb0); return; }
    t.a.push_back(x), t.b.push_back(y);
  }
  (void)hipEventRecord(t.a[t.used], st);
  bgemm_launch(st, ta, tb, g, nb0);
  (void)hipEventRecord(t.b[t.used], st);
  ++t.used;
  t.flops += 2.0 * g.M * g.N * g.K * (double)nb0 * g.nb1;
}
static void bgemm_launch(hipStream_t st, bool ta, bool tb, BG g, int nb0) {
  const bool exact = train_gemm_exact();
  const int T = !exact && g.M >= 96 && g.N >= 96 ? 128 : 64;
  // deep-K products onto few output tiles (shared-weight gradients: K = all rows of the batch) would leave most CUs
  // idle: cut K so that the grid has >= ~512 workgroups (two per CU; more only adds atomic traffic); legal whenever the result is accumulated (C zeroed before)
  const long tiles = (long)((g.N + T - 1) / T) * ((g.M + T - 1) / T) * nb0 * g.nb1;
  constexpr long want = 256;
  // two 128 x 128 workgroups fit on a CU: 512 workgroups (same box, alternating: step 37.70 -> 37.47 ms; 1 024: 39.2)
  constexpr long want_split = 512;
  if (g.allow_split && g.accumulate != 0 && g.ksplit == 1 && tiles < want_split && g.K >= 256) {
    long ks = (want_split + tiles - 1) / tiles, kmax = g.K / 128;
    g.ksplit = (int)(ks < kmax ? ks : kmax);
    if (g.ksplit < 1) g.ksplit = 1;
  }
  dim3 grid((g.N + T - 1) / T, (g.M + T - 1) / T, nb0 * g.nb1 * g.ksplit);
  if (!exact) {
    // float4 staging: 16-byte aligned pieces that never straddle an edge (k-contiguous operand: K % 4 == 0;
    // row-contiguous operand: its row count % 4 == 0); otherwise the all-dword variant
    auto al = [](const float* p, int ld, long s0, long s1, int extent) {
      return ((uintptr_t)p % 16 == 0) && ld % 4 == 0 && s0 % 4 == 0 && s1 % 4 == 0 && extent % 4 == 0;
    };
    const int a_extent = ta ? g.M : g.K;
    const bool vec = al(g.A, g.lda, g.sA0, g.sA1, g.a_padded && g.lda >= ((a_extent + 3) & ~3) ? 4 : a_extent) && al(g.B, g.ldb, g.sB0, g.sB1, tb ? g.K : g.N);
    // between one and two 128 x 128 workgroups per CU: 256 x 128 tiles (eight waves) make it one round
    const long t128 = (long)grid.x * grid.y * grid.z, t256 = (long)grid.x * ((g.M + 255) / 256) * grid.z;
    if (T == 128 && vec && t128 > want && t128 <= 2 * want && t256 <= want) {
      HVLA_BGEMM_CHOSE(256, 1, g.ksplit, 0);
      launch_bgemm3<256, 128, true>(st, ta, tb, g, dim3(grid.x, (g.M + 255) / 256, grid.z));
      return;
    }
    HVLA_BGEMM_CHOSE(T, vec ? 1 : 0, g.ksplit, 0);
    if (T == 128) { if (vec) launch_bgemm3<128, 128, true>(st, ta, tb, g, grid); else launch_bgemm3<128, 128, false>(st, ta, tb, g, grid); }
    else { if (vec) launch_bgemm3<64, 64, true>(st, ta, tb, g, grid); else launch_bgemm3<64, 64, false>(st, ta, tb, g, grid); }
    return;
  }
  HVLA_BGEMM_CHOSE(64, 0, g.ksplit, 1);
  if (!ta && !tb) hipLaunchKernelGGL((bgemm_kernel<false, false>), grid, dim3(256), 0, st, g);
  else if (!ta && tb) hipLaunchKernelGGL((bgemm_kernel<false, true>), grid, dim3(256), 0, st, g);
  else if (ta && !tb) hipLaunchKernelGGL((bgemm_kernel<true, false>), grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL((bgemm_kernel<true, true>), grid, dim3(256), 0, st, g);
}

// ------------------------------------------------------------------------------------------------
// The grouped form (train.h bgemm_groups): a layer-token model's weight generation reads another context row per
// run of theta columns, so each of its three products is a list of sub-products that differ in their operand origins.  A workgroup
// column takes the origins, the column origin and width and the K range from tiles[blockIdx.x]; everything after that is
// bgemm3_kernel's text -- the same staging, split, core and stores.  A kernel of its own and not a shared body: the existing
// instantiations keep their ISA (tests/test_isa_guards.py, tests/test_abi.py).  BM = BN in {64, 128}, four waves.
// ------------------------------------------------------------------------------------------------
template <bool TA, bool TB, int BM, int BN, bool VEC>
__global__ __launch_bounds__(256, 2) void bgemm3_groups_kernel(BG g, const BGTile* __restrict__ tiles) {
  constexpr int NTH = 256;
  constexpr int WM = BM / 2, WN = BN / 2, IM = WM / 32, IN = WN / 32;
  constexpr bool SA = TA, SB = !TB;
  constexpr int NA = SA ? 32 * (BM + 32) : BM * 32, NB = SB ? 32 * (BN + 32) : BN * 32;
  constexpr int NST = VEC ? 3 : 2;
  constexpr int PA = BM * 8 / NTH, PB = BN * 8 / NTH;
  constexpr int LPS = (PA + PB) * (VEC ? 1 : 4);
  __shared__ __attribute__((aligned(16))) __bf16 Ah[NA], Al[NA], Bh[NB], Bl[NB];
  const BGTile t = tiles[blockIdx.x];
  const int kbeg = t.k0, kend = t.k1 ? t.k1 : g.K, N = t.N;       // k1 == 0: the launch's whole K (the table does not depend on the batch)
  const float* A = g.A + t.a;
  const float* B = g.B + t.b;
  float* C = g.C + t.c;
  const int m0 = blockIdx.y * BM, n0 = t.n0 + blockIdx.z * BN;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave >> 1, wn = wave & 1, col = lane & 31, half = lane >> 5;
  f32x16 acc[IM][IN];
#pragma unroll
  for (int a = 0; a < IM; ++a)
#pragma unroll
    for (int b = 0; b < IN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  StageRegs<PA, VEC> ra[NST];
  StageRegs<PB, VEC> rb[NST];
#pragma unroll
  for (int s2 = 0; s2 < NST; ++s2) {
    stage_load<SA, BM, VEC, NTH>(A, g.lda, m0, g.M, kbeg + 32 * s2, kend, ra[s2]);
    stage_load<SB, BN, VEC, NTH>(B, g.ldb, n0, N, kbeg + 32 * s2, kend, rb[s2]);
  }
  for (int k0 = kbeg; k0 < kend; k0 += 32 * NST) {
#pragma unroll
    for (int s2 = 0; s2 < NST; ++s2) {
      const int kcur = k0 + 32 * s2;
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 1) * LPS) : "memory");
      tie(ra[s2]);
      tie(rb[s2]);
      stage_store<SA, BM, VEC, NTH>(Ah, Al, ra[s2]);
      stage_store<SB, BN, VEC, NTH>(Bh, Bl, rb[s2]);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      stage_load<SA, BM, VEC, NTH>(A, g.lda, m0, g.M, kcur + 32 * NST, kend, ra[s2]);
      stage_load<SB, BN, VEC, NTH>(B, g.ldb, n0, N, kcur + 32 * NST, kend, rb[s2]);
#pragma unroll
      for (int kk = 0; kk < 32; kk += 16) {
        Split8 fa[IM], fb[IN];
#pragma unroll
        for (int a = 0; a < IM; ++a) fa[a] = load_frag<SA, BM>(Ah, Al, wm * WM + a * 32, kk, lane);
#pragma unroll
        for (int b = 0; b < IN; ++b) fb[b] = load_frag<SB, BN>(Bh, Bl, wn * WN + b * 32, kk, lane);
#pragma unroll
        for (int a = 0; a < IM; ++a)
#pragma unroll
          for (int b = 0; b < IN; ++b) acc[a][b] = mma32_x3(fa[a], fb[b], acc[a][b]);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const float* bias = g.bias ? g.bias + t.bias : nullptr;
  auto store = [&](auto fullc, auto modec) {
    constexpr bool FULL = decltype(fullc)::value;
    constexpr int MODE = decltype(modec)::value;    // 0 store, 1 read-modify-write, 2 atomic add
#pragma unroll
    for (int b = 0; b < IN; ++b) {
      const int n = n0 + wn * WN + b * 32 + col;
      if (!FULL && n >= N) continue;
      const float bn = bias ? bias[n] : 0.f;
#pragma unroll
      for (int a = 0; a < IM; ++a) {
        float old[16];
        if constexpr (MODE == 1) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * WM + a * 32 + crow(r, half);
            old[r] = (FULL || m < g.M) ? C[(long)m * g.ldc + n] : 0.f;
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * WM + a * 32 + crow(r, half);
          if (!FULL && m >= g.M) continue;
          const float v = g.alpha * acc[a][b][r] + bn;
          float* c = C + (long)m * g.ldc + n;
          if constexpr (MODE == 2) unsafeAtomicAdd(c, v);
          else if constexpr (MODE == 1) *c = old[r] + v;
          else *c = v;
        }
      }
    }
  };
  using Yes = std::integral_constant<bool, true>;
  using No = std::integral_constant<bool, false>;
  using M0 = std::integral_constant<int, 0>;
  using M1 = std::integral_constant<int, 1>;
  using M2 = std::integral_constant<int, 2>;
  const bool full = m0 + BM <= g.M && n0 + BN <= N;
  const int mode = g.accumulate;
  if (full) {
    if (mode == 2) store(Yes{}, M2{}); else if (mode == 1) store(Yes{}, M1{}); else store(Yes{}, M0{});
  } else {
    if (mode == 2) store(No{}, M2{}); else if (mode == 1) store(No{}, M1{}); else store(No{}, M0{});
  }
}

template <bool TA, bool TB>
static void launch_groups(hipStream_t st, const BG& g, const BGTile* tiles, dim3 grid, int tile, bool vec) {
  if (tile == 128) {
    if (vec) hipLaunchKernelGGL((bgemm3_groups_kernel<TA, TB, 128, 128, true>), grid, dim3(256), 0, st, g, tiles);
    else hipLaunchKernelGGL((bgemm3_groups_kernel<TA, TB, 128, 128, false>), grid, dim3(256), 0, st, g, tiles);
  } else {
    if (vec) hipLaunchKernelGGL((bgemm3_groups_kernel<TA, TB, 64, 64, true>), grid, dim3(256), 0, st, g, tiles);
    else hipLaunchKernelGGL((bgemm3_groups_kernel<TA, TB, 64, 64, false>), grid, dim3(256), 0, st, g, tiles);
  }
}
// the three products of the weight generation: (ta, tb) = (0, 0) forward, (1, 0) dW_h, (0, 1) dctx
static void bgemm_groups_launch(hipStream_t st, bool ta, bool tb, const BG& g, const BGTile* tiles, int ntiles, int tile, int nz, bool vec_ok) {
  if (ntiles <= 0 || g.M <= 0) return;
  const dim3 grid(ntiles, (g.M + tile - 1) / tile, nz);
  const bool vec = vec_ok && g.lda % 4 == 0 && g.ldb % 4 == 0 && ((uintptr_t)g.A | (uintptr_t)g.B) % 16 == 0 && (!ta || g.M % 4 == 0);
  if (!ta && !tb) launch_groups<false, false>(st, g, tiles, grid, tile, vec);
  else if (ta && !tb) launch_groups<true, false>(st, g, tiles, grid, tile, vec);
  else launch_groups<false, true>(st, g, tiles, grid, tile, vec);
}
void bgemm_groups(hipStream_t st, bool ta, bool tb, BG g, const BGTile* tiles, int ntiles, int tile, int nz, bool vec_ok, double flops) {
  GemmTimer* tp = g_gemm_timers_on ? gemm_timer_here() : nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (!tp || !tp->on || hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { bgemm_groups_launch(st, ta, tb, g, tiles, ntiles, tile, nz, vec_ok); return; }
  GemmTimer& t = *tp;
  if (t.used == t.a.size()) {
    hipEvent_t x, y;
    if (hipEventCreate(&x) != hipSuccess) { bgemm_groups_launch(st, ta, tb, g, tiles, ntiles, tile, nz, vec_ok); return; }
    if (hipEventCreate(&y) != hipSuccess) { (void)hipEventDestroy(x); bgemm_groups_launch(st, ta, tb, g, tiles, ntiles, tile, nz, vec_ok); return; }
    t.a.push_back(x), t.b.push_back(y);
  }
  (void)hipEventRecord(t.a[t.used], st);
  bgemm_groups_launch(st, ta, tb, g, tiles, ntiles, tile, nz, vec_ok);
  (void)hipEventRecord(t.b[t.used], st);
  ++t.used;
  t.flops += flops;
}

}  // namespace hvla
