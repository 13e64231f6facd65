// weightgen_body.inc -- the body of weightgen_kernel (hypernet.hip), included twice: by weightgen_kernel itself
// (HVLA_WEIGHTGEN_SLOTS 0) and by weightgen_slots_kernel (HVLA_WEIGHTGEN_SLOTS 1), the episode-pool form, which stores the
// generated row of input episode r at arena row slot[r] (entries outside [0, rows) store nothing); input rows, staging and
// arithmetic are the same.  With HVLA_WEIGHTGEN_SLOTS 0 the compiler sees the kernel's text as it was before the pool existed
// (DESIGN.md §10).
  constexpr int CH = 2 * KS;                       // 16-byte chunks per ctx row (C = 16 KS bf16)
  constexpr int IPW = KS / 2 > 0 ? KS / 2 : 1;     // DMA instructions per wave and episode tile (2 planes x 32 rows x CH chunks / 64 lanes / 4 waves)
  __shared__ __attribute__((aligned(16))) __bf16 stage[2][32][128];
  __shared__ __attribute__((aligned(16))) __bf16 cbuf[2][2][32 * KS * 16];      // [buffer][hi / lo][row][chunk ^ row][8]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int wg = blockIdx.x;
  const bool active = wg * 4 + wave < p.ntiles;      // a ragged last workgroup: its spare waves still stage and go to the barriers
  const int tile = active ? wg * 4 + wave : p.ntiles - 1;
  const bool via_lds = wg * 4 + 3 < p.ntiles && (wg * 4 + 4) * 32 <= p.Gm;     // workgroup-uniform
  const int col = lane & 31, half = lane >> 5;
  const uint32_t lds_c = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)&cbuf[0][0][0];
  auto stage_ctx = [&](int b0, int buf) {
#pragma unroll
    for (int u = 0; u < IPW; ++u) {
      const int j = wave * IPW + u;                  // instruction of the tile: plane j / KS, 1 KB piece j % KS
      if (KS < 2 && j >= 2 * KS) break;
      const int plane = j / KS, piece = j % KS;
      const int pos = piece * 64 + lane;             // 16-byte position inside the plane's tile
      const int r = pos / CH, c = pos % CH;
      int b = b0 + r;
      b = b < p.B ? b : p.B - 1;
      const __bf16* src = (plane ? p.ctx_lo : p.ctx_hi) + (size_t)b * (KS * 16) + ((c ^ (r & (CH - 1))) * 8);
      const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_c + (uint32_t)(((buf * 2 + plane) * 32 * KS * 16) * 2 + piece * 1024));
      uint32_t keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(src), "s"(dst));
    }
  };
  stage_ctx(0, 0);
  bf16x8 ah[KS], al[KS];
  {
    const bf16x8* Ah = reinterpret_cast<const bf16x8*>(p.wcat_hi) + ((size_t)tile * KS) * 64 + lane;
    const bf16x8* Al = reinterpret_cast<const bf16x8*>(p.wcat_lo) + ((size_t)tile * KS) * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      ah[ks] = __builtin_nontemporal_load(Ah + ks * 64);
      al[ks] = __builtin_nontemporal_load(Al + ks * 64);
    }
  }
  // this lane's 16 consecutive packed positions and their bias
  const int pos0 = tile * 32 + half * 16;
  float bias[16];
#pragma unroll
  for (int r = 0; r < 16; r += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p.bcat + pos0 + r);
    bias[r] = v[0], bias[r + 1] = v[1], bias[r + 2] = v[2], bias[r + 3] = v[3];
  }
  int it = 0;
  for (int b0 = 0; b0 < p.B; b0 += 32, ++it) {
    const int b = b0 + col;
    const bool more = b0 + 32 < p.B;
    // the other buffer was last read two barriers ago (every iteration has at least one behind its MFMAs)
    if (more) {
      stage_ctx(b0 + 32, (it + 1) & 1);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPW) : "memory");     // this tile has landed (the A fragments and the last stores are older still)
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();                               // ... for every wave's share of it
    const __bf16* ch = &cbuf[it & 1][0][0] + col * (KS * 16);
    const __bf16* cl = &cbuf[it & 1][1][0] + col * (KS * 16);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = bias[r];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int sw = ((ks * 2 + half) ^ (col & (CH - 1))) * 8;
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(ch + sw), bl = *reinterpret_cast<const bf16x8*>(cl + sw);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[ks], bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ks], bl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ks], bh, acc, 0, 0, 0);
    }
    if (via_lds) {
      bf16x8 h0, h1, l0, l1;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        __bf16 hi, lo;
        split1(acc[j], hi, lo);
        h0[j] = hi, l0[j] = lo;
        split1(acc[8 + j], hi, lo);
        h1[j] = hi, l1[j] = lo;
      }
      __syncthreads();                           // the previous episode tile's rows have been read
      // A row is 256 B = twice the 32 write banks, and the eight lanes of a ds_write_b128 group hold eight consecutive rows at ONE
      // position: eight-way conflicts on every write (65 % of this kernel's LDS cycles, profiles/r3_pmc_sq_by_kernel.csv).  The
      // 16-byte chunk index is XORed with the row, here and where the rows are read back: both sides are conflict-free.
      const int c0 = wave * 4 + half * 2, sx = col & 15;
      *reinterpret_cast<bf16x8*>(&stage[0][col][((c0 + 0) ^ sx) * 8]) = h0;
      *reinterpret_cast<bf16x8*>(&stage[0][col][((c0 + 1) ^ sx) * 8]) = h1;
      *reinterpret_cast<bf16x8*>(&stage[1][col][((c0 + 0) ^ sx) * 8]) = l0;
      *reinterpret_cast<bf16x8*>(&stage[1][col][((c0 + 1) ^ sx) * 8]) = l1;
      __syncthreads();
      const size_t gpos = (size_t)wg * 128 + (lane & 15) * 8;          // 16 lanes x 16 B = one episode's 256-byte run
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int row = wave * 8 + u * 4 + (lane >> 4);
#if HVLA_WEIGHTGEN_SLOTS
        const int orow = b0 + row < p.B ? slot[b0 + row] : -1;     // arena row of this episode
        if (b0 + row < p.B && orow >= 0 && orow < rows) {
#define HVLA_OROW orow
#else
        if (b0 + row < p.B) {
#define HVLA_OROW (b0 + row)
#endif
          const bf16x8 vh = *reinterpret_cast<const bf16x8*>(&stage[0][row][((lane & 15) ^ (row & 15)) * 8]);
          const bf16x8 vl = *reinterpret_cast<const bf16x8*>(&stage[1][row][((lane & 15) ^ (row & 15)) * 8]);
          *reinterpret_cast<bf16x8*>(p.wh + (size_t)HVLA_OROW * p.Gm + gpos) = vh;
          *reinterpret_cast<bf16x8*>(p.wl + (size_t)HVLA_OROW * p.Gm + gpos) = vl;
        }
#undef HVLA_OROW
      }
    } else {
#if HVLA_WEIGHTGEN_SLOTS
      const int ob = b < p.B ? slot[b] : -1;      // arena row of this lane's episode
      if (active && b < p.B && ob >= 0 && ob < rows) {
#define HVLA_OB ob
#else
      if (active && b < p.B) {
#define HVLA_OB b
#endif
        if (pos0 < p.Gm) {
          bf16x8 h0, h1, l0, l1;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            __bf16 hi, lo;
            split1(acc[j], hi, lo);
            h0[j] = hi, l0[j] = lo;
            split1(acc[8 + j], hi, lo);
            h1[j] = hi, l1[j] = lo;
          }
          bf16x8* dh = reinterpret_cast<bf16x8*>(p.wh + (size_t)HVLA_OB * p.Gm + pos0);
          bf16x8* dl = reinterpret_cast<bf16x8*>(p.wl + (size_t)HVLA_OB * p.Gm + pos0);
          dh[0] = h0, dh[1] = h1, dl[0] = l0, dl[1] = l1;
        } else {
          f32x4* dv = reinterpret_cast<f32x4*>(p.vf + (size_t)HVLA_OB * p.Gv + (pos0 - p.Gm));
#pragma unroll
          for (int r = 0; r < 16; r += 4) dv[r >> 2] = f32x4{acc[r], acc[r + 1], acc[r + 2], acc[r + 3]};
        }
      }
      __syncthreads();                             // (the via_lds form has its two: here one, so that nobody stages over a tile still being read)
    }
  }
#undef HVLA_OB
