// policy_body.inc -- the body of the eight policy kernels (policy.hip), included once by each: by policy_kernel itself (HVLA_POLICY_SLOTS
// 0) and by policy_kernel_slots (HVLA_POLICY_SLOTS 1), the episode-pool form, where the workgroup of call row b reads its weights from arena
// row slots[b] (one wave-uniform load at entry; a row outside [0, p.B), the arena's rows, is skipped) and writes tokens / actions / logits /
// attention at call row b as always.  With HVLA_POLICY_SLOTS 0 the preprocessor hands the compiler the kernel's text as it was
// before the pool existed, so policy_kernel<8, 2> compiles to the same code (DESIGN.md §10).
// HVLA_POLICY_LANG 1 (policy_kernel_lang / policy_kernel_slots_lang, DESIGN.md §11): use_language_token.  The episode's language
// tokens lead the sequence; their K / V of every layer were written once per episode by lang_prefix_kernel (policy.hip) into the
// episode's arena row (LangLayout::m_lkv).  Patch queries and the action query attend over one more key tile, the prefix of the
// current layer and head pair, staged by LDS-DMA into `pre` at the q tile of the pair; its keys >= lang_T are masked.  Undefined = 0.
// HVLA_POLICY_BIAS 1 (policy_kernel_bias / policy_kernel_slots_bias, DESIGN.md §20): return_attention_map.  The mask of
// base_vit.py:209-214 is ADDED to the scores (multi_head_attetion.py:88-98), so a patch query has one more key, the action token's
// own k / v of the layer and head (ka / va: f32 in LDS, visible behind the barrier pair in front of the attention), one logit --
// log2 e in the kernel's log2 domain -- below the patch keys.  It is one VALU key per patch lane in both softmax passes; the action
// row (every key + 1: a constant the softmax row ignores) and the last layer (no patch rows) are untouched.  Undefined = 0.
// HVLA_POLICY_DIFF 1, with HVLA_POLICY_BIAS 1 (policy_kernel_diff / policy_kernel_slots_diff, DESIGN.md §22): use_differential_transformer.
// A head's 16 q / k features are two 8-feature parts; each part has its own softmax over all keys (the mask added as under BIAS, no
// 1 / sqrt(d)), the head's output is (A1 - lambda A2) V, RMS-normalised over its 16 values and scaled by subln's weight and
// 1 - lambda_init(l).  The K image holds part 0 on elements j < 4 and part 1 on j >= 4 of both lane halves (kphi), so a query fragment
// with the other part's elements zeroed gives the part's scores from the same MFMAs against the same K fragment: the two-pass softmax
// runs once per part (a rolled loop: the second copy of the unrolled key loops does not fit the register budget), the action row's
// partials and their combine likewise.  No q / k / v / out bias: their slots in the arena are padding, i.e. zeros.  Undefined = 0.
  extern __shared__ __attribute__((aligned(16))) char smem[];
#if HVLA_POLICY_DIFF
  constexpr int NDP = 2;                                               // softmaxes per head: rows of the partial table per head and wave
#else
  constexpr int NDP = 1;
#endif
#if HVLA_POLICY_LANG
  constexpr int SP = NW * 32, VLD = SP + 8, NHR = 2, NP = 10;          // NP: <= 8 waves + the language prefix + the own key
  constexpr int NPART = NW + 1, SPX = SP + 32;                         // partials before the own key; keys of the attention-map export
  constexpr bool lds_lang = true;                                      // the form of accept.h's policy_lds() this body is held to, below
  static_assert(NW + 2 <= NP, "partial table");
#else
  constexpr int SP = NW * 32, VLD = SP + 8, NHR = 2, NP = 9;           // NHR heads resident in LDS at a time; NP: partials per head (<= 8 waves + the own key)
  constexpr int NPART = NW, SPX = SP;
  constexpr bool lds_lang = false;
  static_assert(NW + 1 <= NP, "partial table");
#endif
  // the action token's scratch sits at the START of the dynamic LDS (compile-time addresses: every access is an immediate
  // offset from a lane term, instead of a loop-invariant address register per buffer that the allocator then spills)
  constexpr int ACT_FLOATS = 384 + 2 * NDP * NP * 20 + NW * 32 + 2 * SPX + 96 + NW * 64, ACT_BYTES = (ACT_FLOATS * 4 + 1023) & ~1023;
#if HVLA_POLICY_LANG
  constexpr bool SPREAD = false;               // (the language variant runs the action row's jobs one wave per tile: with act_rows64
                                               // it does not fit policy_kernel's register budget, DESIGN.md §11)
#else
  constexpr bool SPREAD = NW == 8;             // the action row's jobs over all eight waves (act_rows64); fewer waves: one wave per tile
#endif
  char* ring = smem + ACT_BYTES;                                       // [PRING][8 KiB] staged weight tiles
  // K of the resident heads: [head][key tile][d half][32 keys][8 d] -- inside a key tile the 16-byte piece of (key, half) sits at
  // lane position half * 32 + key, so a wave's write of its tile and every wave's ds_read_b128 of a tile are lane-linear 1 KiB
  // accesses.  ([key][16 d] rows of 32 B put keys c and c + 8 of a ds_read_b128 lane group on the same banks: two-way conflicts on
  // every K read of the two softmax passes, most of this kernel's 16 % SQ_LDS_BANK_CONFLICT of round 3.)
  __bf16* Kh = reinterpret_cast<__bf16*>(ring + PRING * 8192);         // [NHR][SP / 32][2][32][8]
  __bf16* Kl = Kh + NHR * SP * 16;
  _Float16* Vt = reinterpret_cast<_Float16*>(Kl + NHR * SP * 16);      // [NHR][hi d 0-15 | lo d 0-15][VLD] fp16
  const int b = blockIdx.x;
#if HVLA_POLICY_SLOTS
  {                                                                    // arena row of this episode's weights (wave-uniform)
    const int wrow = __builtin_amdgcn_readfirstlane(slots[b]);
    if (wrow < 0 || wrow >= p.B) return;                               // (p.B = the arena's rows; workgroup-uniform: before any barrier)
    const ptrdiff_t d = (ptrdiff_t)wrow - b;                           // the arena pointers move by (row - b) rows: from here on the
    p.wh += d * p.pl.Gm;                                               // body indexes them with b, as policy_kernel does
    p.wl += d * p.pl.Gm;
    p.vf += d * p.pl.Gv;
  }
#endif
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#if HVLA_POLICY_LANG
  char* pre = reinterpret_cast<char*>(Vt + NHR * 32 * VLD);           // [8 KiB] the resident head pair's language prefix:
                                                                       // [head][K hi 1 KiB | K lo 1 KiB | V^T 2 KiB] (lang_prefix_kernel)
  char* park = pre + LANG_PAIR_BYTES + wave * 4096;
#else
  char* park = reinterpret_cast<char*>(Vt + NHR * 32 * VLD) + wave * 4096;   // [NW][4 KiB]: phase A's attention outputs
#endif
  // The per-layer vectors of the episode (LayerNorm scale / bias, the four biases; then encoder_norm and the head bias:
  // Gv - v_layer0 floats, 12 KB at the README geometry) are copied to LDS once.  Read from global memory where they are
  // used, each of them -- one per staged tile -- made the compiler wait with vmcnt(0), i.e. for the weight tiles whose DMA
  // had just been issued as well: the three-tile prefetch was undone by a 64-byte bias load (tools/policy_timeline.py:
  // 4 us per tile step for 0.2 us of MFMAs).
#if HVLA_POLICY_LANG
  float* vlds = reinterpret_cast<float*>(pre + LANG_PAIR_BYTES + NW * 4096);
#else
  float* vlds = reinterpret_cast<float*>(reinterpret_cast<char*>(Vt + NHR * 32 * VLD) + NW * 4096);
#endif
  // accept.h's policy_lds() is what hvla_create and launch_policy_nw size this LDS by: the chain of pointers above is held to it.
  // (Taking every pointer as smem + its offset from that table instead changes the instruction streams of all twelve kernels:
  // profiles/policy_weightgen_template_isa.txt.)
  constexpr PolicyLds T = policy_lds(NW, lds_lang, NDP == 2);
  static_assert(T.nhr == NHR && T.np == NP && T.spx == SPX && T.act_floats == ACT_FLOATS && T.ring == ACT_BYTES, "accept.h: action scratch");
  static_assert(T.kh == T.ring + PRING * 8192 && T.kl == T.kh + NHR * SP * 16 * 2 && T.vt == T.kl + NHR * SP * 16 * 2 &&
                T.pre == T.vt + NHR * 32 * VLD * 2 && T.park == T.pre + (lds_lang ? LANG_PAIR_BYTES : 0) && T.vlds == T.park + NW * 4096,
                "accept.h: ring, K, V^T, prefix, park, vectors");
  const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
  const int P = NW * 32;
  const int token = wave * 32 + col;
  const PolicyLayout& L = p.pl;
  // ---- the action token's state (f32, natural feature order)
  float* xa = reinterpret_cast<float*>(smem);                          // [64] residual row
  float* h0 = xa + 64;                                                 // [64] LayerNorm_0 output (also the final norm)
  float* h1 = xa + 128;                                                // [64] LayerNorm_1 output
  float* qa = xa + 192, *ka = xa + 224, *va = xa + 256;                // [32] q (scaled), k, v of the resident head pair
  float* oa = xa + 288;                                                // [64] attention output, all four heads
  float* ga = xa + 352;                                                // [32] GELU(fc1) of the current hidden tile
  float* part = xa + 384;                                              // [2][NDP][NP][20]: per head (, part) and wave (max, sum, P.V[16])
  float* pbuf = part + 2 * NDP * NP * 20;                                   // [NW][32] wave-private: p in V^T column order
  float* pexp = pbuf + NW * 32;                                        // [2][SPX] p per key (attention-map export only; LANG: the prefix at SP)
  float* qkv1 = pexp + 2 * SPX;                                        // [96] q / k / v of head pair 1 (SPREAD: pair 0's are still being combined
                                                                       //      by one wave while every wave writes pair 1's)
  float* hpriv = qkv1 + 96 + wave * 64;                                // [NW][64] this wave's own LayerNorm output (SPREAD)
  const __bf16* __restrict__ wh = p.wh + (size_t)b * L.Gm;
  const __bf16* __restrict__ wl = p.wl + (size_t)b * L.Gm;
  const float* __restrict__ vf = p.vf + (size_t)b * L.Gv;
  const int E = p.E;
  const int nproj = 2 * (E / 64), TM = p.M / 32, ntiles = nproj + p.L * (8 + 2 * TM) + 1;
#if HVLA_POLICY_LANG
  // lang_T and the prefix's offset in the arena row (LangLayout::m_lkv: behind the head's four fragments) are held in VGPRs: this
  // variant's SGPRs are all taken (held to policy_kernel's budget of SGPRs parked in VGPR lanes, tests/test_abi.py)
  const int lang_Tv = opaque(lang_T);
  const int lkv0 = opaque(L.m_head + 4 * 512);
#endif

  // ---- the staging pipeline (see PRING above)
  const uint32_t lds_ring = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)ring;
#if HVLA_POLICY_SLOTS || HVLA_POLICY_LANG
  constexpr bool stream_nt = true;                                     // the pool and language forms stream their weights non-temporally at
                                                                       // every K: one SGPR fewer, which keeps them at policy_kernel's SGPR budget
#else
  const bool stream_nt = (int)gridDim.x >= 64;                         // (uniform) see dma()
#endif
  int ti = 0;                                                          // next tile to consume
  bool mine = false;                                                   // the tile just acquired is this wave's action-row job
  auto dma = [&](int i) {                        // fragment f of tile i is moved by wave f mod NW: one each at NW = 8
    if (i < ntiles) {
      const int off = policy_tile_offset(L, i, nproj, TM, E, p.L);
      for (int f = wave; f < 8; f += NW) {
        const __bf16* src = (f < 4 ? wh : wl) + off + (f & 3) * 512 + lane * 8;
        // issued by hand (guide 5.7: M0 saved, set, used and restored in one statement): the compiler must not know about
        // this LDS write, or it drains vmcnt to 0 in front of EVERY ds_read of the kernel (it cannot tell the ring from
        // K / V) and the tiles in flight are waited for at once.  The counted wait in acquire() orders it.
        const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_ring + (uint32_t)((i % PRING) * 8192 + f * 1024));
        uint32_t keep;
        // An episode's weights are read once, by this CU only: at a big batch (every CU streaming its own 806 KB) the
        // non-temporal form lands sooner (guide, "nt-weights": -2.8 % of the kernel at B = 256, same box); alone on the chip
        // the default policy is the faster one (B = 1: +1 % with nt), so the hint follows the batch size.
        if (stream_nt)
          asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                       : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
        else
          asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                       : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
      }
    }
  };
#if HVLA_POLICY_LANG
  // the language prefix of layer l, head pair ph (arena rows, LangLayout::m_lkv: head 0 in the hi plane, head 1 in the lo plane)
  // -> pre: issued right behind the q tile's barrier (every wave is done with the previous pair's prefix); the k and v tiles'
  // full fences land it before the attention reads it
  const uint32_t lds_pre = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)pre;
  auto dma_lang = [&](int l, int ph) {
    const int off = opaque(lkv0) + (2 * l + ph) * 2048;
    for (int f = wave; f < 8; f += NW) {
      const __bf16* src = (f < 4 ? wh : wl) + off + (f & 3) * 512 + lane * 8;
      const uint32_t dst = __builtin_amdgcn_readfirstlane(opaque((int)(lds_pre + (uint32_t)(f * 1024))));
      uint32_t keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    }
  };
#endif
  // tile `ti` has landed for every wave and every wave is done with tile ti - 1 (LDS reads and writes retired in front of
  // the barrier), whose slot then takes tile ti + PRING - 1.  With one DMA per wave and tile (NW = 8) a wave's DMA of tile
  // ti is older than its DMAs of tiles ti + 1 and ti + 2, so all but the two youngest vector-memory operations suffice
  // while those two exist (any other vector-memory operation in between only makes the wait stricter); the small test
  // geometries (several DMAs per wave) simply drain.
  // `younger8`: eight more vector-memory operations (the projection's prefetch of the next token values) were issued behind
  // the two youngest DMAs: they may stay in flight too.  With the plain vmcnt(2) they had to land at the very next tile, one
  // HBM round trip per pair of projection tiles (19 % of the kernel, tools/policy_timeline.py).
  auto acquire = [&](bool younger8 = false) -> const char* {
    if (NW == 8 && ti + PRING - 2 < ntiles) {
      if (younger8) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PRING - 2 + 8) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PRING - 2) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");              // nothing below may be placed in front of the s_barrier (see the barrier in the layer loop)
    __builtin_amdgcn_sched_barrier(0);
    // A FULL fence behind every tile's barrier, written out: s_waitcnt vmcnt(0) lgkmcnt(0) + a second barrier -- every LDS-DMA of
    // every wave has landed and every LDS operation has retired before any wave touches the tile.  (Round 4 wrote __syncthreads()
    // here and called it this fence; on gfx950 that builtin emits lgkmcnt(0) + s_barrier and NO vmcnt -- the advisor read the ISA --
    // so round 4's remedy was one more barrier, a schedule perturbation like round 3's.  tools/kernel_resources.sh now greps the
    // ISA for the wait.)  The counted wait above is sufficient by the ISA's rules and by tools/lds_dma_visibility_probe.hip (0
    // stale words of 3.3e10); this is the one remedy for round 3's one-wave race that is an ORDERING and not a schedule
    // perturbation (profiles/r4_race_root_cause.txt).  It drains the two prefetched tiles at every tile step: + 4 % of the kernel
    // (0.2190 -> 0.2278 ms per 256 episodes, 0.1987 -> 0.2060 at B = 1, same box, round 5: profiles/r5_policy_fence_ab.txt;
    // the second barrier alone was + 0.5 %).
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    dma(ti + PRING - 1);
    const char* slot = ring + (ti % PRING) * 8192;
    mine = (ti % NW) == wave;
    ++ti;
    return slot;
  };
  for (int i = threadIdx.x * 4; i < L.Gv - L.v_layer0; i += NW * 64 * 4)        // (v_layer0 and Gv are multiples of 4)
    *reinterpret_cast<f32x4*>(vlds + i) = *reinterpret_cast<const f32x4*>(vf + L.v_layer0 + i);
  if (threadIdx.x < 64)                                                // action token: zeros + its position row (base_vit.py:182-204)
    xa[threadIdx.x] = vf[L.v_pos + P * 64 + (threadIdx.x >> 5) * 32 + cidx(threadIdx.x & 31)];
  const float* vtail = vlds - L.v_layer0;                              // vtail + v_xxx = the LDS copy of vf + v_xxx for v_xxx >= v_layer0
  f32x16 x[2];
  // the residual starts as the projection bias: loaded and WAITED FOR before the first DMA goes out (a compiler-placed wait
  // for these loads at the first MFMA would be a vmcnt(0) that drains the weight tiles in flight)
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float bv[16];
    ldv16(vf + L.v_proj_bias + (t * 2 + half) * 16, bv);
#pragma unroll
    for (int r = 0; r < 16; ++r) x[t][r] = bv[r];
  }
  asm volatile("" : "+v"(x[0]), "+v"(x[1]));
#pragma unroll
  for (int i = 0; i < PRING - 1; ++i) dma(i);
#if defined(HVLA_BENCH_HOOKS)
  int nstamp = 0;
#define HVLA_STAMP() do { if (p.stamps && blockIdx.x == 0 && threadIdx.x == 0) p.stamps[nstamp] = __builtin_readcyclecounter(); ++nstamp; } while (0)
#else
#define HVLA_STAMP() do { } while (0)
#endif
  HVLA_STAMP();                                 // 0: start

  // ---------------- image_embedding_projection (base_vit.py:130-133) + pos-emb (:182-204)
  {
    const float* tp = p.tokens + ((size_t)b * P + token) * E + 16 * half;
    float tv[2][16];
    ldv16(tp, tv[0]);
    ldv16(tp + 32, tv[1]);
    for (int kk = 0; kk < E / 64; ++kk) {                   // four k-steps: two staged tiles (m-tile 0, 1)
      Split8 bf[4];
      bf[0] = split8(tv[0]); bf[1] = split8(tv[0] + 8); bf[2] = split8(tv[1]); bf[3] = split8(tv[1] + 8);
      // The next group's token values (8 loads per lane) stay in flight under BOTH tiles of this group: acquire(true)
      // leaves them outstanding.  (Issuing them by hand with counted waits of their own was tried and is unsafe: the
      // compiler copies the destination registers of an asm load at the loop's phi before any wait we can place.)
      const bool pre = kk + 1 < E / 64;
      if (pre) {
        ldv16(tp + 64 * (kk + 1), tv[0]);
        ldv16(tp + 64 * (kk + 1) + 32, tv[1]);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const char* slot = acquire(pre);
        x[t] = tile_mma<4, TIE>(slot, lane, bf, x[t]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float pe[16];
    ldv16(vf + L.v_pos + token * 64 + (t * 2 + half) * 16, pe);
#pragma unroll
    for (int r = 0; r < 16; ++r) x[t][r] += pe[r];
  }

  HVLA_STAMP();                                 // 1: projection done
#if HVLA_POLICY_DIFF
  const float qscale = 1.4426950408889634f;                   // exp -> exp2 alone: differential_transformer.py:215-216 does not scale the scores
#else
  const float qscale = rsqrtf(16.f) * 1.4426950408889634f;    // 1/sqrt(hd), and exp -> exp2
#endif
  const int slot_k = wave * 32 + col;                          // this lane's key slot in LDS
  const int vpos = (wave * 32) | vperm32(col);

  for (int l = 0; l < p.L; ++l) {
    const bool last = l == p.L - 1;
    const bool full = !last;                  // do the patch waves need their own rows?  (base_vit.py:226: only the action row is read)
    const float* vl = vtail + L.v_layer0 + l * L.v_layer_stride;    // LDS
    // the action row's attention over this wave's 32 keys for resident head hl: (max, sum, P.V) -> part[hl][wave]
    // (HVLA_POLICY_DIFF: for part c of the head, the features 8 c .. 8 c + 7 of q and k -> part[hl][c][wave])
    auto act_attend = [&](int hl, const float* qbase, int c = 0) {
      const int lane = opaque((int)(threadIdx.x & 63)), col = lane & 31, half = lane >> 5;
      const int slot_k = wave * 32 + col;
      const float* qv = qbase + hl * 16 + 4 * half;
      const f32x4 q0 = *reinterpret_cast<const f32x4*>(qv), q1 = *reinterpret_cast<const f32x4*>(qv + 8);
      const bf16x8 khi = *reinterpret_cast<const bf16x8*>(Kh + kpos(hl * SP + slot_k, half));
      const bf16x8 klo = *reinterpret_cast<const bf16x8*>(Kl + kpos(hl * SP + slot_k, half));
      float s = 0.f;
#if HVLA_POLICY_DIFF
      if (c == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf((float)khi[j] + (float)klo[j], q0[j], s);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf((float)khi[4 + j] + (float)klo[4 + j], q1[j], s);
      }
#else
      (void)c;
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf((float)khi[j] + (float)klo[j], q0[j], s);
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf((float)khi[4 + j] + (float)klo[4 + j], q1[j], s);
#endif
      s += __shfl_xor(s, 32, 64);               // both halves: the score of key `col` (log2 domain)
      const float m = wmax64(s);
      const float pj = __builtin_amdgcn_exp2f(s - m);
      const float ls = wsum64(half == 0 ? pj : 0.f);
      float* pb = pbuf + wave * 32;
      if (half == 0) pb[vperm32(col)] = pj;     // the order of the V^T image's columns
      if (p.amap && half == 0) pexp[hl * SPX + slot_k] = pj;
      const _Float16* vrow = Vt + (hl * 32 + col) * VLD + wave * 32 + 16 * half;      // row col: d (hi) or 16 + d (lo x 2^10)
      const f16x8 v0 = *reinterpret_cast<const f16x8*>(vrow), v1 = *reinterpret_cast<const f16x8*>(vrow + 8);
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4 pa = *reinterpret_cast<const f32x4*>(pb + 16 * half + 4 * i);
        const f32x4 pc = *reinterpret_cast<const f32x4*>(pb + 16 * half + 8 + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) a = fmaf((float)v0[4 * i + j], pa[j], a);
#pragma unroll
        for (int j = 0; j < 4; ++j) a = fmaf((float)v1[4 * i + j], pc[j], a);
      }
      a += __shfl_xor(a, 32, 64);
      const float od = fmaf(__shfl_xor(a, 16, 64), 1.f / 1024.f, a);     // lanes < 16: hi row d + lo row d
#if HVLA_POLICY_DIFF
      float* pp = part + ((hl * NDP + c) * NP + wave) * 20;
#else
      float* pp = part + (hl * NP + wave) * 20;
#endif
      if (lane == 0) pp[0] = m, pp[1] = ls;
      if (lane < 16) pp[2 + lane] = od;
    };
#if HVLA_POLICY_LANG
    // the same over the language prefix's 32 keys (keys >= lang_T masked) -> part[hl][NW]; one wave
    auto act_attend_lang = [&](int hl, const float* qbase) {
      const int lane = opaque((int)(threadIdx.x & 63)), col = lane & 31, half = lane >> 5;
      const float* qv = qbase + hl * 16 + 4 * half;
      const f32x4 q0 = *reinterpret_cast<const f32x4*>(qv), q1 = *reinterpret_cast<const f32x4*>(qv + 8);
      const char* ph_ = pre + hl * 4096;
      const bf16x8 khi = *reinterpret_cast<const bf16x8*>(ph_ + lane * 16);
      const bf16x8 klo = *reinterpret_cast<const bf16x8*>(ph_ + 1024 + lane * 16);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf((float)khi[j] + (float)klo[j], q0[j], s);
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf((float)khi[4 + j] + (float)klo[4 + j], q1[j], s);
      s += __shfl_xor(s, 32, 64);
      if (col >= opaque(lang_Tv)) s = -1e30f;            // padding of the 32-key tile (not T5 padding: that is attended, base_vit.py:207-212)
      const float m = wmax64(s);
      const float pj = __builtin_amdgcn_exp2f(s - m);
      const float ls = wsum64(half == 0 ? pj : 0.f);
      float* pb = pbuf + wave * 32;
      if (half == 0) pb[vperm32(col)] = pj;
      if (p.amap && half == 0) pexp[hl * SPX + SP + col] = pj;
      const _Float16* vrow = reinterpret_cast<const _Float16*>(ph_ + 2048) + col * 32 + 16 * half;
      const f16x8 v0 = *reinterpret_cast<const f16x8*>(vrow), v1 = *reinterpret_cast<const f16x8*>(vrow + 8);
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4 pa = *reinterpret_cast<const f32x4*>(pb + 16 * half + 4 * i);
        const f32x4 pc = *reinterpret_cast<const f32x4*>(pb + 16 * half + 8 + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) a = fmaf((float)v0[4 * i + j], pa[j], a);
#pragma unroll
        for (int j = 0; j < 4; ++j) a = fmaf((float)v1[4 * i + j], pc[j], a);
      }
      a += __shfl_xor(a, 32, 64);
      const float od = fmaf(__shfl_xor(a, 16, 64), 1.f / 1024.f, a);
      float* pp = part + (hl * NP + NW) * 20;
      if (lane == 0) pp[0] = m, pp[1] = ls;
      if (lane < 16) pp[2 + lane] = od;
    };
#endif
    // combine the partials of head pair `pair` (all waves' keys + the action token's own key, base_vit.py:209-214: the
    // action row sees every token) -> oa[(2 pair + hl) * 16 + d]; run by ONE wave, after the barrier that follows the
    // attention of that pair and before anything overwrites qa / ka / va
#if HVLA_POLICY_DIFF
    // ... per part (the action row's mask row is + 1 on every key, its own included: no offset), then (A1 - lambda A2) V, the RMSNorm
    // over the head's 16 values, subln's weight and 1 - lambda_init (differential_transformer.py:223-247)
    auto act_combine = [&](int pair) {
      const int lane = opaque((int)(threadIdx.x & 63));
      const float* qa = (SPREAD && pair) ? qkv1 : xa + 192;
      const float *ka = qa + 32, *va = qa + 64;
      float linit;
      const float lam = diff_lambda(vl + L.v_fc2_b + 64, l, lane, linit);
      const float wn = vl[L.v_fc2_b + 96 + (lane & 15)] * (1.f - linit);
#pragma unroll
      for (int hl = 0; hl < NHR; ++hl) {
        float od = 0.f;
#pragma unroll 1
        for (int c = 0; c < NDP; ++c) {       // (rolled: two copies of the combine do not fit the q tile's register budget)
          const float self = wsum64((lane < 16 && (lane >> 3) == c) ? qa[hl * 16 + lane] * ka[hl * 16 + lane] : 0.f);
          const float* pt = part + (hl * NDP + c) * NP * 20;
          const float mt = lane < NPART ? pt[lane * 20] : (lane == NPART ? self : -1e30f);
          const float lt = lane < NPART ? pt[lane * 20 + 1] : (lane == NPART ? 1.f : 0.f);
          const float M = wmax64(mt);
          const float f = __builtin_amdgcn_exp2f(mt - M);
          const float inv = 1.f / wsum64(f * lt);
          float o = 0.f;
#pragma unroll
          for (int t = 0; t < NPART; ++t) o = fmaf(__shfl(f, t, 64), pt[t * 20 + 2 + (lane & 15)], o);
          o = fmaf(__shfl(f, NPART, 64), va[hl * 16 + (lane & 15)], o) * inv;
          od = c ? fmaf(-lam, o, od) : o;
        }
        const float r = rsqrtf(wsum64(lane < 16 ? od * od : 0.f) * (1.f / 16.f) + 1e-5f);
        if (lane < 16) oa[(2 * pair + hl) * 16 + lane] = od * r * wn;
      }
    };
#else
    auto act_combine = [&](int pair) {
      const int lane = opaque((int)(threadIdx.x & 63));
      const float* qa = (SPREAD && pair) ? qkv1 : xa + 192;            // [q 32 | k 32 | v 32] of this head pair
      const float *ka = qa + 32, *va = qa + 64;
#pragma unroll
      for (int hl = 0; hl < NHR; ++hl) {
        const float self = wsum64(lane < 16 ? qa[hl * 16 + lane] * ka[hl * 16 + lane] : 0.f);
        const float* pt = part + hl * NP * 20;
        const float mt = lane < NPART ? pt[lane * 20] : (lane == NPART ? self : -1e30f);
        const float lt = lane < NPART ? pt[lane * 20 + 1] : (lane == NPART ? 1.f : 0.f);
        const float M = wmax64(mt);
        const float f = __builtin_amdgcn_exp2f(mt - M);
        const float inv = 1.f / wsum64(f * lt);
        float od = 0.f;
#pragma unroll
        for (int t = 0; t < NPART; ++t) od = fmaf(__shfl(f, t, 64), pt[t * 20 + 2 + (lane & 15)], od);
        od = fmaf(__shfl(f, NPART, 64), va[hl * 16 + (lane & 15)], od);
        if (lane < 16) oa[(2 * pair + hl) * 16 + lane] = od * inv;
        if (p.amap) {                           // attention_weights[0][0, head, -1, :-1] (hypervla_interface.py:213-215)
          constexpr int HEADS = 2 * NHR;      // the kernel is specialised for 64 features = 4 heads of 16 (hvla_create refuses anything else):
#if HVLA_POLICY_LANG
          // [B, L, heads, lang_T + P]: the language keys first (the reference's sequence order).  Key j of pexp: patch j < SP, or
          // language key j - SP (partial NW = j >> 5 as well)
          const int lT = opaque(lang_Tv);
          float* am = p.amap + (((size_t)b * p.L + l) * HEADS + 2 * pair + hl) * (P + lT);
          for (int j = lane; j < SPX; j += 64) {
            const float v = pexp[hl * SPX + j] * __shfl(f, j >> 5, 64) * inv;
            if (j < SP) am[lT + j] = v;
            else if (j - SP < lT) am[j - SP] = v;
          }
#else
          float* am = p.amap + (((size_t)b * p.L + l) * HEADS + 2 * pair + hl) * P;   // the caller's [B, L, heads, P] buffer
          for (int j = lane; j < SP; j += 64) am[j] = pexp[hl * SP + j] * __shfl(f, j >> 5, 64) * inv;
#endif
        }
      }
    };
#endif
    Split8 of[2];                             // attention outputs of the resident head pair as out-projection B fragments
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {          // heads 2 ph, 2 ph + 1 resident
      Split8 qf[2];
      {
        Split8 hb[4];
        // x is not touched before both phases are done; the LayerNorm is redone per phase ON PURPOSE (the empty asm keeps
        // the compiler from sharing it: its 32 registers would otherwise stay live across the first phase's attention)
        asm volatile("" : "+v"(x[0]), "+v"(x[1]));
        ln_frags(x, vl + L.v_ln0_s, vl + L.v_ln0_b, half, hb);
#pragma unroll
        for (int k = 0; k < 3; ++k) {         // q, k, v tile of this head pair
          const int t = 2 * k + ph;
          const char* slot = acquire();
#if HVLA_POLICY_LANG
          if (k == 0) dma_lang(l, ph);
#endif
          if constexpr (SPREAD) {             // the action row through this tile: four of its 32 outputs per wave
            const int lane = opaque((int)(threadIdx.x & 63));
            if (k == 0) {
              if (ph == 0) act_ln_private(xa, vl + L.v_ln0_s, vl + L.v_ln0_b, hpriv, lane);
              else if (mine) act_combine(0);  // pair 0's partials were completed before this tile's barrier; its q / k / v stay in qa
            }
            const int rho = 4 * wave + ((lane >> 3) & 3);
            float y = act_rows64(slot, lane, wave, hpriv) + vl[L.v_qkv_b + t * 32 + cidx(rho)];
            if (k == 0) y *= qscale;
            if ((lane & 39) == 0) ((ph ? qkv1 : qa) + k * 32)[rho] = y;      // one lane per row (piece 0 of the hi plane)
          } else if (mine) {                  // fewer than eight waves: one wave per tile
            const int lane = opaque((int)(threadIdx.x & 63)), col = lane & 31, half = lane >> 5;
            if (k == 0) {
              if (ph == 0) act_ln(xa, vl + L.v_ln0_s, vl + L.v_ln0_b, h0, lane);
              else act_combine(0);            // pair 0's partials were completed before this tile's barrier
            }
            float y = act_matvec64(slot, lane, h0) + vl[L.v_qkv_b + t * 32 + cidx(col)];
            if (k == 0) y *= qscale;
            if (half == 0) (k == 0 ? qa : (k == 1 ? ka : va))[col] = y;
          }
          if (k == 0 && !full) continue;
          f32x16 a;
          {
            float bv[16];
            ldv16(vl + L.v_qkv_b + (t * 2 + half) * 16, bv);
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = bv[r];
          }
          a = tile_mma<4, TIE>(slot, lane, hb, a);
          if (k == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] *= qscale;
            qf[0] = acc_frag<0>(a);
            qf[1] = acc_frag<1>(a);
          } else if (k == 1) {
            const Split8 k0 = acc_frag<0>(a), k1 = acc_frag<1>(a);
            *reinterpret_cast<bf16x8*>(Kh + kpos(0 * SP + slot_k, half)) = k0.hi;
            *reinterpret_cast<bf16x8*>(Kl + kpos(0 * SP + slot_k, half)) = k0.lo;
            *reinterpret_cast<bf16x8*>(Kh + kpos(1 * SP + slot_k, half)) = k1.hi;
            *reinterpret_cast<bf16x8*>(Kl + kpos(1 * SP + slot_k, half)) = k1.lo;
          } else {
            // row d = crow(j, half) = 8 (j >> 2) + (j & 3) + 4 half of head r >> 3: ONE per-lane base (half, key position) and
            // compile-time offsets (32 separately computed addresses get hoisted out of the layer loop and spilled)
            _Float16* vb = Vt + (4 * half) * VLD + vpos;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = (r >> 3) * 32 + 8 * ((r & 7) >> 2) + (r & 3);
              const _Float16 hi = (_Float16)a[r], lo = (_Float16)((a[r] - (float)hi) * 1024.f);   // lo x 2^10: out of fp16's subnormal range
              vb[row * VLD] = hi;
              vb[(row + 16) * VLD] = lo;
            }
          }
        }
      }
      // K / V of this head pair (and the action row's q / k / v) become visible to every wave at the next barrier.  That
      // barrier is the next tile's acquire, which comes before the attention only if we take it now: tile "out" of this phase
      // is consumed after both phases, so synchronise here explicitly.
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_barrier();             // see below: 8 more barriers per launch, nothing measurable
      // Run-to-run determinism (tools/policy_determinism_probe.py, tools/policy_race_locator.py; profiles/r3_policy_race.txt).
      // With the time stamps of the bench flavour compiled in, 3-10 % of the launches of this kernel gave slightly different
      // actions again (round 1's symptom): ONE wave's K of the first head pair of layer 0 off by ~1e-2 relative, every
      // other wave's bits unchanged -- not late weight DMA (waiting for all of it with vmcnt(0) did not help), not a
      // missing LDS wait the compiler could see (a block-by-block check of the ISA finds none).  What removes it, each on
      // its own, 0 of 40 000 episode-runs: the MFMA's A operands (weight / K / V fragments out of LDS) passed through an
      // empty asm (TIE = 2, round 1's remedy), a second s_barrier here, or a different job rotation.  A compiler barrier
      // behind the s_barrier (the builtin is "no memory, side effects only": nothing else keeps the loads of the code
      // below behind it) halves the rate but does not remove it.  The product carries all three: TIE = 2, the second
      // barrier, the compiler barrier.
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      HVLA_STAMP();                             // 2 + 6 l + 2 ph: q / k / v of the head pair done
#if HVLA_POLICY_DIFF
#pragma unroll
      for (int hl = 0; hl < NHR; ++hl) {
        act_attend(hl, (SPREAD && ph) ? qkv1 : qa, 0);
        act_attend(hl, (SPREAD && ph) ? qkv1 : qa, 1);
      }
#else
#pragma unroll
      for (int hl = 0; hl < NHR; ++hl) act_attend(hl, (SPREAD && ph) ? qkv1 : qa);
#endif
#if HVLA_POLICY_LANG
      if (wave == NW - 1) {                   // the action row over the language prefix: one more partial
#pragma unroll
        for (int hl = 0; hl < NHR; ++hl) act_attend_lang(hl, (SPREAD && ph) ? qkv1 : qa);
      }
#endif
      if (full) {
#pragma unroll
        for (int hl = 0; hl < NHR; ++hl) {
          __builtin_amdgcn_sched_barrier(0);
#if HVLA_POLICY_DIFF
          // part c of the head: the query with the other part's elements zeroed, its own softmax; ovd = A1 V - lambda A2 V
          float linit;
          const float lam = diff_lambda(vl + L.v_fc2_b + 64, l, opaque((int)(threadIdx.x & 63)), linit);
          float ovd[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) ovd[j] = 0.f;
#pragma unroll 1
          for (int c = 0; c < NDP; ++c) {
          const Split8 qsel = diff_part(qf[hl], c);
#else
          {
          const Split8& qsel = qf[hl];
#endif
          auto scores = [&](int kt, float init) {      // S^T tile: keys on the accumulator rows, this lane's query on the lane
            Split8 kf;
            kf.hi = *reinterpret_cast<const bf16x8*>(Kh + kpos(hl * SP + kt * 32 + col, half));
            kf.lo = *reinterpret_cast<const bf16x8*>(Kl + kpos(hl * SP + kt * 32 + col, half));
            f32x16 sc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] = init;
            return mma32_x3p<TIE>(kf, qsel, sc);
          };
#if HVLA_POLICY_LANG
          auto lscores = [&](float init) {             // the language prefix tile, keys >= lang_T masked
            const int ln = opaque((int)(threadIdx.x & 63));
            Split8 kf;
            kf.hi = *reinterpret_cast<const bf16x8*>(pre + hl * 4096 + ln * 16);
            kf.lo = *reinterpret_cast<const bf16x8*>(pre + hl * 4096 + 1024 + ln * 16);
            f32x16 sc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] = init;
            sc = mma32_x3p<TIE>(kf, qf[hl], sc);
            // key crow(r, half) >= lang_T is padding of the tile.  The limit goes through an empty asm here: sixteen compares against
            // a loop-invariant value would otherwise be hoisted out of the layer loop as sixteen lane masks (SGPR pairs) kept live
            const int lim = opaque(lang_Tv) - 4 * (ln >> 5);
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if ((r & 3) + 8 * (r >> 2) >= lim) sc[r] = -1e30f;
            return sc;
          };
#endif
          // pass 1: row maximum (scores are in the log2 domain: q carries 1/sqrt(hd) log2 e).  Patches cannot see the
          // action token (base_vit.py:209-214): structural, its key is in no tile.  (HVLA_POLICY_BIAS: they do, below.)
          float m2 = -1e30f;
#if HVLA_POLICY_LANG
          // (rolled in this variant: unrolled, the lane's addresses of the eight key tiles are hoisted out of the layer loop into
          // registers it does not have, DESIGN.md §11)
#pragma unroll 1
#endif
          for (int kt = 0; kt < NW; ++kt) {
            const f32x16 sc = scores(kt, 0.f);
#pragma unroll
            for (int r = 0; r < 16; ++r) m2 = fmaxf(m2, sc[r]);
          }
#if HVLA_POLICY_LANG
          {
            const f32x16 sc = lscores(0.f);
#pragma unroll
            for (int r = 0; r < 16; ++r) m2 = fmaxf(m2, sc[r]);
          }
#endif
          m2 = fmaxf(m2, __shfl_xor(m2, 32, 64));
#if HVLA_POLICY_BIAS
          // the action token's key: this lane's 8 of the query's 16 values (the B fragment's hi + lo, the order of act_attend's
          // q0 / q1) against ka in f32, the other 8 from lane ^ 32; the mask's 0 against the patch keys' 1 is - log2 e here
          float sa;
          {
            const int ln = opaque((int)(threadIdx.x & 63));
            const float* kv = ((SPREAD && ph) ? qkv1 : qa) + 32 + hl * 16 + 4 * (ln >> 5);
            const f32x4 k0 = *reinterpret_cast<const f32x4*>(kv), k1 = *reinterpret_cast<const f32x4*>(kv + 8);
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) s = fmaf((float)qsel.hi[j] + (float)qsel.lo[j], k0[j], s);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = fmaf((float)qsel.hi[4 + j] + (float)qsel.lo[4 + j], k1[j], s);
            sa = s + __shfl_xor(s, 32, 64) - 1.4426950408889634f;
          }
          m2 = fmaxf(m2, sa);
#endif
          // pass 2: p = exp2(s - max) straight out of the accumulator (initialised to -max); P = hi + lo in fp16 against
          // V = [hi | lo x 2^10] in fp16: four MFMAs per key tile, all four hi / lo cross terms
          float lsum = 0.f;
          f32x16 O;
#pragma unroll
          for (int r = 0; r < 16; ++r) O[r] = 0.f;
#if HVLA_POLICY_LANG
#pragma unroll 1
#endif
          for (int kt = 0; kt < NW; ++kt) {
            const f32x16 sc = scores(kt, -m2);
            const _Float16* vp = Vt + (hl * 32 + col) * VLD + kt * 32 + half * 8;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {               // one k-step (16 keys) at a time: bounds the live exponentials
              f16x8 phi, plo;
#pragma unroll
              for (int r = 0; r < 8; ++r) {
                const float e = __builtin_amdgcn_exp2f(sc[8 * ks + r]);
                lsum += e;
                phi[r] = (_Float16)e;
                plo[r] = (_Float16)(e - (float)phi[r]);
              }
              f16x8 v = *reinterpret_cast<const f16x8*>(vp + 16 * ks);
              if constexpr (TIE == 1 || TIE == 2) asm volatile("" : "+v"(v));
              O = __builtin_amdgcn_mfma_f32_32x32x16_f16(v, plo, O, 0, 0, 0);
              O = __builtin_amdgcn_mfma_f32_32x32x16_f16(v, phi, O, 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
#if HVLA_POLICY_LANG
          {
            const f32x16 sc = lscores(-m2);
            const int ln = opaque((int)(threadIdx.x & 63));
            const _Float16* vp = reinterpret_cast<const _Float16*>(pre + hl * 4096 + 2048) + (ln & 31) * 32 + (ln >> 5) * 8;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              f16x8 phi, plo;
#pragma unroll
              for (int r = 0; r < 8; ++r) {
                const float e = __builtin_amdgcn_exp2f(sc[8 * ks + r]);
                lsum += e;
                phi[r] = (_Float16)e;
                plo[r] = (_Float16)(e - (float)phi[r]);
              }
              f16x8 v = *reinterpret_cast<const f16x8*>(vp + 16 * ks);
              if constexpr (TIE == 1 || TIE == 2) asm volatile("" : "+v"(v));
              O = __builtin_amdgcn_mfma_f32_32x32x16_f16(v, plo, O, 0, 0, 0);
              O = __builtin_amdgcn_mfma_f32_32x32x16_f16(v, phi, O, 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
#endif
#if HVLA_POLICY_BIAS
          const float ea = __builtin_amdgcn_exp2f(sa - m2);
          lsum = fmaf(ea, 0.5f, lsum);                // both halves hold the same ea and are summed below: once per query (no lane mask,
                                                      // which would be one more loop-invariant SGPR pair)
#endif
          const float inv = 1.f / wave_xor_sum32(lsum);
          float ov[8];
#if HVLA_POLICY_BIAS
          {                                           // + e va, f32: ov[j] is d = 8 (j >> 2) + 4 half + (j & 3) of the head
            const int ln = opaque((int)(threadIdx.x & 63));
            const float* vv = ((SPREAD && ph) ? qkv1 : qa) + 64 + hl * 16 + 4 * (ln >> 5);
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(vv), v1 = *reinterpret_cast<const f32x4*>(vv + 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              ov[j] = fmaf(ea, v0[j], fmaf(O[8 + j], 1.f / 1024.f, O[j])) * inv;
              ov[4 + j] = fmaf(ea, v1[j], fmaf(O[12 + j], 1.f / 1024.f, O[4 + j])) * inv;
            }
          }
#else
#pragma unroll
          for (int j = 0; j < 8; ++j) ov[j] = fmaf(O[8 + j], 1.f / 1024.f, O[j]) * inv;     // V_hi.P + V_lo.P (lo stored x 2^10)
#endif
#if HVLA_POLICY_DIFF
          const float coef = c ? -lam : 1.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) ovd[j] = fmaf(coef, ov[j], ovd[j]);
          }
          {   // RMSNorm over the head's 16 values (8 here, 8 in lane ^ 32), subln's weight (natural order) and 1 - lambda_init
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) ss = fmaf(ovd[j], ovd[j], ss);
            ss += __shfl_xor(ss, 32, 64);
            const float r = rsqrtf(ss * (1.f / 16.f) + 1e-5f) * (1.f - linit);
            const int ln = opaque((int)(threadIdx.x & 63));
            const float* wv = vl + L.v_fc2_b + 96 + 4 * (ln >> 5);
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(wv), w1 = *reinterpret_cast<const f32x4*>(wv + 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              ovd[j] *= r * w0[j];
              ovd[4 + j] *= r * w1[j];
            }
          }
          of[hl] = split8(ovd);
#else
          of[hl] = split8(ov);
          }
#endif
        }
        if (ph == 0) {                        // phase A's outputs wait in LDS (wave-private, lane-linear) for the out-projection
#pragma unroll
          for (int hl = 0; hl < 2; ++hl) {
            *reinterpret_cast<bf16x8*>(park + (2 * hl) * 1024 + lane * 16) = of[hl].hi;
            *reinterpret_cast<bf16x8*>(park + (2 * hl + 1) * 1024 + lane * 16) = of[hl].lo;
          }
        }
      }
      // the next phase / layer rewrites K and V: its writes come two barriers from here (q tile, k tile), behind every
      // wave's last read of this phase
      HVLA_STAMP();                             // 3 + 6 l + 2 ph: attention of the head pair done
    }
    // ---------------- out-projection of the four heads (two staged tiles), straight into the residual
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      const char* slot = acquire();
      if constexpr (SPREAD) {
        const int lane = opaque((int)(threadIdx.x & 63));
        if (ph == 0 && mine) act_combine(1);  // writes oa[32..63] (next tile's input); this tile reads oa[0..31]
        const int tb = (lane >> 4) & 1, rho = 4 * wave + ((lane >> 2) & 3);
        float y = act_rows32x2(slot, lane, wave, tb, 2 + tb, oa + (2 * ph) * 16, oa + (2 * ph + 1) * 16);
        if (ph == 1) y += vl[L.v_out_b + tb * 32 + cidx(rho)];
        if ((lane & 35) == 0) xa[32 * tb + rho] += y;
      } else if (mine) {
        const int lane = opaque((int)(threadIdx.x & 63)), col = lane & 31, half = lane >> 5;
        if (ph == 0) act_combine(1);
#pragma unroll
        for (int t = 0; t < 2; ++t) {         // fragment (hl, t): output rows 32 t.., k = the 16 d of head 2 ph + hl
          float y = frag_dot(slot, t, lane, oa + (2 * ph) * 16 + 4 * half) + frag_dot(slot, 2 + t, lane, oa + (2 * ph + 1) * 16 + 4 * half);
          y += __shfl_xor(y, 32, 64);
          if (ph == 1) y += vl[L.v_out_b + t * 32 + cidx(col)];
          if (half == 0) xa[32 * t + col] += y;
        }
      }
      if (!full) continue;
#pragma unroll
      for (int hl = 0; hl < 2; ++hl) {
        Split8 ob[1];
        if (ph == 0) {
          ob[0].hi = *reinterpret_cast<const bf16x8*>(park + (2 * hl) * 1024 + lane * 16);
          ob[0].lo = *reinterpret_cast<const bf16x8*>(park + (2 * hl + 1) * 1024 + lane * 16);
        } else {
          ob[0] = of[hl];
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) x[t] = tile_mma<1, TIE>(slot, lane, ob, x[t], hl * 2 + t);
      }
    }
    if (full) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float bv[16];
        ldv16(vl + L.v_out_b + (t * 2 + half) * 16, bv);
#pragma unroll
        for (int r = 0; r < 16; ++r) x[t][r] += bv[r];
      }
    }
    HVLA_STAMP();                               // 6 + 6 l: out-projection done
    // ---------------- MLP (transformer.py:56-75): fc1 -> tanh-GELU -> fc2, hidden tile by hidden tile
    {
      Split8 hb[4];
      if (full) ln_frags(x, vl + L.v_ln1_s, vl + L.v_ln1_b, half, hb);
      for (int t = 0; t < TM; ++t) {
        const char* s1 = acquire();
        if constexpr (SPREAD) {
          const int lane = opaque((int)(threadIdx.x & 63));
          if (t == 0) act_ln_private(xa, vl + L.v_ln1_s, vl + L.v_ln1_b, hpriv, lane);
          const int rho = 4 * wave + ((lane >> 3) & 3);
          const float y = gelu_tanh(act_rows64(s1, lane, wave, hpriv) + vl[L.v_fc1_b + t * 32 + cidx(rho)]);
          if ((lane & 39) == 0) ga[rho] = y;
        } else if (mine) {
          const int lane = opaque((int)(threadIdx.x & 63)), col = lane & 31, half = lane >> 5;
          if (t == 0) act_ln(xa, vl + L.v_ln1_s, vl + L.v_ln1_b, h1, lane);
          const float y = gelu_tanh(act_matvec64(s1, lane, h1) + vl[L.v_fc1_b + t * 32 + cidx(col)]);
          if (half == 0) ga[col] = y;
        }
        Split8 gf[2];
        if (full) {
          f32x16 a;
          {
            float bv[16];
            ldv16(vl + L.v_fc1_b + (t * 2 + half) * 16, bv);
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = bv[r];
          }
          a = tile_mma<4, TIE>(s1, lane, hb, a);
#pragma unroll
          for (int r = 0; r < 16; ++r) a[r] = gelu_tanh(a[r]);
          gf[0] = acc_frag<0>(a);
          gf[1] = acc_frag<1>(a);
        }
        const char* s2 = acquire();
        if constexpr (SPREAD) {
          const int lane = opaque((int)(threadIdx.x & 63));
          const int tb = (lane >> 4) & 1, rho = 4 * wave + ((lane >> 2) & 3);
          float y = act_rows32x2(s2, lane, wave, 2 * tb, 2 * tb + 1, ga, ga + 16);
          if (t == TM - 1) y += vl[L.v_fc2_b + tb * 32 + cidx(rho)];
          if ((lane & 35) == 0) xa[32 * tb + rho] += y;
        } else if (mine) {
          const int lane = opaque((int)(threadIdx.x & 63)), col = lane & 31, half = lane >> 5;
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) {    // fragments 2 mt + ks: output rows 32 mt.., k-step ks of the 32 hidden values
            float y = frag_dot(s2, 2 * mt, lane, ga + 4 * half) + frag_dot(s2, 2 * mt + 1, lane, ga + 16 + 4 * half);
            y += __shfl_xor(y, 32, 64);
            if (t == TM - 1) y += vl[L.v_fc2_b + mt * 32 + cidx(col)];
            if (half == 0) xa[32 * mt + col] += y;
          }
        }
        if (full) {
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) x[mt] = tile_mma<2, TIE>(s2, lane, gf, x[mt], mt * 2);
        }
      }
      if (full) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          float bv[16];
          ldv16(vl + L.v_fc2_b + (t * 2 + half) * 16, bv);
#pragma unroll
          for (int r = 0; r < 16; ++r) x[t][r] += bv[r];
        }
      }
    }
    HVLA_STAMP();                               // 7 + 6 l: MLP done
  }

  // ---------------- encoder_norm on the action token + mix head (action_heads.py:455-472,534-538)
  {
    HVLA_STAMP();                               // 2 + 6 L: layers done
    const char* slot = acquire();
    if (SPREAD || mine) {
      const int lane = opaque((int)(threadIdx.x & 63)), col = lane & 31, half = lane >> 5;
      float v;
      bool writer;
      int n;
      if constexpr (SPREAD) {
        act_ln_private(xa, vtail + L.v_norm_s, vtail + L.v_norm_b, hpriv, lane);
        n = 4 * wave + ((lane >> 3) & 3);
        v = act_rows64(slot, lane, wave, hpriv) + vtail[L.v_head_b + cidx(n)];
        writer = (lane & 39) == 0;
      } else {
        act_ln(xa, vtail + L.v_norm_s, vtail + L.v_norm_b, h0, lane);
        n = col;
        v = act_matvec64(slot, lane, h0) + vtail[L.v_head_b + cidx(col)];
        writer = half == 0;
      }
      if (writer) {
        const int A = p.horizon * (p.action_dim - 1), ad = p.action_dim;
        float* act = p.actions + (size_t)b * p.horizon * ad;
        if (n < A) {
          act[(n / (ad - 1)) * ad + (n % (ad - 1))] = tanhf(v / p.tanh_scale) * p.max_action;
        } else if (n < A + p.horizon) {
          act[(n - A) * ad + (ad - 1)] = v >= 0.f ? 1.f : 0.f;
          if (p.logits) p.logits[(size_t)b * p.horizon + (n - A)] = v;
        }
      }
    }
  }
