// train_launch_trace.h -- what csrc/train.hip's launch seam becomes under -DHVLA_TRAIN_TRACE (tools/train_launch_trace.hip and
// tools/train_extent_trace.hip only; neither library sets the flag).  Included by train.hip INSIDE namespace hvla, behind
// HeadP / AuxP / BG: KL, ENQ and bgemm() print one line per operation and enqueue nothing, so the host sequencing of train_step / train_apply / train_accumulate runs on
// a machine without a GPU, on pointers nobody dereferences.  tests/native/train_step_trace.txt is this output, recorded once.
//
// Pointers print as buffer+offset (elements of the pointer's type) against the fake bases below, 2^40 bytes apart and 4 KiB
// aligned like device allocations, so that the alignment and ordering tests of the sequencing see what they see in production.
constexpr const char* TRACE_BUFFERS[] = {"params", "grads", "mu", "nu", "ema", "theta", "dtheta", "work", "loss", "actions", "logits",
                                         "sqsum", "wd_mask", "params0", "tok", "attn_mask", "cls", "tokens", "images", "target", "tmask",
                                         "amask", "acc", "frozen", "pos_w", "aux_ref", "aux_ent", "aux_align", "event", "st", "tiles"};
constexpr int TRACE_NBUF = sizeof(TRACE_BUFFERS) / sizeof(TRACE_BUFFERS[0]);
void* train_trace_buffer(const char* name) {
  for (int i = 0; i < TRACE_NBUF; ++i)
    if (!strcmp(TRACE_BUFFERS[i], name)) return reinterpret_cast<void*>((uintptr_t)(i + 1) << 40);
  fprintf(stderr, "train_trace_buffer: no buffer '%s'\n", name);
  abort();
}
static void trace_ptr(const void* p, int elem) {
  if (!p) { printf("null"); return; }
  const uintptr_t u = (uintptr_t)p, i = (u + ((uintptr_t)1 << 39)) >> 40;
  if (i < 1 || i > (uintptr_t)TRACE_NBUF) { printf("?%llx", (unsigned long long)u); return; }
  const long long d = (long long)u - (long long)(i << 40);
  if (d % elem) printf("%s%+lldB", TRACE_BUFFERS[i - 1], d);
  else printf("%s%+lld", TRACE_BUFFERS[i - 1], d / elem);
}
template <class T> static void trace_arg(T* p) { trace_ptr(p, (int)sizeof(T)); }
static void trace_arg(hipEvent_t e) { trace_ptr(e, 1); }
static void trace_arg(hipStream_t s) { trace_ptr(s, 1); }
static void trace_arg(std::nullptr_t) { printf("null"); }
static void trace_arg(bool v) { printf("%d", (int)v); }
static void trace_arg(int v) { printf("%d", v); }
static void trace_arg(unsigned v) { printf("%u", v); }
static void trace_arg(long v) { printf("%ld", v); }
static void trace_arg(unsigned long v) { printf("%lu", v); }
static void trace_arg(long long v) { printf("%lld", v); }
static void trace_arg(float v) { printf("%.9g", (double)v); }
static void trace_arg(hipMemcpyKind k) { printf("kind%d", (int)k); }
static void trace_arg(dim3 d) { printf("(%u,%u,%u)", d.x, d.y, d.z); }
template <class... Ts> static void trace_list(const Ts&... a) {
  const char* sep = "";
  ((printf("%s", sep), trace_arg(a), sep = " "), ...);
}
#define TRACE_F(s, f) (printf(" " #f "="), trace_arg((s).f))
static void trace_arg(const BG& g) {      // positional, in the order of the struct (train.h)
  printf("BG{"), trace_list(g.A, g.B, g.C, g.bias, g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.sA0, g.sA1, g.sB0, g.sB1, g.sC0, g.sC1, g.sBias0, g.nb1,
                            g.alpha, g.accumulate, g.ksplit, g.allow_split, g.a_padded, g.sBias1), printf("}");
}
static void trace_arg(const HeadP& p) {
  printf("HeadP{");
  TRACE_F(p, x); TRACE_F(p, xstride); TRACE_F(p, theta); TRACE_F(p, dtheta); TRACE_F(p, G); TRACE_F(p, o_wc); TRACE_F(p, o_bc); TRACE_F(p, o_wd);
  TRACE_F(p, o_bd); TRACE_F(p, o_ns); TRACE_F(p, o_nb); TRACE_F(p, target); TRACE_F(p, tmask); TRACE_F(p, amask); TRACE_F(p, loss); TRACE_F(p, dxrow);
  TRACE_F(p, actions); TRACE_F(p, logits); TRACE_F(p, B); TRACE_F(p, S); TRACE_F(p, D); TRACE_F(p, Hz); TRACE_F(p, ad);
  TRACE_F(p, tanh_scale); TRACE_F(p, max_action); TRACE_F(p, clip_target);
  printf(" }");
}
static void trace_arg(const AuxP& a) {
  printf("AuxP{");
  TRACE_F(a, p); TRACE_F(a, dp); TRACE_F(a, sb); TRACE_F(a, sh); TRACE_F(a, S); TRACE_F(a, Sp); TRACE_F(a, H); TRACE_F(a, P); TRACE_F(a, w_ent);
  TRACE_F(a, w_align); TRACE_F(a, ref); TRACE_F(a, loss); TRACE_F(a, ent); TRACE_F(a, align); TRACE_F(a, gscale);
  printf(" }");
}
static void trace_arg(const NoiseKey& k) {
  printf("NoiseKey{");
  TRACE_F(k, k0); TRACE_F(k, k1); TRACE_F(k, site); TRACE_F(k, draw); TRACE_F(k, sample0);
  printf(" }");
}
#undef TRACE_F
#define KL(kernel, grid, block, ...) (printf("%s ", #kernel), trace_list(dim3(grid), dim3(block), __VA_ARGS__), (void)printf("\n"))
#define ENQ(fn, ...) (printf("%s ", #fn), trace_list(__VA_ARGS__), (void)printf("\n"))
// train.h's bgemm(): these builds do not compile csrc/train_gemm.hip
void bgemm(hipStream_t, bool ta, bool tb, BG g, int nb0) { printf("bgemm "), trace_list(ta, tb, nb0, g), (void)printf("\n"); }
// ... and its grouped form (layer tokens): the table prints as tiles+<entries>, its grid as ntiles, tile and nz
void bgemm_groups(hipStream_t, bool ta, bool tb, BG g, const BGTile* tiles, int ntiles, int tile, int nz, bool vec_ok, double) {
  printf("bgemm_groups "), trace_list(ta, tb, g, tiles, ntiles, tile, nz, vec_ok), (void)printf("\n");
}
