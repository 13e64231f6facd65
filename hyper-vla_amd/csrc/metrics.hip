// metrics.hip — what the reference's training loop logs at every step, from the device buffers of the fine-tune step
// (include/hvla.h hvla_train_metrics / hvla_loss_terms; scripts/train.py:494-529 `info`, :546-583 validation_action_loss).
//
// Every kernel here: no allocation, no host synchronisation, launched on the caller's stream only; writes nothing but the output
// vector and the caller's scratch; every sum in a FIXED order without atomics, accumulated in f64 and rounded to f32 once at the
// final store -- a metric is a function of the data alone (bit-reproducible) and within one f32 rounding of the exact value.
// (sqsum_kernel of train.hip, the clip's norm, adds f32 partial sums with atomics: its sqsum[0] and GRAD_NORM^2 differ by that
// rounding)
//
//   norms_kernel<MODE>      one pass over the flat training vector, NORMS_WG workgroups whatever n is, workgroup w owns the
//                           contiguous chunk [w chunk, (w + 1) chunk), chunk a multiple of 4 elements.  MODE bit 0 (PRE) reads
//                           grads, params and the frozen mask: sum g^2 over EVERY element (the reference's optax.global_norm(grads),
//                           frozen elements of a computed bucket included; a bucket declared frozen was not computed and
//                           contributes zeros), sum p^2 over the elements param_norm counts (not frozen: param_norm_callable,
//                           octo/utils/train_utils.py:437-441, zeroes frozen leaves; not the baked position slot while the source is
//                           on: it is a derived quantity, the source tail is the parameter), and sum p^2 over the shared encoder
//                           leaves (the slot again replaced by the tail) for base_params_norm.  MODE bit 1 (UPDATE) reads params and
//                           the snapshot: sum (p - prev)^2 outside the slot.  16-byte loads when every pointer is 16-byte aligned
//                           (a chunk then starts aligned; the boundaries inside the vector -- L.total, the slot -- need not be:
//                           they are compared per element); the last n % 4 elements, or everything when a pointer is not
//                           aligned, go scalar.  A thread's f64 partials -> wave xor-shuffle -> LDS -> one f64 quadruple per
//                           workgroup into the scratch.
//   norms_finish_kernel     one workgroup: the partials in ascending workgroup order.
//   row_norms_kernel        sum theta_b^2 of row b of theta [B, G], one workgroup per row (base_params_norm, scripts/train.py:384).
//   loss_terms_kernel       the two halves of MixActionHead.loss per sample (action_heads.py:517-521 `metrics`), with the expressions
//                           and the summation order of head_loss_kernel (train.hip): one wave per sample, lane = output; and the
//                           unmasked squared error against clip(target, -5, 5) (scripts/train.py:580-581).
//   metrics_finish_kernel   one workgroup assembles the output vector: means over b in ascending order, per-task sums and counts,
//                           the square roots.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "train.h"

namespace hvla {

constexpr int NORMS_WG = HVLA_TRAIN_METRICS_WORKGROUPS, NORMS_THREADS = 256, NORMS_SUMS = 4;   // sums: g2, p2, d2, e2
constexpr int MAXB = HVLA_TRAIN_METRICS_MAX_BATCH;
// the caller's scratch, in doubles
constexpr long SC_PARTIAL = 0, SC_SUMS = SC_PARTIAL + (long)NORMS_WG * NORMS_SUMS, SC_ROWSQ = SC_SUMS + 8, SC_SQERR = SC_ROWSQ + MAXB,
               SC_TERMS = SC_SQERR + MAXB /* f32 continuous [MAXB] | gripper [MAXB] */, SC_END = SC_TERMS + MAXB;
static_assert(SC_END == HVLA_TRAIN_METRICS_SCRATCH_DOUBLES, "include/hvla.h states the scratch size");
static_assert(NORMS_WG * NORMS_SUMS * sizeof(double) <= 32768, "norms_finish_kernel stages the partials in LDS");

struct NormsP {
  const float* g;            // grads   (PRE)
  const float* p;            // params
  const float* prev;         // the snapshot (UPDATE)
  const uint8_t* frozen;     // nullable
  long n, chunk;             // chunk % 4 == 0
  long slot0, slot1;         // the baked position slot, out of p2 / d2 / e2 (slot0 == slot1: the source is off)
  long enc0;                 // e2 counts [enc0, n) outside the slot (n: nothing -- frozen encoder)
  int vec;                   // every pointer 16-byte aligned
  double* partial;           // [NORMS_WG][NORMS_SUMS]
};

template <int MODE>
__device__ __forceinline__ void norms_elem(const NormsP& a, long i, float g, float p, float pv, unsigned fz, double& g2, double& p2,
                                           double& d2, double& e2) {
  const bool slot = i >= a.slot0 && i < a.slot1;
  if (MODE & 1) {
    const double gd = (double)g, pd = (double)p, q = pd * pd;      // exact products of f32 values
    g2 += gd * gd;
    p2 += (slot || fz) ? 0.0 : q;
    e2 += (slot || i < a.enc0) ? 0.0 : q;
  }
  if (MODE & 2) {
    const double d = (double)p - (double)pv;
    d2 += slot ? 0.0 : d * d;
  }
}

template <int MODE>
__global__ void __launch_bounds__(NORMS_THREADS) norms_kernel(NormsP a) {
  __shared__ double red[NORMS_THREADS / 64][NORMS_SUMS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long c0 = (long)blockIdx.x * a.chunk;
  const long c1 = c0 < a.n ? (c0 + a.chunk < a.n ? c0 + a.chunk : a.n) : c0;      // [c0, c1), empty behind the vector's end
  double g2 = 0.0, p2 = 0.0, d2 = 0.0, e2 = 0.0;
  if (a.vec) {
    const long v1 = c0 + ((c1 - c0) & ~3L);                                        // c0 % 4 == 0: whole groups of 4 below v1 <= n
    for (long i = c0 + 4L * tid; i < v1; i += 4L * NORMS_THREADS) {
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f), pv = g;
      unsigned fz = 0;
      const float4 p = *reinterpret_cast<const float4*>(a.p + i);
      if (MODE & 1) {
        g = *reinterpret_cast<const float4*>(a.g + i);
        if (a.frozen) fz = *reinterpret_cast<const unsigned*>(a.frozen + i);
      }
      if (MODE & 2) pv = *reinterpret_cast<const float4*>(a.prev + i);
      norms_elem<MODE>(a, i, g.x, p.x, pv.x, fz & 0xffu, g2, p2, d2, e2);
      norms_elem<MODE>(a, i + 1, g.y, p.y, pv.y, fz & 0xff00u, g2, p2, d2, e2);
      norms_elem<MODE>(a, i + 2, g.z, p.z, pv.z, fz & 0xff0000u, g2, p2, d2, e2);
      norms_elem<MODE>(a, i + 3, g.w, p.w, pv.w, fz & 0xff000000u, g2, p2, d2, e2);
    }
    const long i = v1 + tid;                                                       // the vector's last n % 4 elements
    if (i < c1)
      norms_elem<MODE>(a, i, (MODE & 1) ? a.g[i] : 0.f, a.p[i], (MODE & 2) ? a.prev[i] : 0.f,
                       ((MODE & 1) && a.frozen) ? a.frozen[i] : 0u, g2, p2, d2, e2);
  } else {
    for (long i = c0 + tid; i < c1; i += NORMS_THREADS)
      norms_elem<MODE>(a, i, (MODE & 1) ? a.g[i] : 0.f, a.p[i], (MODE & 2) ? a.prev[i] : 0.f,
                       ((MODE & 1) && a.frozen) ? a.frozen[i] : 0u, g2, p2, d2, e2);
  }
  for (int o = 32; o; o >>= 1) {
    g2 += __shfl_xor(g2, o, 64); p2 += __shfl_xor(p2, o, 64); d2 += __shfl_xor(d2, o, 64); e2 += __shfl_xor(e2, o, 64);
  }
  if (lane == 0) { red[wave][0] = g2; red[wave][1] = p2; red[wave][2] = d2; red[wave][3] = e2; }
  __syncthreads();
  if (tid < NORMS_SUMS) {
    double s = red[0][tid];
    for (int w = 1; w < NORMS_THREADS / 64; ++w) s += red[w][tid];
    a.partial[(long)blockIdx.x * NORMS_SUMS + tid] = s;
  }
}

// sums[s] = partial[0][s] + partial[1][s] + ...; only the sums of `mode` are written (PRE: g2, p2, e2; UPDATE: d2)
__global__ void __launch_bounds__(256) norms_finish_kernel(const double* __restrict__ partial, double* __restrict__ sums, int mode) {
  __shared__ double sh[NORMS_WG * NORMS_SUMS];
  for (int i = threadIdx.x; i < NORMS_WG * NORMS_SUMS; i += 256) sh[i] = partial[i];
  __syncthreads();
  const int s = threadIdx.x;
  if (s >= NORMS_SUMS || !(mode & (s == 2 ? 2 : 1))) return;
  double acc = 0.0;
  for (int w = 0; w < NORMS_WG; ++w) acc += sh[w * NORMS_SUMS + s];
  sums[s] = acc;
}

__global__ void __launch_bounds__(256) row_norms_kernel(const float* __restrict__ theta, long G, int vec, double* __restrict__ rowsq) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const float* row = theta + (long)blockIdx.x * G;
  double s = 0.0;
  if (vec) {                                   // G % 4 == 0 and theta 16-byte aligned
    for (long i = 4L * tid; i < G; i += 4L * 256) {
      const float4 v = *reinterpret_cast<const float4*>(row + i);
      const double x = v.x, y = v.y, z = v.z, w = v.w;
      s += x * x; s += y * y; s += z * z; s += w * w;
    }
  } else {
    for (long i = tid; i < G; i += 256) { const double x = row[i]; s += x * x; }
  }
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) rowsq[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One wave per sample, lane = output as in head_loss_kernel (lanes < A: continuous (h, a); lanes A .. A + Hz: the gripper of step h),
// the same f32 expressions and the same xor-shuffle order, so that continuous[b] and gripper[b] are the two terms whose sum that
// kernel stores.  sqerr: f64, every (h, a), no mask, the gripper column being the 0 / 1 threshold `actions` holds.
__global__ void __launch_bounds__(64) loss_terms_kernel(const float* __restrict__ actions, const float* __restrict__ logits,
                                                        const float* __restrict__ target, const uint8_t* __restrict__ tmask,
                                                        const uint8_t* __restrict__ amask, float* __restrict__ continuous,
                                                        float* __restrict__ gripper, float* __restrict__ sqerr,
                                                        double* __restrict__ sqerr64, int Hz, int ad, float max_action, int clip_target) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int A = Hz * (ad - 1), NO = A + Hz;                 // NO <= 32 (hvla_create)
  const bool tm = tmask[b] != 0;
  float cs = 0.f, cm = 0.f, ds = 0.f, dm = 0.f;
  double se = 0.0;
  if (lane < NO) {
    int h, a;
    if (lane < A) { h = lane / (ad - 1); a = lane % (ad - 1); } else { h = lane - A; a = ad - 1; }
    const long o = ((long)b * Hz + h) * ad + a;
    const float mk = (tm && amask[o]) ? 1.f : 0.f;
    const float raw = target[o];
    const float tgt = clip_target ? fminf(fmaxf(raw, -max_action), max_action) : raw;
    const float pred = actions[o];
    if (lane < A) {
      cs = (pred - tgt) * (pred - tgt) * mk; cm = mk;
    } else {
      const float z = logits[(long)b * Hz + h];
      const float sp = log1pf(expf(-fabsf(z)));
      ds = (tgt * (fmaxf(-z, 0.f) + sp) + (1.f - tgt) * (fmaxf(z, 0.f) + sp)) * mk; dm = mk;
    }
    const double d = (double)pred - (double)fminf(fmaxf(raw, -5.f), 5.f);       // the literal +-5 of scripts/train.py:580
    se = d * d;
  }
  for (int o = 32; o; o >>= 1) {
    cs += __shfl_xor(cs, o, 64); cm += __shfl_xor(cm, o, 64); ds += __shfl_xor(ds, o, 64); dm += __shfl_xor(dm, o, 64);
    se += __shfl_xor(se, o, 64);
  }
  if (lane != 0) return;
  const float nc = (float)A, nd = (float)Hz;
  const float dc = fmaxf(cm / nc, 1e-5f), dd = fmaxf(dm / nd, 1e-5f);
  continuous[b] = (cs / nc) / dc * (float)(ad - 1);
  gripper[b] = (ds / nd) / dd;
  if (sqerr) sqerr[b] = (float)se;
  if (sqerr64) sqerr64[b] = se;
}

struct FinishP {
  int select, B, n_tasks, horizon;
  const float* loss;         // [B]; everything below nullable: its slots are then not written
  const float* cont;
  const float* grip;
  const double* sqerr;
  const double* rowsq;
  const float* ent;
  const float* align;
  const int32_t* task_ids;
  const double* sums;        // g2, p2, d2, e2
  double enc_sq;             // frozen encoder: the caller's; < 0: sums[3]
  float* out;
};
template <typename T>
__device__ __forceinline__ double mean_of(const T* __restrict__ v, int B) {
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += (double)v[b];
  return s / (double)B;
}
__global__ void __launch_bounds__(256) metrics_finish_kernel(FinishP a) {
  const int tid = threadIdx.x;
  const bool pre = a.select & HVLA_METRICS_PRE, upd = a.select & HVLA_METRICS_UPDATE;
  float* rep = a.out + HVLA_METRIC_LOCAL_N + 2 * a.n_tasks;                       // the replicated block
  if (tid >= 64) {                                                                // the tasks: waves 1 .. 3
    if (!pre || !a.task_ids || !a.loss) return;
    for (int t = tid - 64; t < a.n_tasks; t += 192) {
      double s = 0.0;
      int c = 0;
      for (int b = 0; b < a.B; ++b)
        if (a.task_ids[b] == t) { s += (double)a.loss[b]; ++c; }                  // an id outside [0, n_tasks) is counted nowhere
      a.out[HVLA_METRIC_LOCAL_N + t] = (float)s;
      a.out[HVLA_METRIC_LOCAL_N + a.n_tasks + t] = (float)c;
    }
    return;
  }
  if (upd && tid == 8) rep[HVLA_METRIC_UPDATE_NORM - HVLA_METRIC_LOCAL_N] = (float)sqrt(a.sums[2]);
  if (!pre) return;
  switch (tid) {
    case 0: if (a.loss) a.out[HVLA_METRIC_TRAINING_LOSS] = (float)mean_of(a.loss, a.B); break;
    case 1: if (a.cont) a.out[HVLA_METRIC_CONTINUOUS_LOSS] = (float)mean_of(a.cont, a.B); break;
    case 2: if (a.grip) a.out[HVLA_METRIC_GRIPPER_LOSS] = (float)mean_of(a.grip, a.B); break;
    case 3: if (a.sqerr) a.out[HVLA_METRIC_MSE] = (float)(mean_of(a.sqerr, a.B) / (double)a.horizon); break;
    case 4:
      if (a.rowsq) {
        const double e = a.enc_sq < 0.0 ? a.sums[3] : a.enc_sq;
        double s = 0.0;
        for (int b = 0; b < a.B; ++b) s += sqrt(a.rowsq[b] + e);
        a.out[HVLA_METRIC_BASE_PARAMS_NORM] = (float)(s / (double)a.B);
      }
      break;
    case 5: if (a.ent) a.out[HVLA_METRIC_ATTENTION_ENTROPY] = (float)mean_of(a.ent, a.B); break;
    case 6: if (a.align) a.out[HVLA_METRIC_ATTENTION_ALIGNMENT] = (float)mean_of(a.align, a.B); break;
    case 7:
      rep[HVLA_METRIC_GRAD_NORM - HVLA_METRIC_LOCAL_N] = (float)sqrt(a.sums[0]);
      rep[HVLA_METRIC_PARAM_NORM - HVLA_METRIC_LOCAL_N] = (float)sqrt(a.sums[1]);
      break;
    default: break;
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

hipError_t launch_loss_terms(const float* actions, const float* logits, const float* target, const uint8_t* tmask, const uint8_t* amask,
                             float* continuous, float* gripper, float* sqerr, double* sqerr64, int B, int horizon, int action_dim,
                             float max_action, bool clip_target, hipStream_t st) {
  hipLaunchKernelGGL(loss_terms_kernel, dim3(B), dim3(64), 0, st, actions, logits, target, tmask, amask, continuous, gripper, sqerr,
                     sqerr64, horizon, action_dim, max_action, clip_target ? 1 : 0);
  return hipGetLastError();
}

hipError_t train_metrics(const Geom& g, const TrainLayout& L, const TrainBuffers& tb, const hvla_train_metrics_in& in, float* out, int B,
                         bool train_encoder, hipStream_t st, const TrainOptions& opt) {
  const PosSource& ps = opt.ps;                              // (off unless the encoder is trained: api.hip train_options)
  const long n = train_vector_elems(L, ps, train_encoder);
  const bool pre = in.select & HVLA_METRICS_PRE, upd = in.select & HVLA_METRICS_UPDATE;
  double* sc = in.scratch;
  if (pre || upd) {
    NormsP a{};
    a.g = tb.grads; a.p = tb.params; a.prev = in.prev_params; a.frozen = opt.frozen;
    a.n = n;
    a.chunk = ((n + NORMS_WG - 1) / NORMS_WG + 3) & ~3L;
    a.slot0 = a.slot1 = 0;
    if (ps.n > 0) { a.slot0 = L.total + L.e_pos; a.slot1 = a.slot0 + (long)(g.P() + 1) * g.E; }
    a.enc0 = train_encoder ? L.total : n;
    a.vec = aligned16(tb.params) && (!pre || (aligned16(tb.grads) && aligned16(opt.frozen))) && (!upd || aligned16(in.prev_params));
    a.partial = sc + SC_PARTIAL;
    if (pre && upd) hipLaunchKernelGGL(norms_kernel<3>, dim3(NORMS_WG), dim3(NORMS_THREADS), 0, st, a);
    else if (pre) hipLaunchKernelGGL(norms_kernel<1>, dim3(NORMS_WG), dim3(NORMS_THREADS), 0, st, a);
    else hipLaunchKernelGGL(norms_kernel<2>, dim3(NORMS_WG), dim3(NORMS_THREADS), 0, st, a);
    hipLaunchKernelGGL(norms_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)(sc + SC_PARTIAL), sc + SC_SUMS, (int)(in.select & 3));
  }
  FinishP f{};
  f.select = in.select & 3; f.B = B; f.n_tasks = in.n_tasks; f.horizon = g.horizon;
  f.sums = sc + SC_SUMS; f.out = out;
  f.enc_sq = train_encoder ? -1.0 : in.encoder_sqsum;
  if (pre) {
    f.loss = tb.loss; f.ent = in.entropy; f.align = in.alignment; f.task_ids = in.task_ids;
    if (tb.theta) {
      hipLaunchKernelGGL(row_norms_kernel, dim3(B), dim3(256), 0, st, (const float*)tb.theta, L.G, (int)(L.G % 4 == 0 && aligned16(tb.theta)),
                         sc + SC_ROWSQ);
      f.rowsq = sc + SC_ROWSQ;
    }
    if (in.target && in.timestep_mask && in.action_mask && tb.actions && tb.logits) {
      float* terms = reinterpret_cast<float*>(sc + SC_TERMS);
      hipLaunchKernelGGL(loss_terms_kernel, dim3(B), dim3(64), 0, st, (const float*)tb.actions, (const float*)tb.logits, in.target,
                         in.timestep_mask, in.action_mask, terms, terms + MAXB, (float*)nullptr, sc + SC_SQERR, g.horizon,
                         g.action_dim, g.max_action, g.clip_target ? 1 : 0);
      f.cont = terms; f.grip = terms + MAXB; f.sqerr = sc + SC_SQERR;
    }
  }
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(256), 0, st, f);
  return hipGetLastError();
}

}  // namespace hvla
