// train.hip — fine-tune step of the hypernetwork (BASELINE config 5):
//   forward + backward of  loss(params) = mean_b MixLoss(policy(theta_b(params), tokens_b), action_b)
//   (scripts/train.py:326-346,453-460; hypervla/components/action_heads.py:474-522), fused
//   clip-by-global-norm + AdamW (bf16 first moment) + EMA (octo/utils/train_utils.py:411-426,
//   scripts/train.py:618-625).  The DINOv2 image encoder is FROZEN in this first version
//   (`fine_tune_pretrained_image_encoder=False`, the reference's config default): its tokens come from
//   hvla_encode; gradients flow to every hypernetwork parameter (73 output heads = W_cat / b_cat, the
//   context encoder, the projections and position embeddings).
//
// Correctness-first f32 implementation: one generic strided/batched f32 GEMM (bgemm(), train_gemm.hip; per-episode weights
// are just a batch stride into theta[B, G]) plus small LayerNorm / softmax / GELU / bias-gradient kernels,
// sequenced by host code.  Activations are kept in a workspace; cheap things (LN output, GELU) are
// recomputed in the backward pass.  Parity: every gradient leaf against autograd on the float64 CPU
// restatement (tests/test_gpu_train.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "train.h"

namespace hvla {

// ------------------------------------------------------------------------------------------------
// row kernels (one wave per row).  Rows are [nb][S][D]; per-row parameters come from p + b * pstride.
// ------------------------------------------------------------------------------------------------
__global__ void ln_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ mean,
                              float* __restrict__ rstd, const float* __restrict__ scale,
                              const float* __restrict__ bias, long pstride, int rows, int S, int D) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (long)row * D;
  float s = 0.f, q = 0.f;
  for (int c = lane; c < D; c += 64) { s += xr[c]; q += xr[c] * xr[c]; }
  for (int o = 32; o; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
  const float m = s / D, var = fmaxf(0.f, q / D - m * m), r = rsqrtf(var + 1e-6f);
  const float* sc = scale + (long)(row / S) * pstride;
  const float* bi = bias + (long)(row / S) * pstride;
  for (int c = lane; c < D; c += 64) y[(long)row * D + c] = (xr[c] - m) * r * sc[c] + bi[c];
  if (lane == 0) { mean[row] = m; rstd[row] = r; }
}

// dx (+)= LN backward; per-row contributions to dscale / dbias are accumulated with atomics into
// dscale + b * pstride (per-episode parameters: pstride = G; shared parameters: pstride = 0).
__global__ void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mean,
                              const float* __restrict__ rstd, const float* __restrict__ scale, float* __restrict__ dx,
                              float* __restrict__ dscale, float* __restrict__ dbias, long pstride, int rows, int S,
                              int D, int accumulate) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float m = mean[row], r = rstd[row];
  const float* xr = x + (long)row * D;
  const float* dyr = dy + (long)row * D;
  const float* sc = scale + (long)(row / S) * pstride;
  float s1 = 0.f, s2 = 0.f;                               // sum(dxhat), sum(dxhat * xhat)
  for (int c = lane; c < D; c += 64) {
    const float xh = (xr[c] - m) * r, dxh = dyr[c] * sc[c];
    s1 += dxh; s2 += dxh * xh;
  }
  for (int o = 32; o; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
  float* ds = dscale + (long)(row / S) * pstride;
  float* db = dbias + (long)(row / S) * pstride;
  for (int c = lane; c < D; c += 64) {
    const float xh = (xr[c] - m) * r, dxh = dyr[c] * sc[c];
    const float v = r * (dxh - s1 / D - xh * s2 / D);
    float* d = dx + (long)row * D + c;
    *d = accumulate ? *d + v : v;
    if (dscale) {
      unsafeAtomicAdd(ds + c, dyr[c] * xh);
      unsafeAtomicAdd(db + c, dyr[c]);
    }
  }
}

// LN backward for SHARED parameters in one pass (round 3; before: ln_bwd_kernel + ln_pgrad_kernel, each reading x and dy: 28 + 22 us
// for 8 224 x 768): a workgroup of eight waves takes 64 rows, a wave its rows one after the other with x and dy of a row in
// registers (float4, read once), dx (+)= r (dxhat - mean(dxhat) - xhat mean(dxhat xhat)), and every lane keeps the dscale / dbias
// sums of its columns; the waves are combined through LDS, one atomic per (workgroup, column).  D % 4 == 0, D <= 1024.
constexpr int LNB_WAVES = 8;
__global__ __launch_bounds__(LNB_WAVES * 64) void ln_bwd_shared_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ scale, float* __restrict__ dx,
                                                            float* __restrict__ dscale, float* __restrict__ dbias, int rows, int D,
                                                            int accumulate) {
  __shared__ f32x4 red[2][LNB_WAVES][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n4 = D / 4;
  f32x4 sc[4], ga[4], gb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    ga[i] = gb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    sc[i] = c < n4 ? reinterpret_cast<const f32x4*>(scale)[c] : ga[i];
  }
  const int r0 = blockIdx.x * 64, r1 = r0 + 64 < rows ? r0 + 64 : rows;
  const float invD = 1.f / (float)D;
  for (int row = r0 + wave; row < r1; row += LNB_WAVES) {
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (long)row * D);
    const f32x4* dr = reinterpret_cast<const f32x4*>(dy + (long)row * D);
    f32x4* ox = reinterpret_cast<f32x4*>(dx + (long)row * D);
    f32x4 xv[4], dv[4], old[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      xv[i] = dv[i] = old[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < n4) {
        xv[i] = xr[c];
        dv[i] = dr[c];
        if (accumulate) old[i] = ox[c];
      }
    }
    const float m = mean[row], r = rstd[row];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (lane + 64 * i < n4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float xh = (xv[i][j] - m) * r, dxh = dv[i][j] * sc[i][j];
          s1 += dxh;
          s2 = fmaf(dxh, xh, s2);
          ga[i][j] = fmaf(dv[i][j], xh, ga[i][j]);
          gb[i][j] += dv[i][j];
          xv[i][j] = xh;                     // keep xhat and dxhat for the second half
          dv[i][j] = dxh;
        }
      }
    }
    for (int o = 32; o; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    s1 *= invD;
    s2 *= invD;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      if (c < n4) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = old[i][j] + r * (dv[i][j] - s1 - xv[i][j] * s2);
        ox[c] = v;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[0][wave][lane + 64 * i] = ga[i], red[1][wave][lane + 64 * i] = gb[i];
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * n4; c += LNB_WAVES * 64) {
    const int which = c >= n4, cc = c - which * n4;
    f32x4 t = red[which][0][cc];
#pragma unroll
    for (int w = 1; w < LNB_WAVES; ++w) t += red[which][w][cc];
    float* o = (which ? dbias : dscale) + 4 * cc;
#pragma unroll
    for (int j = 0; j < 4; ++j) unsafeAtomicAdd(o + j, t[j]);
  }
}

// shared LayerNorm parameters: dscale[c] += sum_r dy[r][c] xhat[r][c], dbias[c] += sum_r dy[r][c]; 64 rows per
// block (blockIdx.y) reduced in registers, one atomic per (block, column) instead of one per element.
__global__ void ln_pgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mean,
                                const float* __restrict__ rstd, float* __restrict__ dscale, float* __restrict__ dbias,
                                int rows, int D) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= D) return;
  const int r0 = blockIdx.y * 64, r1 = r0 + 64 < rows ? r0 + 64 : rows;
  float a = 0.f, b = 0.f;
  for (int r = r0; r < r1; ++r) {
    const float d = dy[(long)r * D + c];
    a = fmaf(d, (x[(long)r * D + c] - mean[r]) * rstd[r], a);
    b += d;
  }
  unsafeAtomicAdd(dscale + c, a);
  unsafeAtomicAdd(dbias + c, b);
}

// LayerScale (DINOv2 layer_scale{1,2}.lambda1): out = res + ls (.) y
__global__ void scale_add_kernel(float* __restrict__ out, const float* __restrict__ res, const float* __restrict__ y,
                                 const float* __restrict__ ls, long n, int D) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = res[i] + ls[i % D] * y[i];
}
// float4 form (D % 4 == 0, 16-byte aligned): no 64-bit modulo per element
__global__ void scale_add4_kernel(f32x4* __restrict__ out, const f32x4* __restrict__ res, const f32x4* __restrict__ y,
                                  const f32x4* __restrict__ ls, long n4, int d4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 l = ls[(int)(i % d4)], r = res[i], v = y[i];
    out[i] = f32x4{fmaf(l[0], v[0], r[0]), fmaf(l[1], v[1], r[1]), fmaf(l[2], v[2], r[2]), fmaf(l[3], v[3], r[3])};
  }
}
// backward: dy = dx (.) ls ; dls[c] += sum_r dx[r][c] y[r][c]  (row chunks of 64 as in ln_pgrad_kernel)
__global__ void ls_bwd_kernel(const float* __restrict__ dx, const float* __restrict__ y, const float* __restrict__ ls,
                              float* __restrict__ dy, float* __restrict__ dls, int rows, int D) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= D) return;
  const int r0 = blockIdx.y * 64, r1 = r0 + 64 < rows ? r0 + 64 : rows;
  const float l = ls[c];
  float a = 0.f;
  for (int r = r0; r < r1; ++r) {
    const float d = dx[(long)r * D + c];
    a = fmaf(d, y[(long)r * D + c], a);
    dy[(long)r * D + c] = d * l;
  }
  unsafeAtomicAdd(dls + c, a);
}

// the same with float4 columns, eight waves x 8 rows x 2 batches per workgroup (all loads of a batch in flight), the dls partials
// of the waves combined through LDS: 34 -> ~15 us for 8 224 x 768.  D % 4 == 0, 16-byte aligned rows.
__global__ __launch_bounds__(512) void ls_bwd4_kernel(const float* __restrict__ dx, const float* __restrict__ y, const float* __restrict__ ls,
                                                      float* __restrict__ dy, float* __restrict__ dls, int rows, int D) {
  __shared__ f32x4 part[8][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c4 = blockIdx.x * 64 + lane, n4 = D / 4;
  f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
  if (c4 < n4) {
    const f32x4 l = reinterpret_cast<const f32x4*>(ls)[c4];
#pragma unroll
    for (int bt = 0; bt < 2; ++bt) {
      const int r0 = (blockIdx.y * 2 + bt) * 64 + wave * 8;
      f32x4 d[8], v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = r0 + u < rows ? r0 + u : rows - 1;
        d[u] = reinterpret_cast<const f32x4*>(dx + (long)r * D)[c4];
        v[u] = reinterpret_cast<const f32x4*>(y + (long)r * D)[c4];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (r0 + u < rows) {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = fmaf(d[u][j], v[u][j], a[j]);
          reinterpret_cast<f32x4*>(dy + (long)(r0 + u) * D)[c4] = d[u] * l;
        }
    }
  }
  part[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && c4 < n4) {
    f32x4 t = part[0][lane];
#pragma unroll
    for (int w = 1; w < 8; ++w) t += part[w][lane];
#pragma unroll
    for (int j = 0; j < 4; ++j) unsafeAtomicAdd(dls + 4 * c4 + j, t[j]);
  }
}

// DINOv2 input side (base_vit.py:111-122 + HF Dinov2Embeddings): normalised patch matrix [B*P][p*p*3] in the flax
// conv kernel's (dy, dx, c) order, then x[b][0] = cls + pos[0], x[b][1+t] = patch_t W + b + pos[1+t].
__global__ void im2col_f32_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int B, int HW, int p) {
  const int gp = HW / p, K = p * p * 3;
  const long n = (long)B * gp * gp * K;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i % K);
    const long t = i / K;
    const int px = (int)(t % gp), py = (int)((t / gp) % gp), b = (int)(t / ((long)gp * gp));
    const int c = k % 3, dx = (k / 3) % p, dy = k / (3 * p);
    const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f, sd = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
    const uint8_t v = img[(((long)b * HW + py * p + dy) * HW + px * p + dx) * 3 + c];
    out[i] = ((float)v / 255.f - mean) / sd;
  }
}
__global__ void enc_x0_kernel(float* __restrict__ x, const float* __restrict__ cls, const float* __restrict__ pos, int B,
                              int S, int E) {
  const long n = (long)B * S * E;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % E), t = (int)((i / E) % S);
    x[i] = (t == 0 ? cls[c] : x[i]) + pos[(long)t * E + c];
  }
}

// One row of a masked softmax in place, by one wave: n columns at pr, row stride ld >= n; [n, ld) is set to 0 (the row is an A
// operand of float4-staged products).  keep(k): column k takes part, every other column becomes 0.
template <class Keep>
__device__ __forceinline__ void softmax_row(float* pr, int n, int ld, int lane, Keep keep) {
  if (lane < ld - n) pr[n + lane] = 0.f;
  float mx = -3.4e38f;
  for (int k = lane; k < n; k += 64) if (keep(k)) mx = fmaxf(mx, pr[k]);
  for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
  for (int k = lane; k < n; k += 64) {
    const float e = keep(k) ? __expf(pr[k] - mx) : 0.f;
    pr[k] = e;
    sum += e;
  }
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o, 64);
  const float inv = 1.f / sum;
  for (int k = lane; k < n; k += 64) pr[k] *= inv;
}
// masked softmax over the last dim of [nmat][R][Cc] in place.  mode 2: no mask; mode 0: policy mask (rows < R-1 cannot see
// column Cc-1, base_vit.py:209-214); mode 1: context mask (hypernetwork.py:149-181) from attn_mask[b][T].
__global__ void softmax_fwd_kernel(float* __restrict__ p, int nmat, int R, int Cc, int mode,
                                   const int64_t* __restrict__ am, int heads, int ld) {      // ld >= Cc: row stride
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nmat * R) return;
  const int mat = row / R, q = row % R;
  softmax_row(p + (long)row * ld, Cc, ld, lane, [=](int k) {
    if (mode == 2) return true;                                    // DINOv2 encoder: dense attention
    if (mode == 0) return !(q < R - 1 && k == Cc - 1);
    const int T = Cc - 2;
    if (k < T) return am[(long)(mat / heads) * T + k] != 0;
    if (k == T) return true;
    return q == T + 1;
  });
}
// The policy's mask under use_language_token (base_vit.py:209-214) on [nmat][S][S], S = T + P + 1: a language query q < T keeps only
// the language keys k < T, and no query but the last keeps key S - 1 (T == 0 would be mode 0 above).  A kernel of its own so that
// the one above keeps its arguments.
__global__ void softmax_lang_fwd_kernel(float* __restrict__ p, int nmat, int S, int T, int ld) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nmat * S) return;
  const int q = row % S;
  softmax_row(p + (long)row * ld, S, ld, lane, [=](int k) { return q < T ? k < T : (q == S - 1 || k < S - 1); });
}

// The context encoder's mask with NL layer tokens (hypernetwork.py:149-181) on [nmat][S][S], S = T + 1 + NL: a
// language key by the episode's mask, the image key always, a layer key for the layer queries only and never token 0's (key T + 1).
// Every row keeps the image key, so no row is empty.  A kernel of its own, as above.
__global__ void softmax_tokens_fwd_kernel(float* __restrict__ p, int nmat, int S, int T, const int64_t* __restrict__ am, int heads, int ld) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nmat * S) return;
  const int mat = row / S, q = row % S;
  softmax_row(p + (long)row * ld, S, ld, lane, [=](int k) {
    if (k < T) return am[(long)(mat / heads) * T + k] != 0;
    if (k == T) return true;
    return q > T && k != T + 1;
  });
}

// The policy's attention under return_attention_map: CustomMultiHeadDotProductAttention adds the 0 / 1 mask of
// base_vit.py:209-214 to the scaled scores (multi_head_attetion.py:88-98) and masks nothing.  Per row only differences count: the
// action row q = S - 1 (every key + 1) is a plain softmax, a patch row sees key S - 1 one logit below the others.  A kernel of its
// own, as above; p stays [S][ld] dense, so the backward, the four products and attention_aux_kernel read it as they are.
__global__ void softmax_bias_fwd_kernel(float* __restrict__ p, int nmat, int S, int ld) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nmat * S) return;
  float* pr = p + (long)row * ld;
  const float drop = row % S < S - 1 ? 1.f : 0.f;
  const auto score = [=](int k) { return k == S - 1 ? pr[k] - drop : pr[k]; };
  if (lane < ld - S) pr[S + lane] = 0.f;
  float mx = -3.4e38f;
  for (int k = lane; k < S; k += 64) mx = fmaxf(mx, score(k));
  for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
  for (int k = lane; k < S; k += 64) {
    const float e = __expf(score(k) - mx);
    pr[k] = e;
    sum += e;
  }
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o, 64);
  const float inv = 1.f / sum;
  for (int k = lane; k < S; k += 64) pr[k] *= inv;
}

// ds = p * (dp - sum_k dp p), in place on dp
__global__ void softmax_bwd_kernel(const float* __restrict__ p, float* __restrict__ dp, int rows, int Cc, int ld) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* pr = p + (long)row * ld;
  float* dr = dp + (long)row * ld;
  if (lane < ld - Cc) dr[Cc + lane] = 0.f;                 // ds is the A operand of two float4-staged products: zeros behind the row
  float s = 0.f;
  for (int k = lane; k < Cc; k += 64) s += pr[k] * dr[k];
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
  for (int k = lane; k < Cc; k += 64) dr[k] = pr[k] * (dr[k] - s);
}

// ---- DifferentialAttention of the policy (vit_kwargs.use_differential_transformer; differential_transformer.py:99-252) ----
// Per head hh two softmaxed tables A1, A2 (sub-heads 2 hh and 2 hh + 1 of p [nb][2 H][S][ld], rows by softmax_bias_fwd_kernel),
// A = A1 - lambda A2, O = A V, N = O rsqrt(mean_16(O^2) + 1e-5) w (1 - lambda_init).  The kernels below are specialised for what
// accept.h admits: D = 64, H = 4, so a head has 16 values, a part 8, and a wave's lane is a row's feature.  Kernels of their own,
// as above: no existing kernel changes its arguments.
// lambda_1 = exp(sum lambda_q1 lambda_k1) and lambda_2 = exp(sum lambda_q2 lambda_k2) of the episode whose theta row is th, on
// every lane: lanes 0-7 form the first sum's products, lanes 8-15 the second's, one 16-lane reduction serves both
__device__ __forceinline__ void diff_lambdas(const float* __restrict__ th, long lq1, long lk1, long lq2, long lk2, int lane, float& l1, float& l2) {
  float a = 0.f, b = 0.f;
  if (lane < 8) a = th[lq1 + lane] * th[lk1 + lane];
  else if (lane < 16) b = th[lq2 + lane - 8] * th[lk2 + lane - 8];
  for (int o = 8; o; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
  l1 = expf(__shfl(a, 0, 64));
  l2 = expf(__shfl(b, 0, 64));
}
// a[nb][H][S][ld] = A1 - lambda A2 with lambda = lambda_1 - lambda_2 + linit; zeros behind the row (a is the A operand of A V and A^T dO)
__global__ void diff_combine_fwd_kernel(const float* __restrict__ p, float* __restrict__ a, const float* __restrict__ theta, long G,
                                        long lq1, long lk1, long lq2, long lk2, float linit, int nb, int H, int S, int ld) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nb * H * S) return;
  const int mat = row / S, q = row % S;
  float l1, l2;
  diff_lambdas(theta + (long)(mat / H) * G, lq1, lk1, lq2, lk2, lane, l1, l2);
  const float lam = l1 - l2 + linit;
  const float* p1 = p + ((long)(2 * mat) * S + q) * ld;
  const float* p2 = p1 + (long)S * ld;
  float* ar = a + (long)row * ld;
  for (int k = lane; k < ld; k += 64) ar[k] = k < S ? p1[k] - lam * p2[k] : 0.f;
}
// subln (RMSNorm over a head's 16 values, one weight for all heads) and the factor post = 1 - lambda_init: n = o r w post
__global__ void diff_subln_fwd_kernel(const float* __restrict__ o, float* __restrict__ n, const float* __restrict__ theta, long G,
                                      long sw, float post, int rows, int S) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float v = o[(long)row * 64 + lane];
  float s = v * v;
  for (int x = 8; x; x >>= 1) s += __shfl_xor(s, x, 64);
  const float r = rsqrtf(s * (1.f / 16.f) + 1e-5f);
  n[(long)row * 64 + lane] = v * r * theta[(long)(row / S) * G + sw + (lane & 15)] * post;
}
// Its backward, one workgroup of four waves per episode: dn holds dN on entry and dO = r (g w - n mean_16(g w n)) on exit, g = post dN,
// n = o r recomputed; dw[d] = sum_{q, hh} g n in a fixed order (a wave its rows in ascending order, the heads by two shuffles, the
// waves in ascending order), so the episode's dtheta row does not depend on the batch around it
__global__ __launch_bounds__(256) void diff_subln_bwd_kernel(const float* __restrict__ o, float* __restrict__ dn, const float* __restrict__ theta,
                                                             float* __restrict__ dtheta, long G, long sw, float post, int S) {
  __shared__ float red[4][64];
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float w = theta[(long)b * G + sw + (lane & 15)];
  float acc = 0.f;
  for (int q = wave; q < S; q += 4) {
    const long i = ((long)b * S + q) * 64 + lane;
    const float v = o[i];
    float s = v * v;
    for (int x = 8; x; x >>= 1) s += __shfl_xor(s, x, 64);
    const float r = rsqrtf(s * (1.f / 16.f) + 1e-5f), nn = v * r, g = post * dn[i], gw = g * w;
    acc = fmaf(g, nn, acc);
    float m = gw * nn;
    for (int x = 8; x; x >>= 1) m += __shfl_xor(m, x, 64);
    dn[i] = r * (gw - nn * (m * (1.f / 16.f)));
  }
  acc += __shfl_xor(acc, 16, 64);
  acc += __shfl_xor(acc, 32, 64);
  red[wave][lane] = acc;
  __syncthreads();
  if (threadIdx.x < 16) dtheta[(long)b * G + sw + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}
// Both softmax backwards of a head's row from ONE dp row (dA1 = dp, dA2 = - lambda dp): ds1 = A1 (dp - t1), ds2 = - lambda A2 (dp - t2),
// t_c = sum_k dp A_c, into ds [nb][2 H][S][ld] next to the tables (zeros behind the rows: ds is the A operand of dq and dk); t2 [nb][H][S]
// is kept for d lambda = - sum t2
__global__ void diff_softmax_bwd_kernel(const float* __restrict__ p, const float* __restrict__ dp, float* __restrict__ ds, float* __restrict__ t2,
                                        const float* __restrict__ theta, long G, long lq1, long lk1, long lq2, long lk2, float linit,
                                        int nb, int H, int S, int ld) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nb * H * S) return;
  const int mat = row / S, q = row % S;
  float l1, l2;
  diff_lambdas(theta + (long)(mat / H) * G, lq1, lk1, lq2, lk2, lane, l1, l2);
  const float lam = l1 - l2 + linit;
  const long o1 = ((long)(2 * mat) * S + q) * ld, o2 = o1 + (long)S * ld;
  const float* p1 = p + o1;
  const float* p2 = p + o2;
  const float* d = dp + (long)row * ld;
  float* s1 = ds + o1;
  float* s2 = ds + o2;
  if (lane < ld - S) s1[S + lane] = s2[S + lane] = 0.f;
  float a = 0.f, b = 0.f;
  for (int k = lane; k < S; k += 64) { a = fmaf(d[k], p1[k], a); b = fmaf(d[k], p2[k], b); }
  for (int x = 32; x; x >>= 1) { a += __shfl_xor(a, x, 64); b += __shfl_xor(b, x, 64); }
  for (int k = lane; k < S; k += 64) {
    s1[k] = p1[k] * (d[k] - a);
    s2[k] = -lam * p2[k] * (d[k] - b);
  }
  if (lane == 0) t2[row] = b;
}
// d lambda = - sum_{hh, q} t2 of the episode (a lane its entries in ascending order, the lanes by xor-shuffle: a fixed order), then
// d lambda_q1 = d lambda lambda_1 lambda_k1, d lambda_k1 = d lambda lambda_1 lambda_q1, d lambda_q2 = - d lambda lambda_2 lambda_k2,
// d lambda_k2 = - d lambda lambda_2 lambda_q2 into the episode's dtheta row.  One wave per episode.
__global__ void diff_lambda_bwd_kernel(const float* __restrict__ t2, const float* __restrict__ theta, float* __restrict__ dtheta, long G,
                                       long lq1, long lk1, long lq2, long lk2, int n) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* th = theta + (long)b * G;
  float* dth = dtheta + (long)b * G;
  float s = 0.f;
  for (int i = lane; i < n; i += 64) s += t2[(long)b * n + i];
  for (int x = 32; x; x >>= 1) s += __shfl_xor(s, x, 64);
  float l1, l2;
  diff_lambdas(th, lq1, lk1, lq2, lk2, lane, l1, l2);
  const float d1 = -s * l1, d2 = s * l2;
  if (lane < 8) {
    dth[lq1 + lane] = d1 * th[lk1 + lane];
    dth[lk1 + lane] = d1 * th[lq1 + lane];
    dth[lq2 + lane] = d2 * th[lk2 + lane];
    dth[lk2 + lane] = d2 * th[lq2 + lane];
  }
}

// The per-episode reductions of a DifferentialAttention policy's backward without atomics, so that the WHOLE dtheta row of a sample is
// the same bits in any batch and in every run (the forms above add row chunks with atomics in the order the chunks finish).  One
// workgroup of four waves per (64 columns, episode): a wave its rows w, w + 4, .. in ascending order, the waves in ascending order.
// out[b * ostride + n] += sum_{r < rows_used} x[b][r][n]; one writer per element
__global__ __launch_bounds__(256) void colsum_episode_kernel(const float* __restrict__ x, float* __restrict__ out, long ostride, int R,
                                                             int rows_used, int N) {
  __shared__ float red[4][64];
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (n < N)
    for (int r = wave; r < rows_used; r += 4) s += x[((long)b * R + r) * N + n];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && n < N) out[(long)b * ostride + n] += ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}
// dscale[b][c] += sum_r dy xhat, dbias[b][c] += sum_r dy over the S rows of episode b (ln_bwd_kernel then runs without its atomics)
__global__ __launch_bounds__(256) void ln_pgrad_episode_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, float* __restrict__ dscale,
                                                               float* __restrict__ dbias, long pstride, int S, int D) {
  __shared__ float red[2][4][64];
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = blockIdx.x * 64 + lane;
  float sa = 0.f, sb = 0.f;
  if (c < D)
    for (int r = wave; r < S; r += 4) {
      const long row = (long)b * S + r;
      const float d = dy[row * D + c];
      sa = fmaf(d, (x[row * D + c] - mean[row]) * rstd[row], sa);
      sb += d;
    }
  red[0][wave][lane] = sa;
  red[1][wave][lane] = sb;
  __syncthreads();
  if (wave == 0 && c < D) {
    dscale[(long)b * pstride + c] += ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
    dbias[(long)b * pstride + c] += ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
  }
}

__device__ __forceinline__ float dgelu_tanh(float x) {
  const float k0 = 0.7978845608028654f, k1 = 0.044715f;
  const float u = k0 * (x + k1 * x * x * x), t = tanhf(u);
  return 0.5f * (1.f + t) + 0.5f * x * (1.f - t * t) * k0 * (1.f + 3.f * k1 * x * x);
}
// erf form (torch nn.GELU(), the DINOv2 MLP): exact erff here, the training path is f32 end to end
__device__ __forceinline__ float gelu_erf_exact(float x) { return 0.5f * x * (1.f + erff(x * 0.7071067811865476f)); }
__device__ __forceinline__ float dgelu_erf(float x) {
  return 0.5f * (1.f + erff(x * 0.7071067811865476f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}
__global__ void gelu_fwd_kernel(const float* __restrict__ u, float* __restrict__ g, long n, int erf_form) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    g[i] = erf_form ? gelu_erf_exact(u[i]) : gelu_tanh(u[i]);
}
__global__ void gelu_bwd_kernel(const float* __restrict__ u, float* __restrict__ dg, long n, int erf_form) {   // dg -> du in place
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    dg[i] *= erf_form ? dgelu_erf(u[i]) : dgelu_tanh(u[i]);
}

// ---- the reference's train=True noise (noise.h; hvla_train_noise) ---------------------------------------------
// A thread owns one Philox block: four consecutive elements of a sample, one 16-byte access per operand.  Samples are blockIdx.y;
// n4 = the per-sample element count / 4 (every site's width is a multiple of 4 under accept.h), rows 16-byte aligned.
// out = [res +] drop(x): x / keep_prob where kept, 0 elsewhere.  out may be x (in place); res == null: no residual.
__global__ void dropout_fwd_kernel(float* out, const float* res, const float* x, int n4, NoiseKey key, uint32_t thr, float keep_prob) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (i >= n4) return;
  const long o = (long)b * n4 + i;
  const PhiloxWords w = noise_block(key, b, (uint32_t)i);
  const f32x4 v = reinterpret_cast<const f32x4*>(x)[o];
  f32x4 y = res ? reinterpret_cast<const f32x4*>(res)[o] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] += dropout_keep(w.w[j], thr) ? v[j] / keep_prob : 0.f;
  reinterpret_cast<f32x4*>(out)[o] = y;
}
// dx = dy (.) multiplier with the mask regenerated; dx == dy is the in-place form, dx != dy keeps dy (the residual's gradient)
__global__ void dropout_bwd_kernel(float* dx, const float* dy, int n4, NoiseKey key, uint32_t thr, float keep_prob) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (i >= n4) return;
  const long o = (long)b * n4 + i;
  const PhiloxWords w = noise_block(key, b, (uint32_t)i);
  f32x4 v = reinterpret_cast<const f32x4*>(dy)[o];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = dropout_keep(w.w[j], thr) ? v[j] / keep_prob : 0.f;
  reinterpret_cast<f32x4*>(dx)[o] = v;
}
// dst[b] = src[b] + sigma z over [n4 * 4] elements per sample, sample strides in elements (a frozen encoder's tokens into their
// copy; a trained encoder's patch rows in place behind every sample's CLS row)
__global__ void token_noise_kernel(float* dst, long dstride, const float* src, long sstride, int n4, NoiseKey key, float sigma) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (i >= n4) return;
  const PhiloxWords w = noise_block(key, b, (uint32_t)i);
  f32x4 v = reinterpret_cast<const f32x4*>(src + (long)b * sstride)[i];
  float z[4];
  noise_box_muller(w.w[0], w.w[1], z[0], z[1]);
  noise_box_muller(w.w[2], w.w[3], z[2], z[3]);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = fmaf(sigma, z[j], v[j]);
  reinterpret_cast<f32x4*>(dst + (long)b * dstride)[i] = v;
}
// hvla_train_noise_probe (test instrumentation): element i's multiplier or normal, one element per thread, any n
__global__ void noise_probe_kernel(float* __restrict__ out, long n, NoiseKey key, uint32_t thr, float keep_prob, int normal) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PhiloxWords w = noise_block(key, 0, (uint32_t)(i >> 2));
  const int j = (int)(i & 3);
  if (normal) {
    float z0, z1;
    noise_box_muller(w.w[j & 2], w.w[(j & 2) + 1], z0, z1);
    out[i] = j & 1 ? z1 : z0;
  } else {
    out[i] = dropout_keep(w.w[j], thr) ? 1.f / keep_prob : 0.f;
  }
}

// column sums: out[b * ostride + n] += sum_{r < rows_used} x[b][r][n]  (bias gradients).  blockIdx.z splits the rows
// into chunks of 64 that are reduced with one atomic each, so long shared-parameter reductions stay parallel.
__global__ void colsum_kernel(const float* __restrict__ x, float* __restrict__ out, long ostride, int R, int rows_used,
                              int N, int nb) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (n >= N || b >= nb) return;
  const int r0 = blockIdx.z * 64, r1 = r0 + 64 < rows_used ? r0 + 64 : rows_used;
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += x[((long)b * R + r) * N + n];
  unsafeAtomicAdd(out + (long)b * ostride + n, s);
}

// the same for 16-byte aligned rows with N % 4 == 0: a thread owns 4 columns (1 KiB per wave and row), 32 rows per chunk,
// eight row loads in flight
__global__ void colsum4_kernel(const float* __restrict__ x, float* __restrict__ out, long ostride, int R, int rows_used,
                               int N, int nb) {
  const int n = (blockIdx.x * blockDim.x + threadIdx.x) * 4, b = blockIdx.y;
  if (n >= N || b >= nb) return;
  const int r0 = blockIdx.z * 32, r1 = r0 + 32 < rows_used ? r0 + 32 : rows_used;
  const float* p = x + ((long)b * R + r0) * N + n;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  int r = r0;
  for (; r + 8 <= r1; r += 8, p += 8L * N) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4*>(p + (long)u * N);
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; r < r1; ++r, p += N) s += *reinterpret_cast<const f32x4*>(p);
  float* o = out + (long)b * ostride + n;
#pragma unroll
  for (int c = 0; c < 4; ++c) unsafeAtomicAdd(o + c, s[c]);
}

// The long shared-parameter reductions of the encoder (8 224 rows x 768 / 3 072 columns): the two kernels above have 800-1 500
// waves of 8 KB in flight for 25-100 MB (17-23 us for the narrow matrices: 1.5 TB/s).  Here a workgroup is eight waves x 8 rows
// x 2 batches, every row load of a batch in flight at once, the eight partial rows combined through LDS, one atomic per column
// and workgroup (four waves x 8 rows x 1 batch, twice the atomics of before, was SLOWER than the old kernels: 37 us).
constexpr int CSB_WAVES = 8, CSB_BATCH = 2;          // 128 rows per workgroup: half the atomics of the 64-row chunks above
__global__ __launch_bounds__(CSB_WAVES * 64) void colsum4b_kernel(const float* __restrict__ x, float* __restrict__ out, int rows, int N) {
  __shared__ f32x4 part[CSB_WAVES][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = (blockIdx.x * 64 + lane) * 4;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (n < N) {
#pragma unroll
    for (int bt = 0; bt < CSB_BATCH; ++bt) {
      const int r0 = (blockIdx.z * CSB_BATCH + bt) * (CSB_WAVES * 8) + wave * 8;
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = r0 + u < rows ? r0 + u : rows - 1;
        v[u] = *reinterpret_cast<const f32x4*>(x + (long)r * N + n);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (r0 + u < rows) s += v[u];
    }
  }
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && n < N) {
    f32x4 t = part[0][lane];
#pragma unroll
    for (int w = 1; w < CSB_WAVES; ++w) t += part[w][lane];
#pragma unroll
    for (int c = 0; c < 4; ++c) unsafeAtomicAdd(out + n + c, t[c]);
  }
}

// x0 assembly: rows < S - 1 already hold the projections (tokens.Wp + bp, under use_language_token tok.Wl + bl in front of them);
// row S - 1 = 0; += pos  (base_vit.py:159-166,182-204)
__global__ void x0_finish_kernel(float* __restrict__ x, const float* __restrict__ pos, long pstride, int S, int D, int nb) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)nb * S * D) return;
  const int c = (int)(i % D), t = (int)((i / D) % S), b = (int)(i / ((long)S * D));
  const float base = t == S - 1 ? 0.f : x[i];
  x[i] = base + pos[(long)b * pstride + (long)t * D + c];
}
__global__ void add_kernel(float* __restrict__ dst, const float* __restrict__ src, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] += src[i];
}
// dst[b * dstride + i] += src[b * n + i]
__global__ void add_strided_kernel(float* __restrict__ dst, long dstride, const float* __restrict__ src, long n, int nb) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)nb * n) return;
  dst[(i / n) * dstride + (i % n)] += src[i];
}

// mix head + loss, forward and backward for the action-token row (one thread block of 64 per episode).
// e = LN_f(x[S-1]); z = e.Wc + bc (A values), l = e.Wd + bd (Hz); cont = tanh(z / ts) * ma.
// Writes loss[b]; if dxrow != null also d/d(theta head leaves) and d/dx[S-1] for loss_total = mean_b loss[b].
struct HeadP {
  const float* x; long xstride;             // [B][S][D], row S-1 used
  const float* theta; float* dtheta; long G;
  int o_wc, o_bc, o_wd, o_bd, o_ns, o_nb;   // leaf offsets in theta
  const float* target; const uint8_t* tmask; const uint8_t* amask;
  float* loss; float* dxrow;                // [B][D]
  float* actions; float* logits;            // optional outputs
  int B, S, D, Hz, ad; float tanh_scale, max_action;
  int clip_target;                          // action_heads.py:499-500
};
__global__ void head_loss_kernel(HeadP p) {
  const int b = blockIdx.x, lane = threadIdx.x;            // 64 lanes, D == 64
  __shared__ float e[64], xh[64], dz[32], sh[4];
  const float* xr = p.x + (long)b * p.xstride + (long)(p.S - 1) * p.D;
  const float* th = p.theta + (long)b * p.G;
  float v = xr[lane], s = v, q = v * v;
  for (int o = 32; o; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
  const float m = s / 64.f, var = fmaxf(0.f, q / 64.f - m * m), r = rsqrtf(var + 1e-6f);
  xh[lane] = (v - m) * r;
  e[lane] = xh[lane] * th[p.o_ns + lane] + th[p.o_nb + lane];
  __syncthreads();
  const int A = p.Hz * (p.ad - 1), NO = A + p.Hz;
  float z = 0.f;
  if (lane < NO) {
    const float* W = lane < A ? th + p.o_wc : th + p.o_wd;
    const int n = lane < A ? lane : lane - A, ld = lane < A ? A : p.Hz;
    for (int k = 0; k < 64; ++k) z = fmaf(e[k], W[k * ld + n], z);
    z += lane < A ? th[p.o_bc + n] : th[p.o_bd + n];
  }
  // ---- loss terms
  const bool tm = p.tmask[b] != 0;
  float cs = 0.f, cm = 0.f, ds = 0.f, dm = 0.f, dzl = 0.f, mk = 0.f, pred = 0.f, tgt = 0.f;
  if (lane < NO) {
    int h, a;
    if (lane < A) { h = lane / (p.ad - 1); a = lane % (p.ad - 1); } else { h = lane - A; a = p.ad - 1; }
    const long o = ((long)b * p.Hz + h) * p.ad + a;
    mk = (tm && p.amask[o]) ? 1.f : 0.f;
    tgt = p.clip_target ? fminf(fmaxf(p.target[o], -p.max_action), p.max_action) : p.target[o];
    if (lane < A) {
      pred = tanhf(z / p.tanh_scale) * p.max_action;
      cs = (pred - tgt) * (pred - tgt) * mk; cm = mk;
      if (p.actions) p.actions[o] = pred;
    } else {
      const float sp = log1pf(expf(-fabsf(z)));
      ds = (tgt * (fmaxf(-z, 0.f) + sp) + (1.f - tgt) * (fmaxf(z, 0.f) + sp)) * mk; dm = mk;
      if (p.actions) p.actions[o] = z >= 0.f ? 1.f : 0.f;
      if (p.logits) p.logits[(long)b * p.Hz + h] = z;
    }
  }
  for (int o = 32; o; o >>= 1) {
    cs += __shfl_xor(cs, o, 64); cm += __shfl_xor(cm, o, 64); ds += __shfl_xor(ds, o, 64); dm += __shfl_xor(dm, o, 64);
  }
  const float nc = (float)A, nd = (float)p.Hz;
  const float dc = fmaxf(cm / nc, 1e-5f), dd = fmaxf(dm / nd, 1e-5f);
  if (lane == 0) p.loss[b] = (cs / nc) / dc * (float)(p.ad - 1) + (ds / nd) / dd;
  if (!p.dxrow) return;
  // ---- backward (d/dz of loss[b] / B)
  const float gb = 1.f / (float)p.B;
  if (lane < A) {
    const float t = pred / p.max_action;                                   // tanh(z / ts)
    dzl = gb * (float)(p.ad - 1) / (nc * dc) * 2.f * (pred - tgt) * mk * p.max_action * (1.f - t * t) / p.tanh_scale;
  } else if (lane < NO) {
    const float sg = 1.f / (1.f + expf(-z));
    dzl = gb / (nd * dd) * (sg - tgt) * mk;
  }
  if (lane < 32) dz[lane] = lane < NO ? dzl : 0.f;
  __syncthreads();
  float* dth = p.dtheta + (long)b * p.G;
  if (lane < NO) {                                                           // bias grads
    if (lane < A) dth[p.o_bc + lane] += dzl; else dth[p.o_bd + lane - A] += dzl;
  }
  // kernel grads dW[k][n] = e[k] dz[n]; de[k] = sum_n W[k][n] dz[n]   (lane = k)
  float de = 0.f;
  for (int n = 0; n < A; ++n) { dth[p.o_wc + lane * A + n] += e[lane] * dz[n]; de = fmaf(th[p.o_wc + lane * A + n], dz[n], de); }
  for (int n = 0; n < p.Hz; ++n) { dth[p.o_wd + lane * p.Hz + n] += e[lane] * dz[A + n]; de = fmaf(th[p.o_wd + lane * p.Hz + n], dz[A + n], de); }
  dth[p.o_ns + lane] += de * xh[lane];
  dth[p.o_nb + lane] += de;
  const float dxh = de * th[p.o_ns + lane];
  float s1 = dxh, s2 = dxh * xh[lane];
  for (int o = 32; o; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
  p.dxrow[(long)b * p.D + lane] = r * (dxh - s1 / 64.f - xh[lane] * s2 / 64.f);
}

// The two attention terms of the reference's sample_loss_fn (scripts/train.py:348-373; hvla_train_attention_losses), on the action
// token's softmax row p[h][k] (query S-1, all S keys: the row is unmasked) of the LAST policy layer, one workgroup per episode:
//   ent = 1/H sum_h -sum_{k<S} p log(p + 1e-8);  m[k] = 1/H sum_h p[h][k];  align = 1/P sum_{k<P} (m[k] - ref[k])^2
// dp == null (LOSS): loss[b] += w_ent ent + w_align align, behind head_loss_kernel; the two terms also go to ent[] / align[].
// dp != null (GRAD): row S-1 of dp[b][h] += gscale d(w_ent ent + w_align align)/dp[h][k], between dp = do v^T and softmax_bwd_kernel;
// recomputed from p, no workspace.  A thread owns keys k, k + 256, ..: the sums run in a fixed order (lanes by xor-shuffle, waves in
// ascending order by one thread), no atomics -- the forward loss stays bit-reproducible.
struct AuxP {
  const float* p; float* dp;                // [B][H][S][Sp]
  long sb, sh;                              // episode and head stride of both
  int S, Sp, H, P;
  float w_ent, w_align;
  const float* ref;                         // [B][P], or null (then w_align == 0)
  float* loss; float* ent; float* align;    // [B]; ent / align nullable
  float gscale;                             // the seed's factor of d mean_b loss_b: 1 / B (head_loss_kernel's gb)
};
__global__ __launch_bounds__(256) void attention_aux_kernel(AuxP a) {
  __shared__ float red[2][4];
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long o = (long)b * a.sb + (long)(a.S - 1) * a.Sp;
  const float* row = a.p + o;
  const float* r = a.ref ? a.ref + (long)b * a.P : nullptr;
  const float invH = 1.f / (float)a.H, eps = 1e-8f;
  const float ge = a.gscale * a.w_ent * invH, ga = a.gscale * a.w_align * 2.f * invH / (float)a.P;
  float es = 0.f, as = 0.f;
  for (int k = threadIdx.x; k < a.S; k += 256) {
    float m = 0.f, e = 0.f;
    for (int h = 0; h < a.H; ++h) {
      const float pv = row[h * a.sh + k];
      m += pv;
      e -= pv * logf(pv + eps);
    }
    const float d = r && k < a.P ? m * invH - r[k] : 0.f;       // the action key counts for the entropy only
    es += e;
    as += d * d;
    if (a.dp) {
      float* drow = a.dp + o;
      for (int h = 0; h < a.H; ++h) {
        const float pv = row[h * a.sh + k];
        drow[h * a.sh + k] += ge * (-logf(pv + eps) - pv / (pv + eps)) + ga * d;
      }
    }
  }
  if (a.dp) return;
  for (int s = 32; s; s >>= 1) { es += __shfl_xor(es, s, 64); as += __shfl_xor(as, s, 64); }
  if (lane == 0) { red[0][wave] = es; red[1][wave] = as; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float ent = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) * invH;
    const float al = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) / (float)a.P;
    a.loss[b] += a.w_ent * ent + a.w_align * al;
    if (a.ent) a.ent[b] = ent;
    if (a.align && r) a.align[b] = al;
  }
}

// context-token assembly with NL layer tokens, Sc = T + 1 + NL rows per episode: rows t < T += pos_tok[t]; row T += pos_img; rows
// T + 1 + j = pos_layer[j] (hypernetwork.py:112-145).  share_layer_index=True is NL = 1; the _tokens kernels take NL.
__device__ __forceinline__ void ctx_rows_fwd(float* __restrict__ x, const float* __restrict__ pos_tok, const float* __restrict__ pos_img,
                                             const float* __restrict__ pos_layer, int B, int T, int NL, int C) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int Sc = T + 1 + NL;
  if (i >= (long)B * Sc * C) return;
  const int c = (int)(i % C), t = (int)((i / C) % Sc);
  if (t < T) x[i] += pos_tok[(long)t * C + c];
  else if (t == T) x[i] += pos_img[c];
  else x[i] = pos_layer[(long)(t - T - 1) * C + c];
}
// dpos_layer[j] = sum_b dx[b][T + 1 + j]
__device__ __forceinline__ void ctx_rows_bwd(const float* __restrict__ dx, float* __restrict__ dpos_tok, float* __restrict__ dpos_img,
                                             float* __restrict__ dpos_layer, float* __restrict__ db_tok, float* __restrict__ db_img,
                                             int B, int T, int NL, int C) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int Sc = T + 1 + NL;
  if (i >= (long)B * Sc * C) return;
  const int c = (int)(i % C), t = (int)((i / C) % Sc);
  const float v = dx[i];
  if (t < T) { unsafeAtomicAdd(dpos_tok + (long)t * C + c, v); unsafeAtomicAdd(db_tok + c, v); }
  else if (t == T) { unsafeAtomicAdd(dpos_img + c, v); unsafeAtomicAdd(db_img + c, v); }
  else unsafeAtomicAdd(dpos_layer + (long)(t - T - 1) * C + c, v);
}
// ctx[row] = (LN(xr) * scale + bias) * post   (encoder_norm on a layer-token row, hypernetwork.py:188-192); one wave per row of
// ctx / xhat [rows][C] and mean / rstd [rows], xr the row's place in the context stream
__device__ __forceinline__ void ctx_final_fwd_row(const float* __restrict__ xr, int row, float* __restrict__ xhat, float* __restrict__ mean,
                                                  float* __restrict__ rstd, const float* __restrict__ scale, const float* __restrict__ bias,
                                                  float* __restrict__ ctx, int C, float post) {
  const int lane = threadIdx.x & 63;
  float s = 0.f, q = 0.f;
  for (int c = lane; c < C; c += 64) { s += xr[c]; q += xr[c] * xr[c]; }
  for (int o = 32; o; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
  const float m = s / C, var = fmaxf(0.f, q / C - m * m), r = rsqrtf(var + 1e-6f);
  for (int c = lane; c < C; c += 64) {
    const float xh = (xr[c] - m) * r;
    xhat[(long)row * C + c] = xh;
    ctx[(long)row * C + c] = (xh * scale[c] + bias[c]) * post;
  }
  if (lane == 0) { mean[row] = m; rstd[row] = r; }
}
__device__ __forceinline__ void ctx_final_bwd_row(const float* __restrict__ xr, float* __restrict__ dxr, int row, const float* __restrict__ dctx,
                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                  const float* __restrict__ scale, float* __restrict__ dscale, float* __restrict__ dbias,
                                                  int C, float post) {
  const int lane = threadIdx.x & 63;
  const float m = mean[row], r = rstd[row];
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float xh = (xr[c] - m) * r, dy = dctx[(long)row * C + c] * post, dxh = dy * scale[c];
    s1 += dxh; s2 += dxh * xh;
  }
  for (int o = 32; o; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
  for (int c = lane; c < C; c += 64) {
    const float xh = (xr[c] - m) * r, dy = dctx[(long)row * C + c] * post, dxh = dy * scale[c];
    dxr[c] += r * (dxh - s1 / C - xh * s2 / C);
    unsafeAtomicAdd(dscale + c, dy * xh);
    unsafeAtomicAdd(dbias + c, dy);
  }
}

__global__ void ctx_rows_kernel(float* __restrict__ x, const float* __restrict__ pos_tok, const float* __restrict__ pos_img,
                                const float* __restrict__ pos_layer, int B, int T, int C) {
  ctx_rows_fwd(x, pos_tok, pos_img, pos_layer, B, T, 1, C);
}
__global__ void ctx_rows_bwd_kernel(const float* __restrict__ dx, float* __restrict__ dpos_tok, float* __restrict__ dpos_img,
                                    float* __restrict__ dpos_layer, float* __restrict__ db_tok, float* __restrict__ db_img,
                                    int B, int T, int C) {
  ctx_rows_bwd(dx, dpos_tok, dpos_img, dpos_layer, db_tok, db_img, B, T, 1, C);
}
// one layer token: x / dx point at episode 0's last row, xstride from one episode's to the next's
__global__ void ctx_final_fwd_kernel(const float* __restrict__ x, long xstride, float* __restrict__ xhat,
                                     float* __restrict__ mean, float* __restrict__ rstd, const float* __restrict__ scale,
                                     const float* __restrict__ bias, float* __restrict__ ctx, int B, int C, float post) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  ctx_final_fwd_row(x + (long)b * xstride, b, xhat, mean, rstd, scale, bias, ctx, C, post);
}
__global__ void ctx_final_bwd_kernel(const float* __restrict__ x, long xstride, const float* __restrict__ dctx,
                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                     const float* __restrict__ scale, float* __restrict__ dx, float* __restrict__ dscale,
                                     float* __restrict__ dbias, int B, int C, float post) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  ctx_final_bwd_row(x + (long)b * xstride, dx + (long)b * xstride, b, dctx, mean, rstd, scale, dscale, dbias, C, post);
}

// NL layer tokens: x / dx are the whole stream [B][Sc][C], row = b NL + j of ctx / xhat / dctx [B][NL][C] is stream row T + 1 + j of episode b
__global__ void ctx_rows_tokens_kernel(float* __restrict__ x, const float* __restrict__ pos_tok, const float* __restrict__ pos_img,
                                       const float* __restrict__ pos_layer, int B, int T, int NL, int C) {
  ctx_rows_fwd(x, pos_tok, pos_img, pos_layer, B, T, NL, C);
}
__global__ void ctx_rows_tokens_bwd_kernel(const float* __restrict__ dx, float* __restrict__ dpos_tok, float* __restrict__ dpos_img,
                                           float* __restrict__ dpos_layer, float* __restrict__ db_tok, float* __restrict__ db_img,
                                           int B, int T, int NL, int C) {
  ctx_rows_bwd(dx, dpos_tok, dpos_img, dpos_layer, db_tok, db_img, B, T, NL, C);
}
__global__ void ctx_final_tokens_fwd_kernel(const float* __restrict__ x, int Sc, int NL, float* __restrict__ xhat,
                                            float* __restrict__ mean, float* __restrict__ rstd, const float* __restrict__ scale,
                                            const float* __restrict__ bias, float* __restrict__ ctx, int rows, int C, float post) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  ctx_final_fwd_row(x + ((long)(row / NL) * Sc + (Sc - NL) + row % NL) * C, row, xhat, mean, rstd, scale, bias, ctx, C, post);
}
__global__ void ctx_final_tokens_bwd_kernel(const float* __restrict__ x, int Sc, int NL, const float* __restrict__ dctx,
                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                            const float* __restrict__ scale, float* __restrict__ dx, float* __restrict__ dscale,
                                            float* __restrict__ dbias, int rows, int C, float post) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long xo = ((long)(row / NL) * Sc + (Sc - NL) + row % NL) * C;
  ctx_final_bwd_row(x + xo, dx + xo, row, dctx, mean, rstd, scale, dscale, dbias, C, post);
}
// db_h[hcols] += sum_b dtheta[b, run] for every run in one launch (the grouped form of colsum_kernel): a workgroup is one 64-column
// tile of the forward's table (train_layout.h group_tiles kind 0: c = theta column origin, bias = head column origin), blockIdx.z a
// chunk of 64 rows, one atomic per (chunk, column) -- with shared heads the L blocks' sums meet in one element
__global__ void colsum_groups_kernel(const float* __restrict__ x, long ld, float* __restrict__ out, const BGTile* __restrict__ tiles, int rows) {
  const BGTile t = tiles[blockIdx.x];
  const int n = t.n0 + threadIdx.x;
  if (n >= t.N) return;
  const int r0 = blockIdx.z * 64, r1 = r0 + 64 < rows ? r0 + 64 : rows;
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += x[(long)r * ld + t.c + n];
  unsafeAtomicAdd(out + t.bias + n, s);
}

// ---- optimizer ------------------------------------------------------------------------------------
// Under create_optimizer(frozen_keys=...) (octo/utils/train_utils.py:242-292: multi_transform{trainable: the whole chain, frozen:
// set_to_zero} by fnmatch over the leaf names; the host resolves the names into `frozen` [n], hvla_train_frozen) the clip sits inside
// the trainable transform, so the global norm is taken over trainable elements only; a frozen element of params / mu / nu / ema is
// neither loaded nor stored, and neither are its g and p0: the mask byte is all it costs.
// The kernels keep one argument list each (tests/native/train_step_trace.txt pins them) and their grid-stride loops (the block and
// grid sizes read inside a kernel compile to the short form); the arithmetic is stated once, in the functions they call.
template <bool FROZEN>
__device__ __forceinline__ void sqsum_sweep(const float* __restrict__ g, const uint8_t* __restrict__ frozen, long n, float* __restrict__ out,
                                            long i0, long step) {
  float s = 0.f;
  for (long i = i0; i < n; i += step) {
    if constexpr (FROZEN) { if (frozen[i]) continue; }
    const float gi = g[i];
    s += gi * gi;
  }
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(out, s);
}
__global__ void sqsum_kernel(const float* __restrict__ g, long n, float* __restrict__ out) {
  sqsum_sweep<false>(g, nullptr, n, out, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}
__global__ void sqsum_frozen_kernel(const float* __restrict__ g, const uint8_t* __restrict__ frozen, long n, float* __restrict__ out) {
  sqsum_sweep<true>(g, frozen, n, out, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}
// clip-by-global-norm's factor from the squared norm in sq[0]
__device__ __forceinline__ float clip_scale(const float* __restrict__ sq, float clip) {
  const float norm = sqrtf(sq[0]);
  return norm < clip ? 1.f : clip / norm;
}
// MultiSteps micro-step (octo/utils/train_utils.py:420-426: chain(clip_by_global_norm, MultiSteps(adamw))): the clipped
// gradient of this micro-batch goes into the running mean, acc += clip(g) / k
__global__ void accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long n, const float* __restrict__ sq,
                                  float clip, float inv_k) {
  const float sc = clip_scale(sq, clip) * inv_k;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) acc[i] = fmaf(g[i], sc, acc[i]);
}
// clip-by-global-norm -> AdamW (mu stored bf16, optax mu_dtype) -> EMA of element i, sc = clip_scale().  Weight decay is decoupled:
//   SHARED = false  the hypernetwork's group: + wd p where mask[i] != 0 (the host builds the mask of the selected
//                   weight_decay_strategy); p0 is not read
//   SHARED = true   optimizer group "shared" (train_utils.py:414-419 + scripts/train.py:465-471): AdamW at base_lr, decay base_wd on
//                   the masked leaves (every image_encoder leaf under weight_decay_strategy v5, the *kernel* leaves under v1), and -- as
//                   the reference does for every shared leaf when base_wd > 0 -- the update gets + base_lr * base_wd * p0 (the pull
//                   back towards the pretrained weights p0); both only under wd > 0
template <bool SHARED>
__device__ __forceinline__ void adamw_update(long i, float* __restrict__ p, const float* __restrict__ g, __bf16* __restrict__ mu,
                                             float* __restrict__ nu, float* __restrict__ ema, float sc, float lr, float b1, float b2,
                                             float eps, float wd, const uint8_t* __restrict__ mask, const float* __restrict__ p0,
                                             float bc1, float bc2, float ema_decay) {
  const float gi = g[i] * sc;
  const float m = b1 * (float)mu[i] + (1.f - b1) * gi;
  const float v = b2 * nu[i] + (1.f - b2) * gi * gi;
  mu[i] = (__bf16)m;
  nu[i] = v;
  float upd = (m / bc1) / (sqrtf(v / bc2) + eps);
  if constexpr (SHARED) {
    if (wd > 0.f) {
      if (mask && mask[i]) upd += wd * p[i];
      if (p0) upd -= wd * p0[i];
    }
  } else {
    if (mask && mask[i]) upd += wd * p[i];
  }
  const float pn = p[i] - lr * upd;
  p[i] = pn;
  if (ema) ema[i] = ema_decay * ema[i] + (1.f - ema_decay) * pn;
}
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, __bf16* __restrict__ mu,
                             float* __restrict__ nu, float* __restrict__ ema, long n, const float* __restrict__ sq,
                             float clip, float lr, float b1, float b2, float eps, float wd,
                             const uint8_t* __restrict__ mask, float bc1, float bc2, float ema_decay) {
  const float sc = clip_scale(sq, clip);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    adamw_update<false>(i, p, g, mu, nu, ema, sc, lr, b1, b2, eps, wd, mask, nullptr, bc1, bc2, ema_decay);
}
__global__ void adamw_shared_kernel(float* __restrict__ p, const float* __restrict__ g, __bf16* __restrict__ mu,
                                    float* __restrict__ nu, float* __restrict__ ema, long n, const float* __restrict__ sq,
                                    float clip, float lr, float b1, float b2, float eps, float wd,
                                    const uint8_t* __restrict__ mask, const float* __restrict__ p0, float bc1, float bc2,
                                    float ema_decay) {
  const float sc = clip_scale(sq, clip);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    adamw_update<true>(i, p, g, mu, nu, ema, sc, lr, b1, b2, eps, wd, mask, p0, bc1, bc2, ema_decay);
}
template <bool SHARED>
__global__ void adamw_frozen_kernel(float* __restrict__ p, const float* __restrict__ g, __bf16* __restrict__ mu,
                                    float* __restrict__ nu, float* __restrict__ ema, const uint8_t* __restrict__ frozen, long n,
                                    const float* __restrict__ sq, float clip, float lr, float b1, float b2, float eps, float wd,
                                    const uint8_t* __restrict__ mask, const float* __restrict__ p0, float bc1, float bc2,
                                    float ema_decay) {
  const float sc = clip_scale(sq, clip);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    if (!frozen[i]) adamw_update<SHARED>(i, p, g, mu, nu, ema, sc, lr, b1, b2, eps, wd, mask, p0, bc1, bc2, ema_decay);
}

// ------------------------------------------------------------------------------------------------
// host sequencing
// ------------------------------------------------------------------------------------------------
// The launch seam: everything train_step / train_apply / train_accumulate enqueue goes through KL, ENQ or bgemm().  Under
// HVLA_TRAIN_TRACE (the two tools/train_*_trace.hip drivers; neither library sets it) the three print one line per operation and enqueue
// nothing: tests/native/train_step_trace.txt pins what a step launches, argument for argument.
#ifdef HVLA_TRAIN_TRACE
#include "../../tools/train_launch_trace.h"
#else
#define KL(kernel, grid, block, ...) hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__)
#define ENQ(fn, ...) (void)fn(__VA_ARGS__)
#endif
static inline dim3 g1(long n, int bs = 256) { long b = (n + bs - 1) / bs; return dim3((unsigned)(b > 65535 ? 65535 : b)); }

// Transformer block forward / backward on rows [nb][S][D] with weights at W + b * wstride (wstride = G for
// the per-episode policy, 0 for the shared context encoder).  Buffers for one layer:
// h, h2, g (the two LayerNorm outputs and the GELU output): kept per block when the plan has room for them (the backward pass
// then reads them instead of recomputing them: two LayerNorm passes and one GELU pass per block), else nullptr
// pa, oraw (a DifferentialAttention block only, else nullptr): A = A1 - lambda A2 [nb][H][S][Sp] and O = A V [nb][S][D] in front of subln,
// both kept for the backward; p is then [nb][2 H][S][Sp] and o holds subln's output, the out-projection's input
struct BlkBuf { float *x_in, *mean0, *rstd0, *q, *k, *v, *p, *o, *x_mid, *mean1, *rstd1, *u, *y1, *y2, *h, *h2, *g, *pa, *oraw; };
// one block's leaves as pointers (T = const float: weights, T = float: their gradients): BlockLeaves' members, bound to a base
template <class T> struct Blk { T *l0s, *l0b, *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo, *l1s, *l1b, *w1, *b1, *w2, *b2, *ls1, *ls2; };
using BlkW = Blk<const float>;
using BlkG = Blk<float>;
template <class T> static Blk<T> bind(T* base, const BlockLeaves& y) {
  auto at = [&](long o) { return o < 0 ? nullptr : base + o; };      // -1: the block has no such leaf (LayerScale)
  return Blk<T>{at(y.ln0_s), at(y.ln0_b), at(y.wq), at(y.bq), at(y.wk), at(y.bk), at(y.wv), at(y.bv), at(y.wo), at(y.bo),
                at(y.ln1_s), at(y.ln1_b), at(y.w1), at(y.b1), at(y.w2), at(y.b2), at(y.ls1), at(y.ls2)};
}
// one dropout rate with its key (noise.h): thr == 0 is off, and nothing is launched
struct Drop {
  uint32_t thr = 0; float keep_prob = 1.f; NoiseKey key;
  Drop() = default;
  Drop(float rate, const NoiseKey& k) : thr(rate > 0.f ? dropout_threshold(rate) : 0), keep_prob(1.0f - rate), key(k) {}
  bool on() const { return thr > 0; }
  NoiseKey at(uint32_t kind, int layer = 0) const { NoiseKey k = key; k.site = kind | (uint32_t)layer << 8; return k; }
};
// block flavour: the flax Encoder1DBlock of the context encoder / generated policy (tanh GELU, masked attention) or the
// HF Dinov2Layer (erf GELU, LayerScale on both residual branches, dense attention).  Its attention, one value per case that exists:
enum class Attn {
  Dense,            // DINOv2: no mask
  Context,          // the context encoder's mask from am (hypernetwork.py:149-181)
  ContextTokens,    // ... with NL layer tokens behind the image row (softmax_tokens_fwd_kernel)
  Policy,           // the policy's mask (base_vit.py:209-214)
  PolicyLang,       // ... with T language rows in front (softmax_lang_fwd_kernel)
  Bias,             // the policy's mask added to the scores (softmax_bias_fwd_kernel)
  Differential,     // DifferentialAttention
};
struct BlkOpt {
  Attn attn = Attn::Dense;
  // erf GELU (the HF Dinov2Layer), else tanh
  int gelu_erf = 0;
  // Context, ContextTokens: attn_mask [B][T]
  const int64_t* am = nullptr;
  // PolicyLang: the language rows.  ContextTokens: the layer tokens
  int T = 0, NL = 0;
  // the policy only: vit_kwargs.dropout_rate at the sites of `layer`, the block's depth
  Drop drop;
  int layer = 0;
  // Differential: the block's five vectors at dif in a row of theta / dtheta (row stride ws)
  DiffLeaves dif{-1, -1, -1, -1, -1};
  const float* theta = nullptr;
  float* dtheta = nullptr;
  float lambda_init() const { return (float)(0.8 - 0.6 * exp(-0.3 * (double)layer)); }      // differential_transformer.py:75-79
  bool differential() const { return attn == Attn::Differential; }
  // The key bias adds q . bk / sqrt(hd) to every kept score of a query's row, and a softmax row ignores a constant: its gradient is
  // zero under any mask (sum_k ds[q][k] = 0).  What the column sum of dk gives instead is the operand rounding of ds in dk = ds^T q,
  // and a language query's few keys carry ds entries of the size of dp: with the language rows the leaf is left at the zero it is
  // (dtheta is cleared at the head of the step).  Without them the step launches what it always launched.  With the mask added as a
  // bias every query has every key, the constant is still one per row, and the leaf is left at zero in the same way:
  // measured at the README geometry the column sum came to 1.9e-3 of the leaf metric's 2e-3, all of it rounding.  Under the policy's
  // dropout (hvla_train_noise) the kept activations are 1 / keep_prob larger and the same rounding came to 1.5e-3 at MID: left at zero too.
  bool key_bias_grad_is_rounding() const { return attn == Attn::PolicyLang || attn == Attn::Bias || drop.on(); }
};
// dP, t2 (a DifferentialAttention policy only, else nullptr): dp = dO V^T [nb][H][S][Sp] and the row sums sum_k dp A2 [nb][H][S];
// dp is then ds [nb][2 H][S][Sp]
struct BlkTmp { float *h, *g, *d, *dq, *dk, *dv, *dp, *y, *dP, *t2; };

// Y[nb][S][N] (+)= X[nb][S][K] W + bias with W per episode (ws = G) or shared (ws = 0: the batch folds into M, so
// S = 257 does not pay a mostly empty 64-row tile per sample)
static void linear(hipStream_t st, int nb, int S, long ws, const float* X, const float* W, const float* bias, float* Y, int K, int N, Store store = Store::Set) {
  if (ws == 0) bgemm(st, false, false, with_bias(product(mat(X, K), mat(W, N), mat(Y, N), nb * S, N, K, store), bias), 1);
  else bgemm(st, false, false, with_bias(product(per_sample(X, S, K), per_episode(W, N, ws), per_sample(Y, S, N), S, N, K, store), bias, ws), nb);
}
// dX[nb][S][K] (+)= dY[nb][S][N] W^T
static void linear_dx(hipStream_t st, int nb, int S, long ws, const float* dY, const float* W, float* dX, int K, int N, Store store = Store::Set) {
  if (ws == 0) bgemm(st, false, true, product(mat(dY, N), mat(W, N), mat(dX, K), nb * S, K, N, store), 1);
  else bgemm(st, false, true, product(per_sample(dY, S, N), per_episode(W, N, ws), per_sample(dX, S, K), S, K, N, store), nb);
}
// the attention products over Hn heads of width w: p_h = alpha q_h k_h^T into the score tables, and y_h = alpha p_h x_h (ta: p_h^T x_h)
static void scores(hipStream_t st, int nb, int S, int D, const float* q, const float* k, float* p, int Hn, int w, float alpha = 1.f) {
  bgemm(st, false, true, product(head_slice(q, S, D, w), head_slice(k, S, D, w), score_table(p, Hn, S), S, S, w, Store::Set, alpha, Hn), nb);
}
static void apply_scores(hipStream_t st, bool ta, int nb, int S, int D, const float* p, const float* x, float* y, int Hn, int w, float alpha = 1.f) {
  bgemm(st, ta, false, a_padded(product(score_table(p, Hn, S), head_slice(x, S, D, w), head_slice(y, S, D, w), S, w, S, Store::Set, alpha, Hn)), nb);
}
// every pointer on a 16-byte boundary (the float4 forms)
template <class... T> static bool aligned16(const T*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0; }
// q, k, v (0, 1, 2) in the memory order of p[] -- or in `order`, when given -- and whether the three are equally spaced, `step` apart
struct Spacing { int ord[3]; long step; bool even; };
template <class T> static Spacing spacing(T* const* p, const int* order = nullptr) {
  Spacing s{{0, 1, 2}, 0, false};
  for (int i = 0; i < 2 && !order; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (p[s.ord[j]] > p[s.ord[j + 1]]) { const int tsw = s.ord[j]; s.ord[j] = s.ord[j + 1]; s.ord[j + 1] = tsw; }
  for (int i = 0; i < 3 && order; ++i) s.ord[i] = order[i];
  s.step = p[s.ord[1]] - p[s.ord[0]];
  s.even = p[s.ord[2]] - p[s.ord[1]] == s.step;
  return s;
}

static void scale_add(hipStream_t st, float* out, const float* res, const float* y, const float* ls, long n, int D) {
  const bool v4 = D % 4 == 0 && aligned16(out, res, y, ls);
  if (v4) KL(scale_add4_kernel, g1(n / 4), dim3(256), reinterpret_cast<f32x4*>(out), reinterpret_cast<const f32x4*>(res), reinterpret_cast<const f32x4*>(y), reinterpret_cast<const f32x4*>(ls), n / 4, D / 4);
  else KL(scale_add_kernel, g1(n), dim3(256), out, res, y, ls, n, D);
}

// out = [res +] drop(x) / dx = dy (.) multiplier over nb samples of n elements each (n % 4 == 0)
static void dropout_fwd(hipStream_t st, const Drop& d, uint32_t kind, int layer, float* out, const float* res, const float* x, int nb, long n) {
  KL(dropout_fwd_kernel, dim3((unsigned)((n / 4 + 255) / 256), nb), dim3(256), out, res, x, (int)(n / 4), d.at(kind, layer), d.thr, d.keep_prob);
}
static void dropout_bwd(hipStream_t st, const Drop& d, uint32_t kind, int layer, float* dx, const float* dy, int nb, long n) {
  KL(dropout_bwd_kernel, dim3((unsigned)((n / 4 + 255) / 256), nb), dim3(256), dx, dy, (int)(n / 4), d.at(kind, layer), d.thr, d.keep_prob);
}

static void block_fwd(hipStream_t st, int nb, int S, int D, int H, int F, long ws, const BlkW& w, const BlkBuf& a,
                      float* x_out, const BlkTmp& t, const BlkOpt& op) {
  const int hd = D / H, rows = nb * S;
  const Drop& dr = op.drop;
  float* const h = a.h ? a.h : t.h;
  float* const h2 = a.h2 ? a.h2 : t.h;
  float* const gg = a.g ? a.g : t.g;
  KL(ln_fwd_kernel, dim3((rows + 3) / 4), dim3(256), a.x_in, h, a.mean0, a.rstd0, w.l0s, w.l0b, ws, rows, S, D);
  const int Sp = score_stride(S);
  if (op.differential()) {
    // DifferentialAttention: bias-free q, k, v; 2 H sub-heads of width hd / 2 with stride hd / 2 in q and k, unscaled
    // scores; softmax_bias_fwd_kernel per sub-head row (the mask is added, as in §20); A = A1 - lambda A2; O = A V; subln into a.o
    const int hp = hd / 2, H2 = 2 * H;
    const DiffLeaves& df = op.dif;
    linear(st, nb, S, ws, h, w.wq, nullptr, a.q, D, D);
    linear(st, nb, S, ws, h, w.wk, nullptr, a.k, D, D);
    linear(st, nb, S, ws, h, w.wv, nullptr, a.v, D, D);
    scores(st, nb, S, D, a.q, a.k, a.p, H2, hp);
    KL(softmax_bias_fwd_kernel, dim3((nb * H2 * S + 3) / 4), dim3(256), a.p, nb * H2, S, Sp);
    KL(diff_combine_fwd_kernel, dim3((nb * H * S + 3) / 4), dim3(256), a.p, a.pa, op.theta, ws, df.lq1, df.lk1, df.lq2, df.lk2, op.lambda_init(), nb, H, S, Sp);
    apply_scores(st, false, nb, S, D, a.pa, a.v, a.oraw, H, hd);
    KL(diff_subln_fwd_kernel, dim3((rows + 3) / 4), dim3(256), a.oraw, a.o, op.theta, ws, df.sw, 1.f - op.lambda_init(), rows, S);
  } else {
    // q, k, v = h Wq, h Wk, h Wv as ONE batched product when weights, biases and outputs are equally spaced in memory order
    // (shared weights): 3 x 390 tiles in one launch instead of three launches of 198 double tiles that fill 77 % of the chip
    const float* Wm[3] = {w.wq, w.wk, w.wv};
    const float* Bm[3] = {w.bq, w.bk, w.bv};
    float* Ym[3] = {a.q, a.k, a.v};
    const Spacing sw = spacing(Wm), sb = spacing(Bm, sw.ord), sy = spacing(Ym, sw.ord);
    const int first = sw.ord[0];
    if (ws == 0 && sw.even && sb.even && sy.even && sw.step % 4 == 0 && sy.step % 4 == 0)
      bgemm(st, false, false, with_bias(product(mat(h, D), inner_batch(Wm[first], D, sw.step), inner_batch(Ym[first], D, sy.step), nb * S, D, D, Store::Set, 1.f, 3),
                                        Bm[first], 0, sb.step), 1);
    else
      for (int i = 0; i < 3; ++i) linear(st, nb, S, ws, h, Wm[i], Bm[i], Ym[i], D, D);
    scores(st, nb, S, D, a.q, a.k, a.p, H, hd, 1.f / sqrtf((float)hd));      // scores[b][h] = q_h k_h^T / sqrt(hd)
    const dim3 sgrid((nb * H * S + 3) / 4);
    // mode (softmax_fwd_kernel): 0 the policy's mask, 1 the context mask from am, 2 none
    auto softmax = [&](int mode) { KL(softmax_fwd_kernel, sgrid, dim3(256), a.p, nb * H, S, S, mode, op.am, H, Sp); };
    switch (op.attn) {
      case Attn::Dense: softmax(2); break;
      case Attn::Context: softmax(1); break;
      case Attn::Policy: softmax(0); break;
      case Attn::ContextTokens: KL(softmax_tokens_fwd_kernel, sgrid, dim3(256), a.p, nb * H, S, S - 1 - op.NL, op.am, H, Sp); break;
      case Attn::PolicyLang: KL(softmax_lang_fwd_kernel, sgrid, dim3(256), a.p, nb * H, S, op.T, Sp); break;
      case Attn::Bias: KL(softmax_bias_fwd_kernel, sgrid, dim3(256), a.p, nb * H, S, Sp); break;
      case Attn::Differential: break;      // (above)
    }
    apply_scores(st, false, nb, S, D, a.p, a.v, a.o, H, hd);
  }
  if (w.ls1) {
    linear(st, nb, S, ws, a.o, w.wo, w.bo, a.y1, D, D);
    scale_add(st, a.x_mid, a.x_in, a.y1, w.ls1, (long)rows * D, D);
  } else if (dr.on()) {                                                    // the branch into t.y (free in a block without LayerScale), then x_mid = x_in + drop(y)
    linear(st, nb, S, ws, a.o, w.wo, w.bo, t.y, D, D);
    dropout_fwd(st, dr, NOISE_ATTN_OUT, op.layer, a.x_mid, a.x_in, t.y, nb, (long)S * D);
  } else {
    ENQ(hipMemcpyAsync, a.x_mid, a.x_in, (size_t)rows * D * 4, hipMemcpyDeviceToDevice, st);
    linear(st, nb, S, ws, a.o, w.wo, w.bo, a.x_mid, D, D, Store::Add);
  }
  KL(ln_fwd_kernel, dim3((rows + 3) / 4), dim3(256), a.x_mid, h2, a.mean1, a.rstd1, w.l1s, w.l1b, ws, rows, S, D);
  linear(st, nb, S, ws, h2, w.w1, w.b1, a.u, D, F);
  KL(gelu_fwd_kernel, g1((long)rows * F), dim3(256), a.u, gg, (long)rows * F, op.gelu_erf);
  if (dr.on()) dropout_fwd(st, dr, NOISE_MLP_HIDDEN, op.layer, gg, nullptr, gg, nb, (long)S * F);     // g is kept (or recomputed) dropped
  if (w.ls2) {
    linear(st, nb, S, ws, gg, w.w2, w.b2, a.y2, F, D);
    scale_add(st, x_out, a.x_mid, a.y2, w.ls2, (long)rows * D, D);
  } else if (dr.on()) {
    linear(st, nb, S, ws, gg, w.w2, w.b2, t.y, F, D);
    dropout_fwd(st, dr, NOISE_MLP_OUT, op.layer, x_out, a.x_mid, t.y, nb, (long)S * D);
  } else {
    ENQ(hipMemcpyAsync, x_out, a.x_mid, (size_t)rows * D * 4, hipMemcpyDeviceToDevice, st);
    linear(st, nb, S, ws, gg, w.w2, w.b2, x_out, F, D, Store::Add);
  }
}

// dx (in/out: gradient wrt the block output on entry, wrt its input on exit).  Weight gradients: per-episode
// (gs = G) written per b; shared (gs = 0) reduced over the batch by folding it into the GEMM's M/K dimension.
// aux (nullable; the last policy layer under hvla_train_attention_losses): the attention terms' gradient joins dp in front of the softmax backward.
static void block_bwd(hipStream_t st, int nb, int S, int D, int H, int F, long ws, long gs, const BlkW& w, const BlkG& gw,
                      const BlkBuf& a, float* dx, const BlkTmp& t, const BlkOpt& op, const AuxP* aux = nullptr) {
  const int hd = D / H, rows = nb * S;
  const bool shared = gs == 0;
  auto wgrad = [&](const float* X, int K, const float* dY, int N, float* dW) {   // dW[K][N] (+)= X^T dY
    if (shared) bgemm(st, true, false, product(mat(X, K), mat(dY, N), mat(dW, N), K, N, rows, Store::AddSplitK), 1);
    else bgemm(st, true, false, product(per_sample(X, S, K), per_sample(dY, S, N), per_episode(dW, N, gs), K, N, S, Store::Add), nb);
  };
  auto bgrad = [&](const float* dY, int N, float* dB) {
    // the 4-column form wins on the narrow matrices of the policy / hypernetwork; on the encoder's 768- and 3072-wide ones
    // its fewer, fatter waves lose to the one-column form (17 vs 23 us)
    if (op.differential()) { KL(colsum_episode_kernel, dim3((N + 63) / 64, nb), dim3(256), dY, dB, gs, S, S, N); return; }      // no atomics
    const bool v4 = N % 4 == 0 && N <= 512 && aligned16(dY);
    if (shared && N % 4 == 0 && N > 512 && rows >= 2048 && aligned16(dY))
      KL(colsum4b_kernel, dim3((N / 4 + 63) / 64, 1, (rows + CSB_WAVES * 8 * CSB_BATCH - 1) / (CSB_WAVES * 8 * CSB_BATCH)), dim3(CSB_WAVES * 64), dY, dB, rows, N);
    else if (shared && v4) KL(colsum4_kernel, dim3((N / 4 + 63) / 64, 1, (rows + 31) / 32), dim3(64), dY, dB, 0, rows, rows, N, 1);
    else if (shared) KL(colsum_kernel, dim3((N + 63) / 64, 1, (rows + 63) / 64), dim3(64), dY, dB, 0, rows, rows, N, 1);
    else if (v4) KL(colsum4_kernel, dim3((N / 4 + 63) / 64, nb, (S + 31) / 32), dim3(64), dY, dB, gs, S, S, N, nb);
    else KL(colsum_kernel, dim3((N + 63) / 64, nb, (S + 63) / 64), dim3(64), dY, dB, gs, S, S, N, nb);
  };
  auto ln_bwd = [&](const float* x, const float* dy, const float* mean, const float* rstd, const float* sc, float* gs_, float* gb_) {
    if (op.differential()) {                                                                                            // no atomics
      KL(ln_bwd_kernel, dim3((rows + 3) / 4), dim3(256), x, dy, mean, rstd, sc, dx, (float*)nullptr, (float*)nullptr, gs, rows, S, D, 1);
      KL(ln_pgrad_episode_kernel, dim3((D + 63) / 64, nb), dim3(256), x, dy, mean, rstd, gs_, gb_, gs, S, D);
      return;
    }
    if (shared && D % 4 == 0 && D <= 1024 && aligned16(x, dy, dx)) {
      KL(ln_bwd_shared_kernel, dim3((rows + 63) / 64), dim3(LNB_WAVES * 64), x, dy, mean, rstd, sc, dx, gs_, gb_, rows, D, 1);
    } else if (shared) {
      KL(ln_bwd_kernel, dim3((rows + 3) / 4), dim3(256), x, dy, mean, rstd, sc, dx, (float*)nullptr, (float*)nullptr, 0, rows, S, D, 1);
      KL(ln_pgrad_kernel, dim3((D + 63) / 64, (rows + 63) / 64), dim3(64), x, dy, mean, rstd, gs_, gb_, rows, D);
    } else {
      KL(ln_bwd_kernel, dim3((rows + 3) / 4), dim3(256), x, dy, mean, rstd, sc, dx, gs_, gb_, gs, rows, S, D, 1);
    }
  };
  auto ls_bwd = [&](const float* dxp, const float* y, const float* ls, float* dy, float* dls) {
    if (D % 4 == 0 && rows >= 1024 && aligned16(dxp, y, dy))
      KL(ls_bwd4_kernel, dim3((D / 4 + 63) / 64, (rows + 127) / 128), dim3(512), dxp, y, ls, dy, dls, rows, D);
    else
      KL(ls_bwd_kernel, dim3((D + 63) / 64, (rows + 63) / 64), dim3(64), dxp, y, ls, dy, dls, rows, D);
  };
  // ---- MLP: x_out = x_mid + [ls2 (.)] (gelu(LN1(x_mid) W1 + b1) W2 + b2)
  const float* h2 = a.h2 ? a.h2 : t.h;
  const float* gg = a.g ? a.g : t.g;
  if (!a.h2) KL(ln_fwd_kernel, dim3((rows + 3) / 4), dim3(256), a.x_mid, t.h, a.mean1, a.rstd1, w.l1s, w.l1b, ws, rows, S, D);   // recompute h2
  if (!a.g) KL(gelu_fwd_kernel, g1((long)rows * F), dim3(256), a.u, t.g, (long)rows * F, op.gelu_erf);                           // recompute g
  const Drop& dr = op.drop;
  if (!a.g && dr.on()) dropout_fwd(st, dr, NOISE_MLP_HIDDEN, op.layer, t.g, nullptr, t.g, nb, (long)S * F);                       //   ... dropped, as block_fwd left it
  const float* dy = dx;
  if (w.ls2) {
    ls_bwd(dx, a.y2, w.ls2, t.y, gw.ls2);
    dy = t.y;
  } else if (dr.on()) {                                                                                                 // the branch's gradient into t.y, dx stays the residual's
    dropout_bwd(st, dr, NOISE_MLP_OUT, op.layer, t.y, dx, nb, (long)S * D);
    dy = t.y;
  }
  wgrad(gg, F, dy, D, gw.w2);
  bgrad(dy, D, gw.b2);
  linear_dx(st, nb, S, ws, dy, w.w2, t.d, F, D);                                                                        // dg = dy W2^T
  if (dr.on()) dropout_bwd(st, dr, NOISE_MLP_HIDDEN, op.layer, t.d, t.d, nb, (long)S * F);
  KL(gelu_bwd_kernel, g1((long)rows * F), dim3(256), a.u, t.d, (long)rows * F, op.gelu_erf);                           // du
  wgrad(h2, D, t.d, F, gw.w1);
  bgrad(t.d, F, gw.b1);
  linear_dx(st, nb, S, ws, t.d, w.w1, t.g, D, F);                                                                       // dh2 -> t.g[rows][D]
  ln_bwd(a.x_mid, t.g, a.mean1, a.rstd1, w.l1s, gw.l1s, gw.l1b);
  //   (dx now = gradient wrt x_mid)
  // ---- attention: x_mid = x_in + [ls1 (.)] (o Wo + bo)
  dy = dx;
  if (w.ls1) {
    ls_bwd(dx, a.y1, w.ls1, t.y, gw.ls1);
    dy = t.y;
  } else if (dr.on()) {
    dropout_bwd(st, dr, NOISE_ATTN_OUT, op.layer, t.y, dx, nb, (long)S * D);
    dy = t.y;
  }
  wgrad(a.o, D, dy, D, gw.wo);
  if (gw.bo) bgrad(dy, D, gw.bo);                                                                                       // (DifferentialAttention's projections have no bias)
  linear_dx(st, nb, S, ws, dy, w.wo, t.d, D, D);                                                                        // do
  // dp = do_h v_h^T ; dv_h = p^T do_h
  const int Sp = score_stride(S);                                                                                       // row stride of p / dp (block_fwd)
  if (op.differential()) {
    // t.d = dN -> dO and dw (subln); dP = dO V^T once per head; dV = A^T dO; both softmax backwards from dP into t.dp = ds [nb][2 H];
    // d lambda from the kept row sums; dq_c = ds_c k_c, dk_c = ds_c^T q_c over the 2 H sub-heads, scale 1
    const int hp = hd / 2, H2 = 2 * H;
    const DiffLeaves& df = op.dif;
    KL(diff_subln_bwd_kernel, dim3(nb), dim3(256), a.oraw, t.d, op.theta, op.dtheta, ws, df.sw, 1.f - op.lambda_init(), S);
    scores(st, nb, S, D, t.d, a.v, t.dP, H, hd);
    apply_scores(st, true, nb, S, D, a.pa, t.d, t.dv, H, hd);
    KL(diff_softmax_bwd_kernel, dim3((nb * H * S + 3) / 4), dim3(256), a.p, t.dP, t.dp, t.t2, op.theta, ws, df.lq1, df.lk1, df.lq2, df.lk2, op.lambda_init(), nb, H, S, Sp);
    KL(diff_lambda_bwd_kernel, dim3(nb), dim3(64), t.t2, op.theta, op.dtheta, ws, df.lq1, df.lk1, df.lq2, df.lk2, H * S);
    apply_scores(st, false, nb, S, D, t.dp, a.k, t.dq, H2, hp);
    apply_scores(st, true, nb, S, D, t.dp, a.q, t.dk, H2, hp);
  } else {
    scores(st, nb, S, D, t.d, a.v, t.dp, H, hd);
    apply_scores(st, true, nb, S, D, a.p, t.d, t.dv, H, hd);
    if (aux) KL(attention_aux_kernel, dim3(nb), dim3(256), *aux);                                                            // dp row S-1 += d aux / dp
    KL(softmax_bwd_kernel, dim3((nb * H * S + 3) / 4), dim3(256), a.p, t.dp, nb * H * S, S, Sp);                             // ds
    const float sc = 1.f / sqrtf((float)hd);
    apply_scores(st, false, nb, S, D, t.dp, a.k, t.dq, H, hd, sc);                                                           // dq = ds k / sqrt(hd)
    apply_scores(st, true, nb, S, D, t.dp, a.q, t.dk, H, hd, sc);                                                            // dk = ds^T q / sqrt(hd)
  }
  const float* h = a.h ? a.h : t.h;
  if (!a.h) KL(ln_fwd_kernel, dim3((rows + 3) / 4), dim3(256), a.x_in, t.h, a.mean0, a.rstd0, w.l0s, w.l0b, ws, rows, S, D);      // recompute h
  const float* dqkv[3] = {t.dq, t.dk, t.dv};
  float* gWm[3] = {gw.wq, gw.wk, gw.wv};
  float* gBm[3] = {gw.bq, gw.bk, gw.bv};
  const float* Wm[3] = {w.wq, w.wk, w.wv};
  // the three weight gradients h^T dq, h^T dk, h^T dv as ONE batched product when the three dY buffers and the three gradient
  // leaves are equally spaced (shared weights; any order): one launch whose split-K needs a third of the atomic adds per element
  const Spacing sg = spacing(gWm), sd = spacing(dqkv, sg.ord);      // q, k, v in the order of their gradient leaves in memory
  const bool one = shared && sd.even && sg.even && sd.step % 4 == 0;
  if (one) bgemm(st, true, false, product(mat(h, D), inner_batch(dqkv[sg.ord[0]], D, sd.step), inner_batch(gWm[sg.ord[0]], D, sg.step), D, D, rows, Store::AddSplitK, 1.f, 3), 1);
  for (int i = 0; i < 3; ++i) {
    if (!one) wgrad(h, D, dqkv[i], D, gWm[i]);
    if (gBm[i] && !(i == 1 && op.key_bias_grad_is_rounding())) bgrad(dqkv[i], D, gBm[i]);      // (BlkOpt: the key bias's gradient)
    linear_dx(st, nb, S, ws, dqkv[i], Wm[i], t.g, D, D, i > 0 ? Store::Add : Store::Set);                                // dh
  }
  ln_bwd(a.x_in, t.g, a.mean0, a.rstd0, w.l0s, gw.l0s, gw.l0b);
}

// ---- workspace plan (shared by the size query and the step so the two cannot drift) ----------------------------
struct Plan {
  std::vector<BlkBuf> cb, pb, eb;
  float *cx_fin, *cdx, *px_fin, *pdx, *ex_fin, *edx, *eh, *patches;
  BlkTmp t;
  float *cmean, *crstd, *ctx, *dctx, *ctxn, *dxrow, *emean, *erstd;
  float *ntok, *ncls;        // hvla_train_noise: the frozen encoder's tokens + sigma z, the masked CLS rows (null: not taken)
  long used;
  // the buffer table, in the order of the takes: a -DHVLA_TRAIN_TRACE build records it for train_trace_plan, the libraries build no
  // string and store nothing
#ifdef HVLA_TRAIN_TRACE
  struct Taken { std::string name; long offset, floats; };
  std::vector<Taken> taken;
  void note(const char* kind, size_t l, const char* name, long offset, long n) {      // kind: "<kind>[<l>].<name>", a block's buffer
    taken.push_back({kind ? std::string(kind) + "[" + std::to_string(l) + "]." + name : std::string(name), offset, n});
  }
#else
  void note(const char*, size_t, const char*, long, long) {}
#endif
};
static Plan make_plan(const Geom& g, int B, bool enc, float* base, const TrainNoise& nz) {
  Plan pl;
  float* ws = base;
  auto take = [&](const char* name, long n, const char* kind = nullptr, size_t l = 0) {
    float* p = ws;
    ws += (n + 3) / 4 * 4;
    pl.note(kind, l, name, p - base, n);
    return p;
  };
  // block l of pl.<kind>.  diff: a DifferentialAttention block -- p holds 2 h tables, and pa and oraw follow the block's other buffers
  auto take_blk = [&](const char* kind, size_t l, long nb, long s, long d, long h, long f, bool ls, bool diff = false) {
    auto tk = [&](const char* name, long n) { return take(name, n, kind, l); };
    const long x = nb * s * d, r = nb * s;
    BlkBuf b; b.x_in = tk("x_in", x); b.mean0 = tk("mean0", r); b.rstd0 = tk("rstd0", r); b.k = tk("k", x); b.q = tk("q", x);      // k, q, v: the order of the weight leaves (block_fwd batches the three)
    b.v = tk("v", x); b.p = tk("p", nb * score_floats(h, s, diff)); b.o = tk("o", x); b.x_mid = tk("x_mid", x); b.mean1 = tk("mean1", r);
    b.rstd1 = tk("rstd1", r); b.u = tk("u", r * f);
    b.y1 = ls ? tk("y1", x) : nullptr; b.y2 = ls ? tk("y2", x) : nullptr;
    // 288 GB of HBM: the LayerNorm and GELU outputs are kept (B = 32 with the encoder trained: 1.8 GB) instead of recomputed
    b.h = tk("h", x); b.h2 = tk("h2", x); b.g = tk("g", r * f);
    b.pa = diff ? tk("pa", nb * score_floats(h, s)) : nullptr; b.oraw = diff ? tk("oraw", x) : nullptr;
    return b;
  };
  const long S = g.pos_rows(), D = g.D, H = g.H, F = g.M, NL = g.NL(), Sc = g.T + 1 + NL, C = g.C, Hc = g.ctx_heads, Fc = g.ctx_mlp;     // S: the policy's rows, T + P + 1 under use_language_token; NL = 1 without layer tokens
  const long Se = g.P() + 1, E = g.E, He = g.enc_heads, Fe = g.enc_mlp;
  const bool diff = g.differential != 0;
  pl.cb.resize(g.ctx_layers); pl.pb.resize(g.L); pl.eb.resize(enc ? g.enc_layers : 0);
  for (size_t l = 0; l < pl.cb.size(); ++l) pl.cb[l] = take_blk("cb", l, B, Sc, C, Hc, Fc, false);
  for (size_t l = 0; l < pl.pb.size(); ++l) pl.pb[l] = take_blk("pb", l, B, S, D, H, F, false, diff);
  for (size_t l = 0; l < pl.eb.size(); ++l) pl.eb[l] = take_blk("eb", l, B, Se, E, He, Fe, true);
  pl.cx_fin = take("cx_fin", B * Sc * C); pl.cdx = take("cdx", B * Sc * C);
  pl.px_fin = take("px_fin", B * S * D); pl.pdx = take("pdx", B * S * D);
  pl.ex_fin = pl.edx = pl.eh = pl.patches = pl.emean = pl.erstd = nullptr;
  if (enc) {
    pl.ex_fin = take("ex_fin", B * Se * E); pl.edx = take("edx", B * Se * E); pl.eh = take("eh", B * Se * E);
    pl.patches = take("patches", (long)B * g.P() * g.patch * g.patch * 3);
    pl.emean = take("emean", B * Se); pl.erstd = take("erstd", B * Se);
  }
  // temporaries are used by one transformer at a time: size them for the largest.  t.g and t.d hold rows x F (the GELU output's
  // gradient, du) AND rows x D (dh2 = du W1^T and the three dh products go to t.g, do = dy Wo^T to t.d): the larger of the two,
  // since accept.h admits F < D (policy mlp 32, ctx_mlp 16, enc_mlp 128 under a wider model)
  auto mx = [&](long a, long b, long c) { c = enc ? c : 0; return a > b ? (a > c ? a : c) : (b > c ? b : c); };
  const long rd = mx(B * S * D, B * Sc * C, B * Se * E), rf = mx(B * S * F, B * Sc * Fc, B * Se * Fe);
  const long hss = mx(B * score_floats(H, S, diff), B * score_floats(Hc, Sc), B * score_floats(He, Se)), rg = rf > rd ? rf : rd;
  pl.t.h = take("t.h", rd); pl.t.g = take("t.g", rg); pl.t.d = take("t.d", rg);
  pl.t.dk = take("t.dk", rd); pl.t.dq = take("t.dq", rd); pl.t.dv = take("t.dv", rd);      // k, q, v: the order of the leaves (block_bwd batches the three)
  pl.t.dp = take("t.dp", hss); pl.t.y = take("t.y", rd);
  pl.cmean = take("cmean", B * NL); pl.crstd = take("crstd", B * NL);
  pl.ctx = take("ctx", B * NL * C); pl.dctx = take("dctx", B * NL * C); pl.ctxn = take("ctxn", B * NL * C);
  pl.dxrow = take("dxrow", B * D);
  // the noise copies come last: every offset above is what it is without noise
  pl.ntok = nz.sigma > 0.f && !enc ? take("ntok", (long)B * g.P() * E) : nullptr;
  pl.ncls = nz.image_dropout > 0.f ? take("ncls", (long)B * E) : nullptr;
  // ... and so do DifferentialAttention's two temporaries (t.dp above holds ds of the 2 H sub-heads)
  pl.t.dP = diff ? take("t.dP", B * score_floats(H, S)) : nullptr;
  pl.t.t2 = diff ? take("t.t2", B * H * S) : nullptr;
  pl.used = ws - base;
  return pl;
}
size_t train_workspace_floats(const Geom& g, int B, bool train_encoder, const TrainNoise& nz) {
  return (size_t)make_plan(g, B, train_encoder, nullptr, nz).used + 64;
}
void train_context_rows(const Geom& g, int B, bool train_encoder, const TrainNoise& nz, long out[3]) {
  const Plan pl = make_plan(g, B, train_encoder, nullptr, nz);
  out[0] = pl.ctx - static_cast<float*>(nullptr); out[1] = pl.dctx - static_cast<float*>(nullptr); out[2] = (long)B * g.NL() * g.C;
}
#ifdef HVLA_TRAIN_TRACE
// One line `plan <name> <offset> <floats>` per buffer of make_plan (offsets into `work`, the floats the plan asked for), for
// tools/train_extent_trace.hip: tests/test_train_workspace_extents.py holds every traced operand to ONE of these buffers.  The names
// are those make_plan's takes give.
void train_trace_plan(const Geom& g, int B, bool train_encoder, const TrainNoise& nz) {
  const Plan pl = make_plan(g, B, train_encoder, static_cast<float*>(train_trace_buffer("work")), nz);
  for (const Plan::Taken& t : pl.taken) printf("plan %s %ld %ld\n", t.name.c_str(), t.offset, t.floats);
}
#endif

hipError_t train_step(const Geom& g, const TrainLayout& L, const TrainBuffers& tb, const TrainInputs& in, int B,
                      const TrainHyper& hp, hipStream_t st, hipEvent_t* bucket_done, const TrainOptions& opt) {
  const PosSource& ps = opt.ps;
  const AttnAux& aux = opt.aux;
  const int frozen_buckets = opt.frozen_buckets;
  const int Tl = g.lang_in_policy ? g.T : 0;       // use_language_token: the policy's rows are [Tl language | P patches | 1 action]
  const int S = g.pos_rows(), P = g.P(), D = g.D, H = g.H, F = g.M, E = g.E;
  const int NL = g.NL(), Sc = g.T + 1 + NL, C = g.C, Hc = g.ctx_heads, Fc = g.ctx_mlp, T = g.T;      // NL > 1: layer tokens
  const bool lt = g.layer_tokens != 0;
  const TokenGroups& tg = opt.groups;
  const float cpost = g.scale_context ? 1.f / sqrtf((float)C) : 1.f;
  const int Se = P + 1, He = g.enc_heads, Fe = g.enc_mlp, Kp = g.patch * g.patch * 3;
  const bool enc = in.images != nullptr;
  const long G = L.G;
  // forward_only (validation, train=False) draws nothing; the plan is the setting's, so a step and a validation share offsets
  const TrainNoise nz = hp.forward_only ? TrainNoise() : opt.noise;
  const Drop pdrop(nz.policy_dropout, nz.key), cdrop(nz.context_dropout, nz.key), idrop(nz.image_dropout, nz.key);
  const Plan pl = make_plan(g, B, enc, tb.work, opt.noise);
  const std::vector<BlkBuf>&cb = pl.cb, &pb = pl.pb, &eb = pl.eb;
  float *cx_fin = pl.cx_fin, *cdx = pl.cdx, *px_fin = pl.px_fin, *pdx = pl.pdx;
  float *cmean = pl.cmean, *crstd = pl.crstd, *ctx = pl.ctx, *dctx = pl.dctx, *ctxn = pl.ctxn, *dxrow = pl.dxrow;
  const BlkTmp& t = pl.t;
  const float* Pm = tb.params;
  float* Gm = tb.grads;
  const float* Pe = Pm + L.total;          // shared DINOv2 leaves (only touched when enc)
  float* Ge = Gm + L.total;
  const bool src_on = enc && ps.n > 0;      // the position table is trained through its interpolation: its source is the vector's tail
  ENQ(hipMemsetAsync, Gm, 0, (size_t)train_vector_elems(L, ps, enc) * 4, st);
  ENQ(hipMemsetAsync, tb.dtheta, 0, (size_t)B * G * 4, st);
  BlkOpt ctx_opt, enc_opt;                  // these two draw nothing
  ctx_opt.attn = lt ? Attn::ContextTokens : Attn::Context;
  ctx_opt.am = in.attn_mask;
  ctx_opt.NL = lt ? NL : 0;
  enc_opt.attn = Attn::Dense;
  enc_opt.gelu_erf = 1;
  // hvla_create refuses every pair of use_language_token, attention_mask_as_bias and differential_attention (api.hip; train_refusal
  // and accept.h add none), so at most one of the three is set; were two, this order is the priority the blocks always had
  const Attn pol_attn = g.differential ? Attn::Differential : Tl ? Attn::PolicyLang : g.mask_as_bias ? Attn::Bias : Attn::Policy;
  const auto pol_at = [&](int l) {
    BlkOpt o;
    o.attn = pol_attn;
    o.T = Tl;
    o.drop = pdrop;
    o.layer = l;                                                                       // the dropout sites carry their layer
    if (o.differential()) { o.dif = L.dif[l]; o.theta = tb.theta; o.dtheta = tb.dtheta; }
    return o;
  };

  // =============================== DINOv2 forward in f32, activations kept (HF Dinov2Model; base_vit.py:111-131) =====
  const float* tokens = in.tokens;         // [B][P][E] rows, episode stride tok_stride
  long tok_stride = (long)P * E;
  if (enc) {
    float* ex0 = eb.empty() ? pl.ex_fin : eb[0].x_in;
    if (src_on) ENQ(launch_position_interp, Pe + L.enc_total, ps.n, ps.w, tb.params + L.total + L.e_pos, ps.grid, E, st);     // tail -> slot
    KL(im2col_f32_kernel, g1((long)B * P * Kp), dim3(256), in.images, pl.patches, B, g.image_size, g.patch);
    bgemm(st, false, false, with_bias(product(per_sample(pl.patches, P, Kp), mat(Pe + L.e_pk, E), per_sample(ex0 + E, Se, E), P, E, Kp), Pe + L.e_pb), B);      // rows 1.. of x0
    KL(enc_x0_kernel, g1((long)B * Se * E), dim3(256), ex0, Pe + L.e_cls, Pe + L.e_pos, B, Se, E);
    for (int l = 0; l < g.enc_layers; ++l)
      block_fwd(st, B, Se, E, He, Fe, 0, bind(Pe, L.enc[l]), eb[l], l + 1 < g.enc_layers ? eb[l + 1].x_in : pl.ex_fin, t, enc_opt);
    KL(ln_fwd_kernel, dim3((B * Se + 3) / 4), dim3(256), pl.ex_fin, pl.eh, pl.emean, pl.erstd, Pe + L.e_lns, Pe + L.e_lnb, 0, B * Se, Se, E);
    tokens = pl.eh + E;                    // drop the CLS row through the pointer: rows 1.. of every [Se][E] block
    tok_stride = (long)Se * E;
  }
  // image_embedding_noise (base_vit.py:123-127): tokens + sigma z, onto the trained encoder's own output (the gradient passes the
  // addition unchanged) or into the workspace's copy of the frozen encoder's
  if (nz.sigma > 0.f) {
    float* const dst = enc ? pl.eh + E : pl.ntok;
    const long dstride = enc ? tok_stride : (long)P * E;
    KL(token_noise_kernel, dim3((unsigned)((P * E / 4 + 255) / 256), B), dim3(256), dst, dstride, tokens, tok_stride, P * E / 4, Drop(0.f, nz.key).at(NOISE_TOKENS), nz.sigma);
    tokens = dst;
    tok_stride = dstride;
  }
  // image_dropout (hypernetwork.py:119-122) on the CLS row the context path reads, into its copy
  const float* cls = in.cls;
  if (idrop.on()) {
    dropout_fwd(st, idrop, NOISE_IMAGE_CLS, 0, pl.ncls, nullptr, in.cls, B, E);
    cls = pl.ncls;
  }

  // =============================== context encoder forward (hypernetwork.py:99-197) ===============================
  float* cx0 = cb.empty() ? cx_fin : cb[0].x_in;
  // tokens: [B][T][lang] . Wt + bt + pos_t  (rows 0..T-1 of each episode's [Sc][C] block)
  const int Kl = g.lang_dim;
  bgemm(st, false, false, with_bias(product(per_sample(in.tok, T, Kl), mat(Pm + L.w_tok, C), per_sample(cx0, Sc, C), T, C, Kl), Pm + L.b_tok), B);
  bgemm(st, false, false, with_bias(product(per_sample(cls, 1, E), mat(Pm + L.w_img, C), per_sample(cx0 + (long)T * C, Sc, C), 1, C, E), Pm + L.b_img), B);      // row T
  if (lt) KL(ctx_rows_tokens_kernel, g1((long)B * Sc * C), dim3(256), cx0, Pm + L.pos_tok, Pm + L.pos_img, Pm + L.pos_layer, B, T, NL, C);
  else KL(ctx_rows_kernel, g1((long)B * Sc * C), dim3(256), cx0, Pm + L.pos_tok, Pm + L.pos_img, Pm + L.pos_layer, B, T, C);
  for (int l = 0; l < g.ctx_layers; ++l)
    block_fwd(st, B, Sc, C, Hc, Fc, 0, bind(Pm, L.layer[l]), cb[l], l + 1 < g.ctx_layers ? cb[l + 1].x_in : cx_fin, t, ctx_opt);
  // ctx = LN_f(x[:, -1]) (/ sqrt(C)); rows gathered through a stride: x = cx_fin + (Sc-1)*C, row stride Sc*C
  if (lt) KL(ctx_final_tokens_fwd_kernel, dim3((B * NL + 3) / 4), dim3(256), cx_fin, Sc, NL, ctxn, cmean, crstd, Pm + L.norm_s, Pm + L.norm_b, ctx, B * NL, C, cpost);
  else KL(ctx_final_fwd_kernel, dim3((B + 3) / 4), dim3(256), cx_fin + (long)(Sc - 1) * C, (long)Sc * C, ctxn, cmean, crstd, Pm + L.norm_s, Pm + L.norm_b, ctx, B, C, cpost);
  if (cdrop.on()) dropout_fwd(st, cdrop, NOISE_CONTEXT, 0, ctx, nullptr, ctx, B, (long)NL * C);      // embedding_dropout_rate (hypernetwork.py:193-195)
  // =============================== theta = ctx W_cat + b_cat (hypernetwork.py:205-233) ===============================
  // layer tokens: theta[b, run] = ctx[b, token(run)] W_h[:, hcols(run)] + b_h[hcols(run)], every run in ONE grouped launch; the K order of
  // an element is C's ascending k steps whatever B and whatever the run's neighbours, so a row stays batch-invariant
  const long Gh = L.Gh;
  const int NLC = NL * C, wg = B >= 96 ? 1 : 0, wc = C >= 96 ? 1 : 0;                  // tile tables: [0] 64, [1] 128 columns (bgemm()'s rule on M)
  const int Gi = (int)G, Ghi = (int)Gh;
  if (lt) bgemm_groups(st, false, false, with_bias(product(mat(ctx, NLC), mat(Pm + L.wcat, Ghi), mat(tb.theta, Gi), B, Gi, C), Pm + L.bcat),
                       tg.fwd[wg], tg.ntiles[wg], wg ? 128 : 64, 1, tg.vec_ok, 2.0 * B * (double)G * C);
  else bgemm(st, false, false, with_bias(product(mat(ctx, C), mat(Pm + L.wcat, Gi), mat(tb.theta, Gi), B, Gi, C), Pm + L.bcat), 1);
  // =============================== policy forward with per-episode weights ===============================
  const float* TH = tb.theta;
  float* px0 = pb[0].x_in;
  // rows [0, Tl) = token_embedding_b Wl_b + bl_b, every position (base_vit.py:159-166 masks nothing); the patches follow at row Tl
  if (Tl) bgemm(st, false, false, with_bias(product(per_sample(in.tok, Tl, Kl), per_episode(TH + L.wl, D, G), per_sample(px0, S, D), Tl, D, Kl), TH + L.bl, G), B);
  bgemm(st, false, false, with_bias(product(per_episode(tokens, E, tok_stride), per_episode(TH + L.wp, D, G), per_sample(px0 + (long)Tl * D, S, D), P, D, E), TH + L.bp, G), B);
  KL(x0_finish_kernel, g1((long)B * S * D), dim3(256), px0, TH + L.pos, G, S, D, B);
  if (pdrop.on()) dropout_fwd(st, pdrop, NOISE_POLICY_INPUT, 0, px0, nullptr, px0, B, (long)S * D);      // base_vit.py:205
  for (int l = 0; l < g.L; ++l)
    block_fwd(st, B, S, D, H, F, G, bind(TH, L.pol[l]), pb[l], l + 1 < g.L ? pb[l + 1].x_in : px_fin, t, pol_at(l));
  // =============================== head + loss (+ backward seed) ===============================
  ENQ(hipMemsetAsync, pdx, 0, (size_t)B * S * D * 4, st);
  HeadP hpp{px_fin, (long)S * D, TH, tb.dtheta, G, (int)L.wc, (int)L.bc, (int)L.wd, (int)L.bd, (int)L.ns, (int)L.nb, in.target, in.tmask, in.amask,
            tb.loss, hp.forward_only ? nullptr : dxrow, tb.actions, tb.logits, B, S, D, g.horizon, g.action_dim, g.tanh_scale, g.max_action, g.clip_target};
  KL(head_loss_kernel, dim3(B), dim3(64), hpp);
  // hvla_train_attention_losses: the last layer's action row, [B][H][S][Sp] like t.dp (block_fwd / block_bwd)
  const int Sp = score_stride(S);
  AuxP auxp{pb[g.L - 1].p, nullptr, score_floats(H, S), (long)S * Sp, S, Sp, H, P, aux.w_ent, aux.w_align, aux.w_align > 0.f ? aux.ref : nullptr,
            tb.loss, aux.ent, aux.align, 1.f / (float)B};
  if (aux.on()) KL(attention_aux_kernel, dim3(B), dim3(256), auxp);
  if (hp.forward_only) return hipGetLastError();
  auxp.dp = t.dp;
  KL(add_strided_kernel, g1((long)B * D), dim3(256), pdx + (long)(S - 1) * D, (long)S * D, dxrow, (long)D, B);
  // =============================== policy backward ===============================
  for (int l = g.L - 1; l >= 0; --l)
    block_bwd(st, B, S, D, H, F, G, G, bind(TH, L.pol[l]), bind(tb.dtheta, L.pol[l]), pb[l], pdx, t, pol_at(l), aux.on() && l == g.L - 1 ? &auxp : nullptr);
  // x0 = [tok Wl + bl ; tokens Wp + bp ; 0] + pos : dpos = dx0, dbp = sum of the P patch rows of dx0, dWp = tokens^T dx0[Tl : Tl + P]
  if (pdrop.on()) dropout_bwd(st, pdrop, NOISE_POLICY_INPUT, 0, pdx, pdx, B, (long)S * D);
  const float* pdx_patch = pdx + (long)Tl * D;
  KL(add_strided_kernel, g1((long)B * S * D), dim3(256), tb.dtheta + L.pos, G, pdx, (long)S * D, B);
  if (g.differential) KL(colsum_episode_kernel, dim3((D + 63) / 64, B), dim3(256), pdx_patch, tb.dtheta + L.bp, G, S, P, D);
  else KL(colsum_kernel, dim3((D + 63) / 64, B, (P + 63) / 64), dim3(64), pdx_patch, tb.dtheta + L.bp, G, S, P, D, B);
  bgemm(st, true, false, product(per_episode(tokens, E, tok_stride), per_sample(pdx_patch, S, D), per_episode(tb.dtheta + L.wp, D, G), E, D, P, Store::Add), B);
  if (Tl) {     // dbl = sum of the language rows, dWl = tok^T dx0[:Tl]; nothing flows into token_embedding (T5 is frozen)
    KL(colsum_kernel, dim3((D + 63) / 64, B, (Tl + 63) / 64), dim3(64), pdx, tb.dtheta + L.bl, G, S, Tl, D, B);
    bgemm(st, true, false, product(per_sample(in.tok, Tl, Kl), per_sample(pdx, S, D), per_episode(tb.dtheta + L.wl, D, G), Kl, D, Tl, Store::Add), B);
  }
  // =============================== DINOv2 backward ===============================
  if (enc) {
    // d tokens_b = (the patch rows of dx0_b) Wp_b^T -> rows 1.. of the final-LayerNorm output gradient (CLS row gets none)
    float* dh = t.y;                                                      // [B][Se][E]; t.y is free between blocks
    ENQ(hipMemsetAsync, dh, 0, (size_t)B * Se * E * 4, st);
    bgemm(st, false, true, product(per_sample(pdx_patch, S, D), per_episode(TH + L.wp, D, G), per_sample(dh + E, Se, E), P, E, D), B);
    float* edx = pl.edx;
    KL(ln_bwd_kernel, dim3((B * Se + 3) / 4), dim3(256), pl.ex_fin, dh, pl.emean, pl.erstd, Pe + L.e_lns, edx, (float*)nullptr, (float*)nullptr, 0, B * Se, Se, E, 0);
    KL(ln_pgrad_kernel, dim3((E + 63) / 64, (B * Se + 63) / 64), dim3(64), pl.ex_fin, dh, pl.emean, pl.erstd, Ge + L.e_lns, Ge + L.e_lnb, B * Se, E);
    for (int l = g.enc_layers - 1; l >= 0; --l)
      block_bwd(st, B, Se, E, He, Fe, 0, 0, bind(Pe, L.enc[l]), bind(Ge, L.enc[l]), eb[l], edx, t, enc_opt);
    // x0[b][0] = cls + pos[0]; x0[b][1+t] = patch_t Wk + bk + pos[1+t]
    KL(colsum_kernel, dim3((Se * E + 63) / 64, 1, (B + 63) / 64), dim3(64), edx, Ge + L.e_pos, 0, B, B, Se * E, 1);       // dpos = sum_b dx0
    ENQ(hipMemcpyAsync, Ge + L.e_cls, Ge + L.e_pos, (size_t)E * 4, hipMemcpyDeviceToDevice, st);                          // dcls = dpos[0]
    KL(colsum_kernel, dim3((E + 63) / 64, 1, (P + 63) / 64), dim3(64), Ge + L.e_pos + E, Ge + L.e_pb, 0, P, P, E, 1);     // dbias = sum_{t>=1} dpos[t]
    bgemm(st, true, false, product(per_sample(pl.patches, P, Kp), per_sample(edx + E, Se, E), mat(Ge + L.e_pk, E), Kp, E, P, Store::Atomic), B);
    if (src_on) {                                                        // dsource = A^T dslot; the slot is no parameter: its gradient is zero
      ENQ(launch_position_adjoint, Ge + L.e_pos, ps.n, ps.w, Ge + L.enc_total, ps.grid, E, st);
      ENQ(hipMemsetAsync, Ge + L.e_pos, 0, (size_t)Se * E * 4, st);
    }
    if (bucket_done) ENQ(hipEventRecord, bucket_done[0], st);           // the shared DINOv2 leaves are final
  }
  // =============================== weight generation backward ===============================
  // hvla_train_frozen: a bucket declared frozen is not computed -- its range of `grads` stays the zeros of the memset above, its
  // event is recorded where it always is.  dtheta is complete here whatever is frozen.
  const bool heads_on = !(frozen_buckets & 2), ctx_on = !(frozen_buckets & 4);
  if (heads_on && lt) {
    // dW_h[:, hcols] += ctx[:, token]^T dtheta[:, run] and db_h[hcols] += sum_b dtheta[b, run], a grouped launch each; with shared heads
    // the L blocks' runs meet in one head: a real sum, by atomics (the range is the memset's zero)
    bgemm_groups(st, true, false, product(mat(ctx, NLC), mat(tb.dtheta, Gi), mat(Gm + L.wcat, Ghi), C, Gi, B, g.shared_block_heads ? Store::Atomic : Store::Add),
                 tg.dw[wc], tg.ntiles[wc], wc ? 128 : 64, 1, tg.vec_ok, 2.0 * B * (double)G * C);
    KL(colsum_groups_kernel, dim3(tg.ntiles[0], 1, (B + 63) / 64), dim3(64), tb.dtheta, G, Gm + L.bcat, tg.fwd[0], B);
  } else if (heads_on) {
    bgemm(st, true, false, product(mat(ctx, C), mat(tb.dtheta, Gi), mat(Gm + L.wcat, Gi), C, Gi, B, Store::Add), 1);                            // dW_cat = ctx^T dtheta
    KL(colsum_kernel, dim3((unsigned)((G + 63) / 64), 1, (B + 63) / 64), dim3(64), tb.dtheta, Gm + L.bcat, 0, B, B, (int)G, 1);                  // db_cat
  }
  if (ctx_on && lt) {
    // dctx[b, token] = dtheta[b, run] W_h[:, hcols]^T: split-K over the runs' K chunks in one grouped launch; nothing reads token 0,
    // whose rows stay the memset's zero
    ENQ(hipMemsetAsync, dctx, 0, (size_t)B * NLC * 4, st);
    const int td = B >= 96 && C >= 96 ? 128 : 64;
    bgemm_groups(st, false, true, product(mat(tb.dtheta, Gi), mat(Pm + L.wcat, Ghi), mat(dctx, NLC), B, C, Gi, Store::Atomic),
                 tg.dctx, tg.ndctx, td, (C + td - 1) / td, tg.vec_ok, 2.0 * B * (double)G * C);
    if (cdrop.on()) dropout_bwd(st, cdrop, NOISE_CONTEXT, 0, dctx, dctx, B, (long)NLC);
  } else if (ctx_on) {
    ENQ(hipMemsetAsync, dctx, 0, (size_t)B * C * 4, st);
    // dctx = dtheta W_cat^T: [B, G] x [G, C], a K = 201 500 product onto a B x C output -> split-K over the whole chip
    bgemm(st, false, true, product(mat(tb.dtheta, Gi), mat(Pm + L.wcat, Gi), mat(dctx, C), B, C, Gi, Store::AddSplitK), 1);
    if (cdrop.on()) dropout_bwd(st, cdrop, NOISE_CONTEXT, 0, dctx, dctx, B, C);
  }
  if (bucket_done) ENQ(hipEventRecord, bucket_done[1], st);             // W_cat, b_cat are final
  // =============================== context encoder backward ===============================
  if (ctx_on) {
    ENQ(hipMemsetAsync, cdx, 0, (size_t)B * Sc * C * 4, st);
    if (lt) KL(ctx_final_tokens_bwd_kernel, dim3((B * NL + 3) / 4), dim3(256), cx_fin, Sc, NL, dctx, cmean, crstd, Pm + L.norm_s, cdx, Gm + L.norm_s, Gm + L.norm_b, B * NL, C, cpost);
    else KL(ctx_final_bwd_kernel, dim3((B + 3) / 4), dim3(256), cx_fin + (long)(Sc - 1) * C, (long)Sc * C, dctx, cmean, crstd, Pm + L.norm_s, cdx + (long)(Sc - 1) * C, Gm + L.norm_s, Gm + L.norm_b, B, C, cpost);
    for (int l = g.ctx_layers - 1; l >= 0; --l)
      block_bwd(st, B, Sc, C, Hc, Fc, 0, 0, bind(Pm, L.layer[l]), bind(Gm, L.layer[l]), cb[l], cdx, t, ctx_opt);
    // inputs: tokens rows -> w_tok, b_tok, pos_tok ; image row -> w_img, b_img, pos_img ; layer row -> pos_layer
    if (lt) KL(ctx_rows_tokens_bwd_kernel, g1((long)B * Sc * C), dim3(256), cdx, Gm + L.pos_tok, Gm + L.pos_img, Gm + L.pos_layer, Gm + L.b_tok, Gm + L.b_img, B, T, NL, C);
    else KL(ctx_rows_bwd_kernel, g1((long)B * Sc * C), dim3(256), cdx, Gm + L.pos_tok, Gm + L.pos_img, Gm + L.pos_layer, Gm + L.b_tok, Gm + L.b_img, B, T, C);
    bgemm(st, true, false, product(per_sample(in.tok, T, Kl), per_sample(cdx, Sc, C), mat(Gm + L.w_tok, C), Kl, C, T, Store::Atomic), B);
    bgemm(st, true, false, product(per_sample(cls, 1, E), per_sample(cdx + (long)T * C, Sc, C), mat(Gm + L.w_img, C), E, C, 1, Store::Atomic), B);
  }
  if (bucket_done) ENQ(hipEventRecord, bucket_done[2], st);             // the context encoder's leaves: everything is final
  return hipGetLastError();
}

// the clip's squared norm of grads[0, n) into tb.sqsum: one global norm over both optimizer groups, under hvla_train_frozen over
// the trainable elements
static void launch_sqsum(hipStream_t st, const TrainBuffers& tb, const uint8_t* frozen, long n) {
  ENQ(hipMemsetAsync, tb.sqsum, 0, 4, st);
  if (frozen) KL(sqsum_frozen_kernel, dim3(1024), dim3(256), tb.grads, frozen, n, tb.sqsum);
  else KL(sqsum_kernel, dim3(1024), dim3(256), tb.grads, n, tb.sqsum);
}
// one optimizer group, elements [off, off + cnt) of the training vector: the hypernetwork's at (lr, weight_decay), or the shared
// DINOv2 leaves' (and the position source's) at (base_lr, base_weight_decay) with the pull towards params0
static void launch_adamw(hipStream_t st, const TrainBuffers& tb, const TrainHyper& hp, const uint8_t* frozen, bool shared, long off, long cnt,
                         float bc1, float bc2) {
  float* const p = tb.params + off;
  const float* const g = tb.grads + off;
  __bf16* const mu = tb.mu + off;
  float* const nu = tb.nu + off;
  float* const ema = hp.ema_decay > 0.f ? tb.ema + off : nullptr;
  const uint8_t* const mask = tb.wd_mask ? tb.wd_mask + off : nullptr;
  const float* const p0 = shared ? tb.params0 : nullptr;
  const float lr = shared ? hp.base_lr : hp.lr, wd = shared ? hp.base_weight_decay : hp.weight_decay;
  const dim3 grid(2048), block(256);
  if (frozen && shared) KL(adamw_frozen_kernel<true>, grid, block, p, g, mu, nu, ema, frozen + off, cnt, tb.sqsum, hp.clip, lr, hp.b1, hp.b2, hp.eps, wd, mask, p0, bc1, bc2, hp.ema_decay);
  else if (frozen) KL(adamw_frozen_kernel<false>, grid, block, p, g, mu, nu, ema, frozen + off, cnt, tb.sqsum, hp.clip, lr, hp.b1, hp.b2, hp.eps, wd, mask, p0, bc1, bc2, hp.ema_decay);
  else if (shared) KL(adamw_shared_kernel, grid, block, p, g, mu, nu, ema, cnt, tb.sqsum, hp.clip, lr, hp.b1, hp.b2, hp.eps, wd, mask, p0, bc1, bc2, hp.ema_decay);
  else KL(adamw_kernel, grid, block, p, g, mu, nu, ema, cnt, tb.sqsum, hp.clip, lr, hp.b1, hp.b2, hp.eps, wd, mask, bc1, bc2, hp.ema_decay);
}

hipError_t train_apply(const TrainLayout& L, const TrainBuffers& tb, const TrainHyper& hp, bool train_encoder, hipStream_t st,
                       const TrainOptions& opt) {
  const PosSource& ps = opt.ps;
  const long tail = train_encoder ? ps.tail() : 0;           // the position table's source (shared group; the slot's gradient is zero)
  launch_sqsum(st, tb, opt.frozen, train_vector_elems(L, ps, train_encoder));
  const float t = (float)(hp.step + 1);
  const float bc1 = 1.f - powf(hp.b1, t), bc2 = 1.f - powf(hp.b2, t);
  launch_adamw(st, tb, hp, opt.frozen, false, 0, L.total, bc1, bc2);
  if (train_encoder) launch_adamw(st, tb, hp, opt.frozen, true, L.total, L.enc_total + tail, bc1, bc2);
  if (tail) {                                                 // the derived slots follow their tails
    const long slot = L.total + L.e_pos, src = L.total + L.enc_total;
    ENQ(launch_position_interp, tb.params + src, ps.n, ps.w, tb.params + slot, ps.grid, ps.E, st);
    if (hp.ema_decay > 0.f && tb.ema) ENQ(launch_position_interp, tb.ema + src, ps.n, ps.w, tb.ema + slot, ps.grid, ps.E, st);
  }
  return hipGetLastError();
}

hipError_t train_accumulate(const TrainLayout& L, const TrainBuffers& tb, float* acc, float inv_k, const TrainHyper& hp,
                            bool train_encoder, hipStream_t st, const TrainOptions& opt) {
  const long n = train_vector_elems(L, opt.ps, train_encoder);
  launch_sqsum(st, tb, opt.frozen, n);
  KL(accumulate_kernel, dim3(2048), dim3(256), acc, tb.grads, n, tb.sqsum, hp.clip, inv_k);
  return hipGetLastError();
}


hipError_t train_noise_probe(const NoiseKey& key, float rate, bool normal, long n, float* out, hipStream_t st) {
  const Drop d(rate, key);
  KL(noise_probe_kernel, g1(n), dim3(256), out, n, key, d.thr, d.keep_prob, normal ? 1 : 0);
  return hipGetLastError();
}

}  // namespace hvla
