// noise.h — the counter-based generator of the fine-tune step's noise (hvla_train_noise): the reference's four
// train=True noise sources (vit_kwargs.dropout_rate base_vit.py:205 + transformer.py:67,74,192; vit_kwargs.image_embedding_noise
// base_vit.py:123-127; hypernet_kwargs.embedding_dropout_rate hypernetwork.py:193-195; hypernet_kwargs.image_dropout
// hypernetwork.py:119-122).  No state and no stored masks: a draw is a pure function of (seed, element, sample, site, draw), so the
// backward pass regenerates what the forward pass drew, and hypervla/train.py restates it in numpy bit for bit.  jax's threefry
// bits are not reproduced: the noise is equal to the reference's in distribution.
//
//   Philox4x32-10 (Salmon et al., SC'11; Random123's constants), key = (seed lo, seed hi),
//   counter = (element >> 2, sample_id, site, draw); element e takes word e & 3 of its block
//     sample_id  the sample's GLOBAL index sample_offset + b (low 32 bits), never its row in the call
//     site       kind | layer << 8, kinds below
//   dropout      keep iff (word >> 8) >= thr, thr = ceil(rate 2^24) (host, double); y = x / keep_prob (f32) or 0,
//                keep_prob = 1.0f - rate (flax divides)
//   normal       Box-Muller on the word pairs (w0, w1) and (w2, w3) of a block: u1 = ((w >> 8) + 1) 2^-24, u2 = (w' >> 8) 2^-24,
//                z0 = sqrt(-2 ln u1) cos(2 pi u2) for the pair's first element, z1 = sqrt(-2 ln u1) sin(2 pi u2) for its second
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HVLA_NOISE_FN __host__ __device__ inline
#else
#define HVLA_NOISE_FN inline
#endif

namespace hvla {

// the sites (per-sample shape; element index row-major over it)
enum NoiseKind : uint32_t {
  NOISE_POLICY_INPUT = 1,   // [S, dim]   x0 after + pos_embedding (base_vit.py:204-205), language prefix rows included
  NOISE_ATTN_OUT = 2,       // [S, dim]   layer l: attention branch behind the out-projection and bias (transformer.py:192)
  NOISE_MLP_HIDDEN = 3,     // [S, mlp]   layer l: behind the GELU (transformer.py:67)
  NOISE_MLP_OUT = 4,        // [S, dim]   layer l: MLP output in front of the residual add (transformer.py:74)
  NOISE_TOKENS = 5,         // [P, enc_dim] DINOv2 tokens + sigma z (base_vit.py:123-127)
  NOISE_CONTEXT = 6,        // [ctx_dim]  context embedding behind the scale_context division (hypernetwork.py:193-195)
  NOISE_IMAGE_CLS = 7,      // [enc_dim]  the initial image's CLS row (hypernetwork.py:119-122; only row 0 is read)
};

struct NoiseKey {
  uint32_t k0 = 0, k1 = 0;  // seed lo, hi
  uint32_t site = 0, draw = 0;
  long sample0 = 0;         // global index of row 0 of the call
};

struct PhiloxWords { uint32_t w[4]; };

HVLA_NOISE_FN uint32_t noise_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

HVLA_NOISE_FN PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = noise_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = noise_mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return PhiloxWords{{c0, c1, c2, c3}};
}

// the four words of block `blk` of sample row b
HVLA_NOISE_FN PhiloxWords noise_block(const NoiseKey& k, long b, uint32_t blk) {
  return philox4x32_10(blk, (uint32_t)(uint64_t)(k.sample0 + b), k.site, k.draw, k.k0, k.k1);
}

// thr = ceil(rate 2^24) in double: P(keep) = 1 - thr / 2^24
inline uint32_t dropout_threshold(float rate) { return (uint32_t)ceil((double)rate * 16777216.0); }

HVLA_NOISE_FN bool dropout_keep(uint32_t word, uint32_t thr) { return (word >> 8) >= thr; }

// the two normals of a word pair
HVLA_NOISE_FN void noise_box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
  const float u1 = (float)((wa >> 8) + 1u) * 5.9604644775390625e-08f, u2 = (float)(wb >> 8) * 5.9604644775390625e-08f;
  const float r = sqrtf(-2.f * logf(u1));
  float s, c;
#if defined(__HIP_DEVICE_COMPILE__)
  sincosf(6.283185307179586f * u2, &s, &c);
#else
  s = sinf(6.283185307179586f * u2);
  c = cosf(6.283185307179586f * u2);
#endif
  z0 = r * c;
  z1 = r * s;
}

}  // namespace hvla
