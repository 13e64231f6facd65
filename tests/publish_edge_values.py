"""Rounding edge values for the publish tests (tests/test_gpu_publish.py case 5, tests/test_publish_host.py): f32 numbers of
the form +-(2m+1) 2^-e chosen so that the two roundings of the packers meet their hard cases.

  fp16 ties        odd 12-bit integers: one bit more than binary16's 11 significant bits, exactly half way
  bf16 ties        odd 9-bit integers: one bit more than bfloat16's 8 (exact in binary16: the residue is zero)
  residue ties     A 2^13 + b (A 11 bits, b an odd 12-bit integer): rounds DOWN to A 2^13 in binary16 and leaves the
                   residue b, a binary16 tie only after the hi part is subtracted; A 2^10 + b (A 8 bits, b odd 9 bits) is
                   the same for bfloat16 (the W_cat hi / lo split and enc_dtype="bf16")
  small odds       1, 3, 5, 7: exact everywhere; at 2^-25 .. 2^-27 they round to zero or to the smallest subnormal

Every integer is placed at every binade 2^-27 .. 2^1 (values below 4, nothing overflows; from 2^-15 down binary16 is
subnormal, below 2^-25 it is zero), with both signs, and +-0 is added."""
import numpy as np

BINADES = range(-27, 2)          # floor(log2 |x|)


def _odd_integers():
    fp16_tie = [2049, 2051, 3071, 3073, 4093, 4095]
    bf16_tie = [257, 259, 383, 385, 509, 511]
    res16 = [a * 8192 + b for a in (1024, 1025, 1536, 2047) for b in (2049, 3071, 4095)]
    resbf = [a * 1024 + b for a in (128, 129, 192, 255) for b in (257, 385, 511)]
    return [1, 3, 5, 7] + fp16_tie + bf16_tie + res16 + resbf


def edge_values() -> np.ndarray:
    """f32 [n]: every odd integer of the families above at every binade, with alternating sign, then +0 and -0."""
    out = []
    for i, odd in enumerate(_odd_integers()):
        top = odd.bit_length() - 1
        for j, t in enumerate(BINADES):
            v = np.ldexp(np.float64(odd), t - top)           # (2m+1) 2^-e with e = top - t, in [2^t, 2^(t+1))
            out.append(-v if (i + j) & 1 else v)
    vals = np.asarray(out + [0.0, -0.0], np.float64)
    f = vals.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), vals)        # all exact in f32 (at most 24 significant bits, no f32 subnormal)
    return f


def edge_block(shape, offset: int = 0) -> np.ndarray:
    """A block of `shape` filled by cycling through the edge values from `offset` on."""
    v = edge_values()
    n = int(np.prod(shape))
    return v[(np.arange(n) + offset) % v.size].reshape(shape)


def overwrite_edge_blocks(params, g):
    """A copy of `params` with the deterministic blocks of case 5 overwritten: a 64 x 64 corner of encoder layer 0's query and
    fc1 kernels, a 128 x 64 block of one output head's kernel (the policy's first fc1), and 64 input rows x 64 channels of the
    patch kernel."""
    E, Fe = g.enc_dim, g.enc_mlp
    p = {k: np.array(v, np.float32, copy=True) for k, v in params.items()}
    L0 = "encoder_image_encoder_encoder_layer_0_"
    q = p[L0 + "attention_attention_query_kernel"].reshape(E, E)
    q[:64, :64] = edge_block((64, 64), 0)
    f1 = p[L0 + "mlp_fc1_kernel"].reshape(E, Fe)
    f1[:64, :64] = edge_block((64, 64), 7)
    head = p["output_head_encoder_Transformer_0_encoderblock_0_MlpBlock_0_Dense_0_kernel/kernel"]
    assert head.shape[0] == g.ctx_dim == 128
    head[:, :64] = edge_block((128, 64), 13)
    pk = p["encoder_image_encoder_embeddings_patch_embeddings_projection_kernel"].reshape(g.patch_in, E)
    pk[100:164, :64] = edge_block((64, 64), 29)
    p[L0 + "attention_attention_query_kernel"], p[L0 + "mlp_fc1_kernel"] = q.reshape(-1), f1.reshape(-1)
    p["encoder_image_encoder_embeddings_patch_embeddings_projection_kernel"] = pk.reshape(-1)
    return p
