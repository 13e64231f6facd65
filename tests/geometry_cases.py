"""The encoder geometries at the edges of hvla_create's contract (csrc/accept.h) and the two bases they vary,
shared by tests/test_gpu_geometry_contract.py (four stages against the oracle) and tests/test_gpu_hidden_state.py (the hidden state
with its CLS row at the same edges).  No GPU and no test here."""
import dataclasses

# The hidden state's bounds against the float64 oracle, from the table at the top of tests/test_gpu_parity.py: whole hidden state
# rms / max with f16 operands (the max also holds the CLS row alone) and rms with bf16 operands.  tests/test_oracle_properties.py
# checks on the CPU that HIDDEN_F16_MAX still sees a missing term of the last layer.
HIDDEN_F16_RMS, HIDDEN_F16_MAX, HIDDEN_BF16_RMS = 2e-3, 2e-2, 1.2e-2


def _mid(**kw):
    """MID (P = 64: policy_kernel<2>, the small-batch encoder forms), every layer count but the encoder's at 1 unless the case says."""
    from hypervla.config import MID
    return dataclasses.replace(MID, **{**dict(layers=1, ctx_layers=1), **kw})


def _full(**kw):
    """The README widths (P = 256: policy_kernel<8>, the action row spread over all waves) with one layer of each kind."""
    from hypervla.config import FULL
    return dataclasses.replace(FULL, **{**dict(enc_layers=1, layers=1, ctx_layers=1), **kw})


ENCODER_P64 = {
    "E 256, mlp 640": dict(enc_dim=256, enc_heads=4, enc_mlp=640),
    "patch 16, image 128": dict(patch=16, image_size=128),
    "patch 4, image 32 (Kp = 128)": dict(patch=4, image_size=32),
}
ENCODER_P256 = {
    "E 256 (one column tile per image)": (dict(enc_dim=256, enc_heads=4, enc_mlp=1024), "f16"),
    "E 640, mlp 384": (dict(enc_dim=640, enc_heads=10, enc_mlp=384), "f16"),
    "E 1024, mlp 1152": (dict(enc_dim=1024, enc_heads=16, enc_mlp=1152, enc_layers=1), "f16"),
    "E 1024, mlp 1152, bf16": (dict(enc_dim=1024, enc_heads=16, enc_mlp=1152, enc_layers=1), "bf16"),
    "E 128, mlp 128 (only QKV on the aligned path)": (dict(enc_dim=128, enc_heads=2, enc_mlp=128), "f16"),
    "patch 8, image 128 (Kp = 384)": (dict(patch=8, image_size=128, enc_layers=1), "f16"),
    "patch 7, image 112": (dict(patch=7, image_size=112, enc_layers=1), "f16"),
    "no encoder layers": (dict(enc_layers=0), "f16"),
}
