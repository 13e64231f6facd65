"""ctypes binding of libhvla (include/hvla.h).  There is no CPU or eager fallback: if the HIP library
is missing or the device is not gfx950 every entry point raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np

_LIB_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib")
# HVLA_LIBRARY_FLAVOUR=bench: tools/ load libhvla_bench.so (the same sources with the hvla_debug_* timing hooks compiled in)
_LIB_PATH = os.path.join(_LIB_DIR, "libhvla_bench.so" if os.environ.get("HVLA_LIBRARY_FLAVOUR") == "bench" else "libhvla.so")

HVLA_ENC_F16, HVLA_ENC_BF16 = 0, 1
_ERRORS = {-1: "HVLA_E_SHAPE", -2: "HVLA_E_DTYPE", -3: "HVLA_E_DEVICE", -4: "HVLA_E_ARENA_FULL",
           -5: "HVLA_E_HIP", -6: "HVLA_E_WEIGHTS", -7: "HVLA_E_STATE"}

EXPORTS = ["hvla_create", "hvla_destroy", "hvla_last_error", "hvla_load_weights", "hvla_num_generated",
           "hvla_generate", "hvla_weights_free", "hvla_release_pooled_arenas", "hvla_weights_batch", "hvla_weights_export",
           "hvla_encode", "hvla_policy", "hvla_step", "hvla_ensemble_reset", "hvla_ensemble",
           "hvla_selftest", "hvla_profile", "hvla_profile_read", "hvla_loss",
           "hvla_train_sizes", "hvla_train_step", "hvla_train_apply", "hvla_encode_hidden", "hvla_t5_load",
           "hvla_t5_encode", "hvla_preprocess", "hvla_encode_audit", "hvla_train_accumulate", "hvla_train_bucket_ranges",
           "hvla_train_wait_bucket", "hvla_set_attention_outputs", "hvla_train_profile", "hvla_train_profile_read",
           "hvla_launches", "hvla_box_probe", "hvla_profile_select", "hvla_weights_alloc", "hvla_generate_slots",
           "hvla_step_slots", "hvla_ensemble_slots", "hvla_post_create", "hvla_post_free", "hvla_post_assign", "hvla_post_step",
           "hvla_create_with", "hvla_create_with_v2", "hvla_create_with_v3", "hvla_train_publish", "hvla_position_interp", "hvla_position_interp_adjoint",
           "hvla_train_position_source", "hvla_train_frozen", "hvla_train_attention_losses", "hvla_train_language_tokens",
           "hvla_weights_import", "hvla_weights_import_slots", "hvla_weights_copy_slots",
           "hvla_loss_terms", "hvla_train_metrics", "hvla_train_noise_set", "hvla_train_noise_probe", "hvla_train_differential",
           "hvla_create_with_v4", "hvla_num_layer_tokens", "hvla_train_layer_tokens",
           "hvla_train_context_rows"]
# hvla_train_metrics (include/hvla.h): select bits, the slots of its output vector, the size of its scratch
HVLA_METRICS_PRE, HVLA_METRICS_UPDATE = 1, 2
(HVLA_METRIC_TRAINING_LOSS, HVLA_METRIC_CONTINUOUS_LOSS, HVLA_METRIC_GRIPPER_LOSS, HVLA_METRIC_MSE, HVLA_METRIC_BASE_PARAMS_NORM,
 HVLA_METRIC_ATTENTION_ENTROPY, HVLA_METRIC_ATTENTION_ALIGNMENT) = range(7)
HVLA_METRIC_LOCAL_N = 7
HVLA_METRIC_GRAD_NORM, HVLA_METRIC_PARAM_NORM, HVLA_METRIC_UPDATE_NORM = 7, 8, 9      # + 2 n_tasks
HVLA_METRIC_N = 10
HVLA_TRAIN_METRICS_WORKGROUPS, HVLA_TRAIN_METRICS_MAX_BATCH = 1024, 4096
HVLA_TRAIN_METRICS_SCRATCH_DOUBLES = 4 * HVLA_TRAIN_METRICS_WORKGROUPS + 8 + 3 * HVLA_TRAIN_METRICS_MAX_BATCH
HVLA_POST_DIM = 7
HVLA_NORM_NORMAL, HVLA_NORM_BOUNDS = 0, 1
HVLA_SETUP_LIBERO, HVLA_SETUP_WIDOWX_BRIDGE, HVLA_SETUP_GOOGLE_ROBOT = 0, 1, 2
PROF_NAMES = ["patch_embed", "layernorm", "qkv_gemm", "attention", "out_gemm", "fc1_gemm", "fc2_gemm", "policy",
              "small_row_gemms"]      # mean rows + the 2 B latency-bound rows per GEMM: CLS rows and weight-rounding compensation rows


class hvla_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32)] + \
               [(n, C.c_int32) for n in ("image_size", "patch", "enc_dim", "enc_layers", "enc_heads",
                                         "enc_mlp", "dim", "layers", "heads", "mlp", "horizon",
                                         "action_dim")] + \
               [("tanh_scale", C.c_float), ("max_action", C.c_float)] + \
               [(n, C.c_int32) for n in ("ctx_dim", "ctx_layers", "ctx_heads", "ctx_mlp", "lang_tokens",
                                         "lang_dim", "scale_context", "max_batch", "enc_dtype", "streams", "clip_target")]


class hvla_policy_options(C.Structure):
    """Model options outside hvla_config (include/hvla.h): struct_size must be sizeof(hvla_policy_options)."""
    _fields_ = [("struct_size", C.c_uint32), ("use_language_token", C.c_int32)]


class hvla_policy_options_v2(C.Structure):
    """hvla_policy_options with attention_mask_as_bias, for hvla_create_with_v2 (include/hvla.h): struct_size must be its sizeof."""
    _fields_ = [("struct_size", C.c_uint32), ("use_language_token", C.c_int32), ("attention_mask_as_bias", C.c_int32)]


class hvla_policy_options_v3(C.Structure):
    """hvla_policy_options_v2 with differential_attention, for hvla_create_with_v3 (include/hvla.h): struct_size must be its sizeof."""
    _fields_ = [("struct_size", C.c_uint32), ("use_language_token", C.c_int32), ("attention_mask_as_bias", C.c_int32),
                ("differential_attention", C.c_int32)]


class hvla_policy_options_v4(C.Structure):
    """hvla_policy_options_v3 with layer_tokens and shared_block_heads, for hvla_create_with_v4 (include/hvla.h): struct_size must be its sizeof."""
    _fields_ = [("struct_size", C.c_uint32), ("use_language_token", C.c_int32), ("attention_mask_as_bias", C.c_int32),
                ("differential_attention", C.c_int32), ("layer_tokens", C.c_int32), ("shared_block_heads", C.c_int32)]


class hvla_tensor_desc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("numel", C.c_int64)]


class hvla_t5_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab", "d_model", "d_kv", "heads", "d_ff", "layers", "buckets", "max_distance")] + \
               [("eps", C.c_float), ("max_tokens", C.c_int32), ("max_batch", C.c_int32)]


class hvla_train_buffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("params", "grads", "mu", "nu", "ema", "theta", "dtheta", "work", "loss",
                                          "actions", "logits", "sqsum", "wd_mask", "params0")]


class hvla_train_hyper(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("lr", "b1", "b2", "eps", "weight_decay", "clip", "ema_decay")] + \
               [("step", C.c_int32), ("forward_only", C.c_int32), ("base_lr", C.c_float),
                ("base_weight_decay", C.c_float), ("train_encoder", C.c_int32)]


class hvla_train_attention(C.Structure):
    """Options of hvla_train_attention_losses (include/hvla.h): struct_size must be sizeof(hvla_train_attention)."""
    _fields_ = [("struct_size", C.c_uint32), ("entropy_weight", C.c_float), ("alignment_weight", C.c_float),
                ("reference_map", C.c_void_p), ("entropy", C.c_void_p), ("alignment", C.c_void_p)]


class hvla_train_noise(C.Structure):
    """Options of hvla_train_noise_set (include/hvla.h): struct_size must be sizeof(hvla_train_noise)."""
    _fields_ = [("struct_size", C.c_uint32), ("policy_dropout", C.c_float), ("image_embedding_noise", C.c_float),
                ("context_dropout", C.c_float), ("image_dropout", C.c_float), ("seed", C.c_uint64), ("sample_offset", C.c_int64),
                ("draw", C.c_uint32)]


class hvla_train_metrics_in(C.Structure):
    """Inputs of hvla_train_metrics (include/hvla.h): struct_size must be sizeof(hvla_train_metrics_in)."""
    _fields_ = [("struct_size", C.c_uint32), ("select", C.c_uint32), ("prev_params", C.c_void_p), ("target", C.c_void_p),
                ("timestep_mask", C.c_void_p), ("action_mask", C.c_void_p), ("task_ids", C.c_void_p), ("n_tasks", C.c_int32),
                ("entropy", C.c_void_p), ("alignment", C.c_void_p), ("encoder_sqsum", C.c_double), ("scratch", C.c_void_p)]


class hvla_post_row(C.Structure):
    """One row of hvla_post_step's caller-owned table (include/hvla.h)."""
    _fields_ = [("normalization", C.c_int32), ("setup", C.c_int32), ("p0", C.c_double * HVLA_POST_DIM),
                ("p1", C.c_double * HVLA_POST_DIM), ("mask", C.c_uint8 * HVLA_POST_DIM)]


_lib = None


def lib_path() -> str:
    return _LIB_PATH


def load_library():
    """dlopen libhvla.so and declare every prototype of include/hvla.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(f"libhvla.so not built at {_LIB_PATH}: run `python -c 'import __graft_entry__ as g; "
                           f"g.build()'` (make -C hyper-vla_amd/csrc). There is no CPU fallback.")
    lib = C.CDLL(_LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.hvla_create.argtypes = [C.POINTER(hvla_config), C.c_int, C.POINTER(vp)]
    lib.hvla_create.restype = C.c_int
    lib.hvla_create_with.argtypes = [C.POINTER(hvla_config), C.POINTER(hvla_policy_options), C.c_int, C.POINTER(vp)]
    lib.hvla_create_with.restype = C.c_int
    lib.hvla_create_with_v2.argtypes = [C.POINTER(hvla_config), C.POINTER(hvla_policy_options_v2), C.c_int, C.POINTER(vp)]
    lib.hvla_create_with_v2.restype = C.c_int
    lib.hvla_create_with_v3.argtypes = [C.POINTER(hvla_config), C.POINTER(hvla_policy_options_v3), C.c_int, C.POINTER(vp)]
    lib.hvla_create_with_v3.restype = C.c_int
    lib.hvla_create_with_v4.argtypes = [C.POINTER(hvla_config), C.POINTER(hvla_policy_options_v4), C.c_int, C.POINTER(vp)]
    lib.hvla_create_with_v4.restype = C.c_int
    lib.hvla_num_layer_tokens.argtypes = [vp]
    lib.hvla_num_layer_tokens.restype = i32
    lib.hvla_destroy.argtypes = [vp]
    lib.hvla_destroy.restype = None
    lib.hvla_last_error.argtypes = [vp]
    lib.hvla_last_error.restype = C.c_char_p
    lib.hvla_load_weights.argtypes = [vp, C.POINTER(hvla_tensor_desc), i32]
    lib.hvla_load_weights.restype = C.c_int
    lib.hvla_num_generated.argtypes = [vp]
    lib.hvla_num_generated.restype = i64
    lib.hvla_generate.argtypes = [vp, vp, vp, vp, i32, C.POINTER(vp), vp]
    lib.hvla_generate.restype = C.c_int
    lib.hvla_weights_free.argtypes = [vp, vp]
    lib.hvla_weights_free.restype = C.c_int
    lib.hvla_release_pooled_arenas.argtypes = [vp]
    lib.hvla_release_pooled_arenas.restype = C.c_int
    lib.hvla_weights_batch.argtypes = [vp]
    lib.hvla_weights_batch.restype = i32
    lib.hvla_launches.argtypes = [vp]
    lib.hvla_launches.restype = i64
    lib.hvla_box_probe.argtypes = [vp, C.POINTER(C.c_float), vp]
    lib.hvla_box_probe.restype = C.c_int
    lib.hvla_weights_export.argtypes = [vp, vp, vp, vp, vp]
    lib.hvla_weights_export.restype = C.c_int
    lib.hvla_encode.argtypes = [vp, vp, vp, i32, vp]
    lib.hvla_encode.restype = C.c_int
    lib.hvla_encode_hidden.argtypes = [vp, vp, vp, i32, vp]
    lib.hvla_encode_hidden.restype = C.c_int
    lib.hvla_preprocess.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
    lib.hvla_preprocess.restype = C.c_int
    lib.hvla_t5_load.argtypes = [vp, C.POINTER(hvla_t5_config), C.POINTER(hvla_tensor_desc), i32]
    lib.hvla_t5_load.restype = C.c_int
    lib.hvla_t5_encode.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    lib.hvla_t5_encode.restype = C.c_int
    lib.hvla_policy.argtypes = [vp, vp, vp, vp, vp, i32, vp]
    lib.hvla_policy.restype = C.c_int
    lib.hvla_step.argtypes = [vp, vp, vp, vp, vp, i32, vp]
    lib.hvla_step.restype = C.c_int
    lib.hvla_ensemble_reset.argtypes = [vp, vp, vp]
    lib.hvla_ensemble_reset.restype = C.c_int
    lib.hvla_ensemble.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.hvla_ensemble.restype = C.c_int
    lib.hvla_loss.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.hvla_loss.restype = C.c_int
    lib.hvla_loss_terms.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.hvla_loss_terms.restype = C.c_int
    lib.hvla_train_metrics.argtypes = [vp, C.POINTER(hvla_train_buffers), C.POINTER(hvla_train_metrics_in), vp, i32, i32, vp]
    lib.hvla_train_metrics.restype = C.c_int
    lib.hvla_train_sizes.argtypes = [vp, i32, i32, C.POINTER(i64)]
    lib.hvla_train_sizes.restype = C.c_int
    lib.hvla_train_step.argtypes = [vp, C.POINTER(hvla_train_buffers), vp, vp, vp, vp, vp, vp, vp, vp, i32,
                                    C.POINTER(hvla_train_hyper), vp]
    lib.hvla_train_step.restype = C.c_int
    lib.hvla_train_apply.argtypes = [vp, C.POINTER(hvla_train_buffers), C.POINTER(hvla_train_hyper), vp]
    lib.hvla_train_accumulate.argtypes = [vp, C.POINTER(hvla_train_buffers), vp, C.c_float, C.POINTER(hvla_train_hyper), vp]
    lib.hvla_train_accumulate.restype = C.c_int
    lib.hvla_train_publish.argtypes = [vp, vp, i64, i32, vp]
    lib.hvla_train_publish.restype = C.c_int
    lib.hvla_position_interp.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.hvla_position_interp.restype = C.c_int
    lib.hvla_position_interp_adjoint.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.hvla_position_interp_adjoint.restype = C.c_int
    lib.hvla_train_position_source.argtypes = [vp, i32, vp]
    lib.hvla_train_position_source.restype = C.c_int
    lib.hvla_train_frozen.argtypes = [vp, vp, i64, i32]
    lib.hvla_train_frozen.restype = C.c_int
    lib.hvla_train_attention_losses.argtypes = [vp, C.POINTER(hvla_train_attention)]
    lib.hvla_train_attention_losses.restype = C.c_int
    lib.hvla_train_language_tokens.argtypes = [vp, i32]
    lib.hvla_train_language_tokens.restype = C.c_int
    lib.hvla_train_differential.argtypes = [vp, i32]
    lib.hvla_train_differential.restype = C.c_int
    lib.hvla_train_layer_tokens.argtypes = [vp, i32]
    lib.hvla_train_layer_tokens.restype = C.c_int
    lib.hvla_train_context_rows.argtypes = [vp, i32, i32, C.POINTER(C.c_int64)]
    lib.hvla_train_context_rows.restype = C.c_int
    lib.hvla_train_noise_set.argtypes = [vp, vp]
    lib.hvla_train_noise_set.restype = C.c_int
    lib.hvla_train_noise_probe.argtypes = [vp, C.c_uint32, i64, i64, vp, vp]
    lib.hvla_train_noise_probe.restype = C.c_int
    lib.hvla_train_bucket_ranges.argtypes = [vp, i32, C.POINTER(C.c_int64)]
    lib.hvla_train_bucket_ranges.restype = C.c_int
    lib.hvla_train_wait_bucket.argtypes = [vp, i32, vp]
    lib.hvla_train_wait_bucket.restype = C.c_int
    lib.hvla_train_profile.argtypes = [vp, i32]
    lib.hvla_train_profile.restype = C.c_int
    lib.hvla_train_profile_read.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(i32)]
    lib.hvla_train_profile_read.restype = C.c_int
    lib.hvla_train_apply.restype = C.c_int
    lib.hvla_profile.argtypes = [vp, i32]
    lib.hvla_profile.restype = C.c_int
    lib.hvla_profile_select.argtypes = [vp, C.c_uint32]
    lib.hvla_profile_select.restype = C.c_int
    lib.hvla_profile_read.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(i32)]
    lib.hvla_profile_read.restype = C.c_int
    lib.hvla_encode_audit.argtypes = [vp, vp, i32, C.POINTER(C.c_float), C.POINTER(i32), vp]
    lib.hvla_encode_audit.restype = C.c_int
    lib.hvla_set_attention_outputs.argtypes = [vp, vp, vp]
    lib.hvla_set_attention_outputs.restype = C.c_int
    lib.hvla_weights_alloc.argtypes = [vp, i32, C.POINTER(vp), vp]
    lib.hvla_weights_alloc.restype = C.c_int
    lib.hvla_generate_slots.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    lib.hvla_generate_slots.restype = C.c_int
    lib.hvla_step_slots.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    lib.hvla_step_slots.restype = C.c_int
    lib.hvla_ensemble_slots.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.hvla_ensemble_slots.restype = C.c_int
    lib.hvla_weights_import.argtypes = [vp, vp, vp, vp, i32, C.POINTER(vp), vp]
    lib.hvla_weights_import.restype = C.c_int
    lib.hvla_weights_import_slots.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    lib.hvla_weights_import_slots.restype = C.c_int
    lib.hvla_weights_copy_slots.argtypes = [vp, vp, vp, vp, vp, i32, vp]
    lib.hvla_weights_copy_slots.restype = C.c_int
    lib.hvla_post_create.argtypes = [vp, i32, C.POINTER(vp), vp]
    lib.hvla_post_create.restype = C.c_int
    lib.hvla_post_free.argtypes = [vp, vp]
    lib.hvla_post_free.restype = C.c_int
    lib.hvla_post_assign.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    lib.hvla_post_assign.restype = C.c_int
    lib.hvla_post_step.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, vp]
    lib.hvla_post_step.restype = C.c_int
    lib.hvla_selftest.argtypes = [vp, vp]
    lib.hvla_selftest.restype = C.c_int
    _lib = lib
    return lib


class NativeError(RuntimeError):
    pass


class Context:
    """One hvla_ctx (one device)."""

    def __init__(self, geometry, device: int = 0, max_batch: int = 256, enc_dtype: str = "f16", streams: int = 1):
        self.lib = load_library()
        g = geometry
        if enc_dtype not in ("f16", "bf16"):
            raise ValueError("enc_dtype must be 'f16' or 'bf16'")
        self.cfg = hvla_config(C.sizeof(hvla_config), g.image_size, g.patch, g.enc_dim, g.enc_layers, g.enc_heads, g.enc_mlp,
                               g.dim, g.layers, g.heads, g.mlp, g.horizon, g.action_dim,
                               g.tanh_scale, g.max_action, g.ctx_dim, g.ctx_layers, g.ctx_heads, g.ctx_mlp,
                               g.lang_tokens, g.lang_dim, int(g.scale_context), int(max_batch),
                               HVLA_ENC_BF16 if enc_dtype == "bf16" else HVLA_ENC_F16, int(streams),
                               int(getattr(g, "clip_target", True)))
        self.geometry, self.device, self.max_batch, self.enc_dtype = g, device, max_batch, enc_dtype
        h = C.c_void_p()
        lang, mab = bool(getattr(g, "lang_in_policy", False)), bool(getattr(g, "mask_as_bias", False))
        diff = bool(getattr(g, "differential", False))
        if bool(getattr(g, "layer_tokens", False)):   # share_layer_index=False: the newest options struct and its entry
            self.options = hvla_policy_options_v4(C.sizeof(hvla_policy_options_v4), int(lang), int(mab), int(diff), 1,
                                                  int(bool(getattr(g, "shared_block_heads", False))))
            rc = self.lib.hvla_create_with_v4(C.byref(self.cfg), C.byref(self.options), device, C.byref(h))
        elif diff:            # use_differential_transformer: the newest options struct and its entry
            self.options = hvla_policy_options_v3(C.sizeof(hvla_policy_options_v3), int(lang), int(mab), 1)
            rc = self.lib.hvla_create_with_v3(C.byref(self.cfg), C.byref(self.options), device, C.byref(h))
        elif mab:             # return_attention_map: the larger options struct has an entry of its own (both sizes are ABI)
            self.options = hvla_policy_options_v2(C.sizeof(hvla_policy_options_v2), int(lang), 1)
            rc = self.lib.hvla_create_with_v2(C.byref(self.cfg), C.byref(self.options), device, C.byref(h))
        elif lang:            # use_language_token: the options struct (hvla_config's size is ABI)
            self.options = hvla_policy_options(C.sizeof(hvla_policy_options), 1)
            rc = self.lib.hvla_create_with(C.byref(self.cfg), C.byref(self.options), device, C.byref(h))
        else:
            rc = self.lib.hvla_create(C.byref(self.cfg), device, C.byref(h))
        if rc != 0:
            why = self.lib.hvla_last_error(None)
            why = why.decode() if why and why != b"null ctx" else ("geometry outside the hand-written kernels' specialisation, "
                                                                   f"or device {device} is not a gfx950 GPU")
            raise NativeError(f"hvla_create failed: {_ERRORS.get(rc, rc)} ({why})")
        self.h = h

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.hvla_last_error(self.h)
            raise NativeError(f"{what}: {_ERRORS.get(rc, rc)}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.hvla_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_generated(self) -> int:
        return int(self.lib.hvla_num_generated(self.h))

    @property
    def num_layer_tokens(self) -> int:
        return int(self.lib.hvla_num_layer_tokens(self.h))

    def load_weights(self, params: Dict[str, np.ndarray]):
        keep = []
        descs = (hvla_tensor_desc * len(params))()
        for i, (k, v) in enumerate(params.items()):
            a = np.ascontiguousarray(np.asarray(v), dtype=np.float32)
            keep.append(a)
            descs[i] = hvla_tensor_desc(k.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), a.size)
        self._check(self.lib.hvla_load_weights(self.h, descs, len(params)), "hvla_load_weights")

    def t5_load(self, t, params: Dict[str, np.ndarray], max_tokens: int, max_batch: int):
        keep = []
        descs = (hvla_tensor_desc * len(params))()
        for i, (k, v) in enumerate(params.items()):
            a = np.ascontiguousarray(np.asarray(v), dtype=np.float32)
            keep.append(a)
            descs[i] = hvla_tensor_desc(k.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), a.size)
        cfg = hvla_t5_config(t.vocab, t.d_model, t.d_kv, t.heads, t.d_ff, t.layers, t.buckets, t.max_distance, t.eps,
                             max_tokens, max_batch)
        self._check(self.lib.hvla_t5_load(self.h, C.byref(cfg), descs, len(params)), "hvla_t5_load")

    def preprocess(self, src_ptr, B, H, W, crop, dst_ptr, stream=0, padded_resize=False):
        flags = (1 if crop else 0) | (2 if padded_resize else 0)          # HVLA_PREPROCESS_CROP | HVLA_PREPROCESS_PAD
        self._check(self.lib.hvla_preprocess(self.h, src_ptr, B, H, W, flags, dst_ptr, C.c_void_p(stream)), "hvla_preprocess")

    def t5_encode(self, ids_ptr, mask_ptr, out_ptr, B, T, stream=0):
        self._check(self.lib.hvla_t5_encode(self.h, ids_ptr, mask_ptr, out_ptr, B, T, C.c_void_p(stream)), "hvla_t5_encode")

    def encode_audit(self, images_ptr, B, stream: int = 0):
        """{site: (largest finite |16-bit operand|, number of inf / NaN)} over all encoder layers (tests)."""
        mx, bad = (C.c_float * 4)(), (C.c_int32 * 4)()
        self._check(self.lib.hvla_encode_audit(self.h, C.c_void_p(images_ptr), B, mx, bad, C.c_void_p(stream)), "hvla_encode_audit")
        return {k: (float(mx[i]), int(bad[i])) for i, k in enumerate(("layernorm_out", "qkv", "attention_out", "gelu_out"))}

    def set_attention_outputs(self, dino_ptr: int = 0, head_ptr: int = 0):
        """Device buffers the following encode / policy / step calls write the two attention maps into (0 = off)."""
        self._check(self.lib.hvla_set_attention_outputs(self.h, C.c_void_p(dino_ptr or None), C.c_void_p(head_ptr or None)),
                    "hvla_set_attention_outputs")

    def train_profile(self, on: bool):
        self._check(self.lib.hvla_train_profile(self.h, int(bool(on))), "hvla_train_profile")

    def train_profile_read(self):
        """(ms summed over the fine-tune step's batched GEMM launches, their f32-equivalent FLOPs, launches) since the last read."""
        ms, fl, n = C.c_float(), C.c_double(), C.c_int32()
        self._check(self.lib.hvla_train_profile_read(self.h, C.byref(ms), C.byref(fl), C.byref(n)), "hvla_train_profile_read")
        return ms.value, fl.value, n.value

    def release_pooled_arenas(self):
        """Give the weight arenas parked by `weights_free` back to the device (up to 4 per context stay resident otherwise)."""
        self._check(self.lib.hvla_release_pooled_arenas(self.h), "hvla_release_pooled_arenas")

    def selftest(self, stream: int = 0):
        self._check(self.lib.hvla_selftest(self.h, C.c_void_p(stream)), "hvla_selftest")

    def profile(self, mode: int):
        self._check(self.lib.hvla_profile(self.h, mode), "hvla_profile")

    def profile_select(self, names):
        """Categories (PROF_NAMES) that mode 1 times."""
        mask = 0
        for n in names:
            mask |= 1 << PROF_NAMES.index(n)
        self._check(self.lib.hvla_profile_select(self.h, mask), "hvla_profile_select")

    def profile_read(self):
        """{category: (total ms, launches)} since the last read."""
        ms = (C.c_float * len(PROF_NAMES))()
        n = (C.c_int32 * len(PROF_NAMES))()
        self._check(self.lib.hvla_profile_read(self.h, ms, n), "hvla_profile_read")
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(PROF_NAMES)}

    def launches(self) -> int:
        """Kernel launches (and memset nodes) enqueued by this ctx since the last call."""
        return int(self.lib.hvla_launches(self.h))

    def box_probe(self, stream=0):
        """(sustained shader clock MHz under a chip-wide MFMA loop, that loop's TFLOP/s, its duration in ms)."""
        out = (C.c_float * 3)()
        self._check(self.lib.hvla_box_probe(self.h, out, C.c_void_p(stream)), "hvla_box_probe")
        return float(out[0]), float(out[1]), float(out[2])

    # raw pointer-level calls (device pointers as ints)
    def generate(self, tok_ptr, mask_ptr, cls_ptr, B, stream=0):
        w = C.c_void_p()
        self._check(self.lib.hvla_generate(self.h, tok_ptr, mask_ptr, cls_ptr, B, C.byref(w), C.c_void_p(stream)),
                    "hvla_generate")
        return w

    def weights_free(self, w):
        self.lib.hvla_weights_free(self.h, w)

    def weights_export(self, w, theta_ptr, ctx_ptr, stream=0):
        self._check(self.lib.hvla_weights_export(self.h, w, theta_ptr, ctx_ptr, C.c_void_p(stream)), "hvla_weights_export")

    def encode(self, img_ptr, tok_ptr, B, stream=0):
        self._check(self.lib.hvla_encode(self.h, img_ptr, tok_ptr, B, C.c_void_p(stream)), "hvla_encode")

    def encode_hidden(self, img_ptr, hidden_ptr, B, stream=0):
        self._check(self.lib.hvla_encode_hidden(self.h, img_ptr, hidden_ptr, B, C.c_void_p(stream)), "hvla_encode_hidden")

    def policy(self, w, tok_ptr, act_ptr, logit_ptr, B, stream=0):
        self._check(self.lib.hvla_policy(self.h, w, tok_ptr, act_ptr, logit_ptr, B, C.c_void_p(stream)), "hvla_policy")

    def step(self, w, img_ptr, act_ptr, logit_ptr, B, stream=0):
        self._check(self.lib.hvla_step(self.h, w, img_ptr, act_ptr, logit_ptr, B, C.c_void_p(stream)), "hvla_step")

    def loss(self, act_ptr, logit_ptr, target_ptr, tmask_ptr, amask_ptr, loss_ptr, B, stream=0):
        self._check(self.lib.hvla_loss(self.h, act_ptr, logit_ptr, target_ptr, tmask_ptr, amask_ptr, loss_ptr, B,
                                       C.c_void_p(stream)), "hvla_loss")

    def train_sizes(self, B, train_encoder=False):
        """(n_params, G, workspace_floats, n_hypernet)"""
        out = (C.c_int64 * 4)()
        self._check(self.lib.hvla_train_sizes(self.h, B, int(train_encoder), out), "hvla_train_sizes")
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def train_step(self, buf, ptrs, B, hyper, stream=0):
        self._check(self.lib.hvla_train_step(self.h, C.byref(buf), *ptrs, B, C.byref(hyper), C.c_void_p(stream)),
                    "hvla_train_step")

    def train_apply(self, buf, hyper, stream=0):
        self._check(self.lib.hvla_train_apply(self.h, C.byref(buf), C.byref(hyper), C.c_void_p(stream)), "hvla_train_apply")

    def train_bucket_ranges(self, train_encoder):
        out = (C.c_int64 * 6)()
        self._check(self.lib.hvla_train_bucket_ranges(self.h, int(train_encoder), out), "hvla_train_bucket_ranges")
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(3)]

    def train_wait_bucket(self, bucket, stream):
        self._check(self.lib.hvla_train_wait_bucket(self.h, int(bucket), C.c_void_p(stream)), "hvla_train_wait_bucket")

    def train_accumulate(self, buf, acc_ptr, inv_k, hyper, stream=0):
        self._check(self.lib.hvla_train_accumulate(self.h, C.byref(buf), C.c_void_p(acc_ptr), C.c_float(inv_k), C.byref(hyper),
                                                   C.c_void_p(stream)), "hvla_train_accumulate")

    def loss_terms(self, act_ptr, logit_ptr, target_ptr, tmask_ptr, amask_ptr, cont_ptr, grip_ptr, sqerr_ptr, B, stream=0):
        """The two halves of hvla_loss per sample and the validation's squared error (device f32 [B] each)."""
        self._check(self.lib.hvla_loss_terms(self.h, *[C.c_void_p(p or None) for p in (act_ptr, logit_ptr, target_ptr, tmask_ptr, amask_ptr,
                                                                                       cont_ptr, grip_ptr, sqerr_ptr)],
                                             B, C.c_void_p(stream)), "hvla_loss_terms")

    def train_metrics(self, buf, select, out_ptr, B, train_encoder, scratch_ptr, prev_params_ptr=0, target_ptr=0, tmask_ptr=0,
                      amask_ptr=0, task_ids_ptr=0, n_tasks=0, entropy_ptr=0, alignment_ptr=0, encoder_sqsum=0.0, stream=0):
        """hvla_train_metrics: the reference's `info` of one step into the device vector at `out_ptr` (f32 [HVLA_METRIC_N + 2 n_tasks])."""
        opts = hvla_train_metrics_in(C.sizeof(hvla_train_metrics_in), int(select), prev_params_ptr or None, target_ptr or None,
                                     tmask_ptr or None, amask_ptr or None, task_ids_ptr or None, int(n_tasks), entropy_ptr or None,
                                     alignment_ptr or None, float(encoder_sqsum), scratch_ptr or None)
        self._check(self.lib.hvla_train_metrics(self.h, C.byref(buf), C.byref(opts), C.c_void_p(out_ptr or None), int(B),
                                                int(bool(train_encoder)), C.c_void_p(stream)), "hvla_train_metrics")

    def train_publish(self, params_ptr, n_params, train_encoder=False, stream=0):
        """Pack the flat training vector at `params_ptr` (device f32 [n_params]) into this context's serving buffers, in place."""
        self._check(self.lib.hvla_train_publish(self.h, C.c_void_p(params_ptr or None), int(n_params), int(bool(train_encoder)),
                                                C.c_void_p(stream)), "hvla_train_publish")

    def position_interp(self, src_ptr, n, w_ptr, dst_ptr, stream=0):
        """dst [1 + P, E] = the resize of the source position table src [1 + n n, E] with the weights w [n, grid] (device pointers)."""
        self._check(self.lib.hvla_position_interp(self.h, C.c_void_p(src_ptr or None), int(n), C.c_void_p(w_ptr or None),
                                                  C.c_void_p(dst_ptr or None), C.c_void_p(stream)), "hvla_position_interp")

    def position_interp_adjoint(self, ddst_ptr, n, w_ptr, dsrc_ptr, stream=0):
        """dsrc [1 + n n, E] = the transpose of `position_interp` applied to ddst [1 + P, E]."""
        self._check(self.lib.hvla_position_interp_adjoint(self.h, C.c_void_p(ddst_ptr or None), int(n), C.c_void_p(w_ptr or None),
                                                          C.c_void_p(dsrc_ptr or None), C.c_void_p(stream)),
                    "hvla_position_interp_adjoint")

    def train_position_source(self, n, w_ptr=0):
        """Train the position table through its interpolation from an n x n source (n = 0: off); `w_ptr` stays the caller's."""
        self._check(self.lib.hvla_train_position_source(self.h, int(n), C.c_void_p(w_ptr or None)), "hvla_train_position_source")

    def train_frozen(self, frozen_ptr=0, n_params=0, frozen_buckets=0):
        """create_optimizer's frozen_keys as a device uint8 mask [n_params] (1 = frozen; 0 / None: off) and the gradient buckets
        that are frozen as a whole (hypervla.train.frozen_plan); the mask stays the caller's."""
        self._check(self.lib.hvla_train_frozen(self.h, C.c_void_p(frozen_ptr or None), int(n_params), int(frozen_buckets)),
                    "hvla_train_frozen")

    def train_attention_losses(self, entropy_weight=0.0, alignment_weight=0.0, reference_ptr=0, entropy_ptr=0, alignment_ptr=0):
        """The reference's attention entropy / alignment terms for the following train_step calls (both weights 0: off, passed as
        NULL); `alignment_weight` is the annealed weight, the device pointers (map [B, P] in, the two [B] metric outputs) stay the caller's."""
        if not (entropy_weight or alignment_weight):
            rc = self.lib.hvla_train_attention_losses(self.h, None)
        else:
            opts = hvla_train_attention(C.sizeof(hvla_train_attention), float(entropy_weight), float(alignment_weight),
                                        reference_ptr or None, entropy_ptr or None, alignment_ptr or None)
            rc = self.lib.hvla_train_attention_losses(self.h, C.byref(opts))
        self._check(rc, "hvla_train_attention_losses")

    def train_noise(self, policy_dropout=0.0, image_embedding_noise=0.0, context_dropout=0.0, image_dropout=0.0, seed=0,
                    sample_offset=0, draw=0, off=False):
        """The reference's train=True noise for the following train_step calls (hvla_train_noise_set; by value).  `off`: NULL, the
        state of a new context.  Make the setting before train_sizes: the noisy copies live in the workspace."""
        if off:
            rc = self.lib.hvla_train_noise_set(self.h, None)
        else:
            opts = hvla_train_noise(C.sizeof(hvla_train_noise), float(policy_dropout), float(image_embedding_noise),
                                    float(context_dropout), float(image_dropout), int(seed) & (2 ** 64 - 1), int(sample_offset),
                                    int(draw) & 0xffffffff)
            rc = self.lib.hvla_train_noise_set(self.h, C.byref(opts))
        self._check(rc, "hvla_train_noise_set")

    def train_noise_probe(self, site, sample_id, n, out_ptr, stream: int = 0):
        """Test instrumentation: the n multipliers (kinds 1-4, 6, 7) or normals (kind 5) of `site` = kind | layer << 8 for the sample
        with global index `sample_id`, under the current setting, into device f32 [n]."""
        self._check(self.lib.hvla_train_noise_probe(self.h, int(site), int(sample_id), int(n), C.c_void_p(out_ptr), C.c_void_p(stream)),
                    "hvla_train_noise_probe")

    def train_language_tokens(self, on=False):
        """Fine-tune a use_language_token context: while on, the hvla_train_* entries serve it (off: they refuse it, the default)."""
        self._check(self.lib.hvla_train_language_tokens(self.h, int(on)), "hvla_train_language_tokens")

    def train_differential(self, on=False):
        """Fine-tune a differential_attention context: while on, the hvla_train_* entries serve it (off: they refuse it, the default)."""
        self._check(self.lib.hvla_train_differential(self.h, int(on)), "hvla_train_differential")

    def train_layer_tokens(self, on=False):
        """Fine-tune a layer_tokens context: while on, the hvla_train_* entries serve it (off: they refuse it, the default)."""
        self._check(self.lib.hvla_train_layer_tokens(self.h, int(on)), "hvla_train_layer_tokens")

    def train_context_rows(self, batch, train_encoder=False):
        """Test instrumentation: (offset of ctx, offset of d ctx, length) in floats of the step's `work` buffer."""
        out = (C.c_int64 * 3)()
        self._check(self.lib.hvla_train_context_rows(self.h, int(batch), int(train_encoder), out), "hvla_train_context_rows")
        return tuple(int(x) for x in out)

    def ensemble_reset(self, w, stream=0):
        self._check(self.lib.hvla_ensemble_reset(self.h, w, C.c_void_p(stream)), "hvla_ensemble_reset")

    def ensemble(self, w, act_ptr, mean_ptr, std_ptr, mask_ptr, out_ptr, stream=0):
        self._check(self.lib.hvla_ensemble(self.h, w, act_ptr, mean_ptr, std_ptr, mask_ptr, out_ptr, C.c_void_p(stream)),
                    "hvla_ensemble")

    # episode pool (include/hvla.h): `slots_ptr` is a device int32 [K] map that hypervla.pool.check_slots has accepted
    def weights_alloc(self, B, stream=0):
        w = C.c_void_p()
        self._check(self.lib.hvla_weights_alloc(self.h, B, C.byref(w), C.c_void_p(stream)), "hvla_weights_alloc")
        return w

    def generate_slots(self, w, slots_ptr, K, tok_ptr, mask_ptr, cls_ptr, stream=0):
        self._check(self.lib.hvla_generate_slots(self.h, w, C.c_void_p(slots_ptr), K, tok_ptr, mask_ptr, cls_ptr,
                                                 C.c_void_p(stream)), "hvla_generate_slots")

    def step_slots(self, w, slots_ptr, K, img_ptr, act_ptr, logit_ptr, stream=0):
        self._check(self.lib.hvla_step_slots(self.h, w, C.c_void_p(slots_ptr), K, img_ptr, act_ptr, logit_ptr, C.c_void_p(stream)),
                    "hvla_step_slots")

    def ensemble_slots(self, w, slots_ptr, K, act_ptr, mean_ptr, std_ptr, mask_ptr, out_ptr, stream=0):
        self._check(self.lib.hvla_ensemble_slots(self.h, w, C.c_void_p(slots_ptr), K, act_ptr, mean_ptr, std_ptr, mask_ptr, out_ptr,
                                                 C.c_void_p(stream)), "hvla_ensemble_slots")

    # weight arenas as values (include/hvla.h): device pointers as ints, 0 / None = NULL
    def weights_import(self, theta_ptr, ctx_ptr, tok_ptr, B, stream=0):
        w = C.c_void_p()
        self._check(self.lib.hvla_weights_import(self.h, C.c_void_p(theta_ptr or None), C.c_void_p(ctx_ptr or None),
                                                 C.c_void_p(tok_ptr or None), B, C.byref(w), C.c_void_p(stream)), "hvla_weights_import")
        return w

    def weights_import_slots(self, w, slots_ptr, K, theta_ptr, ctx_ptr, tok_ptr, stream=0):
        self._check(self.lib.hvla_weights_import_slots(self.h, w, C.c_void_p(slots_ptr or None), K, C.c_void_p(theta_ptr or None),
                                                       C.c_void_p(ctx_ptr or None), C.c_void_p(tok_ptr or None), C.c_void_p(stream)),
                    "hvla_weights_import_slots")

    def weights_copy_slots(self, dst, dst_slots_ptr, src, src_slots_ptr, K, stream=0):
        self._check(self.lib.hvla_weights_copy_slots(self.h, dst, C.c_void_p(dst_slots_ptr or None), src,
                                                     C.c_void_p(src_slots_ptr or None), K, C.c_void_p(stream)), "hvla_weights_copy_slots")

    # post-processing of pool slots (include/hvla.h hvla_post_*; hypervla.postprocess drives these)
    def post_create(self, B, stream=0):
        p = C.c_void_p()
        self._check(self.lib.hvla_post_create(self.h, B, C.byref(p), C.c_void_p(stream)), "hvla_post_create")
        return p

    def post_free(self, p):
        self.lib.hvla_post_free(self.h, p)

    def post_assign(self, p, slots_ptr, K, rows_ptr, ensemble_ptr, stream=0):
        self._check(self.lib.hvla_post_assign(self.h, p, C.c_void_p(slots_ptr), K, C.c_void_p(rows_ptr), C.c_void_p(ensemble_ptr),
                                              C.c_void_p(stream)), "hvla_post_assign")

    def post_step(self, p, slots_ptr, K, act_ptr, table_ptr, n_rows, raw_ptr, env_ptr, stream=0):
        self._check(self.lib.hvla_post_step(self.h, p, C.c_void_p(slots_ptr), K, C.c_void_p(act_ptr), C.c_void_p(table_ptr), n_rows,
                                            C.c_void_p(raw_ptr or None), C.c_void_p(env_ptr), C.c_void_p(stream)), "hvla_post_step")
