"""The layer limits of the training path (csrc/train_layout.h: train_refusal) at every hvla_train_* entry.  hvla_create serves a
17-layer policy at the MID widths; the tables of the fine-tune step hold 16.  Nothing is launched: every argument but the context
is null or a placeholder, and an entry that got past the refusal would answer "null pointer" or a size mismatch instead."""
import ctypes as C
import dataclasses

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def test_every_training_entry_refuses_a_policy_beyond_the_layer_limit():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    from hypervla import _native
    from hypervla.config import MID, generated_leaves
    from hypervla.train import train_param_layout
    ctx = _native.Context(dataclasses.replace(MID, layers=17), 0, 1)          # no weights loaded
    try:
        lib, h = ctx.lib, ctx.h
        out = (C.c_int64 * 6)()
        buf, hy = _native.hvla_train_buffers(), _native.hvla_train_hyper()
        mask = torch.zeros(8, dtype=torch.uint8, device="cuda")
        att = _native.hvla_train_attention(C.sizeof(_native.hvla_train_attention), 1.0, 0.0, None, None, None)
        null = C.c_void_p(None)
        calls = {
            "sizes": lambda: lib.hvla_train_sizes(h, 1, 0, C.cast(out, C.POINTER(C.c_int64))),
            "bucket_ranges": lambda: lib.hvla_train_bucket_ranges(h, 0, C.cast(out, C.POINTER(C.c_int64))),
            "position_source": lambda: lib.hvla_train_position_source(h, 2, null),
            "frozen": lambda: lib.hvla_train_frozen(h, C.c_void_p(mask.data_ptr()), 8, 0),
            "attention_losses": lambda: lib.hvla_train_attention_losses(h, C.byref(att)),
            "step": lambda: lib.hvla_train_step(h, C.byref(buf), *([null] * 8), 1, C.byref(hy), null),
            "apply": lambda: lib.hvla_train_apply(h, C.byref(buf), C.byref(hy), null),
            "accumulate": lambda: lib.hvla_train_accumulate(h, C.byref(buf), null, C.c_float(1.0), C.byref(hy), null),
            "publish": lambda: lib.hvla_train_publish(h, null, 0, 0, null),
        }
        for name, call in calls.items():
            rc = call()
            msg = lib.hvla_last_error(h).decode()
            assert rc == -1 and "too many layers" in msg, (name, rc, msg)         # HVLA_E_SHAPE
    finally:
        ctx.close()
    g = dataclasses.replace(MID, layers=16)
    ctx = _native.Context(g, 0, 1)
    try:
        layout, total = train_param_layout(g, False)
        leaves = generated_leaves(g)
        n, G, work, n_hyper = ctx.train_sizes(1, False)
        assert (n, n_hyper) == (total, total) and G == leaves[-1].offset + leaves[-1].size and work > 0
        layout_enc, total_enc = train_param_layout(g, True)
        assert ctx.train_sizes(1, True)[0] == total_enc and ctx.train_sizes(1, True)[3] == total
    finally:
        ctx.close()
