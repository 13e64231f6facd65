"""What the serving entries of include/hvla.h answer to arguments they refuse: one table, return codes only.  Nothing is launched:
every row is refused before its entry enqueues anything, and the one device buffer that stands in for every non-null pointer is
larger than anything an entry could touch if a row were let through.  The smallest geometry hvla_create accepts is MID (TINY is
outside the kernels' specialisation and refused at create), so the contexts are MID ones.  The rows that carry two faults pin the
ORDER of an entry's checks where the codes differ (an unloaded context wins over a bad count; hvla_ensemble* do not ask whether the
context is loaded)."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPE, STATE = -1, -7                       # HVLA_E_SHAPE, HVLA_E_STATE
MAX_BATCH, POOL = 4, 2


def _table(big, small, raw, w, d):
    """(entry, case, call, expected code).  big / small: loaded contexts of max_batch 4 / 1, raw: a context without weights,
    w: a pool of POOL slots of `big`, d: a device pointer that is valid for everything."""
    lib, n, st = big.lib, C.c_void_p(None), C.c_void_p(None)
    out = C.c_void_p()
    mx, bad = (C.c_float * 4)(), (C.c_int32 * 4)()
    rows = []

    def add(entry, case, code, *args):
        rows.append((entry, case, lambda: getattr(lib, entry)(*args), code))

    # ---- batch entries without an arena: (ctx, required pointers ..., B)
    for entry, ptrs in (("hvla_encode", 2), ("hvla_encode_hidden", 2)):
        call = lambda ctx, B, p: (ctx, *p, B, st)
        add(entry, "null ctx", STATE, *call(n, 1, [d] * ptrs))
        add(entry, "not loaded", STATE, *call(raw.h, 1, [d] * ptrs))
        add(entry, "batch 0", SHAPE, *call(big.h, 0, [d] * ptrs))
        add(entry, "batch max_batch + 1", SHAPE, *call(big.h, MAX_BATCH + 1, [d] * ptrs))
        for i in range(ptrs):
            add(entry, f"null pointer {i}", SHAPE, *call(big.h, 1, [n if j == i else d for j in range(ptrs)]))
        add(entry, "not loaded and batch 0", STATE, *call(raw.h, 0, [d] * ptrs))
    audit = lambda ctx, B, im=d, a=mx, b=bad: (ctx, im, B, a, b, st)
    add("hvla_encode_audit", "null ctx", STATE, *audit(n, 1))
    add("hvla_encode_audit", "not loaded", STATE, *audit(raw.h, 1))
    add("hvla_encode_audit", "batch 0", SHAPE, *audit(big.h, 0))
    add("hvla_encode_audit", "batch max_batch + 1", SHAPE, *audit(big.h, MAX_BATCH + 1))
    add("hvla_encode_audit", "null images", SHAPE, *audit(big.h, 1, im=n))
    add("hvla_encode_audit", "null maxabs", SHAPE, *audit(big.h, 1, a=None))
    add("hvla_encode_audit", "null nonfinite", SHAPE, *audit(big.h, 1, b=None))
    add("hvla_encode_audit", "not loaded and batch 0", STATE, *audit(raw.h, 0))
    # ---- batch entries on an arena: (ctx, w, in, actions, logits, B); logits may be null
    for entry in ("hvla_policy", "hvla_step"):
        call = lambda ctx, B, arena=w, a=d, b=d: (ctx, arena, a, b, d, B, st)
        add(entry, "null ctx", STATE, *call(n, POOL))
        add(entry, "null arena", STATE, *call(big.h, POOL, arena=n))
        add(entry, "not loaded", STATE, *call(raw.h, POOL))
        add(entry, "batch 0", SHAPE, *call(big.h, 0))
        add(entry, "batch max_batch + 1", SHAPE, *call(big.h, MAX_BATCH + 1))
        add(entry, "batch != arena batch", SHAPE, *call(big.h, POOL - 1))
        add(entry, "null input", SHAPE, *call(big.h, POOL, a=n))
        add(entry, "null actions", SHAPE, *call(big.h, POOL, b=n))
        add(entry, "not loaded and batch 0", STATE, *call(raw.h, 0))
    gen = lambda ctx, B, t=d, m=d, c=d, o=C.byref(out): (ctx, t, m, c, B, o, st)
    add("hvla_generate", "null ctx", STATE, *gen(n, 1))
    add("hvla_generate", "null out", STATE, *gen(big.h, 1, o=None))
    add("hvla_generate", "not loaded", STATE, *gen(raw.h, 1))
    add("hvla_generate", "batch 0", SHAPE, *gen(big.h, 0))
    add("hvla_generate", "batch max_batch + 1", SHAPE, *gen(big.h, MAX_BATCH + 1))
    add("hvla_generate", "null tokens", SHAPE, *gen(big.h, 1, t=n))
    add("hvla_generate", "null mask", SHAPE, *gen(big.h, 1, m=n))
    add("hvla_generate", "null cls", SHAPE, *gen(big.h, 1, c=n))
    add("hvla_generate", "not loaded and batch 0", STATE, *gen(raw.h, 0))
    alloc = lambda ctx, B, o=C.byref(out): (ctx, B, o, st)
    add("hvla_weights_alloc", "null ctx", STATE, *alloc(n, 1))
    add("hvla_weights_alloc", "null out", STATE, *alloc(big.h, 1, o=None))
    add("hvla_weights_alloc", "not loaded", STATE, *alloc(raw.h, 1))
    add("hvla_weights_alloc", "batch 0", SHAPE, *alloc(big.h, 0))
    add("hvla_weights_alloc", "batch max_batch + 1", SHAPE, *alloc(big.h, MAX_BATCH + 1))
    add("hvla_weights_alloc", "not loaded and batch 0", STATE, *alloc(raw.h, 0))
    # ---- pooled entries: (ctx, w, slots, K, required pointers ...)
    for entry, ptrs, tail in (("hvla_generate_slots", 3, ()), ("hvla_step_slots", 2, (d,))):
        call = lambda ctx, K, arena=w, s=d, p=None: (ctx, arena, s, K, *(p or [d] * ptrs), *tail, st)
        add(entry, "null ctx", STATE, *call(n, 1))
        add(entry, "null arena", STATE, *call(big.h, 1, arena=n))
        add(entry, "not loaded", STATE, *call(raw.h, 1))
        add(entry, "null slot map", SHAPE, *call(big.h, 1, s=n))
        add(entry, "K = 0", SHAPE, *call(big.h, 0))
        add(entry, "K > pool size", SHAPE, *call(big.h, POOL + 1))
        add(entry, "K > max_batch", SHAPE, *call(small.h, POOL))
        for i in range(ptrs):
            add(entry, f"null pointer {i}", SHAPE, *call(big.h, 1, p=[n if j == i else d for j in range(ptrs)]))
        add(entry, "null slot map and K = 0", SHAPE, *call(big.h, 0, s=n))
        add(entry, "not loaded and K = 0", STATE, *call(raw.h, 0))
    # ---- the ensemble entries do not ask for a loaded context, and hvla_ensemble_slots not for max_batch
    ens = lambda ctx, arena=w, p=None: (ctx, arena, *(p or [d] * 5), st)
    add("hvla_ensemble", "null ctx", STATE, *ens(n))
    add("hvla_ensemble", "null arena", STATE, *ens(big.h, arena=n))
    for i in range(5):
        add("hvla_ensemble", f"null pointer {i}", SHAPE, *ens(big.h, p=[n if j == i else d for j in range(5)]))
    add("hvla_ensemble", "not loaded and null pointer 0", SHAPE, *ens(raw.h, p=[n, d, d, d, d]))
    enss = lambda ctx, K, arena=w, s=d, p=None: (ctx, arena, s, K, *(p or [d] * 5), st)
    add("hvla_ensemble_slots", "null ctx", STATE, *enss(n, 1))
    add("hvla_ensemble_slots", "null arena", STATE, *enss(big.h, 1, arena=n))
    add("hvla_ensemble_slots", "null slot map", SHAPE, *enss(big.h, 1, s=n))
    add("hvla_ensemble_slots", "K = 0", SHAPE, *enss(big.h, 0))
    add("hvla_ensemble_slots", "K > pool size", SHAPE, *enss(big.h, POOL + 1))
    for i in range(5):
        add("hvla_ensemble_slots", f"null pointer {i}", SHAPE, *enss(big.h, 1, p=[n if j == i else d for j in range(5)]))
    add("hvla_ensemble_slots", "null slot map and K = 0", SHAPE, *enss(big.h, 0, s=n))
    add("hvla_ensemble_slots", "not loaded and null slot map", SHAPE, *enss(raw.h, 1, s=n))
    add("hvla_ensemble_reset", "null ctx", STATE, n, w, st)
    add("hvla_ensemble_reset", "null arena", STATE, big.h, n, st)
    return rows


def test_every_serving_entry_refuses_with_the_code_of_its_first_failed_check():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    from hypervla import _native
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    big, small = HyperVLA.from_synthetic(MID, device=0, max_batch=MAX_BATCH), HyperVLA.from_synthetic(MID, device=0, max_batch=1)
    raw = _native.Context(MID, 0, MAX_BATCH)                   # no weights loaded
    buf = torch.zeros(8 << 20, dtype=torch.uint8, device="cuda")   # (zeros: as a slot map it names slot 0)
    w = big._ctx.weights_alloc(POOL)
    try:
        for c in (big._ctx, small._ctx, raw):
            c.launches()                                       # (reads and clears the count)
        rows = _table(big._ctx, small._ctx, raw, w, C.c_void_p(buf.data_ptr()))
        got = [(entry, case, call(), want) for entry, case, call, want in rows]
        wrong = [r for r in got if r[2] != r[3]]
        assert not wrong, wrong
        assert len({e for e, _, _, _ in got}) == 12 and len(got) == 100
        assert sum(c.launches() for c in (big._ctx, small._ctx, raw)) == 0      # nothing was enqueued
    finally:
        big._ctx.weights_free(w)
        raw.close()
