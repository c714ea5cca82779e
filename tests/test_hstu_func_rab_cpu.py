"""CPU checks of the four entry points that read mask functions beside a relative bias inside the kernels
(mi355_hstu_attn_fwd_kv_rab_func, mi355_hstu_attn_bwd_rab_func and their _f16 twins), called with null tensors in the manner of
test_hstu_entry_points_cpu.py: a well-formed batch = 0 call returns 0, each check of their own fails with the sibling's message, and
of two wrong arguments the one checked first is reported -- window, causal mask, rab (drab), func, then the shared checks.  No call
here gets as far as a launch."""
import ctypes

import pytest

H, D = 2, 64
_BUF = ctypes.create_string_buffer(64)
_P = ctypes.addressof(_BUF)   # a non-null pointer for arguments that must not be NULL (never read: every call returns first)

_FWD = "q k v out q_row k_row v_row o_row q_head k_head v_head o_head "
_BWD = "dout q k v dq dk dv q_row k_row v_row do_row q_head k_head v_head do_head "
_MASK = "num_contexts num_targets group wl wr alpha scaling "
_RAB = "rab rab_b rab_h rab_r "
_DRAB = "drab drab_b drab_h drab_r "
_FUNC = "func func_h func_p n_func func_neg "
_PAGED = "kv_cache page_offsets page_ids last_page_lens page_size "
SIGNATURES = {
    "fwd_kv_rab_func": (_FWD + "cu cu_k batch heads head_dim max_q max_k " + _MASK + _RAB + _FUNC + _PAGED + "stream").split(),
    "bwd_rab_func": (_BWD + "cu batch heads head_dim max_q " + _MASK + _RAB + _DRAB + _FUNC + "func_ws func_ws_bytes stream").split(),
}
DEFAULTS = {"heads": H, "head_dim": D, "group": 1, "wl": -1, "wr": 0, "alpha": 0.25, "scaling": 1.0, "rab": _P, "func": _P,
            "func_p": 1, "n_func": 1, "func_neg": -1e9}
_POINTERS = {"q", "k", "v", "out", "dout", "dq", "dk", "dv", "cu", "cu_k", "num_contexts", "num_targets", "kv_cache", "page_offsets",
             "page_ids", "last_page_lens", "rab", "drab", "func", "func_ws", "stream"}
ENTRIES = list(SIGNATURES)
SUFFIXES = ["", "_f16"]

WINDOW = ({"wl": -5}, b"bad window")
NOT_CAUSAL_MASK = ({"wr": -1, "num_contexts": _P}, b"contextual / target masks require the causal mask (-1, 0)")
NO_RAB = ({"rab": None}, b"rab must be [batch][heads or 1][max_seqlen")
DRAB = ({"drab": _P}, b"drab must hold one [max_seqlen][max_seqlen] matrix per head")
FUNC = ({"n_func": 2}, b"func must be int32 [heads or 1][n_func odd][tokens], func_neg negative")
NO_FUNC = ({"func": None}, b"func must be int32 [heads or 1][n_func odd][tokens], func_neg negative")
HEAD_DIM = ({"head_dim": 48}, b"head_dim must be one of 32, 64, 128, 256")
GROUP = ({"group": 0}, b"target_group_size must be >= 1")
SCALING = ({"scaling": 0.0}, b"scaling_seqlen must be positive")
STRIDES = ({"k_row": 4}, b"strides must be multiples of 8 elements (16-byte rows)")
PAGED = ({"kv_cache": _P}, b"a paged cache needs cu_seqlens_k, page_offsets, page_ids, last_page_lens and page_size")
GRAD_STRIDES = ({}, b"bound dq/dk/dv strides must be multiples of 8 elements")   # (by a binding, see _call)

EACH = ([(e, w) for e in ENTRIES for w in (WINDOW, NOT_CAUSAL_MASK, NO_RAB, FUNC, NO_FUNC, HEAD_DIM, GROUP, SCALING, STRIDES)] +
        [("bwd_rab_func", DRAB), ("bwd_rab_func", GRAD_STRIDES), ("fwd_kv_rab_func", PAGED)])
# (first, second): both wrong in one call, `first` is what the call reports
ORDER = ([(e, WINDOW, NOT_CAUSAL_MASK) for e in ENTRIES] + [(e, NOT_CAUSAL_MASK, NO_RAB) for e in ENTRIES] +
         [(e, WINDOW, NO_RAB) for e in ENTRIES] + [(e, NO_RAB, FUNC) for e in ENTRIES] + [(e, WINDOW, FUNC) for e in ENTRIES] +
         [(e, FUNC, HEAD_DIM) for e in ENTRIES] + [(e, NO_RAB, HEAD_DIM) for e in ENTRIES] + [(e, WINDOW, HEAD_DIM) for e in ENTRIES] +
         [(e, NOT_CAUSAL_MASK, HEAD_DIM) for e in ENTRIES] + [(e, HEAD_DIM, GROUP) for e in ENTRIES] +
         [(e, GROUP, SCALING) for e in ENTRIES] + [(e, SCALING, STRIDES) for e in ENTRIES] +
         [("bwd_rab_func", NO_RAB, DRAB), ("bwd_rab_func", DRAB, FUNC), ("bwd_rab_func", FUNC, GRAD_STRIDES),
          ("bwd_rab_func", HEAD_DIM, GRAD_STRIDES), ("bwd_rab_func", GRAD_STRIDES, GROUP), ("fwd_kv_rab_func", STRIDES, PAGED),
          ("fwd_kv_rab_func", FUNC, PAGED)])


def _lib():
    import hstu  # noqa: F401  (registers the attention entry points in the binding table)
    import mi355_native as N

    return N.lib()


def _call(lib, entry, suffix, *wrong):
    """the well-formed batch = 0 call of `entry` with the arguments of `wrong` replaced"""
    values = dict(DEFAULTS)
    for changes, _ in wrong:
        values.update(changes)
    if GRAD_STRIDES in wrong:   # dq row stride: no multiple of 8
        lib.mi355_hstu_attn_bwd_bind_grad_strides(H * D + 4, D, H * D, D, H * D, D)
    args = [values.get(n, None if n in _POINTERS else 0) for n in SIGNATURES[entry]]
    return getattr(lib, "mi355_hstu_attn_" + entry + suffix)(*args)


def _message(entry, wrong):
    if wrong is STRIDES:
        return (b"q/k/v/dout " if entry.startswith("bwd") else b"q/k/v ") + STRIDES[1]
    return wrong[1]


def _id(case):
    return "-".join(c if isinstance(c, str) else (str(sorted(c[0])) + c[1].decode()[:20]).strip().replace(" ", "_") for c in case)


def test_the_header_declares_the_four_symbols_and_the_library_exports_them():
    import os
    import re

    lib = _lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "recsys_amd.h")).read()
    for entry in ENTRIES:
        for suffix in SUFFIXES:
            name = "mi355_hstu_attn_" + entry + suffix
            assert re.search(r"\bint " + name + r"\(", header), name + " is not declared in include/recsys_amd.h"
            assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(SIGNATURES[entry])


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_well_formed_empty_batch_returns_ok(entry, suffix):
    lib = _lib()
    assert _call(lib, entry, suffix) == 0, lib.mi355_last_error()


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("case", EACH, ids=_id)
def test_each_check_fails_with_the_siblings_message(case, suffix):
    entry, wrong = case
    lib = _lib()
    assert _call(lib, entry, suffix, wrong) == -1
    assert _message(entry, wrong) in lib.mi355_last_error()
    assert _call(lib, entry, suffix) == 0, "the failed call left something to the next one: %r" % lib.mi355_last_error()


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("case", ORDER, ids=_id)
def test_of_two_wrong_arguments_the_first_checked_is_reported(case, suffix):
    entry, first, second = case
    lib = _lib()
    assert _call(lib, entry, suffix, first, second) == -1
    assert _message(entry, first) in lib.mi355_last_error()
    assert _call(lib, entry, suffix, second) == -1        # (the second one alone is refused as well)
    assert _message(entry, second) in lib.mi355_last_error()
    assert _call(lib, entry, suffix) == 0, lib.mi355_last_error()


def test_the_dispatch_no_longer_refuses_func_beside_rab_with_contexts():
    """the refusal text is gone from both host files (the kernels read both operands now); the dense A/B switch alone still
    refuses contexts, which a dense bias cannot express"""
    import inspect

    import hstu.hstu_attn_interface as hi
    import hstu.hstu_ops_gpu as ops

    for mod in (hi, ops):
        assert "needs the in-kernel mask functions (no rab)" not in inspect.getsource(mod)
    for name in ("hstu_varlen_fwd_rab_func", "hstu_varlen_bwd_rab_func", "HstuAttnRabFuncFunc"):
        assert hasattr(hi, name)
    assert list(inspect.signature(hi.hstu_varlen_bwd_rab_func).parameters)[-3:] == ["dq", "dk", "dv"]
    assert all(p.kind is p.KEYWORD_ONLY for p in list(inspect.signature(hi.hstu_varlen_bwd_rab_func).parameters.values())[-3:])
