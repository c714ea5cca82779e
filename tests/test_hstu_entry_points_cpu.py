"""CPU checks of the HSTU attention entry points of the C ABI (the thirteen typed names and their _f16 twins), called with null
tensors as test_hstu_qkvpacked_cpu.py does: a well-formed batch = 0 call returns 0, every check an entry point makes of its own
and every check all of them share fails with its own message, and of two wrong arguments the one checked first is reported --
which pins the order of the checks.  No call here gets as far as a launch."""
import ctypes

import pytest

H, D = 2, 64
_BUF = ctypes.create_string_buffer(64)
_P = ctypes.addressof(_BUF)   # a non-null pointer for arguments that must not be NULL (never read: every call returns first)

_FWD = "q k v out q_row k_row v_row o_row q_head k_head v_head o_head "
_BWD = "dout q k v dq dk dv q_row k_row v_row do_row q_head k_head v_head do_head "
_PAGED = "kv_cache page_offsets page_ids last_page_lens page_size "
_RAB = "rab rab_b rab_h rab_r "
_DRAB = "drab drab_b drab_h drab_r "
_FUNC = "func func_h func_p n_func func_neg "
_MASK = "num_contexts num_targets group wl wr alpha scaling "
# the argument lists of include/recsys_amd.h, by name
SIGNATURES = {k: v.split() for k, v in {
    "fwd": _FWD + "cu batch heads head_dim max_q num_contexts num_targets group causal alpha scaling stream",
    "fwd_kv": _FWD + "cu cu_k batch heads head_dim max_q num_contexts num_targets group causal alpha scaling " + _PAGED + "stream",
    "fwd_window": _FWD + "cu batch heads head_dim max_q wl wr alpha scaling stream",
    "fwd_kv_window": _FWD + "cu cu_k batch heads head_dim max_q wl wr alpha scaling " + _PAGED + "stream",
    "fwd_rab": _FWD + "cu batch heads head_dim max_q " + _MASK + _RAB + "stream",
    "fwd_kv_rab": _FWD + "cu cu_k batch heads head_dim max_q max_k " + _MASK + _RAB + _PAGED + "stream",
    "fwd_kv_func": _FWD + "cu cu_k batch heads head_dim max_q max_k " + _MASK + _FUNC + _PAGED + "stream",
    "bwd": _BWD + "cu batch heads head_dim max_q num_contexts num_targets group causal alpha scaling ws ws_bytes stream",
    "bwd_window": _BWD + "cu batch heads head_dim max_q wl wr alpha scaling ws ws_bytes stream",
    "bwd_rab": _BWD + "cu batch heads head_dim max_q " + _MASK + _RAB + _DRAB + "stream",
    "bwd_kv": _BWD + "cu cu_k batch heads head_dim max_q max_k " + _MASK + _RAB + _DRAB + "stream",
    "bwd_func": _BWD + "cu batch heads head_dim max_q " + _MASK + _FUNC + "func_ws func_ws_bytes ws ws_bytes stream",
}.items()}
# a well-formed batch = 0 call: every pointer NULL and every integer 0 but these
DEFAULTS = {"heads": H, "head_dim": D, "group": 1, "causal": 1, "wl": -1, "wr": 0, "alpha": 0.25, "scaling": 1.0,
            "func_p": 1, "n_func": 1, "func_neg": -1e9}
_POINTERS = {"q", "k", "v", "out", "dout", "dq", "dk", "dv", "cu", "cu_k", "num_contexts", "num_targets", "kv_cache", "page_offsets",
             "page_ids", "last_page_lens", "rab", "drab", "func", "func_ws", "ws", "stream"}
_NEEDS = {"fwd_rab": {"rab": _P}, "fwd_kv_rab": {"rab": _P}, "bwd_rab": {"rab": _P}, "fwd_kv_func": {"func": _P},
          "bwd_func": {"func": _P}, "fwd_window": {"wl": 8, "wr": 3}, "fwd_kv_window": {"wl": 8, "wr": 3},
          "bwd_window": {"wl": 8, "wr": 3}}
ENTRIES = list(SIGNATURES)
SUFFIXES = ["", "_f16"]

# the wrong arguments, by the message of the check that refuses them
HEAD_DIM = ({"head_dim": 48}, b"head_dim must be one of 32, 64, 128, 256")
GROUP = ({"group": 0}, b"target_group_size must be >= 1")
SCALING = ({"scaling": 0.0}, b"scaling_seqlen must be positive")
STRIDES = ({"k_row": 4}, b"strides must be multiples of 8 elements (16-byte rows)")   # (see _message: q/k/v or q/k/v/dout)
NOT_CAUSAL = ({"causal": 0, "num_contexts": _P}, b"contextual / target masks require causal attention")
NOT_CAUSAL_MASK = ({"wr": -1, "num_targets": _P}, b"contextual / target masks require the causal mask (-1, 0)")
WINDOW = ({"wl": -5}, b"bad window")
NO_RAB = ({"rab": None}, b"rab must be [batch][heads or 1][max_seqlen")
SHORT_RAB = ({"rab": _P, "rab_r": -8}, b"rab must be [batch][heads or 1][max_seqlen_k][max_seqlen_k]")
DRAB = ({"drab": _P}, b"drab must hold one [max_seqlen][max_seqlen] matrix per head")
DRAB_NO_RAB = ({"drab": _P, "drab_h": 64}, b"drab needs rab and must hold")
FUNC = ({"n_func": 2}, b"func must be int32 [heads or 1][n_func odd][tokens], func_neg negative")
PAGED = ({"kv_cache": _P}, b"a paged cache needs cu_seqlens_k, page_offsets, page_ids, last_page_lens and page_size")
DELTA_Q = ({"max_q": 5, "max_k": 3}, b"max_seqlen_q <= max_seqlen_k")
NO_CU = ({"batch": 1}, b"cu_seqlens_q and cu_seqlens_k are required")
GRAD_STRIDES = ({}, b"bound dq/dk/dv strides must be multiples of 8 elements")   # (by a binding, see _call)

_WINDOWED = ("fwd_window", "fwd_kv_window", "bwd_window")
_MASKED = ("fwd_rab", "fwd_kv_rab", "fwd_kv_func", "bwd_rab", "bwd_func", "bwd_kv")
_PLAIN = ("fwd", "fwd_kv", "bwd")
_PAGED_ENTRIES = ("fwd_kv", "fwd_kv_window", "fwd_kv_rab", "fwd_kv_func")
_BACKWARDS = ("bwd", "bwd_window", "bwd_rab", "bwd_func", "bwd_kv")

OWN = ([(e, WINDOW) for e in _WINDOWED + _MASKED] + [(e, NOT_CAUSAL_MASK) for e in _MASKED] +
       [(e, NO_RAB) for e in ("fwd_rab", "fwd_kv_rab", "bwd_rab")] + [("bwd_kv", SHORT_RAB), ("bwd_rab", DRAB), ("bwd_kv", DRAB_NO_RAB)] +
       [(e, FUNC) for e in ("fwd_kv_func", "bwd_func")] + [(e, PAGED) for e in _PAGED_ENTRIES] + [("bwd_kv", DELTA_Q), ("bwd_kv", NO_CU)])
SHARED = ([(e, w) for e in ENTRIES for w in (HEAD_DIM, SCALING, STRIDES)] + [(e, GROUP) for e in _PLAIN + _MASKED] +
          [(e, NOT_CAUSAL) for e in _PLAIN] + [(e, GRAD_STRIDES) for e in _BACKWARDS])
# (first, second): both wrong in one call, `first` is what the call reports
ORDER = ([(e, HEAD_DIM, SCALING) for e in ENTRIES] + [(e, SCALING, STRIDES) for e in ENTRIES] +
         [(e, HEAD_DIM, GROUP) for e in _PLAIN + _MASKED] + [(e, GROUP, SCALING) for e in _PLAIN + _MASKED] +
         [(e, GROUP, NOT_CAUSAL) for e in _PLAIN] + [(e, NOT_CAUSAL, SCALING) for e in _PLAIN] +
         [(e, STRIDES, PAGED) for e in _PAGED_ENTRIES] +
         [(e, HEAD_DIM, GRAD_STRIDES) for e in _BACKWARDS] + [(e, GRAD_STRIDES, SCALING) for e in _BACKWARDS] +
         [(e, GRAD_STRIDES, GROUP) for e in ("bwd", "bwd_rab", "bwd_func", "bwd_kv")] +
         # the entry points with checks of their own make them in front of the shared ones ...
         [(e, WINDOW, HEAD_DIM) for e in _WINDOWED + _MASKED if e != "bwd_kv"] +
         [(e, NOT_CAUSAL_MASK, HEAD_DIM) for e in _MASKED if e != "bwd_kv"] +
         [(e, WINDOW, NOT_CAUSAL_MASK) for e in _MASKED] +
         [(e, NO_RAB, WINDOW) for e in ("fwd_rab", "fwd_kv_rab", "bwd_rab")] + [(e, FUNC, WINDOW) for e in ("fwd_kv_func", "bwd_func")] +
         [("bwd_rab", NO_RAB, DRAB), ("bwd_rab", DRAB, WINDOW), ("bwd_rab", DRAB, GRAD_STRIDES), ("bwd_window", WINDOW, GRAD_STRIDES),
          ("bwd_func", FUNC, GRAD_STRIDES),
          # ... but the delta-q backward, which makes them behind
          ("bwd_kv", HEAD_DIM, WINDOW), ("bwd_kv", STRIDES, NO_CU), ("bwd_kv", NO_CU, DELTA_Q), ("bwd_kv", DELTA_Q, SHORT_RAB),
          ("bwd_kv", SHORT_RAB, DRAB_NO_RAB), ("bwd_kv", DRAB_NO_RAB, WINDOW)])


def _lib():
    import hstu  # noqa: F401  (registers the attention entry points in the binding table)
    import mi355_native as N

    return N.lib()


def _call(lib, entry, suffix, *wrong):
    """the well-formed batch = 0 call of `entry` with the arguments of `wrong` replaced"""
    values = {**DEFAULTS, **_NEEDS.get(entry, {})}
    for changes, _ in wrong:
        values.update(changes)
    if GRAD_STRIDES in wrong:   # dq row stride: no multiple of 8
        lib.mi355_hstu_attn_bwd_bind_grad_strides(H * D + 4, D, H * D, D, H * D, D)
    args = [values.get(n, None if n in _POINTERS else 0) for n in SIGNATURES[entry]]
    return getattr(lib, "mi355_hstu_attn_" + entry + suffix)(*args)


def _message(entry, wrong):
    if wrong is STRIDES:
        return (b"q/k/v/dout " if entry in _BACKWARDS else b"q/k/v ") + STRIDES[1]
    return wrong[1]


def _id(case):
    return "-".join(c if isinstance(c, str) else c[1].decode()[:24].strip().replace(" ", "_") for c in case)


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_well_formed_empty_batch_returns_ok(entry, suffix):
    lib = _lib()
    assert _call(lib, entry, suffix) == 0, lib.mi355_last_error()


@pytest.mark.parametrize("suffix", SUFFIXES)
def test_the_forward_hint_is_typed_and_an_empty_forward_after_it_returns_ok(suffix):
    lib = _lib()
    assert getattr(lib, "mi355_hstu_attn_fwd_hint_tokens" + suffix)(4096) is None
    assert _call(lib, "fwd", suffix) == 0, lib.mi355_last_error()


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("case", OWN + SHARED, ids=_id)
def test_each_check_fails_with_its_own_message(case, suffix):
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
