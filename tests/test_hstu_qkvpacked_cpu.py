"""CPU checks of the strided in-place backward and of the packed entry point: the stride binding of the C ABI
(mi355_hstu_attn_bwd_bind_grad_strides: declared, exported, checked and consumed by the next backward of any of the five
variants and both operand types, never left behind), and the Python surface the reference's kernel package has
(`hstu.hstu_attn_qkvpacked_func`, the package `hstu_attn` with the legacy `hstu_attn_varlen_func`): names, order, defaults and
the ValueErrors raised in front of any device work."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, D = 2, 64
BIND = "mi355_hstu_attn_bwd_bind_grad_strides"
_BUF = ctypes.create_string_buffer(64)
_P = ctypes.addressof(_BUF)   # a non-null pointer for the arguments that must not be NULL (batch = 0: never read)

# batch = 0 calls with null tensors, well formed otherwise: [7 tensors] [8 strides] then what each variant takes
_HEAD = [None] * 7 + [0] * 8
BACKWARDS = {
    "mi355_hstu_attn_bwd": _HEAD + [None, 0, H, D, 0, None, None, 1, 1, 0.25, 1.0, None, 0, None],
    "mi355_hstu_attn_bwd_window": _HEAD + [None, 0, H, D, 0, 8, 3, 0.25, 1.0, None, 0, None],
    "mi355_hstu_attn_bwd_rab": _HEAD + [None, 0, H, D, 0, None, None, 1, -1, 0, 0.25, 1.0, _P, 0, 0, 0, None, 0, 0, 0, None],
    "mi355_hstu_attn_bwd_func": _HEAD + [None, 0, H, D, 0, None, None, 1, -1, 0, 0.25, 1.0, _P, 0, 1, 1, -1e9, None, 0, None, 0, None],
    "mi355_hstu_attn_bwd_kv": _HEAD + [None, None, 0, H, D, 0, 0, None, None, 1, -1, 0, 0.25, 1.0, None, 0, 0, 0, None, 0, 0, 0, None],
}
VARIANTS = [n + s for n in BACKWARDS for s in ("", "_f16")]


def _lib():
    import hstu  # noqa: F401  (registers the attention entry points in the binding table)
    import mi355_native as N

    return N.lib()


def _call(lib, name):
    return getattr(lib, name)(*BACKWARDS[name.replace("_f16", "")])


def test_the_bind_call_is_declared_and_exported():
    import mi355_native as N

    lib = _lib()
    header = open(os.path.join(ROOT, "include", "recsys_amd.h")).read()
    m = re.search(r"\bvoid\s+" + BIND + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{BIND} is not declared in include/recsys_amd.h"
    assert [a.split()[-1] for a in m.group(1).split(",")] == ["dq_row_stride", "dq_head_stride", "dk_row_stride", "dk_head_stride",
                                                              "dv_row_stride", "dv_head_stride"]
    assert hasattr(lib, BIND) and BIND in N.exported_symbols()
    # one binding serves both operand types (as mi355_hstu_attn_bwd_hint_tokens): no _f16 twin to forget
    assert not re.search(BIND + r"_f16\b", header)


@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("strides", [(H * D + 4, D, H * D, D, H * D, D),      # dq row stride: no multiple of 8
                                     (4 * H * D, D, 4 * H * D, D + 4, 4 * H * D, D),   # dk head stride: no multiple of 8
                                     (4 * H * D, D, 4 * H * D, D, 4 * H * D, D - 8)],  # dv head stride < head_dim
                         ids=["row_not_8", "head_not_8", "head_below_head_dim"])
def test_bad_strides_fail_the_next_backward_and_are_gone_after_it(name, strides):
    lib = _lib()
    assert _call(lib, name) == 0, lib.mi355_last_error()       # (the call itself is well formed)
    lib.mi355_hstu_attn_bwd_bind_grad_strides(*strides)
    assert _call(lib, name) == -1
    assert b"dq/dk/dv strides" in lib.mi355_last_error()
    assert _call(lib, name) == 0, "the binding outlived the call that consumed it"


@pytest.mark.parametrize("name", VARIANTS)
def test_good_strides_are_accepted_and_consumed_by_an_early_return(name):
    lib = _lib()
    lib.mi355_hstu_attn_bwd_bind_grad_strides(4 * H * D, D, 4 * H * D, D, 4 * H * D, D)
    assert _call(lib, name) == 0, lib.mi355_last_error()       # batch == 0: returns in front of any launch
    # the strides fit head_dim 64 only: had they stayed bound, this head_dim 256 call would refuse them
    args = list(BACKWARDS[name.replace("_f16", "")])
    args[args.index(D)] = 256
    assert getattr(lib, name)(*args) == 0, lib.mi355_last_error()


@pytest.mark.parametrize("suffix", ["", "_f16"])
def test_a_binding_is_dropped_by_a_call_that_fails_its_own_checks_first(suffix):
    """the window / rab / func entry points check arguments of their own in front of the plain backward, which takes the binding"""
    lib = _lib()
    bad = (H * D + 4, D, H * D, D, H * D, D)
    wrong = {"mi355_hstu_attn_bwd_window": (20, -5, b"bad window"),      # window_left
             "mi355_hstu_attn_bwd_rab": (27, None, b"rab must be"),      # rab
             "mi355_hstu_attn_bwd_func": (27, None, b"func must be"),    # func
             "mi355_hstu_attn_bwd_kv": (19, 3, b"head_dim")}             # head_dim
    for name, (pos, value, msg) in wrong.items():
        args = list(BACKWARDS[name])
        args[pos] = value
        lib.mi355_hstu_attn_bwd_bind_grad_strides(*bad)
        assert getattr(lib, name + suffix)(*args) == -1 and msg in lib.mi355_last_error(), name
        for later in BACKWARDS:
            assert _call(lib, later + suffix) == 0, f"{name}'s failed check left the binding to {later}"


PACKED_PARAMS = [("qkv", inspect.Parameter.empty), ("cu_seqlens_q", inspect.Parameter.empty), ("cu_seqlens_k", inspect.Parameter.empty),
                 ("max_seqlen_q", inspect.Parameter.empty), ("max_seqlen_k", inspect.Parameter.empty), ("num_contexts", None),
                 ("num_targets", None), ("target_group_size", 1), ("window_size", (-1, -1)), ("alpha", 1.0), ("rab", None),
                 ("has_drab", False), ("func", None), ("scaling_seqlen", -1)]
LEGACY_VARLEN_PARAMS = [("q", inspect.Parameter.empty), ("k", inspect.Parameter.empty), ("v", inspect.Parameter.empty),
                        ("cu_seqlens_q", inspect.Parameter.empty), ("cu_seqlens_k", inspect.Parameter.empty),
                        ("max_seqlen_q", inspect.Parameter.empty), ("max_seqlen_k", inspect.Parameter.empty), ("num_contexts", None),
                        ("num_targets", None), ("target_group_size", 1), ("window_size", (-1, -1)), ("alpha", 1.0), ("rab", None),
                        ("has_drab", False), ("kv_cache", None), ("page_offsets", None), ("page_ids", None), ("last_page_lens", None),
                        ("cu_seqlens_t", None), ("func", None), ("scaling_seqlen", -1)]


def _params(fn):
    sig = inspect.signature(fn)
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    return [(n, p.default) for n, p in sig.parameters.items()]


def test_signatures_are_the_reference_packages():
    import hstu
    import hstu_attn

    assert _params(hstu.hstu_attn_qkvpacked_func) == PACKED_PARAMS
    assert _params(hstu_attn.hstu_attn_qkvpacked_func) == PACKED_PARAMS
    assert _params(hstu_attn.hstu_attn_varlen_func) == LEGACY_VARLEN_PARAMS
    assert issubclass(hstu.HstuAttnQKVPackedFunc, torch.autograd.Function)


def test_hstu_attn_exports_exactly_the_two_functions():
    import hstu_attn

    assert hstu_attn.__all__ == ["hstu_attn_varlen_func", "hstu_attn_qkvpacked_func"]


def test_raw_backwards_take_keyword_only_gradients():
    import hstu

    for fn in (hstu.hstu_varlen_bwd, hstu.hstu_varlen_bwd_window, hstu.hstu_varlen_bwd_rab, hstu.hstu_varlen_bwd_func,
               hstu.hstu_varlen_bwd_kv):
        p = inspect.signature(fn).parameters
        for n in ("dq", "dk", "dv"):
            assert p[n].kind == inspect.Parameter.KEYWORD_ONLY and p[n].default is None, (fn.__name__, n)


def _packed_value_errors(call):
    """the five ValueErrors of the reference's wrappers (hstu_attn_interface.py:468-487), on CPU tensors: raised before device work"""
    cu = torch.tensor([0, 5, 12], dtype=torch.int32)
    n = torch.tensor([1, 1], dtype=torch.int32)
    with pytest.raises(ValueError, match="rab is None, but has_drab is True"):
        call(cu, 7, 7, has_drab=True)
    with pytest.raises(ValueError, match="context is True and causal is not True"):
        call(cu, 7, 7, num_contexts=n, window_size=(-1, -1))
    with pytest.raises(ValueError, match="target is True and causal is not True"):
        call(cu, 7, 7, num_targets=n, window_size=(4, 0))
    with pytest.raises(ValueError, match="target_group_size should be greater than 0"):
        call(cu, 7, 7, target_group_size=0)
    with pytest.raises(ValueError, match="seq_len_q >= seq_len_k"):
        call(cu, 8, 7)


def test_packed_value_errors_come_before_device_work():
    import hstu

    qkv = torch.zeros(12, 3, H, D, dtype=torch.bfloat16)
    _packed_value_errors(lambda cu, mq, mk, **kw: hstu.hstu_attn_qkvpacked_func(qkv, cu, cu, mq, mk, **kw))
    # a packed call is self attention
    cu = torch.tensor([0, 5, 12], dtype=torch.int32)
    with pytest.raises(ValueError, match="self attention"):
        hstu.hstu_attn_qkvpacked_func(qkv, cu, cu, 5, 7)
    with pytest.raises(ValueError, match="self attention"):
        hstu.hstu_attn_qkvpacked_func(qkv, cu, torch.tensor([0, 5, 8, 12], dtype=torch.int32), 7, 7)


def test_legacy_varlen_value_errors_come_before_device_work():
    import hstu_attn

    q = torch.zeros(12, H, D, dtype=torch.bfloat16)
    _packed_value_errors(lambda cu, mq, mk, **kw: hstu_attn.hstu_attn_varlen_func(q, q, q, cu, cu, mq, mk, **kw))
