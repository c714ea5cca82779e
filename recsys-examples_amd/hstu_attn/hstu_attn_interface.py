"""The two functions of the reference's `hstu_attn` package on top of `hstu`."""
import hstu
from hstu import hstu_attn_qkvpacked_func  # noqa: F401  (same signature in both packages)


def hstu_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, num_contexts=None, num_targets=None,
                          target_group_size=1, window_size=(-1, -1), alpha=1.0, rab=None, has_drab=False, kv_cache=None,
                          page_offsets=None, page_ids=None, last_page_lens=None, cu_seqlens_t=None, func=None, scaling_seqlen=-1):
    """hstu_attn_varlen_func with the legacy parameter order (corelib/hstu/hstu_attn/hstu_attn_interface.py:185-279): a thin
    adapter onto hstu.hstu_attn_varlen_func, which has the order the example pins.  The checks the legacy function makes itself
    raise the same ValueErrors; `cu_seqlens_t` (target offsets of the reference's paged-cache calls, hstu_api.cpp:141) has no kernel here and must be None."""
    if num_targets is None and target_group_size < 1:
        raise ValueError("AssertError: target_group_size should be greater than 0 when target is True")
    if max_seqlen_q > max_seqlen_k:
        raise ValueError("AssertError: seq_len_q >= seq_len_k, this is undefined behavior")
    if cu_seqlens_t is not None:
        raise NotImplementedError("cu_seqlens_t is not supported")
    return hstu.hstu_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, None, None, max_seqlen_q, max_seqlen_k, scaling_seqlen,
                                      num_contexts, num_targets, target_group_size, tuple(window_size), alpha, rab, has_drab,
                                      kv_cache, page_offsets, page_ids, last_page_lens, func)
