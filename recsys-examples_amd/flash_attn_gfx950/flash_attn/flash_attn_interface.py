"""`flash_attn.flash_attn_interface` of flash-attn 2 as far as the reference calls it: both functions return `out` alone.
Arguments this kernel does not carry (dropout, window, softcap, alibi, attention probabilities) are refused unless they have
their defaults.  Both are differentiable in q, k, v (softmax_attn.py)."""
import softmax_attn as _P


def flash_attn_func(q, k, v, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0,
                    alibi_slopes=None, deterministic=False, return_attn_probs=False):
    return _P.flash_attn_func(q, k, v, softmax_scale=softmax_scale, causal=causal, dropout_p=dropout_p,
                              window_size=window_size, softcap=softcap, alibi_slopes=alibi_slopes,
                              deterministic=deterministic, return_attn_probs=return_attn_probs)


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=0.0,
                           softmax_scale=None, causal=False, window_size=(-1, -1), softcap=0.0, alibi_slopes=None,
                           deterministic=False, return_attn_probs=False, block_table=None):
    return _P.flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                                     softmax_scale=softmax_scale, causal=causal, dropout_p=dropout_p,
                                     window_size=window_size, softcap=softcap, alibi_slopes=alibi_slopes,
                                     deterministic=deterministic, return_attn_probs=return_attn_probs,
                                     block_table=block_table)
