"""`flash_attn.cute.interface.flash_attn_func` as the reference calls it: returns (out, lse).  arbitrary=True takes
aux_tensors=[arbitrary_func]; the linear_*_block_sparse_tensors (forward and backward ones) are accepted and not read.
Differentiable in q, k, v (softmax_attn.py); lse carries no gradient."""
import softmax_attn as _P


def flash_attn_func(q, k, v, softmax_scale=None, causal=False, arbitrary=False, linear_k_block_sparse_tensors=None,
                    linear_q_block_sparse_tensors=None, aux_tensors=None, **unsupported):
    return _P.flash_attn_func(q, k, v, softmax_scale=softmax_scale, causal=causal, arbitrary=arbitrary,
                              linear_k_block_sparse_tensors=linear_k_block_sparse_tensors,
                              linear_q_block_sparse_tensors=linear_q_block_sparse_tensors, aux_tensors=aux_tensors,
                              return_lse=True, **unsupported)
