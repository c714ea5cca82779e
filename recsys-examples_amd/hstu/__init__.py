"""Drop-in for the `hstu` package of the reference (pip `fbgemm_gpu_hstu`, built from the un-vendored
third_party/FBGEMM submodule): `hstu_attn_varlen_func` with the positional order the example pins
(examples/hstu/modules/hstu_attention.py:296-314, test/hstu_attn/test_hstu_attn_smoke.py:105-121), on top of
the gfx950 MFMA kernels (mi355_hstu_attn_fwd / mi355_hstu_attn_bwd), and `hstu_attn_qkvpacked_func` of the reference's own
kernel package (corelib/hstu/hstu_attn/hstu_attn_interface.py:432-506; the package `hstu_attn` next to this one carries that
package's import names and legacy argument order).
"""
from .hstu_attn_interface import (HstuAttnVarlenFunc, HstuAttnWindowFunc, append_kvcache, hstu_attn_varlen_func,  # noqa: F401
                                  hstu_varlen_bwd, hstu_varlen_bwd_window, hstu_varlen_fwd, hstu_varlen_fwd_kv,
                                  hstu_varlen_fwd_window, HstuAttnRabFunc, hstu_varlen_fwd_rab, hstu_varlen_bwd_rab,
                                  HstuAttnDeltaQFunc, hstu_varlen_bwd_kv, HstuAttnQKVPackedFunc, hstu_attn_qkvpacked_func,
                                  hstu_varlen_bwd_func, HstuAttnRabFuncFunc, hstu_varlen_fwd_rab_func, hstu_varlen_bwd_rab_func)
from .hstu_fp8 import (HstuAttnFp8Func, get_bm_and_bn_block_size_bwd, get_bm_and_bn_block_size_fwd,  # noqa: F401
                       quantize_for_backward, quantize_for_block_scale, quantize_for_head_batch_tensor,
                       quantize_for_two_directions, varlen_bwd, varlen_fwd)

try:  # `import hstu` registers torch.ops.fbgemm.hstu_varlen_* (the example relies on it: fused_hstu_op.py:19)
    from . import hstu_ops_gpu  # noqa: F401
except Exception as _e:  # pragma: no cover - e.g. a torch build without torch.library
    import warnings

    warnings.warn(f"hstu: torch.ops.fbgemm.hstu_varlen_* were not registered ({_e})")
