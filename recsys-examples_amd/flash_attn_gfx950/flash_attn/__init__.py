"""Stand-in for the `flash_attn` package on MI355X: the three import paths the semantic-ID generative-retrieval code uses
(`flash_attn.flash_attn_func`, `flash_attn.flash_attn_interface.flash_attn_varlen_func`, `flash_attn.cute.interface.
flash_attn_func`), forward and backward, on the HIP kernels of recsys-examples_amd/softmax_attn.py (the forward is the kernel
of prefill_attn.py; q, k and v receive gradients through csrc/softmax_attn_bwd.hip).

Put the PARENT of this directory (flash_attn_gfx950/) on sys.path.  It is deliberately not a top-level directory of the
package, so that it never shadows a real flash-attn installation by accident.
"""
import os
import sys

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _PKG not in sys.path:  # (flash_attn_gfx950/ may be all the caller put on the path)
    sys.path.insert(0, _PKG)

from .flash_attn_interface import flash_attn_func, flash_attn_varlen_func  # noqa: E402

__all__ = ["flash_attn_func", "flash_attn_varlen_func"]
