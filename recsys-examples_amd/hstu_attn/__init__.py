"""Drop-in for the `hstu_attn` package of the reference (corelib/hstu/hstu_attn/__init__.py:16-18), whose kernel test imports
`from hstu_attn import hstu_attn_varlen_func, hstu_attn_qkvpacked_func` (corelib/hstu/test.py).  Both run the gfx950 kernels of
the `hstu` package next to this one; `hstu_attn_varlen_func` here has that package's LEGACY parameter order."""
from .hstu_attn_interface import hstu_attn_qkvpacked_func, hstu_attn_varlen_func

__all__ = ["hstu_attn_varlen_func", "hstu_attn_qkvpacked_func"]
