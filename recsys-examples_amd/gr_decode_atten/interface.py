"""Stand-in for the reference's `corelib/gr_decode_atten/interface.py` on MI355X.

`examples/sid-gr-inference` binds its decode attention by putting the directory named by GR_DECODE_ATTEN_ROOT on sys.path and
importing a module called `interface` (existing_kernel_backend.py:80-98).  Pointing GR_DECODE_ATTEN_ROOT at THIS directory
makes that import find the HIP implementation; nothing from cutlass or quack is needed.
"""
import os
import sys

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:  # (the directory may be all the caller put on the path)
    sys.path.insert(0, _PKG)

from beam_decode_attn import BeamDecodeAttn, beam_decode_attn, num_splits  # noqa: E402,F401

__all__ = ["BeamDecodeAttn", "beam_decode_attn"]
