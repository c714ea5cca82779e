"""`flash_attn.cute`: the interface module alone (no CuTe DSL here; block_sparsity is absent on purpose, so that the
reference's build_block_sparsity returns (None, None) and the kernel derives its own tile skipping)."""
from .interface import flash_attn_func  # noqa: F401

__all__ = ["flash_attn_func"]
