"""Fake (meta) kernels of `INFERENCE_EMB::get_table_range` and `INFERENCE_EMB::expand_table_ids` (reference:
corelib/dynamicemb/dynamicemb/index_range_meta.py; there the second one comes from the operator library's own Meta kernel).
Same function names, checks and error texts as the reference module."""
from __future__ import annotations

import warnings
from typing import Optional

import torch

from . import inference_ops  # noqa: F401  (defines the operators)


def _validate_1d(name: str, t: torch.Tensor) -> None:
    if t.dim() != 1:
        raise RuntimeError(f"INFERENCE_EMB index-range operators expect 1D {name}, got dim={t.dim()}")


def _get_table_range_fake(offsets: torch.Tensor, feature_offsets: torch.Tensor):
    _validate_1d("offsets", offsets)
    _validate_1d("feature_offsets", feature_offsets)
    return feature_offsets.new_empty(feature_offsets.shape)


def _expand_table_ids_fake(offsets: torch.Tensor, indices: torch.Tensor,
                           table_offsets_in_feature: Optional[torch.Tensor] = None, num_tables: int = 0,
                           local_batch_size: int = 1):
    _validate_1d("offsets", offsets)
    if table_offsets_in_feature is not None:
        _validate_1d("table_offsets_in_feature", table_offsets_in_feature)
    if local_batch_size <= 0:
        raise RuntimeError("INFERENCE_EMB::expand_table_ids expects local_batch_size > 0")
    return torch.empty_like(indices, dtype=torch.int64)


def register_index_range_fake() -> bool:
    """Registers both fake kernels; True on success (also when they are there already), False with a warning otherwise."""
    try:
        inference_ops.register_fake("get_table_range", _get_table_range_fake)
        inference_ops.register_fake("expand_table_ids", _expand_table_ids_fake)
        return True
    except Exception as e:  # noqa: BLE001
        warnings.warn(f"Failed to register fake kernels for INFERENCE_EMB index-range operators. Original error: {e}",
                      RuntimeWarning, stacklevel=2)
        return False


REGISTERED = register_index_range_fake()
