"""Fake (meta) kernel of `INFERENCE_EMB::table_lookup` (reference: corelib/dynamicemb/dynamicemb/lookup_meta.py): shapes and
dtypes only, so `torch.export` / `torch.compile` trace the lookup without running it.  Same function names, checks and error
texts as the reference module; `REGISTERED` says whether the operator has its fake kernel."""
from __future__ import annotations

import warnings
from typing import Optional

import torch

from . import inference_ops  # noqa: F401  (defines the operator)


def _validate_1d(name: str, t: torch.Tensor) -> None:
    if t.dim() != 1:
        raise RuntimeError(f"INFERENCE_EMB::table_lookup expects 1D {name}, got dim={t.dim()}")


def _table_lookup_fake(table_storage: torch.Tensor, table_bucket_offsets: torch.Tensor, bucket_capacity: int,
                       keys: torch.Tensor, table_ids: torch.Tensor, score_input: Optional[torch.Tensor], policy_type: int,
                       ovf_storage: Optional[torch.Tensor] = None, ovf_bucket_capacity: int = 0,
                       ovf_output_offsets: Optional[torch.Tensor] = None):
    _validate_1d("keys", keys)
    _validate_1d("table_ids", table_ids)
    n = keys.numel()
    if table_ids.numel() != n:
        raise RuntimeError("INFERENCE_EMB::table_lookup expects keys and table_ids to have same length")
    if score_input is not None and score_input.numel() != n:
        raise RuntimeError("INFERENCE_EMB::table_lookup expects score_input length == keys length")
    if ovf_storage is not None and ovf_output_offsets is None:
        raise RuntimeError("INFERENCE_EMB::table_lookup with ovf_storage requires ovf_output_offsets")
    # (score_out, founds, indices)
    return (keys.new_empty((n,), dtype=torch.int64), keys.new_empty((n,), dtype=torch.bool),
            keys.new_empty((n,), dtype=torch.int64))


def register_lookup_fake() -> bool:
    """Registers the fake kernel; True on success (also when it is there already), False with a warning otherwise."""
    try:
        return inference_ops.register_fake("table_lookup", _table_lookup_fake)
    except Exception as e:  # noqa: BLE001
        warnings.warn(f"Failed to register fake kernel for INFERENCE_EMB::table_lookup. Original error: {e}", RuntimeWarning,
                      stacklevel=2)
        return False


REGISTERED = register_lookup_fake()
