"""The `INFERENCE_EMB` operator namespace of the reference's inference path on MI355X.

Importing this module registers, under `torch.ops.INFERENCE_EMB`, the three operators the reference builds into
`inference_emb_ops.so` (corelib/dynamicemb/src/table_operation/{lookup,expand_table_ids,get_table_range}_torch_binding.cu) with
the same schemas, so `examples/hstu/modules/exportable_embedding.py` and the `inference_aoti/` export scripts call them
unchanged -- and a fourth operator of this project, `inference_emb_forward`: the whole forward of an
`InferenceEmbeddingCollection` as one kernel launch (csrc/inference_emb.hip).

The CUDA implementations sit over the C ABI (include/recsys_amd.h); there is no CPU implementation.  Every operator has a
fake kernel (`dynamicemb.lookup_meta`, `dynamicemb.index_range_meta`, and below), so `torch.export` traces them without a GPU.
Registration is idempotent: an operator that is already defined -- by an earlier import, or by a real `inference_emb_ops`
library -- keeps its definition, and a CUDA kernel is only added where none exists."""
from __future__ import annotations

from typing import Optional

import torch

NAMESPACE = "INFERENCE_EMB"

SCHEMAS = {
    "table_lookup": "table_lookup(Tensor table_storage, Tensor table_bucket_offsets, int bucket_capacity, Tensor keys, "
                    "Tensor table_ids, Tensor? score_input, int policy_type, Tensor? ovf_storage=None, "
                    "int ovf_bucket_capacity=0, Tensor? ovf_output_offsets=None) -> (Tensor, Tensor, Tensor)",
    "expand_table_ids": "expand_table_ids(Tensor offsets, Tensor indices, Tensor? table_offsets_in_feature=None, "
                        "int num_tables=0, int local_batch_size=1) -> Tensor",
    "get_table_range": "get_table_range(Tensor offsets, Tensor feature_offsets) -> Tensor",
    # this project's fused forward: keys [N] -> rows [N, D] (pooling_mode -1) or bags [B, D] (1 sum, 2 mean)
    "inference_emb_forward": "inference_emb_forward(Tensor keys, Tensor offsets, Tensor feature_offsets, "
                             "Tensor? table_storage, Tensor? table_bucket_offsets, int bucket_capacity, Tensor table_offsets, "
                             "Tensor weight, Tensor? pooling_offsets, Tensor? per_sample_weights, int pooling_mode, "
                             "bool use_dynamic_hash, int local_batch_size=1) -> Tensor",
}


def _has_op(name: str) -> bool:
    try:
        torch._C._dispatch_find_schema_or_throw(f"{NAMESPACE}::{name}", "")
        return True
    except RuntimeError:
        return False


def _has_kernel(name: str, key: str) -> bool:
    return torch._C._dispatch_has_kernel_for_dispatch_key(f"{NAMESPACE}::{name}", key)


# ------------------------------------------------------------------------------------------ CUDA kernels (C ABI)
def _table_lookup_cuda(table_storage, table_bucket_offsets, bucket_capacity, keys, table_ids, score_input, policy_type,
                       ovf_storage=None, ovf_bucket_capacity=0, ovf_output_offsets=None):
    import dynamicemb_extensions as ext

    if ovf_storage is not None and ovf_output_offsets is None:
        raise RuntimeError("INFERENCE_EMB::table_lookup with ovf_storage requires ovf_output_offsets")
    return ext.table_lookup(table_storage, table_bucket_offsets, bucket_capacity, keys.contiguous(), table_ids.contiguous(),
                            score_input, policy_type, ovf_storage, ovf_bucket_capacity, ovf_output_offsets)


def _expand_table_ids_cuda(offsets, indices, table_offsets_in_feature=None, num_tables=0, local_batch_size=1):
    import mi355_native as N

    if not offsets.is_cuda:
        raise RuntimeError("INFERENCE_EMB::expand_table_ids expects CUDA offsets.")
    fo = table_offsets_in_feature
    if fo is not None and not fo.is_cuda:
        raise RuntimeError("INFERENCE_EMB::expand_table_ids expects CUDA table_offsets_in_feature when provided.")
    n = indices.size(0)
    out = torch.empty(n, dtype=torch.int64, device=offsets.device)
    if n == 0:
        return out
    if local_batch_size <= 0:
        raise RuntimeError("INFERENCE_EMB::expand_table_ids expects local_batch_size > 0")
    if fo is not None and fo.numel() == 0:
        fo = None
    _check_index_tensor("expand_table_ids", "offsets", offsets, offsets.device)
    _check_index_tensor("expand_table_ids", "table_offsets_in_feature", fo, offsets.device)
    if fo is not None and fo.numel() != num_tables + 1:
        raise RuntimeError(f"INFERENCE_EMB::expand_table_ids expects table_offsets_in_feature of length num_tables + 1 "
                           f"({num_tables + 1}), got {fo.numel()}")
    N.require_contiguous(offsets, fo)
    N.check(N.lib().mi355_inference_expand_table_ids(N.ptr(offsets), offsets.numel(), N.ptr(fo), int(num_tables),
                                                     int(local_batch_size), n, N.ptr(out), N.stream()), "expand_table_ids")
    return out


def _check_index_tensor(op: str, name: str, t, device) -> None:
    """offset / index arrays are read as int64 words on the device of the call"""
    if t is None:
        return
    if t.dtype != torch.int64:
        raise RuntimeError(f"INFERENCE_EMB::{op} expects int64 {name}, got {t.dtype}")
    if t.device != device:
        raise RuntimeError(f"INFERENCE_EMB::{op} expects {name} on {device}, got {t.device}")


def _get_table_range_cuda(offsets, feature_offsets):
    import dynamicemb_extensions as ext

    return ext.get_table_range(offsets, feature_offsets)


def _out_shape(keys, weight, pooling_offsets, per_sample_weights, pooling_mode):
    """shape checks shared by the real and the fake kernel of the fused forward"""
    if keys.dim() != 1:
        raise RuntimeError(f"INFERENCE_EMB::inference_emb_forward expects 1D keys, got dim={keys.dim()}")
    if weight.dim() != 2:
        raise RuntimeError(f"INFERENCE_EMB::inference_emb_forward expects 2D weight, got dim={weight.dim()}")
    if pooling_mode not in (-1, 1, 2):
        raise RuntimeError(f"INFERENCE_EMB::inference_emb_forward expects pooling_mode -1, 1 or 2, got {pooling_mode}")
    if pooling_mode == -1:
        return (keys.size(0), weight.size(1))
    if pooling_offsets is None:
        raise RuntimeError("INFERENCE_EMB::inference_emb_forward with pooling requires pooling_offsets")
    if pooling_offsets.dim() != 1:
        raise RuntimeError(f"INFERENCE_EMB::inference_emb_forward expects 1D pooling_offsets, got dim={pooling_offsets.dim()}")
    if per_sample_weights is not None:
        if pooling_mode == 2:   # (torch.nn.EmbeddingBag refuses it as well)
            raise RuntimeError("INFERENCE_EMB::inference_emb_forward: per_sample_weights is not supported with mean pooling")
        if per_sample_weights.dim() != 1 or per_sample_weights.size(0) != keys.size(0):
            raise RuntimeError("INFERENCE_EMB::inference_emb_forward expects per_sample_weights length == keys length")
    return (pooling_offsets.size(0) - 1, weight.size(1))


def _inference_emb_forward_cuda(keys, offsets, feature_offsets, table_storage, table_bucket_offsets, bucket_capacity,
                                table_offsets, weight, pooling_offsets, per_sample_weights, pooling_mode, use_dynamic_hash,
                                local_batch_size=1):
    import mi355_native as N

    shape = _out_shape(keys, weight, pooling_offsets, per_sample_weights, pooling_mode)
    if keys.dtype not in (torch.int64, torch.uint64):
        raise ValueError(f"unsupported key_type: {keys.dtype}")
    if weight.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"unsupported output_dtype: {weight.dtype}")
    if use_dynamic_hash and (table_storage is None or table_bucket_offsets is None):
        raise RuntimeError("INFERENCE_EMB::inference_emb_forward with use_dynamic_hash requires the table arena")
    for name, t in (("offsets", offsets), ("feature_offsets", feature_offsets), ("table_offsets", table_offsets),
                    ("pooling_offsets", pooling_offsets), ("table_bucket_offsets", table_bucket_offsets if use_dynamic_hash else None)):
        _check_index_tensor("inference_emb_forward", name, t, weight.device)
    for name, t in (("keys", keys), ("table_storage", table_storage if use_dynamic_hash else None), ("per_sample_weights", per_sample_weights)):
        if t is not None and t.device != weight.device:
            raise RuntimeError(f"INFERENCE_EMB::inference_emb_forward expects {name} on {weight.device}, got {t.device}")
    T = table_offsets.numel() - 1
    if feature_offsets.numel() != T + 1:
        raise RuntimeError("INFERENCE_EMB::inference_emb_forward expects feature_offsets and table_offsets of equal length")
    psw = per_sample_weights
    if psw is not None and psw.dtype != torch.float32:
        psw = psw.float()
    keys = keys.contiguous()
    N.require_contiguous(offsets, feature_offsets, table_storage, table_bucket_offsets, table_offsets, weight, pooling_offsets, psw)
    out = torch.empty(shape, dtype=weight.dtype, device=weight.device)
    pooled = pooling_mode != -1
    N.check(N.lib().mi355_inference_emb_forward(
        N.ptr(keys), keys.numel(), N.ptr(offsets), offsets.numel(), N.ptr(feature_offsets), T, int(local_batch_size),
        N.ptr(table_storage if use_dynamic_hash else None), N.ptr(table_bucket_offsets if use_dynamic_hash else None),
        int(bucket_capacity), N.ptr(table_offsets), N.ptr(weight), weight.size(1), N.dt(weight),
        N.ptr(pooling_offsets if pooled else None), shape[0] if pooled else 0, N.ptr(psw if pooled else None),
        int(pooling_mode), int(bool(use_dynamic_hash)), N.ptr(out), N.stream()), "inference_emb_forward")
    return out


def _inference_emb_forward_fake(keys, offsets, feature_offsets, table_storage, table_bucket_offsets, bucket_capacity,
                                table_offsets, weight, pooling_offsets, per_sample_weights, pooling_mode, use_dynamic_hash,
                                local_batch_size=1):
    if offsets.dim() != 1:
        raise RuntimeError(f"INFERENCE_EMB::inference_emb_forward expects 1D offsets, got dim={offsets.dim()}")
    return weight.new_empty(_out_shape(keys, weight, pooling_offsets, per_sample_weights, pooling_mode))


_CUDA = {
    "table_lookup": _table_lookup_cuda,
    "expand_table_ids": _expand_table_ids_cuda,
    "get_table_range": _get_table_range_cuda,
    "inference_emb_forward": _inference_emb_forward_cuda,
}

# (module reload: the Library object that owns the definitions lives on)
_lib = globals().get("_lib") or torch.library.Library(NAMESPACE, "FRAGMENT")
_fake_done = globals().get("_fake_done") or set()


def register_fake(name: str, fn) -> bool:
    """fake kernel of INFERENCE_EMB::<name>, once; an operator that already has a Meta kernel (a real library) keeps it"""
    if name in _fake_done or _has_kernel(name, "Meta"):
        return True
    torch.library.register_fake(f"{NAMESPACE}::{name}", lib=_lib)(fn)
    _fake_done.add(name)
    return True


def register() -> None:
    for name, schema in SCHEMAS.items():
        if not _has_op(name):
            _lib.define(schema)
        if not _has_kernel(name, "CUDA"):
            _lib.impl(name, _CUDA[name], "CUDA")
    register_fake("inference_emb_forward", _inference_emb_forward_fake)


register()

from . import index_range_meta, lookup_meta  # noqa: E402,F401  (the fake kernels of the three reference operators)
