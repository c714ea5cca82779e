"""DynamicEmbDump / DynamicEmbLoad (reference dump_load.py:103-330): save / restore every dynamic embedding table of a
model in the reference's wire format -- one folder per embedding collection (named by the collection's path in the model),
per table and rank the raw little-endian files `<table>_emb_{keys,values,scores,opt_values}.rank_R.world_size_W` plus
`<table>_opt_args.json` (written / read by BatchedDynamicEmbeddingTablesV2.dump / .load)."""
import glob
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch.distributed as dist
from torch import nn


def dump_key_files(save_dir: str, table_name: str) -> List[str]:
    """the key files of one table in a dump folder, every rank's"""
    return sorted(glob.glob(os.path.join(save_dir, f"{table_name}_emb_keys.rank_*.world_size_*")))


def iter_dump_batches(save_dir: str, table_name: str, key_file: str, dim: int, opt_dim: int = 0, batch: int = 1 << 16):
    """Batches of one rank's files of a table (`key_file` is one of `dump_key_files`): NumPy arrays
    (keys i64[n], embeddings f32[n, dim], scores i64[n] or None, optimizer state f32[n, opt_dim] or None).  Scores are None when
    the score file is missing; the optimizer state when opt_dim == 0 or its file is missing."""
    suffix = key_file[key_file.index("_emb_keys") + len("_emb_keys"):]
    path = lambda item: os.path.join(save_dir, f"{table_name}_emb_{item}{suffix}")  # noqa: E731
    nkeys = os.path.getsize(key_file) // 8
    with open(key_file, "rb") as fk, open(path("values"), "rb") as fv:
        fs = open(path("scores"), "rb") if os.path.exists(path("scores")) else None
        fo = open(path("opt_values"), "rb") if (opt_dim and os.path.exists(path("opt_values"))) else None
        try:
            for start in range(0, nkeys, batch):
                n = min(batch, nkeys - start)
                keys = np.frombuffer(fk.read(8 * n), dtype=np.int64)
                emb = np.frombuffer(fv.read(4 * dim * n), dtype=np.float32).reshape(n, dim)
                sc = np.frombuffer(fs.read(8 * n), dtype=np.int64) if fs else None
                op = np.frombuffer(fo.read(4 * opt_dim * n), dtype=np.float32).reshape(n, opt_dim) if fo else None
                yield keys, emb, sc, op
        finally:
            if fs:
                fs.close()
            if fo:
                fo.close()


def _unwrap(m: nn.Module) -> nn.Module:
    """wrappers that only forward (DistributedModelParallel, DDP, Float16Module) do not show up in a collection's path"""
    while True:
        inner = getattr(m, "_dmp_wrapped_module", None)
        if inner is None and type(m).__name__ in ("DistributedDataParallel", "Float16Module", "DDP"):
            inner = getattr(m, "module", None)
        if not isinstance(inner, nn.Module):
            return m
        m = inner


def find_sharded_modules(model: nn.Module, path: str = "model") -> List[Tuple[str, nn.Module]]:
    """(path, module) of every sharded collection that holds dynamic embedding tables; paths start at "model" and skip
    wrapper modules, as the folder names of the reference's dumps do (dump_load.py:31-50)"""
    model = _unwrap(model)
    if hasattr(model, "dynamic_embedding_modules"):
        return [(path, model)]
    found = []
    for name, child in model.named_children():
        found.extend(find_sharded_modules(child, f"{path}.{name}" if path else name))
    return found


def get_dynamic_emb_module(model: nn.Module) -> List[nn.Module]:
    """every BatchedDynamicEmbeddingTablesV2 under `model`"""
    return [m for _, coll in find_sharded_modules(model) for m in coll.dynamic_embedding_modules()]


def _barrier(pg) -> None:
    if dist.is_available() and dist.is_initialized():
        dist.barrier(group=pg)


def DynamicEmbDump(path: str, model: nn.Module, table_names: Optional[Dict[str, List[str]]] = None,
                   optim: Optional[bool] = False, counter: Optional[bool] = False, pg=None,
                   allow_overwrite: bool = False) -> None:
    """table_names: {collection path: [table names]} to restrict the dump (default: everything)"""
    colls = find_sharded_modules(model)
    rank = dist.get_rank(group=pg) if dist.is_available() and dist.is_initialized() else 0
    if rank == 0:
        os.makedirs(path, exist_ok=True)
    _barrier(pg)
    for cpath, coll in colls:
        if table_names is not None and cpath not in table_names:
            continue
        folder = os.path.join(path, cpath)
        if rank == 0:
            if os.path.isdir(folder) and os.listdir(folder) and not allow_overwrite:
                raise FileExistsError(f"{folder} is not empty (pass allow_overwrite=True to replace the dump)")
            os.makedirs(folder, exist_ok=True)
        _barrier(pg)
        only = None if table_names is None else table_names[cpath]
        for m in coll.dynamic_embedding_modules():
            m.dump(folder, optim=bool(optim), counter=bool(counter), table_names=only, pg=pg)
    _barrier(pg)


def DynamicEmbLoad(path: str, model: nn.Module, table_names: Optional[Dict[str, List[str]]] = None,
                   optim: bool = False, counter: bool = False, pg=None) -> None:
    """every rank reads every file of a table and keeps the keys it owns (`key % world_size == rank`), so a dump taken
    with one world size loads into another"""
    for cpath, coll in find_sharded_modules(model):
        if table_names is not None and cpath not in table_names:
            continue
        folder = os.path.join(path, cpath)
        if not os.path.isdir(folder):
            raise FileNotFoundError(f"no dump of collection {cpath!r} under {path}")
        only = None if table_names is None else table_names[cpath]
        for m in coll.dynamic_embedding_modules():
            m.load(folder, optim=optim, counter=counter, table_names=only, pg=pg)
    _barrier(pg)
