"""Exportable inference embedding collection (reference: corelib/dynamicemb/dynamicemb/exportable_tables.py), for MI355X.

A frozen, buffer-only module that serves what `BatchedDynamicEmbeddingTablesV2` trained: a `LinearBucketTable` arena without
optimizer or score state (one score word per slot, never written at inference) and one dense `weight` buffer
`[sum(capacity + 1), D]` in HBM -- the place of the reference's NVE layer -- whose section `t` starts with an all-zero row that
unknown keys land on.  `forward` is made of `torch.ops.INFERENCE_EMB` operators only (`dynamicemb.inference_ops`), so
`torch.export` traces it (with fake kernels; no GPU needed for that):

* `fused=True` (default): the one-launch forward of this project, `INFERENCE_EMB::inference_emb_forward`
  (csrc/inference_emb.hip) -- the exported graph holds one node;
* `fused=False`: the reference's own graph -- `get_table_range` / `expand_table_ids`, `table_lookup`, `index_select`, then
  a torch gather or `embedding_bag` -- the comparison leg of the fused operator.

Names, constructor arguments, buffer names and methods are the reference's."""
from __future__ import annotations

import itertools
import os
import warnings
from typing import Dict, List, Optional

import torch
from torch.nn import ModuleDict

from . import inference_ops  # noqa: F401  (registers torch.ops.INFERENCE_EMB)
from .dump_load import dump_key_files, iter_dump_batches
from .dynamicemb_config import DynamicEmbInitializerArgs, DynamicEmbInitializerMode, DynamicEmbTableOptions

try:  # the TorchRec config type of `create_inference_embedding_collection` / `apply_inference_embedding_collection`
    from ._torchrec import EmbeddingConfig
except ImportError:  # no TorchRec: the collection itself (DynamicEmbTableOptions in, tensors out) does not need it
    EmbeddingConfig = None

# (dynamicemb_extensions.ScorePolicy without importing the native loader at module import)
_POLICY_CONST, _POLICY_ASSIGN = 0, 1
_EMPTY_KEY = 0xFFFFFFFFFFFFFFFF


def _resolve_capacity(opt) -> int:
    """`init_capacity`, else `max_capacity` (a TorchRec config: `num_embeddings`); must be > 0"""
    cap = getattr(opt, "init_capacity", None)
    if cap is None:
        cap = getattr(opt, "max_capacity", None)
    if cap is None:
        cap = getattr(opt, "num_embeddings", None)
    if cap is None or cap <= 0:
        raise ValueError("Each table option must provide init_capacity or max_capacity > 0")
    return int(cap)


def _resolve_embedding_dim(table_options) -> int:
    dims = set()
    for opt in table_options:
        d = getattr(opt, "dim", None)
        if d is None:
            d = getattr(opt, "embedding_dim", None)
        if d is not None:
            dims.add(int(d))
    if len(dims) != 1:
        raise ValueError("InferenceEmbeddingTable requires exactly one shared embedding dim across all table_options")
    dim = dims.pop()
    if dim <= 0:
        raise ValueError("Embedding dim must be > 0")
    return dim


def _derive_grouped_offsets(feature_table_map: List[int]) -> List[int]:
    """boundaries of the runs of equal table ids: [0, 0, 1, 2] -> [0, 2, 3, 4]"""
    offsets = [0]
    for i in range(1, len(feature_table_map)):
        if feature_table_map[i] != feature_table_map[i - 1]:
            offsets.append(i)
    offsets.append(len(feature_table_map))
    return offsets


def _fmix64(k: int) -> int:
    m = (1 << 64) - 1
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & m
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & m
    k ^= k >> 33
    return k


def _empty_arena(storage: torch.Tensor, num_buckets: int, bucket_capacity: int) -> None:
    """LinearBucketTable._init_table: every key Empty, every digest the Empty key's, scores 0"""
    if storage.is_cuda:
        import dynamicemb_extensions as ext

        ext.table_init(storage, bucket_capacity, num_buckets, 1)
        return
    # (a collection on the CPU exists to be exported; the same bytes without the kernel)
    b = storage.view(num_buckets, 17 * bucket_capacity)
    b[:, : 8 * bucket_capacity] = 0xFF
    b[:, 8 * bucket_capacity: 9 * bucket_capacity] = ((_fmix64(_EMPTY_KEY) & 0x7FFFFFFFFFFFFFFF) >> 32) & 0xFF
    b[:, 9 * bucket_capacity:] = 0


class InferenceLinearBucketTable(torch.nn.Module):
    """Lookup-only hash table of the inference collection: the single-score `LinearBucketTable` arena (17 bytes per slot) as
    buffers, looked up through `INFERENCE_EMB::table_lookup`."""

    def __init__(self, capacity: List[int], key_type: torch.dtype = torch.int64, bucket_capacity: int = 128,
                 device: Optional[torch.device] = None):
        super().__init__()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.key_type_ = key_type
        self.bucket_capacity_ = bucket_capacity
        self.num_tables_ = len(capacity)
        bucket_offsets = [0]
        for cap in capacity:
            bucket_offsets.append(bucket_offsets[-1] + (cap + bucket_capacity - 1) // bucket_capacity)
        self.num_buckets_ = bucket_offsets[-1]
        self.capacity_ = self.num_buckets_ * bucket_capacity
        self.register_buffer("table_storage_", torch.zeros(17 * self.capacity_, dtype=torch.uint8, device=device))
        self.register_buffer("table_bucket_offsets_", torch.tensor(bucket_offsets, dtype=torch.int64, device=device))
        self.register_buffer("bucket_sizes", torch.zeros(self.num_buckets_, dtype=torch.int32, device=device))
        self.register_buffer("_ref_counter", torch.zeros(self.capacity_, dtype=torch.int32, device=device))
        self.score_policy = _POLICY_CONST
        self.reset()

    def reset(self) -> None:
        _empty_arena(self.table_storage_, self.num_buckets_, self.bucket_capacity_)
        self.bucket_sizes.zero_()
        self._ref_counter.zero_()

    def lookup(self, keys: torch.Tensor, table_ids: torch.Tensor, score_value: Optional[torch.Tensor] = None,
               score_policy: int = 0) -> tuple:
        """(scores, founds, table-relative slot indices or -1); scores are not touched (ScorePolicy.CONST)"""
        return torch.ops.INFERENCE_EMB.table_lookup(self.table_storage_, self.table_bucket_offsets_, self.bucket_capacity_,
                                                    keys, table_ids, score_value, self.score_policy, None, 0, None)


class InferenceEmbeddingCollection(torch.nn.Module):
    """Export-compatible embedding collection over custom operators.

    `pooling_mode` is fixed at construction: -1 no pooling, `forward` returns `(N, D)`; 1 sum / 2 mean, `(B, D)`.
    `table_options`: `DynamicEmbTableOptions` (or TorchRec `EmbeddingConfig`s); `global_hbm_for_values` is accepted and
    ignored -- the reference sizes an NVE cache with it, here the whole `weight` is one HBM buffer.  `fused` (an extension):
    see the module docstring; it can also be flipped on the module (`m.fused = False`) before a call or an export."""

    def __init__(self, table_options, use_dynamic_hash: bool, pooling_mode: int, table_names: Optional[List[str]] = None,
                 feature_names: Optional[List[str]] = None, feature_table_map: Optional[List[int]] = None,
                 output_dtype: torch.dtype = torch.float32, device: Optional[torch.device] = None,
                 key_type: torch.dtype = torch.int64, fused: bool = True):
        super().__init__()
        self.embedding_configs = table_options
        if pooling_mode not in (-1, 1, 2):
            raise ValueError(f"pooling_mode must be -1 (no pooling), 1 (sum), or 2 (mean), got {pooling_mode}")
        if not table_options:
            raise ValueError("table_options must be non-empty")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if key_type not in (torch.int64, torch.uint64):
            raise ValueError(f"unsupported key_type: {key_type}")
        if output_dtype not in (torch.float32, torch.float16):
            raise ValueError(f"unsupported output_dtype: {output_dtype}")
        capacities = [_resolve_capacity(opt) for opt in table_options]
        num_tables = len(table_options)
        if table_names is None:
            table_names = [f"table_{i}" for i in range(num_tables)]
        if len(table_names) != num_tables:
            raise ValueError("table_names size must match table_options")
        if feature_table_map is None:
            feature_table_map = list(range(num_tables))
        if not isinstance(feature_table_map, list) or len(feature_table_map) == 0:
            raise ValueError("feature_table_map must be a non-empty list")
        if any(t < 0 or t >= num_tables for t in feature_table_map):
            raise ValueError(f"feature_table_map contains out-of-range table id (must be in [0, {num_tables}))")
        if any(b < a for a, b in zip(feature_table_map, feature_table_map[1:])):
            raise ValueError("feature_table_map must be non-decreasing (features for the same table must be contiguous)")
        feature_offsets = _derive_grouped_offsets(feature_table_map)
        if len(feature_offsets) != num_tables + 1:
            raise ValueError("feature_table_map must name every table (each table needs at least one feature)")
        self.emb_dim_ = _resolve_embedding_dim(table_options)

        self.device = device
        self.output_dtype_ = output_dtype
        self.key_type_ = key_type
        self.num_tables_ = num_tables
        self.num_features_ = len(feature_table_map)
        self.table_names_ = table_names
        self.feature_names_ = feature_names
        self.pooling_mode_ = pooling_mode       # plain Python values: constants of an exported graph
        self.score_policy = _POLICY_CONST
        self.use_dynamic_hash = bool(use_dynamic_hash)
        self.fused = bool(fused)

        rows = [c + 1 for c in capacities]      # every section starts with the row of the keys that are not found
        self.register_buffer("feature_table_map_", torch.tensor(feature_table_map, dtype=torch.int64, device=device))
        self.register_buffer("feature_offsets_", torch.tensor(feature_offsets, dtype=torch.int64, device=device))
        self.register_buffer("capacity_list_", torch.tensor(rows, dtype=torch.int64, device=device))
        self.register_buffer("table_offsets_", torch.tensor(list(itertools.accumulate([1] + rows)), dtype=torch.int64,
                                                            device=device))
        if self.use_dynamic_hash:
            self.hash_table = InferenceLinearBucketTable(capacity=capacities, key_type=key_type, bucket_capacity=128,
                                                         device=device)
        self.register_buffer("weight", torch.zeros(sum(rows), self.emb_dim_, dtype=output_dtype, device=device))

    # ------------------------------------------------------------------------------------------------ loading
    def load_from_embedding_table(self, table_weights: torch.Tensor) -> None:
        """`table_weights` `[sum of capacities, D]`: the rows of all tables, table after table (row i of table t is the row of
        slot / identity index i).  The last table takes whatever rows remain."""
        assert table_weights.size(0) <= self.weight.size(0) - self.num_tables_, (
            f"Provided table_weights has more rows ({table_weights.size(0)}) than the collection holds "
            f"({self.weight.size(0) - self.num_tables_} excluding the reserved 'not found' rows)")
        assert table_weights.size(1) == self.emb_dim_, (
            f"Provided table_weights has embedding dim {table_weights.size(1)}, expected {self.emb_dim_}")
        self.weight.zero_()
        offs = self.table_offsets_.tolist()
        for t in range(self.num_tables_):
            src = offs[t] - t - 1           # the same table in a layout without the reserved rows
            n = offs[t + 1] - offs[t] - 1
            if t == self.num_tables_ - 1:
                n = table_weights.size(0) - src
            self.weight[offs[t]: offs[t] + n].copy_(table_weights[src: src + n].to(self.weight.dtype))

    def load_from_dynamicemb_file(self, save_dir: str, table_names: Optional[List[str]] = None) -> None:
        """Reads the per-table files `BatchedDynamicEmbeddingTablesV2.dump` writes (`<table>_emb_{keys,values,scores}.rank_R.
        world_size_W`, every rank's), inserts the keys into the hash table and stores their rows.  Keys the table cannot
        take (their bucket is full) are counted and warned about.  The hash table has ceil(capacity / 128) buckets of 128
        slots, so with a capacity that is not a multiple of 128 a key can be given a slot index >= capacity, for which
        `weight` has no row: the load then raises "insufficient rows" (as the reference, one index earlier: see below).
        Round the capacity up to a multiple of 128 to rule that out."""
        if not os.path.exists(save_dir):
            raise RuntimeError(f"Save directory does not exist: {save_dir}")
        if not self.use_dynamic_hash:
            raise RuntimeError("load_from_dynamicemb_file needs use_dynamic_hash=True (use load_from_embedding_table)")
        import dynamicemb_extensions as ext

        wanted = set(self.table_names_ if table_names is None else table_names)
        ht, dev, D = self.hash_table, self.device, self.emb_dim_
        ht.reset()
        self.weight.zero_()
        offs = self.table_offsets_.tolist()
        for t, name in enumerate(self.table_names_):
            if name not in wanted:
                continue
            key_files = dump_key_files(save_dir, name)
            if not key_files:
                print(f"[INFO] No checkpoint files found for table: {name}")
                continue
            rows_t = offs[t + 1] - offs[t] - 1
            for kf in key_files:
                for k_np, e_np, s_np, _ in iter_dump_batches(save_dir, name, kf, D):
                    n = k_np.size
                    keys = torch.from_numpy(k_np.copy()).to(dev)
                    emb = torch.from_numpy(e_np.copy()).to(dev)
                    scores = torch.from_numpy(s_np.copy()).to(dev) if s_np is not None else None
                    tids = torch.full((n,), t, dtype=torch.int64, device=dev)
                    idx = ext.table_insert(ht.table_storage_, ht.table_bucket_offsets_, ht.bucket_capacity_, ht.bucket_sizes,
                                           keys, tids, scores, _POLICY_ASSIGN if scores is not None else _POLICY_CONST,
                                           ht._ref_counter, None, None)
                    ok = idx >= 0
                    failed = n - int(ok.sum().item())
                    if failed:
                        print(f"[WARN] table_insert failed for {failed} keys in table {name}.")
                        warnings.warn(f"table_insert failed for {failed} keys in table {name}.", RuntimeWarning, stacklevel=2)
                    idx = idx[ok]
                    if idx.numel() == 0:
                        continue
                    top = int(idx.max().item())
                    # (the reference compares with capacity + 1, which lets index == capacity through onto the NEXT
                    #  table's reserved row)
                    if top >= rows_t:
                        raise RuntimeError(f"weight has insufficient rows ({rows_t}) for loaded index {top}.")
                    self.weight.index_copy_(0, idx + offs[t], emb[ok].to(self.weight.dtype))

    # ------------------------------------------------------------------------------------------------ forward
    def forward(self, keys: torch.Tensor, offsets: torch.Tensor, pooling_offsets: Optional[torch.Tensor] = None,
                per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """keys `(N,)` int64 / uint64, of all tables and bags; offsets: CSR boundaries of the feature slots inside `keys`
        (they give every key its table); pooling_offsets `(B+1,)`: the bags, required when pooling; per_sample_weights
        `(N,)` (sum pooling only).  Returns `(N, D)` without pooling, `(B, D)` with."""
        pooled = self.pooling_mode_ >= 0
        if pooled and pooling_offsets is None:
            raise ValueError("pooling_offsets is required when pooling_mode is 1 (sum) or 2 (mean)")
        if per_sample_weights is not None and self.pooling_mode_ == 2:
            raise ValueError("per_sample_weights is not supported with mean pooling (as torch.nn.EmbeddingBag)")
        ht = self.hash_table if self.use_dynamic_hash else None
        if self.fused:
            return torch.ops.INFERENCE_EMB.inference_emb_forward(
                keys, offsets, self.feature_offsets_, ht.table_storage_ if ht is not None else None,
                ht.table_bucket_offsets_ if ht is not None else None, ht.bucket_capacity_ if ht is not None else 0,
                self.table_offsets_, self.weight, pooling_offsets if pooled else None,
                per_sample_weights if pooled else None, self.pooling_mode_, self.use_dynamic_hash,
                (offsets.size(0) - 1) // self.num_features_)
        # the reference's graph: table boundaries inside `keys`, a table id per key, slot indices, absolute rows, gather
        table_range = torch.ops.INFERENCE_EMB.get_table_range(offsets, self.feature_offsets_)
        table_ids = torch.ops.INFERENCE_EMB.expand_table_ids(table_range, keys, None, self.num_tables_, 1)
        if ht is not None:
            _scores, _founds, index = ht.lookup(keys=keys, table_ids=table_ids, score_value=None, score_policy=self.score_policy)
        else:
            index = keys.view(torch.int64) if keys.dtype == torch.uint64 else keys
        rows = index + torch.index_select(self.table_offsets_, 0, table_ids)
        if not pooled:
            return torch.index_select(self.weight, 0, rows)
        psw = per_sample_weights.to(self.weight.dtype) if per_sample_weights is not None else None
        return torch.nn.functional.embedding_bag(rows, self.weight, pooling_offsets, mode="sum" if self.pooling_mode_ == 1 else "mean",
                                                 per_sample_weights=psw, include_last_offset=True)


def create_inference_embedding_collection(embedding_configs: List["EmbeddingConfig"], pooling_mode: int = -1, use_dynamic: bool = True
                                          ) -> InferenceEmbeddingCollection:
    """collection for TorchRec `EmbeddingConfig`s: one table per config, its features in order"""
    table_names = [c.name for c in embedding_configs]
    feature_names = list(itertools.chain(*[c.feature_names for c in embedding_configs]))
    feature_table_map = list(itertools.chain(*[[i] * len(c.feature_names) for i, c in enumerate(embedding_configs)]))
    table_options = [DynamicEmbTableOptions(embedding_dtype=torch.float32, dim=c.embedding_dim, max_capacity=c.num_embeddings,
                                            local_hbm_for_values=0, bucket_capacity=128,
                                            initializer_args=DynamicEmbInitializerArgs(mode=DynamicEmbInitializerMode.NORMAL),
                                            training=False) for c in embedding_configs]
    return InferenceEmbeddingCollection(table_options, use_dynamic, pooling_mode, table_names, feature_names,
                                        feature_table_map, device=torch.device("cuda"))


def _is_embedding_collection(module: torch.nn.Module) -> bool:
    """a TorchRec `EmbeddingCollection`: `embedding_configs()` and an `embeddings` ModuleDict of nn.Embedding"""
    if isinstance(module, InferenceEmbeddingCollection) or not callable(getattr(module, "embedding_configs", None)):
        return False
    emb = getattr(module, "embeddings", None)
    return isinstance(emb, ModuleDict) and len(emb) > 0 and all(isinstance(m, torch.nn.Embedding) for m in emb.values())


def apply_inference_embedding_collection(model: torch.nn.Module, dynamic_table_configs: Dict[str, bool],
                                         trained_emb_table_sizes: Dict[str, int]):
    """Replaces every TorchRec `EmbeddingCollection` under `model` by an `InferenceEmbeddingCollection`.

    dynamic_table_configs: table name -> use_dynamic_hash (one value per collection); trained_emb_table_sizes: table name ->
    rows of the trained table (default: the config's `num_embeddings`).  Returns `model`."""
    targets = [(name, m) for name, m in model.named_modules() if name and _is_embedding_collection(m)]
    for name, module in targets:
        configs = module.embedding_configs()
        for c in configs:
            if c.name not in trained_emb_table_sizes:
                print(f"[WARNING] Table {c.name} in module {name} is missing the trained vocab size for inference.\n"
                      f"          Using {c.num_embeddings} rows from the training config.")
            c.num_embeddings = trained_emb_table_sizes.get(c.name, c.num_embeddings)
        use_dynamic = {c.name: dynamic_table_configs[c.name] for c in configs if c.name in dynamic_table_configs}
        assert len(use_dynamic) > 0, \
            "At least one table in the embedding collection module should have a config in dynamic_table_configs."
        assert len(set(use_dynamic.values())) == 1, \
            f"All tables in the same embedding collection module should have the same config in dynamic_table_configs. Got:\n{use_dynamic}"
        pooling = getattr(configs[0], "pooling", "NONE")
        pooling = getattr(pooling, "name", pooling)
        if pooling not in ("NONE", "SUM", "MEAN"):
            raise ValueError(f"Unsupported pooling config: {pooling}")
        coll = create_inference_embedding_collection(configs, {"NONE": -1, "SUM": 1, "MEAN": 2}[pooling],
                                                     next(iter(use_dynamic.values())))
        coll.embedding_configs = configs
        parent_name, _, attr = name.rpartition(".")
        setattr(model.get_submodule(parent_name) if parent_name else model, attr, coll)
        print(f"[INFO] converting {name} to InferenceEmbeddingCollection with use_dynamic={next(iter(use_dynamic.values()))} "
              f"and tables={coll.table_names_}")
    return model
