"""GPU tests of the exportable inference embedding collection (dynamicemb/exportable_tables.py, dynamicemb/inference_ops.py,
csrc/inference_emb.hip).  Expected values are computed from the key -> row dictionary that was loaded (NumPy / float64), never
from the slot indices of the code under test.

Bound of the pooled comparisons (derived, not tuned): the kernel adds L products w_i * row_i in fp32, one rounding each
(fused multiply-add), so |out - ref| <= L * 2^-24 * sum_i |w_i * row_i| before the store, plus half an ulp of the output dtype at
the reference value for the store's rounding.  Mean pooling is the sum with w_i = 1 / L (the division is one more rounding of
a value no larger than the sum of the |w_i * row_i|)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mods():
    import dynamicemb_extensions as ext
    from dynamicemb.dynamicemb_config import DynamicEmbTableOptions
    from dynamicemb.exportable_tables import InferenceEmbeddingCollection

    return ext, DynamicEmbTableOptions, InferenceEmbeddingCollection


def _collection(caps, fmap, dim, pooling_mode=-1, use_dynamic_hash=True, dtype=torch.float32, fused=True, **kw):
    _, TO, C = _mods()
    return C([TO(dim=dim, max_capacity=c) for c in caps], use_dynamic_hash, pooling_mode, feature_table_map=list(fmap),
             output_dtype=dtype, device=torch.device(DEV), fused=fused, **kw)


def _load_dict(m, t, keys_np, rows):
    """puts {key: row} of table t into the collection: hash mode through table_insert + index_copy_, identity mode by index"""
    ext = _mods()[0]
    off = int(m.table_offsets_[t].item())
    keys = torch.from_numpy(keys_np).to(DEV)
    if m.use_dynamic_hash:
        ht = m.hash_table
        idx = ext.table_insert(ht.table_storage_, ht.table_bucket_offsets_, ht.bucket_capacity_, ht.bucket_sizes, keys,
                               torch.full_like(keys, t), None, 0, ht._ref_counter, None, None)
        assert bool((idx >= 0).all()), "fixture: a bucket overflowed"
    else:
        idx = keys
    m.weight.index_copy_(0, idx + off, rows.to(DEV))


def _dict_rows(known_keys, known_rows, query):
    """rows of `query` out of the dictionary (zeros for keys it does not hold), on the CPU"""
    order = np.argsort(known_keys)
    sk = known_keys[order]
    pos = np.searchsorted(sk, query)
    pos_c = np.minimum(pos, len(sk) - 1)
    hit = sk[pos_c] == query
    out = torch.zeros(len(query), known_rows.shape[1], dtype=known_rows.dtype)
    out[torch.from_numpy(hit)] = known_rows[torch.from_numpy(order[pos_c[hit]])]
    return out


def _fixture(T, dim, dtype, use_dynamic_hash, pooling_mode=-1, cap=4096, per_table=1500, seed=0):
    """collection with T tables (one extra feature on table 0), `per_table` known keys each; -> m, [(keys, rows)] per table"""
    rng = np.random.default_rng(seed)
    fmap = [0] + list(range(T))
    m = _collection([cap] * T, fmap, dim, pooling_mode, use_dynamic_hash, dtype)
    tables = []
    for t in range(T):
        if use_dynamic_hash:
            keys = np.unique(rng.integers(0, 1 << 40, size=per_table + 64))[:per_table].astype(np.int64) * 2   # known keys are even
            rng.shuffle(keys)
        else:
            keys = rng.permutation(cap)[:per_table].astype(np.int64)
        rows = torch.from_numpy(rng.standard_normal((per_table, dim)).astype(np.float32)).to(dtype)
        _load_dict(m, t, keys, rows)
        tables.append((keys, rows))
    return m, tables, fmap


def _queries(tables, fmap, n, use_dynamic_hash, rng, cap=4096):
    """n keys, feature-major (one CSR slot per feature), about half of them unknown; -> keys, offsets, expected rows (CPU)"""
    F = len(fmap)
    cuts = np.sort(rng.integers(0, n + 1, size=F - 1)) if n else np.zeros(F - 1, dtype=np.int64)
    offsets = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    keys = np.zeros(n, dtype=np.int64)
    D = tables[0][1].shape[1]
    exp = torch.zeros(n, D, dtype=tables[0][1].dtype)
    for f, t in enumerate(fmap):
        lo, hi = offsets[f], offsets[f + 1]
        if hi == lo:
            continue
        known, rows = tables[t]
        q = known[rng.integers(0, len(known), size=hi - lo)]
        unknown = rng.random(hi - lo) < 0.5
        if use_dynamic_hash:
            q = np.where(unknown, q + 1, q)             # odd keys were never inserted
        else:
            q = np.where(unknown, rng.integers(0, cap, size=hi - lo), q)   # any row of the table: loaded or still zero
        keys[lo:hi] = q
        exp[lo:hi] = _dict_rows(known, rows, q)
    return keys, offsets, exp


def _ulp_half(ref, dtype):
    p, emin = (23, -126) if dtype == torch.float32 else (10, -14)
    _, e = np.frexp(np.abs(ref))
    return 0.5 * np.ldexp(1.0, np.maximum(e - 1, emin) - p)


def _assert_pooled(out, ref, bound_sum, lengths, dtype, what):
    """every element: |out - ref| <= L * 2^-24 * sum|w row| + half an ulp of the output dtype at ref"""
    got = out.double().cpu().numpy()
    bound = lengths[:, None] * 2.0 ** -24 * bound_sum + _ulp_half(ref, dtype)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: elements {err.size}, max |err| {err.max() if err.size else 0:.3e}, worst err / bound {worst:.3f}")
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} of {err.size} elements beyond the bound (worst ratio {worst})"


# ---------------------------------------------------------------------------------------------------- 1. operators
def test_reference_ops_equal_the_extension_ops_bit_for_bit():
    ext = _mods()[0]
    m, tables, fmap = _fixture(3, 8, torch.float32, True)
    rng = np.random.default_rng(1)
    keys, offsets, _ = _queries(tables, fmap, 5000, True, rng)
    k = torch.from_numpy(keys).to(DEV)
    off = torch.from_numpy(offsets).to(DEV)
    ht = m.hash_table
    rng_new = torch.ops.INFERENCE_EMB.get_table_range(off, m.feature_offsets_)
    assert torch.equal(rng_new, ext.get_table_range(off, m.feature_offsets_))
    tids = torch.ops.INFERENCE_EMB.expand_table_ids(off, k, m.feature_offsets_, 3, 1)
    a = torch.ops.INFERENCE_EMB.table_lookup(ht.table_storage_, ht.table_bucket_offsets_, 128, k, tids, None, 0, None, 0, None)
    b = ext.table_lookup(ht.table_storage_, ht.table_bucket_offsets_, 128, k, tids, None, 0)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert 0.3 < a[1].float().mean().item() < 0.7      # about half the keys are known
    # a feature-x-batch offsets array (B = 4)
    off4 = torch.from_numpy(np.concatenate([[0], np.cumsum(rng.integers(0, 5, size=4 * 4))]).astype(np.int64)).to(DEV)
    assert torch.equal(torch.ops.INFERENCE_EMB.get_table_range(off4, m.feature_offsets_), ext.get_table_range(off4, m.feature_offsets_))


@pytest.mark.parametrize("lbs", [1, 4])
@pytest.mark.parametrize("with_feature_offsets", [False, True])
def test_expand_table_ids_against_searchsorted(lbs, with_feature_offsets):
    import dynamicemb.inference_ops  # noqa: F401

    rng = np.random.default_rng(lbs * 2 + with_feature_offsets)
    F = 7
    lengths = rng.integers(0, 40, size=F * lbs)
    lengths[lbs * 2: lbs * 4] = 0                       # two features (a whole table below) without keys
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(offsets[-1])
    fo = np.array([0, 2, 3, 4, 7], dtype=np.int64) if with_feature_offsets else np.arange(F + 1, dtype=np.int64)
    seg = offsets[fo * lbs]
    want = np.maximum(np.searchsorted(seg, np.arange(n), side="right") - 1, 0)   # the largest t with seg[t] <= i
    keys = torch.zeros(n, dtype=torch.int64, device=DEV)
    got = torch.ops.INFERENCE_EMB.expand_table_ids(torch.from_numpy(offsets).to(DEV), keys,
                                                   torch.from_numpy(fo).to(DEV) if with_feature_offsets else None,
                                                   len(fo) - 1 if with_feature_offsets else 0, lbs)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    empty = torch.ops.INFERENCE_EMB.expand_table_ids(torch.from_numpy(offsets).to(DEV), keys[:0], None, 0, lbs)
    assert empty.dtype == torch.int64 and empty.numel() == 0


# ---------------------------------------------------------------------------------------------------- 2. round trip
def test_round_trip_from_a_trained_module(tmp_path):
    from dynamicemb.batched_dynamicemb_tables import BatchedDynamicEmbeddingTablesV2
    from dynamicemb.dynamicemb_config import DynamicEmbPoolingMode, DynamicEmbTableOptions, EmbOptimType

    D, B, fmap = 16, 8, [0, 0, 1]
    opts = [DynamicEmbTableOptions(dim=D, max_capacity=2048, index_type=torch.int64, embedding_dtype=torch.float32) for _ in range(2)]
    tr = BatchedDynamicEmbeddingTablesV2(opts, table_names=["user", "item"], feature_table_map=fmap,
                                         pooling_mode=DynamicEmbPoolingMode.NONE, optimizer=EmbOptimType.SGD, learning_rate=0.1,
                                         output_dtype=torch.float32, device=torch.device(DEV))
    rng = np.random.default_rng(7)
    tr.train()
    batches = []
    for _ in range(4):
        lengths = rng.integers(0, 6, size=len(fmap) * B)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(DEV)
        keys = torch.from_numpy(rng.integers(0, 300, size=int(lengths.sum())).astype(np.int64)).to(DEV)
        out = tr(keys, off)
        out.backward(torch.randn_like(out))
        batches.append((keys, off))
    tr.dump(str(tmp_path))
    tr.eval()

    m = _collection([4096, 4096], fmap, D, table_names=["user", "item"])
    m.load_from_dynamicemb_file(str(tmp_path))
    with torch.no_grad():
        for keys, off in batches:
            want = tr(keys, off)
            assert want.abs().sum().item() > 0
            for fused in (True, False):
                m.fused = fused
                got = m(keys, off)
                assert got.shape == want.shape and torch.equal(got, want), f"fused={fused}"
        keys, off = batches[-1]
        m.fused = True
        assert not m(keys + 1_000_000, off).any()        # unseen keys: zero rows
        # one table only: the other one's keys are unknown afterwards
        m.load_from_dynamicemb_file(str(tmp_path), table_names=["item"])
        got, want = m(keys, off), tr(keys, off)
        first_item = int(off[2 * B].item())
        assert not got[:first_item].any() and torch.equal(got[first_item:], want[first_item:])


# ---------------------------------------------------------------------------------------------------- 3. fused == composed
@pytest.mark.parametrize("use_dynamic_hash", [True, False])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("D", [8, 64, 128, 132, 7])
def test_fused_equals_composed_without_pooling(D, dtype, T, use_dynamic_hash):
    m, tables, fmap = _fixture(T, D, dtype, use_dynamic_hash)
    rng = np.random.default_rng(D * 8 + T)
    for n in (0, 1, 63, 64, 65, 100_000):
        keys, offsets, exp = _queries(tables, fmap, n, use_dynamic_hash, rng)
        k, off = torch.from_numpy(keys).to(DEV), torch.from_numpy(offsets).to(DEV)
        m.fused = True
        fused = m(k, off)
        m.fused = False
        composed = m(k, off)
        assert fused.shape == (n, D) and fused.dtype == dtype
        # bit-equal: compared as integers, so that a NaN or a signed zero could not hide a difference
        as_int = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(fused.view(as_int), composed.view(as_int)), f"n={n}"
        assert torch.equal(fused.cpu().view(as_int), exp.view(as_int)), f"n={n}: not the dictionary's rows"
        if n >= 63:
            assert int((exp.abs().sum(1) == 0).sum()) > n // 8       # unknown keys are really in there


def test_identity_keys_outside_the_table_give_zero_rows():
    m, tables, fmap = _fixture(2, 8, torch.float32, False, cap=64, per_table=64)
    keys = torch.tensor([-1, 64, 1 << 40, 3, 0, 63, 64, -5], dtype=torch.int64, device=DEV)
    off = torch.tensor([0, 2, 4, 8], dtype=torch.int64, device=DEV)         # features 0, 1 -> table 0; feature 2 -> table 1
    out = m(keys, off).cpu()
    for i, (t, k) in enumerate([(0, -1), (0, 64), (0, 1 << 40), (0, 3), (1, 0), (1, 63), (1, 64), (1, -5)]):
        want = _dict_rows(tables[t][0], tables[t][1], np.array([k], dtype=np.int64))[0]
        assert torch.equal(out[i], want), (i, t, k)
    assert not out[[0, 1, 2, 6, 7]].any() and out[[3, 4, 5]].abs().sum(1).min() > 0


def test_uint64_keys():
    m, tables, fmap = _fixture(1, 8, torch.float32, True)
    m2 = _collection([4096], fmap, 8, key_type=torch.uint64)
    m2.load_state_dict(m.state_dict())
    k = torch.from_numpy(tables[0][0][:100].copy()).to(DEV)
    off = torch.tensor([0, 50, 100], dtype=torch.int64, device=DEV)
    assert torch.equal(m2(k.view(torch.uint64), off), m(k, off)) and torch.equal(m(k, off).cpu(), tables[0][1][:100])


# ---------------------------------------------------------------------------------------------------- 4. pooling
def _bags(n_bags, rng, max_len=40):
    lengths = rng.integers(0, max_len + 1, size=n_bags)
    lengths[:3] = [0, max_len, 1]
    return lengths, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@pytest.mark.parametrize("use_dynamic_hash", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("D", [64, 7, 264])
@pytest.mark.parametrize("mode,weighted", [(1, False), (1, True), (2, False)])
def test_pooled_against_float64(mode, weighted, D, dtype, use_dynamic_hash):
    m, tables, fmap = _fixture(3, D, dtype, use_dynamic_hash, pooling_mode=mode)
    rng = np.random.default_rng(D + mode + 2 * weighted)
    lengths, pool = _bags(400, rng)
    n = int(pool[-1])
    keys, offsets, exp = _queries(tables, fmap, n, use_dynamic_hash, rng)
    w = rng.uniform(-2, 2, size=n).astype(np.float32) if weighted else None
    rows = exp.double().numpy()
    wi = np.ones(n) if w is None else w.astype(np.float64)
    if mode == 2:
        wi = wi / np.maximum(np.repeat(lengths, lengths), 1)
    ref = np.zeros((len(lengths), D))
    mag = np.zeros((len(lengths), D))
    bag_of = np.repeat(np.arange(len(lengths)), lengths)
    np.add.at(ref, bag_of, wi[:, None] * rows)
    np.add.at(mag, bag_of, np.abs(wi[:, None] * rows))
    args = (torch.from_numpy(keys).to(DEV), torch.from_numpy(offsets).to(DEV), torch.from_numpy(pool).to(DEV),
            torch.from_numpy(w).to(DEV) if weighted else None)
    out = m(*args)
    assert out.shape == (len(lengths), D) and out.dtype == dtype
    assert not out[0].any()                              # the empty bag
    _assert_pooled(out, ref, mag, lengths.astype(np.float64), dtype, f"pooled mode={mode} weighted={weighted} D={D} {dtype}")
    if not weighted:   # the composed leg (torch's embedding_bag, its own rounding order; fp16 spacing at these sums is 2^-6): a sanity check
        m.fused = False
        torch.testing.assert_close(m(*args).float(), out.float(), rtol=1e-2, atol=5e-2)


def test_weighted_mean_is_refused():
    m, tables, fmap = _fixture(1, 8, torch.float32, True, pooling_mode=2)
    k = torch.from_numpy(tables[0][0][:10].copy()).to(DEV)
    off = torch.tensor([0, 4, 10], dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="not supported with mean pooling"):
        m(k, off, off, torch.ones(10, device=DEV))
    with pytest.raises(RuntimeError, match="not supported with mean pooling"):
        ht = m.hash_table
        torch.ops.INFERENCE_EMB.inference_emb_forward(k, off, m.feature_offsets_, ht.table_storage_, ht.table_bucket_offsets_, 128,
                                                      m.table_offsets_, m.weight, off, torch.ones(10, device=DEV), 2, True, 1)


# ---------------------------------------------------------------------------------------------------- 5. export
@pytest.mark.parametrize("pooling_mode", [-1, 1])
@pytest.mark.parametrize("fused", [True, False])
def test_export_save_load_replays_eager(fused, pooling_mode, tmp_path):
    from torch.export import Dim, export

    m, tables, fmap = _fixture(3, 64, torch.float32, True, pooling_mode=pooling_mode)
    m.fused = fused
    rng = np.random.default_rng(11)

    def inputs(n):
        keys, offsets, _ = _queries(tables, fmap, n, True, rng)
        a = (torch.from_numpy(keys).to(DEV), torch.from_numpy(offsets).to(DEV))
        if pooling_mode != -1:
            a += (torch.from_numpy(np.arange(0, n + 1, n // 16, dtype=np.int64)).to(DEV),)
        return a

    shapes = {"keys": {0: Dim("n", min=2, max=1 << 24)}, "offsets": None}
    if pooling_mode != -1:
        shapes["pooling_offsets"] = None
    ep = export(m, inputs(320), dynamic_shapes=shapes)
    ops = [str(n.target) for n in ep.graph.nodes if n.op == "call_function" and "INFERENCE_EMB" in str(n.target)]
    assert len(ops) == (1 if fused else 3)
    path = str(tmp_path / "collection.pt2")
    torch.export.save(ep, path)
    replay = torch.export.load(path).module()
    for n in (320, 4800):                                 # the traced key count and another one
        a = inputs(n)
        got, want = replay(*a), m(*a)
        assert got.shape == want.shape and torch.equal(got, want) and want.abs().sum().item() > 0


# ---------------------------------------------------------------------------------------------------- 6. model surgery
def test_apply_swaps_the_embedding_collection():
    from dynamicemb._torchrec import EmbeddingCollection, EmbeddingConfig
    from dynamicemb.exportable_tables import InferenceEmbeddingCollection, apply_inference_embedding_collection

    cfgs = [EmbeddingConfig(num_embeddings=1000, embedding_dim=16, name="user", feature_names=["u0", "u1"]),
            EmbeddingConfig(num_embeddings=500, embedding_dim=16, name="item", feature_names=["i0"])]
    ec = EmbeddingCollection(tables=cfgs, device=torch.device("meta"))
    if not hasattr(ec, "embeddings"):   # the protocol stand-in: give it the real module's per-table nn.Embedding dict
        ec.embeddings = torch.nn.ModuleDict({c.name: torch.nn.Embedding(c.num_embeddings, c.embedding_dim, device="meta") for c in cfgs})

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.sparse = torch.nn.Module()
            self.sparse.ec = ec
            self.dense = torch.nn.Linear(16, 4)

    model = Toy()
    out = apply_inference_embedding_collection(model, {"user": True, "item": True}, {"user": 2000})
    assert out is model
    new = model.sparse.ec
    assert isinstance(new, InferenceEmbeddingCollection) and isinstance(model.dense, torch.nn.Linear)
    assert new.embedding_configs is cfgs or list(new.embedding_configs) == list(cfgs)
    assert new.table_names_ == ["user", "item"] and new.feature_names_ == ["u0", "u1", "i0"]
    assert new.feature_table_map_.tolist() == [0, 0, 1] and new.use_dynamic_hash and new.pooling_mode_ == -1
    assert new.table_offsets_.tolist() == [1, 2002, 2503]                 # the trained size of `user`, the config's of `item`
    assert new.weight.is_cuda and tuple(new.weight.shape) == (2001 + 501, 16)
    k = torch.arange(6, device=DEV)
    assert tuple(new(k, torch.tensor([0, 2, 4, 6], device=DEV)).shape) == (6, 16)
    # a second pass finds nothing left to convert
    apply_inference_embedding_collection(model, {"user": True, "item": True}, {})
    assert model.sparse.ec is new


# ---------------------------------------------------------------------------------------------------- 7. C2-sized smoke
def test_c2_sized_sum_pooling_against_embedding_bag():
    """1 M-row table, 360 K Zipf keys, sum pooling; the reference is torch's embedding_bag in float64 over the rows that were loaded"""
    ext = _mods()[0]
    D, rows_n, n = 128, 1 << 20, 360_000
    m = _collection([rows_n], [0], D, pooling_mode=1)
    rng = np.random.default_rng(5)
    known_n = 600_000
    dict_keys = (np.arange(known_n, dtype=np.int64) * 2654435761 + 12345) % (1 << 44)         # distinct: the multiplier is odd
    gen = torch.Generator(device=DEV).manual_seed(5)
    dict_rows = torch.randn(known_n + 1, D, device=DEV, generator=gen)
    dict_rows[known_n] = 0                                                                    # the dictionary's answer for unknown keys
    ht = m.hash_table
    inserted = torch.zeros(known_n, dtype=torch.bool, device=DEV)
    for s in range(0, known_n, 1 << 16):
        k = torch.from_numpy(dict_keys[s: s + (1 << 16)]).to(DEV)
        idx = ext.table_insert(ht.table_storage_, ht.table_bucket_offsets_, 128, ht.bucket_sizes, k, torch.zeros_like(k), None, 0,
                               ht._ref_counter, None, None)
        ok = idx >= 0
        inserted[s: s + k.numel()] = ok
        m.weight.index_copy_(0, idx[ok] + 1, dict_rows[s: s + k.numel()][ok])
    assert inserted.float().mean().item() > 0.999
    ranks = np.minimum(rng.zipf(1.2, size=n) - 1, known_n + 50_000 - 1)                      # ranks >= known_n: unknown keys
    known = ranks < known_n
    keys = np.where(known, dict_keys[np.minimum(ranks, known_n - 1)], (1 << 50) + ranks)
    lengths = rng.integers(1, 11, size=n // 5)
    lengths = lengths[np.cumsum(lengths) <= n]
    pool = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(pool[-1])
    keys, ranks, known = keys[:n], ranks[:n], known[:n]
    ref_idx = torch.from_numpy(np.where(known, ranks, known_n)).to(DEV)
    ref_idx = torch.where(inserted[ref_idx.clamp(max=known_n - 1)] | (ref_idx == known_n), ref_idx, torch.full_like(ref_idx, known_n))
    pool_t = torch.from_numpy(pool).to(DEV)
    rows64 = dict_rows.double()
    bag = torch.nn.functional.embedding_bag
    ref = bag(ref_idx, rows64, pool_t, mode="sum", include_last_offset=True).cpu().numpy()
    mag = bag(ref_idx, rows64.abs(), pool_t, mode="sum", include_last_offset=True).cpu().numpy()
    out = m(torch.from_numpy(keys).to(DEV), torch.tensor([0, n], dtype=torch.int64, device=DEV), pool_t)
    assert out.shape == (len(lengths), D)
    _assert_pooled(out, ref, mag, lengths.astype(np.float64), torch.float32, "C2-sized sum pooling")


def test_wrong_index_dtypes_and_lengths_are_refused():
    """int32 offsets (TorchRec can produce them) would be read as int64 words: refused, not misread"""
    m, tables, fmap = _fixture(3, 8, torch.float32, True, pooling_mode=1)
    k = torch.from_numpy(tables[0][0][:10].copy()).to(DEV)
    off = torch.tensor([0, 4, 6, 8, 10], dtype=torch.int64, device=DEV)
    pool = torch.tensor([0, 5, 10], dtype=torch.int64, device=DEV)
    assert tuple(m(k, off, pool).shape) == (2, 8)
    with pytest.raises(RuntimeError, match="expects int64 offsets"):
        m(k, off.int(), pool)
    with pytest.raises(RuntimeError, match="expects int64 pooling_offsets"):
        m(k, off, pool.int())
    with pytest.raises(RuntimeError, match="expects offsets on"):
        m(k, off.cpu(), pool)
    with pytest.raises(RuntimeError, match="expects int64 offsets"):
        torch.ops.INFERENCE_EMB.expand_table_ids(off.int(), k, None, 0, 1)
    with pytest.raises(RuntimeError, match="of length num_tables \\+ 1"):
        torch.ops.INFERENCE_EMB.expand_table_ids(off, k, m.feature_offsets_, 2, 1)
