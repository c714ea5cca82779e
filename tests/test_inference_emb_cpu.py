"""CPU checks of the exportable inference embedding collection: the INFERENCE_EMB operator namespace carries the reference's
schemas, every operator has a fake kernel with the reference's shape checks, an InferenceEmbeddingCollection built on the CPU
exports with a dynamic key count (only fake kernels run), and the constructor validates as the reference does."""
import importlib

import pytest
import torch

SCHEMAS = {
    "table_lookup": "INFERENCE_EMB::table_lookup(Tensor table_storage, Tensor table_bucket_offsets, int bucket_capacity, "
                    "Tensor keys, Tensor table_ids, Tensor? score_input, int policy_type, Tensor? ovf_storage=None, "
                    "int ovf_bucket_capacity=0, Tensor? ovf_output_offsets=None) -> (Tensor, Tensor, Tensor)",
    "expand_table_ids": "INFERENCE_EMB::expand_table_ids(Tensor offsets, Tensor indices, Tensor? table_offsets_in_feature=None, "
                        "int num_tables=0, int local_batch_size=1) -> Tensor",
    "get_table_range": "INFERENCE_EMB::get_table_range(Tensor offsets, Tensor feature_offsets) -> Tensor",
}


def _coll(pooling_mode=-1, fused=True, use_dynamic_hash=True, caps=(300, 500), fmap=(0, 0, 1), dim=8, **kw):
    from dynamicemb.dynamicemb_config import DynamicEmbTableOptions
    from dynamicemb.exportable_tables import InferenceEmbeddingCollection

    opts = [DynamicEmbTableOptions(dim=dim, max_capacity=c) for c in caps]
    return InferenceEmbeddingCollection(opts, use_dynamic_hash, pooling_mode, feature_table_map=list(fmap), device="cpu",
                                        fused=fused, **kw)


def _inference_ops_of(ep):
    return [str(n.target) for n in ep.graph.nodes if n.op == "call_function" and "INFERENCE_EMB" in str(n.target)]


def test_reference_schemas_character_for_character():
    import dynamicemb.inference_ops  # noqa: F401

    for name, want in SCHEMAS.items():
        assert str(getattr(torch.ops.INFERENCE_EMB, name).default._schema) == want
    assert hasattr(torch.ops.INFERENCE_EMB, "inference_emb_forward")


def test_registering_again_does_not_raise():
    import dynamicemb.inference_ops as ops
    from dynamicemb import index_range_meta, lookup_meta

    assert lookup_meta.REGISTERED and index_range_meta.REGISTERED
    ops.register()
    assert lookup_meta.register_lookup_fake() and index_range_meta.register_index_range_fake()
    importlib.reload(ops)
    test_reference_schemas_character_for_character()
    _export(_coll(), -1)   # the definitions and fake kernels survived the reload


def test_fake_kernels_shapes_dtypes_and_errors():
    import dynamicemb.inference_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        st = torch.empty(17 * 128 * 4, dtype=torch.uint8)
        tbo = torch.empty(3, dtype=torch.int64)
        keys = torch.empty(10, dtype=torch.int64)
        tids = torch.empty(10, dtype=torch.int64)
        s, f, i = torch.ops.INFERENCE_EMB.table_lookup(st, tbo, 128, keys, tids, None, 0)
        assert (s.shape, f.shape, i.shape) == ((10,), (10,), (10,))
        assert (s.dtype, f.dtype, i.dtype) == (torch.int64, torch.bool, torch.int64)
        with pytest.raises(RuntimeError, match="expects 1D keys, got dim=2"):
            torch.ops.INFERENCE_EMB.table_lookup(st, tbo, 128, keys.view(2, 5), tids, None, 0)
        with pytest.raises(RuntimeError, match="keys and table_ids to have same length"):
            torch.ops.INFERENCE_EMB.table_lookup(st, tbo, 128, keys, tids[:9], None, 0)
        with pytest.raises(RuntimeError, match="score_input length == keys length"):
            torch.ops.INFERENCE_EMB.table_lookup(st, tbo, 128, keys, tids, tids[:3], 1)
        with pytest.raises(RuntimeError, match="with ovf_storage requires ovf_output_offsets"):
            torch.ops.INFERENCE_EMB.table_lookup(st, tbo, 128, keys, tids, None, 0, st, 384, None)

        off = torch.empty(7, dtype=torch.int64)
        fo = torch.empty(3, dtype=torch.int64)
        r = torch.ops.INFERENCE_EMB.get_table_range(off, fo)
        assert r.shape == (3,) and r.dtype == torch.int64
        with pytest.raises(RuntimeError, match="index-range operators expect 1D offsets, got dim=2"):
            torch.ops.INFERENCE_EMB.get_table_range(off.view(7, 1), fo)
        t = torch.ops.INFERENCE_EMB.expand_table_ids(off, keys.to(torch.uint64), fo, 2, 1)
        assert t.shape == (10,) and t.dtype == torch.int64
        with pytest.raises(RuntimeError, match="expects local_batch_size > 0"):
            torch.ops.INFERENCE_EMB.expand_table_ids(off, keys, None, 0, 0)

        w = torch.empty(50, 8, dtype=torch.float16)
        to = torch.empty(3, dtype=torch.int64)
        po = torch.empty(5, dtype=torch.int64)
        fwd = torch.ops.INFERENCE_EMB.inference_emb_forward
        o = fwd(keys, off, fo, st, tbo, 128, to, w, None, None, -1, True, 1)
        assert o.shape == (10, 8) and o.dtype == torch.float16
        o = fwd(keys, off, fo, None, None, 0, to, w, po, None, 1, False, 1)
        assert o.shape == (4, 8) and o.dtype == torch.float16
        with pytest.raises(RuntimeError, match="requires pooling_offsets"):
            fwd(keys, off, fo, st, tbo, 128, to, w, None, None, 2, True, 1)
        with pytest.raises(RuntimeError, match="not supported with mean pooling"):
            fwd(keys, off, fo, st, tbo, 128, to, w, po, torch.empty(10), 2, True, 1)
        with pytest.raises(RuntimeError, match="expects 1D keys"):
            fwd(keys.view(5, 2), off, fo, st, tbo, 128, to, w, None, None, -1, True, 1)


def _export(m, pooling_mode, n=10):
    from torch.export import Dim, export

    keys = torch.arange(n, dtype=torch.int64)
    off = torch.tensor([0, 3, 6, n], dtype=torch.int64)
    args = (keys, off)
    shapes = {"keys": {0: Dim("n", min=2, max=1 << 24)}, "offsets": None}
    if pooling_mode != -1:
        args += (torch.tensor([0, 5, n], dtype=torch.int64),)
        shapes["pooling_offsets"] = None
    return export(m, args, dynamic_shapes=shapes)


@pytest.mark.parametrize("pooling_mode", [-1, 1, 2])
def test_export_fused_holds_the_one_fused_op(pooling_mode):
    ep = _export(_coll(pooling_mode, fused=True), pooling_mode)
    assert _inference_ops_of(ep) == ["INFERENCE_EMB.inference_emb_forward.default"]
    out = [n for n in ep.graph.nodes if n.op == "output"][0].args[0][0].meta["val"]
    assert out.shape[1] == 8 and (pooling_mode == -1) == (not isinstance(out.shape[0], int))   # (N, D) with N symbolic / (B, D)


@pytest.mark.parametrize("pooling_mode", [-1, 1, 2])
def test_export_composed_holds_exactly_the_three_reference_ops(pooling_mode):
    ep = _export(_coll(pooling_mode, fused=False), pooling_mode)
    assert sorted(_inference_ops_of(ep)) == ["INFERENCE_EMB.expand_table_ids.default", "INFERENCE_EMB.get_table_range.default",
                                             "INFERENCE_EMB.table_lookup.default"]


def test_fused_switch_on_the_module():
    m = _coll(-1, fused=True)
    m.fused = False
    assert len(_inference_ops_of(_export(m, -1))) == 3


def test_derive_grouped_offsets_and_table_offsets():
    from dynamicemb.exportable_tables import _derive_grouped_offsets

    assert _derive_grouped_offsets([0, 0, 1, 2]) == [0, 2, 3, 4]
    assert _derive_grouped_offsets([0]) == [0, 1]
    assert _derive_grouped_offsets([0, 1, 1, 1]) == [0, 1, 4]
    m = _coll(caps=(300, 500, 7), fmap=(0, 0, 1, 2))
    # cumsum of [1, cap0 + 1, cap1 + 1, cap2 + 1]; row table_offsets_[t] - 1 is table t's zero row
    assert m.table_offsets_.tolist() == [1, 302, 803, 811]
    assert m.capacity_list_.tolist() == [301, 501, 8]
    assert m.feature_offsets_.tolist() == [0, 2, 3, 4] and m.feature_table_map_.tolist() == [0, 0, 1, 2]
    assert tuple(m.weight.shape) == (301 + 501 + 8, 8) and m.weight.dtype == torch.float32
    assert not m.weight.any()
    ht = m.hash_table
    assert ht.table_bucket_offsets_.tolist() == [0, 3, 7, 8] and ht.table_storage_.numel() == 17 * 128 * 8
    assert ht.bucket_sizes.numel() == 8 and ht._ref_counter.numel() == 8 * 128
    # an empty arena: every key word is the Empty key
    assert bool((ht.table_storage_.view(8, 17 * 128)[:, : 8 * 128] == 0xFF).all())
    names = {n for n, _ in m.named_buffers()}
    assert {"feature_table_map_", "feature_offsets_", "capacity_list_", "table_offsets_", "weight", "hash_table.table_storage_",
            "hash_table.table_bucket_offsets_", "hash_table.bucket_sizes", "hash_table._ref_counter"} <= names
    assert not list(m.parameters())
    assert not hasattr(_coll(use_dynamic_hash=False), "hash_table")


def test_constructor_validation_errors():
    from dynamicemb.dynamicemb_config import DynamicEmbTableOptions
    from dynamicemb.exportable_tables import InferenceEmbeddingCollection as C

    ok = [DynamicEmbTableOptions(dim=8, max_capacity=100), DynamicEmbTableOptions(dim=8, max_capacity=100)]
    with pytest.raises(ValueError, match="pooling_mode must be -1"):
        C(ok, True, 0, device="cpu")
    with pytest.raises(ValueError, match="table_options must be non-empty"):
        C([], True, -1, device="cpu")
    with pytest.raises(ValueError, match="unsupported key_type"):
        C(ok, True, -1, device="cpu", key_type=torch.int32)
    with pytest.raises(ValueError, match="unsupported output_dtype"):
        C(ok, True, -1, device="cpu", output_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="init_capacity or max_capacity > 0"):
        C([DynamicEmbTableOptions(dim=8)], True, -1, device="cpu")
    with pytest.raises(ValueError, match="init_capacity or max_capacity > 0"):
        C([DynamicEmbTableOptions(dim=8, max_capacity=0)], True, -1, device="cpu")
    with pytest.raises(ValueError, match="exactly one shared embedding dim"):
        C([DynamicEmbTableOptions(dim=8, max_capacity=10), DynamicEmbTableOptions(dim=16, max_capacity=10)], True, -1, device="cpu")
    with pytest.raises(ValueError, match="table_names size must match"):
        C(ok, True, -1, table_names=["a"], device="cpu")
    with pytest.raises(ValueError, match="must be a non-empty list"):
        C(ok, True, -1, feature_table_map=[], device="cpu")
    with pytest.raises(ValueError, match="out-of-range table id"):
        C(ok, True, -1, feature_table_map=[0, 2], device="cpu")
    with pytest.raises(ValueError, match="must be non-decreasing"):
        C(ok, True, -1, feature_table_map=[1, 0], device="cpu")
    # init_capacity wins over max_capacity
    m = C([DynamicEmbTableOptions(dim=8, init_capacity=10, max_capacity=100, global_hbm_for_values=1 << 30)], False, 1, device="cpu")
    assert m.table_offsets_.tolist() == [1, 12]
    with pytest.raises(ValueError, match="pooling_offsets is required"):
        m(torch.arange(3), torch.tensor([0, 3]))


def test_load_from_embedding_table_layout():
    m = _coll(use_dynamic_hash=False, caps=(3, 2), fmap=(0, 1), dim=4)
    w = torch.arange(20, dtype=torch.float32).view(5, 4) + 1
    m.load_from_embedding_table(w)
    assert torch.equal(m.weight[1:4], w[:3]) and torch.equal(m.weight[5:7], w[3:])
    assert not m.weight[0].any() and not m.weight[4].any()
