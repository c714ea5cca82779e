"""CPU checks of the HSTU positional encoder: the float64 twin (tests/position_twin.py) against answers worked out by hand, the
timestamp generator's margin property, the argument checks of hstu_position / split_2D_jagged that run before any launch, and the
new entry points of the built library."""
import ctypes

import pytest
import torch

import position_twin as T


def _off(*lengths):
    return torch.tensor([0] + list(torch.tensor(lengths).cumsum(0)), dtype=torch.int64)


# ---- the twin against hand-written answers ----
def test_twin_position_index_by_hand():
    assert T.position_index(_off(5), torch.tensor([3]), 8).tolist() == [0, 1, 2, 3, 3]
    # longer than the table: rows past K - 1 share the last row whatever high says
    assert T.position_index(_off(10), torch.tensor([20]), 4).tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 3, 3]
    assert T.position_index(_off(3), torch.tensor([0]), 8).tolist() == [0, 0, 0]
    # two sequences, the second shifted by 2: 2, 3, then everything from high = 4 on
    assert T.position_index(_off(2, 4), torch.tensor([9, 4]), 8, torch.tensor([0, 2])).tolist() == [0, 1, 2, 3, 4, 4]


def test_twin_forward_and_row_sums_by_hand():
    jag = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    dense = torch.tensor([[10.0, 20.0], [100.0, 200.0]])
    out, mag = T.add_position_embeddings(jag, _off(3), torch.tensor([1]), dense, scale=2.0)
    assert out.tolist() == [[12.0, 24.0], [106.0, 208.0], [110.0, 212.0]]
    assert mag.tolist() == [[12.0, 24.0], [106.0, 208.0], [110.0, 212.0]]
    total, mags, count = T.rows_sum(torch.tensor([[1.0, -1.0], [2.0, 2.0], [-4.0, 3.0]]), torch.tensor([0, 1, 1]), 3)
    assert total.tolist() == [[1.0, -1.0], [-2.0, 5.0], [0.0, 0.0]]
    assert mags.tolist() == [[1.0, 1.0], [6.0, 5.0], [0.0, 0.0]]
    assert count.tolist() == [1.0, 2.0, 0.0]


@pytest.mark.parametrize("mcsl,interleave,Np,expected", [
    (0, False, 16, [4, 3, 2, 1, 0, 0]),     # high = 6 - 2: counts back from the first target, the targets share row 0
    (2, False, 16, [0, 1, 4, 3, 2, 2]),     # shifted by 2, the two contextual rows keep their own index
    (0, True, 16, [2, 1, 0, 0, 0, 0]),      # interleaved: high = 6 - 2 * 2
    (2, True, 16, [0, 1, 2, 2, 2, 2]),
    (0, False, 4, [3, 3, 2, 1, 0, 0]),      # capped at the last row of the table
])
def test_twin_timestamp_position_index_by_hand(mcsl, interleave, Np, expected):
    p = T.timestamp_position_index(_off(6), torch.tensor([6]), torch.tensor([2]), interleave, mcsl, Np)
    assert p.tolist() == expected
    if not interleave:   # no targets at all: high = 6
        p = T.timestamp_position_index(_off(6), torch.tensor([6]), None, False, 0, 16)
        assert p.tolist() == [6, 5, 4, 3, 2, 1]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_twin_bucket_at_exact_squares(dtype):
    # (fp32, the kernel's format, tells one second apart only below 2^24 s: m = 2047 is for the float64 twin alone)
    m = torch.tensor([1, 2, 3, 7, 45, 500] + ([2047] if dtype == torch.float64 else []), dtype=torch.int64)
    dt = 60 * m * m
    assert T.time_bucket(dt, "sqrt", dtype=dtype).tolist() == m.tolist()
    assert T.time_bucket(dt - 1, "sqrt", dtype=dtype).tolist() == (m - 1).tolist()
    assert T.time_bucket(dt + 1, "sqrt", dtype=dtype).tolist() == m.tolist()
    # the ends: nothing below bucket 0, nothing above the last
    assert T.time_bucket(torch.tensor([0, -5, 59, 60 * 2048 * 2048, 10 ** 12]), "sqrt", dtype=dtype).tolist() == [0, 0, 0, 2048, 2048]
    assert T.time_bucket(torch.tensor([0, 59, 60, 163, 164]), "log", dtype=dtype).tolist() == [0, 0, 0, 0, 1]   # 60 e = 163.1


@pytest.mark.parametrize("fn", ["sqrt", "log"])
def test_generated_timestamps_keep_their_margin(fn):
    off = _off(0, 1, 7, 67, 130, 40)
    ts = T.make_timestamps(off, fn, seed=3, recent=(4, 120))
    dt = T.time_deltas(off, ts)
    assert bool(T.buckets_are_safe(dt, fn).all())
    # so fp32 and fp64 put every row in the same bucket
    assert torch.equal(T.time_bucket(dt, fn, dtype=torch.float32), T.time_bucket(dt, fn))
    # the deliberate rows: dt = 0 at every sequence's end, a negative dt, and (sqrt) one past the last bucket
    assert int((dt == 0).sum()) >= 5 and int((dt < 0).sum()) >= 3
    t = T.time_bucket(dt, fn)
    if fn == "sqrt":
        assert int((t == 2048).sum()) >= 3
    assert int((t[75:205] == 0).sum()) >= 120   # `recent`: 120 rows of the 130-row sequence in bucket 0
    assert not bool(T.buckets_are_safe(torch.tensor([60 * 9 + 1]), "sqrt").all())   # (the property can fail)


# ---- argument checks that need no device ----
def _pos_args(D=8, B=2):
    return dict(jagged=torch.zeros(5, D), jagged_offsets=torch.tensor([0, 2, 5]), high_inds=torch.tensor([2, 3]), max_seq_len=3,
                dense=torch.zeros(4, D))


def test_add_position_embeddings_argument_errors():
    import hstu_position as P
    import mi355_native as N

    with pytest.raises(ValueError, match="2-D"):
        P.add_position_embeddings(**{**_pos_args(), "jagged": torch.zeros(5)})
    with pytest.raises(ValueError, match="2-D"):
        P.add_position_embeddings(**{**_pos_args(), "dense": torch.zeros(4, 8, 1)})
    with pytest.raises(ValueError, match=r"shape\[1\]"):
        P.add_position_embeddings(**{**_pos_args(), "dense": torch.zeros(4, 16)})
    with pytest.raises(ValueError, match="jagged_offsets"):
        P.add_position_embeddings(**{**_pos_args(), "high_inds": torch.tensor([2, 3, 4])})
    with pytest.raises(ValueError, match="ind_offsets"):
        P.add_position_embeddings(**_pos_args(), ind_offsets=torch.tensor([1]))
    with pytest.raises(ValueError, match="float32 or"):
        P.add_position_embeddings(**{**_pos_args(), "dense": torch.zeros(4, 8, dtype=torch.float16)})
    with pytest.raises(N.NativeError, match="GPU"):   # well-formed, but on the CPU: no fallback
        P.triton_add_position_embeddings(**_pos_args())


def _ts_args(D=8):
    return dict(seq_embeddings=torch.zeros(5, D), seq_offsets=torch.tensor([0, 2, 5]), pos_embeddings=torch.zeros(4, D),
                ts_embeddings=torch.zeros(9, D), timestamps=torch.zeros(5, dtype=torch.int64), max_seq_len=3,
                max_contextual_seq_len=0, seq_lengths=torch.tensor([2, 3]), num_targets=None, interleave_targets=False,
                time_bucket_fn="sqrt")


def test_add_timestamp_positional_embeddings_argument_errors():
    import hstu_position as P
    import mi355_native as N

    with pytest.raises(ValueError, match="2-D"):
        P.add_timestamp_positional_embeddings(**{**_ts_args(), "seq_embeddings": torch.zeros(5)})
    with pytest.raises(ValueError, match=r"shape\[1\]"):
        P.add_timestamp_positional_embeddings(**{**_ts_args(), "ts_embeddings": torch.zeros(9, 4)})
    with pytest.raises(ValueError, match="time_bucket_fn"):
        P.add_timestamp_positional_embeddings(**{**_ts_args(), "time_bucket_fn": "cbrt"})
    with pytest.raises(ValueError, match="seq_offsets"):
        P.add_timestamp_positional_embeddings(**{**_ts_args(), "seq_offsets": torch.tensor([0, 5])})
    with pytest.raises(ValueError, match="timestamps"):
        P.add_timestamp_positional_embeddings(**{**_ts_args(), "timestamps": torch.zeros(4, dtype=torch.int64)})
    with pytest.raises(ValueError, match="num_targets"):
        P.add_timestamp_positional_embeddings(**{**_ts_args(), "num_targets": torch.tensor([1])})
    with pytest.raises(N.NativeError, match="GPU"):
        P.triton_add_timestamp_positional_embeddings(**_ts_args())


def test_encoder_has_the_reference_parameters():
    import hstu_position as P

    enc = P.HSTUPositionalEncoder(num_position_buckets=16, num_time_buckets=2048, embedding_dim=8,
                                  training_dtype=torch.bfloat16, is_inference=False, use_time_encoding=True,
                                  static_max_seq_len=64)
    assert enc._position_embeddings_weight.shape == (16, 8) and enc._timestamp_embeddings_weight.shape == (2049, 8)
    assert float(enc._position_embeddings_weight.detach().abs().max()) <= 0.25
    plain = P.HSTUPositionalEncoder(16, 2048, 8, torch.bfloat16, use_time_encoding=False)
    assert [n for n, _ in plain.named_parameters()] == ["_position_embeddings_weight"]
    high = P._get_high_inds(torch.tensor([3, 40, 9]), plain._position_embeddings_weight, torch.tensor([1, 2, 9]), False)
    assert high.tolist() == [2, 15, 0]
    assert P._get_high_inds(torch.tensor([9]), plain._position_embeddings_weight, torch.tensor([2]), True).tolist() == [5]


def test_split_2D_jagged_argument_errors():
    import hstu_cuda_ops as H
    import mi355_native as N

    v, o = torch.zeros(6, 4), torch.tensor([0, 2, 3])
    with pytest.raises(NotImplementedError, match="n_prefix_to_right"):
        H.split_2D_jagged(v, 3, offsets_a=o, offsets_b=o, n_prefix_to_right=1)
    with pytest.raises(ValueError, match="both be None"):
        H.split_2D_jagged(v, 3)
    with pytest.raises(ValueError, match="2-D"):
        H.split_2D_jagged(torch.zeros(6), 3, offsets_a=o, offsets_b=o)
    with pytest.raises(ValueError, match="same number"):
        H.split_2D_jagged(v, 3, offsets_a=o, offsets_b=torch.tensor([0, 3]))
    with pytest.raises(N.NativeError, match="GPU"):
        H.triton_split_2D_jagged(v, 3, offsets_a=o, offsets_b=o)
    assert H.triton_split_2D_jagged is H.split_2D_jagged


# ---- the library ----
def test_library_exports_the_position_entry_points():
    import mi355_native as N

    lib = N.lib()
    for name in ("mi355_hstu_add_position_embeddings", "mi355_hstu_add_position_embeddings_bwd",
                 "mi355_hstu_add_position_embeddings_bwd_workspace_bytes", "mi355_hstu_add_timestamp_position_embeddings",
                 "mi355_hstu_index_rows_sum", "mi355_hstu_index_rows_sum_workspace_bytes"):
        assert hasattr(lib, name) and name in N.exported_symbols()
    # (chunks + owners) fp32 rows: 130 rows are 3 chunks of 64, 130 list entries 5 chunks of 32 (64 from 2^18 entries on)
    assert lib.mi355_hstu_add_position_embeddings_bwd_workspace_bytes(130, 6, 72) == (3 + 6) * 72 * 4
    assert lib.mi355_hstu_index_rows_sum_workspace_bytes(130, 48, 72) == (5 + 48) * 72 * 4
    assert lib.mi355_hstu_index_rows_sum_workspace_bytes(1 << 18, 48, 72) == (4096 + 48) * 72 * 4


def test_position_entry_points_reject_bad_arguments():
    import mi355_native as N

    lib = N.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    rc = lib.mi355_hstu_add_position_embeddings(p, 8, 4, 0, 1, p, p, None, 1, p, 8, 4, 0, 1.0, p, 8, None)
    assert rc == -1 and b"D must be" in lib.mi355_last_error()
    rc = lib.mi355_hstu_add_position_embeddings(p, 8, 4, 8, 1, p, p, None, 1, p, 8, 4, 2, 1.0, p, 8, None)
    assert rc == -1 and b"fp32 or" in lib.mi355_last_error()   # bf16 rows, fp16 table
    rc = lib.mi355_hstu_add_position_embeddings_bwd(p, 8, 4, 8, 1, p, p, 1, 1.0, None, 0, p, 8, 4, 0, None, 0, None)
    assert rc == -1 and b"workspace" in lib.mi355_last_error()
    rc = lib.mi355_hstu_add_timestamp_position_embeddings(p, 8, 4, 8, 1, p, p, 1, p, 8, 4, p, 8, 4, 0, p, None, 0, 0, 2, 2048,
                                                          60.0, 1.0, 0, p, 8, None, None, None)
    assert rc == -1 and b"time_bucket_fn" in lib.mi355_last_error()
    rc = lib.mi355_hstu_index_rows_sum(p, 4, 4, 8, 1, p, p, 4, p, 8, 4, 0, p, 1 << 20, None)
    assert rc == -1 and b"stride" in lib.mi355_last_error()
