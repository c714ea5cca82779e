"""The per-op chain of the embedding forward (csrc/value_ops.hip, csrc/gather_dev.h) at small shapes, one case per dispatch
class of launch_pooled and of the sequence gather (cases, references and bag layouts: tests/forward_cases.py; that the
references can be met and reject seeded mistakes: tests/test_forward_variants_cpu.py), the flat-table copy, the row-address
and sum_chunks kernels, and the one-kernel eval forward (gather_pooled_eval_kernel / gather_rows_eval_kernel) at bag
lengths designed for its split between the run's first LPR keys and the keys probed per bag.

Pooled and sequence outputs are compared BIT FOR BIT with the fp32 sum in key order (oracle.gather_pooled /
gather_sequence) -- the kernels' own promise -- and, element by element, with the fp64 value and forward_bound
(|err| / bound <= 1).  Output, source and dense buffers are interiors of larger allocations with sentinel-filled guard
blocks; row addresses stay inside the source allocation.  Everything an op does not own -- guards, the pad of a row stride,
rows past n_dev, the source, the state part of table rows -- is compared bit for bit, and a second run into a fresh
sentinel-filled output must give the same bytes (no atomics on this path)."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import forward_cases as fc  # noqa: E402
from forward_cases import CASES, FLAT_CASES, GUARD, SEQ_CASES  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from oracle.vec_twin import VecEmbeddingTwin, bound_use, forward_bound  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
_TI = {"f32": torch.int32, "bf16": torch.int16, "f16": torch.int16}
_NI = {"f32": np.int32, "bf16": np.int16, "f16": np.int16}


def _record(kind, case, use):
    try:
        from conftest import record_tolerance_use
        record_tolerance_use(kind, case, float(use))
    except ImportError:
        pass


def _alloc(bits, dtype):
    """a whole allocation on the device from its bit patterns"""
    return torch.from_numpy(np.ascontiguousarray(bits).view(_NI[dtype])).to(DEV).view(_TD[dtype])


def _bits(t, dtype):
    return t.contiguous().view(_TI[dtype]).cpu().numpy().view(fc.BITS[dtype])


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(DEV)


def _addresses(interior, slots, stride, dtype):
    """absolute row addresses inside `interior` (0: no row)"""
    a = np.where(slots >= 0, interior.data_ptr() + slots * stride * fc.EB[dtype], 0).astype(np.int64)
    end = interior.data_ptr() + interior.numel() * fc.EB[dtype]
    assert ((a == 0) | ((a >= interior.data_ptr()) & (a + stride * fc.EB[dtype] <= end))).all()
    return a


# ------------------------------------------------------------------------------------------------ pooled gather
def _run_pooled(case, inp, src, out):
    """one mi355_gather_pooled of `case` from the allocation `src` into the allocation `out`; returns the dispatch class
    the arguments select"""
    import dynamicemb_extensions as e
    from mi355_native import check, dt, lib, ptr, stream
    D, TD, st, n = case.D, case.total_D, case.stride, inp["n"]
    src_in = src[GUARD:-GUARD].view(-1, st)
    out_in = out[GUARD:-GUARD].view(fc.B, TD)
    offsets, doff = _i64(inp["offsets"]), None
    if inp["D_offsets"] is not None:
        doff = torch.from_numpy(inp["D_offsets"]).to(DEV)
    al = fc._aligned(D, TD, st if case.src == "dense" else 0) and out_in.data_ptr() % 16 == 0
    if doff is not None:
        al = al and bool((inp["D_offsets"] % 4 == 0).all())
    comb = int(case.mean)
    if case.src == "dense":
        inp_t = src_in[:, :D]
        assert inp_t.stride(0) == st and inp_t.data_ptr() % 16 == 0
        e.gather_embedding_pooled(inp_t, out_in, _i64(inp["rev"]), offsets, comb, TD, fc.B, doff, D)
    else:
        addr = _addresses(src_in, inp["slots"], st, case.sdt)
        if al:                                                # vector kernels read 4 elements per lane
            assert (addr % (4 * fc.EB[case.sdt]) == 0).all()
        if case.src == "addr":
            e.gather_embedding_pooled(None, out_in, _i64(inp["rev"]), offsets, comb, TD, fc.B, doff, D, row_addr=_i64(addr),
                                      src_dtype=_TD[case.sdt])
        else:                                                 # one address per occurrence, no reverse index: the C ABI
            occ = _i64(addr[inp["rev"]])
            check(lib().mi355_gather_pooled(None, 0, ptr(occ), dt(_TD[case.sdt]), None, n, ptr(offsets), fc.FB, fc.B, comb, D,
                                            ptr(doff), TD, ptr(out_in), dt(out_in), int(al), stream()), "gather_pooled")
    torch.cuda.synchronize()
    return fc.pooled_class(D, al, case.src != "dense", case.src != "occ", n, fc.FB, doff is not None, st)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_pooled_gather_bit_for_bit(case):
    """MEAN included: the division of the fp32 sum by the bag length is correctly rounded on the device (measured on the
    MI355X: every MEAN case of this file agrees with the NumPy division to the bit)."""
    inp = fc.make_inputs(case)
    ref = fc.reference(case, inp)
    src = _alloc(inp["src_bits"], case.sdt)
    out = _alloc(inp["out0"], case.ddt)
    klass = _run_pooled(case, inp, src, out)
    assert klass == case.klass, f"{case.name}: the arguments select {klass}, the case is listed as {case.klass}"
    if "_unr" in klass:
        assert (inp["n"] <= 8 * fc.FB) == ("_unr4_" in klass)
    got = _bits(out, case.ddt)
    use, same, foreign = fc.judge(case, ref, got)
    worst = float(use.max())
    print(f"forward_variants_use {case.klass:26s} s={case.sdt:4s} d={case.ddt:4s} {'mean' if case.mean else 'sum ':4s} "
          f"{worst:.4f} bit_identical={bool(same.all())}  ({case.name})")
    _record("fwd_" + case.kernel, case.name, worst)
    assert foreign == 0, f"{case.name}: {foreign} guard elements of the output changed"
    assert (_bits(src, case.sdt) == inp["src_bits"]).all(), f"{case.name}: the source changed"
    bad = np.argwhere(use > 1)
    assert not bad.size, (f"{case.name}: {len(bad)} elements beyond the bound, first (b, column) = {tuple(bad[0])}: use "
                          f"{use[tuple(bad[0])]}, columns {sorted(set(bad[:, 1].tolist()))[:12]}")
    diff = np.argwhere(~same)
    assert not diff.size, (f"{case.name}: {len(diff)} elements differ from the fp32 sum in key order, first (b, column) = "
                           f"{tuple(diff[0])}, columns {sorted(set(diff[:, 1].tolist()))[:12]}")
    again = _alloc(inp["out0"], case.ddt)
    _run_pooled(case, inp, src, again)
    assert (_bits(again, case.ddt) == got).all(), f"{case.name}: two runs differ"


# ------------------------------------------------------------------------------------------------ sequence gather
@pytest.mark.parametrize("case", SEQ_CASES, ids=lambda c: c.name)
def test_sequence_gather_bit_for_bit(case):
    import dynamicemb_extensions as e
    from mi355_native import check, dt, lib, ptr, stream
    inp = fc.make_seq_inputs(case)
    want = fc.seq_emulate(case, inp)            # oracle.gather_sequence on the rows the op owns, the sentinel elsewhere
    D, st, dst = case.D, case.stride, case.D + case.dst_pad
    src = _alloc(inp["src_bits"], case.sdt)
    src_in = src[GUARD:-GUARD].view(-1, st)
    index = _i64(inp["index"]) if inp["index"] is not None else None
    n_dev = _i64([inp["n_eff"]]) if case.n_dev else None

    def run():
        out = _alloc(inp["out0"], case.ddt)
        out_in = out[GUARD:-GUARD].view(fc.SEQ_N + 1, dst)
        al = fc._aligned(D, st, dst) and src_in.data_ptr() % 16 == 0 and out_in.data_ptr() % 16 == 0
        assert al == case.aligned
        if case.src == "dense" and index is not None and n_dev is None:
            e.gather_embedding(src_in[:, :D], out_in[:fc.SEQ_N, :D], index)
        else:
            addr = _i64(_addresses(src_in, inp["slots"], st, case.sdt)) if case.src == "addr" else None
            check(lib().mi355_gather_rows(ptr(src_in) if addr is None else None, st if addr is None else 0, ptr(addr),
                                          dt(_TD[case.sdt]), ptr(index), fc.SEQ_N, ptr(n_dev), D, ptr(out_in), dst, dt(out_in),
                                          int(al), stream()), "gather_rows")
        torch.cuda.synchronize()
        return _bits(out, case.ddt)

    got = run()
    body = (got != want)[GUARD:-GUARD].reshape(fc.SEQ_N + 1, dst)
    assert not body[:inp["n_eff"], :D].any(), f"{case.name}: rows {sorted(set(np.argwhere(body[:, :D])[:, 0].tolist()))[:12]} differ"
    assert (got == want).all(), f"{case.name}: {(got != want).sum()} elements the op does not own changed (guards, pad, rows past n)"
    assert (_bits(src, case.sdt) == inp["src_bits"]).all(), f"{case.name}: the source changed"
    assert (run() == got).all(), f"{case.name}: two runs differ"


# ------------------------------------------------------------------------------------------------ flat-table copy
@pytest.mark.parametrize("case", FLAT_CASES, ids=lambda c: c.name)
def test_flat_table_copy_bit_for_bit(case):
    import dynamicemb_extensions as e
    from mi355_native import check, dt, lib, ptr, stream
    inp = fc.make_flat_inputs(case)
    want_t, want_d = fc.flat_copy_reference(case, inp)
    d = case.dtype
    tabs = [_alloc(fc.guarded(t, d), d) for t in inp["tables"]]
    dense = _alloc(fc.guarded(inp["dense"], d), d)
    dense_in = dense[GUARD:-GUARD].view(fc.FLAT_N, case.dense_dim + fc.FLAT_PAD)[:, :case.dense_dim]
    tptr = _i64([t[GUARD:].data_ptr() for t in tabs])
    tv, te = _i64([v for v, _, _ in fc.FLAT_TABLES]), _i64([x for _, x, _ in fc.FLAT_TABLES])
    idx, tid = _i64(inp["idx"]), _i64(inp["tid"])
    M = fc.FLAT_MAX_EMB
    if case.region == 0:
        f = e.load_from_flat_table_contiguous if case.load else e.store_to_flat_table_contiguous
        f(tptr, idx, case.table, dense_in, tv, te, M, False)
    elif case.region == 2:
        f = e.load_from_flat_table_value if case.load else e.store_to_flat_table_value
        f(tptr, idx, tid, dense_in, tv, te, M, False)
    elif case.load:
        e.load_from_flat_table_emb(tptr, idx, tid, dense_in, tv, te, M, False)
    else:                                                     # (no wrapper stores region 1)
        check(lib().mi355_flat_table_copy(0, 1, fc.FLAT_N, None, ptr(dense_in), case.dense_dim, dense_in.stride(0), dt(dense_in),
                                          ptr(idx), ptr(tid), 0, ptr(tptr), ptr(tv), ptr(te), M, stream()), "flat_table_copy")
    torch.cuda.synchronize()
    assert (_bits(dense, d) == fc.guarded(want_d, d)).all(), f"{case.name}: dense buffer"
    for t in range(2):
        assert (_bits(tabs[t], d) == fc.guarded(want_t[t], d)).all(), f"{case.name}: table {t}"
    changed = (want_d != inp["dense"]).any() if case.load else any((want_t[t] != inp["tables"][t]).any() for t in range(2))
    assert changed                                            # (the reference itself moved something)


# ------------------------------------------------------------------------------------------------ row addresses
@pytest.mark.parametrize("elem_bytes", [4, 2])
@pytest.mark.parametrize("with_ids,with_n_dev", [(False, False), (True, False), (True, True), (False, True)])
def test_row_addresses_exact(elem_bytes, with_ids, with_n_dev):
    import dynamicemb_extensions as e
    from mi355_native import check, lib, ptr, stream
    rng = np.random.default_rng(elem_bytes + 2 * with_ids + 4 * with_n_dev)
    n, n_eff = 700, 533                                       # three blocks, the count ends inside the third
    ptrs = np.array([0x7F0000001000, 0x7F1000002000], np.int64)   # (addresses are only computed, never followed)
    vdims = np.array([24, 10], np.int64)
    slots = rng.integers(-1, 5000, n).astype(np.int64)
    slots[[0, 255, 256, n_eff - 1, n - 1]] = -1
    tid = rng.integers(0, 2, n).astype(np.int64) if with_ids else np.zeros(n, np.int64)
    want = np.where(slots < 0, 0, ptrs[tid] + slots * vdims[tid] * elem_bytes)
    if not with_n_dev:
        got = e.row_addresses(_i64(slots), _i64(tid) if with_ids else None, _i64(ptrs), _i64(vdims), elem_bytes).cpu().numpy()
        assert (got == want).all()
        return
    got = e.row_addresses(_i64(slots), _i64(tid) if with_ids else None, _i64(ptrs), _i64(vdims), elem_bytes, _i64([n_eff]))
    assert (got.cpu().numpy()[:n_eff] == want[:n_eff]).all()
    out = torch.full((n + 2,), -77, dtype=torch.int64, device=DEV)       # the rows past n_dev: through the C ABI, into a guarded buffer
    a_n, a_s, a_t, a_p, a_v = _i64([n_eff]), _i64(slots), _i64(tid), _i64(ptrs), _i64(vdims)
    check(lib().mi355_row_addresses(n, ptr(a_n), ptr(a_s), ptr(a_t) if with_ids else None, ptr(a_p), ptr(a_v), elem_bytes,
                                    ptr(out[1:]), stream()), "row_addresses")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[1:n_eff + 1] == want[:n_eff]).all() and (got[n_eff + 1:] == -77).all() and got[0] == -77


# ------------------------------------------------------------------------------------------------ sum_chunks
@pytest.mark.parametrize("n", [4, 1028])
@pytest.mark.parametrize("chunks", [1, 2, 5])
def test_sum_chunks_family_bit_for_bit(n, chunks):
    """mi355_sum_chunks (fp32 chunks), _typed (chunks in a wire dtype) and _self (one chunk read in place, every
    self_index): the fp32 sum in chunk order 0 .. W - 1, one rounding, for every dtype pair"""
    from mi355_native import check, dt, lib, ptr, stream
    rng = np.random.default_rng(n + chunks)
    for s in fc.DTYPES:
        x = orc.round_to(rng.standard_normal((chunks, n)).astype(np.float32), s)
        acc = np.zeros(n, np.float32)
        for c in range(chunks):
            acc = acc + x[c]
        xin = _alloc(fc.guarded(fc.to_bits(x, s), s), s)
        x_in = xin[GUARD:-GUARD]
        for d in fc.DTYPES:
            want = fc.guarded(fc.to_bits(orc.round_to(acc, d), d), d)
            out0 = fc.guarded(np.full(n, fc.SENTINEL[d], fc.BITS[d]), d)
            calls = [("typed", lambda o: lib().mi355_sum_chunks_typed(ptr(x_in), dt(x_in), chunks, n, ptr(o), dt(o), stream()))]
            if s == "f32":
                calls.append(("f32", lambda o: lib().mi355_sum_chunks(ptr(x_in), chunks, n, ptr(o), dt(o), stream())))
            for si in range(chunks):                          # the self chunk lives elsewhere; its place in `in` holds poison
                poisoned = x.copy()
                poisoned[si] = 1e30
                pin = _alloc(fc.to_bits(orc.round_to(poisoned, s), s), s)
                own = _alloc(fc.guarded(fc.to_bits(x[si], s), s), s)
                calls.append((f"self{si}", lambda o, pin=pin, own=own, si=si: lib().mi355_sum_chunks_self(
                    ptr(pin), dt(pin), chunks, n, ptr(own[GUARD:-GUARD]), si, ptr(o), dt(o), stream())))
            for what, call in calls:
                out = _alloc(out0, d)
                check(call(out[GUARD:-GUARD]), "sum_chunks")
                torch.cuda.synchronize()
                assert (_bits(out, d) == want).all(), f"sum_chunks {what} n={n} chunks={chunks} {s}->{d}"
        assert (_bits(xin, s) == fc.guarded(fc.to_bits(x, s), s)).all()


# ------------------------------------------------------------------------------------------------ one-kernel eval forward
# gather_pooled_eval_kernel / gather_rows_eval_kernel (gather_dev.h, fused_fwd.hip).  A lane group owns KIT = 4 consecutive
# bags = one run of keys; lane c probes key c of the run (rp0), keys past the run's first LPR are probed when their bag is
# reached.  `in_first` = run_lo + LPR - lo is what a bag takes from rp0.  Every aligned group of four bags below puts the
# LPR boundary of its run before a bag, on a bag's first key, inside a bag, on its last key or behind it.
_EVAL_PAIRS = (("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16"))
_EVAL_B = 107                                    # bags per feature: not a multiple of KIT, so runs cross table boundaries
_EVAL_KNOWN = 300                                # preloaded keys per table (the SAME keys in every table, different rows)


def _eval_groups(lpr):
    return [(lpr - 1, 3, 2, 1),                  # bag 1: in_first = 1 (the boundary behind its first key); bag 2, 3: before
            (lpr, 3, 0, 2),                      # bag 1: in_first = 0 (the boundary on its first key)
            (lpr - 3, 6, 1, 0),                  # bag 1: 3 of 6 keys (inside)
            (lpr - 4, 5, 2, 2),                  # bag 1: in_first = L - 1 (on its last key)
            (lpr - 5, 5, 3, 1),                  # bag 1: in_first = L (behind its last key); bag 2 starts on the boundary
            (2, 3, 1, 2),                        # everything inside the first LPR keys
            (2 * lpr + 3, 1, 0, 2),              # a bag longer than 2 LPR at the head of a run
            (1, 2 * lpr + 1, 2, 0),              # ... and inside a run
            (0, 0, 0, 0)]                        # a run without keys between runs with keys


def _eval_lengths(lpr, F, rng):
    """[F * _EVAL_B] bag lengths: per feature the groups above, aligned to global bag numbers that are multiples of 4
    (bags of one key in front), short random bags, and four empty bags at the end"""
    pat = np.array(_eval_groups(lpr)).ravel()
    lens = []
    for f in range(F):
        lead = -(f * _EVAL_B) % 4
        fill = rng.integers(0, 4, _EVAL_B - lead - pat.size - 4)
        lens.append(np.concatenate([np.ones(lead, np.int64), pat, fill, np.zeros(4, np.int64)]))
    return np.concatenate(lens).astype(np.int64)


def _in_first_classes(off, lpr):
    """which positions of the LPR boundary the batch holds (per non-empty bag)"""
    FBn = off.size - 1
    seen = set()
    for bag in range(FBn):
        lo, L = int(off[bag]), int(off[bag + 1] - off[bag])
        if L == 0:
            continue
        i = int(off[bag - bag % 4]) + lpr - lo
        seen.add("before" if i < 0 else "on_first" if i == 0 else "behind_first" if i == 1 and L > 1 else
                 "on_last" if i == L - 1 else "behind_last" if i == L else "after" if i > L else "inside")
        if L > 2 * lpr:
            seen.add("long")
    return seen


def _eval_cases():
    c, k = [], 0
    for T in (1, 3):
        for pooling in ("SUM", "MEAN", "NONE"):
            for D in (8, 64, 256):                            # the pairs in rotation: SUM and MEAN together see all four
                c.append((T, pooling, D) + _EVAL_PAIRS[k % 4])
                k += 1
        left = set(_EVAL_PAIRS) - {x[3:] for x in c if x[0] == T and x[1] == "NONE"}
        c += [(T, "NONE", 64) + p for p in sorted(left)]      # the pair the three sequence cases leave out
    return c


_EVAL_CASES = _eval_cases()
for _T in (1, 3):       # every instantiation: {pooled, rows} x {one table, several} x the four dtype pairs
    for _seq in (False, True):
        assert {(s, d) for T, p, D, s, d in _EVAL_CASES if T == _T and (p == "NONE") == _seq} == set(_EVAL_PAIRS), (_T, _seq)


@pytest.mark.parametrize("T,pooling,D,edt,odt", _EVAL_CASES, ids=lambda v: str(v))
def test_one_kernel_eval_forward_at_designed_bags(T, pooling, D, edt, odt):
    from dynamicemb.batched_dynamicemb_tables import BatchedDynamicEmbeddingTablesV2 as B2
    from dynamicemb.dynamicemb_config import (DynamicEmbInitializerArgs as IA, DynamicEmbInitializerMode as IM,
                                              DynamicEmbPoolingMode as PM, DynamicEmbScoreStrategy as SS,
                                              DynamicEmbTableOptions as TO, EmbOptimType as OT)
    import dynamicemb_extensions as e
    name = f"eval_T{T}_{pooling}_D{D}_{edt}_{odt}"
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lpr = 1 << fc.lpr_log2_for(D)
    opts = [TO(dim=D, max_capacity=1024, index_type=torch.int64, embedding_dtype=_TD[edt], bucket_capacity=128,
               initializer_args=IA(mode=IM.CONSTANT, value=0.25), score_strategy=SS.STEP) for _ in range(T)]
    m = B2(table_options=opts, feature_table_map=list(range(T)), pooling_mode=getattr(PM, pooling), optimizer=OT.SGD,
           output_dtype=_TD[odt], learning_rate=0.05, device=torch.device(DEV))
    twin = VecEmbeddingTwin([D] * T, list(range(T)), pooling, "sgd")
    known = (1 << 33) + 7 * np.arange(_EVAL_KNOWN, dtype=np.int64)
    for t in range(T):
        rows = orc.round_to(rng.standard_normal((_EVAL_KNOWN, D)).astype(np.float32), edt)
        V = m.value_dims[t]
        full = np.concatenate([rows, np.zeros((_EVAL_KNOWN, V - D), np.float32)], 1)
        m._insert_rows(t, torch.from_numpy(known).to(DEV), torch.from_numpy(full).to(DEV).to(_TD[edt]),   # (exact: rounded above)
                       torch.zeros(_EVAL_KNOWN, dtype=torch.int64, device=DEV))
        twin.load(t, known, rows, 0)
    lens = _eval_lengths(lpr, T, rng)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    keys = np.where(rng.random(n) < 0.75, known[rng.integers(0, _EVAL_KNOWN, n)], (1 << 45) + rng.integers(0, 1 << 30, n))
    want_pos = {"before", "on_first", "behind_first", "inside", "on_last", "behind_last", "after", "long"}
    assert _in_first_classes(off, lpr) >= want_pos, sorted(want_pos - _in_first_classes(off, lpr))
    assert off[-5] == off[-1] == n                            # trailing empty bags
    # what selects the one-kernel branch of mi355_demb_forward_fused (`!train && n > 0 && ...`, fused_fwd.hip)
    m.eval()
    fp, _, _, use_count = m._fused_scores()
    P = e.ScorePolicy
    tb = m.table
    assert m._fused and not m.training and n > 0 and 1 <= m.num_tables <= 128
    assert all(d % 4 == 0 for d in m.dims) and all(v % 4 == 0 for v in m.value_dims)          # aligned16
    assert not use_count and fp in (P.CONST, P.ASSIGN, P.GLOBAL_TIMER)
    assert tb.bucket_capacity_ & (tb.bucket_capacity_ - 1) == 0 and tb.num_buckets_ < (1 << 31)
    assert m.embedding_dtype in (torch.float32, torch.bfloat16) and m.output_dtype in (torch.float32, torch.bfloat16)
    assert pooling == "NONE" or n <= 8 * (off.size - 1)
    assert m.max_D <= 4 << fc.lpr_log2_for(m.max_D)           # rows of one column group
    size0 = int(m.size())
    with torch.no_grad():
        out = m(torch.from_numpy(keys).to(DEV), torch.from_numpy(off).to(DEV))
        out2 = m(torch.from_numpy(keys).to(DEV), torch.from_numpy(off).to(DEV))
    torch.cuda.synchronize()
    x = twin.forward(keys, off, False)
    got = out.double().cpu().numpy()
    assert got.shape == x.shape
    u = bound_use(got, x, forward_bound(x, twin.abs_sum, twin.nterms, odt, pooling == "MEAN"))
    print(f"forward_variants_use {'eval_' + ('rows' if pooling == 'NONE' else 'pooled') + ('_mt' if T > 1 else '') + f'_lpr{lpr}':26s} "
          f"s={edt:4s} d={odt:4s} {pooling.lower():4s} {u.max():.4f}  ({name})")
    _record("fwd_eval", name, u.max())
    bad = np.argwhere(u > 1)
    assert not bad.size, f"{name}: {len(bad)} elements beyond the bound, rows {sorted(set(bad[:, 0].tolist()))[:12]}"
    zero = np.broadcast_to(twin.abs_sum == 0, got.shape)     # unknown keys only, empty bags: exactly zero
    assert zero.any() and (got[zero] == 0).all(), f"{name}: the output of unknown keys is not zero"
    assert torch.equal(out, out2), f"{name}: two runs differ"
    assert int(m.size()) == size0, f"{name}: the eval forward inserted keys"
