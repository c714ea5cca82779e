"""The partition kernel's head-key work (fused_part3_kernel, csrc/fused_fwd.hip): records whose key occurs more than 8 times in
a tile are expanded into CSR entries by groups of 16 lanes, up to kBigMax = 512 such records per partition (more: the record's
own thread expands it), and chunked hot rows are registered by a wave.

Two batches on path (c) (every step asserts `st.lazy`):
  * head: 256 tiles of 1 408 keys; ONE key takes 30 % of every tile (422 occurrences per tile: lists of several hundred entries),
    and four keys that the table's hash puts into ONE slot-range partition occur 9 times in every tile -- 1 024 long records in that
    partition, so the fallback beyond kBigMax runs.  The test counts the long records per partition from the step's own outputs and
    FAILS if no partition exceeded kBigMax;
  * c2: a plain C2-shaped Zipf-0.99 batch on a 1 M-row table.
Each is compared (a) with oracle/vec_twin.py through the per-element bounds of tests/test_path_c_oracle_gpu.py (its `_run`:
forward_bound for outputs, row_bracket for the rows after one SGD step), and (b) with the per-op chain (MI355_FUSED=0): the same
number of unique rows, the same unique keys, and -- exactly -- the same CSR: row pointers by key and, per key, the bag of every
entry (entries < 0 resolved through tile_bags); the per-op chain's output and rows go through the same twin bounds."""
import numpy as np
import pytest
import torch

from oracle.vec_twin import VecEmbeddingTwin, bound_use, forward_bound, interval_use
from test_fused_fwd_gpu import _mk
from test_path_c_oracle_gpu import _run, _setup, _warm_rows, _zipf_keys, _lens

pytestmark = pytest.mark.gpu
DEV = "cuda"
TL, TILES, KBIGMAX = 1408, 256, 512
CAP = 1 << 20


def _al256(x):
    return (x + 255) // 256 * 256


def _partition_of(keys, S, C, spp):
    """slot-range partition of a key: the bucket of its hash (test_path_c_oracle_gpu.py, the flooded-partition case)"""
    h = keys.astype(np.uint64)
    h ^= h >> np.uint64(33); h *= np.uint64(0xFF51AFD7ED558CCD)
    h ^= h >> np.uint64(33); h *= np.uint64(0xC4CEB9FE1A85EC53)
    h ^= h >> np.uint64(33)
    h &= np.uint64(0x7FFFFFFFFFFFFFFF)
    return ((h % np.uint64(S)) // np.uint64(C) * np.uint64(C) // np.uint64(spp)).astype(np.int64)


def _geometry(m, n):
    from mi355_native import lib
    P = int(lib().mi355_demb_forward_fused_partitions(n, m.num_tables, m.table.num_buckets_))
    assert P == TILES
    S, C = m.table.capacity_, m.table.bucket_capacity_
    return P, S, C, -(-((S + 1 + P - 1) // P) // C) * C


def _head_batch(rng, S, C, spp):
    """[TILES * TL] keys: per tile 422 x the head key, 9 x each of four keys of ONE partition, 9..12 x each of 30 other keys,
    the rest drawn from 200 K cold keys; shuffled inside the tile.  Bags of 8."""
    cand = np.arange(1 << 30, (1 << 30) + 400_000, dtype=np.int64)
    part = _partition_of(cand, S, C, spp)
    same = cand[part == 7][:4]
    assert same.size == 4
    head, warm = cand[-1], cand[1000:1030]
    cold = (1 << 32) + np.arange(200_000, dtype=np.int64)
    tiles = []
    for t in range(TILES):
        ks = [np.full(422, head), np.repeat(same, 9), np.repeat(warm, rng.integers(9, 13, warm.size))]
        fill = TL - sum(k.size for k in ks)
        ks.append(cold[rng.integers(0, cold.size, fill)])
        tiles.append(rng.permutation(np.concatenate(ks)))
    keys = np.concatenate(tiles)
    assert keys.size == TILES * TL
    return keys, np.arange(0, keys.size + 1, 8, dtype=np.int64)


def _c2_batch(rng):
    off = _lens(rng, 65536, 1, 10)
    return _zipf_keys(rng, int(off[-1]), 0.99, 1_000_000, 1 << 41), off


def _csr_by_key(st, keys, off, pathc):
    """(unique keys sorted, their counts, (key, bag) of every CSR entry sorted) from a step's own arrays: row pointers and CSR at
    the head of its backward workspace, entries < 0 resolved through tile_bags; keys of the unique rows through the reverse indices"""
    n = keys.numel()
    nu = int(st.uoff[-1])
    rev = st.rev[:n]
    uk = torch.empty(nu, dtype=torch.int64, device=DEV)
    uk[rev] = keys
    assert torch.equal(uk[rev], keys) and int(torch.unique(rev).numel()) == nu
    uk = uk.cpu().numpy()
    bags = np.repeat(np.arange(off.numel() - 1), np.diff(off.cpu().numpy()))
    if not pathc:      # per-op chain: the grouping is the reverse index itself
        ent_key, ent_bag = keys.cpu().numpy(), bags
        cnt = np.bincount(rev.cpu().numpy(), minlength=nu)
    else:
        o = st.off["bwd_ws"]
        ws = st.buf[o: o + _al256(4 * (n + 1)) + 2 * _al256(4 * n) + 4 * n].view(torch.int32).cpu().numpy()
        ptr = ws[: nu + 1].astype(np.int64)
        csr = ws[_al256(4 * (n + 1)) // 4:][:n].astype(np.int64)
        tb = ws[(_al256(4 * (n + 1)) + _al256(4 * n)) // 4:][:n]
        assert ptr[0] == 0 and ptr[-1] == n and (np.diff(ptr) > 0).all()
        cnt = np.diff(ptr)
        assert np.array_equal(cnt, st.csr_cnt[:nu].cpu().numpy())
        ref = csr < 0
        assert ((~csr[ref]) < n).all() and (csr[~ref] < off.numel() - 1).all()
        ent_bag = np.where(ref, tb[np.where(ref, ~csr, 0)], csr)
        ent_key = np.repeat(uk, cnt)
    ou = np.argsort(uk)
    oe = np.lexsort((ent_bag, ent_key))
    return uk[ou], cnt[ou], ent_key[oe], ent_bag[oe]


def _long_records_per_partition(st, n, spp, P):
    """records (tile, unique row) with more than 8 occurrences, per partition, from the step's reverse indices and slots"""
    nu = int(st.uoff[-1])
    rev = st.rev[:n].cpu().numpy()
    part_u = (st.slots[:nu].cpu().numpy() // spp).astype(np.int64)
    tl = min(max((-(-n // TILES) + 63) // 64 * 64, 256), 2048 if n > TILES * 1024 else 1024)      # the probe kernel's tile length
    pair, pc = np.unique((np.arange(n) // tl) * nu + rev, return_counts=True)
    return np.bincount(part_u[pair % nu], weights=pc > 8, minlength=P).astype(np.int64), int(pc.max())


@pytest.mark.parametrize("case", ["head", "c2"])
def test_partition_kernel_head_keys_against_the_twin_and_the_per_op_chain(case, monkeypatch):
    assert torch.cuda.get_device_properties(0).multi_processor_count == TILES, "the tile length below assumes 256 CUs"
    rng = np.random.default_rng(11 if case == "head" else 12)
    lr, D = 0.05, 32
    monkeypatch.setenv("MI355_FUSED", "1")
    probe = _mk(True, (D,), cap=CAP, monkeypatch=monkeypatch)
    P, S, C, spp = _geometry(probe, TILES * TL)
    del probe
    keys, off = _head_batch(rng, S, C, spp) if case == "head" else _c2_batch(rng)
    n = keys.size
    u = np.unique(keys)
    warm = u[rng.random(u.size) < 0.5]
    # ---- (a) path (c) against the twin, per-element bounds (one SGD step)
    m, twin = _setup(case, np.random.default_rng(5), [D], [0], "SUM", "SGD", "f32", "f32", "TIMESTAMP", CAP, lr, warm=[warm])
    _run("part3_" + case, rng, m, twin, None, 0, "f32", "f32", "impl", True, extra_steps=[(keys, off)])
    # ---- (b) the same batch on a second fused module and on the per-op chain: integers exactly
    kt, ot = torch.from_numpy(keys).to(DEV), torch.from_numpy(off).to(DEV)
    rows = _warm_rows(np.random.default_rng(5), warm.size, D, "SGD")
    got = {}
    for fused in (True, False):
        mm = _mk(fused, (D,), cap=CAP, learning_rate=lr, monkeypatch=monkeypatch)
        mm.train()
        mm._insert_rows(0, torch.from_numpy(warm).to(DEV), torch.from_numpy(rows).to(DEV),
                        torch.zeros(warm.size, dtype=torch.int64, device=DEV))
        out, st = mm._forward_impl(kt, ot, train=True)
        assert bool(getattr(st, "lazy", False)) == fused, "path (c) not taken" if fused else "the per-op chain reports a lazy step"
        if fused:
            assert _geometry(mm, n)[3] == spp
            big, longest = _long_records_per_partition(st, n, spp, P)
            print(f"part3_head {case}: long records per partition max {big.max()} (kBigMax {KBIGMAX}), longest list {longest}")
            if case == "head":
                assert big.max() > KBIGMAX, f"no partition holds more than kBigMax long records ({big.max()}): the fallback did not run"
                assert longest >= 400
        got[fused] = _csr_by_key(st, kt, ot, fused) + (out.double().cpu().numpy(),)
        if not fused:
            # the per-op chain through the same bounds as `_run` applies to path (c): new keys are UNIFORM rows here, so the
            # reference twin reads them from the table
            def init(ks, d, _m=mm):
                f, r = _m.lookup_rows(torch.from_numpy(np.asarray(ks)).to(DEV), 0)
                assert bool(f.all())
                return r[:, :d].cpu().numpy()
            tw = VecEmbeddingTwin([D], [0], "SUM", "sgd", lr=lr, init=init, grad_dtype="f32")
            tw.load(0, warm, rows, 0)
            x = tw.forward(keys, off, True)
            fu = bound_use(got[False][4], x, forward_bound(x, tw.abs_sum, tw.nterms, "f32", False))
            assert (fu <= 1).all(), f"{case}: per-op forward beyond its bound"
            g = torch.from_numpy(rng.uniform(-0.5, 1.0, x.shape).astype(np.float32)).to(DEV)
            mm._backward_impl(st, g)
            tw.backward(g.double().cpu().numpy())
            uk2, lo, hi, slack = tw.row_bracket(0)
            f, r = mm.lookup_rows(torch.from_numpy(uk2).to(DEV), 0)
            assert bool(f.all())
            assert (interval_use(r.cpu().numpy(), lo, hi, slack) <= 1).all(), f"{case}: per-op rows outside the bracket"
    for i, what in enumerate(["unique keys", "row pointer differences by key", "CSR entry keys", "CSR entry bags"]):
        assert np.array_equal(got[True][i], got[False][i]), f"{case}: {what} differ between path (c) and the per-op chain"
