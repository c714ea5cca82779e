"""The vectorised twin (oracle/vec_twin.py) on the CPU: (i) it computes what the per-key dict twin computes, over several
training steps, for every pooling, every optimizer, several tables of mixed dims; (ii) the element-wise bounds the GPU
tests of the partitioned index path use (tests/test_path_c_oracle_gpu.py) accept a simulated product -- fp32 sums in a
shuffled order, one rounding to the gradient / output dtype -- and REJECT it when one planted error is in it: a lost
occurrence of a hot key, a bag's gradient applied twice, a reduced gradient rounded twice or not at all, a MEAN divided by
the wrong length, one column of one row read from the neighbouring row; (iii) its cost at the size of the C2 batch."""
import time

import numpy as np
import pytest

from oracle import oracle as orc
from oracle.dict_twin import DictEmbeddingTwin
from oracle.vec_twin import (VecEmbeddingTwin, bound_use, debug_rows, forward_bound, interval_use, update_rows)

OPTS = ["sgd", "adam", "adagrad", "rowwise_adagrad"]


def _batch(rng, F, B, hi, maxlen=6):
    lens = rng.integers(0, maxlen, F * B)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rng.integers(0, hi, int(off[-1])).astype(np.int64), off


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("pooling", ["SUM", "MEAN", "NONE"])
def test_vec_twin_matches_the_dict_twin(pooling, opt):
    dims, fmap = ([8, 8], [0, 1, 1]) if pooling == "NONE" else ([8, 16, 4], [0, 1, 1, 2])
    F, B, hi, lr = len(fmap), 24, 300, 0.05
    a = DictEmbeddingTwin(dims, fmap, pooling, opt, lr=lr)
    b = VecEmbeddingTwin(dims, fmap, pooling, opt, lr=lr, init=debug_rows)
    rng = np.random.default_rng(11)
    occ, seen = [dict() for _ in dims], [dict() for _ in dims]
    for step in range(6):
        keys, off = _batch(rng, F, B, hi)
        tab = np.asarray(fmap)[np.repeat(np.arange(F * B) // B, np.diff(off))]
        for k_, t_ in zip(keys.tolist(), tab.tolist()):
            occ[t_][k_] = occ[t_].get(k_, 0) + 1
            seen[t_][k_] = step
        ra, rb = a.forward(keys, off, True), b.forward(keys, off, True)
        np.testing.assert_allclose(rb, ra, rtol=1e-12, atol=0, err_msg=f"step {step}: forward")
        g = rng.uniform(-1.0, 1.2, size=ra.shape).astype(np.float32)
        a.backward(g)
        b.backward(g)
        for t in range(len(dims)):
            assert b.keys[t].tolist() == sorted(a.tables[t])
            want = np.stack([a.tables[t][int(k)] for k in b.keys[t]])
            # (Adam: the dict twin forms 1 - beta^t in fp32 from the fp64 power, the vectorised one exactly from the fp32
            # beta, as the product does: a few ulps of the step.)  Carried from the dict twin, so outputs stay exact.
            np.testing.assert_allclose(b.rows[t], want, rtol=4e-6, atol=1e-6, err_msg=f"step {step}: rows")
            b.set_rows(t, b.keys[t], want)
        if step % 2 == 1:        # eval: unknown keys read zeros and are not inserted
            ek, eo = _batch(rng, F, 5, 2 * hi)
            np.testing.assert_allclose(b.forward(ek, eo, False), a.forward(ek, eo, False), rtol=1e-12, atol=0)
    assert b.step == 6 and b.iter == 6
    for t in range(len(dims)):      # scores: occurrences over the training forwards / the last forward that touched a key
        k, lfu, last = b.scores(t)
        assert lfu.tolist() == [occ[t][int(x)] for x in k] and last.tolist() == [seen[t][int(x)] for x in k]


# ----------------------------------------------------------------------------------------------- planted errors
D, LR = 16, 0.05
HOT = 77


def _hot_batch(rng, B=300):
    """one table, one feature: bags of 0-9 keys over 2 000 keys, plus key HOT in ~200 bags (a hot row on every path)"""
    lens = rng.integers(0, 10, B)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = rng.integers(0, 2000, int(off[-1])).astype(np.int64)
    keys[rng.random(keys.size) < 0.15] = HOT
    return keys, off


def _sim_forward(rows_of, keys, off, pooling, out_dtype, rng, plant=None):
    """the product's forward: fp32 sum over each bag in a shuffled order, MEAN times fp32(1 / L), one rounding"""
    B = off.size - 1
    out = np.zeros((B, D), np.float32)
    R = rows_of(keys)
    bad_bag = int(np.nonzero(np.diff(off) >= 2)[0][3])
    for b in range(B):
        lo, hi = int(off[b]), int(off[b + 1])
        if hi == lo:
            continue
        r = R[lo:hi].copy()
        if plant == "neighbour" and b == bad_bag:
            r[0, 5] = rows_of(keys[lo:lo + 1] + 1)[0, 5]           # one column of one row read from the next key's row
        acc = np.add.accumulate(r[rng.permutation(hi - lo)], axis=0, dtype=np.float32)[-1]
        if pooling == "MEAN":
            L = hi - lo + (1 if plant == "mean_len" and b == bad_bag else 0)
            acc = acc * (np.float32(1) / np.float32(L))
        out[b] = acc
    return orc.round_to(out, out_dtype)


def _sim_reduce(keys, off, grads, pooling, gdt, rng, plant=None):
    """the product's reduced gradients: per unique key an fp32 sum of its terms in a shuffled order, rounded once"""
    lens = np.diff(off)
    bag = np.repeat(np.arange(off.size - 1), lens)
    g = grads.astype(np.float32)
    if pooling == "MEAN":
        L = lens.astype(np.float32)
        if plant == "mean_len":
            L[int(np.nonzero(lens >= 2)[0][3])] += 1
        g = g * (np.float32(1) / np.maximum(L, 1))[:, None]
    terms = g[bag]
    kk = keys
    if plant == "drop":                         # one occurrence of the hot key lost
        j = int(np.nonzero(keys == HOT)[0][7])
        terms, kk = np.delete(terms, j, axis=0), np.delete(keys, j)
    if plant == "twice":                        # one bag's gradient applied twice
        b = int(np.nonzero(lens >= 3)[0][0])
        sl = slice(int(off[b]), int(off[b + 1]))
        terms, kk = np.concatenate([terms, terms[sl]]), np.concatenate([kk, keys[sl]])
    uk = np.unique(keys)
    out = np.zeros((uk.size, D), np.float32)
    for i, k in enumerate(uk):
        x = terms[kk == k]
        x = x[rng.permutation(len(x))]
        if plant == "round_twice" and len(x) >= 2:      # partial sums rounded before they are combined, and again after
            h = len(x) // 2
            p = [orc.round_to(np.add.accumulate(y, axis=0, dtype=np.float32)[-1][None], gdt)[0] for y in (x[:h], x[h:])]
            out[i] = p[0] + p[1]
        else:
            out[i] = np.add.accumulate(x, axis=0, dtype=np.float32)[-1]
    return uk, out if plant == "round_never" else orc.round_to(out, gdt)


def _run(opt, pooling, gdt, plant, out_dtype="f32", seed=5):
    """two training steps of the twin; the simulated product of the SECOND step (optimizer state carried) -> worst use
    of the forward bound and of the row bracket"""
    rng = np.random.default_rng(seed)
    twin = VecEmbeddingTwin([D], [0], pooling, opt, lr=LR, init=lambda k, d: rng.standard_normal((len(k), d)).astype(np.float32),
                            grad_dtype=gdt)
    for step in range(2):
        keys, off = _hot_batch(rng)
        x = twin.forward(keys, off, True)
        last = step == 1
        out = _sim_forward(lambda k: twin.get_rows(0, k)[1][:, :D], keys, off, pooling, out_dtype, rng, plant if last else None)
        f_use = bound_use(out, x, forward_bound(x, twin.abs_sum, twin.nterms, out_dtype, pooling == "MEAN")).max()
        g = orc.round_to(rng.uniform(-0.6, 1.0, x.shape).astype(np.float32), gdt)
        twin.backward(g)
        uk, red = _sim_reduce(keys, off, g, pooling, gdt, rng, plant if last else None)
        prod = update_rows(opt, twin.last_grad[0]["rows_before"], red, D, twin.hp, twin.iter)
        k2, lo, hi, slack = twin.row_bracket(0)
        assert np.array_equal(k2, uk)
        r_use = interval_use(prod, lo, hi, slack).max()
        if not last:
            assert f_use <= 1 and r_use <= 1
            twin.set_rows(0, uk, prod)              # carry the product's rows, as the GPU tests do
    return f_use, r_use


@pytest.mark.parametrize("gdt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("pooling", ["SUM", "MEAN"])
@pytest.mark.parametrize("opt", OPTS)
def test_bounds_accept_the_unmodified_product(opt, pooling, gdt):
    for out_dtype in ("f32", "bf16"):
        f_use, r_use = _run(opt, pooling, gdt, None, out_dtype)
        assert f_use <= 1 and r_use <= 1, (f_use, r_use)


@pytest.mark.parametrize("plant,opt,pooling,gdt,where", [
    ("drop", "sgd", "SUM", "f32", "rows"),
    ("drop", "adam", "SUM", "bf16", "rows"),
    ("twice", "sgd", "SUM", "bf16", "rows"),
    ("twice", "rowwise_adagrad", "MEAN", "f32", "rows"),
    ("round_twice", "adam", "SUM", "bf16", "rows"),
    ("round_twice", "sgd", "SUM", "f16", "rows"),
    ("round_never", "sgd", "SUM", "bf16", "rows"),
    ("round_never", "adagrad", "MEAN", "bf16", "rows"),
    ("mean_len", "sgd", "MEAN", "f32", "rows"),
    ("mean_len", "adam", "MEAN", "f32", "forward"),
    ("neighbour", "sgd", "SUM", "f32", "forward"),
    ("neighbour", "sgd", "MEAN", "bf16", "forward"),
])
def test_bounds_reject_a_planted_error(plant, opt, pooling, gdt, where):
    out_dtype = "bf16" if gdt == "bf16" else "f32"
    clean = _run(opt, pooling, gdt, None, out_dtype)
    assert max(clean) <= 1, clean
    f_use, r_use = _run(opt, pooling, gdt, plant, out_dtype)
    use = r_use if where == "rows" else f_use
    print(f"planted {plant:12s} {opt:16s} {pooling} {gdt}: worst {where} use {use:.3g} (clean {max(clean):.3g})")
    assert use > 1, f"the {where} bound did not reject the planted error ({use})"


def test_c2_scale_runtime():
    """one training step at the C2 batch (65 536 bags of 1-10 keys, Zipf 0.99 over 10 M rows -- ~360 K keys), D = 128:
    forward, backward and the row bracket must stay a few seconds"""
    rng = np.random.default_rng(0)
    B, rows = 65536, 10_000_000
    lens = rng.integers(1, 11, B)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    w = np.arange(1, rows + 1, dtype=np.float64) ** -0.99
    cdf = np.cumsum(w)
    keys = np.searchsorted(cdf / cdf[-1], rng.random(int(off[-1]))).astype(np.int64)
    twin = VecEmbeddingTwin([128], [0], "SUM", "adam", lr=0.01, init=lambda k, d: np.full((len(k), d), 0.5, np.float32),
                            grad_dtype="bf16")
    t0 = time.perf_counter()
    x = twin.forward(keys, off, True)
    fb = forward_bound(x, twin.abs_sum, twin.nterms, "bf16")
    twin.backward(orc.round_to(rng.uniform(-1, 1, x.shape).astype(np.float32), "bf16"))
    twin.row_bracket(0)
    dt = time.perf_counter() - t0
    print(f"vec twin, C2 batch ({keys.size} keys, {twin.keys[0].size} unique, D = 128, Adam): one step {dt:.2f} s")
    assert fb.shape == x.shape and dt < 60
