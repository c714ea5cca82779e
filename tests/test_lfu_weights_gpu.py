"""Per-key frequency weights (forward's per_sample_weights, prefetch's frequency_counters, prefetch_async's per_sample_weights).

The reference treats them as COUNTS (BatchedDynamicEmbeddingTablesV2.forward -> prefetch(..., frequency_counters), summed per
unique key by segmented_unique): an LFU score, LRU_LFU's frequency word and the admission counter grow by the sum of a key's
weights in the step instead of its occurrence count; outputs and gradients are never weighted.  Checked here on path (c) (the
partitioned index stage of the C2 step: probe_c_kernel + the partition kernel), path (b) (the per-slot-counter probe), the
staged prefetch and the one-call / per-op paths, against numpy accumulations of the weights."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mk(strategy="LFU", dims=(16,), fmap=None, pooling="SUM", opt="SGD", cap=1 << 16, bucket=128, **kw):
    from dynamicemb.batched_dynamicemb_tables import BatchedDynamicEmbeddingTablesV2 as B2
    from dynamicemb.dynamicemb_config import (DynamicEmbInitializerArgs as IA, DynamicEmbInitializerMode as IM,
                                              DynamicEmbPoolingMode as PM, DynamicEmbScoreStrategy as SS,
                                              DynamicEmbTableOptions as TO, EmbOptimType as OT)
    topt = {k: kw.pop(k) for k in ("admit_strategy", "admission_counter", "external_storage") if k in kw}
    opts = [TO(dim=d, max_capacity=cap, index_type=torch.int64, embedding_dtype=torch.float32, bucket_capacity=bucket,
               initializer_args=IA(mode=IM.UNIFORM, lower=-0.5, upper=0.5),
               score_strategy=tuple(getattr(SS, x) for x in strategy) if isinstance(strategy, tuple) else getattr(SS, strategy), **topt)
            for d in dims]
    m = B2(table_options=opts, feature_table_map=fmap or list(range(len(dims))), pooling_mode=getattr(PM, pooling),
           optimizer=getattr(OT, opt), learning_rate=0.1, output_dtype=torch.float32, device=torch.device(DEV), **kw)
    m.train()
    return m


def _scores(m, word=None):
    """{(table, key): score} of every stored key (word: the score word of a multi-word score, e.g. LRU_LFU's frequency = 1)"""
    import dynamicemb_extensions as ext

    out = {}
    for t in range(m.num_tables):
        if word is None:
            for k, _, s in m._export_table(t):
                out.update({(t, a): b for a, b in zip(k.cpu().tolist(), s.cpu().tolist())})
        else:
            tb = m.table
            C = tb.bucket_capacity_
            b0, b1 = int(tb.table_bucket_offsets_cpu_[t]), int(tb.table_bucket_offsets_cpu_[t + 1])
            n = (b1 - b0) * C
            cnt, keys, sc, _ = ext.table_export_batch(tb.table_storage_, C, n, b0 * C, torch.int64, None, b0 * C, tb.num_scores_, word)
            c = int(cnt.item())
            out.update({(t, a): b for a, b in zip(keys[:c].cpu().tolist(), sc[:c].cpu().tolist())})
    return out


def _rows(m):
    out = {}
    for t in range(m.num_tables):
        for k, r, _ in m._export_table(t):
            out.update({(t, a): b for a, b in zip(k.cpu().tolist(), r.cpu().numpy())})
    return out


def _batch(rng, T, B, maxlen, universe, zipf=None, n=None):
    """T features of B bags each (feature-major); keys of feature t are keys of table t"""
    lens = rng.integers(1, maxlen + 1, size=T * B)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nk = int(off[-1])
    keys = (rng.zipf(zipf, nk) % universe).astype(np.int64) if zipf else rng.integers(0, universe, nk).astype(np.int64)
    return keys, off


def _tables_of(off, T, B):
    lens = np.diff(off)
    return np.repeat(np.repeat(np.arange(T), B), lens)


def _step(m, keys, off, w=None, backward=True):
    """one training step; the output gradient is 2^-7 everywhere, so that every reduced row gradient is exact whatever order the
    backward adds it in (the rows of two runs are then comparable bit for bit)"""
    k = torch.from_numpy(keys).to(DEV)
    o = torch.from_numpy(off).to(DEV)
    wt = torch.from_numpy(w).to(DEV) if w is not None else None
    out = m(k, o, per_sample_weights=wt)
    if backward:
        out.backward(torch.full_like(out, 2.0 ** -7))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy()


def _c2(rng):
    """a C2-shaped batch: one table, 4096 bags of 1..175 keys ~ 360 K Zipf keys on a 1 M-row table"""
    lens = rng.integers(1, 176, size=4096)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = (rng.zipf(1.05, int(off[-1])) % 2_000_000).astype(np.int64) + (1 << 40)
    return keys, off


# ---------------------------------------------------------------------------------------------------- all-ones == none
@pytest.mark.parametrize("opt", ["SGD", "ADAM"])
@pytest.mark.parametrize("path", ["c", "b"])
def test_all_ones_weights_equal_no_weights_bit_for_bit(path, opt):
    rng = np.random.default_rng(11)
    if path == "c":
        batches = [_c2(rng) for _ in range(2)]
        kw = dict(dims=(128,), cap=1 << 20)
    else:
        batches = [_batch(rng, 2, 256, 20, 5000, zipf=1.2) for _ in range(3)]
        kw = dict(dims=(16, 32), cap=1 << 14)
    a, b = _mk(opt=opt, **kw), _mk(opt=opt, **kw)
    if path == "c":
        assert a._fused and a._plan_ok
    for keys, off in batches:
        oa = _step(a, keys, off)
        ob = _step(b, keys, off, np.ones(keys.size, np.float32))
        assert np.array_equal(oa, ob)
        if path == "c":
            assert keys.size >= 300_000
    sa, sb = _scores(a), _scores(b)
    assert sa == sb and len(sa) > 0
    ra, rb = _rows(a), _rows(b)
    assert ra.keys() == rb.keys() and all(np.array_equal(ra[k], rb[k]) for k in ra)


@pytest.mark.parametrize("strategy", ["LFU", "STEP"])
def test_all_ones_weights_equal_no_weights_under_prefetch_async(strategy):
    """STEP: the staged prefetch of path (c); LFU: the pinning prefetch (the staged one is for recency scores)"""
    rng = np.random.default_rng(5)
    batches = [_c2(rng) for _ in range(3)]
    a, b = _mk(strategy, dims=(64,), cap=1 << 20), _mk(strategy, dims=(64,), cap=1 << 20)
    outs = {}
    for m, ones in ((a, False), (b, True)):
        res = []
        dev = [(torch.from_numpy(k).to(DEV), torch.from_numpy(o).to(DEV)) for k, o in batches]
        w = [torch.ones(k.numel(), dtype=torch.int32, device=DEV) for k, _ in dev]
        m.prefetch_async(*dev[0], per_sample_weights=w[0] if ones else None)
        for i, (k, o) in enumerate(dev):
            out = m(k, o, per_sample_weights=w[i] if ones else None)
            if i + 1 < len(dev):
                m.prefetch_async(*dev[i + 1], per_sample_weights=w[i + 1] if ones else None)
            out.backward(torch.full_like(out, 2.0 ** -7))
            res.append(out.detach().cpu().numpy())
        torch.cuda.synchronize()
        outs[ones] = res
    for x, y in zip(outs[False], outs[True]):
        assert np.array_equal(x, y)
    assert _scores(a) == _scores(b)
    ra, rb = _rows(a), _rows(b)
    assert ra.keys() == rb.keys() and all(np.array_equal(ra[k], rb[k]) for k in ra)


# ---------------------------------------------------------------------------------------------------- scores follow weights
@pytest.mark.parametrize("pooling", ["SUM", "NONE"])
@pytest.mark.parametrize("path", ["c", "b"])
def test_lfu_scores_are_weight_sums(path, pooling):
    rng = np.random.default_rng(21 + len(pooling))
    T = 2
    if path == "c":
        if pooling == "NONE":
            B, maxlen, uni = 40_000, 1, 30_000      # sequence: 2 x 40 K tokens
        else:
            B, maxlen, uni = 4096, 20, 40_000
        cap, dims = 1 << 19, (16, 16)
    else:
        B, maxlen, uni, cap, dims = 300, 8, 3000, 1 << 14, (16, 16)
    m = _mk(dims=dims, pooling=pooling, cap=cap)
    acc = {}
    for _ in range(3):
        keys, off = _batch(rng, T, B, maxlen, uni, zipf=1.3)
        w = rng.integers(1, 9, keys.size).astype(np.int64)
        tt = _tables_of(off, T, B)
        _step(m, keys, off, w)
        for t, k, x in zip(tt.tolist(), keys.tolist(), w.tolist()):
            acc[(t, k)] = acc.get((t, k), 0) + x
        if path == "c":
            assert m._plan_ok
    sc = _scores(m)
    assert sc == acc


def test_lru_lfu_frequency_word_is_weight_sum():
    """the compound score (timer word, frequency word): the frequency word grows by the weight sums; float weights truncate"""
    rng = np.random.default_rng(4)
    m = _mk(("TIMESTAMP", "LFU"), dims=(16,), cap=1 << 19)
    assert m.table.num_scores_ == 2
    acc = {}
    for _ in range(3):
        keys, off = _batch(rng, 1, 8192, 20, 60_000, zipf=1.2)    # ~86 K keys: path (c)
        w = rng.integers(1, 9, keys.size).astype(np.float64) + 0.7      # truncated: 1..8
        _step(m, keys, off, w)
        for k, x in zip(keys.tolist(), w.astype(np.int64).tolist()):
            acc[(0, k)] = acc.get((0, k), 0) + x
    assert _scores(m, word=1) == acc


def test_weights_do_not_pool():
    rng = np.random.default_rng(8)
    keys, off = _batch(rng, 2, 512, 12, 2000)
    for pooling in ("SUM", "MEAN", "NONE"):
        a, b = _mk(dims=(16, 16), pooling=pooling), _mk(dims=(16, 16), pooling=pooling)
        w = rng.integers(1, 9, keys.size).astype(np.int64)
        assert np.array_equal(_step(a, keys, off), _step(b, keys, off, w))
        if pooling != "MEAN":      # (second step: the rows after the first -- exact gradients, see _step)
            assert np.array_equal(_step(a, keys, off), _step(b, keys, off, w))


@pytest.mark.parametrize("strategy", ["TIMESTAMP", "STEP"])
def test_other_strategies_ignore_weights(strategy, monkeypatch):
    import dynamicemb_extensions as ext

    monkeypatch.setattr(ext, "TIMER_OVERRIDE", 123456789, raising=False)
    rng = np.random.default_rng(9)
    a, b = _mk(strategy, dims=(16,)), _mk(strategy, dims=(16,))
    for _ in range(2):
        keys, off = _batch(rng, 1, 512, 10, 3000, zipf=1.2)
        w = rng.integers(1, 9, keys.size).astype(np.int64)
        assert np.array_equal(_step(a, keys, off), _step(b, keys, off, w))
    assert _scores(a) == _scores(b)


def test_eval_ignores_weights():
    """an eval forward with weights behaves as one without (an LFU eval lookup counts occurrences, as before)"""
    rng = np.random.default_rng(2)
    keys, off = _batch(rng, 1, 256, 8, 1000)
    a, b = _mk(dims=(16,)), _mk(dims=(16,))
    _step(a, keys, off)
    _step(b, keys, off)
    a.eval()
    b.eval()
    with torch.no_grad():
        oa = _step(a, keys, off, backward=False)
        ob = _step(b, keys, off, rng.integers(1, 9, keys.size).astype(np.int64), backward=False)
    assert np.array_equal(oa, ob)
    assert _scores(a) == _scores(b)


# ---------------------------------------------------------------------------------------------------- eviction
def test_eviction_follows_weights():
    """one bucket of 128 slots filled by 128 keys, then 8 unseen keys: LFU evicts the 8 lowest scores -- the weights decide which
    (a CPU model: lowest sum first); unweighted, the occurrence counts (made to disagree with the weights) decide"""
    rng = np.random.default_rng(13)
    base = np.arange(1000, 1128, dtype=np.int64)
    wts = rng.permutation(np.arange(1, 129)).astype(np.int64)           # distinct weight sums
    occ = 129 - wts                                                    # distinct counts, the opposite order
    new = np.arange(5000, 5008, dtype=np.int64)

    def run(weighted):
        m = _mk(dims=(8,), cap=128, pooling="NONE")
        assert m.table.capacity_ == 128
        if weighted:
            k1, w1 = base, wts
        else:
            k1, w1 = np.repeat(base, occ), None
        _step(m, k1, np.arange(k1.size + 1, dtype=np.int64), w1)
        _step(m, new, np.arange(new.size + 1, dtype=np.int64), np.ones(new.size, np.int64) if weighted else None)
        return {k for (_, k) in _scores(m)}

    sw, su = run(True), run(False)
    model_w = set(base[np.argsort(wts)[8:]].tolist()) | set(new.tolist())
    model_u = set(base[np.argsort(occ)[8:]].tolist()) | set(new.tolist())
    assert sw == model_w
    assert su == model_u
    assert sw != su


# ---------------------------------------------------------------------------------------------------- admission
def test_admission_counts_weights():
    from dynamicemb.embedding_admission import FrequencyAdmissionStrategy, KVCounter
    from dynamicemb.dynamicemb_config import DynamicEmbInitializerArgs as IA, DynamicEmbInitializerMode as IM

    def run(w):
        m = _mk("TIMESTAMP", dims=(8,), cap=4096,
                admit_strategy=FrequencyAdmissionStrategy(threshold=4, initializer_args=IA(mode=IM.CONSTANT, value=0.0)),
                admission_counter=KVCounter(capacity=4096, bucket_capacity=128))
        keys = np.array([77, 78], dtype=np.int64)
        _step(m, keys, np.array([0, 1, 2], dtype=np.int64), w)
        return {k for (_, k) in _scores(m)}

    assert run(np.array([5, 1], np.int64)) == {77}
    assert run(None) == set()


# ---------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_raise_before_launch():
    m = _mk(dims=(8,))
    k = torch.arange(10, dtype=torch.int64, device=DEV)
    o = torch.tensor([0, 5, 10], dtype=torch.int64, device=DEV)
    for bad in (torch.ones(9, device=DEV), torch.ones(10), torch.ones(10, 1, device=DEV)):
        with pytest.raises(ValueError):
            m(k, o, per_sample_weights=bad)
        with pytest.raises(ValueError):
            m.prefetch(k, o, frequency_counters=bad)
        with pytest.raises(ValueError):
            m.prefetch_async(k, o, per_sample_weights=bad)
    torch.cuda.synchronize()
    assert _scores(m) == {}


# ---------------------------------------------------------------------------------------------------- external storage
def test_external_storage_receives_weight_sums():
    from test_module_gpu import _DictStore

    seen = []

    class Rec:
        def __new__(cls, options, optimizer):
            s = _DictStore(options, optimizer)
            f = s.find

            def find(unique_keys, table_ids, copy_mode, lfu_accumulated_frequency=None):
                if lfu_accumulated_frequency is not None:
                    seen.append(dict(zip(unique_keys.cpu().tolist(), lfu_accumulated_frequency.cpu().tolist())))
                return f(unique_keys, table_ids, copy_mode, lfu_accumulated_frequency)

            s.find = find
            return s

    m = _mk(dims=(8,), external_storage=Rec)
    keys = np.array([3, 4, 3, 5, 3, 4], dtype=np.int64)
    w = np.array([2, 1, 3, 7, 1, 4], dtype=np.int64)
    _step(m, keys, np.array([0, 3, 6], dtype=np.int64), w)
    assert seen and seen[-1] == {3: 6, 4: 5, 5: 7}


# ---------------------------------------------------------------------------------------------------- flood re-run
def _fmix64(k):
    k = k.astype(np.uint64)
    k ^= k >> np.uint64(33); k *= np.uint64(0xFF51AFD7ED558CCD)
    k ^= k >> np.uint64(33); k *= np.uint64(0xC4CEB9FE1A85EC53)
    k ^= k >> np.uint64(33)
    return k


@pytest.mark.parametrize("mode", ["notice", "1"])
def test_flooded_weighted_step_scores_once(mode, tmp_path):
    """4 000 distinct keys of partition 0 drawn 80 000 times flood its record list; the re-run (the notice's, or the in-line
    gated chain of MI355_FUSED_OVERFLOW_RERUN=1) must not add the weight sums a second time"""
    code = r"""
import sys, numpy as np, torch
sys.path[:0] = [sys.argv[2], sys.argv[3]]
import test_lfu_weights_gpu as T
import mi355_native
m = T._mk(dims=(16,), cap=1 << 20)
S, C = m.table.capacity_, 128
n = 80_000
P = mi355_native.lib().mi355_demb_forward_fused_partitions(n, 1, m.table.num_buckets_)
assert P > 0
spp = -(-((S + 1 + P - 1) // P) // C) * C
cand = np.arange(1 << 30, (1 << 30) + 6 * 4000 * P, dtype=np.int64)
h = T._fmix64(cand) & np.uint64(0x7FFFFFFFFFFFFFFF)
bucket = (h % np.uint64(S)) // np.uint64(C)
pool = cand[(bucket * np.uint64(C)) // np.uint64(spp) == 0][:4000]
rng = np.random.default_rng(3)
keys = pool[rng.integers(0, 4000, n)]
off = np.arange(0, n + 1, 4, dtype=np.int64)
w = rng.integers(1, 9, n).astype(np.int64)
T._step(m, keys, off, w)
acc = {}
for k, x in zip(keys.tolist(), w.tolist()):
    acc[(0, k)] = acc.get((0, k), 0) + x
sc = T._scores(m)
assert int(m._fused_aux[6]) != 0, "no flood"
assert sc == acc, "scores differ"
print("OK", getattr(m, "overflow_reruns", 0))
"""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, **({"MI355_FUSED_OVERFLOW_RERUN": "1"} if mode == "1" else {}))
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path), here, os.path.join(root, "recsys-examples_amd")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
