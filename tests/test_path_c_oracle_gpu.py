"""The timed C2 training step's kernels on the partitioned index path -- path (c): probe_c_kernel, fused_part3_kernel,
gather_pooled_late_kernel / gather_rows_late_kernel and bwd_kernel with its hot-row lists -- against an INDEPENDENT twin
(oracle/vec_twin.py: sorted key arrays, fp64 pooling, the fp32 optimizer maths of oracle.py), not against another HIP path.

Every element is compared with a bound derived from the arithmetic (oracle/vec_twin.py: forward_bound, grad_sum_error,
grad_interval, update_bracket), not with a max-norm: outputs within gamma(n) sum|terms| + half an ulp of the output dtype;
rows within the fp32 update of the twin at both ends of the reduced gradient's rounding interval, plus the fp32 evaluation
slack.  After each backward the touched rows are checked and the twin carries the product's rows on (so every step is
judged by a one-step bound); after the last step every stored key, row and score is compared exactly, then an eval forward
of known and unknown keys (gather_pooled_eval_kernel).  Every case asserts it ran on path (c) (the step context is lazy)
and that the fused forward's per-slot counters are clear afterwards.

Warm keys are preloaded with random per-column rows and state; new keys get the CONSTANT initialiser (one case: UNIFORM,
whose rows the twin reads back after their first forward and checks for range).  Out of scope: eviction -- every case
keeps its universe of keys far below the table's capacity.  Path (c) needs rows of <= 256 elements in multiples of 4 and
an fp32 / bf16 output (fused_fwd.hip, `pathc`): D = 13, D = 512 and an fp16 output take the per-slot-counter path, and
the two cases here that use them assert so while checking the same backward kernels against the twin."""
import time

import numpy as np
import pytest
import torch

from oracle.vec_twin import (VecEmbeddingTwin, bound_use, constant_rows, forward_bound, interval_use)

pytestmark = pytest.mark.gpu
DEV = "cuda"
_OPT = {"SGD": "sgd", "ADAM": "adam", "EXACT_ADAGRAD": "adagrad", "EXACT_ROWWISE_ADAGRAD": "rowwise_adagrad"}
_TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
INIT = 0.25


def _record(kind, case, use):
    """worst |err| / bound per comparison kind: printed per step, and summarised at the end of the run by conftest's hook"""
    use = float(use)
    try:
        from conftest import record_tolerance_use
        record_tolerance_use(kind, case, use)
    except ImportError:
        pass
    print(f"path_c_bound_used {kind:14s} {use:9.6f}  ({case})")


def _counters_clear(m, except_flag=False):
    """header + per-slot occurrence counters of the fused forward are all zero between steps (except_flag: aux[6] holds the
    epoch of the last flooded step -- a value, not state)"""
    torch.cuda.synchronize()
    aux = m._fused_aux.clone()
    if except_flag:
        aux[5] = 0
        aux[6] = 0
    cap = m.table.capacity_
    H = 64 + 4 * 4096
    return int(aux[:H].abs().sum()) == 0 and int(aux[H: H + 2 * (cap + 1): 2].abs().sum()) == 0


def _module(dims, fmap, pooling, opt, out_dtype, strategy, cap, lr, init="CONSTANT"):
    from dynamicemb.batched_dynamicemb_tables import BatchedDynamicEmbeddingTablesV2 as B2
    from dynamicemb.dynamicemb_config import (DynamicEmbInitializerArgs as IA, DynamicEmbInitializerMode as IM,
                                              DynamicEmbPoolingMode as PM, DynamicEmbScoreStrategy as SS,
                                              DynamicEmbTableOptions as TO, EmbOptimType as OT)
    ia = IA(mode=IM.CONSTANT, value=INIT) if init == "CONSTANT" else IA(mode=IM.UNIFORM, lower=-0.5, upper=0.5)
    opts = [TO(dim=d, max_capacity=cap, index_type=torch.int64, embedding_dtype=torch.float32, bucket_capacity=128,
               initializer_args=ia, score_strategy=getattr(SS, strategy)) for d in dims]
    m = B2(table_options=opts, feature_table_map=fmap, pooling_mode=getattr(PM, pooling), optimizer=getattr(OT, opt),
           output_dtype=_TD[out_dtype], learning_rate=lr, device=torch.device(DEV))
    assert m._fused and m._plan_ok
    m.train()
    return m


def _warm_rows(rng, n, d, opt):
    """random per-column rows [emb | state]: state of the optimizer's sign (Adam m any sign, v >= 0, AdaGrad G >= 0)"""
    w = rng.standard_normal((n, d)).astype(np.float32)
    if opt == "SGD":
        return w
    if opt == "ADAM":
        return np.concatenate([w, 0.01 * rng.standard_normal((n, d)), rng.uniform(0, 1e-3, (n, d))], 1).astype(np.float32)
    if opt == "EXACT_ADAGRAD":
        return np.concatenate([w, rng.uniform(0, 1, (n, d))], 1).astype(np.float32)
    return np.concatenate([w, rng.uniform(0, 1, (n, 1)), np.zeros((n, 3))], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ batches
def _zipf_keys(rng, n, alpha, universe, base):
    """n keys of a Zipf(alpha) law over `universe` ranks, ranks scattered over the key space by a fixed permutation"""
    w = np.arange(1, universe + 1, dtype=np.float64) ** -alpha
    cdf = np.cumsum(w)
    r = np.searchsorted(cdf / cdf[-1], rng.random(n))
    return base + (r * 2654435761) % (1 << 40)


def _lens(rng, bags, lo, hi):
    lens = rng.integers(lo, hi + 1, bags)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _c2(rng, step, F=1):
    """C2: 65 536 bags of 1-10 keys, Zipf 0.99 (~360 K keys, the head row in tens of thousands of bags)"""
    off = _lens(rng, 65536 * F, 1, 10)
    return _zipf_keys(rng, int(off[-1]), 0.99, 2_000_000, 1 << 41), off


def _uniform(bags, lo, hi, universe, F=1):
    def gen(rng, step):
        off = _lens(rng, bags * F, lo, hi)
        return (1 << 42) + rng.integers(0, universe, int(off[-1])), off
    return gen


def _hot_classes(rng, step):
    """one batch with every hot-row class of csrc/hot.h: <= 4 occurrences (regular walk), 5-128 (one wave), 129-1024 (one
    chunk), > 1024 (several chunks, atomics, last ticket applies the sink), and 2 200 rows x 160 occurrences so that the
    chunk tasks outnumber the 2 048 hot blocks"""
    parts = []
    base = 1 << 43
    def cls(n, lo, hi):
        nonlocal base
        k = base + np.arange(n)
        base += n
        parts.append(np.repeat(k, rng.integers(lo, hi + 1, n)))
    cls(60_000, 1, 4)
    cls(2_000, 5, 128)
    cls(200, 129, 1024)
    for c in (1025, 2048, 5000, 20000, 40000):
        cls(1, c, c)
    cls(2_200, 160, 160)
    keys = np.concatenate(parts)
    keys = keys[rng.permutation(keys.size)]
    keys = keys[: keys.size // 8 * 8]
    return keys, np.arange(0, keys.size + 1, 8, dtype=np.int64)


CASES = {
    # name: (batch, dims, fmap, pooling, optimizer, out dtype, grad dtype, score, api, steps, path c?)
    "c2_adam_bf16": (_c2, [128], [0], "SUM", "ADAM", "bf16", "bf16", "TIMESTAMP", "autograd", 2, True),
    "c2_sgd_bf16": (_c2, [128], [0], "SUM", "SGD", "bf16", "bf16", "LFU", "autograd", 3, True),
    "above_64k_mean_adagrad": (_uniform(22_500, 0, 6, 150_000), [64], [0], "MEAN", "EXACT_ADAGRAD", "f32", "f32", "STEP", "autograd", 3, True),
    "below_393k_rowwise_f16": (_uniform(86_500, 1, 8, 600_000), [32], [0], "SUM", "EXACT_ROWWISE_ADAGRAD", "f32", "f16", "LFU", "impl", 3, True),
    "above_393k_mean_sgd_f16": (_uniform(100_000, 0, 8, 600_000), [32], [0], "MEAN", "SGD", "bf16", "f16", "TIMESTAMP", "impl", 3, True),
    "over_720k_unique_sgd": (_uniform(160_000, 1, 9, 40_000_000), [16], [0], "SUM", "SGD", "f32", "f32", "STEP", "impl", 2, True),
    "near_1m_adam": (_uniform(231_000, 1, 8, 3_000_000), [8], [0], "SUM", "ADAM", "f32", "bf16", "STEP", "impl", 3, True),
    "sequence_sgd_bf16": (_uniform(30_000, 2, 6, 100_000), [64], [0], "NONE", "SGD", "bf16", "bf16", "LFU", "autograd", 3, True),
    "sequence_adam": (_uniform(25_000, 2, 6, 100_000), [32], [0], "NONE", "ADAM", "f32", "f32", "STEP", "impl", 3, True),
    "mixed_dims_rowwise_bf16": (_uniform(20_000, 1, 6, 200_000, F=4), [32, 64, 128], [0, 1, 2, 2], "SUM", "EXACT_ROWWISE_ADAGRAD",
                                "bf16", "bf16", "TIMESTAMP", "autograd", 3, True),
    "mixed_dims_mean_adam_f16": (_uniform(30_000, 0, 7, 200_000, F=3), [16, 48], [0, 0, 1], "MEAN", "ADAM", "f32", "f16", "LFU",
                                 "impl", 3, True),
    "mixed_dims_sgd": (_uniform(25_000, 1, 5, 200_000, F=3), [8, 24, 40], [0, 1, 2], "SUM", "SGD", "f32", "bf16", "STEP", "impl", 3,
                       True),
    "hot_classes_adam": (_hot_classes, [32], [0], "SUM", "ADAM", "f32", "bf16", "LFU", "impl", 2, True),
    "d13_f16_out_sgd": (_uniform(20_000, 1, 6, 100_000), [13], [0], "SUM", "SGD", "f16", "f16", "STEP", "impl", 3, False),
    "d512_adam_bf16": (_uniform(20_000, 1, 6, 60_000), [512], [0], "SUM", "ADAM", "bf16", "bf16", "TIMESTAMP", "autograd", 3, False),
}


def _run(case, rng, m, twin, gen, steps, out_dtype, gdt, api, pathc, extra_steps=()):
    """train `steps` batches of `gen` (then the batches of extra_steps), each step checked against the twin"""
    mean = twin.pooling == "MEAN"
    for it in range(steps + len(extra_steps)):
        keys, off = gen(rng, it) if it < steps else extra_steps[it - steps]
        kt, ot = torch.from_numpy(keys).to(DEV), torch.from_numpy(off).to(DEV)
        if api == "autograd":
            out = m(kt, ot)
            st = out.grad_fn.step
        else:
            out, st = m._forward_impl(kt, ot, train=True)
        assert bool(getattr(st, "lazy", False)) == pathc, f"{case} step {it}: path (c) {'not ' if pathc else ''}taken"
        x = twin.forward(keys, off, True)
        reruns = getattr(m, "overflow_reruns", 0)
        got = out.detach().double().cpu().numpy()
        fu = bound_use(got, x, forward_bound(x, twin.abs_sum, twin.nterms, out_dtype, mean))
        _record("pathc_forward", case, fu.max())
        assert (fu <= 1).all(), f"{case} step {it}: forward beyond its bound at {np.argwhere(fu > 1)[:5].tolist()}"
        g = torch.from_numpy(rng.uniform(-0.5, 1.0, x.shape).astype(np.float32)).to(DEV).to(_TD[gdt])
        if api == "autograd":
            assert g.dtype == out.dtype
            out.backward(g)
        else:
            m._backward_impl(st, g)
        twin.backward(g.double().cpu().numpy())
        # (a step whose partition list flooded -- re-run on the per-slot counters -- leaves its epoch in aux[6] for the steps
        # after it: a value, not state)
        flooded = getattr(m, "overflow_reruns", 0) > reruns
        ever = getattr(m, "overflow_reruns", 0) > 0
        assert _counters_clear(m, except_flag=ever), f"{case} step {it}: per-slot counters left set (flooded: {flooded})"
        if flooded:
            print(f"path_c case {case} step {it}: a partition list flooded and the step was re-run")
        for t in range(len(twin.dims)):
            if twin.last_grad[t] is None:
                continue
            uk, lo, hi, slack = twin.row_bracket(t)
            f, rows = m.lookup_rows(torch.from_numpy(uk).to(DEV), t)
            assert bool(f.all()), f"{case} step {it}: keys of the batch missing from table {t}"
            rows = rows.cpu().numpy()
            u = interval_use(rows, lo, hi, slack)
            d = twin.dims[t]
            _record("pathc_row_emb", case, u[:, :d].max())
            i, j = np.unravel_index(np.argmax(u), u.shape)
            if u[i, j] > 0.5:
                lg = twin.last_grad[t]
                print(f"path_c worst row element {case} step {it}: key {int(uk[i])} col {int(j)} cnt {int(lg['cnt'][i])} "
                      f"got {rows[i, j]!r} span [{lo[i, j]!r}, {hi[i, j]!r}] slack {slack[i, j]!r} before {lg['rows_before'][i, j]!r} "
                      f"s {lg['s'][i, min(j, d - 1)]!r} use {u[i, j]:.6f}")
            if u.shape[1] > d:
                _record("pathc_row_state", case, u[:, d:].max())
            bad = np.argwhere(u > 1)
            assert bad.size == 0, (f"{case} step {it} table {t}: {len(bad)} row elements outside the bracket, first (key, col) "
                                   f"{[(int(uk[i]), int(j)) for i, j in bad[:4]]}, occurrences {twin.last_grad[t]['cnt'][bad[:4, 0]].tolist()}, "
                                   f"got {rows[bad[0, 0], bad[0, 1]]!r} bracket [{lo[bad[0, 0], bad[0, 1]]!r}, {hi[bad[0, 0], bad[0, 1]]!r}]"
                                   f" slack {slack[bad[0, 0], bad[0, 1]]!r}")
            twin.set_rows(t, uk, rows)       # the next step is judged from the rows the product holds


def _final_checks(case, m, twin, strategy):
    """every stored key, row and score; then an eval forward of known and unknown keys"""
    torch.cuda.synchronize()
    assert int(m.size()) == twin.size()
    for t in range(len(twin.dims)):
        ks, rs, ss = [], [], []
        for k, r, s in m._export_table(t):
            ks.append(k.cpu().numpy()); rs.append(r.cpu().numpy()); ss.append(s.cpu().numpy())
        k, r, s = np.concatenate(ks), np.concatenate(rs), np.concatenate(ss)
        o = np.argsort(k)
        k, r, s = k[o], r[o], s[o]
        tk, lfu, last = twin.scores(t)
        assert np.array_equal(k, tk), f"{case} table {t}: stored key sets differ ({k.size} vs {tk.size})"
        # rows the last steps did not touch must be exactly what the twin holds (nobody else wrote them)
        assert np.array_equal(r, twin.rows[t]), f"{case} table {t}: {int((r != twin.rows[t]).any(1).sum())} stored rows differ"
        if strategy == "LFU":
            assert np.array_equal(s, lfu.astype(s.dtype)), f"{case} table {t}: LFU scores differ"
        elif strategy == "STEP":
            assert np.array_equal(s, last.astype(s.dtype)), f"{case} table {t}: STEP scores differ"
        else:      # TIMESTAMP: keys touched by a later step never score below keys touched by an earlier one
            groups = sorted(set(last.tolist()))
            for a, b in zip(groups, groups[1:]):
                assert s[last == a].max() <= s[last == b].min(), f"{case} table {t}: timestamps of step {a} above step {b}"


def _eval_check(case, m, twin, rng, out_dtype):
    F, B = len(twin.fmap), 4096
    off = _lens(rng, F * B, 0, 6)
    n = int(off[-1])
    known = np.concatenate(twin.keys)
    keys = np.where(rng.random(n) < 0.6, known[rng.integers(0, known.size, n)], (1 << 45) + rng.integers(0, 1 << 30, n))
    size0 = int(m.size())
    m.eval()
    with torch.no_grad():
        out = m(torch.from_numpy(keys).to(DEV), torch.from_numpy(off).to(DEV))
    m.train()
    x = twin.forward(keys, off, False)
    got = out.double().cpu().numpy()
    u = bound_use(got, x, forward_bound(x, twin.abs_sum, twin.nterms, out_dtype, twin.pooling == "MEAN"))
    _record("pathc_eval", case, u.max())
    assert (u <= 1).all(), f"{case}: eval forward beyond its bound"
    zero = twin.abs_sum == 0           # bags of unknown keys only (and empty bags): exactly zero
    assert (got[zero] == 0).all(), f"{case}: eval output of unknown keys is not zero"
    assert int(m.size()) == size0, f"{case}: the eval forward inserted keys"


def _setup(case, rng, dims, fmap, pooling, opt, out_dtype, gdt, strategy, cap, lr, init="CONSTANT", warm=None):
    m = _module(dims, fmap, pooling, opt, out_dtype, strategy, cap, lr, init)
    twin_init = constant_rows(INIT)
    if init != "CONSTANT":
        def twin_init(keys, d, _m=m):        # UNIFORM: the twin reads the rows the product drew (range checked there)
            t = dims.index(d)
            f, r = _m.lookup_rows(torch.from_numpy(np.asarray(keys)).to(DEV), t)
            assert bool(f.all())
            r = r[:, :d].cpu().numpy()
            assert (r >= -0.5).all() and (r < 0.5).all(), "UNIFORM rows outside [lower, upper)"
            assert (r.max(1) > r.min(1)).all(), "UNIFORM rows constant along the row"
            return r
    twin = VecEmbeddingTwin(dims, fmap, pooling, _OPT[opt], lr=lr, init=twin_init, grad_dtype=gdt)
    score = 0
    for t, d in enumerate(dims):
        wk = warm[t] if warm is not None else None
        if wk is None or wk.size == 0:
            continue
        rows = _warm_rows(rng, wk.size, d, opt)
        V = m.value_dims[t]
        rows = np.concatenate([rows, np.zeros((wk.size, V - rows.shape[1]), np.float32)], 1)
        m._insert_rows(t, torch.from_numpy(wk).to(DEV), torch.from_numpy(rows).to(DEV),
                       torch.full((wk.size,), score, dtype=torch.int64, device=DEV))
        twin.load(t, wk, rows, score)
    return m, twin


@pytest.mark.parametrize("case", list(CASES))
def test_path_c_step_against_the_vec_twin(case):
    gen, dims, fmap, pooling, opt, out_dtype, gdt, strategy, api, steps, pathc = CASES[case]
    t0 = time.perf_counter()
    rng = np.random.default_rng(sum(map(ord, case)))
    lr = {"SGD": 0.05, "ADAM": 0.01, "EXACT_ADAGRAD": 0.05, "EXACT_ROWWISE_ADAGRAD": 0.05}[opt]
    # warm keys: about half of what the first batch draws, per table
    k0, o0 = gen(np.random.default_rng(rng.integers(1 << 31)), 0)
    F, B = len(fmap), (o0.size - 1) // len(fmap)
    tab = np.asarray(fmap)[np.repeat(np.arange(F * B) // B, np.diff(o0))]
    warm = []
    for t in range(len(dims)):
        u = np.unique(k0[tab == t])
        warm.append(u[rng.random(u.size) < 0.5])
    cap = max(1 << 21, 1 << int(np.ceil(np.log2(4 * steps * max(k0.size, 1) + 1))))
    cap = min(cap, 1 << 23)
    m, twin = _setup(case, rng, dims, fmap, pooling, opt, out_dtype, gdt, strategy, cap, lr, warm=warm)
    _run(case, rng, m, twin, gen, steps, out_dtype, gdt, api, pathc)
    _final_checks(case, m, twin, strategy)
    _eval_check(case, m, twin, rng, out_dtype)
    print(f"path_c case {case}: {time.perf_counter() - t0:.1f} s")


def test_path_c_uniform_initialiser_against_the_vec_twin():
    """UNIFORM new rows: the twin takes them from the table after their first forward (in [lower, upper), not constant)"""
    case = "uniform_init_sgd"
    rng = np.random.default_rng(41)
    gen = _uniform(20_000, 1, 6, 200_000)
    m, twin = _setup(case, rng, [32], [0], "SUM", "SGD", "f32", "f32", "STEP", 1 << 21, 0.05, init="UNIFORM",
                     warm=[(1 << 42) + np.arange(0, 200_000, 3, dtype=np.int64)])
    _run(case, rng, m, twin, gen, 3, "f32", "f32", "impl", True)
    _final_checks(case, m, twin, "STEP")
    _eval_check(case, m, twin, rng, "f32")


def test_flooded_partition_and_the_step_after_against_the_vec_twin():
    """the flood of test_overflowed_partition_is_rerun_and_no_update_is_lost -- 4 000 keys of one slot-range partition drawn
    80 000 times, one sequence lookup each -- re-run on the per-slot-counter path by the backward, and the step after it,
    against the twin instead of against another HIP path"""
    from mi355_native import lib
    case = "flood_sequence_sgd"
    rng = np.random.default_rng(3)
    m, twin = _setup(case, rng, [16], [0], "NONE", "SGD", "f32", "f32", "TIMESTAMP", 1 << 20, 0.5)
    n, C = 80_000, 128
    P = int(lib().mi355_demb_forward_fused_partitions(n, m.num_tables, m.table.num_buckets_))
    assert P > 0
    S = m.table.capacity_
    spp = -(-((S + 1 + P - 1) // P) // C) * C
    cand = np.arange(1 << 30, (1 << 30) + 6 * 4000 * P, dtype=np.int64)
    h = cand.astype(np.uint64)
    h ^= h >> np.uint64(33); h *= np.uint64(0xFF51AFD7ED558CCD)
    h ^= h >> np.uint64(33); h *= np.uint64(0xC4CEB9FE1A85EC53)
    h ^= h >> np.uint64(33)
    h &= np.uint64(0x7FFFFFFFFFFFFFFF)
    bucket = (h % np.uint64(S)) // np.uint64(C)
    pool = cand[(bucket * np.uint64(C)) // np.uint64(spp) == 0][:4000]
    assert pool.size == 4000
    flood = pool[rng.integers(0, 4000, n)]
    reruns0 = getattr(m, "overflow_reruns", 0)
    normal = _uniform(30_000, 1, 6, 200_000)
    k1, o1 = normal(rng, 0)
    k3, o3 = normal(rng, 2)
    extra = [(k1, o1), (flood, np.arange(n + 1, dtype=np.int64)), (k3, o3)]
    _run(case, rng, m, twin, None, 0, "f32", "f32", "impl", True, extra_steps=extra)
    assert getattr(m, "overflow_reruns", 0) == reruns0 + 1, "the flood did not overflow a partition list"
    _final_checks(case, m, twin, "TIMESTAMP")

