"""WHICH keys the fused index stage evicts (csrc/fused_fwd.hip, csrc/part3_lean.h), against the CPU model of tests/evict_model.py.

The fused DynamicEmb forward carries three hand-written copies of the scored hash table's eviction: evict_phase inside
fused_mid_kernel (the per-slot-counter path (b), batches below 65 536 keys), part_evict under fused_part3_kernel (the pooled
partitioned path (c)) and part_evict under part3_lean.h (sequence lookups: the partition blocks ride in the gather's launch).
Every case fills its tables to capacity in four generations of training steps, then runs two or three measured steps whose
batches mix resident keys (60 % of the occurrences) with keys nobody has seen; around each measured step the tables are
exported and evict_model.check_step holds the step to the rule: hits stay and are scored by the policy; exactly the e lowest
eligible scores leave (ties on the cut may fall either way); a bucket with more newcomers than it can make room for refuses
exactly the surplus; a new key's row is the initialiser's row followed by the state's initial value, bit for bit, before the
backward and the optimizer's update of that row after it; every bystander keeps key, score and row bit for bit; sizes add up
and the per-slot counters are clear.  tests/test_evict_model_cpu.py vets the same batches on the CPU (enough evictions, case 3
only where meant, no partition near kDefMax deferred records -- so a key refused while a victim existed is a bug, not a limit).
Two cases run PAST that budget (a partition block evicts for at most kDefMax deferred (tile, key) records per step): there a
new key may go without a slot, but as a whole -- every occurrence of a key with a slot reads its row and counts for its score
and its update, a key without one reads zeros everywhere.

Out of scope: pinned slots (the counter array, cache rows of an external store), the prefetch pipeline's `protect` bound,
reclaimed (erased) slots, the overflow arena, and the flooded-partition re-run (tests/test_path_c_oracle_gpu.py has that)."""
import numpy as np
import pytest
import torch

import evict_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
INIT, STATE0, LR = 0.25, 0.0625, 0.1
U32 = 2.0 ** -24


def _mk(cfg):
    from dynamicemb.batched_dynamicemb_tables import BatchedDynamicEmbeddingTablesV2 as B2
    from dynamicemb.dynamicemb_config import (DynamicEmbInitializerArgs as IA, DynamicEmbInitializerMode as IM,
                                              DynamicEmbPoolingMode as PM, DynamicEmbScoreStrategy as SS,
                                              DynamicEmbTableOptions as TO, EmbOptimType as OT)
    strat = (SS.TIMESTAMP, SS.LFU) if cfg.policy == "LRU_LFU" else getattr(SS, cfg.policy)
    opts = [TO(dim=cfg.dim, max_capacity=cap, index_type=torch.int64, embedding_dtype=torch.float32, bucket_capacity=cfg.C,
               initializer_args=IA(mode=IM.CONSTANT, value=INIT), score_strategy=strat) for cap in cfg.caps]
    m = B2(table_options=opts, feature_table_map=list(range(len(cfg.caps))), pooling_mode=getattr(PM, cfg.pooling),
           optimizer=getattr(OT, cfg.opt), learning_rate=LR, initial_accumulator_value=STATE0, output_dtype=torch.float32,
           device=torch.device(DEV))
    m.train()
    assert m._fused and m._plan_ok
    assert m.table.bucket_capacity_ == cfg.C and list(m.table.per_table_capacity_) == list(cfg.caps)
    assert np.array_equal(m.table.table_bucket_offsets_cpu_.numpy(), M.tbo_of(cfg.caps, cfg.C))
    return m


def _export(m):
    """per table (keys, compared score word, rows) on the host: m._export_table for one-word scores; the LAST word of a two-word
    score (the one reduce_min compares) through table_export_batch"""
    import dynamicemb_extensions as ext

    tb = m.table
    out = []
    for t in range(m.num_tables):
        if tb.num_scores_ == 1:
            parts = list(m._export_table(t))
            k = torch.cat([p[0] for p in parts]) if parts else torch.zeros(0, dtype=torch.int64)
            r = torch.cat([p[1] for p in parts]) if parts else torch.zeros(0, m.value_dims[t])
            s = torch.cat([p[2] for p in parts]) if parts else torch.zeros(0, dtype=torch.int64)
        else:
            C = tb.bucket_capacity_
            b0, b1 = int(tb.table_bucket_offsets_cpu_[t]), int(tb.table_bucket_offsets_cpu_[t + 1])
            cnt, keys, sc, idx = ext.table_export_batch(tb.table_storage_, C, (b1 - b0) * C, b0 * C, torch.int64, None, b0 * C,
                                                        tb.num_scores_, tb.num_scores_ - 1)
            c = int(cnt.item())
            k, s, r = keys[:c], sc[:c], m.values[t][idx[:c].to(m.values[t].device)]
        out.append((k.cpu().numpy(), s.cpu().numpy(), r.float().cpu().numpy()))
    return out


def _timer_words(m):
    """{key: word 0} of a two-word score (table 0)"""
    import dynamicemb_extensions as ext

    tb = m.table
    C = tb.bucket_capacity_
    n = int(tb.table_bucket_offsets_cpu_[1]) * C
    cnt, keys, sc, _ = ext.table_export_batch(tb.table_storage_, C, n, 0, torch.int64, None, 0, tb.num_scores_, 0)
    c = int(cnt.item())
    return keys[:c].cpu().numpy(), sc[:c].cpu().numpy()


def _forward(m, cfg, bt, monkeypatch):
    import dynamicemb_extensions as ext

    if cfg.policy == "STEP":
        assert m._step == bt.value, "the module's step counter is not the score the model expects"
    elif cfg.policy == "CUSTOMIZED":
        m.set_score(bt.value)
    else:
        monkeypatch.setattr(ext, "TIMER_OVERRIDE", int(bt.value), raising=False)
    k, o = torch.from_numpy(bt.keys).to(DEV), torch.from_numpy(bt.off).to(DEV)
    if bt.w is None:
        out, st = m._forward_impl(k, o, train=True)
    else:
        w = m._check_weights(torch.from_numpy(bt.w).to(DEV), k)
        out, st = m._with_weights(w, m._forward_impl, k, o, train=True)
    return out, st, bool(getattr(st, "lazy", False))


def _backward(m, st, out):
    m._backward_impl(st, torch.full_like(out, 2.0 ** -7))     # an exact gradient: every reduced row gradient is occurrences * 2^-7
    torch.cuda.synchronize()


def _updater(m, cfg):
    """update(t, rows, occurrences) of evict_model.check_step: the optimizer's step (oracle/oracle.py, fp32 like the kernels) on a
    row gradient of occurrences * 2^-7 in every column.  Tolerance per element: the update is a dozen fp32 operations on values no
    larger than |old| + |new| + lr, each rounded to 2^-24 relative, the device's sqrt and division within two units of that:
    16 * 2^-24 * (|old| + |new| + lr).  (SGD: two roundings; the same bound is kept.)"""
    from oracle import oracle as orc

    D = cfg.dim
    it = m._iter_num

    def update(t, rows, cnt):
        old = rows.copy()
        g = np.repeat((cnt.astype(np.float32) * np.float32(2.0 ** -7))[:, None], D, axis=1)
        if cfg.opt == "SGD":
            new = orc.sgd_update(rows, g, D, LR)
        elif cfg.opt == "ADAM":
            new = orc.adam_update(rows, g, D, LR, m.beta1, m.beta2, m.eps, m.weight_decay, it)
        else:
            new = orc.rowwise_adagrad_update(rows, g, D, LR, m.eps)
        return new, 16 * U32 * (np.abs(old.astype(np.float64)) + np.abs(new.astype(np.float64)) + LR)

    return update


def _check_output(cfg, bt, out, before, fresh, rep):
    """what the forward returned: a hit reads the row it had before the step, a new key its fresh row, a refused key zeros.
    Sequence lookups: bit for bit.  Pooled (SUM): against the float64 sum of the bag; an fp32 sum of L terms in any order is
    within L * 2^-24 * sum|x| of it."""
    D, T = cfg.dim, len(cfg.caps)
    n = bt.keys.size
    rows = np.zeros((n, D), np.float32)
    refused = set(zip(rep.refused[0].tolist(), rep.refused[1].tolist()))
    for t in range(T):
        sel = np.flatnonzero(bt.tids == t)
        bk, _, br = before[t]
        o = np.argsort(bk)
        p = np.minimum(np.searchsorted(bk[o], bt.keys[sel]), bk.size - 1)
        hit = bk[o][p] == bt.keys[sel]
        r = np.where(hit[:, None], br[o][p][:, :D], fresh[t][None, :D])
        if refused:
            r[np.array([(t, x) in refused for x in bt.keys[sel].tolist()])] = 0.0
        rows[sel] = r
    got = out.detach().float().cpu().numpy()
    if cfg.pooling == "NONE":
        assert got.shape == rows.shape
        ne = (got.view(np.uint32) != rows.view(np.uint32)).any(axis=1)
        assert not ne.any(), f"occurrence {int(np.flatnonzero(ne)[0])} (key {int(bt.keys[np.flatnonzero(ne)[0]])}): the output row is not the key's row"
        return
    nb = bt.off.size - 1
    Bn = nb // T
    bag = np.repeat(np.arange(nb), np.diff(bt.off))
    ref, mag = np.zeros((nb, D)), np.zeros((nb, D))
    np.add.at(ref, bag, rows.astype(np.float64))
    np.add.at(mag, bag, np.abs(rows.astype(np.float64)))
    tol = np.diff(bt.off)[:, None] * U32 * mag
    got = got.reshape(Bn, T, D).transpose(1, 0, 2).reshape(nb, D)       # [B, T * D] -> bag f * B + b
    err = np.abs(got - ref)
    assert (err <= tol).all(), f"bag {int(np.argmax((err - tol).max(axis=1)))}: pooled output off by {float((err - tol).max()):.3e} beyond its bound"


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_the_step_evicts_what_the_model_allows(name, monkeypatch):
    from mi355_native import lib
    from test_fused_fwd_gpu import _counters_clear

    g = M.generate(name)
    cfg, spec = g.cfg, g.spec
    T = len(cfg.caps)
    m = _mk(cfg)
    fresh = [np.concatenate([np.full(cfg.dim, INIT, np.float32), np.full(m.value_dims[t] - cfg.dim, STATE0, np.float32)]) for t in range(T)]
    if cfg.opt != "SGD":
        assert m.value_dims[0] > cfg.dim, "the case is meant to see optimizer state columns"
    for bt in g.fill:
        out, st, _ = _forward(m, cfg, bt, monkeypatch)
        _backward(m, st, out)
    assert int(m.size()) == sum(cfg.caps), "the fill did not leave the table full"
    assert _counters_clear(m)
    after = _export(m)
    total_ev = 0
    for j, bt in enumerate(g.steps):
        before = after
        n = bt.keys.size
        P = int(lib().mi355_demb_forward_fused_partitions(n, T, m.table.num_buckets_))
        assert P == M.partitions(n, T, int(spec.tbo[-1]))
        out, st, lazy = _forward(m, cfg, bt, monkeypatch)
        # the path the step took
        assert (P > 0) == (cfg.site != "b") and lazy == (cfg.site != "b"), f"site {cfg.site}: {P} partitions, lazy {lazy}"
        # point 4: the rows of the step's new keys before the backward
        mid = []
        for t in range(T):
            kt = np.unique(bt.keys[bt.tids == t])
            nk = kt[~np.isin(kt, before[t][0])]
            f, r = m.lookup_rows(torch.from_numpy(nk).to(DEV), t)
            mid.append((nk, f.cpu().numpy(), r.float().cpu().numpy()))
        has = None
        if j == len(g.steps) - 1:      # (reading the numbering materialises the step's reverse indices: the last step only)
            nu = int(st.uoff[-1])
            has = (st.slots[:nu][st.rev] >= 0).cpu().numpy()
        _backward(m, st, out)
        after = _export(m)
        rep = M.check_step(before, bt, after, spec, fresh=fresh, mid=mid, update=_updater(m, cfg), over_budget=cfg.over_budget)
        print(f"{name} step {j}: {n} keys, {P} partitions, {rep.evictions} evictions, {rep.case3.size} over-full buckets, "
              f"{rep.refused[1].size} refused")
        total_ev += rep.evictions
        assert rep.evictions >= 1000
        assert cfg.over_budget or (rep.case3.size > 0) == bool(cfg.case3)
        _check_output(cfg, bt, out, before, fresh, rep)
        if has is not None:     # index -1 for exactly the occurrences of refused keys
            refused = set(zip(rep.refused[0].tolist(), rep.refused[1].tolist()))
            want = np.array([(a, b) not in refused for a, b in zip(bt.tids.tolist(), bt.keys.tolist())]) if refused else np.ones(n, bool)
            assert np.array_equal(has, want)
        if cfg.policy == "LRU_LFU":      # the word that is NOT compared: the timer, for every key of the batch
            tk, tw = _timer_words(m)
            assert (tw[np.isin(tk, bt.keys)] == bt.value).all()
        # point 6
        assert int(m.size()) == sum(len(a[0]) for a in after) == sum(cfg.caps)
        for t in range(T):
            assert int(m.size(t)) == len(after[t][0])
        assert _counters_clear(m)
    assert getattr(m, "overflow_reruns", 0) == 0, "a partition list flooded: the case left the regime it is meant for"
