"""The eviction model of tests/evict_model.py on the CPU: (a) its successor state against the oracle's insert, (b) the
conditions the GPU test (tests/test_fused_eviction_gpu.py) relies on, for the very batches it runs, (c) check_step's teeth."""
from types import SimpleNamespace

import numpy as np
import pytest

import evict_model as M
from oracle import oracle as orc


# ---------------------------------------------------------------------------------------------------- (a) against the oracle
def _oracle_state(tab):
    keys, _, scores = tab._view()
    ok = (keys & np.uint64(orc.LOCKED_KEY & orc.RECLAIM_KEY & orc.EMPTY_KEY)) != np.uint64(orc.LOCKED_KEY & orc.RECLAIM_KEY & orc.EMPTY_KEY)
    b = np.repeat(np.arange(tab.num_buckets), tab.C).reshape(keys.shape)
    t = np.searchsorted(tab.tbo, b[ok], side="right") - 1
    return set(zip(t.tolist(), keys[ok].astype(np.int64).tolist(), scores[..., -1][ok].astype(np.int64).tolist()))


def _model_state(s):
    return set(zip(s.tids.tolist(), s.keys.tolist(), s.scores.tolist()))


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("C", [16, 128])
def test_apply_step_agrees_with_the_oracle_insert(C, T):
    """one insert call of the oracle, hits first and then the new keys: its per-call lock scratch is exactly "hit slots are
    locked before any eviction".  LFU with weight sums that never tie (every key carries its own low six digits), tables that
    fill up and evict over six steps, and a last step that sends C + 5 unseen keys into one full bucket (point 3)."""
    caps = [8 * C, 4 * C, 6 * C][:T]
    tab = orc.OracleTable(caps, bucket_capacity=C)
    spec = SimpleNamespace(tbo=tab.tbo, C=C, policy="LFU")
    assert np.array_equal(spec.tbo, M.tbo_of(caps, C))
    rng = np.random.default_rng(10 * C + T)
    state = M.empty_state()
    serial = {}
    saw_case3 = saw_evictions = 0
    for step in range(7):
        ut, uk = [], []
        for t, cap in enumerate(caps):
            k = rng.choice(3 * cap, cap // 2, replace=False).astype(np.int64) + (t << 20)
            ut.append(np.full(k.size, t, np.int64)); uk.append(k)
        if step == 6:     # C + 5 keys nobody has seen, all of one bucket of the last table, besides hits there
            t = T - 1
            cand = np.arange(1 << 30, (1 << 30) + 400 * C * (int(tab.tbo[t + 1] - tab.tbo[t])), dtype=np.int64)
            b = M.bucket_of(cand, np.full(cand.size, t), spec.tbo, C)
            k = cand[b == spec.tbo[t] + 1][: C + 5]
            assert k.size == C + 5
            ut.append(np.full(k.size, t, np.int64)); uk.append(k)
        ut, uk = np.concatenate(ut), np.concatenate(uk)
        res = set(zip(state.tids.tolist(), state.keys.tolist()))
        hit = np.array([(a, b) in res for a, b in zip(ut.tolist(), uk.tolist())])
        order = np.concatenate([np.flatnonzero(hit), np.flatnonzero(~hit)])
        ut, uk, hit = ut[order], uk[order], hit[order]
        w = np.empty(uk.size, np.int64)
        for i, (a, b, h) in enumerate(zip(ut.tolist(), uk.tolist(), hit.tolist())):
            w[i] = 1_000_000 * int(rng.integers(1, 9)) + (0 if h else serial.setdefault((a, b), len(serial) + 1))
        batch = SimpleNamespace(keys=uk, tids=ut, w=w, value=0)
        state, info = M.apply_step(state, batch, spec)
        _, results, _ = tab.insert(uk, ut, score_in=w, policy=orc.POLICY_ACCUMULATE)
        assert _oracle_state(tab) == _model_state(state), f"step {step}"
        busy = set(zip(ut[results == orc.RES_BUSY].tolist(), uk[results == orc.RES_BUSY].tolist()))
        assert busy == set(zip(info.refused[0].tolist(), info.refused[1].tolist()))
        assert int((results == orc.RES_EVICT).sum()) == info.evictions
        saw_case3 += int(info.case3.sum())
        saw_evictions += info.evictions
    assert saw_case3 >= 1 and saw_evictions > 2 * C


def test_vectorised_hash_and_buckets_agree_with_the_oracle():
    rng = np.random.default_rng(0)
    keys = np.concatenate([rng.integers(0, 1 << 47, 2000), np.arange(50)]).astype(np.int64)
    assert M.hash63(keys).tolist() == [orc.hash64(int(k)) for k in keys]
    tab = orc.OracleTable([64, 256, 128], bucket_capacity=16)
    tids = rng.integers(0, 3, keys.size)
    ko, off, inv = tab.bucketize(keys, tids)
    b = M.bucket_of(keys, tids, tab.tbo, 16)
    assert np.array_equal(np.unique(b), np.unique(b[inv][off[:-1]]))
    assert (np.diff(b[inv]) >= 0).all()          # the oracle's order is by bucket: ours sorts the same way


# ---------------------------------------------------------------------------------------------------- (b) the GPU cases' inputs
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_the_batches_of_the_gpu_case_meet_what_its_assertions_rely_on(name):
    g = M.generate(name)
    cfg, spec = g.cfg, g.spec
    T, NB = len(cfg.caps), int(spec.tbo[-1])
    assert all(c % cfg.C == 0 for c in cfg.caps)
    state = M.empty_state()
    other = None           # tied cases: a second replay that breaks every tie the other way
    assert len(g.fill) <= 8
    for i, bt in enumerate(g.fill):
        assert bt.keys.size <= 32 * 1024 and bt.value == M.score_value(cfg, i)
        state, info = M.apply_step(state, bt, spec)
        assert info.evictions == 0 and info.refused[1].size == 0
    assert state.keys.size == sum(cfg.caps), "the fill leaves the table full"
    assert 2 <= len(g.steps) <= 3 or (cfg.over_budget and len(g.steps) == 1)
    seen = set(zip(state.tids.tolist(), state.keys.tolist()))
    case3_steps = 0
    for j, bt in enumerate(g.steps):
        n = bt.keys.size
        P = M.partitions(n, T, NB)
        if cfg.site == "b":
            assert 15_000 <= n < 65_536 and P == 0
        else:
            assert 66_000 <= n <= 70_000 and P > 0
            assert (cfg.pooling == "NONE") == (cfg.site == "lean")
            if cfg.pooling != "NONE":
                assert n <= 8 * (bt.off.size - 1)           # short bags: what the pooled path (c) takes
        assert bt.off[0] == 0 and bt.off[-1] == n and (bt.off.size - 1) % T == 0
        # features are tables: the keys of table t are the bags of feature t
        Bn = (bt.off.size - 1) // T
        assert np.array_equal(bt.tids, np.repeat(np.arange(T), np.diff(bt.off[::Bn])))
        before = set(zip(state.tids.tolist(), state.keys.tolist()))
        ut, uk, cnt, inc = M.unique_batch(bt)
        is_res = np.array([(a, b) in before for a, b in zip(ut.tolist(), uk.tolist())])
        assert not any((a, b) in seen for a, b in zip(ut[~is_res].tolist(), uk[~is_res].tolist())), "a new key was seen before"
        by_occ = cfg.site == "b" or cfg.over_budget
        frac = cnt[is_res].sum() / n if by_occ else is_res.mean()
        assert abs(frac - cfg.res_share) <= 0.05, f"{frac:.2f} of the {'occurrences' if by_occ else 'unique keys'} are resident keys"
        if cfg.tie_free:
            assert bt.w is not None and (bt.w >= 1).all()
        else:
            assert bt.w is None
        if not cfg.tie_free:
            # whatever way the device breaks its ties, the step hits the same keys and evicts as many: the generator draws its
            # hits from keys that score above every cut their bucket has seen
            other, io = M.apply_step(state if other is None else other, bt, spec, tie_break="key_desc")
        state, info = M.apply_step(state, bt, spec, tie_break=None if cfg.tie_free else "key")
        if not cfg.tie_free:
            assert io.hits == info.hits == int(is_res.sum()) and io.evictions == info.evictions
            assert np.array_equal(io.deferred, info.deferred) and np.array_equal(io.case3, info.case3)
            assert sorted(other.scores.tolist()) == sorted(state.scores.tolist())
        seen |= set(zip(ut.tolist(), uk.tolist()))
        assert info.evictions >= 1000, f"step {j}: {info.evictions} evictions"
        assert int((info.n_new >= 2).sum()) >= 50
        if cfg.case3:
            case3_steps += int(info.case3.any())
            assert info.refused[1].size >= 1
        else:
            assert not info.case3.any() and info.refused[1].size == 0
        if P:
            b = np.arange(NB)
            t = np.searchsorted(spec.tbo, b, side="right") - 1
            part = M.partition_of(b, t, spec.tbo, cfg.C, P, np.bincount(bt.tids, minlength=T))
            per = np.bincount(part, weights=info.deferred, minlength=P)
            assert per.max() <= M.K_DEF_MAX // 2, f"a partition gets {int(per.max())} deferred keys"      # (keys: also past the record budget)
            assert part.max() < P
            # the budget is spent per (tile, key) record: bounded by the occurrences of the keys that are not resident
            ub = M.bucket_of(uk[~is_res], ut[~is_res], spec.tbo, cfg.C)
            occ = np.bincount(part[ub], weights=cnt[~is_res], minlength=P)
            assert (cnt[~is_res] > 1).sum() >= 100       # deferred keys with several records are part of the case
            if cfg.over_budget:
                # ... and from below by the distinct (1 024-key tile, key) pairs: no tile of the probe kernel is larger
                ob = M.bucket_of(bt.keys, bt.tids, spec.tbo, cfg.C)
                new_occ = ~np.isin(M._comp(bt.tids, bt.keys), M._comp(ut[is_res], uk[is_res]))
                pairs = np.unique(np.stack([np.arange(n)[new_occ] // 1024, bt.keys[new_occ], part[ob[new_occ]]], axis=1), axis=0)
                recs = np.bincount(pairs[:, 2], minlength=P)
                assert recs.max() > M.K_DEF_MAX + 50, f"no partition is past the budget ({int(recs.max())} deferred records at most)"
                assert int((recs > M.K_DEF_MAX).sum()) >= 3
            else:
                assert occ.max() <= M.K_DEF_MAX // 2, f"a partition gets {int(occ.max())} occurrences of deferred keys"
        assert state.keys.size == sum(cfg.caps)
    if cfg.case3:
        assert case3_steps == len(g.steps)
    assert M.score_value(cfg, 0) != M.score_value(cfg, 1)


def test_every_site_sees_a_tie_free_and_a_tied_configuration():
    for site in ("b", "c", "lean"):
        kinds = {c.tie_free for c in M.CASES.values() if c.site == site}
        assert kinds == {True, False}, site
        assert any(c.opt != "SGD" for c in M.CASES.values() if c.site == site)
    assert any(c.policy == "LRU_LFU" and c.site == "c" for c in M.CASES.values())
    assert any(c.case3 and c.site == "b" for c in M.CASES.values())
    assert {c.policy for c in M.CASES.values()} == set(M.POLICIES)


# ---------------------------------------------------------------------------------------------------- (c) check_step has teeth
V = 12     # columns of the made-up rows: 8 of embedding, 4 of state


def _rows(keys, salt):
    k = np.asarray(keys, np.int64)
    return ((k[:, None] * 31 + np.arange(V)[None, :] * 7 + salt) % 1009).astype(np.float32) / 64.0


def _tables(state, T, salt_of):
    out = []
    for t in range(T):
        s = state.tids == t
        k = state.keys[s]
        out.append((k.copy(), state.scores[s].copy(), salt_of(t, k)))
    return out


def _honest(name="b_3t_lfu_adam"):
    """before / after / mid of the case's first measured step as an honest device would leave them"""
    g = M.generate(name)
    T = len(g.cfg.caps)
    state = M.empty_state()
    for bt in g.fill:
        state, _ = M.apply_step(state, bt, g.spec)
    bt = g.steps[0]
    nxt, info = M.apply_step(state, bt, g.spec)
    fresh = [np.concatenate([np.full(8, 0.25, np.float32), np.full(4, 0.0625, np.float32)]) for _ in range(T)]
    ut, uk, _, _ = M.unique_batch(bt)
    touched = set(zip(ut.tolist(), uk.tolist()))

    def after_rows(t, k):      # untouched keys keep their rows, the batch's keys were updated by the backward
        r = _rows(k, 0)
        upd = np.array([(t, x) in touched for x in k.tolist()])
        r[upd] = _rows(k[upd], 5)
        return r

    before = _tables(state, T, lambda t, k: _rows(k, 0))
    after = _tables(nxt, T, after_rows)
    res = set(zip(state.tids.tolist(), state.keys.tolist()))
    mid = []
    for t in range(T):
        k = np.array([b for a, b in zip(ut.tolist(), uk.tolist()) if a == t and (a, b) not in res], np.int64)
        mid.append((k, np.ones(k.size, bool), np.repeat(fresh[t][None, :], k.size, axis=0)))
    return g, bt, before, after, mid, fresh, state, nxt, info


def test_check_step_passes_an_honest_step():
    g, bt, before, after, mid, fresh, state, nxt, info = _honest()
    rep = M.check_step(before, bt, after, g.spec, fresh=fresh, mid=mid)
    assert rep.evictions == info.evictions >= 1000 and rep.refused[1].size == 0


def _a_cut_bucket(g, state, nxt, info):
    """a bucket that evicted some but not all of its eligible keys -> (victim with the highest score, survivor with the lowest)"""
    gone = ~np.isin(M._comp(state.tids, state.keys), M._comp(nxt.tids, nxt.keys))
    rb = M.bucket_of(state.keys, state.tids, g.spec.tbo, g.spec.C)
    for b in np.flatnonzero(info.deferred > 0):
        i = np.flatnonzero(rb == b)
        v = i[gone[i]]
        s = i[~gone[i]]
        in_next = M._find(M._comp(nxt.tids, nxt.keys), M._comp(state.tids[s], state.keys[s]))
        s = s[nxt.scores[in_next] == state.scores[s]]          # survivors the batch did not hit
        if v.size and s.size:
            return int(v[np.argmax(state.scores[v])]), int(s[np.argmin(state.scores[s])])
    raise AssertionError("no bucket with a cut")


def _swap(after, before, t, drop_key, add_from_before_key=None):
    k, s, r = after[t]
    keep = k != drop_key
    k, s, r = k[keep], s[keep], (r[keep] if r is not None else None)
    if add_from_before_key is not None:
        bk, bs, br = before[t]
        j = np.flatnonzero(bk == add_from_before_key)
        k, s, r = np.concatenate([k, bk[j]]), np.concatenate([s, bs[j]]), (np.concatenate([r, br[j]]) if r is not None else None)
    out = list(after)
    out[t] = (k, s, r)
    return out


def test_check_step_refuses_a_victim_swapped_for_the_next_lowest_survivor():
    g, bt, before, after, mid, fresh, state, nxt, info = _honest()
    v, s = _a_cut_bucket(g, state, nxt, info)
    t = int(state.tids[v])
    assert int(state.tids[s]) == t and state.scores[v] < state.scores[s]
    bad = _swap(after, before, t, int(state.keys[s]), int(state.keys[v]))     # the second-lowest left, the lowest stayed
    with pytest.raises(AssertionError, match="a victim scored"):
        M.check_step(before, bt, bad, g.spec, fresh=fresh, mid=mid)


def test_check_step_refuses_a_stale_state_column_in_a_new_row():
    g, bt, before, after, mid, fresh, state, nxt, info = _honest()
    t = 1
    k, f, r = mid[t]
    r = r.copy()
    r[3, 9] = before[t][2][0, 9]          # the victim's optimizer state, left in the new key's row
    assert r[3, 9] != fresh[t][9]
    bad = list(mid)
    bad[t] = (k, f, r)
    with pytest.raises(AssertionError, match="not the fresh row"):
        M.check_step(before, bt, after, g.spec, fresh=fresh, mid=bad)
    r = mid[t][2].copy()
    r[5, 2] = np.float32(0.25) + np.float32(2.0 ** -22)      # one bit pattern off in the embedding part
    bad[t] = (k, f, r)
    with pytest.raises(AssertionError, match="not the fresh row"):
        M.check_step(before, bt, after, g.spec, fresh=fresh, mid=bad)


def test_check_step_refuses_a_refused_key_although_a_victim_existed():
    g, bt, before, after, mid, fresh, state, nxt, info = _honest()
    v, _ = _a_cut_bucket(g, state, nxt, info)
    t = int(state.tids[v])
    b = M.bucket_of(state.keys[v:v + 1], state.tids[v:v + 1], g.spec.tbo, g.spec.C)[0]
    nk = mid[t][0]
    nk = nk[M.bucket_of(nk, np.full(nk.size, t), g.spec.tbo, g.spec.C) == b]
    bad = _swap(after, before, t, int(nk[0]), int(state.keys[v]))     # the victim kept its slot, the new key went without
    with pytest.raises(AssertionError, match="got no slot although"):
        M.check_step(before, bt, bad, g.spec)


def test_check_step_past_the_eviction_budget_allows_a_refusal_but_no_eviction_without_a_placement():
    g, bt, before, after, mid, fresh, state, nxt, info = _honest()
    v, _ = _a_cut_bucket(g, state, nxt, info)
    t = int(state.tids[v])
    b = M.bucket_of(state.keys[v:v + 1], state.tids[v:v + 1], g.spec.tbo, g.spec.C)[0]
    nk = mid[t][0]
    nk = nk[M.bucket_of(nk, np.full(nk.size, t), g.spec.tbo, g.spec.C) == b]
    M.check_step(before, bt, after, g.spec, over_budget=True)
    M.check_step(before, bt, _swap(after, before, t, int(nk[0]), int(state.keys[v])), g.spec, over_budget=True)
    with pytest.raises(AssertionError, match="resident key.s. left for"):
        M.check_step(before, bt, _swap(after, before, t, int(nk[0])), g.spec, over_budget=True)      # a victim left for nobody


def test_check_step_refuses_an_evicted_hit_a_changed_bystander_and_a_wrong_score():
    g, bt, before, after, mid, fresh, state, nxt, info = _honest()
    ut, uk, _, _ = M.unique_batch(bt)
    res = set(zip(state.tids.tolist(), state.keys.tolist()))
    t, hk = next((a, b) for a, b in zip(ut.tolist(), uk.tolist()) if (a, b) in res)
    with pytest.raises(AssertionError, match="hit by the batch and is gone"):
        M.check_step(before, bt, _swap(after, before, t, hk), g.spec)
    # a key outside the batch whose row changed in one bit / whose score moved
    touched = set(zip(ut.tolist(), uk.tolist()))
    k, s, r = after[0]
    i = next(i for i, x in enumerate(k.tolist()) if (0, x) not in touched)
    r2 = r.copy(); r2[i, 11] = np.nextafter(r2[i, 11], np.float32(9))
    with pytest.raises(AssertionError, match="its row changed"):
        M.check_step(before, bt, [(k, s, r2)] + after[1:], g.spec)
    s2 = s.copy(); s2[i] += 1
    with pytest.raises(AssertionError, match="its score went"):
        M.check_step(before, bt, [(k, s2, r)] + after[1:], g.spec)
    j = next(i for i, x in enumerate(k.tolist()) if (0, x) in res and (0, x) in touched)
    s3 = s.copy(); s3[j] += 1
    with pytest.raises(AssertionError, match="the policy gives"):
        M.check_step(before, bt, [(k, s3, r)] + after[1:], g.spec)


def test_check_step_is_tie_tolerant_and_counts_case_three():
    """a STEP case: any choice among equal scores on the cut passes; in an over-full bucket exactly e - |E| keys go without"""
    g = M.generate("b_c16_step_case3")
    state = M.empty_state()
    for bt in g.fill:
        state, _ = M.apply_step(state, bt, g.spec)
    bt = g.steps[0]
    with pytest.raises(ValueError, match="a tie sits on the cut"):
        M.apply_step(state, bt, g.spec)
    nxt, info = M.apply_step(state, bt, g.spec, tie_break="key")
    before, after = _tables(state, 1, lambda t, k: None), _tables(nxt, 1, lambda t, k: None)
    rep = M.check_step(before, bt, after, g.spec)
    assert rep.case3.size == g.cfg.case3 and rep.refused[1].size == info.refused[1].size >= g.cfg.case3
    # the other choice on a tied cut: the victim with the highest score back, an equal-scoring survivor out
    gone = ~np.isin(state.keys, nxt.keys)
    rb = M.bucket_of(state.keys, state.tids, g.spec.tbo, g.spec.C)
    ut, uk, _, _ = M.unique_batch(bt)
    done = False
    for b in np.flatnonzero((info.deferred > 0) & ~info.case3):
        i = np.flatnonzero(rb == b)
        v, s = i[gone[i]], i[~gone[i] & ~np.isin(state.keys[i], uk)]
        tie = s[state.scores[s] == state.scores[v].max()] if v.size else s[:0]
        if tie.size:
            other = _swap(after, before, 0, int(state.keys[tie[0]]), int(state.keys[v[np.argmax(state.scores[v])]]))
            M.check_step(before, bt, other, g.spec)
            done = True
            break
    assert done, "no tied cut in the case"
    # one refused key too many in a case-3 bucket
    rk = rep.placed[1][np.isin(M.bucket_of(rep.placed[1], rep.placed[0], g.spec.tbo, g.spec.C), rep.case3)]
    with pytest.raises(AssertionError, match="the rule refuses"):
        M.check_step(before, bt, _swap(after, before, 0, int(rk[0])), g.spec)
