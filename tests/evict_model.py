"""CPU model of WHICH keys one training forward of the scored hash table evicts -- test infrastructure in plain numpy for
tests/test_evict_model_cpu.py and tests/test_fused_eviction_gpu.py (the three hand-written copies of the eviction in the
fused index stage: evict_phase of fused_mid_kernel, part_evict under fused_part3_kernel and under part3_lean.h).

The rule, per bucket b of one step (buckets as `locate` of oracle/demb_oracle.c: tbo[t] + (hash63(key) % (nb_t C)) / C):
R the resident keys with their scores, K the unique batch keys of the bucket, H = K & R, N = K \\ R, free = C - |R|,
E = R \\ H the eligible keys, e = max(0, |N| - free).  After the step
  1. every key of H is there, with the policy's update of its score;
  2. e <= |E|: every key of N has a slot and exactly e keys V of E are gone, max score(V) <= min score(E \\ V) (ties may sit
     on the cut: any choice among them is right; the compared word of a multi-word score is the LAST one, reduce_min);
  3. e > |E|: all of E is gone and exactly e - |E| keys of N have no slot (which: free);
  4. a new key's row is the initialiser's embedding followed by the state's initial value, never the victim's;
  5. every key of R \\ (H | V) keeps key, row and score bit for bit;
  6. the table holds exactly what the buckets hold.
Path (c) spends an eviction budget: a partition block evicts for at most kDefMax deferred (tile, key) records per step.  Past
it (check_step(over_budget=True)) a new key may go without a slot although a victim exists -- but as a whole: a key that has a
slot has it for every occurrence (full score, full update, its row in every output), a key without has none (zeros, no update),
and a bucket evicts exactly as many keys as it places beyond its free slots, lowest scores first.

Out of scope here: pinned slots (the counter array, cache rows of an external store), the prefetch pipeline's `protect` bound,
reclaimed (erased) slots, the overflow arena and the flooded-partition re-run (tests/test_path_c_oracle_gpu.py covers that one).

`check_step` judges a device step from table exports (tie-tolerant); `apply_step` is the deterministic successor state, used on
the CPU only (against oracle.OracleTable.insert, and to replay the generators); `generate` draws the fill and the measured
batches of every GPU case, so that the CPU test vets exactly the batches the GPU test runs."""
import functools
from types import SimpleNamespace

import numpy as np

_U = np.uint64
KEY_BITS = 48          # keys of the model are below 2^48: (table, key) packs into one int64


# ---------------------------------------------------------------------------------------------------- hash and buckets
def fmix64(k):
    k = np.ascontiguousarray(k).astype(np.uint64)
    k ^= k >> _U(33); k *= _U(0xFF51AFD7ED558CCD)
    k ^= k >> _U(33); k *= _U(0xC4CEB9FE1A85EC53)
    k ^= k >> _U(33)
    return k


def hash63(keys):
    """orc_hash: fmix64(key) & INT64_MAX"""
    return fmix64(np.asarray(keys).astype(np.int64).view(np.uint64)) & _U(0x7FFFFFFFFFFFFFFF)


def tbo_of(caps, C):
    """bucket offsets of the logical tables (scored_hashtable: ceil(capacity / C) buckets each)"""
    return np.concatenate([[0], np.cumsum([(c + C - 1) // C for c in caps])]).astype(np.int64)


def bucket_of(keys, table_ids, tbo, C):
    """global bucket of every (key, table): tbo[t] + (hash63(key) % (nb_t * C)) // C"""
    t = np.asarray(table_ids, np.int64)
    tbo = np.asarray(tbo, np.int64)
    cap = ((tbo[t + 1] - tbo[t]) * C).astype(np.uint64)
    return tbo[t] + ((hash63(keys) % cap) // _U(C)).astype(np.int64)


def partition_of(buckets, table_ids, tbo, C, P, keys_per_table):
    """slot-range partition of path (c) for every bucket.  One table: (bucket * C) // spp with spp = ceil(ceil((S + 1) / P) / C) * C.
    Several tables: table t owns 1 + (P - T) * n_t // n partitions (n_t: its keys in the batch), which split its buckets evenly."""
    b = np.asarray(buckets, np.int64)
    tbo = np.asarray(tbo, np.int64)
    T = tbo.size - 1
    if T == 1:
        S = int(tbo[-1]) * C
        spp = -(-((S + 1 + P - 1) // P) // C) * C
        return (b * C) // spp
    n_t = np.asarray(keys_per_table, np.int64)
    pt = 1 + (P - T) * n_t // max(int(n_t.sum()), 1)
    pb = np.concatenate([[0], np.cumsum(pt)])
    t = np.asarray(table_ids, np.int64)
    psc = (pt.astype(np.uint64) << _U(32)) // (tbo[1:] - tbo[:-1]).astype(np.uint64)
    x = (((b - tbo[t]).astype(np.uint64) * psc[t]) >> _U(32)).astype(np.int64)
    return pb[t] + np.minimum(x, pt[t] - 1)


def _comp(tids, keys):
    keys = np.asarray(keys, np.int64)
    assert keys.size == 0 or (int(keys.min()) >= 0 and int(keys.max()) < (1 << KEY_BITS)), "model keys are in [0, 2^48)"
    return (np.asarray(tids, np.int64) << KEY_BITS) | keys


# ---------------------------------------------------------------------------------------------------- score policies
POLICIES = ("STEP", "CUSTOMIZED", "TIMESTAMP", "LFU", "LRU_LFU")


def hit_score(policy, old, inc, value):
    """the compared score word of a key the step found (LRU_LFU: the frequency word)"""
    return old + inc if policy in ("LFU", "LRU_LFU") else np.full_like(old, value)


def new_score(policy, inc, value):
    return inc.copy() if policy in ("LFU", "LRU_LFU") else np.full_like(inc, value)


def unique_batch(batch):
    """unique (table, key) of a batch in order of first occurrence -> (tids, keys, occurrences, inc) with inc = what a counting
    policy adds: the weight sum, or the occurrences"""
    c = _comp(batch.tids, batch.keys)
    u, first, inv, cnt = np.unique(c, return_index=True, return_inverse=True, return_counts=True)
    inc = np.bincount(inv, weights=None if batch.w is None else batch.w.astype(np.float64), minlength=u.size)
    order = np.argsort(first, kind="stable")
    u, cnt, inc = u[order], cnt[order], np.rint(inc[order]).astype(np.int64)
    return u >> KEY_BITS, u & ((1 << KEY_BITS) - 1), cnt.astype(np.int64), inc


# ---------------------------------------------------------------------------------------------------- successor state
def empty_state():
    z = np.zeros(0, np.int64)
    return SimpleNamespace(tids=z, keys=z, scores=z)


def apply_step(state, batch, spec, tie_break=None):
    """-> (state after the step, info).  state: tids / keys / scores (compared word) of every resident key; spec: tbo, C, policy.
    A tie between a victim and a survivor raises unless tie_break is "key" (the lower key goes first) or "key_desc".  Of the keys a
    bucket refuses (point 3) the model refuses the LAST ones in batch order, as one insert call of the oracle does.
    info: evictions, refused (tids, keys), per global bucket: new keys `n_new`, deferred keys `deferred` (= e), `cut` (highest
    victim score, -1: none), `case3` (bool)."""
    tbo, C, pol = np.asarray(spec.tbo, np.int64), spec.C, spec.policy
    NB = int(tbo[-1])
    ut, uk, _cnt, inc = unique_batch(batch)
    uc, sc = _comp(ut, uk), _comp(state.tids, state.keys)
    order = np.argsort(sc)
    pos = np.searchsorted(sc[order], uc)
    pos = order[np.minimum(pos, max(sc.size - 1, 0))] if sc.size else np.zeros(uc.size, np.int64)
    hit = sc[pos] == uc if sc.size else np.zeros(uc.size, bool)
    scores = state.scores.copy()
    is_hit_res = np.zeros(sc.size, bool)
    is_hit_res[pos[hit]] = True
    scores[pos[hit]] = hit_score(pol, scores[pos[hit]], inc[hit], batch.value)
    rb = bucket_of(state.keys, state.tids, tbo, C)
    ub = bucket_of(uk, ut, tbo, C)
    nR = np.bincount(rb, minlength=NB)
    assert int(nR.max(initial=0)) <= C, "the state holds more keys in a bucket than it has slots"
    nN = np.bincount(ub[~hit], minlength=NB)
    e = np.maximum(0, nN - (C - nR))
    gone = np.zeros(sc.size, bool)
    placed = ~hit
    cut = np.full(NB, -1, np.int64)
    case3 = np.zeros(NB, bool)
    res_by_bucket = np.argsort(rb, kind="stable")
    r0 = np.concatenate([[0], np.cumsum(nR)])
    new_idx = np.flatnonzero(~hit)
    new_by_bucket = new_idx[np.argsort(ub[new_idx], kind="stable")]      # (stable: batch order inside a bucket)
    n0 = np.concatenate([[0], np.cumsum(nN)])
    for b in np.flatnonzero(e > 0):
        idx = res_by_bucket[r0[b]: r0[b + 1]]
        el = idx[~is_hit_res[idx]]
        if tie_break in ("key", "key_desc"):
            el = el[np.lexsort((state.keys[el] if tie_break == "key" else -state.keys[el], scores[el]))]
        else:
            el = el[np.argsort(scores[el], kind="stable")]
        k = int(e[b])
        if k > el.size:
            case3[b] = True
            gone[el] = True
            placed[new_by_bucket[n0[b]: n0[b + 1]][nN[b] - (k - el.size):]] = False
            if el.size:
                cut[b] = scores[el[-1]]
            continue
        if k < el.size and scores[el[k - 1]] == scores[el[k]] and tie_break is None:
            raise ValueError(f"bucket {b}: a tie sits on the cut (score {int(scores[el[k]])}, {k} of {el.size} eligible keys leave)")
        gone[el[:k]] = True
        cut[b] = scores[el[k - 1]]
    keep = ~gone
    new = placed & ~hit
    out = SimpleNamespace(tids=np.concatenate([state.tids[keep], ut[new]]), keys=np.concatenate([state.keys[keep], uk[new]]),
                          scores=np.concatenate([scores[keep], new_score(pol, inc[new], batch.value)]))
    refused = ~placed & ~hit
    info = SimpleNamespace(evictions=int(gone.sum()), refused=(ut[refused], uk[refused]), n_new=nN, deferred=e, cut=cut, case3=case3,
                           hits=int(hit.sum()))
    return out, info


# ---------------------------------------------------------------------------------------------------- judging a device step
def _snap(tables):
    """per-table (keys, scores, rows) -> flat arrays (rows: list per table, index into it)"""
    tids = np.concatenate([np.full(len(k), t, np.int64) for t, (k, _, _) in enumerate(tables)]) if tables else np.zeros(0, np.int64)
    keys = np.concatenate([np.asarray(k, np.int64) for k, _, _ in tables]) if tables else np.zeros(0, np.int64)
    scores = np.concatenate([np.asarray(s, np.int64) for _, s, _ in tables]) if tables else np.zeros(0, np.int64)
    local = np.concatenate([np.arange(len(k), dtype=np.int64) for k, _, _ in tables]) if tables else np.zeros(0, np.int64)
    return SimpleNamespace(tids=tids, keys=keys, scores=scores, local=local, comp=_comp(tids, keys), rows=[r for _, _, r in tables])


def _find(hay_comp, needles):
    """index of every needle in hay (or -1)"""
    if hay_comp.size == 0:
        return np.full(needles.size, -1, np.int64)
    order = np.argsort(hay_comp)
    p = np.minimum(np.searchsorted(hay_comp[order], needles), hay_comp.size - 1)
    idx = order[p]
    return np.where(hay_comp[idx] == needles, idx, -1)


def _rows_of(snap, idx):
    """rows of flat entries idx (all of one table) as uint32 bit patterns"""
    t = int(snap.tids[idx[0]])
    return np.ascontiguousarray(np.asarray(snap.rows[t])[snap.local[idx]], dtype=np.float32).view(np.uint32)


def check_step(before, batch, after, spec, fresh=None, mid=None, update=None, over_budget=False):
    """Points 1-6 of the module docstring for one training step.  before / after: per table (keys, scores, rows) -- the
    compared score word; rows may be None (then no row is compared).  spec: tbo, C, policy.  fresh: per table the row of a
    new key (embedding initialiser, then the state's initial value).  mid: per table (keys, found, rows) of the step's NEW keys
    read between the forward and the backward (point 4, bit for bit).  update(t, rows, occurrences) -> (rows the backward
    should leave, absolute tolerance per element): applied to the old rows of hits and the fresh rows of new keys.
    over_budget: the step may have run past path (c)'s eviction budget (module docstring): refusals are not held to the rule.
    Raises AssertionError naming the first offending bucket; returns SimpleNamespace(refused=(tids, keys), evictions, case3
    buckets, placed=(tids, keys))."""
    tbo, C, pol = np.asarray(spec.tbo, np.int64), spec.C, spec.policy
    NB = int(tbo[-1])
    B, A = _snap(before), _snap(after)
    ut, uk, cnt, inc = unique_batch(batch)
    uc = _comp(ut, uk)
    bB, bA, bU = bucket_of(B.keys, B.tids, tbo, C), bucket_of(A.keys, A.tids, tbo, C), bucket_of(uk, ut, tbo, C)

    def fail(b, what):
        rb, ra, ru = np.flatnonzero(bB == b), np.flatnonzero(bA == b), np.flatnonzero(bU == b)
        t = int(np.searchsorted(tbo, b, side="right") - 1)
        in_after = _find(A.comp, B.comp[rb]) >= 0
        in_batch = _find(uc, B.comp[rb]) >= 0
        o = np.argsort(B.scores[rb], kind="stable")
        res = [f"{int(B.keys[i])}:{int(B.scores[i])}{'h' if h else ''}{'' if a else ' GONE'}"
               for i, h, a in zip(rb[o], in_batch[o], in_after[o])]
        new = [f"{int(uk[i])}{'' if a else ' REFUSED'}" for i, a in zip(ru, _find(A.comp, uc[ru]) >= 0) if _find(B.comp, uc[i:i + 1])[0] < 0]
        raise AssertionError(f"bucket {b} (table {t}, local bucket {b - int(tbo[t])}, C = {C}, policy {pol}): {what}\n"
                             f"  residents before, by score (key:score, h = hit by the batch): {res}\n"
                             f"  new keys of the batch: {new}\n"
                             f"  keys after: {len(ra)}, scores after: {sorted(int(x) for x in A.scores[ra])}")

    # point 6 (and sanity): no duplicate, nothing foreign, no bucket over capacity
    s = np.sort(A.comp)
    if s.size > 1 and (s[1:] == s[:-1]).any():
        d = int(np.flatnonzero(s[1:] == s[:-1])[0])
        fail(int(bA[np.flatnonzero(A.comp == s[d])[0]]), f"key {int(s[d] & ((1 << KEY_BITS) - 1))} is stored twice")
    a_in_b, a_in_u = _find(B.comp, A.comp), _find(uc, A.comp)
    foreign = (a_in_b < 0) & (a_in_u < 0)
    if foreign.any():
        i = int(np.flatnonzero(foreign)[0])
        fail(int(bA[i]), f"key {int(A.keys[i])} is in the table but was neither resident nor in the batch")
    nA = np.bincount(bA, minlength=NB)
    if (nA > C).any():
        fail(int(np.flatnonzero(nA > C)[0]), "more keys than slots")
    # point 1: hits stay, with the policy's score
    u_in_b, u_in_a = _find(B.comp, uc), _find(A.comp, uc)
    hit = u_in_b >= 0
    lost = hit & (u_in_a < 0)
    if lost.any():
        i = int(np.flatnonzero(lost)[0])
        fail(int(bU[i]), f"key {int(uk[i])} was hit by the batch and is gone")
    want = hit_score(pol, B.scores[u_in_b[hit]], inc[hit], batch.value)
    bad = A.scores[u_in_a[hit]] != want
    if bad.any():
        i = int(np.flatnonzero(hit)[np.flatnonzero(bad)[0]])
        fail(int(bU[i]), f"hit key {int(uk[i])}: score {int(A.scores[u_in_a[i]])} after, the policy gives {int(want[np.flatnonzero(bad)[0]])} "
                         f"(before {int(B.scores[u_in_b[i]])}, inc {int(inc[i])}, value {batch.value})")
    # new keys: placed or refused, with the policy's score
    new = ~hit
    placed, refused = new & (u_in_a >= 0), new & (u_in_a < 0)
    want = new_score(pol, inc[placed], batch.value)
    bad = A.scores[u_in_a[placed]] != want
    if bad.any():
        i = int(np.flatnonzero(placed)[np.flatnonzero(bad)[0]])
        fail(int(bU[i]), f"new key {int(uk[i])}: score {int(A.scores[u_in_a[i]])}, the policy gives {int(want[np.flatnonzero(bad)[0]])}")
    # points 2 and 3: how many leave, and which
    b_in_a = _find(A.comp, B.comp)
    gone = b_in_a < 0
    res_hit = _find(uc, B.comp) >= 0
    nR, nH = np.bincount(bB, minlength=NB), np.bincount(bB[res_hit], minlength=NB)
    nN, nRef = np.bincount(bU[new], minlength=NB), np.bincount(bU[refused], minlength=NB)
    nG = np.bincount(bB[gone], minlength=NB)
    nE = nR - nH
    e = np.maximum(0, nN - (C - nR))
    c3 = e > nE
    if over_budget:      # refusals are the device's choice: a bucket evicts for what it placed beyond its free slots, no more
        placed_e = np.maximum(0, nN - nRef - (C - nR))
        bad = (nG != placed_e) | (nRef < e - nE)
        if bad.any():
            b = int(np.flatnonzero(bad)[0])
            fail(b, f"{int(nG[b])} resident key(s) left for {int(nN[b] - nRef[b])} new key(s) placed with {int(C - nR[b])} free slot(s) "
                    f"({int(nRef[b])} refused, e = {int(e[b])}, eligible {int(nE[b])})")
    bad = ~c3 & (nRef > 0) & (not over_budget)
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        fail(b, f"{int(nRef[b])} new key(s) got no slot although {int(nE[b])} eligible key(s) could make room for e = {int(e[b])}")
    bad = (nG != np.where(c3, nE, e)) & (not over_budget)
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        fail(b, f"{int(nG[b])} resident key(s) left, the rule evicts {int(np.where(c3, nE, e)[b])} (e = {int(e[b])}, eligible {int(nE[b])})")
    bad = c3 & (nRef != e - nE) & (not over_budget)
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        fail(b, f"{int(nRef[b])} new key(s) refused, the rule refuses e - |E| = {int(e[b] - nE[b])}")
    big = np.iinfo(np.int64).max
    vmax = np.full(NB, -1, np.int64)
    np.maximum.at(vmax, bB[gone], B.scores[gone])
    stay = ~gone & ~res_hit
    smin = np.full(NB, big, np.int64)
    np.minimum.at(smin, bB[stay], B.scores[stay])
    bad = vmax > smin
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        fail(b, f"a victim scored {int(vmax[b])} while an eligible key scoring {int(smin[b])} stayed")
    # point 5: survivors keep score and row bit for bit
    si = np.flatnonzero(stay)
    bad = A.scores[b_in_a[si]] != B.scores[si]
    if bad.any():
        i = int(si[np.flatnonzero(bad)[0]])
        fail(int(bB[i]), f"key {int(B.keys[i])} was not in the batch and its score went {int(B.scores[i])} -> {int(A.scores[b_in_a[i]])}")
    have_rows = all(r is not None for r in B.rows) and all(r is not None for r in A.rows)
    T = tbo.size - 1
    if have_rows:
        for t in range(T):
            st = si[B.tids[si] == t]
            if st.size == 0:
                continue
            ne = (_rows_of(B, st) != _rows_of(A, b_in_a[st])).any(axis=1)
            if ne.any():
                i = int(st[np.flatnonzero(ne)[0]])
                fail(int(bB[i]), f"key {int(B.keys[i])} was not in the batch and its row changed")
    # point 4: fresh rows between forward and backward
    if mid is not None:
        for t in range(T):
            mk, mf, mr = mid[t]
            mk = np.asarray(mk, np.int64)
            if mk.size == 0:
                continue
            mc = _comp(np.full(mk.size, t), mk)
            j = _find(uc, mc)
            assert (j >= 0).all() and new[j].all(), "mid: not new keys of this step"
            if (np.asarray(mf, bool) != placed[j]).any():
                i = int(j[np.flatnonzero(np.asarray(mf, bool) != placed[j])[0]])
                fail(int(bU[i]), f"new key {int(uk[i])} is {'in' if placed[i] else 'not in'} the table after the step but the lookup before the backward said otherwise")
            ok = np.asarray(mf, bool)
            got = np.ascontiguousarray(np.asarray(mr)[ok], dtype=np.float32).view(np.uint32)
            wantr = np.ascontiguousarray(fresh[t], dtype=np.float32).view(np.uint32)
            ne = (got != wantr[None, :]).any(axis=1)
            if ne.any():
                r = int(np.flatnonzero(ne)[0])
                i = int(j[np.flatnonzero(ok)[r]])
                col = int(np.flatnonzero(got[r] != wantr)[0])
                fail(int(bU[i]), f"new key {int(uk[i])}: its row before the backward is not the fresh row (column {col}: "
                                 f"{float(got[r].view(np.float32)[col])!r}, fresh {float(np.float32(fresh[t][col]))!r})")
    # the backward: the optimizer's update of the old row (hits) / of the fresh row (new keys)
    if update is not None and have_rows:
        for t in range(T):
            for sel, what in ((hit & (ut == t), "hit"), (placed & (ut == t), "new")):
                ii = np.flatnonzero(sel)
                if ii.size == 0:
                    continue
                if what == "hit":
                    old = np.asarray(B.rows[t], np.float32)[B.local[u_in_b[ii]]]
                else:
                    old = np.repeat(np.asarray(fresh[t], np.float32)[None, :], ii.size, axis=0)
                exp, tol = update(t, old.copy(), cnt[ii])
                got = np.asarray(A.rows[t], np.float32)[A.local[u_in_a[ii]]]
                err = np.abs(got.astype(np.float64) - exp.astype(np.float64))
                ne = (err > tol).any(axis=1)
                if ne.any():
                    r = int(np.flatnonzero(ne)[0])
                    col = int(np.argmax(err[r] - tol[r] if np.ndim(tol) == 2 else err[r]))
                    fail(int(bU[ii[r]]), f"{what} key {int(uk[ii[r]])} ({int(cnt[ii[r]])} occurrences): row after the backward differs from the "
                                         f"optimizer's update of its {'old' if what == 'hit' else 'fresh'} row (column {col}: {float(got[r, col])!r}, "
                                         f"expected {float(exp[r, col])!r}, |err| {err[r, col]:.3e})")
    return SimpleNamespace(refused=(ut[refused], uk[refused]), placed=(ut[placed], uk[placed]), hits=(ut[hit], uk[hit]),
                           evictions=int(gone.sum()), case3=np.flatnonzero(c3), e=e, n_new=nN)


# ---------------------------------------------------------------------------------------------------- the GPU cases
# site: "b" evict_phase (batches below 65 536 keys), "c" part_evict under fused_part3_kernel (pooled, from 65 536 keys), "lean"
# part_evict under part3_lean.h (sequence lookups, from 65 536 tokens).  new / hits: unique new keys / hit keys per bucket and
# measured step (inclusive ranges).  Tie-free: LFU and LRU_LFU (distinct weight sums inside every bucket); STEP, CUSTOMIZED and
# TIMESTAMP tie inside a fill generation.
def _case(site, C, caps, policy, pooling, opt, n_occ, new, hits, case3=0, steps=2, seed=0, over_budget=False, res_share=0.6):
    return SimpleNamespace(site=site, C=C, caps=tuple(caps), policy=policy, pooling=pooling, opt=opt, n_occ=n_occ, new=new, hits=hits,
                           case3=case3, steps=steps, seed=seed, gens=4, dim=8, tie_free=policy in ("LFU", "LRU_LFU"),
                           over_budget=over_budget, res_share=res_share)


CASES = {
    "b_c16_lfu_adam":         _case("b", 16, [2048], "LFU", "NONE", "ADAM", 20_000, (8, 9), (5, 7), seed=1),
    "b_c16_step_case3":       _case("b", 16, [2048], "STEP", "SUM", "SGD", 20_000, (8, 9), (5, 7), case3=5, steps=3, seed=2),
    "b_c128_custom_adagrad":  _case("b", 128, [8192], "CUSTOMIZED", "NONE", "EXACT_ROWWISE_ADAGRAD", 20_000, (16, 24), (30, 60), seed=3),
    "b_3t_timestamp":         _case("b", 16, [1024, 2048, 4096], "TIMESTAMP", "SUM", "SGD", 20_000, (3, 4), (4, 9), seed=4),
    "b_3t_lfu_adam":          _case("b", 16, [1024, 2048, 4096], "LFU", "SUM", "ADAM", 20_000, (3, 4), (4, 9), steps=3, seed=5),
    "c_c16_lfu_adam":         _case("c", 16, [16384], "LFU", "SUM", "ADAM", 68_000, (1, 3), (2, 4), seed=6),
    "c_c16_step":             _case("c", 16, [16384], "STEP", "SUM", "SGD", 68_000, (1, 3), (2, 4), steps=3, seed=7),
    "c_c128_lrulfu_adagrad":  _case("c", 128, [131072], "LRU_LFU", "SUM", "EXACT_ROWWISE_ADAGRAD", 68_000, (2, 8), (5, 10), seed=8),
    "c_c128_timestamp":       _case("c", 128, [131072], "TIMESTAMP", "SUM", "SGD", 68_000, (2, 8), (5, 10), seed=9),
    "c_2t_custom_adam":       _case("c", 16, [16384, 16384], "CUSTOMIZED", "SUM", "ADAM", 68_000, (1, 2), (2, 3), seed=10),
    "c_2t_lfu":               _case("c", 16, [16384, 16384], "LFU", "SUM", "SGD", 68_000, (1, 2), (2, 3), seed=11),
    "lean_c128_lfu_adam":     _case("lean", 128, [131072], "LFU", "NONE", "ADAM", 68_000, (2, 8), (5, 10), seed=12),
    "lean_c128_step":         _case("lean", 128, [131072], "STEP", "NONE", "SGD", 68_000, (2, 8), (5, 10), steps=3, seed=13),
    # past the eviction budget: new keys are 65 % of the occurrences, each in several tiles -- partitions meet more than kDefMax
    # deferred records in the one measured step (one: which keys go without is the device's choice, the model cannot follow it)
    "c_c16_step_budget":      _case("c", 16, [16384], "STEP", "SUM", "SGD", 68_000, (1, 3), (4, 10), steps=1, seed=14, over_budget=True, res_share=0.35),
    "lean_c128_lfu_budget":   _case("lean", 128, [131072], "LFU", "NONE", "ADAM", 68_000, (2, 10), (10, 30), steps=1, seed=15, over_budget=True, res_share=0.35),
}
# A partition block evicts for at most kDefMax deferred RECORDS per step (csrc/fused_fwd.hip: a record is a (tile, key) pair of the
# probe kernel; a key that no tile found a slot for has one record per tile it occurs in, at most one per occurrence).  A record
# beyond the budget gets no eviction of its own: it joins the slot another record of its key took in this step, or the key goes
# without a row, like an insert that returns Busy.  The cases stay at half the budget, counted in deferred OCCURRENCES (an upper
# bound of the records whatever the probe kernel's tile shape); the two over-budget cases are held to the whole-key rule only.
K_DEF_MAX = 512


def score_value(cfg, idx):
    """the step's score for the assigning policies (idx: 0 .. gens - 1 the fill, then the measured steps).  STEP: the module's
    step counter.  CUSTOMIZED: set_score values that do NOT follow insertion order.  TIMESTAMP: timer overrides whose low 32 bits
    run against the whole word.  LFU: unused; LRU_LFU: the timer word (not compared)."""
    if cfg.policy == "STEP":
        return idx
    if cfg.policy == "CUSTOMIZED":
        return [40, 10, 30, 20][idx] if idx < cfg.gens else 50 + 10 * (idx - cfg.gens)
    if cfg.policy == "TIMESTAMP":
        order = [2, 0, 3, 1][idx] if idx < cfg.gens else idx
        return ((order + 1) << 33) + 1000 - order
    return 7_000_000 + idx


def _lay_out(cfg, rng, ut, uk, cnt, wsum):
    """occurrences of the unique keys (cnt each) as a feature-major batch: offsets, per-occurrence table ids and weights"""
    T = len(cfg.caps)
    keys, tids, w = [], [], []
    for t in range(T):
        sel = np.flatnonzero(ut == t)
        occ = np.repeat(sel, cnt[sel])
        rng.shuffle(occ)
        keys.append(uk[occ]); tids.append(np.full(occ.size, t, np.int64))
        if wsum is not None:
            # every occurrence weighs 1000 but the first of its key, which carries the rest of the key's sum
            first = np.zeros(occ.size, bool)
            first[np.unique(occ, return_index=True)[1]] = True
            w.append(np.where(first, wsum[occ] - 1000 * (cnt[occ] - 1), 1000).astype(np.int64))
    n_t = np.array([k.size for k in keys])
    if cfg.pooling == "NONE":
        assert T == 1
        off = np.arange(n_t[0] + 1, dtype=np.int64)
    else:
        Bn = max(int(n_t.sum()) // (4 * T), 1)      # ~4 keys per bag: path (c) wants n <= 8 bags
        lens = np.concatenate([rng.multinomial(int(n), np.full(Bn, 1.0 / Bn)) for n in n_t])
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return SimpleNamespace(keys=np.concatenate(keys).astype(np.int64), off=off, tids=np.concatenate(tids),
                           w=np.concatenate(w) if wsum is not None else None)


def partitions(n, T, num_buckets):
    """slot-range partitions the fused forward uses for a training batch of n keys (0: the per-slot-counter path, b) -- for the
    batch sizes of the cases here: 1 024 keys per partition from 65 536 keys, at least 8 buckets and, with several tables, 4
    partitions per table (the GPU test holds mi355_demb_forward_fused_partitions to this)"""
    P = (n + 1023) // 1024
    assert n <= 256 * 1024, "beyond the cases of this file"
    return P if n >= 65536 and num_buckets >= 8 * P and (T == 1 or P >= 4 * T) else 0


@functools.lru_cache(maxsize=None)
def generate(name):
    """-> SimpleNamespace(cfg, spec, fill=[batch], steps=[batch]).  A batch: keys, off, tids (per occurrence), w (weights or None),
    value (score_value of the step).  The fill puts exactly C keys into every bucket, a quarter per generation; a measured step
    hits keys that are resident WHATEVER the device's tie-break was (scores above every cut of their bucket so far) and brings
    keys nobody has seen; about 60 % of its occurrences (site b) or of its unique keys (sites c, lean) are resident keys."""
    cfg = CASES[name]
    rng = np.random.default_rng(1000 + cfg.seed)
    C, T = cfg.C, len(cfg.caps)
    tbo = tbo_of(cfg.caps, C)
    NB = int(tbo[-1])
    spec = SimpleNamespace(tbo=tbo, C=C, policy=cfg.policy)
    lfu = cfg.tie_free
    # a pool of candidate keys per table, queued per bucket
    pt, pk = [], []
    for t, cap in enumerate(cfg.caps):
        k = (np.int64(t + 1) << 40) + rng.permutation(12 * cap).astype(np.int64)
        pt.append(np.full(k.size, t, np.int64)); pk.append(k)
    pt, pk = np.concatenate(pt), np.concatenate(pk)
    pb = bucket_of(pk, pt, tbo, C)
    o = np.argsort(pb, kind="stable")
    pt, pk, pb = pt[o], pk[o], pb[o]
    start = np.concatenate([[0], np.cumsum(np.bincount(pb, minlength=NB))])
    ptr = start[:-1].copy()
    low = np.zeros(NB, np.int64)          # LFU: every key a bucket ever sees gets its own low three digits: sums never tie

    def take(counts):
        assert (ptr + counts <= start[1:]).all(), "the candidate pool ran dry"
        idx = np.repeat(ptr, counts) + (np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts))
        ptr[:] += counts
        return idx

    def lfu_sums(buckets):
        """a distinct weight sum (before the repeats' 1000 each) for new keys of these buckets"""
        o2 = np.argsort(buckets, kind="stable")
        rank = np.empty(buckets.size, np.int64)
        c = np.bincount(buckets, minlength=NB)
        rank[o2] = np.arange(buckets.size) - np.repeat(np.cumsum(c) - c, c)
        lo = low[buckets] + rank + 1
        np.add.at(low, buckets, 1)
        assert int(lo.max(initial=0)) < 1000
        return 1000 * rng.integers(1, 60, buckets.size) + lo

    state, maxcut = empty_state(), np.full(NB, -1, np.int64)
    fill, steps = [], []
    per_gen = C // cfg.gens
    for g in range(cfg.gens):
        idx = take(np.full(NB, per_gen, np.int64))
        ut, uk = pt[idx], pk[idx]
        cnt = np.ones(idx.size, np.int64)
        wsum = lfu_sums(pb[idx]) if lfu else None
        bt = _lay_out(cfg, rng, ut, uk, cnt, wsum)
        bt.value = score_value(cfg, g)
        fill.append(bt)
        state, _ = apply_step(state, bt, spec)
    for j in range(cfg.steps):
        rb = bucket_of(state.keys, state.tids, tbo, C)
        certain = state.scores > maxcut[rb]
        n_new = rng.integers(cfg.new[0], cfg.new[1] + 1, NB)
        n_hit = np.minimum(rng.integers(cfg.hits[0], cfg.hits[1] + 1, NB), C - n_new)
        c3 = rng.choice(NB, cfg.case3, replace=False) if cfg.case3 else np.zeros(0, np.int64)
        n_hit[c3] = C - n_new[c3] + rng.integers(1, 4, c3.size)          # |H| + |N| > C: e > |E|
        # hits: a random choice among the certain residents of the bucket
        ci = np.flatnonzero(certain)
        ci = ci[np.argsort(rng.random(ci.size))]
        ci = ci[np.argsort(rb[ci], kind="stable")]
        cc = np.bincount(rb[ci], minlength=NB)
        n_hit = np.minimum(n_hit, cc)
        c0 = np.cumsum(cc) - cc
        hi = ci[np.repeat(c0, n_hit) + (np.arange(int(n_hit.sum())) - np.repeat(np.cumsum(n_hit) - n_hit, n_hit))]
        ni = take(n_new)
        ut, uk = np.concatenate([state.tids[hi], pt[ni]]), np.concatenate([state.keys[hi], pk[ni]])
        nh, nn = hi.size, ni.size
        # every key occurs at least once.  Site b: 60 % of the OCCURRENCES are resident keys (the over-budget cases: 35 %).  Sites c and lean: 60 % of the unique
        # KEYS are resident and a new key occurs 1.5 times on average (some in several tiles: "another record of the same key got
        # here first"), the rest of the batch repeats the hits -- a partition block evicts for at most kDefMax deferred (tile, key)
        # RECORDS per step, and a deferred key has up to one record per occurrence (see K_DEF_MAX)
        total = max(cfg.n_occ, nh + nn)
        if cfg.site == "b" or cfg.over_budget:
            extra_h = max(int(cfg.res_share * total) - nh, 0)
            extra_n = max(total - nh - nn - extra_h, 0)
        else:
            extra_n = nn // 2
            extra_h = total - nh - nn - extra_n
        cnt = np.concatenate([1 + rng.multinomial(extra_h, np.full(nh, 1.0 / nh)), 1 + rng.multinomial(extra_n, np.full(nn, 1.0 / nn))])
        wsum = None
        if lfu:
            wsum = np.concatenate([1000 * cnt[:nh], lfu_sums(pb[ni]) + 1000 * (cnt[nh:] - 1)])
        perm = rng.permutation(nh + nn)
        bt = _lay_out(cfg, rng, ut[perm], uk[perm], cnt[perm], wsum[perm] if lfu else None)
        bt.value = score_value(cfg, cfg.gens + j)
        steps.append(bt)
        state, info = apply_step(state, bt, spec, tie_break=None if lfu else "key")
        maxcut = np.maximum(maxcut, info.cut)
    return SimpleNamespace(cfg=cfg, spec=spec, fill=fill, steps=steps)
