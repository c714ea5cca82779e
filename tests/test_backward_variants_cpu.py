"""CPU checks of the small-shape net under the fused backward and the optimizer ops (tests/backward_cases.py): the case list
covers every instantiation class of launch_bwd / launch_opt, the reference's brackets can be met by the kernels' arithmetic
-- a NumPy emulation that does not run update_bracket's code: fp32 sums in orders of its own, one rounding to the gradient
dtype, the fp32 step written out here, one rounding of every stored element -- and the brackets reject seeded mistakes
wherever they apply."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import backward_cases as bc  # noqa: E402
from backward_cases import CASES, OPT_CASES  # noqa: E402
from oracle import oracle as orc  # noqa: E402

f32 = np.float32


# ------------------------------------------------------------------------------------------------ the emulation
def _seq_sum(X):
    """fp32 sum of the rows of X, one after the other"""
    acc = np.zeros(X.shape[1], f32)
    for x in X:
        acc = acc + x
    return acc


def _row_sum(X, hot, nsub, rng, chunk_twice):
    """fp32 sum of a unique row's terms in the shape of its class (hot.h), in an order that is neither the reference's nor
    necessarily the kernel's: regular rows backwards; wave rows as `nsub` slices folded pairwise; block rows as four
    partials per 1024-entry chunk, the chunks added in a shuffled order"""
    n = X.shape[0]
    if not hot or n <= 4:
        return _seq_sum(X[::-1])
    if n <= 128:
        per = -(-n // nsub)
        parts = [_seq_sum(X[i * per:(i + 1) * per]) for i in range(nsub)]
        while len(parts) > 1:
            parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
        return parts[0]
    chunks = []
    for lo in range(0, n, 1024):
        C = X[lo:lo + 1024]
        q = -(-C.shape[0] // 4)
        p = [C[i * q:(i + 1) * q].sum(axis=0, dtype=f32) for i in range(4)]
        chunks.append((p[0] + p[1]) + (p[2] + p[3]))
    if chunk_twice and len(chunks) > 1:
        chunks.append(chunks[0])
    acc = np.zeros(X.shape[1], f32)
    for i in rng.permutation(len(chunks)):
        acc = acc + chunks[i]
    return acc


def _truncate(x, dtype):
    """fp32 -> 16-bit towards zero (the seeded mistake), as fp32"""
    x = np.ascontiguousarray(x, f32)
    if dtype == "bf16":
        return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
        over = np.abs(h.astype(f32)) > np.abs(x)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(f32)


def _store(x, dtype, mistake):
    if dtype == "f32":
        return np.asarray(x, f32)
    if mistake == "truncated_store":
        return _truncate(x, dtype)
    with np.errstate(over="ignore"):
        return orc.round_to(np.asarray(x, f32), dtype)


def _step(opt, rows, g, w, so, hp, it, mistake):
    """the fp32 step of apply_sink on table rows [k, vdim] (fp32 values) of width w, state at `so`; returns the new rows"""
    r = np.array(rows, f32, copy=True)
    g = np.asarray(g, f32)
    lr, eps = f32(hp["lr"]), f32(hp["eps"])
    W = r[:, :w].copy()
    if opt == "store":
        r[:, :w] = g
    elif opt == "sgd":
        r[:, :w] = W - g * lr
    elif opt == "adam":
        im, iv = (so, so + w) if mistake != "adam_m_v_swapped" else (so + w, so)
        m, v = r[:, im:im + w].copy(), r[:, iv:iv + w].copy()
        b1, b2 = f32(hp["beta1"]), f32(hp["beta2"])
        bias1, bias2 = f32(1.0 - float(b1) ** it), f32(1.0 - float(b2) ** it)
        m = b1 * m + (f32(1) - b1) * g
        v = b2 * v + ((f32(1) - b2) * g) * g
        with np.errstate(invalid="ignore"):
            upd = (m / bias1) / (np.sqrt(v / bias2) + eps) + f32(hp["weight_decay"]) * W
        r[:, :w] = W - lr * upd
        r[:, im:im + w], r[:, iv:iv + w] = m, v
    elif opt == "adagrad":
        G = r[:, so:so + w] + g * g
        r[:, :w] = W - lr * g / (np.sqrt(G) + eps)
        r[:, so:so + w] = G
    else:
        sq = g * g
        s = np.zeros(g.shape[0], f32)
        for j in range(w - 1, -1, -1):             # a plain backwards fp32 sum (the twin sums pairwise)
            s = s + sq[:, j]
        G0 = r[:, so].copy()
        G = G0 + s / f32(w)
        used = G0 if mistake == "rowwise_G_before" else G
        with np.errstate(invalid="ignore"):        # (the mistake `state_at_D` reads the pad, of any sign, as G)
            r[:, :w] = W - lr * g / (np.sqrt(used)[:, None] + eps)
        r[:, so] = G
    return r


def emulate(case, inp, mistake=None):
    """the whole allocation after the kernel's arithmetic (fp32 images), optionally with one seeded mistake"""
    rng = np.random.default_rng(len(case.name))
    T = inp["table"].copy()
    vec = case.vector
    l = bc.lanes_log2(case.D, vec)
    nsub, gw = 64 >> l, (4 if vec else 1) << l
    so = case.D if mistake == "state_at_D" else case.state_offset
    mean = case.mode == "mean" and mistake != "sum_for_mean"
    for grp in bc.group_terms(case, inp):
        w = grp["w"]
        X = grp["X"]
        if mean:
            X = X * (f32(1) / np.maximum(grp["L"], 1).astype(f32))[:, None]
        S = np.zeros((len(grp["u"]), w), f32)
        for i, (a, c) in enumerate(zip(grp["start"], grp["cnt"])):
            n = c - 1 if (mistake == "drop_last_of_odd_rows" and c % 2 == 1) else c
            S[i] = _row_sum(X[a:a + n], case.hot, nsub, rng, mistake == "chunk_twice")
        g = orc.round_to(S, case.gdt) if (case.round_grad and mistake != "grad_not_rounded") else S
        if mistake == "second_group_from_first" and w > gw:
            g = g.copy()
            g[:, gw:2 * gw] = g[:, :min(gw, w - gw)]
        slot = inp["slots"][grp["u"]]
        ok = slot >= 0
        cols = bc.state_columns(case.opt, w, so)
        new = _step(case.opt, T[slot[ok] + 1], g[ok], w, so, case.hp, case.it, mistake)
        T[slot[ok][:, None] + 1, cols[None, :]] = _store(new[:, cols], case.wdt, mistake)
        if mistake == "failed_row_to_row0" and (~ok).any():
            for gi in g[~ok]:
                new = _step(case.opt, T[1:2], gi[None], w, so, case.hp, case.it, mistake)
                T[1, cols] = _store(new[0, cols], case.wdt, mistake)
    if case.opt == "store":
        T[inp["slots"][inp["cnt"] == 0] + 1] = 0
    return T


def _applies(case, mistake):
    gw = (4 if case.vector else 1) << bc.lanes_log2(case.D, case.vector)
    return {
        "drop_last_of_odd_rows": True,
        "sum_for_mean": case.mode == "mean",
        "second_group_from_first": case.D > gw,
        "state_at_D": case.state_pad > 0 and case.opt in ("adam", "adagrad", "rowwise_adagrad"),
        "adam_m_v_swapped": case.opt == "adam",
        "rowwise_G_before": case.opt == "rowwise_adagrad",
        "grad_not_rounded": case.round_grad and case.gdt != "f32",
        "truncated_store": case.wdt != "f32",
        "failed_row_to_row0": case.opt != "store",
        "chunk_twice": case.hot,
    }[mistake]


MISTAKES = ("drop_last_of_odd_rows", "sum_for_mean", "second_group_from_first", "state_at_D", "adam_m_v_swapped",
            "rowwise_G_before", "grad_not_rounded", "truncated_store", "failed_row_to_row0", "chunk_twice")


# ------------------------------------------------------------------------------------------------ the case list
def test_case_list_covers_every_instantiation_class_and_switch():
    table = {"vector_ncol1": (4, 36, 128, 256), "vector_ncol2": (260, 512), "vector_ncol4": (516, 1024),
             "scalar_ncol1": (7, 63), "scalar_ncol2": (65,), "scalar_ncol4": (129,), "scalar_ncol16": (257, 1023)}
    plain = {(c.klass, c.D, c.opt) for c in CASES if (c.wdt, c.gdt, c.mode) == ("f32", "f32", "sum")
             and c.hot and not c.state_pad and not c.nu_extra}
    for k, Ds in table.items():
        for D in Ds:
            for opt in bc.SINKS:
                assert (k, D, opt) in plain, (k, D, opt)
    for opt in bc.SINKS:
        assert ("scalar_ncol1_strided", 64, opt) in plain
        assert {c.klass for c in CASES if c.mode == "doff" and c.opt == opt} == {"vector_ncol1_doffsets", "scalar_ncol2_doffsets"}
    for opt in ("sgd", "adam", "rowwise_adagrad"):
        for D in (36, 260, 65):
            assert {(c.wdt, c.gdt) for c in CASES if c.D == D and c.opt == opt and c.mode == "sum"} == \
                {(w, g) for w in bc.DTYPES for g in bc.DTYPES}
    assert {c.wdt for c in CASES if c.opt == "adagrad" and c.D == 128} == {"f32", "bf16", "f16"}
    classes = set(table) | {"scalar_ncol1_strided"}
    for mode in ("seq", "mean"):
        for opt in ("sgd", "adam"):
            assert {c.klass for c in CASES if c.mode == mode and c.opt == opt} == classes
    assert {(c.opt, c.vector) for c in CASES if c.state_pad == 8} == {(o, v) for o in ("adam", "rowwise_adagrad") for v in (True, False)}
    assert {c.D for c in CASES if not c.hot} == {36, 260, 65}
    assert {c.opt for c in CASES if not c.round_grad and c.gdt == "bf16"} == {"sgd", "adam"}
    assert {c.D for c in CASES if c.nu_extra == 37} == {36, 65}
    oplain = {(c.klass, c.D, c.opt) for c in OPT_CASES if (c.wdt, c.gdt) == ("f32", "f32")}
    for k, Ds in table.items():
        for D in Ds:
            for opt in bc.SINKS[1:]:
                assert (k, D, opt) in oplain
    assert {"vector_ncol1_mixed", "scalar_ncol2_mixed"} <= {c.klass for c in OPT_CASES}


def test_batch_profile():
    c = bc.CASE_BY_NAME["class_D36_adam"]
    inp = bc.make_inputs(c)
    cnt = inp["cnt"]
    assert inp["nu"] == 77 and set(bc.PROFILE) <= set(cnt.tolist()) and (cnt == 0).sum() == 2
    assert sorted(cnt[inp["failed"]].tolist()) == [3, 40, 300] and (inp["slots"][inp["failed"]] == -1).all()
    assert 6000 < inp["n"] < 8000 and np.array_equal(np.bincount(inp["rev"], minlength=77), cnt)
    assert inp["grads"].nbytes <= 11 << 20
    m = bc.make_inputs(bc.CASE_BY_NAME["mean_D36_adam"])
    L = np.diff(m["offsets"])
    assert L.min() == 0 and L.max() <= 6 and L.size == 2 * m["B"] and L.sum() == m["n"]
    d = bc.make_inputs(bc.CASE_BY_NAME["class_doffsets_vector_adam"])
    feat = np.searchsorted(d["offsets"], np.arange(d["n"]), side="right") - 1
    feat //= d["B"]
    for u in range(77):        # a unique row belongs to one feature, and its width is that feature's
        f = set(feat[d["rev"] == u].tolist())
        assert len(f) <= 1 and all(bc.DOFF_VECTOR[x] == d["width"][u] for x in f)
    for f in range(3):         # every feature holds rows of the regular, wave and block classes
        k = set(bc.row_class(cnt_f := d["cnt"][(d["width"] == bc.DOFF_VECTOR[f]) & (d["cnt"] > 0)]).tolist())
        assert {0, 1, 2} <= k, (f, cnt_f)
    assert max(bc.make_inputs(c)["grads"].nbytes for c in CASES if c.D >= 1023) <= 13 << 20


# ------------------------------------------------------------------------------------------------ brackets
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_emulation_inside_the_bracket_and_mistakes_outside(case):
    inp = bc.make_inputs(case)
    ref = bc.reference(case, inp)
    # the reference's own nominal result -- the bracket is not empty and nothing else is expected to move
    assert (ref["lo"] - ref["slack"] <= ref["hi"] + ref["slack"]).all()
    use, changed = bc.judge(ref, emulate(case, inp))
    assert changed == 0, f"{case.name}: the emulation changed {changed} rows the reference expects untouched"
    assert use.max() <= 1, f"{case.name}: emulation outside the bracket, use {use.max()} at {np.argwhere(use > 1)[:4].tolist()}"
    for mistake in MISTAKES:
        if not _applies(case, mistake):
            continue
        use, changed = bc.judge(ref, emulate(case, inp, mistake))
        assert changed > 0 or use.max() > 1, f"{case.name}: the bracket accepts the mistake `{mistake}` (use {use.max():.3f})"


def _emulate_opt(case, inp, form, mistake=None):
    T = (inp["table"] if form == "flat" else inp["buffer"]).copy()
    r = (inp["idx"] if form == "flat" else np.arange(bc.OPT_ROWS)) + 1
    width = np.full(bc.OPT_ROWS, case.D) if form == "flat" else inp["width"]
    for w in sorted(set(width.tolist())):
        i = np.flatnonzero(width == w)
        cols = bc.state_columns(case.opt, int(w), case.D)
        new = _step(case.opt, T[r[i]], inp["grads"][i, :w], int(w), case.D, case.hp, case.it, mistake)
        T[r[i][:, None], cols[None, :]] = _store(new[:, cols], case.wdt, mistake)
    return T


@pytest.mark.parametrize("case", OPT_CASES, ids=lambda c: c.name)
def test_optimizer_op_emulation_inside_the_bracket_and_mistakes_outside(case):
    inp = bc.make_opt_inputs(case)
    for form in ("flat", "padded"):
        ref = bc.opt_reference(case, inp, form)
        use, changed = bc.judge(ref, _emulate_opt(case, inp, form))
        assert changed == 0 and use.max() <= 1, f"{case.name} {form}: use {use.max()}, {changed} other rows changed"
        for mistake, applies in (("adam_m_v_swapped", case.opt == "adam"), ("rowwise_G_before", case.opt == "rowwise_adagrad"),
                                 ("truncated_store", case.wdt != "f32")):
            if applies:
                use, _ = bc.judge(ref, _emulate_opt(case, inp, form, mistake))
                assert use.max() > 1, f"{case.name} {form}: the bracket accepts the mistake `{mistake}`"
    if case.widths:           # a narrower row read at the full width is a mistake the mixed buffer must catch
        ref = bc.opt_reference(case, inp, "padded")
        wide = dict(inp, width=np.full(bc.OPT_ROWS, case.D, np.int64))
        use, _ = bc.judge(ref, _emulate_opt(case, wide, "padded"))
        assert use.max() > 1
