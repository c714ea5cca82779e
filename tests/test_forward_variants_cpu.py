"""CPU checks of the small-shape net under the embedding forward's per-op chain (tests/forward_cases.py): the case list
owns every dispatch class of launch_pooled and of the sequence gather, the bag layouts carry the lengths and the empty
bags the kernels branch on, the fp32 reference (oracle.gather_pooled: key order, one rounding) lies inside the fp64
reference's bound on every case -- so bit identity and the bound can both hold -- and a NumPy emulation of the kernels'
arithmetic with one seeded mistake at a time leaves an element outside the bound, or changes a guard element, on every case
where the mistake applies."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import forward_cases as fc  # noqa: E402
from forward_cases import CASES, SEQ_CASES  # noqa: E402

_REF = {}


def _ref(case):
    """inputs and references of a case, computed once for the tests of this file"""
    if case.name not in _REF:
        inp = fc.make_inputs(case)
        _REF[case.name] = (inp, fc.reference(case, inp))
    return _REF[case.name]


def test_every_pooled_class_has_a_case():
    have = {c.klass for c in CASES}
    missing = [k for k in fc.REQUIRED_POOLED if k not in have]
    assert not missing, f"dispatch classes of launch_pooled without a case: {missing}"
    by = {}
    for c in CASES:
        by.setdefault(c.klass, set()).add(c.mean)
    assert all(by[k] == {False, True} for k in fc.REQUIRED_POOLED), "a class without SUM or without MEAN"
    for kernel, dims in (("pipe", fc.PIPE_D), ("vec", fc.VEC_D)):
        got = {c.D for c in CASES if c.kernel == kernel and not c.widths}
        assert set(dims) <= got, f"{kernel}: widths {sorted(set(dims) - got)} without a case"
    for kernel, D in fc.DTYPE_D.items():                    # the nine dtype pairs at one width per kernel, SUM and MEAN
        pairs = {(c.sdt, c.ddt, c.mean) for c in CASES if c.kernel == kernel and c.D == D and not c.widths}
        assert len(pairs) == 18, f"{kernel} at D = {D}: {len(pairs)} of 18 (source, output, combiner) triples"
    for kernel in ("pipe", "vec", "scalar"):                # D_offsets with a feature narrower than max_D, every source
        assert any(c.kernel == kernel and c.widths and min(c.widths) < c.D for c in CASES)
    for k in ("vec_ncol2", "pipe_addr1", "pipe_addr2"):
        assert any(c.klass.startswith(k) and c.widths for c in CASES), f"{k}: no D_offsets case"


def test_every_sequence_class_has_a_case():
    have = {c.klass for c in SEQ_CASES}
    assert not [k for k in fc.REQUIRED_SEQ if k not in have]
    for k in fc.REQUIRED_SEQ:
        mine = [c for c in SEQ_CASES if c.klass == k]
        assert {c.ddt for c in mine} == set(fc.DTYPES), f"{k}: output dtypes {sorted({c.ddt for c in mine})}"
        assert any(not c.index for c in mine) and any(c.n_dev for c in mine) and any(c.dst_pad for c in mine), k
    assert any(c.D == 300 and c.aligned for c in SEQ_CASES)


@pytest.mark.parametrize("lpr", fc.LPRS)
@pytest.mark.parametrize("long", [False, True])
def test_bag_layouts(lpr, long):
    lay = fc.layout(lpr, long)
    off, lens, n = lay["offsets"], lay["lens"], lay["n"]
    assert off.size == fc.FB + 1 and n == off[-1] and (n > 8 * fc.FB) == long and n <= 700
    assert all(fc.FB % g for g in (2, 4, 8, 16, 32))
    assert set(fc.special_lengths(lpr)) <= set(lens.tolist())
    assert any(l % 4 for l in lens.tolist())                # the lock-step kernel's round of RPR = 4 rows ends inside a bag
    assert lens[0] == 0                                      # an empty first bag
    assert (lens[4:8] == 0).all() and 4 % fc.KIT == 0        # one whole lane group's bags empty
    assert off[fc.FB - 2] == off[fc.FB - 1] == off[fc.FB] == n    # empty bags at the very end: offsets == n
    rev = lay["rev"]
    big = int(np.argmax(lens))
    assert lens[big] == 2 * lpr + 1 and rev[off[big]] in fc.MISSING and rev[off[big + 1] - 1] in fc.MISSING
    assert rev.min() >= 0 and rev.max() < fc.NU and np.unique(rev).size < n      # repeated rows


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_inside_the_bound_and_mistakes_outside(case):
    inp, ref = _ref(case)
    # the emulation without a mistake IS reference (1), and reference (1) lies inside reference (2)
    clean = fc.emulate(case, inp)
    use, same, foreign = fc.judge(case, ref, clean)
    assert same.all() and foreign == 0, f"{case.name}: the emulation differs from oracle.gather_pooled"
    assert use.max() <= 1, f"{case.name}: the fp32 reference uses {use.max()} of the bound"
    if case.src != "dense":                                  # a row address of 0 is a row of zeros: MEAN still divides by L
        assert (inp["slots"][list(fc.MISSING)] == -1).all()
    for m in fc.MISTAKES:
        if not fc.applies(m, case):
            continue
        use, same, foreign = fc.judge(case, ref, fc.emulate(case, inp, m))
        assert use.max() > 1 or foreign > 0, f"{case.name}: the mistake `{m}` passes (worst use {use.max()})"
        assert not same.all()


def test_every_mistake_applies_somewhere():
    for m in fc.MISTAKES:
        ks = {c.kernel for c in CASES if fc.applies(m, c)}
        want = {"pipe", "vec", "scalar"} - ({"pipe"} if m == "col_shift" else set())    # pipe rows are one column group
        assert want <= ks, f"`{m}` applies to {sorted(ks)} only"
    for m in fc.SEQ_MISTAKES:
        assert any(fc.seq_applies(m, c) for c in SEQ_CASES), m


@pytest.mark.parametrize("case", SEQ_CASES, ids=lambda c: c.name)
def test_sequence_mistakes_change_the_bytes(case):
    inp = fc.make_seq_inputs(case)
    clean = fc.seq_emulate(case, inp)
    st = case.D + case.dst_pad
    body = clean[fc.GUARD:-fc.GUARD].reshape(fc.SEQ_N + 1, st)
    s = fc.SENTINEL[case.ddt]
    assert (body[inp["n_eff"]:] == s).all() and (body[:, case.D:] == s).all() and (body[:inp["n_eff"], :case.D] != s).all()
    if case.index:                                           # a negative index and (row addresses) a zero address read zeros
        zero = [5] + ([0, 33] if case.src == "addr" else [])
        assert (fc.from_bits(body[zero, :case.D], case.ddt) == 0).all()
    for m in fc.SEQ_MISTAKES:
        if fc.seq_applies(m, case):
            assert (fc.seq_emulate(case, inp, m) != clean).any(), f"{case.name}: the mistake `{m}` leaves every byte"
