"""The mask probes of tests/hstu_probe.py, the parts that need no device: for every case tests/test_hstu_probe_gpu.py runs (the two
files read one table), the oracle's tested tensor is the direct count over the oracle's own mask (unit x integer without a bias),
the case has teeth -- the standing tolerance is at most half of what one (query, key) pair contributes, at EVERY element of the tested
tensor, and max_count x rel_tolerance <= 1/2 -- and a mask bit flipped at any edge (diagonal, window ends, targets, groups, contexts, row
lk - lq, tile edges, func interval ends) is flagged by the standing rule with the reference held fixed."""
import numpy as np
import pytest
import torch

import hstu_probe as hp

CPU_LIMIT = 600          # flipped bits per case, head and tensor, spread evenly over the edges found
REAL_RULE = 3            # of which this many go through the suite's own assertion (the others through its tolerance array)


@pytest.fixture
def rule(monkeypatch):
    """_close_elementwise of tests/test_hstu_gpu.py, with its report to the tolerance summary switched off (mutated tensors are not
    kernels' results)"""
    import conftest
    import test_hstu_gpu as tg

    monkeypatch.setattr(conftest, "record_tolerance_use", lambda *a: None)
    return tg._close_elementwise


@pytest.mark.parametrize("bits", [7, 10])
@pytest.mark.parametrize("k", [2, 4])
def test_tolerance_array_is_the_standing_rule(rule, k, bits):
    rng = np.random.default_rng(k + bits)
    ref = rng.uniform(-2, 2, (50, 2, 8)) * 2.0 ** rng.integers(-20, 3, (50, 2, 8))
    ref[0] = 0
    mag = np.abs(ref) * rng.uniform(1, 30, ref.shape)
    tol = hp.tolerance(ref, mag, k, bits)
    sign = np.where(rng.random(ref.shape) < 0.5, -1.0, 1.0)
    rule(torch.from_numpy(ref + 0.999 * sign * tol), ref, mag, k, bits)
    for e in ((0, 1, 3), (7, 0, 0), (49, 1, 7)):
        x = ref.copy()
        x[e] += 1.001 * sign[e] * tol[e]
        with pytest.raises(AssertionError):
            rule(torch.from_numpy(x), ref, mag, k, bits)


def test_relative_tolerances():
    """about 1.3 % / 1.7 % in bf16 (forward / backward), much less in fp16, about 6.3 % in FP8"""
    assert hp.rel_tolerance("bf16_fwd") == 1e-3 + 2.0 ** -7 + 2 * 2.0 ** -9
    assert hp.rel_tolerance("bf16_bwd") == 1e-3 + 2.0 ** -7 + 4 * 2.0 ** -9
    assert hp.rel_tolerance("fp16_bwd") == 1e-3 + 2.0 ** -10 + 4 * 2.0 ** -12
    for kind in ("fp8_fwd", "fp8_bwd"):
        assert 2.0 ** -4 + 2.0 ** -11 + 2.0 ** -16 <= hp.rel_tolerance(kind) <= 2.0 ** -4 + 2.0 ** -11 + 2.0 ** -16 + 1e-5


def test_the_case_table_covers_what_it_must():
    names = set(hp.BY_NAME)
    for d in (32, 64, 128, 256):
        for m in hp.VARLEN_MASKS:
            c = hp.BY_NAME[f"varlen_{m}_d{d}_bf16"]
            assert set(hp.BASE) <= set(c.lengths) and max(c.lengths) >= min(hp.longest(d), 2300)
            assert (f"varlen_{m}_d{d}_fp16" in names) == (d in (32, 256))
        assert {1025, 2300} <= set(hp.BY_NAME[f"varlen_causal_d{d}_bf16"].lengths) or d != 256
    for c in hp.CASES:
        if c.family == "paged":      # a cached part that ends on a page end, one key past one, inside its first page
            cached = {k - 3 for k in c.lengths}
            assert any(x > 0 and x % c.page == 0 for x in cached) and any(x % c.page == 1 and x > c.page for x in cached)
            assert any(0 < x < c.page for x in cached)
        if c.family == "fp8":        # mode 1's transposed direction meets columns that are empty within a 128-token tile
            assert any(0 < n < c.d for n in c.lengths)
    assert {c.quant for c in hp.CASES if c.family == "fp8"} == set(range(6))
    assert {c.func for c in hp.CASES if c.family == "func" and c.d == 256} >= set(hp.FUNC_SHAPES)


def _tested(case):
    """(probe, tensor) pairs the GPU file puts its teeth on"""
    if case.family == "paged":
        return [("pv", "out")]
    return [(p, t) for p in hp.PROBES for t in hp.TESTED[p]]


def _tolerances(case, probe):
    """{tensor: (reference, tolerance array)} of the rule the GPU file applies to this case"""
    if case.family == "fp8":
        return hp.fp8_cpu_reference(case, probe)
    res = hp.expected(case, probe, backward=case.family != "paged")
    return {t: (ref, hp.tolerance(ref, mag, hp.rule_k(t), hp.BITS[case.dtype])) for t, (ref, mag) in res.items()}


@pytest.mark.parametrize("name", list(hp.BY_NAME))
def test_counts_teeth_and_flipped_bits(name, rule):
    case = hp.BY_NAME[name]
    G = hp.fp8_suites()[0]
    if case.family == "fp8" and case.quant >= 2:
        # modes 1 .. 5 share one proof: without a device the mode enters neither the probe inputs nor the bound (fp8_cpu_reference runs
        # them all as scaled-P emulations on the inputs themselves), so the mode-1 case of the same mask and head dim stands for them
        twin = hp.BY_NAME[name.replace(f"fp8_m{case.quant}_", "fp8_m1_")]
        assert twin._replace(name="", quant=None) == case._replace(name="", quant=None)
        return
    for probe in hp.PROBES:
        tested = [t for p, t in _tested(case) if p == probe]
        if not tested:
            continue
        tols = _tolerances(case, probe)
        oracle = hp.expected(case, probe, backward=case.family != "paged")
        for tensor in tested + (["drab"] if case.rab is not None and probe != "pv" else []):
            ref, tol = tols[tensor] if tensor in tols else (None, None)
            if tensor == "drab":
                # the mask itself: a positive constant (two under the checkerboard) on visible pairs, exactly 0 elsewhere
                ref = oracle["drab"][0]
                n = max(case.lengths)
                for b, m in enumerate(hp.oracle_masks(case)):
                    L = m.shape[1]
                    w = hp.pair_weights(case, probe, "drab", b, L, L) * m
                    want = w if case.rab == "heads" else w.sum(0, keepdims=True)
                    np.testing.assert_allclose(ref[b, :, :L, :L], want, rtol=1e-12, atol=0)
                    assert not ref[b, :, L:].any() and not ref[b, :, :, L:].any()
                continue
            # 1. the oracle's tensor is the direct count over the oracle's mask
            val, cnt = hp.folded(case, probe, tensor)
            np.testing.assert_allclose(oracle[tensor][0], val, rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(ref, val, rtol=1e-9, atol=1e-300)       # (FP8: the emulation is the oracle's value too)
            assert (val >= 0).all() and ((val > 0) == (cnt > 0)).all()
            unit = min(float(hp.pair_weights(case, probe, tensor, b, 1, 1).min()) for b in range(len(case.lengths)))
            if case.rab is None:
                k = val / unit
                assert np.abs(k - np.rint(k)).max() < 1e-9 and (np.rint(k) == cnt).all()
            if case.family != "fp8":
                np.testing.assert_allclose(oracle[tensor][1], np.abs(val), rtol=1e-12, atol=1e-300)   # mag = |ref|: the rule is relative
            # 2. teeth: one pair is at least twice the tolerance, wherever it lands
            assert float(tol.max()) <= unit / 2, f"{name} {tensor}: tolerance {tol.max():.3e} against a pair of {unit:.3e}"
            kind = ("fp8" if case.family == "fp8" else case.dtype) + ("_fwd" if tensor == "out" else "_bwd")
            assert float(val.max()) / unit * hp.rel_tolerance(kind) <= 0.5, f"{name} {tensor}: count {val.max() / unit:.1f}"
            # 3. a flipped mask bit is flagged, the reference held fixed
            edges = hp.edge_pairs(case, CPU_LIMIT)
            assert edges
            real = 0
            for what, b, h, i, j in edges:
                idx, delta = hp.flip(case, probe, tensor, b, h, i, j)
                assert abs(delta) > tol[idx], f"{name} {tensor}: {what} ({b}, {h}, {i}, {j}) hides under the rule"
                if real < REAL_RULE and what == "run end":
                    real += 1
                    x = ref.copy()
                    x[idx] += delta
                    if case.family == "fp8":
                        assert not G.violations(torch.from_numpy(ref), torch.from_numpy(ref), torch.from_numpy(tol)).any()
                        assert G.violations(torch.from_numpy(x), torch.from_numpy(ref), torch.from_numpy(tol)).any()
                    else:
                        mag = oracle[tensor][1]
                        rule(torch.from_numpy(ref), ref, mag, hp.rule_k(tensor), hp.BITS[case.dtype])
                        with pytest.raises(AssertionError):
                            rule(torch.from_numpy(x), ref, mag, hp.rule_k(tensor), hp.BITS[case.dtype])
