"""One-hot mask probes of the HSTU attention kernels: inputs for which the suite's standing element-wise rule is sharp.

The random-operand comparisons allow k * 2^-9 * sum|P v| around every element, which a single wrong (query, key) pair never exceeds
on a long row.  The probes hold S = 1 on every pair (q, k constant, or one of them one-hot against a constant), keep every summand
non-negative, and send each key (or query) to an output column of its own, col_h(pos) = (pos + h * (pos // d)) mod d:

  probe "pv":  q = k = 1/2, alpha = 4 / d; v[j] one-hot in col_h(j); dO[i] one-hot in col_h(i)
               out[i, h, c] = SiLU(1) / scaling * #{j visible from i: col_h(j) = c}          (the mask row, folded modulo d)
               dV[j, h, c]  = SiLU(1) / scaling * #{i that see j: col_h(i) = c}              (the mask column)
  probe "dq":  q = 1/2, k[j] = 1/2 one-hot(col_h(j)), alpha = 4; v = dO = 1/2, scaling = d (dS = SiLU'(1) on every visible pair)
               dQ[i, h, c] = dS / 2 * #{j visible from i: col_h(j) = c}
  probe "dk":  the "dq" probe with q and k exchanged: dK[j, h, c] = dS / 2 * #{i that see j: col_h(i) = c}

so mag = |ref|, the rule becomes a relative one, and one wrong pair moves one element by 1 / count of it.  With a relative bias the
bias takes two levels in a checkerboard (s = 1 or 2) and the counts are weighted by the two P (dS) values.  Every value is 0, 1/4,
1/2 or 1 (and d / 4 in a bias): exact in bf16, fp16 and e4m3.

The masks are the oracle's alone: the expected tensors come from oracle/hstu_oracle.py on the probe inputs, and the dense mask the
CPU proofs count over is read off the oracle too (its forward on an identity v).  numpy and the oracle only (torch and the FP8
suites' emulations are imported by the FP8 helpers alone, when called); CASES is the one table
tests/test_hstu_probe_cpu.py (teeth, mutations) and tests/test_hstu_probe_gpu.py (the kernels) both run.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import hstu_oracle as ho

H = 2
SILU1, DSILU1 = float(ho._silu(1.0)), float(ho._dsilu(1.0))
PROBES = ("pv", "dq", "dk")
TESTED = {"pv": ("out", "dv"), "dq": ("dq",), "dk": ("dk",)}          # the sparse tensors of each probe: where the teeth are
BASE = (0, 1, 31, 32, 33, 64, 65, 127, 128, 129, 255, 257)
BITS = {"bf16": 7, "fp16": 10}

# name, family (varlen | func | rab | rab_func | delta_q | paged | fp8), d, dtype (bf16 | fp16), lengths (keys per sequence),
# lq (queries per sequence; None = self attention), window, targets (bool), ctx (bool), grp, func (shape name), rab (None | "shared" |
# "heads"), quant (FP8 mode), page (page size)
Case = namedtuple("Case", "name family d dtype lengths lq window targets ctx grp func rab quant page")


def _case(name, family, d, dtype, lengths, lq=None, window=(-1, 0), targets=False, ctx=False, grp=1, func=None, rab=None, quant=None,
          page=0):
    return Case(name, family, d, dtype, tuple(int(x) for x in lengths), None if lq is None else tuple(int(x) for x in lq),
                tuple(window), targets, ctx, grp, func, rab, quant, page)


# ------------------------------------------------------------------------------------------------------------- the standing rules
def tolerance(ref, mag, k, bits=7):
    """the tolerance array of tests/test_hstu_gpu.py: _close_elementwise (its terms, as an array: the CPU file pins the two against
    each other): 1e-3 |ref| + 1 ulp(ref) + k * 2^-(bits + 2) * mag"""
    ref = np.asarray(ref, np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - bits)
    if bits == 10:
        ulp = np.maximum(ulp, 2.0 ** -24)
    return 1e-3 * np.abs(ref) + ulp + k * 2.0 ** -(bits + 2) * np.asarray(mag, np.float64) + 1e-30


def rule_k(tensor):
    """k of the standing rule: 2 for the forward (P: one rounding), 4 for the gradients"""
    return 2 if tensor == "out" else 4


def rel_tolerance(kind):
    """relative size of the standing rule where mag = |ref|, at its widest (ref a power of two: one ulp is 2^-bits of it).
    kind: "bf16_fwd", "bf16_bwd", "fp16_fwd", "fp16_bwd" from `tolerance`; "fp8_fwd" / "fp8_bwd" from the bound of the FP8 emulations
    (tests/test_hstu_fp8_gpu.py: emulate, tests/test_hstu_fp8_bwd_cpu.py: _bound) on one pair of large operands, where their absolute
    terms vanish."""
    dt, way = kind.split("_")
    if dt != "fp8":
        return float(tolerance(np.ones(1), np.ones(1), 2 if way == "fwd" else 4, BITS[dt])[0])
    import torch

    big = torch.full((1, 1, 64), 2.0 ** 20, dtype=torch.float64)
    if way == "fwd":
        one = torch.ones(1, 1, dtype=torch.float64)
        emu, bound = fp8_suites()[0].emulate(dict(q=torch.ones(1, 1, 64, dtype=torch.float64), k=torch.ones(1, 1, 64, dtype=torch.float64), v=big,
                                                 descale_q=one, descale_k=one, descale_v=one), 3, [0, 1], 1.0 / 64, 1.0)
    else:
        x = torch.full((1, 1), 2.0 ** 20, dtype=torch.float64)
        emu = x @ big[0]
        bound = fp8_suites()[1]._bound(x, big[0], emu, 3)
    return float((bound / emu.abs()).max())


@functools.lru_cache(maxsize=None)
def fp8_suites():
    """(tests/test_hstu_fp8_gpu.py, tests/test_hstu_fp8_bwd_cpu.py) as modules, imported the way the FP8 backward tests import their
    siblings: the emulations and bounds the FP8 probes are judged with"""
    import importlib.util
    import os

    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("hstu_fp8_bwd_cpu_suite", os.path.join(here, "test_hstu_fp8_bwd_cpu.py"))
    e = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(e)
    return e.G, e


# --------------------------------------------------------------------------------------------------------------------- the cases
def longest(d, dtype="bf16"):
    """the longest sequence of a case: three rows short of the largest multiple of d whose full (non-causal) column count -- L / d in
    both heads, every d consecutive positions being a permutation of the columns -- keeps count x rel_tolerance <= 1/2 for the gradients
    (the wider rule): 30 d - 3 in bf16, 7 d - 3 in FP8; capped at 2 300 rows (the length DESIGN.md's mask-probe paragraph
    gives the reason for: the float64 oracle costs L^2 d per head and every later run of the suite pays it)"""
    per_col = int(0.5 / rel_tolerance("bf16_bwd" if dtype != "fp8" else "fp8_bwd"))
    return min(per_col * d - 3, 2300)


VARLEN_MASKS = {
    "causal": dict(window=(-1, 0)), "full": dict(window=(-1, -1)),
    "w70_0": dict(window=(70, 0)), "w33_200": dict(window=(33, 200)), "wm1_65": dict(window=(-1, 65)), "w300_m1": dict(window=(300, -1)),
    "w0_0": dict(window=(0, 0)),
    "tgt_g1": dict(targets=True, grp=1), "tgt_g3": dict(targets=True, grp=3), "ctx_tgt": dict(targets=True, ctx=True, grp=2),
}
FP8_MASKS = {   # MASKS of tests/test_hstu_fp8_gpu.py
    "causal": dict(window=(-1, 0)), "full": dict(window=(-1, -1)), "window": dict(window=(37, 5)),
    "ctx_tgt_g1": dict(targets=True, ctx=True, grp=1), "ctx_tgt_g3": dict(targets=True, ctx=True, grp=3),
}
FUNC_SHAPES = ("prefix_gap_band", "three_bounds", "blind_rows", "sink_window")
DQ_LQ, DQ_LK = (130, 9, 1, 0, 64, 33), (200, 46, 300, 50, 64, 257)      # tests/test_hstu_delta_q_bwd_gpu.py


def _lengths(d, dtype="bf16"):
    if dtype == "fp8":
        return BASE + (longest(d, "fp8"),)
    return BASE + ((1025, 2300) if d == 256 else (longest(d),))


def _build_cases():
    cs = []
    for d in (32, 64, 128, 256):
        for m, spec in VARLEN_MASKS.items():
            for dtype in ("bf16", "fp16") if d in (32, 256) else ("bf16",):     # (neighbours: the two share their references)
                cs.append(_case(f"varlen_{m}_d{d}_{dtype}", "varlen", d, dtype, _lengths(d), **spec))
    for d in (64, 256):
        for shape in FUNC_SHAPES:
            cs.append(_case(f"func_{shape}_d{d}_bf16", "func", d, "bf16", BASE + (1500,), window=(-1, -1), func=shape))
        cs.append(_case(f"func_sink_window_w450_60_d{d}_bf16", "func", d, "bf16", BASE + (1500,), window=(450, 60), func="sink_window"))
    cs.append(_case("func_three_bounds_causal_tgt_d64_bf16", "func", 64, "bf16", BASE + (700,), targets=True, grp=2, func="three_bounds"))
    cs.append(_case("rabfunc_three_bounds_d64_bf16", "rab_func", 64, "bf16", BASE + (385,), window=(-1, -1), func="three_bounds", rab="heads"))
    for d in (32, 64, 128, 256):
        for rab in ("shared", "heads"):
            cs.append(_case(f"rab_{rab}_causal_d{d}_bf16", "rab", d, "bf16", BASE + (385,), rab=rab))
        cs.append(_case(f"rab_heads_w33_200_d{d}_bf16", "rab", d, "bf16", BASE + (385,), window=(33, 200), rab="heads"))
    for d in (32, 64, 128, 256):
        cs.append(_case(f"deltaq_causal_d{d}_bf16", "delta_q", d, "bf16", DQ_LK, DQ_LQ))
        cs.append(_case(f"deltaq_w7_5_d{d}_bf16", "delta_q", d, "bf16", DQ_LK, DQ_LQ, window=(7, 5)))
        cs.append(_case(f"deltaq_ctx_tgt_d{d}_bf16", "delta_q", d, "bf16", DQ_LK, DQ_LQ, targets=True, ctx=True, grp=2))
    # paged keys, 16 per page: the cached part (keys - candidates) of a sequence ends on a page end (16, 32, 128), one key past one
    # (17, 65), inside its first page (5); the queries are the last lq keys (new history + the 3 candidates)
    pk, pq = (35, 131, 20, 68, 8, 19, 300), (10, 131, 20, 4, 8, 5, 40)
    for d in (32, 64, 128, 256):
        cs.append(_case(f"paged_tgt_d{d}_bf16", "paged", d, "bf16", pk, pq, targets=True, page=16))
    for d in (64, 256):
        cs.append(_case(f"paged_w7_5_d{d}_bf16", "paged", d, "bf16", pk, pq, window=(7, 5), page=16))
    for d in (64, 128, 256):
        for m, spec in FP8_MASKS.items():
            for mode in range(6):       # (neighbours: modes 1 .. 5 share their CPU reference)
                cs.append(_case(f"fp8_m{mode}_{m}_d{d}", "fp8", d, "bf16", _lengths(d, "fp8"), quant=mode, **spec))
    return cs


# ----------------------------------------------------------------------------------------------------------------- case geometry
def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def geometry(case):
    """(offq, offk, qpos, kpos): jagged offsets of the queries and keys and every token's ABSOLUTE position in its sequence (the
    queries of a delta-q sequence are the last lq of its keys)"""
    lk = np.asarray(case.lengths, np.int64)
    lq = lk if case.lq is None else np.asarray(case.lq, np.int64)
    kpos = np.concatenate([np.arange(n) for n in lk]) if lk.sum() else np.zeros(0, np.int64)
    qpos = np.concatenate([np.arange(k - q, k) for q, k in zip(lq, lk)]) if lq.sum() else np.zeros(0, np.int64)
    return offsets(lq), offsets(lk), qpos.astype(np.int64), kpos.astype(np.int64)


def mask_args(case):
    """(num_contexts, num_targets) per sequence, or None: 5 contextual rows and 7 targets where the sequence has them (the rule of the
    FP8 suites' masks); the delta-q cases take the numbers of tests/test_hstu_delta_q_bwd_gpu.py, the paged ones 3 candidates"""
    lk = np.asarray(case.lengths, np.int64)
    if case.family == "delta_q" and case.targets and case.lq == DQ_LQ:
        return np.array([3, 2, 4, 0, 5, 1]), np.minimum(np.array([8, 5, 1, 0, 7, 8]), np.asarray(case.lq))
    if case.family == "paged":
        return None, (np.full(lk.size, 3) if case.targets else None)
    nc = np.minimum(5, lk) if case.ctx else None
    nt = np.minimum(lk - (nc if nc is not None else 0), 7) if case.targets else None
    return nc, nt


def oracle_kwargs(case):
    nc, nt = mask_args(case)
    if case.targets or case.ctx:
        return dict(causal=True, num_targets=nt, num_contextuals=nc, target_group_size=case.grp)
    return dict(local_window=case.window)


def col(pos, h, d):
    return (pos + h * (pos // d)) % d


def _const(T, d, val):
    return np.full((T, H, d), val, np.float64)


def _onehot(pos, d, val):
    x = np.zeros((pos.size, H, d), np.float64)
    for h in range(H):
        x[np.arange(pos.size), h, col(pos, h, d)] = val
    return x


def func_of(case):
    """the mask functions of a func case, int32 [H, n_func, T]: the shapes of test_mask_functions_on_the_two_wave_kind_forward...
    (tests/test_hstu_gpu.py) scaled to the longest sequence of the case"""
    if case.func is None:
        return None
    import zlib

    rng = np.random.default_rng(zlib.crc32(case.func.encode()))
    _, offk, _, pos = geometry(case)
    T, n = int(offk[-1]), max(case.lengths)
    r = lambda lo, hi: rng.integers(lo, max(hi, lo + 1), size=(H, T))
    f = np.zeros((H, 3 if case.func == "three_bounds" else 5, T), np.int64)
    if case.func == "prefix_gap_band":      # a short prefix, two bands far to the right: whole tiles between them see nothing
        f[:, 0] = r(0, n // 15); f[:, 1] = r(6 * n // 10, 2 * n // 3); f[:, 2] = f[:, 1] + r(0, n // 8)
        f[:, 3] = r(5 * n // 6, 7 * n // 8); f[:, 4] = f[:, 3] + r(0, n // 10)
    elif case.func == "three_bounds":
        f[:, 0] = r(0, n // 5); f[:, 1] = r(n // 4, 2 * n // 5); f[:, 2] = f[:, 1] + r(0, n // 3)
    elif case.func == "blind_rows":         # half of the 64-row groups see nothing at all, the others a band
        blind = ((pos // 64) % 2 == 0)[None, :]
        f[:, 1] = np.where(blind, 0, r(n // 3, n // 3 + 20)); f[:, 2] = np.where(blind, 0, f[:, 1] + r(1, 90))
    elif case.func == "sink_window":        # the first keys and a causal window: whole tiles between them leave the stream
        f[:, 0] = np.minimum(pos + 1, r(40, 70)); f[:, 1] = np.maximum(pos - r(150, 260), 0); f[:, 2] = pos + 1
    else:
        raise KeyError(case.func)
    return f.astype(np.int32)


def rab_of(case, probe):
    """the bias of a rab case, float64 [B, H or 1, N, N]: 0 and 1 / alpha-of-the-probe's q.k in a checkerboard over (i, j), shifted by
    the head and the sequence -- s = 1 on one colour and 2 on the other"""
    if case.rab is None:
        return None
    B, N = len(case.lengths), max(case.lengths)
    hr = H if case.rab == "heads" else 1
    i, j = np.arange(N)[:, None], np.arange(N)[None, :]
    level = case.d / 4.0 if probe == "pv" else 0.25
    return np.stack([np.stack([((i + j + h + b) % 2) * level for h in range(hr)]) for b in range(B)])


def inputs(case, probe):
    return _inputs(_ref_key(case), probe)


@functools.lru_cache(maxsize=4)
def _inputs(case, probe):
    """dict(q, k, v, dout [float64, exact in bf16 / fp16 / e4m3], alpha, scaling, offq, offk, rab, func) of a probe of a case"""
    offq, offk, qpos, kpos = geometry(case)
    d, Tq, Tk = case.d, int(offq[-1]), int(offk[-1])
    if probe == "pv":
        t = dict(q=_const(Tq, d, 0.5), k=_const(Tk, d, 0.5), v=_onehot(kpos, d, 1.0), dout=_onehot(qpos, d, 1.0), alpha=4.0 / d,
                 scaling=float(max(case.lengths)))
    else:
        hot_q = probe == "dk"
        t = dict(q=_onehot(qpos, d, 0.5) if hot_q else _const(Tq, d, 0.5), k=_const(Tk, d, 0.5) if hot_q else _onehot(kpos, d, 0.5),
                 v=_const(Tk, d, 0.5), dout=_const(Tq, d, 0.5), alpha=4.0, scaling=float(d))
    t.update(offq=offq, offk=offk, rab=rab_of(case, probe), func=func_of(case))
    return t


def _pad(x, offq, offk):
    """rows of x (lq per sequence) moved to the END of that sequence's lk rows, zeros in front (the delta-q backward of the oracle is
    its self-attention backward on such q / dout: tests/test_hstu_delta_q_bwd_cpu.py pins the identity)"""
    out = np.zeros((int(offk[-1]),) + x.shape[1:], x.dtype)
    for b in range(len(offq) - 1):
        n = int(offq[b + 1] - offq[b])
        out[int(offk[b + 1]) - n:int(offk[b + 1])] = x[int(offq[b]):int(offq[b + 1])]
    return out


def _unpad(x, offq, offk):
    return np.concatenate([x[int(offk[b + 1]) - int(offq[b + 1] - offq[b]):int(offk[b + 1])] for b in range(len(offq) - 1)])


def _ref_key(case):
    return case._replace(name="", dtype="", quant=None)


def expected(case, probe, backward=True):
    """{'out', 'dq', 'dk', 'dv', 'drab'}: (reference, magnitude) float64 of a probe, from the oracle.  The magnitudes are the oracle's
    hstu_attn_magnitudes*; under mask functions (which those do not take) and for drab they are |reference|, which is the same
    thing here: every summand of every probe is >= 0."""
    return _expected(_ref_key(case), probe, backward)


@functools.lru_cache(maxsize=6)
def _expected(case, probe, backward):
    t = inputs(case, probe)
    kw = oracle_kwargs(case)
    offq, offk = t["offq"], t["offk"]
    res = {}
    if case.lq is not None:
        dkw = dict(causal=kw.get("causal", True), num_targets=kw.get("num_targets"), num_contextuals=kw.get("num_contextuals"),
                   target_group_size=kw.get("target_group_size", 1), window=kw.get("local_window"))
        res["out"] = (ho.hstu_attn_fwd_delta_q(t["q"], t["k"], t["v"], offq, offk, t["alpha"], t["scaling"], **dkw),
                      ho.hstu_attn_magnitudes_delta_q(t["q"], t["k"], t["v"], offq, offk, t["alpha"], t["scaling"], **dkw))
        if backward:
            qp, dp = _pad(t["q"], offq, offk), _pad(t["dout"], offq, offk)
            g = ho.hstu_attn_bwd(dp, qp, t["k"], t["v"], offk, t["alpha"], t["scaling"], **kw)
            m = ho.hstu_attn_magnitudes(dp, qp, t["k"], t["v"], offk, t["alpha"], t["scaling"], **kw)
            res.update(dq=(_unpad(g[0], offq, offk), _unpad(m[1], offq, offk)), dk=(g[1], m[2]), dv=(g[2], m[3]))
        return res
    fkw = dict(kw, rab=t["rab"])
    out = ho.hstu_attn_fwd(t["q"], t["k"], t["v"], offk, t["alpha"], t["scaling"], func=t["func"], **fkw)
    g = ho.hstu_attn_bwd(t["dout"], t["q"], t["k"], t["v"], offk, t["alpha"], t["scaling"], func=t["func"], **fkw) if backward else None
    if t["func"] is None:
        m = ho.hstu_attn_magnitudes(t["dout"] if backward else None, t["q"], t["k"], t["v"], offk, t["alpha"], t["scaling"], **fkw)
    else:
        m = (np.abs(out),) + ((None,) * 3 if g is None else tuple(np.abs(x) for x in g[:3]))
    res["out"] = (out, m[0])
    if backward:
        res.update(dq=(g[0], m[1]), dk=(g[1], m[2]), dv=(g[2], m[3]))
        if t["rab"] is not None:
            res["drab"] = (g[3], np.abs(g[3]))
    return res


# ------------------------------------------------------------------------------------------- what the CPU proofs count and flip
def oracle_masks(case):
    """[per sequence] bool [H, lq, lk]: the pairs the oracle lets through, read off its forward on constant q, k and an identity v
    (out[i, h, j] != 0 iff query i sees key j) -- no statement of the masks but the oracle's"""
    return _oracle_masks(_ref_key(case)._replace(rab=None, d=0))


@functools.lru_cache(maxsize=2)
def _oracle_masks(case):
    offq, offk, _, _ = geometry(case)
    nc, nt = mask_args(case)
    kw = oracle_kwargs(case)
    f = func_of(case)
    masks = []
    for b in range(len(case.lengths)):
        q0, q1, k0, k1 = int(offq[b]), int(offq[b + 1]), int(offk[b]), int(offk[b + 1])
        lq, lk = q1 - q0, k1 - k0
        one = dict(kw)
        if "num_targets" in one:
            one.update(num_targets=None if nt is None else nt[b:b + 1], num_contextuals=None if nc is None else nc[b:b + 1])
        v = np.broadcast_to(np.eye(lk)[:, None, :], (lk, H, lk))
        if case.lq is not None:
            dkw = dict(causal=one.get("causal", True), num_targets=one.get("num_targets"), num_contextuals=one.get("num_contextuals"),
                       target_group_size=one.get("target_group_size", 1), window=one.get("local_window"))
            o = ho.hstu_attn_fwd_delta_q(np.ones((lq, H, 1)), np.ones((lk, H, 1)), v, [0, lq], [0, lk], 1.0, 1.0, **dkw)
        else:
            o = ho.hstu_attn_fwd(np.ones((lk, H, 1)), np.ones((lk, H, 1)), v, [0, lk], 1.0, 1.0,
                                 func=None if f is None else f[:, :, k0:k1], **one)
        masks.append(np.ascontiguousarray(np.transpose(o != 0, (1, 0, 2))))
    return masks


def pair_weights(case, probe, tensor, b, lq, lk):
    """[H, lq, lk] (a broadcast view without a bias) what one visible pair (i, j) of sequence b adds to the element of `tensor` it lands
    in: SiLU(s) v / scaling for out and dV, dS / 2 for dQ and dK, dS for drab (s = 1; 1 or 2 under a bias)"""
    return np.broadcast_to(_pair_weights(_ref_key(case), probe, tensor, b if case.rab is not None else 0, lq, lk), (H, lq, lk))


@functools.lru_cache(maxsize=64)
def _pair_weights(case, probe, tensor, b, lq, lk):
    t = inputs(case, probe)
    s = np.ones((1, 1, 1))
    if case.rab is not None:
        n = max(case.lengths)
        s = s + (np.broadcast_to(t["rab"][b], (H, n, n))[:, lk - lq:lk, :lk] != 0)
    if tensor in ("out", "dv"):
        return ho._silu(s) / t["scaling"]
    assert probe != "pv", "the dq / dk / drab pair weights are those of the dq / dk probes"
    ds = case.d * 0.25 * ho._dsilu(s) * t["alpha"] / t["scaling"]       # dO . v = d * 1/2 * 1/2 on every pair
    return ds if tensor == "drab" else ds * 0.5


def folded(case, probe, tensor):
    """the tested tensor from direct counts over the oracle's masks: sum of the pair weights over the visible pairs of every
    (row, column-of-the-other-side) -- and the counts themselves.  Returns (value, count), float64 / int64 of the tensor's shape."""
    offq, offk, qpos, kpos = geometry(case)
    d = case.d
    by_query = tensor in ("out", "dq")
    n_rows = int((offq if by_query else offk)[-1])
    val, cnt = np.zeros((n_rows, H, d)), np.zeros((n_rows, H, d), np.int64)
    for b, m in enumerate(oracle_masks(case)):
        q0, q1, k0, k1 = int(offq[b]), int(offq[b + 1]), int(offk[b]), int(offk[b + 1])
        if q1 == q0 or k1 == k0:
            continue
        w = pair_weights(case, probe, tensor, b, q1 - q0, k1 - k0) * m
        for h in range(H):
            if by_query:
                hot = np.eye(d)[col(kpos[k0:k1], h, d)]
                val[q0:q1, h], cnt[q0:q1, h] = w[h] @ hot, np.rint(m[h].astype(np.float64) @ hot)
            else:
                hot = np.eye(d)[col(qpos[q0:q1], h, d)]
                val[k0:k1, h], cnt[k0:k1, h] = w[h].T @ hot, np.rint(m[h].T.astype(np.float64) @ hot)
    return val, cnt


def max_count(case):
    """the largest number of pairs folded into one element of a tested tensor of the case"""
    return max(int(folded(case, "pv", t)[1].max()) for t in ("out", "dv"))


def edge_pairs(case, limit=None):
    """[(name, b, h, i, j)]: mask bits worth flipping, found on the oracle's mask itself.  Rows: the first and last of every 32 / 64 /
    128 tile, the rows around the contextual / target / group boundaries and the first query (row lk - lq of the keys); in each row
    every end of a visible run (both sides: the diagonal, i - wl - 1, i + wr + 1, the ends of func intervals, the first and last
    target, the group and context boundaries) and the first and last key of every tile.  i is the query's row among the lq queries,
    j the key."""
    offq, offk, _, _ = geometry(case)
    nc, nt = mask_args(case)
    out = []
    for b, m in enumerate(oracle_masks(case)):
        lq, lk = m.shape[1], m.shape[2]
        if lq == 0 or lk == 0:
            continue
        rows = {0, lq - 1, lq // 2}
        for t in (32, 64, 128):
            for e in range(t, lk + 1, t):
                rows.update((e - 1 - (lk - lq), e - (lk - lq)))
        c = 0 if nc is None else int(nc[b])
        hst = lk - (0 if nt is None else int(nt[b]))
        for x in (c - 1, c, hst - 1, hst, hst + case.grp - 1, hst + case.grp, lk - 1):
            rows.add(x - (lk - lq))
        cols = {0, lk - 1}
        for t in (32, 64, 128):
            for e in range(t, lk + 1, t):
                cols.update((e - 1, e))
        for h in range(H):
            for i in sorted(r for r in rows if 0 <= r < lq):
                row = m[h, i]
                ends = np.nonzero(row[1:] != row[:-1])[0]
                for j in sorted(set(ends.tolist()) | set((ends + 1).tolist())):
                    out.append(("run end", b, h, i, j))
                for j in sorted(x for x in cols if 0 <= x < lk):
                    out.append(("tile edge", b, h, i, j))
    if limit is not None and len(out) > limit:
        out = [out[k] for k in np.linspace(0, len(out) - 1, limit).astype(int)]
    return out


def flip(case, probe, tensor, b, h, i, j):
    """(index, delta): the element of `tensor` that flipping mask bit (i, j) of sequence b, head h moves, and by how much"""
    offq, offk, qpos, kpos = geometry(case)
    m = oracle_masks(case)[b]
    lq, lk = m.shape[1], m.shape[2]
    w = pair_weights(case, probe, tensor, b, lq, lk)[h, i, j]
    sign = -1.0 if m[h, i, j] else 1.0
    if tensor in ("out", "dq"):
        return (int(offq[b]) + i, h, int(col(kpos[int(offk[b]) + j], h, case.d))), sign * w
    return (int(offk[b]) + j, h, int(col(qpos[int(offq[b]) + i], h, case.d))), sign * w


def locate(case, tensor, index):
    """(sequence, row in the sequence, head, column) of a flat element of a tested tensor: what a failure message names"""
    offq, offk, _, _ = geometry(case)
    off = offq if tensor in ("out", "dq") else offk
    b = int(np.searchsorted(off, index[0], side="right") - 1)
    return b, int(index[0] - off[b]), int(index[1]), int(index[2])


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------------------------ FP8 references
def fp8_mask_args(case, device="cpu"):
    """(num_contexts, num_targets, group, window) of an FP8 case as the FP8 suites' emulations take them"""
    import torch

    nc, nt = mask_args(case)
    ti = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=torch.int32, device=device)
    return ti(nc), ti(nt), case.grp, case.window


def fp8_cpu_reference(case, probe):
    return _fp8_cpu_reference(_ref_key(case)._replace(quant=min(case.quant, 1)), probe)


@functools.lru_cache(maxsize=6)
def _fp8_cpu_reference(case, probe):
    """{'out' | 'dq' | 'dk' | 'dv': (emulation, bound)} float64 numpy of an FP8 case WITHOUT a device (the quantisers are kernels): the
    probes' values are exact in e4m3 and every group maximum is 1/2 or 1, so a quantiser returns 448 (or 0) times its descale -- the input
    itself, times 1 + 2^-8 at most where the reference rounds amax / 448 to bf16 (modes 1 (vt), 3, 4, 5), one factor per tensor.  A
    constant factor moves value and bound alike, so the emulations of the FP8 suites are run here on the inputs themselves with descales
    of 1 (mode 0 as mode 0: its bound alone has no P / dS scale); on the device the GPU file runs them on the quantised operands."""
    import torch

    G, E = fp8_suites()
    t = inputs(case, probe)
    B = len(case.lengths)
    mode = 0 if case.quant == 0 else 3
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    kw = dict(q=f64(t["q"]), k=f64(t["k"]), v=f64(t["v"]), dout=f64(t["dout"]), q_t=None, k_t=None, dout_t=None)
    for w in ("q", "k", "v", "do"):
        kw["descale_" + w] = torch.ones(B, H, dtype=torch.float64)
    nc, nt, g, window = fp8_mask_args(case)
    off = torch.from_numpy(t["offk"])
    emu, bound = G.emulate(kw, mode, off, t["alpha"], t["scaling"], nc, nt, g, window)
    res = {"out": (emu.numpy(), bound.numpy())}
    for n, (e, b) in E.emulate_bwd(kw, mode, off, t["alpha"], t["scaling"], nc, nt, g, window).items():
        res[n] = (e.numpy(), b.numpy())
    return res
