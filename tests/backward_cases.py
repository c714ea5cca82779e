"""Cases, inputs and the reference of the small-shape net under the fused backward (csrc/backward.hip: bwd_kernel behind
dynamicemb_extensions.backward_fused) and the optimizer ops (opt_rows_kernel behind the *_update_for_flat_table /
*_for_padded_buffer wrappers).  No GPU and no product import here: tests/test_backward_variants_cpu.py checks on these cases
that the brackets can be met by the kernel's arithmetic and reject seeded mistakes, tests/test_backward_variants_gpu.py runs
the kernels against them.

One occurrence profile (PROFILE) is shared by all cases: it sits on both sides of every threshold of csrc/hot.h (<= 4
occurrences: the regular walk; 5-128: one wave; 129-1024: one block; more: several blocks, float atomics and a ticket) and
of the two-entries-per-round walk.  The case list is a covering design over launch_bwd / launch_opt, not a cross product:
every instantiation class (vector / scalar rows x NCOL, the forced-scalar D = 64, the D_offsets loop) with every sink in
fp32, the nine (weight, gradient) dtype pairs on three widths, and the modes and switches once each.

The reference is oracle/vec_twin.py's: the fp64 sum of a unique row's gradient terms (MEAN: each divided by its bag length
first), grad_sum_error, grad_interval in the gradient dtype ("f32" when round_grad is off), update_bracket.  Two extensions
live here and not in the twin:
  * 16-bit table rows.  The kernel evaluates the step in fp32 from the fp32 value of the stored row and rounds every stored
    element once, to nearest even.  Rounding is monotone, so the accepted set is [rnd_w(lo - slack), rnd_w(hi + slack)] and
    nothing is added to it.
  * a row narrower than its table row and a state behind a pad.  A row of width Dr keeps [emb Dr | ... | state at
    state_offset], Adam's v behind its m at state_offset + Dr (optimizer_kernel.cuh of the reference: v_ptr = m_ptr + dim);
    the twin's [emb | state] columns are mapped there and everything between must come back bit-identical.

Out of scope, covered by tests/test_path_c_oracle_gpu.py: the walk compiled for 4 groups (it needs more than 720 K unique
rows: `over_720k_unique_sgd`), the reference-entry form of the CSR (`tile_bags`) and `one_feature` -- the last two cannot be
reached through dynamicemb_extensions."""
import zlib
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from oracle import oracle as orc
from oracle.vec_twin import grad_interval, grad_sum_error, update_bracket

KIND = {"store": 0, "sgd": 1, "adam": 2, "adagrad": 3, "rowwise_adagrad": 4}
SINKS = tuple(KIND)
DTYPES = ("f32", "bf16", "f16")
LR = {"store": 0.0, "sgd": 0.05, "adam": 0.01, "adagrad": 0.05, "rowwise_adagrad": 0.05}
ADAM_ITER = 3
# occurrences of the profile rows: both sides of khot = 4, kwave = 128, kchunk = 1024 and of two chunks
PROFILE = (1, 2, 3, 4, 5, 6, 127, 128, 129, 130, 1023, 1024, 1025, 2049)
FAILED = (3, 40, 300)            # failed inserts (slot -1, address 0): regular, wave and block class
N_SMALL, N_EMPTY = 58, 2         # rows of 1-2 occurrences; unique rows the batch never names
NU = len(PROFILE) + len(FAILED) + N_SMALL + N_EMPTY      # 77: odd, no multiple of any NB * kit * NSUB
CAP = 150                        # rows of the table under test (between two guard rows)
ROW_CLASSES = ("regular", "wave", "block", "multi")


@dataclass(frozen=True)
class Case:
    name: str
    D: int
    opt: str = "sgd"               # store | sgd | adam | adagrad | rowwise_adagrad
    wdt: str = "f32"               # table rows (store: the dense output)
    gdt: str = "f32"
    mode: str = "sum"              # sum (F = 1) | mean (F = 2, bags of 0-6 keys) | seq | doff (three features, D_offsets)
    widths: Tuple[int, ...] = ()   # doff: the features' widths (the last one = D)
    grad_pad: int = 0              # elements added to the gradient row stride (1: D = 64 walks the scalar kernels)
    state_pad: int = 0             # state_offset = D + state_pad
    hot: bool = True               # False: group_by_unique(dim=0), backward_fused(hot=None)
    round_grad: bool = True
    nu_extra: int = 0              # max_unique = NU + nu_extra, nu_dev = NU

    @property
    def hp(self) -> Dict[str, float]:
        return dict(lr=LR[self.opt], beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)

    @property
    def it(self) -> int:
        return ADAM_ITER

    @property
    def F(self) -> int:
        return {"sum": 1, "mean": 2, "seq": 1, "doff": 3}[self.mode]

    @property
    def total_D(self) -> int:
        return sum(self.widths) if self.mode == "doff" else self.F * self.D

    @property
    def grad_stride(self) -> int:
        return self.total_D + self.grad_pad

    @property
    def state_offset(self) -> int:
        return self.D + self.state_pad

    @property
    def n_state(self) -> int:
        return {"store": 0, "sgd": 0, "adam": 2 * self.D, "adagrad": self.D,
                "rowwise_adagrad": 4 if self.wdt == "f32" else 8}[self.opt]       # row-wise: one element of a 16-byte pad

    @property
    def vdim(self) -> int:
        return self.D if self.opt == "store" else self.state_offset + self.n_state

    @property
    def vector(self) -> bool:
        """what dynamicemb_extensions.backward_fused decides from the shapes (`_aligned`)"""
        al = self.D % 4 == 0 and self.grad_stride % 4 == 0
        if self.mode == "doff":
            al = al and all(w % 4 == 0 for w in self.widths)
        if self.opt != "store":
            al = al and self.state_offset % 4 == 0
        return al

    @property
    def klass(self) -> str:
        """the instantiation class launch_bwd picks"""
        return kernel_class(self.D, self.vector) + ("_doffsets" if self.mode == "doff" else "") + \
            ("_strided" if self.grad_pad else "")


def lanes_log2(D: int, vector: bool) -> int:
    """lpr_log2_for of backward.hip: lanes of one column group"""
    l, per = 3, 4 if vector else 1
    while (per << l) < D and l < 6:
        l += 1
    return l


def kernel_class(D: int, vector: bool) -> str:
    per = 4 if vector else 1
    g = per << lanes_log2(D, vector)
    ncol = -(-D // g)
    ncol = 1 if ncol <= 1 else 2 if ncol <= 2 else 4 if (ncol <= 4 or vector) else 16
    return f"{'vector' if vector else 'scalar'}_ncol{ncol}"


def row_class(cnt) -> np.ndarray:
    """index into ROW_CLASSES by occurrence count (hot.h)"""
    c = np.asarray(cnt)
    return (c > 4).astype(int) + (c > 128) + (c > 1024)


CLASS_D = (4, 36, 128, 256, 260, 512, 516, 1024, 7, 63, 65, 129, 257, 1023)
MODE_D = (36, 260, 516, 7, 65, 129, 257)          # one width per class for the sequence / MEAN cases
DOFF_VECTOR = (32, 64, 128)                        # D / 4, D / 2, D
DOFF_SCALAR = (7, 30, 65)


def _cases() -> List[Case]:
    c: List[Case] = []
    for opt in SINKS:                                   # every instantiation class x every sink, fp32 rows and gradients
        for D in CLASS_D:
            c.append(Case(f"class_D{D}_{opt}", D, opt))
        c.append(Case(f"class_D64_stride65_{opt}", 64, opt, grad_pad=1))
        c.append(Case(f"class_doffsets_vector_{opt}", 128, opt, mode="doff", widths=DOFF_VECTOR))
        c.append(Case(f"class_doffsets_scalar_{opt}", 65, opt, mode="doff", widths=DOFF_SCALAR))
    for opt in ("sgd", "adam", "rowwise_adagrad"):      # the nine dtype pairs
        for D in (36, 260, 65):
            for w in DTYPES:
                for g in DTYPES:
                    if (w, g) != ("f32", "f32"):
                        c.append(Case(f"dtype_D{D}_{opt}_w{w}_g{g}", D, opt, wdt=w, gdt=g))
    c.append(Case("dtype_D128_adagrad_wbf16_gbf16", 128, "adagrad", wdt="bf16", gdt="bf16"))
    c.append(Case("dtype_D128_adagrad_wf16_gf16", 128, "adagrad", wdt="f16", gdt="f16"))
    for mode in ("seq", "mean"):                        # sequence and MEAN: once per class on SGD and Adam
        for opt in ("sgd", "adam"):
            for D in MODE_D:
                c.append(Case(f"{mode}_D{D}_{opt}", D, opt, mode=mode))
            c.append(Case(f"{mode}_D64_strided_{opt}", 64, opt, mode=mode, grad_pad=1))
    for opt in ("adam", "rowwise_adagrad"):             # state behind a pad
        for D in (36, 65):
            c.append(Case(f"statepad_D{D}_{opt}", D, opt, state_pad=8))
    c.append(Case("nohot_D36_sgd", 36, "sgd", hot=False))
    c.append(Case("nohot_D260_adam", 260, "adam", hot=False))
    c.append(Case("nohot_D65_rowwise_adagrad", 65, "rowwise_adagrad", hot=False))
    c.append(Case("noround_D36_sgd_gbf16", 36, "sgd", gdt="bf16", round_grad=False))
    c.append(Case("noround_D36_adam_gbf16", 36, "adam", gdt="bf16", round_grad=False))
    c.append(Case("nudev_D36_adam", 36, "adam", nu_extra=37))
    c.append(Case("nudev_D65_sgd", 65, "sgd", nu_extra=37))
    return c


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def warm_rows(rng, n: int, d: int, opt: str, n_state: int, pad: int) -> np.ndarray:
    """random rows [emb | pad | state] with the state of the optimizer's sign (Adam m any sign, v >= 0, AdaGrad G >= 0;
    row-wise: every element of the state's pad is random, only the first is state); the pad is random too"""
    w = rng.standard_normal((n, d))
    p = rng.standard_normal((n, pad))
    if opt == "adam":
        st = np.concatenate([0.01 * rng.standard_normal((n, d)), rng.uniform(0, 1e-3, (n, d))], 1)
    elif opt in ("adagrad", "rowwise_adagrad"):
        st = rng.uniform(0, 1, (n, n_state))
    else:
        st = np.zeros((n, 0))
    return np.concatenate([w, p, st], 1).astype(np.float32)


def _narrow_adam_v(rng, opt: str, body: np.ndarray, rows, width, so: int) -> None:
    """Adam rows narrower than the table row keep v right behind their own m (state_columns): give it v's sign"""
    if opt == "adam":
        for r, w in zip(rows, width):
            if r > 0 and so + 2 * w < body.shape[1]:
                body[r, so + w:so + 2 * w] = rng.uniform(0, 1e-3, w)


def _bag_lengths(rng, n: int, F: int) -> np.ndarray:
    """lengths of 0-6 keys that sum to n, their number a multiple of F"""
    lens = rng.integers(0, 7, size=n + 8)
    c = np.cumsum(lens)
    k = int(np.searchsorted(c, n))
    lens = lens[:k + 1].copy()
    lens[k] -= c[k] - n
    return np.concatenate([lens, np.zeros(-len(lens) % F, np.int64)]).astype(np.int64)


def make_inputs(case: Case) -> dict:
    """NumPy inputs of a case, from a generator seeded by its name.  Values are fp32 arrays already rounded to the case's
    dtypes.  `table` is the whole allocation: row 0 and the last row are guards, the table under test lies between."""
    rng = _rng(case.name)
    D = case.D
    cnt = np.array(list(PROFILE) + list(FAILED) + list(rng.integers(1, 3, N_SMALL)) + [0] * N_EMPTY, np.int64)
    failed = np.zeros(NU, bool)
    failed[len(PROFILE):len(PROFILE) + len(FAILED)] = True
    perm = rng.permutation(NU)                          # the unique-row number says nothing about the class
    cnt, failed = cnt[perm], failed[perm]
    feat = np.zeros(NU, np.int64)
    width = np.full(NU, D, np.int64)
    if case.mode == "doff":
        feat = perm % 3                                 # every feature gets rows of every class
        width = np.asarray(case.widths, np.int64)[feat]
    n = int(cnt.sum())
    inp = dict(cnt=cnt, failed=failed, width=width, n=n, nu=NU, max_unique=NU + case.nu_extra, offsets=None, D_offsets=None)
    if case.mode == "doff":
        per_f = [rng.permutation(np.repeat(np.arange(NU), np.where(feat == f, cnt, 0))) for f in range(3)]
        B = max(len(p) for p in per_f) // 3
        lens = np.concatenate([rng.multinomial(len(p), np.full(B, 1.0 / B)) for p in per_f])
        inp["rev"] = np.concatenate(per_f).astype(np.int64)
        inp["D_offsets"] = np.concatenate([[0], np.cumsum(case.widths)]).astype(np.int32)
    else:
        inp["rev"] = rng.permutation(np.repeat(np.arange(NU), cnt)).astype(np.int64)
        lens = _bag_lengths(rng, n, case.F) if case.mode != "seq" else None
        B = len(lens) // case.F if lens is not None else n
    if lens is not None:
        inp["offsets"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    inp["B"] = B
    g = rng.uniform(-0.5, 1.0, (B, case.grad_stride)).astype(np.float32)
    inp["grads"] = orc.round_to(g, case.gdt)            # [B, stride]; the kernel sees the first total_D columns
    if case.opt == "store":                             # the "table" is the dense output: row u belongs to unique row u
        slots = np.arange(NU, dtype=np.int64)
        cap = inp["max_unique"]
        body = rng.standard_normal((cap + 2, D)).astype(np.float32)
        inp["failed"] = failed = np.zeros(NU, bool)
    else:
        slots = rng.choice(CAP, NU, replace=False).astype(np.int64)
        slots[failed] = -1
        cap = CAP
        body = warm_rows(rng, cap + 2, D, case.opt, case.n_state, case.state_pad)
        _narrow_adam_v(rng, case.opt, body, slots + 1, width, case.state_offset)
    inp["slots"], inp["cap"] = slots, cap
    inp["table"] = orc.round_to(body, case.wdt)
    assert inp["table"].shape == (cap + 2, case.vdim)
    return inp


def entry_sources(case: Case, inp: dict):
    """per key position: the gradient row, the first column and the bag length of its term"""
    n = inp["n"]
    j = np.arange(n)
    if case.mode == "seq":
        return j, np.zeros(n, np.int64), np.ones(n, np.int64)
    off = inp["offsets"]
    bag = np.searchsorted(off, j, side="right") - 1
    f, b = np.divmod(bag, inp["B"])
    d0 = inp["D_offsets"][f].astype(np.int64) if case.mode == "doff" else f * case.D
    return b, d0, np.diff(off)[bag]


def group_terms(case: Case, inp: dict) -> List[dict]:
    """the gradient terms of every unique row that occurs, grouped by row width: dict(w, u [k], cnt [k], start [k],
    X [sum cnt, w] fp32 -- the raw gradient rows, a unique row's terms consecutive, in batch order -- and L [sum cnt])"""
    if "_terms" in inp:
        return inp["_terms"]
    row, d0, L = entry_sources(case, inp)
    rev = inp["rev"]
    out = []
    for w in sorted(set(inp["width"][inp["cnt"] > 0].tolist())):
        sel = np.flatnonzero(inp["width"][rev] == w)
        sel = sel[np.argsort(rev[sel], kind="stable")]
        u, c = np.unique(rev[sel], return_counts=True)
        X = inp["grads"][row[sel][:, None], d0[sel][:, None] + np.arange(w)[None, :]]
        out.append(dict(w=int(w), u=u, cnt=c, start=np.concatenate([[0], np.cumsum(c)[:-1]]), X=X, L=L[sel]))
    inp["_terms"] = out
    return out


def state_columns(opt: str, w: int, so: int) -> np.ndarray:
    """table-row columns of the twin's [emb | state] columns for a row of width w with its state at `so`"""
    emb = np.arange(w)
    if opt == "adam":
        return np.concatenate([emb, so + emb, so + w + emb])
    if opt == "adagrad":
        return np.concatenate([emb, so + emb])
    if opt == "rowwise_adagrad":
        return np.concatenate([emb, [so]])
    return emb


def rows_bracket(opt: str, wdt: str, hp, it: int, before: np.ndarray, g_lo, g_hi, w: int, so: int):
    """(lo, hi, slack) [k, vdim] of table rows `before` (fp32 values of the stored rows) after the step with any gradient
    in [g_lo, g_hi]: update_bracket on the twin's columns, the weight dtype's rounding, everything else unchanged"""
    before = np.asarray(before, np.float32)
    LO = before.astype(np.float64)
    HI, SL = LO.copy(), np.zeros_like(LO)
    cols = state_columns(opt, w, so)
    if opt == "store":
        lo, hi = np.asarray(g_lo, np.float64), np.asarray(g_hi, np.float64)
        slack = np.zeros_like(lo)
    else:
        lo, hi, slack = update_bracket(opt, before[:, cols], g_lo, g_hi, w, hp, it)
    if wdt != "f32":
        with np.errstate(over="ignore"):
            lo = orc.round_to((lo - slack).astype(np.float32), wdt).astype(np.float64)
            hi = orc.round_to((hi + slack).astype(np.float32), wdt).astype(np.float64)
        slack = np.zeros_like(lo)
    LO[:, cols], HI[:, cols], SL[:, cols] = lo, hi, slack
    return LO, HI, SL


def reference(case: Case, inp: dict) -> dict:
    """dict(rows, u, cnt, lo, hi, slack, zero_ok, before): `rows` the rows of `table` (the whole allocation) the step
    touches, [lo - slack, hi + slack] per element of them (elements the step does not touch: lo = hi = the value before,
    slack 0), and `before` = the expected bytes of every other row.  zero_ok marks the elements where an exact 0 is accepted
    as well: the columns past a narrower feature's width in the dense output, which the regular walk clears and the wave
    and block paths leave alone."""
    mean = case.mode == "mean"
    gdt = case.gdt if case.round_grad else "f32"
    T = inp["table"]
    rows, us, cnts, LO, HI, SL, ZO = [], [], [], [], [], [], []
    for grp in group_terms(case, inp):
        X = grp["X"].astype(np.float64)
        if mean:
            X = X / np.maximum(grp["L"], 1)[:, None]
        s = np.add.reduceat(X, grp["start"], axis=0)
        A = np.add.reduceat(np.abs(X), grp["start"], axis=0)
        err = grad_sum_error(grp["cnt"][:, None], A, mean)
        g_lo, _, g_hi = grad_interval(s, err, gdt)
        ok = inp["slots"][grp["u"]] >= 0
        r = inp["slots"][grp["u"]][ok] + 1
        lo, hi, sl = rows_bracket(case.opt, case.wdt, case.hp, case.it, T[r], g_lo[ok], g_hi[ok], grp["w"],
                                  case.state_offset)
        zo = np.zeros(lo.shape, bool)
        if case.opt == "store":
            zo[:, grp["w"]:] = True
        rows.append(r); us.append(grp["u"][ok]); cnts.append(grp["cnt"][ok])
        LO.append(lo); HI.append(hi); SL.append(sl); ZO.append(zo)
    if case.opt == "store":                              # unique rows without occurrences read exactly 0
        e = np.flatnonzero(inp["cnt"] == 0)
        z = np.zeros((e.size, case.vdim))
        rows.append(inp["slots"][e] + 1); us.append(e); cnts.append(np.zeros(e.size, np.int64))
        LO.append(z); HI.append(z.copy()); SL.append(z.copy()); ZO.append(np.zeros(z.shape, bool))
    return dict(rows=np.concatenate(rows), u=np.concatenate(us), cnt=np.concatenate(cnts), lo=np.concatenate(LO),
                hi=np.concatenate(HI), slack=np.concatenate(SL), zero_ok=np.concatenate(ZO), before=T)


def bracket_use(got, lo, hi, slack, zero_ok=None) -> np.ndarray:
    """per element: how far `got` lies outside [lo, hi] in units of the slack (<= 1: accepted; an element without slack
    admits only [lo, hi]; a value equal to a bound -- an overflowed fp16 state included -- is inside)"""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(got < lo, lo - got, np.where(got > hi, got - hi, 0.0))
        use = np.where(out == 0, 0.0, np.where(slack > 0, out / np.where(slack > 0, slack, 1.0), np.inf))
    use[np.isnan(got)] = np.inf
    if zero_ok is not None:
        use[zero_ok & (got == 0)] = 0.0
    return use


def same_bits(a, b) -> np.ndarray:
    """element-wise bit identity of two fp32 arrays (of fp32 images of 16-bit values)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)


def judge(ref: dict, got: np.ndarray) -> Tuple[np.ndarray, int]:
    """(bracket use [k, vdim] of the touched rows, number of other rows that changed) of a whole allocation `got`"""
    use = bracket_use(got[ref["rows"]], ref["lo"], ref["hi"], ref["slack"], ref["zero_ok"])
    rest = np.ones(got.shape[0], bool)
    rest[ref["rows"]] = False
    changed = int((~same_bits(got[rest], ref["before"][rest]).all(axis=1)).sum())
    return use, changed


def worst_by_row_class(ref: dict, use: np.ndarray) -> Dict[str, float]:
    rc = row_class(ref["cnt"])
    return {ROW_CLASSES[k]: float(use[rc == k].max()) for k in range(4) if (rc == k).any()}


# ------------------------------------------------------------------------------------------------ optimizer ops
@dataclass(frozen=True)
class OptCase:
    """one call of opt_rows_kernel: 40 rows with dense gradients, through the flat-table wrapper (rows by address inside a
    larger table) and through the padded-buffer wrapper (rows in a dense buffer); `widths`: a padded buffer whose rows
    belong to three tables of different widths, the state behind the widest"""
    name: str
    D: int
    opt: str
    wdt: str = "f32"
    gdt: str = "f32"
    widths: Tuple[int, ...] = ()

    @property
    def hp(self):
        return dict(lr=LR[self.opt], beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)

    @property
    def it(self):
        return ADAM_ITER

    @property
    def n_state(self):
        return {"sgd": 0, "adam": 2 * self.D, "adagrad": self.D, "rowwise_adagrad": 4 if self.wdt == "f32" else 8}[self.opt]

    @property
    def vdim(self):
        return self.D + self.n_state

    @property
    def vector(self):
        return self.D % 4 == 0 and all(w % 4 == 0 for w in self.widths)

    @property
    def klass(self):
        return kernel_class(self.D, self.vector) + ("_mixed" if self.widths else "")


OPT_ROWS, OPT_CAP = 40, 64


def _opt_cases() -> List[OptCase]:
    c = []
    for opt in SINKS[1:]:
        for D in CLASS_D:
            c.append(OptCase(f"opt_D{D}_{opt}", D, opt))
        c.append(OptCase(f"opt_mixed_vector_{opt}", 128, opt, widths=DOFF_VECTOR))
        c.append(OptCase(f"opt_mixed_scalar_{opt}", 65, opt, widths=DOFF_SCALAR))
    for opt in SINKS[1:]:
        for D in (36, 260, 65):
            for w in DTYPES:
                for g in DTYPES:
                    if (w, g) != ("f32", "f32"):
                        c.append(OptCase(f"opt_D{D}_{opt}_w{w}_g{g}", D, opt, wdt=w, gdt=g))
    c.append(OptCase("opt_mixed_vector_adam_wbf16_gf16", 128, "adam", wdt="bf16", gdt="f16", widths=DOFF_VECTOR))
    c.append(OptCase("opt_mixed_scalar_rowwise_adagrad_wf16_gbf16", 65, "rowwise_adagrad", wdt="f16", gdt="bf16",
                     widths=DOFF_SCALAR))
    return c


OPT_CASES = _opt_cases()
assert len({c.name for c in OPT_CASES}) == len(OPT_CASES)


def make_opt_inputs(case: OptCase) -> dict:
    """grads [40, D]; `table` [OPT_CAP + 2, vdim] with guard rows and the rows `idx` of its interior (flat form); `buffer`
    [40 + 2, vdim] with guard rows (padded form); table_ids / table_emb_dims for the rows of different widths"""
    rng = _rng(case.name)
    D = case.D
    inp = dict(grads=orc.round_to(rng.uniform(-0.5, 1.0, (OPT_ROWS, D)).astype(np.float32), case.gdt),
               idx=rng.choice(OPT_CAP, OPT_ROWS, replace=False).astype(np.int64),
               table=orc.round_to(warm_rows(rng, OPT_CAP + 2, D, case.opt, case.n_state, 0), case.wdt),
               buffer=orc.round_to(warm_rows(rng, OPT_ROWS + 2, D, case.opt, case.n_state, 0), case.wdt),
               table_ids=None, width=np.full(OPT_ROWS, D, np.int64))
    if case.widths:
        inp["table_ids"] = rng.integers(0, len(case.widths), OPT_ROWS).astype(np.int64)
        inp["width"] = np.asarray(case.widths, np.int64)[inp["table_ids"]]
        body = inp["buffer"].copy()
        _narrow_adam_v(rng, case.opt, body, np.arange(OPT_ROWS) + 1, inp["width"], D)
        inp["buffer"] = orc.round_to(body, case.wdt)
    return inp


def opt_reference(case: OptCase, inp: dict, form: str) -> dict:
    """as reference(), for `table` (form "flat": every row at the table's own width D) or `buffer` (form "padded": row i of
    the buffer's interior at width[i]); the gradient interval is one point"""
    T = inp["table"] if form == "flat" else inp["buffer"]
    r_all = (inp["idx"] if form == "flat" else np.arange(OPT_ROWS)) + 1
    width = np.full(OPT_ROWS, case.D, np.int64) if form == "flat" else inp["width"]
    k, V = OPT_ROWS, case.vdim
    LO, HI, SL = np.zeros((k, V)), np.zeros((k, V)), np.zeros((k, V))
    for w in sorted(set(width.tolist())):
        i = np.flatnonzero(width == w)
        g = inp["grads"][i, :w]
        LO[i], HI[i], SL[i] = rows_bracket(case.opt, case.wdt, case.hp, case.it, T[r_all[i]], g, g, int(w), case.D)
    return dict(rows=r_all, u=np.arange(k), cnt=np.ones(k, np.int64), lo=LO, hi=HI, slack=SL, zero_ok=None, before=T)
