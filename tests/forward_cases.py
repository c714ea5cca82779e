"""Cases, inputs, references and a NumPy emulation for the small-shape net under the embedding forward's per-op chain
(csrc/value_ops.hip, csrc/gather_dev.h): mi355_gather_pooled (gather_pooled_pipe_kernel, gather_pooled_vec_kernel,
gather_pooled_scalar_kernel) and mi355_gather_rows (gather_rows_kernel).  No GPU and no product import here:
tests/test_forward_variants_cpu.py shows on these cases that every dispatch class is owned, that the fp32 reference lies
inside the bound and that seeded mistakes are rejected; tests/test_forward_variants_gpu.py runs the kernels.

Dispatch.  `pooled_class` restates launch_pooled: aligned16 (what dynamicemb_extensions.gather_embedding_pooled decides
from the shapes; the GPU test adds the pointers), lpr_log2_for, ncol, kAddr from row_addr / rev, UNR from n <= 8 FB.

Bag layouts.  F = 3, B = 23 (FB = 69: no multiple of a lane-group count or of KIT = 4).  One "short" (n <= 8 FB) and one
"long" (n > 8 FB) layout per lane-group width LPR, each with bags of 0, 1, 2, 3, 4, 5, LPR - 1, LPR, LPR + 1 and 2 LPR + 1
keys, an empty first bag, the aligned group of bags 4..7 empty and two empty bags at the end (offsets[FB - 1] ==
offsets[FB] == n).  About 100 unique rows.  Row-address sources are tables of [embedding | state] rows (value_dim = D + 8)
in which three unique rows have no row (address 0); the longest bag starts and ends with one of them.

References, per output element:
  (1) oracle.gather_pooled / oracle.gather_sequence: the fp32 sum in key order, one division, one rounding -- compared
      bit for bit (`exact_bits`);
  (2) the fp64 pooled value with oracle/vec_twin.py's forward_bound (any summation order), asserted as use <= 1.

Memory.  Output and source are the interior of flat allocations with a guard block of GUARD elements (a multiple of 16
bytes in every dtype) on either side, filled with SENTINEL; arrays of a whole allocation are carried as BITS (uint32 /
uint16) so that foreign bytes compare exactly."""
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import oracle as orc
from oracle.vec_twin import bound_use, forward_bound

DTYPES = ("f32", "bf16", "f16")
EB = {"f32": 4, "bf16": 2, "f16": 2}
SENTINEL = {"f32": 0x7FA5A5A5, "bf16": 0x7FA5, "f16": 0x7DA5}      # NaNs of the three formats
_BITS = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}
BITS = _BITS
GUARD = 64                       # elements per guard block
F, B = 3, 23
FB = F * B
KIT = 4                          # bags per lane group of the pipelined kernel
NU = 101                         # unique rows
CAP = 128                        # rows of a row-address source
STATE = 8                        # state elements behind the embedding of a table row
MISSING = (3, 40, 77)            # unique rows without a row (address 0) in row-address sources
EMPTY_BAGS = (0, 4, 5, 6, 7, FB - 2, FB - 1)
LPRS = (8, 16, 32, 64)


# ------------------------------------------------------------------------------------------------ bits
def to_bits(v, dtype: str) -> np.ndarray:
    """bit patterns of fp32 values that are exact in `dtype`"""
    v = np.ascontiguousarray(v, np.float32)
    if dtype == "f32":
        return v.view(np.uint32).copy()
    if dtype == "bf16":
        return (v.view(np.uint32) >> 16).astype(np.uint16)
    return v.astype(np.float16).view(np.uint16).copy()


def from_bits(b, dtype: str) -> np.ndarray:
    b = np.ascontiguousarray(b, _BITS[dtype])
    if dtype == "f32":
        return b.view(np.float32).copy()
    if dtype == "bf16":
        return (b.astype(np.uint32) << 16).view(np.float32)
    return b.view(np.float16).astype(np.float32)


def guarded(interior_bits: np.ndarray, dtype: str) -> np.ndarray:
    g = np.full(GUARD, SENTINEL[dtype], _BITS[dtype])
    return np.concatenate([g, np.ascontiguousarray(interior_bits, _BITS[dtype]).ravel(), g])


def trunc_to(x, dtype: str) -> np.ndarray:
    """fp32 -> dtype by truncation (toward zero), as fp32 values"""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f32":
        return x
    if dtype == "bf16":
        return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float32)


# ------------------------------------------------------------------------------------------------ dispatch
def lpr_log2_for(D: int) -> int:
    l = 3
    while (4 << l) < D and l < 6:
        l += 1
    return l


def _aligned(*vals) -> bool:
    return all(v % 4 == 0 for v in vals)


def pooled_class(D: int, aligned: bool, has_addr: bool, has_rev: bool, n: int, fb: int, has_doff: bool = False,
                 src_stride: int = 0) -> str:
    """the kernel instantiation launch_pooled picks (dtypes apart).  Scalar launches are one instantiation per dtype
    pair; they are named after what a case exercises in it (the column loop e = lane + 64 k, the source, D_offsets)."""
    if not aligned:
        if has_addr:
            return "scalar_addr"
        if has_doff:
            return "scalar_doffsets"
        if D % 4 == 0:
            return f"scalar_D{D}_stride{src_stride}"
        return f"scalar_D{D}"
    l = lpr_log2_for(D)
    ncol = -(-D // (4 << l))
    if ncol <= 1:
        k = 2 if (has_addr and not has_rev) else 1 if has_addr else 0
        return f"pipe_addr{k}_unr{4 if n <= 8 * fb else 8}_lpr{1 << l}"
    src = "dense" if not has_addr else "addr_rev" if has_rev else "addr_norev"
    return f"vec_ncol{2 if ncol <= 2 else 4}_{src}"


REQUIRED_POOLED = tuple(
    [f"pipe_addr{k}_unr{u}_lpr{l}" for k in (0, 1, 2) for u in (4, 8) for l in LPRS]
    + [f"vec_ncol{c}_{s}" for c in (2, 4) for s in ("dense", "addr_rev", "addr_norev")]
    + ["scalar_D7", "scalar_D65", "scalar_D130", "scalar_D1023", "scalar_D64_stride65", "scalar_addr", "scalar_doffsets"])
PIPE_D = (4, 8, 12, 32, 36, 64, 100, 128, 132, 256)
VEC_D = (260, 384, 512, 516, 768, 1024)
DTYPE_D = {"pipe": 36, "vec": 260, "scalar": 65}


@dataclass(frozen=True)
class Case:
    name: str
    D: int                          # uniform width, or max_D with `widths`
    src: str = "dense"              # dense | addr (row addresses per unique row, through rev) | occ (per occurrence, rev NULL)
    mean: bool = False
    sdt: str = "f32"
    ddt: str = "f32"
    long: bool = False              # the layout with n > 8 FB
    widths: Tuple[int, ...] = ()    # D_offsets: the features' widths
    src_pad: int = 0                # dense source: elements added to the row stride

    @property
    def feat_widths(self) -> Tuple[int, ...]:
        return self.widths if self.widths else (self.D,) * F

    @property
    def total_D(self) -> int:
        return sum(self.feat_widths)

    @property
    def stride(self) -> int:
        """elements between source rows"""
        return self.D + (self.src_pad if self.src == "dense" else STATE)

    @property
    def aligned(self) -> bool:
        """dynamicemb_extensions.gather_embedding_pooled's decision from the shapes (row addresses carry no stride of
        their own there; the cases keep table rows 16-byte aligned whenever the widths are)"""
        al = _aligned(self.D, self.total_D, self.stride if self.src == "dense" else 0)
        return al and all(w % 4 == 0 for w in np.cumsum(self.feat_widths))

    @property
    def lpr(self) -> int:
        return 1 << lpr_log2_for(self.D) if self.aligned else 8

    @property
    def klass(self) -> str:
        n = layout(self.lpr, self.long)["n"]
        return pooled_class(self.D, self.aligned, self.src != "dense", self.src != "occ", n, FB, bool(self.widths), self.stride)

    @property
    def kernel(self) -> str:
        return self.klass.split("_")[0]


def _cases() -> List[Case]:
    c: List[Case] = []
    for D in PIPE_D:                                       # every pipe class on every width it serves, SUM and MEAN
        for src in ("dense", "addr", "occ"):
            for lg in (False, True):
                for mean in (False, True):
                    c.append(Case(f"pipe_D{D}_{src}_{'long' if lg else 'short'}_{'mean' if mean else 'sum'}", D, src, mean, long=lg))
    for i, D in enumerate(VEC_D):                          # the lock-step kernel: NCOL 2 and 4, three sources
        for src in ("dense", "addr", "occ"):
            for mean in (False, True):
                lg = D in (384, 768)
                c.append(Case(f"vec_D{D}_{src}_{'long' if lg else 'short'}_{'mean' if mean else 'sum'}", D, src, mean, long=lg))
    for D in (7, 65, 130, 1023):                           # the scalar kernel: the column loop e = lane + 64 k up to k = 15
        for mean in (False, True):
            c.append(Case(f"scalar_D{D}_dense_{'mean' if mean else 'sum'}", D, mean=mean, long=D == 65))
    for mean in (False, True):
        m = "mean" if mean else "sum"
        c.append(Case(f"scalar_D64_stride65_{m}", 64, mean=mean, src_pad=1))
        c.append(Case(f"scalar_D65_addr_{m}", 65, "addr", mean))
        c.append(Case(f"scalar_D65_occ_{m}", 65, "occ", mean, long=True))
        c.append(Case(f"scalar_doffsets_7_30_65_{m}", 65, mean=mean, widths=(7, 30, 65)))
        c.append(Case(f"scalar_doffsets_65_30_7_addr_{m}", 65, "addr", mean, widths=(65, 30, 7)))
        for src in ("dense", "addr", "occ"):               # D_offsets with widths below max_D, the narrow feature first and last
            for lg in (False, True):
                c.append(Case(f"pipe_doffsets_8_16_32_{src}_{'long' if lg else 'short'}_{m}", 32, src, mean, long=lg,
                              widths=(8, 16, 32)))
            c.append(Case(f"pipe_doffsets_32_16_8_{src}_{m}", 32, src, mean, widths=(32, 16, 8)))
            c.append(Case(f"vec_doffsets_260_8_512_{src}_{m}", 512, src, mean, widths=(260, 8, 512)))
        c.append(Case(f"vec_doffsets_512_8_260_addr_{m}", 512, "addr", mean, widths=(512, 8, 260)))
    for s in DTYPES:                                       # the nine dtype pairs at one width per kernel
        for d in DTYPES:
            if (s, d) == ("f32", "f32"):
                continue
            for mean in (False, True):
                m = "mean" if mean else "sum"
                for src in ("dense", "addr", "occ"):
                    c.append(Case(f"dtype_pipe_D36_{src}_{m}_s{s}_d{d}", 36, src, mean, s, d, long=mean))
                    c.append(Case(f"dtype_vec_D260_{src}_{m}_s{s}_d{d}", 260, src, mean, s, d))
                c.append(Case(f"dtype_scalar_D65_dense_{m}_s{s}_d{d}", 65, "dense", mean, s, d))
                c.append(Case(f"dtype_scalar_D65_addr_{m}_s{s}_d{d}", 65, "addr", mean, s, d))
    return c


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------------ layouts
_LAYOUTS: Dict[Tuple[int, bool], dict] = {}


def special_lengths(lpr: int) -> Tuple[int, ...]:
    return (0, 1, 2, 3, 4, 5, lpr - 1, lpr, lpr + 1, 2 * lpr + 1)


def layout(lpr: int, long: bool) -> dict:
    """dict(offsets [FB + 1], rev [n], n, lens): shared by every case of the lane-group width and kind"""
    key = (lpr, long)
    if key in _LAYOUTS:
        return _LAYOUTS[key]
    rng = _rng(f"layout_{lpr}_{long}")
    free = [i for i in range(FB) if i not in EMPTY_BAGS]
    place = rng.permutation(free)
    lens = np.zeros(FB, np.int64)
    sp = special_lengths(lpr)
    lens[place[:len(sp)]] = sp
    rest = place[len(sp):]
    if long:                                              # about 600 keys: past 8 FB = 552 by a margin
        avg = (8 * FB + 48 - sum(sp)) // rest.size
        lens[rest] = rng.integers(max(avg - 3, 1), avg + 4, rest.size)
        if lens.sum() <= 8 * FB:
            lens[rest[0]] += 8 * FB + 1 - lens.sum()
    else:
        lens[rest] = rng.integers(0, 5, rest.size)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offsets[-1])
    assert (n > 8 * FB) if long else (n <= 8 * FB)
    rev = rng.integers(0, NU, n).astype(np.int64)
    big = int(np.argmax(lens))                            # the longest bag starts and ends with a row that may be missing
    rev[offsets[big]], rev[offsets[big + 1] - 1] = MISSING[0], MISSING[1]
    one = int(np.flatnonzero(lens == 1)[0])               # and the bag of one key IS one (MEAN of nothing present)
    rev[offsets[one]] = MISSING[2]
    _LAYOUTS[key] = dict(offsets=offsets, rev=rev, n=n, lens=lens)
    return _LAYOUTS[key]


def _source(rng, src: str, D: int, stride: int, sdt: str):
    """(bits of the whole source allocation, slots [NU]): dense -- NU rows of `stride` elements, unique row u is row u;
    otherwise a table of CAP rows [embedding D | state], unique row u in row slots[u] (-1: no row)"""
    rows = NU if src == "dense" else CAP
    body = orc.round_to(rng.standard_normal((rows, stride)).astype(np.float32), sdt)
    if src == "dense":
        slots = np.arange(NU, dtype=np.int64)
    else:
        slots = rng.choice(CAP, NU, replace=False).astype(np.int64)
        slots[list(MISSING)] = -1
    return guarded(to_bits(body, sdt), sdt), slots


def make_inputs(case: Case) -> dict:
    lay = layout(case.lpr, case.long)
    rng = _rng(case.name)
    src_bits, slots = _source(rng, case.src, case.D, case.stride, case.sdt)
    doff = np.concatenate([[0], np.cumsum(case.widths)]).astype(np.int32) if case.widths else None
    out0 = guarded(np.full(B * case.total_D, SENTINEL[case.ddt], _BITS[case.ddt]), case.ddt)
    return dict(lay, src_bits=src_bits, slots=slots, D_offsets=doff, out0=out0)


def unique_rows(src_bits, slots, sdt: str, stride: int, D: int) -> np.ndarray:
    """[len(slots), D] fp32: the embedding of every unique row, zeros where it has no row"""
    body = from_bits(src_bits[GUARD:-GUARD], sdt).reshape(-1, stride)
    out = np.zeros((slots.size, D), np.float32)
    ok = slots >= 0
    out[ok] = body[slots[ok], :D]
    return out


def reference(case: Case, inp: dict) -> dict:
    """dict(exact_bits [B total_D]: reference (1); x, bound [B, total_D]: reference (2))"""
    uniq = unique_rows(inp["src_bits"], inp["slots"], case.sdt, case.stride, case.D)
    off, rev = inp["offsets"], inp["rev"]
    exact = orc.gather_pooled(uniq, rev, off, B, int(case.mean), inp["D_offsets"], case.ddt)
    TD = case.total_D
    x, S, nt = np.zeros((B, TD)), np.zeros((B, TD)), np.zeros((B, TD))
    rows = uniq[rev].astype(np.float64)
    lens = np.diff(off)
    d0 = np.concatenate([[0], np.cumsum(case.feat_widths)])
    for f in range(F):
        w = case.feat_widths[f]
        L = lens[f * B:(f + 1) * B]
        nz = L > 0
        starts = off[f * B:(f + 1) * B][nz]
        if starts.size:
            mine = rows[:off[(f + 1) * B], :w]              # (reduceat's last segment runs to the end of what it is given)
            x[nz, d0[f]:d0[f] + w] = np.add.reduceat(mine, starts, axis=0)
            S[nz, d0[f]:d0[f] + w] = np.add.reduceat(np.abs(mine), starts, axis=0)
        nt[:, d0[f]:d0[f] + w] = L[:, None]
        if case.mean:
            x[nz, d0[f]:d0[f] + w] /= L[nz, None]
            S[nz, d0[f]:d0[f] + w] /= L[nz, None]
    return dict(exact_bits=to_bits(exact, case.ddt).ravel(), x=x, bound=forward_bound(x, S, nt, case.ddt, case.mean))


def judge(case: Case, ref: dict, got_bits: np.ndarray) -> Tuple[np.ndarray, np.ndarray, int]:
    """(use [B, total_D] of reference (2), bit identity with reference (1) [B, total_D], guard elements that changed) of a
    whole output allocation"""
    got_bits = np.asarray(got_bits)
    inner = got_bits[GUARD:-GUARD]
    val = from_bits(inner, case.ddt).reshape(B, case.total_D)
    use = bound_use(val, ref["x"], ref["bound"])
    same = (inner == ref["exact_bits"]).reshape(B, case.total_D)
    s = SENTINEL[case.ddt]
    foreign = int((got_bits[:GUARD] != s).sum() + (got_bits[-GUARD:] != s).sum())
    return use, same, foreign


# ------------------------------------------------------------------------------------------------ emulation and mistakes
MISTAKES = ("drop_last", "add_next", "layout_bf", "mean_present", "zero_as_row0", "col_shift", "doff_wide", "acc_in_out",
            "trunc_store")


def applies(mistake: str, case: Case) -> bool:
    return {"drop_last": True, "add_next": True, "layout_bf": True,
            "mean_present": case.mean and case.src != "dense",
            "zero_as_row0": case.src != "dense",
            "col_shift": case.D > (256 if case.aligned else 64),
            "doff_wide": bool(case.widths),
            "acc_in_out": case.ddt != "f32",
            "trunc_store": case.ddt != "f32"}[mistake]


def emulate(case: Case, inp: dict, mistake: Optional[str] = None) -> np.ndarray:
    """the whole output allocation (bits) after the kernels' arithmetic -- the rows of a bag added in fp32 in key order,
    one correctly rounded division for MEAN, one rounding to nearest even at the store -- with one seeded mistake:
      drop_last     the last row of a bag is not added          add_next    the row after the bag is added as well
      layout_bf     bag i is taken for (b, f) = divmod(i, F)     mean_present  MEAN divides by the rows present, not by L
      zero_as_row0  address 0 reads row 0 of the table           col_shift   column groups k >= 1 read four elements on
      doff_wide     every feature is stored max_D wide (the stores of the narrow features landing last)
      acc_in_out    the sum is kept in the output dtype          trunc_store   the store truncates"""
    n, off, rev, slots = inp["n"], inp["offsets"], inp["rev"], inp["slots"]
    TD, D = case.total_D, case.D
    lo, hi = off[:-1].copy(), off[1:].copy()
    Ltrue = hi - lo
    if mistake == "drop_last":
        hi = hi - (Ltrue > 0)
    if mistake == "add_next":
        hi = np.minimum(hi + 1, n)
    bag = np.arange(FB)
    f_of, b_of = (bag % F, bag // F) if mistake == "layout_bf" else (bag // B, bag % B)
    widths = np.asarray(case.feat_widths, np.int64)
    d0s = np.concatenate([[0], np.cumsum(widths)])
    s = slots[rev]
    present = s >= 0
    readable = np.ones(n, bool) if mistake == "zero_as_row0" else present
    cols = np.arange(D)
    group = 256 if case.aligned else 64
    csrc = cols + 4 * (cols >= group) if mistake == "col_shift" else cols
    src = from_bits(inp["src_bits"], case.sdt)
    idx = GUARD + np.where(present, s, 0)[:, None] * case.stride + csrc[None, :]
    R = src[np.minimum(idx, src.size - 1)]
    R[~readable] = 0
    acc = np.zeros((FB, D), np.float32)
    Le = hi - lo
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(int(Le.max())):
            m = Le > r
            acc[m] = acc[m] + R[lo[m] + r]
            if mistake == "acc_in_out":
                acc[m] = orc.round_to(acc[m], case.ddt)
        acc[cols[None, :] >= widths[f_of][:, None]] = 0      # lanes past a feature's width load the zero row
        L = Ltrue
        if mistake == "mean_present":
            cp = np.concatenate([[0], np.cumsum(present)])
            L = cp[off[1:]] - cp[off[:-1]]
        if case.mean:
            nz = L > 0
            acc[nz] = acc[nz] / L[nz].astype(np.float32)[:, None]
        val = trunc_to(acc, case.ddt) if mistake == "trunc_store" else orc.round_to(acc, case.ddt)
    out = inp["out0"].copy()
    order = range(F - 1, -1, -1) if mistake == "doff_wide" else range(F)
    for f in order:
        sel = np.flatnonzero(f_of == f)
        w = D if mistake == "doff_wide" else int(widths[f])
        pos = GUARD + b_of[sel][:, None] * TD + d0s[f] + np.arange(w)[None, :]
        ok = pos < out.size
        out[pos[ok]] = to_bits(val[sel, :w], case.ddt)[ok]
    return out


# ------------------------------------------------------------------------------------------------ sequence gather
@dataclass(frozen=True)
class SeqCase:
    name: str
    D: int
    src: str = "dense"              # dense | addr
    sdt: str = "f32"
    ddt: str = "f32"
    index: bool = True              # False: index == NULL (row i of the source / address i)
    n_dev: bool = False             # the device-side count is SEQ_NDEV < SEQ_N
    dst_pad: int = 0                # dst_stride = D + dst_pad
    src_pad: int = 0

    @property
    def stride(self) -> int:
        return self.D + (self.src_pad if self.src == "dense" else STATE)

    @property
    def aligned(self) -> bool:
        return _aligned(self.D, self.stride, self.D + self.dst_pad)

    @property
    def klass(self) -> str:
        return f"rows_{'vec' if self.aligned else 'scalar'}_{self.src}_lpr{1 << lpr_log2_for(self.D)}"


SEQ_N, SEQ_NDEV = 90, 53             # rows of a sequence case (several blocks at every LPR; SEQ_N <= NU: index == NULL)
REQUIRED_SEQ = tuple(f"rows_{k}_{s}_lpr{l}" for k in ("vec", "scalar") for s in ("dense", "addr") for l in (8, 64))


def _seq_cases() -> List[SeqCase]:
    c: List[SeqCase] = []
    for D in (8, 256, 7, 131):                              # vec / scalar at LPR 8 / 64
        for src in ("dense", "addr"):
            for d in DTYPES:
                c.append(SeqCase(f"seq_D{D}_{src}_sf32_d{d}", D, src, ddt=d))
            c.append(SeqCase(f"seq_D{D}_{src}_sbf16_df32", D, src, "bf16", "f32"))
            c.append(SeqCase(f"seq_D{D}_{src}_sf16_dbf16", D, src, "f16", "bf16"))
            c.append(SeqCase(f"seq_D{D}_{src}_noindex", D, src, index=False))
            c.append(SeqCase(f"seq_D{D}_{src}_ndev", D, src, n_dev=True))
            c.append(SeqCase(f"seq_D{D}_{src}_dstpad8_dbf16", D, src, ddt="bf16", dst_pad=8))
    for src in ("dense", "addr"):                           # the vector loop past one lane-group pass
        c.append(SeqCase(f"seq_D300_{src}", 300, src))
        c.append(SeqCase(f"seq_D300_{src}_sbf16_df16_dstpad8_ndev", 300, src, "bf16", "f16", n_dev=True, dst_pad=8))
    c.append(SeqCase("seq_D64_stride65_scalar", 64, src_pad=1))
    return c


SEQ_CASES = _seq_cases()
assert len({c.name for c in SEQ_CASES}) == len(SEQ_CASES)
SEQ_MISTAKES = ("zero_as_row0", "negative_as_row0", "col_shift", "trunc_store", "ignore_n_dev", "dense_stride", "one_more_row")


def seq_applies(mistake: str, case: SeqCase) -> bool:
    return {"zero_as_row0": case.src == "addr", "negative_as_row0": case.index,
            "col_shift": case.D > (4 if case.aligned else 1) << lpr_log2_for(case.D),
            "trunc_store": (case.sdt, case.ddt) in (("f32", "bf16"), ("f32", "f16"), ("f16", "bf16")),   # the pairs that round
            "ignore_n_dev": case.n_dev, "dense_stride": case.dst_pad > 0, "one_more_row": True}[mistake]


def make_seq_inputs(case: SeqCase) -> dict:
    rng = _rng(case.name)
    src_bits, slots = _source(rng, case.src, case.D, case.stride, case.sdt)
    if case.index:
        index = rng.integers(0, NU, SEQ_N).astype(np.int64)
        index[[5, 64]] = -1                                  # no key: a zero row
        index[[0, 33, SEQ_NDEV - 1]] = MISSING               # (row-address sources) a key without a row
    else:
        index = None
    out0 = guarded(np.full((SEQ_N + 1) * (case.D + case.dst_pad), SENTINEL[case.ddt], _BITS[case.ddt]), case.ddt)
    return dict(src_bits=src_bits, slots=slots, index=index, out0=out0, n=SEQ_N, n_eff=SEQ_NDEV if case.n_dev else SEQ_N)


def seq_emulate(case: SeqCase, inp: dict, mistake: Optional[str] = None) -> np.ndarray:
    """the whole output allocation (bits): [SEQ_N + 1 rows of D + dst_pad] between the guards -- the extra row, the pad
    and the rows past n_dev keep the sentinel.  mistake None: oracle.gather_sequence on the rows the op owns."""
    D, st = case.D, case.D + case.dst_pad
    n = inp["n"] if mistake == "ignore_n_dev" else inp["n_eff"]
    n = n + 1 if mistake == "one_more_row" else n
    idx = inp["index"] if inp["index"] is not None else np.arange(SEQ_N + 1)
    idx = np.concatenate([idx, [7]])[:n]
    if mistake == "negative_as_row0":
        idx = np.maximum(idx, 0)
    s = np.where(idx >= 0, inp["slots"][np.maximum(idx, 0)], -1)
    if mistake is None:
        val = orc.gather_sequence(unique_rows(inp["src_bits"], s, case.sdt, case.stride, D), np.arange(n), case.ddt)
    else:
        has = s >= 0
        if mistake == "zero_as_row0":
            has = idx >= 0
        cols = np.arange(D)
        group = (4 if case.aligned else 1) << lpr_log2_for(D)
        csrc = cols + 4 * (cols >= group) if mistake == "col_shift" else cols
        src = from_bits(inp["src_bits"], case.sdt)
        pos = GUARD + np.maximum(s, 0)[:, None] * case.stride + csrc[None, :]
        v = src[np.minimum(pos, src.size - 1)]
        v[~has] = 0
        with np.errstate(invalid="ignore", over="ignore"):
            val = trunc_to(v, case.ddt) if mistake == "trunc_store" else orc.round_to(v, case.ddt)
    out = inp["out0"].copy()
    dst = D if mistake == "dense_stride" else st
    pos = GUARD + np.arange(n)[:, None] * dst + np.arange(D)[None, :]
    out[pos] = to_bits(val, case.ddt)
    return out


# ------------------------------------------------------------------------------------------------ flat-table copy
FLAT_TABLES = ((24, 16, 47), (10, 6, 43))     # (value_dim, emb_dim, rows) of the two tables (rows >= FLAT_N: unique indices)
FLAT_N = 41                                   # rows per call: eleven blocks of four waves, the last one part-filled
FLAT_MAX_EMB = 16
FLAT_PAD = 4                                  # elements between the dense rows (dense_stride = dense_dim + FLAT_PAD)


@dataclass(frozen=True)
class FlatCase:
    region: int                     # 0 contiguous (one table), 1 embedding, 2 embedding + state re-padded to FLAT_MAX_EMB
    load: bool
    dtype: str
    dense_dim: int
    table: int = 0                  # region 0: the table

    @property
    def name(self) -> str:
        return f"flat_r{self.region}_{'load' if self.load else 'store'}_{self.dtype}_dd{self.dense_dim}_t{self.table}"


def _flat_cases() -> List[FlatCase]:
    c = []
    for load in (True, False):
        for d in DTYPES:
            c += [FlatCase(0, load, d, 16, 0), FlatCase(0, load, d, 30, 0), FlatCase(0, load, d, 7, 1),
                  FlatCase(0, load, d, 13, 1),                      # region 0: dense_dim below and above value_dim, both tables
                  FlatCase(1, load, d, 4), FlatCase(1, load, d, 20),    # region 1: below and above both emb_dims
                  FlatCase(2, load, d, FLAT_MAX_EMB + 8)]           # region 2: the widest state (8) behind FLAT_MAX_EMB
    return c


FLAT_CASES = _flat_cases()


def make_flat_inputs(case: FlatCase) -> dict:
    """tables: interiors [rows, value_dim] (bits); dense [FLAT_N, dense_dim + FLAT_PAD] (bits); idx (-1: skipped; unique
    per table, stores of one row twice race by design) and table_ids"""
    rng = _rng(case.name)
    tables = [to_bits(orc.round_to(rng.standard_normal((r, v)).astype(np.float32), case.dtype), case.dtype)
              for v, _, r in FLAT_TABLES]
    dense = to_bits(orc.round_to(rng.standard_normal((FLAT_N, case.dense_dim + FLAT_PAD)).astype(np.float32), case.dtype),
                    case.dtype)
    tid = np.full(FLAT_N, case.table, np.int64) if case.region == 0 else rng.integers(0, 2, FLAT_N).astype(np.int64)
    idx = np.zeros(FLAT_N, np.int64)
    for t, (_, _, r) in enumerate(FLAT_TABLES):
        m = tid == t
        idx[m] = rng.permutation(r)[:m.sum()]
    idx[[2, 17, FLAT_N - 1]] = -1
    return dict(tables=tables, dense=dense, idx=idx, tid=tid)


def flat_copy_reference(case: FlatCase, inp: dict):
    """(tables, dense) after the call, by slicing"""
    tables = [t.copy() for t in inp["tables"]]
    dense = inp["dense"].copy()
    for i in range(FLAT_N):
        r, t = int(inp["idx"][i]), int(inp["tid"][i])
        if r < 0:
            continue
        v, e, _ = FLAT_TABLES[t]
        if case.region == 2:
            spans = [(0, 0, e), (e, FLAT_MAX_EMB, v - e)]      # (table column, dense column, length)
        else:
            spans = [(0, 0, min(v if case.region == 0 else e, case.dense_dim))]
        for tc, dc, ln in spans:
            if case.load:
                dense[i, dc:dc + ln] = tables[t][r, tc:tc + ln]
            else:
                tables[t][r, tc:tc + ln] = dense[i, dc:dc + ln]
    return tables, dense
