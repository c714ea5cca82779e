"""CPU oracle -- TEST INFRASTRUCTURE ONLY.

`VecEmbeddingTwin`: the contract of `dict_twin.DictEmbeddingTwin` (a key -> row map per table, rows [embedding | optimizer
state] in fp32, pooling in fp64, the fp32 optimizer maths of oracle.py) without its per-key Python loops, so that it keeps
up with the batches the partitioned index path serves (64 K - 1 M keys).  Each table is a SORTED key array with its row
matrix; a batch is deduplicated with np.unique, looked up with np.searchsorted, new keys are appended and the table
re-sorted.  Nothing here imports the product.

Besides the values, the twin keeps what the element-wise bounds below are built from: per output element the sum of the
absolute values of its terms and their number, per unique key of a backward its occurrence count and the sum of |g|.
"""
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from . import oracle as orc

U32 = 2.0 ** -24                       # unit roundoff of fp32 (round to nearest)
_MANT = {"f32": 23, "bf16": 7, "f16": 10}
_EMIN = {"f32": -126, "bf16": -126, "f16": -14}
_STATE = {"sgd": lambda d: 0, "adam": lambda d: 2 * d, "adagrad": lambda d: d, "rowwise_adagrad": lambda d: 4}


def gamma(n) -> np.ndarray:
    """gamma(n) = n u / (1 - n u), u = 2^-24: |fl(sum of n + 1 terms) - sum| <= gamma(n) * sum |terms| in ANY order
    (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4)"""
    n = np.maximum(np.asarray(n, np.float64), 0.0)
    return n * U32 / (1.0 - n * U32)


def ulp(x, dtype: str) -> np.ndarray:
    """spacing of `dtype` (f32 / bf16 / f16) at |x| (subnormal spacing below the smallest normal)"""
    a = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(a)                                  # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    e = np.maximum(np.where(a > 0, e - 1, _EMIN[dtype]), _EMIN[dtype])
    return np.ldexp(1.0, (e - _MANT[dtype]).astype(np.int64))


def round_grad(x, dtype: str) -> np.ndarray:
    """fp64 -> fp32 (RNE) -> the gradient dtype (RNE), as fp32 values"""
    return orc.round_to(np.asarray(x, np.float64).astype(np.float32), dtype)


def debug_rows(keys: np.ndarray, dim: int) -> np.ndarray:
    """DEBUG initialiser, vectorised: every element = float(key % 100000) (dict_twin.debug_row)"""
    return np.repeat((np.asarray(keys, np.int64) % 100000).astype(np.float32)[:, None], dim, axis=1)


def constant_rows(value: float) -> Callable[[np.ndarray, int], np.ndarray]:
    """CONSTANT initialiser: every element = value"""
    return lambda keys, dim: np.full((len(keys), dim), np.float32(value), np.float32)


# ------------------------------------------------------------------------------------------------ bounds
def forward_bound(x, abs_sum, nterms, out_dtype: str, mean: bool = False) -> np.ndarray:
    """Bound on |out - x| for one pooled / sequence output element.

    x: the fp64 value (the fp64 sum of the exact fp32 rows, MEAN: divided by the bag length L = nterms); abs_sum: the sum
    of |terms| (MEAN: also divided by L); nterms: the number of terms.  The product adds the n fp32 rows in fp32 in an
    unknown order -- n - 1 roundings, |err| <= gamma(n - 1) * sum|terms| whatever the order -- MEAN then scales by 1 / L:
    one more rounding when it divides, two when it multiplies by a rounded reciprocal, so gamma(n + 1) * abs_sum covers
    both.  Last, ONE rounding to the output dtype, at most half an ulp of the value it rounds, which lies within
    |x| + gamma * abs_sum.  (The fp64 reference itself is off by <= n 2^-53 abs_sum: negligible here, and included.)
    An empty bag (n = 0) must read exactly 0 -- its bound is the smallest spacing of the dtype."""
    n = np.asarray(nterms, np.float64)
    g = gamma(n - 1 + (2 if mean else 0))
    e = g * abs_sum + n * 2.0 ** -53 * abs_sum
    return e + 0.5 * ulp(np.abs(x) + e, out_dtype)


def grad_sum_error(cnt, abs_sum, mean: bool = False) -> np.ndarray:
    """Bound on |s32 - s| of a reduced gradient: s the fp64 sum of a key's cnt gradient terms, s32 the product's fp32 sum of
    the same terms in any order (gamma(cnt - 1) * sum|g|); MEAN scales every term by 1 / L first (<= 2 roundings per term:
    gamma(cnt + 1)).  Plus the fp64 sum's own rounding (<= cnt 2^-53 sum|g|)."""
    c = np.asarray(cnt, np.float64)
    return (gamma(c - 1 + (2 if mean else 0)) + c * 2.0 ** -53) * abs_sum


def grad_interval(s, err, gdt: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(lo, nominal, hi) of the reduced gradient the optimizer may see: the product's fp32 sum lies in [s - err, s + err];
    rounding to fp32 and then to the gradient dtype is monotone, so the rounded value lies in
    [rnd(s - err), rnd(s + err)] -- with a bf16 / fp16 gradient that is one value, or two neighbours when the interval
    straddles a rounding boundary.  nominal = rnd(s)."""
    s = np.asarray(s, np.float64)
    return round_grad(s - err, gdt), round_grad(s, gdt), round_grad(s + err, gdt)


def _f(x):
    return np.float32(x)


def adam_bias(beta: float, t: int) -> np.float32:
    """1 - beta^t for the fp32 hyper-parameter beta, evaluated exactly (fp64) and rounded once to fp32"""
    b = float(np.float32(beta))
    return np.float32(1.0 - b ** int(t))


def update_rows(opt: str, rows: np.ndarray, g: np.ndarray, d: int, hp: Dict[str, float], it: int) -> np.ndarray:
    """the fp32 optimizer step of oracle.py on a copy of `rows` ([k, d + state]) with the reduced gradient g ([k, d])"""
    r = np.array(rows, np.float32, copy=True)
    g = np.asarray(g, np.float32)
    if opt == "sgd":
        orc.sgd_update(r, g, d, hp["lr"])
    elif opt == "adam":
        w, m, v = r[:, :d], r[:, d:2 * d], r[:, 2 * d:3 * d]
        b1, b2 = _f(hp["beta1"]), _f(hp["beta2"])
        m[:] = b1 * m + (_f(1) - b1) * g
        v[:] = b2 * v + (_f(1) - b2) * g * g
        mh, vh = m / adam_bias(hp["beta1"], it), v / adam_bias(hp["beta2"], it)
        w[:] = w - _f(hp["lr"]) * (mh / (np.sqrt(vh) + _f(hp["eps"])) + _f(hp["weight_decay"]) * w)
    elif opt == "adagrad":
        orc.adagrad_update(r, g, d, hp["lr"], hp["eps"])
    elif opt == "rowwise_adagrad":
        orc.rowwise_adagrad_update(r, g, d, hp["lr"], hp["eps"])
    else:
        raise ValueError(opt)
    return r


def update_bracket(opt: str, rows: np.ndarray, g_lo: np.ndarray, g_hi: np.ndarray, d: int, hp: Dict[str, float],
                   it: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(lo, hi, slack): [lo - slack, hi + slack] holds every element of the updated rows ([k, d + state]) when the optimizer sees ANY gradient in [g_lo, g_hi].

    Range: each step is monotone in the quantities it reads, so the range is spanned by the twin's fp32 update at the
    interval's corners.  SGD: w - lr g (monotone in g).  AdaGrad: G + g^2 (monotone in g^2; 0 when the interval straddles
    0) and w - lr g / (sqrt(G + g^2) + eps) (d/dg >= 0).  Row-wise AdaGrad: G + sum(g^2) / D over the row's interval of
    g^2, then w - lr g / (sqrt(G') + eps) at the four corners (g, G').  Adam: m (monotone in g), v (monotone in g^2), then
    w at the four corners (m', v') -- the update is monotone in each for a fixed other.

    Slack: the twin and the product each evaluate the step in fp32 -- every operation rounds once (or less, fused): per
    side |err(w')| <= u |w'| + k u |delta| (+ Adam's rounding of m' carried through the division), with k counting the
    roundings of delta (SGD 1; AdaGrad 6; row-wise (D + 2) / 2 + 5 for the sum of squares; Adam 10 -- two of them the bias
    terms 1 - beta^t, which the product forms in double from the fp32 beta).  The two sides differ by at most twice that;
    state elements likewise (m': 2 u (|b1 m| + (1 - b1) |g|) per side, v' 4 u v', AdaGrad G' 2 u G', row-wise
    gamma(D + 2) G')."""
    rows = np.asarray(rows, np.float32)
    glo, ghi = np.minimum(g_lo, g_hi).astype(np.float32), np.maximum(g_lo, g_hi).astype(np.float32)
    straddle = (glo < 0) & (ghi > 0)
    sq_lo = np.where(straddle, _f(0), np.minimum(glo * glo, ghi * ghi)).astype(np.float32)
    sq_hi = np.maximum(glo * glo, ghi * ghi).astype(np.float32)
    gmag = np.maximum(np.abs(glo), np.abs(ghi)).astype(np.float64)
    lr, eps = _f(hp["lr"]), _f(hp["eps"])
    w = rows[:, :d]
    cands, slack = [], np.zeros(rows.shape, np.float64)
    if opt == "sgd":
        for gg in (glo, ghi):
            r = rows.copy(); r[:, :d] = w - gg * lr; cands.append(r)
        delta = gmag * float(lr)
        k = 1.0
    elif opt == "adagrad":
        G = rows[:, d:2 * d]
        for gg, sq in ((glo, sq_lo), (ghi, sq_hi)):
            r = rows.copy()
            r[:, d:2 * d] = G + sq
            r[:, :d] = w - lr * gg / (np.sqrt(G + gg * gg) + eps)
            cands.append(r)
        Gn = (G + sq_hi).astype(np.float64)
        slack[:, d:2 * d] = 4 * U32 * Gn
        delta = float(lr) * gmag / (np.sqrt((G + sq_lo).astype(np.float64)) + float(eps))
        k = 6.0
    elif opt == "rowwise_adagrad":
        G = rows[:, d]
        Gs = [G + sq.sum(axis=1, dtype=np.float32) / _f(d) for sq in (sq_lo, sq_hi)]
        for gg in (glo, ghi):
            for Gn in Gs:
                r = rows.copy(); r[:, d] = Gn; r[:, :d] = w - lr * gg / (np.sqrt(Gn)[:, None] + eps); cands.append(r)
        slack[:, d] = 2 * gamma(d + 2) * Gs[1].astype(np.float64)
        delta = float(lr) * gmag / (np.sqrt(Gs[0].astype(np.float64))[:, None] + float(eps))
        k = (d + 2) / 2 + 5
    elif opt == "adam":
        m, v = rows[:, d:2 * d], rows[:, 2 * d:3 * d]
        b1, b2 = _f(hp["beta1"]), _f(hp["beta2"])
        bias1, bias2 = adam_bias(hp["beta1"], it), adam_bias(hp["beta2"], it)
        ms = [b1 * m + (_f(1) - b1) * gg for gg in (glo, ghi)]
        vs = [b2 * v + (_f(1) - b2) * sq for sq in (sq_lo, sq_hi)]
        wd = _f(hp["weight_decay"])
        for mm in ms:
            for vv in vs:
                r = rows.copy()
                r[:, d:2 * d], r[:, 2 * d:3 * d] = mm, vv
                r[:, :d] = w - lr * ((mm / bias1) / (np.sqrt(vv / bias2) + eps) + wd * w)
                cands.append(r)
        e_m = 2 * U32 * (np.abs(float(b1) * m.astype(np.float64)) + (1 - float(b1)) * gmag)
        slack[:, d:2 * d] = 2 * e_m
        slack[:, 2 * d:3 * d] = 8 * U32 * vs[1].astype(np.float64)
        den = np.sqrt(vs[0].astype(np.float64) / float(bias2)) + float(eps)
        mmag = np.maximum(np.abs(ms[0]), np.abs(ms[1])).astype(np.float64)
        delta = float(lr) * (mmag / float(bias1) / den + float(wd) * np.abs(w.astype(np.float64)))
        slack[:, :d] += 2 * float(lr) * e_m / float(bias1) / den
        k = 10.0
    else:
        raise ValueError(opt)
    C = np.stack(cands)
    lo, hi = C.min(axis=0).astype(np.float64), C.max(axis=0).astype(np.float64)
    wmag = np.maximum(np.abs(lo[:, :d]), np.abs(hi[:, :d]))
    slack[:, :d] += 2 * (U32 * wmag + k * U32 * delta)
    return lo, hi, slack


def interval_use(got, lo, hi, slack) -> np.ndarray:
    """per element: how far `got` lies outside the span [lo, hi] of the candidate results, in units of the slack (<= 1:
    accepted; 0: inside the span).  An element with no slack (state the step does not touch) admits only the span."""
    got = np.asarray(got, np.float64)
    out = np.maximum(np.maximum(lo - got, got - hi), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(slack > 0, out / np.where(slack > 0, slack, 1), np.where(out == 0, 0.0, np.inf))
    r[np.isnan(got)] = np.inf
    return r


def bound_use(got, want, bound) -> np.ndarray:
    """|got - want| / bound per element (<= 1: within the bound)"""
    got = np.asarray(got, np.float64)
    r = np.abs(got - want) / bound
    r[np.isnan(got)] = np.inf
    return r


# ------------------------------------------------------------------------------------------------ the twin
class VecEmbeddingTwin:
    """Same contract as DictEmbeddingTwin (training inserts unseen keys through `init`, state = state_init; eval reads
    zeros for them and inserts nothing; every unique key of a batch is updated once with the sum -- MEAN: length-scaled --
    of its gradients, rounded once to the gradient dtype; Adam's step count is the number of backward calls), plus scores:
    `lfu` = occurrences summed over training forwards, `last` = the number of the training forward (from 0) that last
    touched the key.  `init(keys, dim) -> [len(keys), dim]` fp32 rows."""

    def __init__(self, dims: List[int], feature_table_map: List[int], pooling: str = "SUM", optimizer: str = "sgd",
                 lr: float = 0.01, eps: float = 1e-8, beta1: float = 0.9, beta2: float = 0.999, weight_decay: float = 0.0,
                 init: Callable[[np.ndarray, int], np.ndarray] = debug_rows, state_init: float = 0.0, grad_dtype: str = "f32"):
        self.dims, self.fmap, self.pooling, self.opt = list(dims), list(feature_table_map), pooling, optimizer
        self.grad_dtype = grad_dtype      # the reduced gradient is rounded once to it before the optimizer step
        self.hp = dict(lr=lr, eps=eps, beta1=beta1, beta2=beta2, weight_decay=weight_decay)
        self.init, self.state_init = init, state_init
        T = len(dims)
        self.keys = [np.empty(0, np.int64) for _ in range(T)]
        self.rows = [np.empty((0, d + _STATE[optimizer](d)), np.float32) for d in dims]
        self.lfu = [np.empty(0, np.int64) for _ in range(T)]
        self.last = [np.empty(0, np.int64) for _ in range(T)]
        self.step = 0        # training forwards so far
        self.iter = 0        # backward calls so far
        self._fwd = None
        self.last_grad: List[Optional[dict]] = [None] * T

    # ---- state
    def value_dim(self, t: int) -> int:
        return self.rows[t].shape[1]

    def size(self) -> int:
        return sum(k.size for k in self.keys)

    def _sort(self, t: int) -> None:
        o = np.argsort(self.keys[t], kind="stable")
        self.keys[t], self.rows[t] = self.keys[t][o], self.rows[t][o]
        self.lfu[t], self.last[t] = self.lfu[t][o], self.last[t][o]

    def load(self, t: int, keys, rows, score: int = 0) -> None:
        """store full rows [n, value_dim] of new keys (a checkpoint / _insert_rows) with score `score` in both scores"""
        keys = np.asarray(keys, np.int64)
        assert np.intersect1d(keys, self.keys[t]).size == 0 and np.unique(keys).size == keys.size
        self.keys[t] = np.concatenate([self.keys[t], keys])
        self.rows[t] = np.concatenate([self.rows[t], np.asarray(rows, np.float32).reshape(keys.size, -1)])
        self.lfu[t] = np.concatenate([self.lfu[t], np.full(keys.size, score, np.int64)])
        self.last[t] = np.concatenate([self.last[t], np.full(keys.size, score, np.int64)])
        self._sort(t)

    def find(self, t: int, keys) -> Tuple[np.ndarray, np.ndarray]:
        """(found, position) of keys in table t"""
        keys = np.asarray(keys, np.int64)
        K = self.keys[t]
        pos = np.searchsorted(K, keys)
        pc = np.minimum(pos, max(K.size - 1, 0))
        found = (pos < K.size) & (K[pc] == keys) if K.size else np.zeros(keys.size, bool)
        return found, pc

    def get_rows(self, t: int, keys) -> Tuple[np.ndarray, np.ndarray]:
        """(found, full rows) of keys (zeros where not found)"""
        f, p = self.find(t, keys)
        out = np.zeros((len(f), self.value_dim(t)), np.float32)
        out[f] = self.rows[t][p[f]]
        return f, out

    def set_rows(self, t: int, keys, rows) -> None:
        """overwrite the full rows of stored keys"""
        f, p = self.find(t, keys)
        assert f.all()
        self.rows[t][p] = np.asarray(rows, np.float32)

    # ---- batch layout
    def _layout(self, keys, offsets):
        F = len(self.fmap)
        offsets = np.asarray(offsets, np.int64)
        B = (offsets.size - 1) // F
        assert offsets.size == F * B + 1
        return F, B, offsets

    def _feature_keys(self, offsets, B, f):
        return int(offsets[f * B]), int(offsets[(f + 1) * B])

    def forward(self, keys, offsets, train: bool = True) -> np.ndarray:
        """pooled [B, sum of feature dims] or sequence [n, D] output in fp64; sets `abs_sum` (sum |terms| per element, MEAN:
        divided by the bag length) and `nterms` (terms per element, broadcastable to the output)"""
        keys = np.asarray(keys, np.int64)
        F, B, offsets = self._layout(keys, offsets)
        T = len(self.dims)
        # unique keys per table over all features of the table
        per_t = []
        for t in range(T):
            rng_ = [self._feature_keys(offsets, B, f) for f in range(F) if self.fmap[f] == t]
            sel = np.concatenate([keys[a:b] for a, b in rng_]) if rng_ else np.empty(0, np.int64)
            uk, inv, cnt = np.unique(sel, return_inverse=True, return_counts=True)
            found, pos = self.find(t, uk)
            if train and (~found).any():
                new = uk[~found]
                d = self.dims[t]
                init = np.asarray(self.init(new, d), np.float32).reshape(new.size, d)
                st = np.full((new.size, self.value_dim(t) - d), np.float32(self.state_init), np.float32)
                self.keys[t] = np.concatenate([self.keys[t], new])
                self.rows[t] = np.concatenate([self.rows[t], np.concatenate([init, st], axis=1)])
                self.lfu[t] = np.concatenate([self.lfu[t], np.zeros(new.size, np.int64)])
                self.last[t] = np.concatenate([self.last[t], np.zeros(new.size, np.int64)])
                self._sort(t)
                found, pos = self.find(t, uk)
            if train:
                self.lfu[t][pos] += cnt
                self.last[t][pos] = self.step
            E = np.zeros((uk.size, self.dims[t]), np.float32)
            E[found] = self.rows[t][pos[found], :self.dims[t]]
            per_t.append((uk, inv, cnt, E, rng_))
        # per feature: the rows of its keys
        cursor = [0] * T
        feat_rows = []
        for f in range(F):
            t = self.fmap[f]
            a, b = self._feature_keys(offsets, B, f)
            uk, inv, cnt, E, _ = per_t[t]
            feat_rows.append(E[inv[cursor[t]:cursor[t] + (b - a)]])
            cursor[t] += b - a
        if self.pooling == "NONE":
            out = np.concatenate(feat_rows).astype(np.float64) if F > 1 else feat_rows[0].astype(np.float64)
            self.abs_sum, self.nterms = np.abs(out), np.ones((out.shape[0], 1))
        else:
            col = np.concatenate([[0], np.cumsum([self.dims[t] for t in self.fmap])])
            out = np.zeros((B, int(col[-1])), np.float64)
            S = np.zeros_like(out)
            nt = np.zeros_like(out)
            for f in range(F):
                a, _ = self._feature_keys(offsets, B, f)
                lens = np.diff(offsets[f * B:(f + 1) * B + 1])
                nz = lens > 0
                starts = (offsets[f * B:(f + 1) * B] - a)[nz]
                R = feat_rows[f]
                c0, c1 = int(col[f]), int(col[f + 1])
                for j in range(0, c1 - c0, 64):          # (column blocks: bounded memory at 1 M keys x D = 256)
                    blk = R[:, j:j + 64].astype(np.float64)
                    if starts.size:
                        out[nz, c0 + j:c0 + j + blk.shape[1]] = np.add.reduceat(blk, starts, axis=0)
                        S[nz, c0 + j:c0 + j + blk.shape[1]] = np.add.reduceat(np.abs(blk), starts, axis=0)
                nt[:, c0:c1] = lens[:, None]
                if self.pooling == "MEAN":
                    out[nz, c0:c1] /= lens[nz, None]
                    S[nz, c0:c1] /= lens[nz, None]
            self.abs_sum, self.nterms = S, nt
        if train:
            self.step += 1
            self._fwd = (keys, offsets, B, per_t)
        return out

    def backward(self, grads) -> None:
        """apply the optimizer to every unique key of the last training forward once.  `grads`: the values the product
        receives (already in the gradient dtype), as any float array.  Sets `last_grad[t]` = dict(keys, cnt, abs_sum, s,
        rows_before) -- s the fp64 reduced gradient, abs_sum the sum of |terms| -- for the bracket of the row check; the
        rows are updated with the nominal gradient round_grad(s, grad_dtype)."""
        assert self._fwd is not None, "backward without a training forward"
        keys, offsets, B, per_t = self._fwd
        self._fwd = None
        self.iter += 1
        G = np.asarray(grads, np.float64)
        F, T = len(self.fmap), len(self.dims)
        mean = self.pooling == "MEAN"
        col = np.concatenate([[0], np.cumsum([self.dims[t] for t in self.fmap])])
        terms: List[List[np.ndarray]] = [[] for _ in range(T)]
        for f in range(F):
            t, d = self.fmap[f], self.dims[self.fmap[f]]
            a, b = self._feature_keys(offsets, B, f)
            if self.pooling == "NONE":
                terms[t].append(G[a:b, :d])
                continue
            lens = np.diff(offsets[f * B:(f + 1) * B + 1])
            gb = G[:, int(col[f]):int(col[f + 1])]
            if mean:
                gb = gb / np.maximum(lens, 1)[:, None]
            terms[t].append(np.repeat(gb, lens, axis=0))
        for t in range(T):
            uk, inv, cnt, _, _ = per_t[t]
            d = self.dims[t]
            if uk.size == 0:
                self.last_grad[t] = None
                continue
            X = np.concatenate(terms[t]) if len(terms[t]) > 1 else terms[t][0]
            order = np.argsort(inv, kind="stable")
            starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            Xs = X[order]
            s = np.add.reduceat(Xs, starts, axis=0)
            A = np.add.reduceat(np.abs(Xs), starts, axis=0)
            del Xs
            found, pos = self.find(t, uk)
            assert found.all()
            before = self.rows[t][pos].copy()
            self.last_grad[t] = dict(keys=uk, cnt=cnt, abs_sum=A, s=s, rows_before=before, mean=mean)
            self.rows[t][pos] = update_rows(self.opt, before, round_grad(s, self.grad_dtype), d, self.hp, self.iter)

    def row_bracket(self, t: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(keys, lo, hi, slack): every element of the rows the last backward updated lies in [lo - slack, hi + slack]
        whatever order the product summed in (grad_sum_error -> grad_interval -> update_bracket)"""
        lg = self.last_grad[t]
        err = grad_sum_error(lg["cnt"][:, None], lg["abs_sum"], lg["mean"])
        g_lo, _, g_hi = grad_interval(lg["s"], err, self.grad_dtype)
        return (lg["keys"],) + update_bracket(self.opt, lg["rows_before"], g_lo, g_hi, self.dims[t], self.hp, self.iter)

    def scores(self, t: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(sorted keys, lfu, last)"""
        return self.keys[t], self.lfu[t], self.last[t]
