"""CPU restatement of the HSTU layer norms in float64 (layer norm and layer-norm-mul-dropout, forward and backward), with
the magnitudes their error bounds need, the bounds themselves, and a numpy Philox4x32-10 that reproduces the keep masks of
csrc/norm_ops.hip bit for bit.  Written from the specification in include/recsys_amd.h; inputs are upcast as they are.

Bounds (per element).  u = unit roundoff of the dtype written (2^-8 bf16, 2^-11 fp16, 2^-24 fp32), s = half its smallest
subnormal (2^-25 fp16, else 0), E = (D + 8) 2^-24, A = mean_j |x_j| of the row, exh = E (|xh| + rstd A): the error of xh from
an fp32 mean and variance summed in any order.
  mean   E A
  rstd   2 E rstd
  y      u |ref| + |w| exh + 2^-22 (|xh| |w| + |b|) + s
  t      u |ref| + |u| (|w| exh + 2^-22 (|xh| |w| + |b|)) + s;  a kept element: that / (1 - p);  a dropped one: exactly 0
  u / x parts of a concat_ux output (this file's choice: a division by the fp32 1 - p, then the rounding):
         (u + 2^-22) |ref| + s
  dx     u |ref| + E (rstd (|g| + |xh| mean|xh g| + mean|g|) + |extra|) + rstd exh (mean|xh g| + |c1|) + s
         (extra: dx_accumulate, or the x part of a concat_ux gradient)
  dw     u |ref| + (N + 1) 2^-24 sum|gp xh| + sum(|gp| exh) + s        gp: the gradient that reaches ln (dy, or dt u)
  db     u |ref| + (N + 1) 2^-24 sum|gp| + s
  du     u |ref| + |dt| (|w| exh + 2^-22 (|xh| |w| + |b|)) + 2^-22 |u part of a concat_ux gradient| + s
"""
from types import SimpleNamespace

import numpy as np
import torch

_M32 = np.uint64(0xFFFFFFFF)


def unit_roundoff(dtype):
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}[dtype]


def half_subnormal(dtype):
    return 2.0 ** -25 if dtype == torch.float16 else 0.0


# ---- dropout masks ----
def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words; the 32 x 32 -> 64 products are taken in uint64"""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & _M32, (p0 >> sh) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
    return c0, c1, c2, c3


def philox_draws(seed, rows, D, which, row0=0):
    """uint32 [rows, D]: the draw of element (row0 + i, col) under mask `which`: key (seed low, seed high), counter
    (row low, row high, col >> 2, which), word col & 3"""
    nc = (D + 3) // 4
    r = np.arange(row0, row0 + rows, dtype=np.uint64)
    c0 = np.broadcast_to((r & _M32)[:, None], (rows, nc)).copy()
    c1 = np.broadcast_to((r >> np.uint64(32))[:, None], (rows, nc)).copy()
    c2 = np.broadcast_to(np.arange(nc, dtype=np.uint64)[None, :], (rows, nc)).copy()
    c3 = np.full((rows, nc), which, dtype=np.uint64)
    words = philox4x32(c0, c1, c2, c3, np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF))
    return np.stack(words, axis=2).reshape(rows, nc * 4)[:, :D].astype(np.uint32)


def keep_mask(seed, rows, D, which, p, row0=0):
    """bool tensor [rows, D]: kept iff draw >= floor(p 2^32)"""
    thr = int(p * 4294967296.0)
    return torch.from_numpy(philox_draws(seed, rows, D, which, row0).astype(np.int64) >= thr)


def _masks(seed, rows, D, p, training, concat_ux):
    """float64 factors keep / (1 - p) of the u / x / t parts (the t part alone without concat_ux)"""
    if not training or p == 0.0:
        one = torch.ones(rows, D, dtype=torch.float64)
        return one, one, one
    f = [keep_mask(seed, rows, D, w, p).double() / (1.0 - p) for w in ((0, 1, 2) if concat_ux else (0,))]
    return (f[0], f[1], f[2]) if concat_ux else (None, None, f[0])


# ---- the ops ----
def _d(t):
    return None if t is None else t.detach().cpu().double()


def _flat_u(u):
    u = _d(u)
    return u.reshape(u.size(0), u.numel() // u.size(0) if u.size(0) else int(torch.tensor(u.shape[1:]).prod()))


def _stats(x, eps, mean=None, rstd=None):
    X = _d(x)
    D = X.size(1)
    m = X.mean(1) if mean is None else _d(mean)
    e = float(torch.tensor(eps, dtype=torch.float32))
    r = 1.0 / torch.sqrt(((X - m[:, None]) ** 2).mean(1) + e) if rstd is None else _d(rstd)
    xh = (X - m[:, None]) * r[:, None]
    A = X.abs().mean(1) if D else X.sum(1)
    E = (D + 8) * 2.0 ** -24
    return SimpleNamespace(x=X, D=D, E=E, mean=m, rstd=r, xh=xh, A=A, exh=E * (xh.abs() + (r * A)[:, None]))


def _wb(w, b, D):
    return (torch.ones(D, dtype=torch.float64) if w is None else _d(w)), (torch.zeros(D, dtype=torch.float64) if b is None else _d(b))


def layer_norm_fwd(x, weight, bias, eps, mean=None, rstd=None):
    """y, mean, rstd and the per-element core |w| exh + 2^-22 (|xh| |w| + |b|) of the y bound"""
    st = _stats(x, eps, mean, rstd)
    w, b = _wb(weight, bias, st.D)
    st.w, st.b = w, b
    st.y = st.xh * w + b
    st.core = w.abs() * st.exh + 2.0 ** -22 * (st.xh.abs() * w.abs() + b.abs())
    return st


def _ln_bwd(st, gp, extra):
    """dx / dw / db of the layer norm for the gradient gp that reaches ln, with their magnitudes"""
    g = st.w * gp
    st.gp, st.g = gp, g
    st.c1, st.c2 = (st.xh * g).mean(1, keepdim=True), g.mean(1, keepdim=True)
    st.m_xhg, st.m_g = (st.xh * g).abs().mean(1, keepdim=True), g.abs().mean(1, keepdim=True)
    r = st.rstd[:, None]
    st.extra = torch.zeros_like(g) if extra is None else extra
    st.dx = (g - (st.xh * st.c1 + st.c2)) * r + st.extra
    st.dw, st.db = (gp * st.xh).sum(0), gp.sum(0)
    st.dw_mag, st.db_mag, st.dw_exh = (gp * st.xh).abs().sum(0), gp.abs().sum(0), (gp.abs() * st.exh).sum(0)
    return st


def layer_norm_bwd(dy, x, weight, eps, dx_accumulate=None, mean=None, rstd=None):
    st = layer_norm_fwd(x, weight, None, eps, mean, rstd)
    return _ln_bwd(st, _d(dy), _d(dx_accumulate))


def ln_mul_dropout_fwd(x, u, weight, bias, eps, p, training, concat_ux=False, seed=0):
    """y ([N, D] or [N, 3 D]), mean, rstd, and the float64 mask factors; `undropped` is y without dropout"""
    st = layer_norm_fwd(x, weight, bias, eps)
    U = _flat_u(u)
    st.u, st.p = U, (p if training else 0.0)
    st.f = _masks(seed, U.size(0), st.D, p, training, concat_ux)
    t = st.y * U
    st.t = t
    if concat_ux:
        st.undropped = torch.cat([U, st.x, t], 1)
        st.out = torch.cat([U * st.f[0], st.x * st.f[1], t * st.f[2]], 1)
        st.kept = torch.cat([f != 0 for f in st.f], 1)
    else:
        st.undropped, st.out, st.kept = t, t * st.f[2], st.f[2] != 0
    return st


def ln_mul_dropout_bwd(dy, x, u, weight, bias, eps, p, training, concat_ux=False, seed=0):
    st = ln_mul_dropout_fwd(x, u, weight, bias, eps, p, training, concat_ux, seed)
    G, D = _d(dy), st.D
    if concat_ux:
        st.du_extra, x_extra, dt = G[:, :D] * st.f[0], G[:, D:2 * D] * st.f[1], G[:, 2 * D:] * st.f[2]
    else:
        st.du_extra, x_extra, dt = torch.zeros_like(G), None, G * st.f[2]
    st.dt = dt
    st.du = dt * st.y + st.du_extra
    return _ln_bwd(st, dt * st.u, x_extra)


# ---- the bounds ----
def bound_mean(st):
    return st.E * st.A


def bound_rstd(st):
    return 2 * st.E * st.rstd


def bound_y(st, dtype):
    return unit_roundoff(dtype) * st.y.abs() + st.core + half_subnormal(dtype)


def bound_out(st, dtype, concat_ux=False):
    """bound of the ln_mul_dropout output at its kept elements (the dropped ones are compared with zero exactly)"""
    u, s = unit_roundoff(dtype), half_subnormal(dtype)
    bt = (u * st.t.abs() + st.u.abs() * st.core + s) / (1.0 - st.p)
    if not concat_ux:
        return bt
    D = st.D
    return torch.cat([(u + 2.0 ** -22) * st.out[:, :D].abs() + s, (u + 2.0 ** -22) * st.out[:, D:2 * D].abs() + s, bt], 1)


def bound_dx(st, dtype):
    r = st.rstd[:, None]
    return (unit_roundoff(dtype) * st.dx.abs() + st.E * (r * (st.g.abs() + st.xh.abs() * st.m_xhg + st.m_g) + st.extra.abs())
            + r * st.exh * (st.m_xhg + st.c1.abs()) + half_subnormal(dtype))


def bound_dw(st, wdtype):
    n = st.x.size(0)
    return unit_roundoff(wdtype) * st.dw.abs() + (n + 1) * 2.0 ** -24 * st.dw_mag + st.dw_exh + half_subnormal(wdtype)


def bound_db(st, wdtype):
    n = st.x.size(0)
    return unit_roundoff(wdtype) * st.db.abs() + (n + 1) * 2.0 ** -24 * st.db_mag + half_subnormal(wdtype)


def bound_du(st, dtype):
    return (unit_roundoff(dtype) * st.du.abs() + st.dt.abs() * st.core + 2.0 ** -22 * st.du_extra.abs()
            + half_subnormal(dtype))


def worst(got, ref, bound):
    """largest |got - ref| / bound over the elements (0 for an empty tensor); a zero bound asks for equality"""
    if ref.numel() == 0:
        return 0.0
    err = (got.detach().cpu().double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, 0.0, float("inf")))
    return float(ratio.max())
