"""CPU restatement in float64 of the HSTU norm family (group norm mul dropout, swish layer norm, RMS norm; forward and
backward), written from the specification in include/recsys_amd.h, with the magnitudes their error bounds need and the bounds
themselves.  The Philox masks, unit_roundoff, half_subnormal and worst are norm_twin's; inputs are upcast as they are.

Bounds (per element), in norm_twin's notation: u = unit roundoff of the dtype written, s = half its smallest subnormal,
h = 2^-24, A = mean_j |x_j| over the normalised extent, E = (n + 8) 2^-24 with n the length of that extent: the error of a
mean, a variance or a c1 / c2 summed in fp32 in any order.  Every term is a rounding or a summation order; no constant is
fitted to the kernels.

Group norm: the layer norm's bounds with D -> L (the extent is a head, n = L), a scalar w_h and b_h per head:
  exh    E (|xh| + rstd A)                                  the error of xh
  core   |w_h| exh + 2^-22 (|xh| |w_h| + |b_h|)             the error of gn before t = gn u
  mean   E A;   rstd   2 E rstd
  t      u |ref| + |u| core + s;  a kept element: that / (1 - p);  a dropped one: exactly 0
  u / x parts of a concat_ux output: (u + 2^-22) |ref| + s
  dx     u |ref| + E (rstd (|g| + |xh| mean|xh g| + mean|g|) + |extra|) + rstd exh (mean|xh g| + |c1|) + s
  du     u |ref| + |dt| core + 2^-22 |u part of a concat_ux gradient| + s
  dw_h   u |ref| + (N L + 1) h sum|gp xh| + sum(|gp| exh) + s     (N L addends of any order, one more rounding)
  db_h   u |ref| + (N L + 1) h sum|gp| + s

Swish layer norm (n = D; ln and core as the layer norm's).  sig = 1 / (1 + expf(-ln)) is the evaluation act_twin bounds:
4 h relative.  The error of ln reaches it through sig' = sig (1 - sig), whose own slope is at most 0.1:
  es     4 h sig + sig (1 - sig) core + 0.05 core^2 (+ 2^-126 where ln < -88 and expf overflows)
  y      u |ref| + |x| es + h |ref| + s                      (one product)
  eq     |dy x| (es + h) + 4 h |q|        q = ((dy x) sig) (1 - sig): es through sig and 1 - sig (sig + (1 - sig) = 1), the
                                          rounding of 1 - sig, three products
  eg     |w| eq + h |g|                   g = w q
  dx     u |ref| + the layer norm's dx terms with extra = dy sig + rstd (eg + |xh| mean(|xh| eg) + mean(eg)) + |dy| es + s
  dw     u |ref| + (N + 1) h sum|q xh| + sum(|q| exh + eq |xh|) + s
  db     u |ref| + (N + 1) h sum|q| + sum(eq) + s

RMS norm (n = D): the layer norm's bounds with the mean terms dropped (no A, no c2).  The reference has no PyTorch statement of
it; this twin rests on the formula rstd = 1 / sqrt(mean(x^2) + eps), y = x rstd w alone.
  exh    E |xh|
  rstd   2 E rstd
  y      u |ref| + |w| exh + 2^-22 |xh| |w| + s
  dx     u |ref| + E rstd (|g| + |xh| mean|xh g|) + rstd exh (mean|xh g| + |c1|) + s
  dw     u |ref| + (N + 1) h sum|dy xh| + sum(|dy| exh) + s
"""
from types import SimpleNamespace

import torch

from norm_twin import _masks, half_subnormal, keep_mask, unit_roundoff, worst  # noqa: F401  (keep_mask, worst: for the tests)

H32 = 2.0 ** -24


def _d(t):
    return None if t is None else t.detach().cpu().double()


def _eps32(eps):
    return float(torch.tensor(eps, dtype=torch.float32))


# ---- group norm mul dropout ----
def gn_mul_dropout_fwd(x, u, weight, bias, eps, p, training, concat_ux, num_heads, linear_dim, seed=0):
    """out ([N, D] or [N, 3 D]), mean / rstd [N H], and what the bounds need; head-shaped tensors are [N, H, L]"""
    X = _d(x)
    n, D = X.shape
    H, L = num_heads, linear_dim
    assert D == H * L
    st = SimpleNamespace(n=n, D=D, H=H, L=L, x=X, E=(L + 8) * H32, p=(p if training else 0.0))
    Xh = X.reshape(n, H, L)
    m = Xh.mean(2, keepdim=True)
    r = 1.0 / torch.sqrt(((Xh - m) ** 2).mean(2, keepdim=True) + _eps32(eps))
    st.m3, st.r3, st.xh = m, r, (Xh - m) * r
    st.mean, st.rstd = m.reshape(n * H), r.reshape(n * H)
    st.A = Xh.abs().mean(2, keepdim=True)
    st.exh = st.E * (st.xh.abs() + r * st.A)
    st.w, st.b = _d(weight).reshape(1, H, 1), _d(bias).reshape(1, H, 1)
    st.gn = st.xh * st.w + st.b
    st.core = st.w.abs() * st.exh + 2.0 ** -22 * (st.xh.abs() * st.w.abs() + st.b.abs())
    st.u = _d(u).reshape(n, H, L)
    st.t = st.gn * st.u
    st.f = _masks(seed, n, D, p, training, concat_ux)
    t2 = st.t.reshape(n, D)
    if concat_ux:
        U2 = st.u.reshape(n, D)
        st.undropped = torch.cat([U2, X, t2], 1)
        st.out = torch.cat([U2 * st.f[0], X * st.f[1], t2 * st.f[2]], 1)
        st.kept = torch.cat([f != 0 for f in st.f], 1)
    else:
        st.undropped, st.out, st.kept = t2, t2 * st.f[2], st.f[2] != 0
    return st


def gn_mul_dropout_bwd(dy, x, u, weight, bias, eps, p, training, concat_ux, num_heads, linear_dim, seed=0):
    st = gn_mul_dropout_fwd(x, u, weight, bias, eps, p, training, concat_ux, num_heads, linear_dim, seed)
    G, n, D, H, L = _d(dy), st.n, st.D, st.H, st.L
    sh = lambda t: t.reshape(n, H, L)   # noqa: E731
    if concat_ux:
        st.du_extra, st.extra, dt = sh(G[:, :D] * st.f[0]), sh(G[:, D:2 * D] * st.f[1]), sh(G[:, 2 * D:] * st.f[2])
    else:
        st.du_extra, st.extra, dt = torch.zeros(n, H, L, dtype=torch.float64), torch.zeros(n, H, L, dtype=torch.float64), sh(G * st.f[2])
    st.dt = dt
    st.du = (dt * st.gn + st.du_extra).reshape(n, D)
    gp = dt * st.u
    g = st.w * gp
    st.gp, st.g = gp, g
    st.c1, st.c2 = (st.xh * g).mean(2, keepdim=True), g.mean(2, keepdim=True)
    st.m_xhg, st.m_g = (st.xh * g).abs().mean(2, keepdim=True), g.abs().mean(2, keepdim=True)
    st.dx = ((g - (st.xh * st.c1 + st.c2)) * st.r3 + st.extra).reshape(n, D)
    st.dw, st.db = (gp * st.xh).sum((0, 2)), gp.sum((0, 2))
    st.dw_mag, st.db_mag = (gp * st.xh).abs().sum((0, 2)), gp.abs().sum((0, 2))
    st.dw_exh = (gp.abs() * st.exh).sum((0, 2))
    return st


def gn_bound_mean(st):
    return (st.E * st.A).reshape(-1)


def gn_bound_rstd(st):
    return 2 * st.E * st.rstd


def gn_bound_out(st, dtype, concat_ux=False):
    u, s, D = unit_roundoff(dtype), half_subnormal(dtype), st.D
    bt = ((u * st.t.abs() + st.u.abs() * st.core + s) / (1.0 - st.p)).reshape(st.n, D)
    if not concat_ux:
        return bt
    return torch.cat([(u + 2.0 ** -22) * st.out[:, :D].abs() + s, (u + 2.0 ** -22) * st.out[:, D:2 * D].abs() + s, bt], 1)


def gn_bound_dx(st, dtype):
    r = st.r3
    b = (st.E * (r * (st.g.abs() + st.xh.abs() * st.m_xhg + st.m_g) + st.extra.abs()) + r * st.exh * (st.m_xhg + st.c1.abs()))
    return unit_roundoff(dtype) * st.dx.abs() + b.reshape(st.n, st.D) + half_subnormal(dtype)


def gn_bound_du(st, dtype):
    b = st.dt.abs() * st.core + 2.0 ** -22 * st.du_extra.abs()
    return unit_roundoff(dtype) * st.du.abs() + b.reshape(st.n, st.D) + half_subnormal(dtype)


def gn_bound_dw(st, wdtype):
    return unit_roundoff(wdtype) * st.dw.abs() + (st.n * st.L + 1) * H32 * st.dw_mag + st.dw_exh + half_subnormal(wdtype)


def gn_bound_db(st, wdtype):
    return unit_roundoff(wdtype) * st.db.abs() + (st.n * st.L + 1) * H32 * st.db_mag + half_subnormal(wdtype)


# ---- layer-norm statistics of whole rows (swish), and without a mean (rms) ----
def _row_stats(x, eps, rms):
    X = _d(x)
    n, D = X.shape
    st = SimpleNamespace(n=n, D=D, x=X, E=(D + 8) * H32)
    if rms:
        m = torch.zeros(n, 1, dtype=torch.float64)
        r = 1.0 / torch.sqrt((X ** 2).mean(1, keepdim=True) + _eps32(eps))
        st.xh = X * r
        st.exh = st.E * st.xh.abs()
    else:
        m = X.mean(1, keepdim=True)
        r = 1.0 / torch.sqrt(((X - m) ** 2).mean(1, keepdim=True) + _eps32(eps))
        st.xh = (X - m) * r
        st.A = X.abs().mean(1, keepdim=True)
        st.exh = st.E * (st.xh.abs() + r * st.A)
    st.m2, st.r2, st.mean, st.rstd = m, r, m.reshape(n), r.reshape(n)
    return st


# ---- swish layer norm ----
def swish_fwd(x, weight, bias, eps):
    st = _row_stats(x, eps, False)
    st.w, st.b = _d(weight), _d(bias)
    st.ln = st.xh * st.w + st.b
    st.core = st.w.abs() * st.exh + 2.0 ** -22 * (st.xh.abs() * st.w.abs() + st.b.abs())
    st.sig = torch.sigmoid(st.ln)
    over = torch.where(st.ln < -88.0, torch.full_like(st.ln, 2.0 ** -126), torch.zeros_like(st.ln))
    st.es = 4 * H32 * st.sig + st.sig * (1 - st.sig) * st.core + 0.05 * st.core ** 2 + over
    st.y = st.sig * st.x
    return st


def swish_bwd(dy, x, weight, bias, eps):
    st = swish_fwd(x, weight, bias, eps)
    G = _d(dy)
    st.dy = G
    q = G * st.x * st.sig * (1 - st.sig)
    g = st.w * q
    st.q, st.g = q, g
    st.eq = (G * st.x).abs() * (st.es + H32) + 4 * H32 * q.abs()
    st.eg = st.w.abs() * st.eq + H32 * g.abs()
    st.c1, st.c2 = (st.xh * g).mean(1, keepdim=True), g.mean(1, keepdim=True)
    st.m_xhg, st.m_g = (st.xh * g).abs().mean(1, keepdim=True), g.abs().mean(1, keepdim=True)
    st.extra = G * st.sig
    st.dx = st.extra + (g - (st.xh * st.c1 + st.c2)) * st.r2
    st.dw, st.db = (q * st.xh).sum(0), q.sum(0)
    st.dw_mag, st.db_mag = (q * st.xh).abs().sum(0), q.abs().sum(0)
    st.dw_err, st.db_err = (q.abs() * st.exh + st.eq * st.xh.abs()).sum(0), st.eq.sum(0)
    return st


def bound_mean(st):
    return (st.E * st.A).reshape(-1)


def bound_rstd(st):
    return 2 * st.E * st.rstd


def swish_bound_y(st, dtype):
    return (unit_roundoff(dtype) + H32) * st.y.abs() + st.x.abs() * st.es + half_subnormal(dtype)


def swish_bound_dx(st, dtype):
    r = st.r2
    ln_terms = st.E * (r * (st.g.abs() + st.xh.abs() * st.m_xhg + st.m_g) + st.extra.abs()) + r * st.exh * (st.m_xhg + st.c1.abs())
    carried = r * (st.eg + st.xh.abs() * (st.xh.abs() * st.eg).mean(1, keepdim=True) + st.eg.mean(1, keepdim=True))
    return unit_roundoff(dtype) * st.dx.abs() + ln_terms + carried + st.dy.abs() * st.es + half_subnormal(dtype)


def swish_bound_dw(st, wdtype):
    return unit_roundoff(wdtype) * st.dw.abs() + (st.n + 1) * H32 * st.dw_mag + st.dw_err + half_subnormal(wdtype)


def swish_bound_db(st, wdtype):
    return unit_roundoff(wdtype) * st.db.abs() + (st.n + 1) * H32 * st.db_mag + st.db_err + half_subnormal(wdtype)


# ---- RMS norm ----
def rms_fwd(x, weight, eps):
    st = _row_stats(x, eps, True)
    st.w = _d(weight)
    st.y = st.xh * st.w
    return st


def rms_bwd(dy, x, weight, eps):
    st = rms_fwd(x, weight, eps)
    G = _d(dy)
    g = st.w * G
    st.dy, st.g = G, g
    st.c1 = (st.xh * g).mean(1, keepdim=True)
    st.m_xhg = (st.xh * g).abs().mean(1, keepdim=True)
    st.dx = (g - st.xh * st.c1) * st.r2
    st.dw = (G * st.xh).sum(0)
    st.dw_mag, st.dw_exh = (G * st.xh).abs().sum(0), (G.abs() * st.exh).sum(0)
    return st


def rms_bound_y(st, dtype):
    return unit_roundoff(dtype) * st.y.abs() + st.w.abs() * st.exh + 2.0 ** -22 * st.xh.abs() * st.w.abs() + half_subnormal(dtype)


def rms_bound_dx(st, dtype):
    r = st.r2
    return (unit_roundoff(dtype) * st.dx.abs() + st.E * r * (st.g.abs() + st.xh.abs() * st.m_xhg)
            + r * st.exh * (st.m_xhg + st.c1.abs()) + half_subnormal(dtype))


def rms_bound_dw(st, wdtype):
    return unit_roundoff(wdtype) * st.dw.abs() + (st.n + 1) * H32 * st.dw_mag + st.dw_exh + half_subnormal(wdtype)
