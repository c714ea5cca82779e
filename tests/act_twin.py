"""CPU restatement of the HSTU activation kernels (csrc/act_ops.hip) in float64: SiLU forward, SiLU backward with the column
sum, the element-wise bounds of their fp32 arithmetic, and an fp32 numpy emulation of that arithmetic as stated in
include/recsys_amd.h.  Inputs are upcast as they are.  unit_roundoff, half_subnormal and worst are norm_twin's.

The kernels compute in fp32
    e = expf(-z)                     at most 1 ulp (2 half-ulps) off, +inf when -z > 88.72...
    s   = z / (1 + e)                one add, one division: half an ulp each
    sig = 1 / (1 + e);  dz = (g sig) (1 + z (1 - sig))
and round each stored value once.  With h = 2^-24 (half an fp32 ulp, relative), u the unit roundoff of the dtype written and
sub half its smallest subnormal:

  s      1 + e carries (2 + 1) h relative, the division one more: |s - ref| <= 4 h |ref| before the rounding.  When e
         overflows (z < -88) the kernel gives 0 where |ref| = |z| / (1 + e) < |z| 2^-128.
         bound_s = u |ref| + 4 h |ref| + [z < -88] |z| 2^-127 + sub
  dz     sig: 4 h relative (as s), and an absolute 2^-128 where e overflows, far below h.  1 - sig: 4 h sig + h <= 5 h absolute.
         z (1 - sig): 5 h |z| + h |z| = 6 h |z|.  f = 1 + that: 6 h |z| + h (1 + |z|) <= 7 h (1 + |z|) absolute, |f| <= 1 + |z|.
         g sig: 5 h relative, |g sig| <= |g|.  The product: |g| 7 h (1 + |z|) + 6 h |g| (1 + |z|) = 13 h |g| (1 + |z|);
         16 h is used.  The term scales with |g| (1 + |z|), not with |dz|: f crosses zero near z = -1.2785, where the
         absolute error of f stays while dz vanishes.  Products that underflow lose at most 2^-149 (1 + |z|).
         bound_dz = u |ref| + 16 h |g| (1 + |z|) + 2^-149 (1 + |z|) + sub
  dbias  the form of norm_twin.bound_db: the rounding of the result, rows + 1 additions of fp32 numbers in any order, and the
         errors the addends (dz before its rounding) bring along:
         bound_dbias = u |ref| + (rows + 1) h sum |dz| + sum (16 h |g| (1 + |z|) + 2^-149 (1 + |z|)) + sub
Every bound is a function of float64 magnitudes of the inputs and the reference, never of the result under test.
"""
from types import SimpleNamespace

import numpy as np
import torch

from norm_twin import half_subnormal, unit_roundoff, worst  # noqa: F401  (worst: for the tests)

H32 = 2.0 ** -24


def sub(dtype):
    """half the smallest subnormal of the dtype (norm_twin's for fp16; bf16 and fp32 have theirs too, far lower)"""
    return max(half_subnormal(dtype), {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}[dtype])


def max_finite(dtype):
    return float(torch.finfo(dtype).max)


def edge_values(dtype):
    """the edge list of the issue, as the dtype holds it"""
    m = max_finite(dtype)
    vals = [0.0, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0, -1.2785, 20.0, -20.0, 89.0, -89.0, 1e4, -1e4, m, -m]
    return torch.tensor(vals, dtype=torch.float64).to(dtype)


def _d(t):
    return t.detach().cpu().double()


def _exp_neg(z):
    return torch.exp(-z)   # float64: +inf past 709, which the formulas below take as the limit


def silu_fwd(z):
    Z = _d(z)
    return SimpleNamespace(z=Z, s=Z / (1.0 + _exp_neg(Z)))


def silu_bwd(g, z):
    """dz and its column sum, with the magnitudes the bounds need"""
    G, Z = _d(g), _d(z)
    sig = 1.0 / (1.0 + _exp_neg(Z))
    zs = torch.where(sig == 1.0, torch.zeros_like(Z), Z * (1.0 - sig))   # (1 - sig is 0 at +max-finite: no 0 * inf)
    dz = G * sig * (1.0 + zs)
    core = 16 * H32 * G.abs() * (1.0 + Z.abs()) + 2.0 ** -149 * (1.0 + Z.abs())
    return SimpleNamespace(g=G, z=Z, dz=dz, core=core, dbias=dz.sum(0), dbias_mag=dz.abs().sum(0), dbias_core=core.sum(0))


def bound_s(st, dtype):
    over = torch.where(st.z < -88.0, st.z.abs() * 2.0 ** -127, torch.zeros_like(st.z))
    return unit_roundoff(dtype) * st.s.abs() + 4 * H32 * st.s.abs() + over + sub(dtype)


def bound_dz(st, dtype):
    return unit_roundoff(dtype) * st.dz.abs() + st.core + sub(dtype)


def bound_dbias(st, bdtype):
    rows = st.z.size(0)
    return unit_roundoff(bdtype) * st.dbias.abs() + (rows + 1) * H32 * st.dbias_mag + st.dbias_core + sub(bdtype)


# ---- the stated arithmetic in fp32 numpy ----
def _np32(t):
    return t.detach().cpu().float().numpy()


def _round(a32, dtype):
    """one rounding of fp32 values to the dtype (round to nearest even, as the kernels' stores)"""
    return torch.from_numpy(np.ascontiguousarray(a32)).to(dtype)


def emulate_silu_fwd(z, dtype):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        z32 = _np32(z)
        one = np.float32(1)
        return _round(z32 / (one + np.exp(-z32)), dtype)


def emulate_silu_bwd(g, z, dtype, bdtype, sig_rounding=None, drop_row=None):
    """(dz, dbias); sig_rounding: a dtype sig is rounded through first (a deliberate fault); drop_row: a row the column sum
    leaves out (another)"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        g32, z32 = _np32(g), _np32(z)
        one = np.float32(1)
        sig = one / (one + np.exp(-z32))
        if sig_rounding is not None:
            sig = torch.from_numpy(sig).to(sig_rounding).float().numpy()
        dz = (g32 * sig) * (one + z32 * (one - sig))
        rows = [r for r in range(dz.shape[0]) if r != drop_row]
        acc = np.zeros(dz.shape[1], dtype=np.float32)
        for r in rows:
            acc = acc + dz[r]
        return _round(dz, dtype), _round(acc, bdtype)
