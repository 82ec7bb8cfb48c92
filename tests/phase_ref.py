"""
Shared by tests/test_gpu_phase_functions.py and tests/test_phase_tables_host.py: the table sets, the probe points, a float64 reference of
the phase-function routines of er3t_amd/csrc/mi3d_device.h on float32 tables, a numpy restatement of build_tables / build_idx
(er3t_amd/csrc/mi3d_api.hip) and a correctly rounded float32 emulation of the lean kernels' formulas.  Nothing here touches a GPU.

Conventions: a table set is (ang [nang] float32 ascending degrees, pha [npf, nang] float32), what Mi3dSolver.set_phase takes.  Tables are
(mu [nang], p [npf, nang], cdf [npf, nang]) float32, mu ascending.  A table is numbered from 0; selector apf = 1 + table (+ fraction).
"""
import functools

import numpy as np

F32 = np.float32
EPS = 2.0**-24          # half an ulp of 1: the unit of the bounds
NB = 512                # buckets of the indices (kTabNB)
NIDX = NB + 2           # entries per index (kTabIdxN)
U_MIN, U_MAX = F32(2.0**-24), F32(1.0 - 2.0**-24)     # the extreme uniform numbers the kernels draw (u01)


# ----------------------------------------------------------------------------------------------
# table sets
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_set(name):
    if name == 'A':        # the reference's default grid of 498 angles, four droplet sizes
        from er3t_amd.synth import pha_mie_synth
        pm = pha_mie_synth()
        ang, pha = pm.data['ang']['data'], pm.data['pha']['data'].T
    elif name == 'B2':     # the smallest table there is
        ang, pha = np.array([0.0, 180.0]), np.array([[1.0, 1.0], [3.0, 0.0]])
    elif name == 'B3':
        ang, pha = np.array([0.0, 90.0, 180.0]), np.array([[5.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    elif name == 'C':      # uniform grid: smooth, zero over a range (runs of equal CDF nodes), nine decades of contrast
        ang = np.linspace(0.0, 180.0, 721)
        mu = np.cos(np.deg2rad(ang))
        pha = np.stack([(1.0-0.49)/(1.0+0.49-1.4*mu)**1.5, np.where((ang > 60.0) & (ang < 120.0), 0.0, 1.0), np.where(ang < 1.0, 1.0e6, 1.0e-3)])
    elif name == 'D':      # finer than float32 resolves near mu = 1: zero-width intervals of the float32 mu grid
        ang = np.concatenate((np.arange(1000)*0.001, np.arange(1.0, 180.25, 0.5)))
        pha = (np.exp(-0.5*(ang/0.5)**2)*1.0e4 + 1.0)[None]
    elif name == 'BIG':    # does not fit the LDS of a launch
        ang = np.linspace(0.0, 180.0, 8001)
        pha = np.ones((2, ang.size))
    else:
        raise KeyError(name)
    ang = np.ascontiguousarray(ang, dtype=F32); pha = np.ascontiguousarray(pha, dtype=F32)
    ang.setflags(write=False); pha.setflags(write=False)
    return ang, pha


SETS = ('A', 'B2', 'B3', 'C', 'D')


def staged_ranges(npf):
    """the (tab_lo, tab_n) the staged paths are tried with, those that exist for npf tables"""
    out = []
    for lo, n in ((0, npf), (1, npf-1), (npf-1, 1), (2, 1)):
        if lo >= 0 and n >= 1 and lo+n <= npf and (lo, n) not in out:
            out.append((lo, n))
    return out


# ----------------------------------------------------------------------------------------------
# build_tables / build_idx restated
# ----------------------------------------------------------------------------------------------
def build_tables_np(ang, pha):
    """float64 restatement of build_tables: (mu, p, cdf) float64 before the cast, and the float32 tables"""
    ang = np.asarray(ang, dtype=F32).astype(np.float64)
    pha = np.atleast_2d(np.asarray(pha, dtype=F32)).astype(np.float64)
    mu = np.cos(ang[::-1]*np.pi/180.0)
    mu[0], mu[-1] = -1.0, 1.0
    if not np.all(np.diff(mu) > 0.0):
        raise ValueError('phase-function angles must ascend strictly from 0 to 180')
    p = pha[:, ::-1].copy()
    dmu = np.diff(mu)
    tot = (0.25*(p[:, 1:]+p[:, :-1])*dmu).sum(axis=1)
    p /= tot[:, None]
    cdf = np.zeros_like(p)
    cdf[:, 1:] = np.cumsum(0.25*(p[:, 1:]+p[:, :-1])*dmu, axis=1)
    cdf[:, -1] = 1.0
    return (mu, p, cdf), (mu.astype(F32), p.astype(F32), cdf.astype(F32))


def bucket_mu(x):
    """tab_bucket_mu: (int)(fmaf(mu, 0.5f, 0.5f) * 512) clipped -- the fused multiply-add rounds once: mu/2 is exact in float64, the sum
    rounds there at 2^-53 and once more to float32, which differs from a single rounding only at a tie no float32 mu/2 + 1/2 can produce
    (its bits below 2^-53 are lost only when |mu| < 2^-28, far from any tie of a float32 near 1/2)"""
    f = (np.asarray(x, dtype=F32).astype(np.float64)*0.5 + 0.5).astype(F32)
    return np.clip(np.trunc(f.astype(np.float64)*NB), 0, NB-1).astype(np.int64)


def bucket_u(x):
    """tab_bucket_u: (int)(u * 512) clipped (the product by a power of two is exact)"""
    return np.clip(np.trunc(np.asarray(x, dtype=F32).astype(np.float64)*NB), 0, NB-1).astype(np.int64)


def index_np(nodes, bucket):
    """what build_idx must leave: entry b <= 512 = the last node whose bucket is below b, clipped to [0, n - 2]; entry 513 = entry 512"""
    bk = bucket(nodes)
    assert np.all(np.diff(bk) >= 0)
    out = np.zeros(NIDX, dtype=np.int64)
    out[:NB+1] = np.clip(np.searchsorted(bk, np.arange(NB+1), side='left') - 1, 0, nodes.size-2)
    out[NB+1:] = out[NB]
    return out


def lean_tab_find_np(a, idx, x, b):
    """lean_tab_find, operation by operation, over arrays of probes x with buckets b"""
    n = a.size
    lo = idx[b].astype(np.int64)
    hi = np.minimum(idx[b+1].astype(np.int64)+1, n-1)
    a1, a2 = a[np.minimum(lo+1, n-1)], a[np.minimum(lo+2, n-1)]
    step = np.where((lo+1 < hi) & (a1 <= x), np.where((lo+2 < hi) & (a2 <= x), 2, 1), 0)
    lo = lo + step
    more = (hi-lo > 1) & (a[np.minimum(lo+1, n-1)] <= x)
    h2 = np.where(more, hi, lo+1)
    lo = np.where(more, lo+1, lo)
    while True:
        act = h2-lo > 1
        if not act.any():
            break
        mid = (lo+h2) >> 1
        up = act & (a[mid] <= x)
        dn = act & ~up
        lo = np.where(up, mid, lo); h2 = np.where(dn, mid, h2)
    return lo


# ----------------------------------------------------------------------------------------------
# probe points
# ----------------------------------------------------------------------------------------------
def _neighbours(v, k):
    """v and its +-1 .. +-k float32 neighbours"""
    v = np.asarray(v, dtype=F32)
    out = [v]
    up, dn = v, v
    for _ in range(k):
        up = np.nextafter(up, F32(np.inf)); dn = np.nextafter(dn, F32(-np.inf))
        out += [up, dn]
    return np.concatenate(out)


def mu_points(mu, beyond):
    """cosines to evaluate a table at: every node and its +-1, +-2 neighbours, every bucket edge and its +-1, +-2 neighbours, -1 and 1,
    4096 random ones -- clipped to [-1, 1], the domain -- and, where the routine takes them (beyond), +-(1 + 2^-23)"""
    rng = np.random.default_rng(20260101)
    edges = (-1.0 + 2.0*np.arange(NB+1)/NB).astype(F32)
    x = np.concatenate([_neighbours(mu, 2), _neighbours(edges, 2), F32([-1.0, 1.0]), rng.uniform(-1.0, 1.0, 4096).astype(F32)])
    x = np.clip(x, F32(-1.0), F32(1.0))
    if beyond:
        x = np.concatenate([x, F32([-(1.0+2.0**-23), 1.0+2.0**-23])])
    return np.ascontiguousarray(x, dtype=F32)


def u_points(cdf_t):
    """uniform numbers to sample one table with: every CDF node and its +-1, +-2 neighbours, every bucket edge and its +-1, +-2 neighbours,
    the extreme values the kernels draw, 4096 random ones; clipped to [2^-24, 1 - 2^-24], the range of the kernels' uniform numbers"""
    rng = np.random.default_rng(20260102)
    edges = (np.arange(NB+1)/NB).astype(F32)
    x = np.concatenate([_neighbours(cdf_t, 2), _neighbours(edges, 2), F32([U_MIN, U_MAX]), rng.uniform(0.0, 1.0, 4096).astype(F32)])
    return np.ascontiguousarray(np.clip(x, U_MIN, U_MAX), dtype=F32)


def selectors(npf):
    """[(apf, usel)]: every table, one beyond the last (clamps), k + 1/2 and k + 2^-20 below the last table with usel around the fraction"""
    out = [(F32(k), F32(0.0)) for k in range(1, npf+1)] + [(F32(npf+3), F32(0.0))]
    for k in range(1, npf):
        for fr in (F32(0.5), F32(2.0**-20)):
            for us in (F32(0.0), np.nextafter(fr, F32(0.0)), fr, np.nextafter(fr, F32(1.0))):
                out.append((F32(k)+fr, us))
    return out


def pick(apf, usel, npf):
    """table_pick + the choice of the sampler: (first table, fraction of the next one, table sampled)"""
    t = F32(apf) - F32(1.0)
    i = int(np.floor(t))
    fr = F32(t - F32(i))
    if i < 0:
        i, fr = 0, F32(0.0)
    if i >= npf-1:
        i, fr = npf-1, F32(0.0)
    return i, fr, (i+1 if (fr > 0.0 and usel < fr) else i)


def tables_touched(apf, npf):
    i, fr, _ = pick(apf, 0.0, npf)
    return (i, i+1) if fr > 0.0 else (i, i)


# ----------------------------------------------------------------------------------------------
# float64 reference on float32 tables
# ----------------------------------------------------------------------------------------------
def interval(nodes, x):
    """the interval of a point: searchsorted(side='right') - 1 on the float32 values, clipped to [0, n - 2] (exact)"""
    return np.clip(np.searchsorted(nodes, np.asarray(x, dtype=F32), side='right') - 1, 0, nodes.size-2)


def eval_ref(mu, p_t, x):
    """(P_ref, lo, zero): the piecewise-linear table at x (clamped into the grid) in float64.  zero marks the points whose interval has
    no width in float32 (x at the grid's end, the last nodes equal): there P_ref is NaN and (plo, phi) of eval_hull bound the value"""
    m = mu.astype(np.float64); p = p_t.astype(np.float64)
    xc = np.clip(np.asarray(x, dtype=F32), mu[0], mu[-1])
    lo = interval(mu, xc)
    w = m[lo+1]-m[lo]
    zero = w == 0.0
    f = np.where(zero, 0.0, (xc.astype(np.float64)-m[lo])/np.where(zero, 1.0, w))
    ref = p[lo] + f*(p[lo+1]-p[lo])
    return np.where(zero, np.nan, ref), lo, zero


def eval_hull(mu, p_t, x):
    """smallest and largest table value over the nodes whose float32 cosine equals x clamped into the grid (the graph of the float32
    table is vertical there), for the points eval_ref marks"""
    xc = np.clip(np.asarray(x, dtype=F32), mu[0], mu[-1])
    a = np.searchsorted(mu, xc, side='left'); b = np.searchsorted(mu, xc, side='right')
    lo_v = np.array([p_t[i:j].min() if j > i else np.nan for i, j in zip(a, b)], dtype=np.float64)
    hi_v = np.array([p_t[i:j].max() if j > i else np.nan for i, j in zip(a, b)], dtype=np.float64)
    return lo_v, hi_v


def sample_ref(mu, p_t, cdf_t, u):
    """(mu_ref, lo, zero): exact inversion of the table's CDF inside the interval of u, float64 on the float32 tables"""
    m = mu.astype(np.float64); p = p_t.astype(np.float64); c = cdf_t.astype(np.float64)
    u = np.asarray(u, dtype=F32)
    lo = interval(cdf_t, u)
    dm = m[lo+1]-m[lo]
    zero = dm == 0.0
    r = 2.0*(u.astype(np.float64)-c[lo])
    sl = np.where(zero, 0.0, (p[lo+1]-p[lo])/np.where(zero, 1.0, dm))
    disc = np.maximum(p[lo]*p[lo] + 2.0*sl*r, 0.0)
    den = p[lo] + np.sqrt(disc)
    t = np.where(den > 0.0, 2.0*r/np.where(den > 0.0, den, 1.0), 0.0)
    return np.clip(m[lo]+t, m[lo], m[lo+1]), lo, zero


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(F32)).astype(np.float64)


def eval_bound(p_t, lo):
    return 8.0*EPS*np.maximum(p_t[lo], p_t[lo+1]).astype(np.float64)


def sample_bound(mu, ref, lo):
    return 2.0*ulp32(ref) + 16.0*EPS*(ref - mu[lo].astype(np.float64))


# ----------------------------------------------------------------------------------------------
# correctly rounded float32 emulation of lean_phase_eval / lean_table_sample
# ----------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.astype(np.float64)*b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _rcp32(a):
    with np.errstate(divide='ignore'):
        return (1.0/a.astype(np.float64)).astype(F32)


def eval_emul(mu, p_t, x, lo):
    """lean_phase_eval's arithmetic for one table in float32, every operation rounded once, on the interval lo"""
    xc = np.clip(np.asarray(x, dtype=F32), F32(-1.0), F32(1.0))
    with np.errstate(invalid='ignore', over='ignore'):
        f = np.fmin((xc-mu[lo])*_rcp32(mu[lo+1]-mu[lo]), F32(1.0))      # (fminf: 0 x inf on an interval without width gives 1)
        return _fma32(f, p_t[lo+1]-p_t[lo], p_t[lo])


def sample_emul(mu, p_t, cdf_t, u, lo):
    """lean_table_sample's arithmetic in float32, every operation rounded once, on the interval lo"""
    u = np.asarray(u, dtype=F32)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        r = F32(2.0)*(u-cdf_t[lo])
        dm = mu[lo+1]-mu[lo]
        sl = (p_t[lo+1]-p_t[lo])*_rcp32(dm)
        disc = np.fmax(_fma32(p_t[lo], p_t[lo], F32(2.0)*sl*r), F32(0.0))      # (fmaxf: a NaN operand gives the other one)
        den = p_t[lo] + np.sqrt(disc)
        t = np.where(den > 0.0, F32(2.0)*r*_rcp32(den), F32(0.0)).astype(F32)
        return np.fmin(mu[lo]+t, mu[lo+1])


# ----------------------------------------------------------------------------------------------
# analytic phase functions (apf < 1): float64 and float32 emulation, class boundaries as the code draws them
# ----------------------------------------------------------------------------------------------
_HG = (0.0009, 0.0011, 0.05, 0.5, 0.6, 0.85, 0.99)
ANALYTIC_SELECTORS = tuple(F32(v) for v in (-2.0, -1.5, -1.25, -1.0) + _HG + tuple(-g for g in _HG))


def analytic_class(apf):
    apf = F32(apf)
    if apf <= F32(-1.5):
        return 'iso'
    if apf <= F32(-1.0):
        return 'ray'
    return 'hg'


def analytic_points():
    """(mu, u): 4001-point grids and 1 - 10^-k, k = 1 .. 8, from both ends (u inside the kernels' range of uniform numbers)"""
    tail = 10.0**-np.arange(1, 9)
    mu = np.concatenate([np.linspace(-1.0, 1.0, 4001), 1.0-tail, -1.0+tail]).astype(F32)
    u = np.clip(np.concatenate([(np.arange(4001)+0.5)/4001.0, 1.0-tail, tail]).astype(F32), U_MIN, U_MAX)
    return mu, u


def analytic_eval(apf, mu, dtype):
    """P(apf, mu) with the formulas of phase_eval_analytic in `dtype` arithmetic (float32: every operation rounded once)"""
    T = dtype
    a = T(F32(apf)); x = np.asarray(mu, dtype=F32).astype(T)
    kind = analytic_class(apf)
    if kind == 'iso':
        return np.ones_like(x)
    if kind == 'ray':
        return T(0.75)*(T(1.0)+x*x)
    d = T(1.0)+a*a-T(2.0)*a*x
    if T is F32:
        r = (1.0/np.sqrt(d.astype(np.float64))).astype(F32)
    else:
        r = 1.0/np.sqrt(d)
    return (T(1.0)-a*a)*r*r*r


def analytic_sample(apf, u, dtype):
    """mu(apf, u) with the formulas of phase_sample_analytic in `dtype` arithmetic; |g| < 1e-3 (float32 comparison) samples isotropically"""
    T = dtype
    a = T(F32(apf)); x = np.asarray(u, dtype=F32).astype(T)
    kind = analytic_class(apf)
    if kind == 'iso' or (kind == 'hg' and abs(F32(apf)) < F32(1e-3)):
        return T(2.0)*x-T(1.0)
    if kind == 'ray':
        q = T(8.0)*x-T(4.0)
        s = T(0.5)*q + np.sqrt(T(0.25)*q*q+T(1.0))
        c = np.exp2(np.log2(s)*T(F32(1.0/3.0)))
        return c - T(1.0)/c
    t = (T(1.0)-a*a)*(T(1.0)/(T(1.0)-a+T(2.0)*a*x))
    m = (T(1.0)+a*a-t*t)*(T(1.0)/(T(2.0)*a))
    return np.clip(m, T(-1.0), T(1.0))


def analytic_bounds(apf, mu, u):
    """(bound on |P - P64| / P64, bound on |mu - mu64|, P64, mu64) of one selector: max(4 E_emul, 8 2^-24), E_emul the float32
    emulation's largest deviation from float64 over the group's points"""
    p64 = analytic_eval(apf, mu, np.float64); m64 = analytic_sample(apf, u, np.float64)
    e_p = np.max(np.abs(analytic_eval(apf, mu, F32).astype(np.float64)-p64)/p64)
    e_m = np.max(np.abs(analytic_sample(apf, u, F32).astype(np.float64)-m64))
    return max(4.0*e_p, 8.0*EPS), max(4.0*e_m, 8.0*EPS), p64, m64
