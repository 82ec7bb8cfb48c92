"""
Shared by tests/test_gpu_device_geometry.py and tests/test_device_geometry_host.py: the probe points, float64 references, correctly rounded
float32 emulations and the bounds for rotate_dir / sincos_turns and for the surface routines (surface_R, lsrt_R, dsm_R, fresnel_unpolarised,
dsm_shadow_lambda) of er3t_amd/csrc/mi3d_device.h.  Everything is deterministic (fixed generator seeds); nothing here touches a GPU.

Conventions: a direction is a row (x, y, z) of float32; `din` travels downward onto the surface (z < 0), `dout` leaves it (z > 0).  The
references take the float32 inputs as exact numbers.  EPS = 2^-24, half an ulp of 1, is the unit of the bounds.

The reflectance formulas are written once for three uses (`mode`):
  'ref'     float64, the formula itself (sin(acos x), pi, sqrt(pi)), with the guards at the float32 constants the device compares against
  'oracle'  float64 with the guards of oracle/mi3d_oracle.c (double constants; the Fresnel clamp at 1e-9): what the host test holds to the
            oracle's C code within 1e-12
  'emul'    float32, every operation rounded once, in the order and form of mi3d_device.h (sqrt(1 - x^2) for sin(acos x), the float32
            constants); acos / exp / erfc correctly rounded.  No fused multiply-add, exact division and square root: the device's
            contractions and 1-ulp rcp / rsq / sqrt are what the factor between E_emul and a bound allows for.
"""
import functools

import numpy as np
from scipy.special import erfc as _erfc

F32 = np.float32
F64 = np.float64
EPS = 2.0**-24
PI = np.pi

# sincos_turns (v_sin_f32 / v_cos_f32 on an angle in turns) against float64: the largest |error| MEASURED on an MI355X over the points of
# sincos_points() (profiles/r16/device_geometry_tests.log), and the bound the tests use: twice that.  The bound may not exceed E_SC_CAP: an
# azimuth error of 2^-16 moves a direction by ten times its own float32 resolution.
E_SC_MEASURED = 1.2418e-07      # = 2^-22.94, the cosine of u = 0.0078061223; 200032 points
E_SC = 2.0*E_SC_MEASURED
E_SC_CAP = 2.0**-16

N_ROT = 200000       # points per rotation class
N_SFC = 100000       # points per surface direction class
A_ROT, B_ROT = 32.0, 4.0      # |new - ref| <= A_ROT EPS + B_ROT EPS st / h2 + st E_SC where h2 >= H2_MODEL
H2_MODEL = 40.0*EPS
ONE_M = F32(1.0 - 2.0**-24)   # the float32 below 1
TINY = 2.0**-100              # added to the scale of a quantity that may underflow in float32 (exp(-x) beyond x = 87): no relative bound below it

MU_SPECIAL = F32([1.0, -1.0, ONE_M, -ONE_M, 0.0])
UPHI_SPECIAL = F32([2.0**-25, 0.25, 0.5, 0.75, ONE_M])      # 2^-25 = 2^-24 x 0.5: the smallest number u01 draws


def _u01(rng, n):
    """uniform numbers as the kernels draw them: (k + 0.5) 2^-23, exact in float32"""
    return ((rng.integers(0, 2**23, n).astype(F64) + 0.5)*2.0**-23).astype(F32)


def normalise32(d):
    """d (n, 3) float32 scaled to unit length the way rotate_dir's last step does it, every operation in float32"""
    d = np.asarray(d, dtype=F32)
    s = (d[:, 0]*d[:, 0] + d[:, 1]*d[:, 1]) + d[:, 2]*d[:, 2]
    n = (F32(1.0)/np.sqrt(s)).astype(F32)
    return np.ascontiguousarray(d*n[:, None], dtype=F32)


# ----------------------------------------------------------------------------------------------
# rotate_dir, sincos_turns
# ----------------------------------------------------------------------------------------------
def _mu_uphi(rng, n):
    mu = (F32(2.0)*_u01(rng, n) - F32(1.0)).astype(F32)
    uphi = _u01(rng, n)
    k = n//20
    for j, v in enumerate(MU_SPECIAL):
        mu[j*k:(j+1)*k] = v
    i = np.arange(n)
    for j, v in enumerate(UPHI_SPECIAL):      # (every special azimuth meets every special cosine: the pattern runs through the blocks above)
        uphi[i % 11 == j] = v
    return mu, uphi


def _sph(th, az, sign):
    return np.stack([np.sin(th)*np.cos(az), np.sin(th)*np.sin(az), sign*np.cos(th)], axis=1)


RINGS = (0.3, 0.1, 0.03, 0.01, 3.0e-3, 1.6e-3)
ROT_CLASSES = ('general',) + tuple('ring_%g' % t for t in RINGS) + ('band', 'poles', 'axes', 'short')


@functools.lru_cache(maxsize=None)
def rotate_points(name):
    """(dirs (n, 3), mu (n,), uphi (n,)) float32 of one class, both hemispheres; directions normalised in float32 except where the class says"""
    n = N_ROT
    rng = np.random.default_rng(1000 + ROT_CLASSES.index(name))
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    az = rng.uniform(0.0, 2.0*PI, n)
    if name == 'general':
        d = normalise32(_sph(np.arccos(rng.uniform(0.0, 1.0, n)), az, sign))
    elif name.startswith('ring_'):          # at this angle from either pole
        d = normalise32(_sph(np.full(n, float(name[5:])), az, sign))
    elif name == 'band':                    # 2 EPS < h2 < 40 EPS: between the pole branch and where the model bound holds
        h2 = np.exp(rng.uniform(np.log(2.0*EPS), np.log(40.0*EPS), n))
        d = normalise32(_sph(np.sqrt(h2), az, sign))
    elif name == 'poles':
        d = np.zeros((n, 3), dtype=F32); d[:, 2] = sign
    elif name == 'axes':                    # on an axis in x and in y, both senses
        d = np.zeros((n, 3), dtype=F32)
        i = np.arange(n)
        d[i, (i//2) % 2] = sign
    elif name == 'short':                   # vertical and one ulp short of unit length
        d = np.zeros((n, 3), dtype=F32); d[:, 2] = sign*ONE_M
        i = np.arange(n)//2 % 4              # ... a quarter of them with a horizontal part below the pole branch's 1e-10, a quarter just above it
        d[i == 1, 0] = F32(3e-11); d[i == 1, 1] = F32(-1e-15); d[i == 2, 1] = F32(-3e-10)
    else:
        raise KeyError(name)
    mu, uphi = _mu_uphi(rng, n)
    for a in (d, mu, uphi):
        a.setflags(write=False)
    return d, mu, uphi


@functools.lru_cache(maxsize=None)
def zero_vector_points():
    """(0, 0, +0) and (0, 0, -0): no direction at all.  It has no horizontal part, so it takes the pole branch, where `uz >= 0.0f` reads
    both zeros as the upper pole: the contract is (st cos, st sin, +mu).  Returns dirs, mu, uphi, and that direction in float64"""
    n = 20000
    rng = np.random.default_rng(1999)
    d = np.zeros((n, 3), dtype=F32); d[1::2, 2] = F32(-0.0)
    mu, uphi = _mu_uphi(rng, n)
    m = mu.astype(F64); phi = 2.0*PI*uphi.astype(F64)
    st = np.sqrt(np.maximum(0.0, 1.0 - m*m))
    want = np.stack([st*np.cos(phi), st*np.sin(phi), m], axis=1)
    for a in (d, mu, uphi, want):
        a.setflags(write=False)
    return d, mu, uphi, want


def pole_branch(d):
    """where rotate_dir takes its pole branch: den2 = 1 - uz^2 rounds to 0 (|uz| = 1 in float32: 1 - 2^-24 already leaves 2^-23), or the
    direction has no horizontal part (both components below 1e-10 in size)"""
    d = np.asarray(d, dtype=F32)
    return (np.abs(d[:, 2]) >= F32(1.0)) | (np.maximum(np.abs(d[:, 0]), np.abs(d[:, 1])) < F32(1e-10))


def rotate_ref(d, mu, uphi):
    """float64 reference of a rotation.  Returns a dict: `u` the input normalised in float64, `h2` its squared horizontal part, `st`,
    `new` the rotated direction with the frame taken from (ux, uy) (e1 = (ux uz, uy uz, -h^2) / h, e2 = (-uy, ux, 0) / h; NaN where h = 0),
    `new_pole` the rotation about the exact axis sign(uz) z with the device's azimuth origin: (st cos, st sin, mu sign(uz))"""
    u = np.asarray(d, dtype=F64)
    u = u/np.linalg.norm(u, axis=1)[:, None]
    m = np.asarray(mu, dtype=F64)
    phi = 2.0*PI*np.asarray(uphi, dtype=F64)
    st = np.sqrt(np.maximum(0.0, 1.0 - m*m))
    cp, sp = np.cos(phi), np.sin(phi)
    h2 = u[:, 0]**2 + u[:, 1]**2
    h = np.sqrt(h2)
    with np.errstate(divide='ignore', invalid='ignore'):
        e1 = np.stack([u[:, 0]*u[:, 2]/h, u[:, 1]*u[:, 2]/h, -h], axis=1)
        e2 = np.stack([-u[:, 1]/h, u[:, 0]/h, np.zeros_like(h)], axis=1)
        new = st[:, None]*(cp[:, None]*e1 + sp[:, None]*e2) + m[:, None]*u
    sg = np.where(u[:, 2] >= 0.0, 1.0, -1.0)
    new_pole = np.stack([st*cp, st*sp, m*sg], axis=1)
    nrm = np.linalg.norm(new_pole, axis=1)
    new_pole = new_pole/np.where(nrm > 0.0, nrm, 1.0)[:, None]
    return dict(u=u, h2=h2, st=st, new=new, new_pole=new_pole)


def rotate_emul(d, mu, uphi, fused_st=False):
    """rotate_dir in correctly rounded float32 (sine and cosine exact, then rounded).  fused_st: 1 - mu^2 rounded once, as the fused
    multiply-add the compiler contracts it to does (every other operation is still rounded on its own)"""
    d = np.asarray(d, dtype=F32)
    ux, uy, uz = d[:, 0], d[:, 1], d[:, 2]
    mu = np.asarray(mu, dtype=F32)
    one = F32(1.0)
    st = np.sqrt(np.maximum(F32(0.0), (1.0 - mu.astype(F64)**2).astype(F32) if fused_st else one - mu*mu)).astype(F32)
    phi = 2.0*PI*np.asarray(uphi, dtype=F64)
    sp, cp = np.sin(phi).astype(F32), np.cos(phi).astype(F32)
    den2 = (one - uz*uz).astype(F32)
    pole = np.minimum(den2, np.maximum(np.abs(ux), np.abs(uy))) < F32(1e-10)
    sg = np.where(uz >= 0.0, one, -one).astype(F32)
    with np.errstate(all='ignore'):
        iden = (one/np.sqrt(den2)).astype(F32)
        den = (den2*iden).astype(F32)
        nx = (st*(ux*uz*cp - uy*sp)*iden + ux*mu).astype(F32)
        ny = (st*(uy*uz*cp + ux*sp)*iden + uy*mu).astype(F32)
        nz = (-st*cp*den + uz*mu).astype(F32)
    nx = np.where(pole, st*cp, nx); ny = np.where(pole, st*sp, ny); nz = np.where(pole, mu*sg, nz)
    return normalise32(np.stack([nx, ny, nz], axis=1)), np.stack([sp, cp], axis=1)


def rotate_check(d, mu, uphi, got, e_sc=None):
    """Hold rotated directions `got` (n, 3) to the reference.  Returns a dict of figures; the callers assert on them:
      nonfinite     outputs that are not finite                      norm      largest | |new| - 1 | in EPS (bound: 4)
      model         largest |new - ref| / (A_ROT EPS + B_ROT EPS st / h2 + st e_sc) over the points with h2 >= H2_MODEL outside the pole branch
      cosine        largest |new . u - mu| over the same bound on the same points (the realised scattering cosine)
      pole          largest |new - ref_pole| / (16 EPS + 2 sqrt(h2)) over the pole branch
      n_model, n_pole, n_between     how many points each rule saw (between: finite and of unit length only)
      locked        points with no horizontal part in, st > 0, and no horizontal part out (the direction stays locked to the axis)
      worst_model, worst_pole        index of the worst point of each rule (or -1)"""
    e_sc = E_SC if e_sc is None else e_sc
    R = rotate_ref(d, mu, uphi)
    got = np.asarray(got, dtype=F64)
    fin = np.all(np.isfinite(got), axis=1)
    out = dict(nonfinite=int((~fin).sum()))
    g = np.where(fin[:, None], got, 0.0)
    out['norm'] = float(np.abs(np.linalg.norm(g[fin], axis=1) - 1.0).max()/EPS) if fin.any() else 0.0
    pole = pole_branch(d)
    model = ~pole & (R['h2'] >= H2_MODEL)
    out['n_model'], out['n_pole'], out['n_between'] = int(model.sum()), int(pole.sum()), int((~pole & ~model).sum())
    out['model'] = out['cosine'] = out['pole'] = 0.0
    out['worst_model'] = out['worst_pole'] = -1
    if model.any():
        b = A_ROT*EPS + B_ROT*EPS*R['st'][model]/R['h2'][model] + R['st'][model]*e_sc
        r = np.linalg.norm(g[model] - R['new'][model], axis=1)/b
        out['model'] = float(r.max()); out['worst_model'] = int(np.flatnonzero(model)[np.argmax(r)])
        out['cosine'] = float((np.abs((g[model]*R['u'][model]).sum(axis=1) - np.asarray(mu, dtype=F64)[model])/b).max())
    if pole.any():
        r = np.linalg.norm(g[pole] - R['new_pole'][pole], axis=1)/(16.0*EPS + 2.0*np.sqrt(R['h2'][pole]))
        out['pole'] = float(r.max()); out['worst_pole'] = int(np.flatnonzero(pole)[np.argmax(r)])
    axis_in = (np.asarray(d)[:, 0] == 0.0) & (np.asarray(d)[:, 1] == 0.0) & (R['st'] > 0.0)
    out['locked'] = int((axis_in & (got[:, 0] == 0.0) & (got[:, 1] == 0.0)).sum())
    return out


@functools.lru_cache(maxsize=None)
def sincos_points():
    """azimuths in turns: the special ones, their float32 neighbours, and 2e5 uniform draws"""
    rng = np.random.default_rng(77)
    sp = []
    for v in list(UPHI_SPECIAL) + [F32(0.125), F32(0.375), F32(0.625), F32(0.875), F32(2.0**-24), F32(2.0**-23)]:
        sp += [v, np.nextafter(v, F32(0.0)), np.nextafter(v, F32(1.0))]
    u = np.concatenate([F32(sp), _u01(rng, 200000)])
    u = u[(u > 0.0) & (u < 1.0)]
    u.setflags(write=False)
    return u


def sincos_ref(u):
    phi = 2.0*PI*np.asarray(u, dtype=F64)
    return np.stack([np.sin(phi), np.cos(phi)], axis=1)


# ----------------------------------------------------------------------------------------------
# surfaces: the formulas
# ----------------------------------------------------------------------------------------------
def _consts(mode):
    T = F32 if mode == 'emul' else F64
    g = (lambda x: T(x)) if mode == 'oracle' else (lambda x: T(F32(x)))      # a guard constant: the device's float32 one unless the oracle's
    k = (lambda x: T(F32(x))) if mode == 'emul' else (lambda x: T(x))        # a constant of the formula
    return T, g, k


def _f(fun, x, T):
    """a library function, correctly rounded: evaluated in float64, rounded to T"""
    return fun(np.asarray(x, dtype=F64)).astype(T)


def lsrt_kernels(din, dout, mode):
    """Ross-Thick / Li-Sparse-Reciprocal kernels for n pairs of directions.  Returns a dict of arrays of type T: kgeo, kvol, the magnitudes
    of their terms tgeo = |O| + sec_i + sec_v + (1 + cos xi) sec_i sec_v / 2 and tvol = |(pi/2 - xi) cos xi + sin xi| / (c_i + c_v) + pi/4,
    sec = max(sec_i, sec_v), D, the distance of the two directions in the plane of tangents (0 at the hot spot), and cxi = cos xi"""
    T, g, k = _consts(mode)
    din = np.asarray(din).astype(T); dout = np.asarray(dout).astype(T)
    one, zero = T(1.0), T(0.0)
    ci = np.maximum(-din[:, 2], g(1e-6)); cv = np.maximum(dout[:, 2], g(1e-6))
    si = np.sqrt(np.maximum(zero, one - ci*ci)); sv = np.sqrt(np.maximum(zero, one - cv*cv))
    hi2 = din[:, 0]*din[:, 0] + din[:, 1]*din[:, 1]; hv2 = dout[:, 0]*dout[:, 0] + dout[:, 1]*dout[:, 1]
    ok = (hi2 > g(1e-24)) & (hv2 > g(1e-24))
    with np.errstate(all='ignore'):
        if mode == 'emul':
            c = (-din[:, 0]*dout[:, 0] - din[:, 1]*dout[:, 1])*(one/np.sqrt(hi2)).astype(T)*(one/np.sqrt(hv2)).astype(T)
        else:
            c = (-din[:, 0]*dout[:, 0] - din[:, 1]*dout[:, 1])/(np.sqrt(hi2)*np.sqrt(hv2))
    cphi = np.clip(np.where(ok, c, one), -one, one).astype(T)
    sphi2 = one - cphi*cphi
    cxi = np.clip(ci*cv + si*sv*cphi, -one, one).astype(T)
    xi = _f(np.arccos, cxi, T)
    sxi = np.sqrt(np.maximum(one - cxi*cxi, zero)) if mode == 'emul' else np.sin(xi)
    if mode == 'emul':
        seci, secv = (one/ci).astype(T), (one/cv).astype(T)
        rsum = (one/(ci + cv)).astype(T)
        a = ((k(0.5)*k(PI) - xi)*cxi + sxi).astype(T)
        kvol = a*rsum - k(0.25)*k(PI)
        tvol = np.abs(a)*rsum + k(0.25)*k(PI)
        ti, tv = si*seci, sv*secv
    else:
        seci, secv = one/ci, one/cv
        a = (0.5*PI - xi)*cxi + sxi
        kvol = a/(ci + cv) - 0.25*PI
        tvol = np.abs(a)/(ci + cv) + 0.25*PI
        ti, tv = si/ci, sv/cv
    D2 = np.maximum(ti*ti + tv*tv - T(2.0)*ti*tv*cphi, zero)
    if mode == 'emul':
        cost = np.minimum(T(2.0)*np.sqrt(D2 + ti*ti*tv*tv*sphi2)*(one/(seci + secv)).astype(T), one)
    else:
        cost = np.minimum(2.0*np.sqrt(D2 + ti*ti*tv*tv*sphi2)/(seci + secv), one)
    t = _f(np.arccos, cost, T)
    sint = np.sqrt(np.maximum(one - cost*cost, zero)) if mode == 'emul' else np.sin(t)
    if mode == 'emul':
        O = (t - sint*cost)*(seci + secv)*T(F32(1.0)/F32(PI))
    else:
        O = (t - sint*cost)*(seci + secv)/PI
    last = T(0.5)*(one + cxi)*seci*secv
    kgeo = O - seci - secv + last
    return dict(kgeo=kgeo.astype(T), kvol=kvol.astype(T), tgeo=np.abs(O) + seci + secv + last, tvol=tvol, sec=np.maximum(seci, secv), D=np.sqrt(D2), cxi=cxi)


def lsrt_R(par, K, mode):
    """R = max(fiso + fgeo kgeo + fvol kvol, 0) from lsrt_kernels' result, and the sum of the magnitudes of its terms"""
    T = F32 if mode == 'emul' else F64
    fiso, fgeo, fvol = (T(F32(x)) for x in par[:3])
    R = np.maximum(fiso + fgeo*K['kgeo'] + fvol*K['kvol'], T(0.0)).astype(T)
    return R, np.abs(F64(fiso)) + np.abs(F64(fgeo))*K['tgeo'].astype(F64) + np.abs(F64(fvol))*K['tvol'].astype(F64)


def fresnel(nr, ni, c, mode, part='both'):
    """reflectance of unpolarised light off a plane of complex index nr + i ni at cosine of incidence c (clamped into [1e-6, 1]).
    part: 'both' (rs + rp) / 2, 's' rs alone"""
    T, g, k = _consts(mode)
    nr, ni = T(F32(nr)), T(F32(ni))
    c = np.minimum(np.maximum(np.asarray(c).astype(T), T(1e-9) if mode == 'oracle' else g(1e-6)), T(1.0))
    s2 = T(1.0) - c*c
    u = nr*nr - ni*ni - s2
    v = np.sqrt(u*u + T(4.0)*nr*nr*ni*ni)
    a2 = np.maximum(T(0.5)*(v + u), T(0.0)); b2 = np.maximum(T(0.5)*(v - u), T(0.0))
    a = np.sqrt(a2)
    rs = ((a - c)*(a - c) + b2)/((a + c)*(a + c) + b2)
    q = s2/c
    rp = rs*((a - q)*(a - q) + b2)/((a + q)*(a + q) + b2)
    return (rs if part == 's' else T(0.5)*(rs + rp)).astype(T)


def shadow_lambda(mu, sigma, mode):
    """Smith's shadowing term L(mu) of a surface of rms slope sigma, and the sum of the magnitudes of its two terms"""
    T, g, k = _consts(mode)
    mu = np.asarray(mu).astype(T); sigma = np.asarray(sigma).astype(T)
    flat = mu >= T(1.0)
    with np.errstate(all='ignore'):
        nu = (mu/(sigma*np.sqrt(T(1.0) - mu*mu))).astype(T)
        e = (_f(np.exp, -nu*nu, T)/((k(1.7724539) if mode == 'emul' else T(np.sqrt(PI)))*nu)).astype(T)
        ec = _f(_erfc, nu, T)
    L = np.where(flat, T(0.0), T(0.5)*(e - ec)).astype(T)
    return L, np.where(flat, 0.0, 0.5*(np.abs(e.astype(F64)) + ec.astype(F64))) + TINY


def dsm_R(par, din, dout, mode):
    """diffuse-specular mixture (diffuse albedo, diffuse fraction, Re m, Im m, slope variance): R, the sum of the magnitudes of its two terms,
    and x = tan^2(theta_n) / s2, the exponent of the facet distribution (-1 where the specular term is not evaluated)"""
    T, g, k = _consts(mode)
    din = np.asarray(din).astype(T); dout = np.asarray(dout).astype(T)
    ad, fd, nr, ni, s2 = (T(F32(x)) for x in par[:5])
    fd = min(max(fd, T(0.0)), T(1.0)); ad = min(max(ad, T(0.0)), T(1.0))
    n = din.shape[0]
    R = np.full(n, fd*ad, dtype=T)
    x = np.full(n, -1.0)
    mi, mv = -din[:, 2], dout[:, 2]
    if s2 > 0.0 and fd < 1.0:
        h = dout - din
        hn = np.sqrt(h[:, 0]*h[:, 0] + h[:, 1]*h[:, 1] + h[:, 2]*h[:, 2]).astype(T)
        with np.errstate(all='ignore'):
            mun = (h[:, 2]/hn).astype(T)
            cchi = ((-din[:, 0]*h[:, 0] - din[:, 1]*h[:, 1] - din[:, 2]*h[:, 2])/hn).astype(T)
            on = (mi > g(1e-6)) & (mv > g(1e-6)) & (hn > g(1e-12)) & (mun > g(1e-6))
            mun2 = mun*mun
            arg = (-(T(1.0) - mun2)/(mun2*s2)).astype(T)
            P = (_f(np.exp, arg, T)/(k(PI)*s2)).astype(T)
            sg = np.sqrt(s2).astype(T) if mode == 'emul' else np.sqrt(s2)
            Li, _ = shadow_lambda(mi, sg, mode)
            Lv, _ = shadow_lambda(mv, sg, mode)
            S = (T(1.0)/(T(1.0) + Li + Lv)).astype(T)
            F = fresnel(nr, ni, cchi, mode)
            spec = ((T(1.0) - fd)*k(PI)*F*P*S/(T(4.0)*mi*mv*mun2*mun2)).astype(T)
        R = np.where(on, R + spec, R).astype(T)
        x = np.where(on, -arg.astype(F64), -1.0)
    R = np.maximum(R, T(0.0)).astype(T)
    return R, np.abs(R.astype(F64)) + TINY, x


# ----------------------------------------------------------------------------------------------
# surfaces: the points
# ----------------------------------------------------------------------------------------------
def _pair(thi, azi, thv, azv):
    return normalise32(_sph(thi, azi, -1.0)), normalise32(_sph(thv, azv, 1.0))


SFC_CLASSES = ('general', 'view_grazing', 'both_grazing', 'hotspot', 'near_vertical', 'plane_forward', 'plane_backward', 'clamped', 'guards')
_DEG = PI/180.0


@functools.lru_cache(maxsize=None)
def surface_dirs(name):
    """(din, dout) (n, 3) float32 of one direction class, normalised in float32"""
    n = N_SFC
    rng = np.random.default_rng(2000 + SFC_CLASSES.index(name))
    azi = rng.uniform(0.0, 2.0*PI, n); daz = rng.uniform(0.0, 2.0*PI, n)
    if name == 'general':
        din, dout = _pair(rng.uniform(0.0, 80.0, n)*_DEG, azi, rng.uniform(0.0, 80.0, n)*_DEG, azi + daz)
    elif name == 'view_grazing':
        din, dout = _pair(rng.uniform(0.0, 80.0, n)*_DEG, azi, rng.uniform(80.0, 89.9, n)*_DEG, azi + daz)
    elif name == 'both_grazing':
        din, dout = _pair(rng.uniform(85.0, 89.99, n)*_DEG, azi, rng.uniform(85.0, 89.99, n)*_DEG, azi + daz)
    elif name == 'hotspot':                  # the viewer within 1e-3 rad of the source, zenith angles up to 80 degrees
        thi = rng.uniform(0.0, 80.0, n)*_DEG
        r = 10.0**rng.uniform(-7.0, -3.0, n)
        din, dout = _pair(thi, azi, np.abs(thi + r*np.cos(daz)), azi + PI + r*np.sin(daz)/np.maximum(np.sin(thi), 1e-3))
        dout[:1000] = -din[:1000]            # the hot spot itself
    elif name == 'near_vertical':            # both within 1e-3 rad of the vertical; exactly vertical: the hi2 / hv2 guard
        din, dout = _pair(rng.uniform(0.0, 1e-3, n), azi, rng.uniform(0.0, 1e-3, n), azi + daz)
        din[:2000] = (0.0, 0.0, -1.0); dout[1000:3000] = (0.0, 0.0, 1.0)
    elif name == 'plane_forward':            # the principal plane, the viewer on the far side of the source
        din, dout = _pair(rng.uniform(0.01, 1.5, n), azi, rng.uniform(0.01, 1.5, n), azi)
    elif name == 'plane_backward':           # the principal plane, the viewer on the source's side (crosses the hot spot)
        din, dout = _pair(rng.uniform(0.01, 1.5, n), azi, rng.uniform(0.01, 1.5, n), azi + PI)
    elif name == 'clamped':                  # diz = 0, doz = 0, both: the 1e-6 clamps of the cosines
        din, dout = _pair(rng.uniform(0.0, 80.0, n)*_DEG, azi, rng.uniform(0.0, 80.0, n)*_DEG, azi + daz)
        i = np.arange(n) % 3
        din[i != 1, 2] = 0.0; dout[i != 0, 2] = 0.0
        din[i != 1] = normalise32(din[i != 1]); dout[i != 0] = normalise32(dout[i != 0])
    elif name == 'guards':                   # both cosines around 1e-6, forward (cos chi at its clamp) and backward (mu_n at its guard)
        mi = 10.0**rng.uniform(-6.5, -5.0, n); mv = 10.0**rng.uniform(-6.5, -5.0, n)
        back = np.arange(n) % 2 == 1
        din, dout = _pair(np.arccos(mi), azi, np.arccos(mv), azi + np.where(back, PI, 0.0) + rng.choice([-1.0, 1.0], n)*10.0**rng.uniform(-7.0, -3.0, n))
        din[:, 2] = -mi.astype(F32); dout[:, 2] = mv.astype(F32)
    else:
        raise KeyError(name)
    din.setflags(write=False); dout.setflags(write=False)
    return din, dout


LSRT_PARAMS = ((0.1, 0.03, 0.05), (0.1, 0.0, 0.0), (0.0, 0.03, 0.0), (0.0, 0.0, 0.05), (-0.2, 0.03, 0.05))
#               diffuse albedo, diffuse fraction, Re m, Im m, slope variance
DSM_PARAMS = ((0.2, 0.3, 1.33, 1e-8, 1e-4), (0.2, 0.3, 1.33, 1e-8, 0.003), (0.2, 0.3, 1.33, 1e-8, 0.05), (0.2, 0.3, 1.33, 1e-8, 0.1),
              (0.2, 0.0, 1.33, 0.0, 0.003), (0.2, 1.0, 1.33, 0.0, 0.003), (0.2, 0.0, 1.33, 0.3, 0.05))
FRESNEL_INDICES = ((1.33, 0.0), (1.33, 1e-8), (1.33, 0.3), (1.5, 0.0))
SIGMAS = tuple(float(np.sqrt(F32(s2))) for s2 in (1e-4, 0.003, 0.05, 0.1))


def _merge_small(b, least=200):
    """bin numbers b >= 0 with bins of fewer than `least` points merged into the next occupied bin above (the last into the one below)"""
    b = b.copy()
    ids = np.unique(b)
    for j, v in enumerate(ids[:-1]):
        if (b == v).sum() < least:
            b[b == v] = ids[j+1]
    ids = np.unique(b)
    if ids.size > 1 and (b == ids[-1]).sum() < least:
        b[b == ids[-1]] = ids[-2]
    return b


def lsrt_bins(name, K):
    """the bins of a direction class: the hot spot and the backward principal plane by the distance D (decades below 1e-2) and the
    secant; the grazing classes by max(sec) (factors of two), and where both directions graze also by 1 + cos xi (decades: towards forward
    scattering 1 + cos xi cancels, and sec_i sec_v multiplies what is left); the clamped class by which cosine is clamped; one bin otherwise"""
    sec, D = K['sec'].astype(F64), K['D'].astype(F64)
    sb = np.floor(np.log2(np.maximum(sec, 1.0))).astype(int)
    fb = np.clip(np.floor(np.log10(np.maximum(1.0 + K['cxi'].astype(F64), 1e-30))).astype(int) + 6, 0, 6)      # 1 + cos xi < 1e-6: 0, ..., >= 1: 6
    if name in ('hotspot', 'plane_backward'):
        db = np.clip(np.floor(np.log10(np.maximum(D, 1e-30))).astype(int) + 9, 0, 7)      # D < 1e-8: 0, ..., D >= 1e-2: 7
        return _merge_small(db*8 + np.minimum(sb, 7))
    if name in ('view_grazing', 'plane_forward'):
        return _merge_small(sb)
    if name in ('both_grazing', 'guards'):
        return _merge_small(sb*8 + fb)
    if name == 'clamped':
        i = np.arange(sec.size) % 3
        return _merge_small(i*8 + np.where(i == 2, fb, 0))
    return np.zeros(sec.size, dtype=int)


def _class_bound(err, scale, bins):
    """per point: max(4 E_emul, 8 EPS) x scale, E_emul the largest err / scale of the float32 emulation in the point's bin"""
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(scale > 0.0, err/scale, np.where(err == 0.0, 0.0, np.inf))
    e = np.zeros(scale.size)
    for v in np.unique(bins):
        e[bins == v] = rel[bins == v].max()
    return np.maximum(4.0*e, 8.0*EPS)*scale, e


@functools.lru_cache(maxsize=None)
def lsrt_case(name):
    """one direction class under every parameter set of LSRT_PARAMS: din, dout, and per set (ref, emul, bound, E_emul), float64 per point"""
    din, dout = surface_dirs(name)
    K64, K32 = lsrt_kernels(din, dout, 'ref'), lsrt_kernels(din, dout, 'emul')
    bins = lsrt_bins(name, K64)
    per = []
    for par in LSRT_PARAMS:
        ref, scale = lsrt_R(par, K64, 'ref')
        em, _ = lsrt_R(par, K32, 'emul')
        bound, e = _class_bound(np.abs(em.astype(F64) - ref), scale, bins)
        per.append(dict(par=par, ref=ref, emul=em, bound=bound, e_emul=e))
    return dict(din=din, dout=dout, bins=bins, per=per)


DSM_POOL_CLASSES = ('general', 'view_grazing', 'hotspot', 'near_vertical', 'plane_forward', 'plane_backward')
DSM_SEC_CLASSES = ('view_grazing', 'both_grazing', 'plane_forward', 'guards')
DSM_SMALL_BIN = 200


@functools.lru_cache(maxsize=None)
def _dsm_all():
    """every direction class, its points dealt out in turn to the parameter sets of DSM_PARAMS.
    Bins, per class and parameter set: the facet exponent x (not evaluated, < 1, < 4, < 16, < 64, beyond), and in the grazing classes
    (DSM_SEC_CLASSES) max(sec) in factors of two.  E_emul of a bin is the emulation's largest scaled error over the bin's points in both
    senses (the pair as given and the reciprocal pair, which the reciprocity check evaluates too).
    A bin of fewer than DSM_SMALL_BIN points gives no estimate: what float32 loses here is x = (1 - mun2) / (mun2 s2), a few EPS / s2
    absolute, and at small slope variance only a handful of a class's points lie near enough to the specular direction to show it (one point
    of view_grazing at s2 = 1e-4).  Such a bin takes the larger of its own figure and that of the same parameter set and exponent bin over the
    classes WITHOUT an amplification of their own (DSM_POOL_CLASSES: not `guards`, `both_grazing`, `clamped`, where 1 / (4 mi mv) reaches
    1e10).  Every bin of DSM_SMALL_BIN points or more stands on its own."""
    out, pool = {}, {}
    for name in SFC_CLASSES:
        din, dout = surface_dirs(name)
        per = []
        for j, par in enumerate(DSM_PARAMS):
            idx = np.arange(j, din.shape[0], len(DSM_PARAMS))
            rin, rout = reverse_pair(din[idx], dout[idx])
            ref, scale, x = dsm_R(par, din[idx], dout[idx], 'ref')
            em, _, _ = dsm_R(par, din[idx], dout[idx], 'emul')
            ref_rev, scale_rev, _ = dsm_R(par, rin, rout, 'ref')
            em_rev, _, _ = dsm_R(par, rin, rout, 'emul')
            xb = np.where(x < 0.0, -1, np.searchsorted([1.0, 4.0, 16.0, 64.0], x, side='right'))
            sec = 1.0/np.maximum(np.minimum(-din[idx, 2].astype(F64), dout[idx, 2].astype(F64)), 2.0**-24)
            sb = np.floor(np.log2(np.maximum(sec, 1.0))).astype(int) if name in DSM_SEC_CLASSES else np.zeros(idx.size, dtype=int)
            rel = np.maximum(np.abs(em.astype(F64) - ref)/scale, np.abs(em_rev.astype(F64) - ref_rev)/scale_rev)
            if name in DSM_POOL_CLASSES:
                for v in np.unique(xb):
                    pool[(j, int(v))] = max(pool.get((j, int(v)), 0.0), float(rel[xb == v].max()))
            per.append(dict(par=par, idx=idx, ref=ref, emul=em, emul_rev=em_rev, scale=scale, scale_rev=scale_rev, ref_rev=ref_rev, xb=xb,
                            bins=(xb + 1)*32 + sb, rel=rel))
        out[name] = dict(din=din, dout=dout, per=per)
    for C in out.values():
        for j, p in enumerate(C['per']):
            e = np.zeros(p['idx'].size); small = np.zeros(p['idx'].size, dtype=bool)
            for v in np.unique(p['bins']):
                m = p['bins'] == v
                own = float(p['rel'][m].max())
                if m.sum() < DSM_SMALL_BIN:
                    own = max(own, pool.get((j, int(p['xb'][m][0])), 0.0)); small[m] = True
                e[m] = own
            f = np.maximum(4.0*e, 8.0*EPS)
            bound = f*p['scale']
            # Reciprocity holds for unit vectors: the facet normal bisects them.  Float32 directions are not of unit length, and where both
            # graze the difference vector h = dout - din is made of their rounding: the float64 formula itself then differs between the two
            # senses (by 2.7 of twice the bound at 85 to 89.99 degrees, by orders of magnitude at cosines of 1e-6).  Where it differs by less
            # than a hundredth of twice the bound (`rec_strict`) the identity is held as the bound says: |R(a) - R(a')| <= 2 bound.  Elsewhere
            # no identity is left to hold, and the device's value on the reciprocal pair is held to the float64 value ON THAT PAIR within the
            # bound on its scale, bound_rev: a second direct comparison, not reciprocity.
            asym = np.abs(p['ref'] - p['ref_rev'])
            p.update(e_emul=e, small=small, bound=bound, bound_rev=f*p['scale_rev'], rec_strict=asym <= 0.01*2.0*bound)
    return out


def dsm_case(name):
    """one direction class: din, dout, and per parameter set (idx into the class, ref, emul, bound, E_emul, the reciprocity tolerance)"""
    return _dsm_all()[name]


@functools.lru_cache(maxsize=None)
def fresnel_points():
    """cosines of incidence: uniform, grazing down to and below the clamp, beyond 1, and Brewster's angle of each real index"""
    rng = np.random.default_rng(31)
    c = np.concatenate([rng.uniform(0.0, 1.0, 60000), 10.0**rng.uniform(-8.0, -1.0, 30000), 1.0 - 10.0**rng.uniform(-7.0, -1.0, 10000),
                        [0.0, 1e-7, 1e-6, 1.0, 1.0 + 2.0**-23, 1.5, -0.5]]).astype(F32)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def fresnel_case(nr, ni):
    c = fresnel_points()
    ref = fresnel(nr, ni, c, 'ref'); em = fresnel(nr, ni, c, 'emul')
    cc = np.clip(c.astype(F64), 1e-6, 1.0)
    bins = np.searchsorted([1e-5, 1e-3, 0.1], cc, side='right')
    bound, e = _class_bound(np.abs(em.astype(F64) - ref), ref, bins)
    return dict(c=c, ref=ref, emul=em, bound=bound, e_emul=e)


@functools.lru_cache(maxsize=None)
def lambda_points():
    rng = np.random.default_rng(32)
    mu = np.concatenate([rng.uniform(0.0, 1.0, 60000), 10.0**rng.uniform(-7.0, -1.0, 30000), 1.0 - 10.0**rng.uniform(-7.0, -1.0, 10000),
                         [1.0, 1.0 + 2.0**-23, 2.0, ONE_M, 1e-6]]).astype(F32)
    mu = mu[mu > 0.0]
    mu.setflags(write=False)
    return mu


@functools.lru_cache(maxsize=None)
def lambda_case(sigma):
    mu = lambda_points()
    ref, scale = shadow_lambda(mu, F32(sigma), 'ref')
    em, _ = shadow_lambda(mu, F32(sigma), 'emul')
    with np.errstate(all='ignore'):
        nu = mu.astype(F64)/(float(F32(sigma))*np.sqrt(np.maximum(1.0 - mu.astype(F64)**2, 1e-300)))
    bins = _merge_small(np.searchsorted([0.01, 0.1, 1.0, 3.0, 6.0], nu, side='right'))
    bound, e = _class_bound(np.abs(em.astype(F64) - ref), scale, bins)
    return dict(mu=mu, ref=ref, emul=em, bound=bound, e_emul=e)


def reverse_pair(din, dout):
    """the reciprocal geometry: light arrives along -dout and leaves along -din"""
    return np.ascontiguousarray(-np.asarray(dout, dtype=F32)), np.ascontiguousarray(-np.asarray(din, dtype=F32))
