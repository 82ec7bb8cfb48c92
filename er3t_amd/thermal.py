"""
Thermal source (Src_mtype = 3): Planck's law and its inverse, the brightness temperature, on the host.

The physics contract is stated in include/mi3d.h (mi3d_set_thermal) and DESIGN.md ("Thermal source"); the kernel evaluates the
same expression in float64 (mi3d_kernels.hip: planck_um).  Radiances are in W m-2 sr-1 um-1 with the wavelength in micrometres.
"""

import numpy as np

__all__ = ['planck', 'brightness_temperature', 'H', 'C', 'K']

# CODATA 2018 (exact in the SI)
H = 6.62607015e-34      # J s
C = 299792458.0         # m / s
K = 1.380649e-23        # J / K


def planck(wvl_um, T):
    """B(lambda, T) in W m-2 sr-1 um-1; wvl_um in micrometres, T in K (arrays broadcast; T <= 0 gives 0)"""
    wl = np.asarray(wvl_um, dtype=np.float64)*1.0e-6
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        b = 2.0*H*C*C/wl**5/np.expm1(H*C/(wl*K*T))*1.0e-6
    return np.where(T > 0.0, b, 0.0)


def dplanck_dT(wvl_um, T):
    """dB/dT(lambda, T) in W m-2 sr-1 um-1 K-1: B x / (T (1 - exp(-x))), x = h c / (lambda k T) (T <= 0 gives 0).  With the emission weights
    K of the backward route the Jacobian of a reading is dR_p/dT_c = Src_flx K[p][c] dB/dT(T_c)"""
    wl = np.asarray(wvl_um, dtype=np.float64)*1.0e-6
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        x = H*C/(wl*K*T)
        d = planck(wvl_um, T)*x/(T*(-np.expm1(-x)))
    return np.where(T > 0.0, d, 0.0)


def brightness_temperature(wvl_um, radiance):
    """the inverse of planck: T in K of a radiance in W m-2 sr-1 um-1 (radiance <= 0 gives 0)"""
    wl = np.asarray(wvl_um, dtype=np.float64)*1.0e-6
    L = np.asarray(radiance, dtype=np.float64)*1.0e6
    with np.errstate(divide='ignore', invalid='ignore'):
        t = H*C/(wl*K)/np.log1p(2.0*H*C*C/(wl**5*L))
    return np.where(L > 0.0, t, 0.0)
