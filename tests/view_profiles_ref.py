"""
Reference helpers for the per-layer profiles of the backward route's satellite views (mi3d_set_view_profiles 1, Rad_mvprf = 1; DESIGN.md §5.16;
tests/test_view_profiles_host.py, tests/test_gpu_view_profiles.py).  The scenes are those of tests/backward_views_ref.py; the float64 weights
of a line of sight are tests/emission_weights_ref.line_weights, summed here per layer and for the surface; the g / run reduction of the
drop-in is restated in plain numpy.  Nothing of the solver is used.
"""

import dataclasses

import numpy as np

from tests import emission_weights_ref as wref


def layer_rows(sc, K):
    """K (n, ncell) in tally order (voxels [nz3][ny][nx], layers [nz], surface cells) -> (n, nz + 1): rows 0 ... nz - 1 the layers from the
    surface up -- a layer of the 3-D region is the sum over its voxels --, row nz the sum over the surface cells"""
    K = np.atleast_2d(np.asarray(K, dtype=np.float64))
    nz, nz3, k3lo, nvox = sc.nz, sc.nz3, sc.iz3l-1, sc.nx*sc.ny*sc.nz3
    out = np.zeros((K.shape[0], nz+1))
    out[:, :nz] = K[:, nvox:nvox+nz]
    if nz3 > 0:
        out[:, k3lo:k3lo+nz3] += K[:, :nvox].reshape(K.shape[0], nz3, -1).sum(axis=2)
    out[:, nz] = K[:, nvox+nz:].sum(axis=1)
    return out


def line_profiles(sc, org, dirs):
    """(K_ref, C_ref), each (n, nz + 1) float64, of the lines of sight from org along dirs through a non-scattering scene: the per-cell
    weights of the line and the same weights times the cells' Planck radiances, summed per layer and for the surface"""
    K = wref.line_weights(sc, org, dirs)
    return layer_rows(sc, K), layer_rows(sc, K*wref.planck_cells(sc)[None, :])


def with_anomalies(sc, seed=11, amp=6.0):
    """the scene with 3-D temperature anomalies of up to +-amp K drawn once from a seeded generator (whatever it carried before)"""
    rng = np.random.default_rng(seed)
    return dataclasses.replace(sc, tmpa3d=rng.uniform(-amp, amp, size=(sc.nz3, sc.ny, sc.nx)).astype(np.float32))


def reduce_runs(jobs, factors):
    """the g / run reduction of the drop-in restated: jobs[ir][ig] arrays of one shape, factors [Ng] -> (runs [..., Nr], mean, population
    standard deviation): per run sum_g factors[ig] * jobs[ir][ig] in float64"""
    runs = np.stack([sum(float(factors[ig])*np.asarray(a, dtype=np.float64) for ig, a in enumerate(row)) for row in jobs], axis=-1)
    return runs, runs.mean(axis=-1), runs.std(axis=-1)
