// mi3d_kernel_backward.hip — backward (adjoint) Monte Carlo for the cameras and point radiometers of thermal jobs
// (Src_mtype = 3, Rad_mrkind = 1; mi3d_set_camera_method 1; DESIGN.md §5.11, contract in include/mi3d.h).
//
// A history starts at the sensor and flies backwards along a line of sight drawn inside its pixel.  It collects ka B(T) along its
// path and eps B(Ts) at the surface; scattering and reflection turn it, absorption is continuous.  No 1 / r^2, no aperture clamp, no
// periodic images: a line of sight wraps through the cyclic domain.
//
// Kernels
//   k_backward_cells   once per job (mi3d_prepare, next to k_thermal_power): {ka, B(T)} of every voxel and layer, {eps, B(Ts)} of every
//                      surface cell, float64 through cell_emission / planck_um, rounded once; the order of DevThermal's CDF
//   k_backward<COUNT, DEBUG>   the histories: one lane owns one, one cell step per trip of the loop, a lane whose history has ended takes
//                      its next id in the same trip.  DEBUG: mi3d_debug_backward -- the same code, direction and score of every id written out
//                      instead of tallied
//   k_backward_w<COUNT>   the same histories with mi3d_set_emission_weights 1: every term w (1 - exp(-ka l)) and w eps
//                      that a history scores is also added to K_raw[pixel][cell], float64
//   k_backward_v<COUNT, DEBUG>   the same histories for the satellite views of mi3d_set_view_method 1: block 0 places the
//                      line of sight on the view's registration level inside pixel id mod npix, the history starts where that line meets the
//                      sensor plane; the views are staged in LDS where the cameras were; ids are handed out by tiles of 8 x 8 pixels
//                      ("bwd_chunk" >= 1) and a lane sums its pixel's scores in a register.  DEBUG: mi3d_debug_backward_views
//   k_backward_vp<COUNT>   the histories of k_backward_v with mi3d_set_view_profiles 1: every term w (1 - exp(-ka l)),
//                      w eps and every term of the score is also added to P_raw[pixel][layer | surface], float64, a run of one (pixel, row)
//                      summed in registers and flushed when it changes
//   k_backward_s<COUNT>, k_backward_vs<COUNT>   the histories of k_backward and of k_backward_v with mi3d_set_pixel_errors 1 (DESIGN.md
//                      §5.17): the square of every score that enters rad[pixel] is also added to rad2[pixel], float64, by the path the
//                      score itself takes (LDS sums, the tile hand-out's register, global atomics)
//   k_backward_vn<COUNT, DEBUG>, k_backward_vns<COUNT>   the histories of k_backward_v and of k_backward_vs for a solar+thermal job
//                      (Src_mtype = 2) with mi3d_set_view_sunlight 1: every scattering and every surface reflection also
//                      scores the sunlight it turns into the line of sight, times the transmittance of a ray from the event to the top.
//                      The ray is flown by the trips of the same loop, one cell step each, and ends in closed form above the 3-D region.
//                      The solar cone draws its direction from Philox blocks 2^31, 2^31 + 1, ... of the history, which the walk never reaches
//   k_backward_vc<COUNT, DEBUG>, k_backward_vcs<COUNT>, k_backward_vcp<COUNT>, k_backward_vcn<COUNT, DEBUG>, k_backward_vcns<COUNT>   the
//                      histories of k_backward_v, _vs, _vp, _vn, _vns under independent columns and partial 3-D (mi3d_set_view_columns 1;
//                      DESIGN.md §5.20): a history keeps the column under its start, crosses every layer level to level and folds its
//                      horizontal position inside the column; no x / y faces, no moves between columns.  DEBUG: mi3d_debug_backward_views
//   k_backward_norm    read-out: tally of pixel p / number of ids in [0, N) that map to p
//   k_backward_norm_se   read-out of the standard error of that mean from rad and rad2
//   k_backward_norm_rows   the same rule for the rows of K_raw, rounded to float32
//   k_backward_norm_profiles   the same rule for the rows of P_raw, its pairs {K, C} parted into two float32 arrays
//
// Philox blocks of history (seed, id), counter (id, block), consumed in sequence; block 0 is the direction, every later decision takes
// the NEXT block when it comes up:
//   block 0                      u0, u1: the line of sight inside pixel id mod npix (u0 along U / theta, u1 along V / phi)
//   a flight                     u0: its scattering optical path, -ln u0; u1: the constituent that scatters at its end, in proportion to
//                                k_s (the 1-D ones first, then the 3-D ones; its position inside the share: which of two mixed tables);
//                                u2: cos(scattering angle); u3: azimuth / 2 pi
//   a reflection                 u0: cos^2 of the new polar angle (cosine law), u1: azimuth / 2 pi, u2: its weight roulette (if played)
//   a roulette after a scattering   u0 of a block of its own, drawn only when the game is played (w < Pho_wmin)
// In a scene that never scatters over a black surface the flight is block 1 and nothing else is drawn.
#include "mi3d_device.h"

namespace mi3d {

constexpr unsigned kBwdMaxCells = 1u << 20;   // cell steps after which a history ends and is counted as capped
constexpr float kBwdWeightEnd = 1.0e-7f;      // a history whose weight falls below this ends (bias <= 1e-7 max B)
constexpr int kBwdChunkAuto = 4;              // mi3d_set_tuning "bwd_chunk" -1: the largest chunk of the tile hand-out
constexpr int kBwdLdsPix = 2048;              // images up to this many pixels are summed per workgroup in LDS
constexpr int kBwdLdsPixErr = 1024;           // ... in the builds with a second tally (VAR): two sums per pixel, the same bytes at most

struct DevBackward {
    int nx, ny, nz, nz3, k3lo, np1d, np3d;
    int nxb, nyb;                      // surface cells (1 x 1: uniform surface)
    int nview, nxr, nyr, cam_mode;     // cam_mode: ViewRec::point of the cameras (kCamRect, kCamCos)
    float dx, dy, inv_dx, inv_dy, ztoa, sfc_sx, sfc_sy;
    float wmin, wfac, src_flx;
    unsigned nvox, vcol_f4, vrow_f4;
    const LayerRec *lay;               // [nz]
    const float4 *vrec;                // DevScene::vrec
    const float2 *csca;                // DevCold::csca
    const float2 *cells;               // [nvox + nz + nxb nyb] k_backward_cells
    const CamRec *cams;                // [nview]
    PhaseTab tab;                      // the phase tables in global memory
    double *rad;                       // [nview][nyr][nxr] raw sums
    unsigned long long *counters;      // [MI3D_NCOUNTER]
    unsigned long long *capped;        // histories ended by kBwdMaxCells
};

// What only the weights build receives (mi3d_set_emission_weights 1): the tally K_raw[npix][ncell] and how its layer and surface part
// (nls = nz + nxb nyb cells per pixel) is summed -- stage: per workgroup in LDS, flushed once at the end; otherwise global atomics
struct BwdWeights {
    double *K;
    unsigned long long ncell;
    int nls, stage;
};

// What only the satellite-view build receives (mi3d_set_view_method 1): the views, the pixel size on the registration level, the domain,
// the tile hand-out's chunk (jch histories of a pixel per item; 0: the plain stride of the camera route) and the debug entry's start points
struct BwdSat {
    const ViewRec *views;              // [nview]
    float pix_dx, pix_dy, Lx, Ly, inv_Lx, inv_Ly;
    int jch;
    float *start_out;                  // [n][3] (DEBUG)
};

// What only the profiles build receives (mi3d_set_view_profiles 1): the tally P_raw[npix][nrow][2] of pairs {K, C}, nrow = nz + 1 (the
// layers from the surface up, then the surface)
struct BwdProfiles {
    double *raw;
    int nrow;
};

// What only the builds with per-pixel standard errors receive (mi3d_set_pixel_errors 1): the tally of the squared scores, shaped as rad
struct BwdErrors {
    double *rad2;
};

// What only the builds with sunlight receive (mi3d_set_view_sunlight 1): the direction d in which sunlight travels
// (sdz < 0), mu0 = |sdz|, F = Src_fsol and the cosine of the solar cone's half angle (>= 1: no cone).  The table of the vertical optical depth from a level to the top is LayerRec::tabove of the layers above
// the 3-D region: it is in LDS with the layer table already
struct BwdSun {
    float sdx, sdy, sdz, mu0, F, cos_cone;
    int ray3d;                         // read by the column builds alone (mi3d_set_view_columns 1): 1 the ray is the direct beam of
                                       // partial 3-D and flies through the cyclic grid, 0 it keeps the event's column (independent columns)
};

// One thread per cell, in the order of DevThermal's CDF (k_thermal_power): voxels in file order, layers, surface cells.
__global__ void __launch_bounds__(256)
k_backward_cells(const ThermalGrid G, int nxb, int nyb, const float *sfc2d, float albedo, const float *tmps2d, float2 *out) {
    const int nx = G.nx, ny = G.ny, nz = G.nz, nz3 = G.nz3, k3lo = G.k3lo;
    const unsigned long nvox = (unsigned long)nx * ny * nz3, nsfc = (unsigned long)nxb * nyb;
    const unsigned long i = (unsigned long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvox + nz + nsfc) return;
    double a = 0.0, b = 0.0;
    if (i < nvox) {
        const unsigned long ncol = (unsigned long)nx * ny;
        const int k3 = (int)(i / ncol), col = (int)(i % ncol), iy = col / nx, ix = col % nx;
        const CellEmission c = cell_emission(G, k3lo + k3, iy, ix, true);
        a = c.ka; b = planck_um(G.wl_um, c.T);
    } else if (i < nvox + nz) {
        const int k = (int)(i - nvox);
        if (!(nz3 > 0 && k >= k3lo && k < k3lo + nz3)) {      // (inside the 3-D region the voxels are read)
            const CellEmission c = cell_emission(G, k, 0, 0, false);
            a = c.ka; b = planck_um(G.wl_um, c.T);
        }
    } else {
        const unsigned long s = i - nvox - nz;
        const double al = sfc2d ? (double)sfc2d[s * 8 + 1] : (double)albedo;
        a = 1.0 - fmin(fmax(al, 0.0), 1.0);
        b = planck_um(G.wl_um, (double)G.tlev[0] + (tmps2d ? (double)tmps2d[s] : 0.0));
    }
    out[i] = make_float2((float)a, (float)b);
}

// the number of ids in [0, N) with id mod npix == p
__device__ inline unsigned long long bwd_pixel_ids(const unsigned long long nphoton, const unsigned npix, const unsigned long long p) {
    return nphoton / npix + (p < nphoton % npix ? 1ull : 0ull);
}
// tally[p] / (number of ids in [0, N) that map to p), 0 where that number is 0
__global__ void __launch_bounds__(256)
k_backward_norm(const double *__restrict__ tally, double *__restrict__ out, unsigned long long nphoton, unsigned npix) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const unsigned long long cnt = bwd_pixel_ids(nphoton, npix, p);
    out[p] = cnt ? tally[p] / (double)cnt : 0.0;
}
// ... and for elements [e0, e0 + ne) of K_raw[npix][ncell]: element e belongs to pixel e / ncell
__global__ void __launch_bounds__(256)
k_backward_norm_rows(const double *__restrict__ K, float *__restrict__ out, unsigned long long nphoton, unsigned npix, unsigned long long ncell,
                     unsigned long long e0, unsigned long long ne) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += stride) {
        const unsigned long long cnt = bwd_pixel_ids(nphoton, npix, (e0 + i) / ncell);
        out[i] = cnt ? (float)(K[e0 + i] / (double)cnt) : 0.0f;
    }
}

// 1 - exp(-a) and exp(-a) for a >= 0: the series where the difference would cancel
__device__ inline float bwd_absorb(const float a, float &e) {
    e = fexp_neg(a);
    return a < 0.03f ? a * (1.0f - a * (0.5f - a * ((1.0f / 6.0f) - a * (1.0f / 24.0f)))) : 1.0f - e;
}
// i + d folded into [0, n), d any float number of cells (a whole number)
__device__ inline int bwd_wrap(const int i, const float d, const int n) {
    const float fn = (float)n;
    float r = (float)i + (d - fn * floorf(d / fn));      // (d folded first: it may be far beyond the integers a float holds)
    r -= fn * floorf(r / fn);
    const int j = (int)r;
    return j < 0 ? 0 : (j >= n ? n - 1 : j);
}

// The histories, single-sourced for all entry points: mi3d_kernel_backward_body.inc is the body of each, with WGT, SAT, PRF, VAR, SUN and COL
// constants of the entry point that includes it (and W, S, P, E, N the arguments of the builds that read them)
template <bool COUNT, bool DEBUG>
__global__ void __launch_bounds__(256)
k_backward(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, float *__restrict__ dir_out, double *__restrict__ score_out) {
    constexpr bool WGT = false, SAT = false, PRF = false, VAR = false, SUN = false, COL = false;
    const BwdWeights W{};
    const BwdSat S{};
    const BwdProfiles P{};
    const BwdErrors E{};
    const BwdSun N{};
#include "mi3d_kernel_backward_body.inc"
}

template <bool COUNT>
__global__ void __launch_bounds__(256)
k_backward_w(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, const BwdWeights W) {
    constexpr bool WGT = true, DEBUG = false, SAT = false, PRF = false, VAR = false, SUN = false, COL = false;
    float *const dir_out = nullptr; double *const score_out = nullptr;
    const BwdSat S{};
    const BwdProfiles P{};
    const BwdErrors E{};
    const BwdSun N{};
#include "mi3d_kernel_backward_body.inc"
}

template <bool COUNT, bool DEBUG>
__global__ void __launch_bounds__(256)
k_backward_v(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, float *__restrict__ dir_out, double *__restrict__ score_out,
             const BwdSat S) {
    constexpr bool WGT = false, SAT = true, PRF = false, VAR = false, SUN = false, COL = false;
    const BwdWeights W{};
    const BwdProfiles P{};
    const BwdErrors E{};
    const BwdSun N{};
#include "mi3d_kernel_backward_body.inc"
}

template <bool COUNT>
__global__ void __launch_bounds__(256)
k_backward_vp(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, const BwdSat S, const BwdProfiles P) {
    constexpr bool WGT = false, DEBUG = false, SAT = true, PRF = true, VAR = false, SUN = false, COL = false;
    float *const dir_out = nullptr; double *const score_out = nullptr;
    const BwdWeights W{};
    const BwdErrors E{};
    const BwdSun N{};
#include "mi3d_kernel_backward_body.inc"
}

// The rule of k_backward_norm_rows for rows [e0, e0 + ne) of P_raw[npix * nrow][2]: row e belongs to pixel e / nrow.  (It stands behind
// the histories so that the code of the kernels before it lies where it lay.)
__global__ void __launch_bounds__(256)
k_backward_norm_profiles(const double *__restrict__ raw, float *__restrict__ outK, float *__restrict__ outC, unsigned long long nphoton, unsigned npix,
                         unsigned long long nrow, unsigned long long e0, unsigned long long ne) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += stride) {
        const unsigned long long cnt = bwd_pixel_ids(nphoton, npix, (e0 + i) / nrow);
        outK[i] = cnt ? (float)(raw[2 * (e0 + i)] / (double)cnt) : 0.0f;
        outC[i] = cnt ? (float)(raw[2 * (e0 + i) + 1] / (double)cnt) : 0.0f;
    }
}

// The histories with mi3d_set_pixel_errors 1: the same body with VAR.  (They stand behind every other kernel so that
// the code of the kernels before them lies where it lay.)
template <bool COUNT>
__global__ void __launch_bounds__(256)
k_backward_s(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, const BwdErrors E) {
    constexpr bool WGT = false, DEBUG = false, SAT = false, PRF = false, VAR = true, SUN = false, COL = false;
    float *const dir_out = nullptr; double *const score_out = nullptr;
    const BwdWeights W{};
    const BwdSat S{};
    const BwdProfiles P{};
    const BwdSun N{};
#include "mi3d_kernel_backward_body.inc"
}

template <bool COUNT>
__global__ void __launch_bounds__(256)
k_backward_vs(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, const BwdSat S, const BwdErrors E) {
    constexpr bool WGT = false, DEBUG = false, SAT = true, PRF = false, VAR = true, SUN = false, COL = false;
    float *const dir_out = nullptr; double *const score_out = nullptr;
    const BwdWeights W{};
    const BwdProfiles P{};
    const BwdSun N{};
#include "mi3d_kernel_backward_body.inc"
}

// The standard error of the mean of pixel p from the raw sums of its n = bwd_pixel_ids(N, npix, p) scores and of their squares:
// sqrt(max(rad2 - rad^2 / n, 0) / (n (n - 1))), float64 throughout and rounded once; 0 where n < 2 (include/mi3d.h, mi3d_get_radiance_se)
__global__ void __launch_bounds__(256)
k_backward_norm_se(const double *__restrict__ tally, const double *__restrict__ tally2, float *__restrict__ out, unsigned long long nphoton, unsigned npix) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const unsigned long long cnt = bwd_pixel_ids(nphoton, npix, p);
    float se = 0.0f;
    if (cnt >= 2ull) {
        const double nn = (double)cnt, t = tally[p];
        const double q = t * t;
        const double ss = fmax(tally2[p] - q / nn, 0.0);
        se = (float)sqrt(ss / (nn * (nn - 1.0)));
    }
    out[p] = se;
}

// The histories of k_backward_v with the sunlight term of a solar+thermal job (mi3d_set_view_sunlight 1): the same body
// with SUN.  (They stand behind every other history kernel so that the code of the kernels before them lies where it lay.)
template <bool COUNT, bool DEBUG>
__global__ void __launch_bounds__(256)
k_backward_vn(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, float *__restrict__ dir_out, double *__restrict__ score_out,
              const BwdSat S, const BwdSun N) {
    constexpr bool WGT = false, SAT = true, PRF = false, VAR = false, SUN = true, COL = false;
    const BwdWeights W{};
    const BwdProfiles P{};
    const BwdErrors E{};
#include "mi3d_kernel_backward_body.inc"
}

template <bool COUNT>
__global__ void __launch_bounds__(256)
k_backward_vns(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, const BwdSat S, const BwdErrors E, const BwdSun N) {
    constexpr bool WGT = false, DEBUG = false, SAT = true, PRF = false, VAR = true, SUN = true, COL = false;
    float *const dir_out = nullptr; double *const score_out = nullptr;
    const BwdWeights W{};
    const BwdProfiles P{};
#include "mi3d_kernel_backward_body.inc"
}

// The histories of the satellite views under independent columns and partial 3-D (mi3d_set_view_columns 1): the same body
// with COL -- a history keeps the column under its start, every layer is crossed level to level, the x / y faces and the moves between
// columns are compiled out.  One entry point per SAT build: plain, errors, profiles, sunlight, sunlight with errors.  With sunlight the
// ray keeps the column too (independent columns) or flies through the cyclic grid as the direct beam (partial 3-D): N.ray3d, one build.
// (They stand behind every other history kernel so that the code of the kernels before them lies where it lay.)
template <bool COUNT, bool DEBUG>
__global__ void __launch_bounds__(256)
k_backward_vc(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, float *__restrict__ dir_out, double *__restrict__ score_out,
              const BwdSat S) {
    constexpr bool WGT = false, SAT = true, PRF = false, VAR = false, SUN = false, COL = true;
    const BwdWeights W{};
    const BwdProfiles P{};
    const BwdErrors E{};
    const BwdSun N{};
#include "mi3d_kernel_backward_body.inc"
}

template <bool COUNT>
__global__ void __launch_bounds__(256)
k_backward_vcs(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, const BwdSat S, const BwdErrors E) {
    constexpr bool WGT = false, DEBUG = false, SAT = true, PRF = false, VAR = true, SUN = false, COL = true;
    float *const dir_out = nullptr; double *const score_out = nullptr;
    const BwdWeights W{};
    const BwdProfiles P{};
    const BwdSun N{};
#include "mi3d_kernel_backward_body.inc"
}

template <bool COUNT>
__global__ void __launch_bounds__(256)
k_backward_vcp(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, const BwdSat S, const BwdProfiles P) {
    constexpr bool WGT = false, DEBUG = false, SAT = true, PRF = true, VAR = false, SUN = false, COL = true;
    float *const dir_out = nullptr; double *const score_out = nullptr;
    const BwdWeights W{};
    const BwdErrors E{};
    const BwdSun N{};
#include "mi3d_kernel_backward_body.inc"
}

template <bool COUNT, bool DEBUG>
__global__ void __launch_bounds__(256)
k_backward_vcn(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, float *__restrict__ dir_out, double *__restrict__ score_out,
               const BwdSat S, const BwdSun N) {
    constexpr bool WGT = false, SAT = true, PRF = false, VAR = false, SUN = true, COL = true;
    const BwdWeights W{};
    const BwdProfiles P{};
    const BwdErrors E{};
#include "mi3d_kernel_backward_body.inc"
}

template <bool COUNT>
__global__ void __launch_bounds__(256)
k_backward_vcns(const DevBackward A, const uint64_t seed, const uint64_t id0, const uint64_t n, const BwdSat S, const BwdErrors E, const BwdSun N) {
    constexpr bool WGT = false, DEBUG = false, SAT = true, PRF = false, VAR = true, SUN = true, COL = true;
    float *const dir_out = nullptr; double *const score_out = nullptr;
    const BwdWeights W{};
    const BwdProfiles P{};
#include "mi3d_kernel_backward_body.inc"
}

// The dynamic LDS of a launch of any build, in bytes: the host's statement of what the top of mi3d_kernel_backward_body.inc lays out, in
// that order -- the workgroup's image sums [npix] (lds_sums), their squares [npix] (lds_sums and var), the staged layer and surface
// weights [npix][nls] (wstage), the layer table [nz], the cameras or -- sat -- the views [nview]; each of the sums rounded up to an even
// number of doubles
__host__ inline size_t backward_lds(int npix, int nz, int nview, int nls, bool lds_sums, bool wstage, bool sat, bool var = false) {
    const size_t sums = lds_sums ? (((size_t)npix + 1) & ~(size_t)1) : 0, wsum = wstage ? (((size_t)npix * nls + 1) & ~(size_t)1) : 0;
    return (sums * (var ? 2 : 1) + wsum) * sizeof(double) + (size_t)nz * sizeof(LayerRec) + (size_t)nview * (sat ? sizeof(ViewRec) : sizeof(CamRec));
}
// are the image's sums taken per workgroup in LDS?  Not by the debug entries, which tally nothing, and not under the tile hand-out, which
// keeps them in registers (the body's `lds_sums`).  The builds with a second tally (var) take half the pixels: the same bytes at most
__host__ inline bool backward_lds_sums(int npix, bool debug, bool tiles, bool var = false) {
    return !debug && npix <= (var ? kBwdLdsPixErr : kBwdLdsPix) && !tiles;
}
// The weights build stages its layer and surface weights where the image's own sums are in LDS and the workgroup's dynamic LDS stays
// within 32 KB (five workgroups on a CU of 160 KB)
constexpr size_t kBwdWgtLds = 32768;

} // namespace mi3d
