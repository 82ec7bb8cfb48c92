/*
 * mi3d.h — C-ABI of libmi3drt.so, the MI355X-native 3D Monte-Carlo radiative-transfer solver.
 *
 * This library replaces the photon-transport program that the reference toolbox (hong-chen/er3t)
 * launches as a subprocess.  The reference has no FFI for this path; its interface is
 *
 *     os.system("<MCARATS_V010_EXE> <Nphoton> <solver 0|1|2> <inp.txt> <out.bin>")
 *                                         (er3t/rtm/mca/mca_run.py:101-115,179-181)
 *
 * where <inp.txt> is a Fortran namelist (er3t/rtm/mca/mca_inp.py:15-384,636-697) naming three
 * little-endian float32 side files (er3t/rtm/mca/mca_atm.py:373-389, mca_sca.py:82-92,
 * mca_sfc.py:136-146) and <out.bin> is a float32 Fortran-order dump described by a GrADS .ctl
 * (er3t/rtm/mca/mca_out.py:48-103).  Every entry point below states which piece of that contract
 * it replaces.  Host arrays are given in exactly the layout of the reference's side files, so a
 * caller can hand over `np.fromfile(side_file, '<f4')` unchanged.
 *
 * Conventions
 *   - every function returns 0 on success or a negative MI3D_E* code; the message for the calling
 *     thread's last failure is available from mi3d_last_error().
 *   - host input buffers are owned by the caller and only read during the call (the library
 *     copies them to the device).  Output buffers are caller-allocated.
 *   - a handle is not re-entrant; different handles may be used from different threads.
 *   - angles are degrees, lengths metres, in the solver's own conventions (Src_the = 180 - SZA,
 *     azimuth = direction of photon travel / camera pointing, counter-clockwise from +x = east;
 *     er3t/rtm/mca/mcarats.py:374-383,527-549).
 */
#ifndef MI3D_H
#define MI3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI3D_VERSION 100 /* 0.1.0 */

/* error codes */
#define MI3D_OK 0
#define MI3D_EINVAL (-1)   /* bad argument / inconsistent shapes            */
#define MI3D_ESTATE (-2)   /* call order (e.g. run before set_atm1d)        */
#define MI3D_EDEVICE (-3)  /* HIP runtime failure (no GPU, OOM, launch)     */
#define MI3D_EUNSUP (-4)   /* valid MCARaTS option this solver does not do  */

/* limits (compile-time table sizes in the kernels) */
#define MI3D_MAX_NP1D 4    /* scattering components of the 1-D background   */
#define MI3D_MAX_NP3D 4    /* scattering components of the 3-D region       */
#define MI3D_MAX_VIEW 16   /* radiance view directions per launch           */
#define MI3D_NCOUNTER 24   /* length of the counter vector, see below       */

/* target (Wld_mtarget, er3t/rtm/mca/mcarats.py:267-287) */
#define MI3D_TARGET_FLUX 1
#define MI3D_TARGET_RADIANCE 2
#define MI3D_TARGET_HEAT 4 /* heating rates beside the fluxes: Flx_mhrt = 1 (mcarats.py:279-283; mca_inp.py:124); with MI3D_TARGET_FLUX
                            * (a thermal job: the NET heating rate, Flx_mhrt = 2, see mi3d_get_heating) */

/* solver (2nd CLI argument of the reference's command line, mcarats.py:450-454) */
#define MI3D_SOLVER_3D 0
#define MI3D_SOLVER_P3D 1 /* partial 3-D: 3-D direct beam, independent columns for all scattered light */
#define MI3D_SOLVER_IPA 2

/* surface model ids (Sfc_mtype / jsfc2d, er3t/rtm/mca/mca_sfc.py:94-128) */
#define MI3D_SFC_LAMBERT 1
#define MI3D_SFC_DSM 2 /* diffuse-specular mixture (whitecaps + Cox-Munk facets): five parameters */
#define MI3D_SFC_LSRT 4

/* indices into the counter vector returned by mi3d_get_counters (all uint64, summed over
 * every run since the last mi3d_reset).  These are the measured quantities SURVEY.md §8(d)
 * builds the algorithmic-bytes figure from. */
#define MI3D_CNT_PHOTONS 0      /* photon histories completed                              */
#define MI3D_CNT_STEPS 1        /* cell-boundary steps + collision stops during transport  */
#define MI3D_CNT_STEPS3D 2      /* ... of which inside the 3-D region (one ext read each)  */
#define MI3D_CNT_SCATTER 3      /* scattering collisions                                   */
#define MI3D_CNT_SURFACE 4      /* surface reflections                                     */
#define MI3D_CNT_LE_RAYS 5      /* local-estimate rays cast (events x views)               */
#define MI3D_CNT_LE_STEPS 6     /* cell steps walked by local-estimate rays                */
#define MI3D_CNT_LE_STEPS3D 7   /* ... of which inside the 3-D region                      */
#define MI3D_CNT_LE_COLUMN 8    /* LE rays answered from the vertical optical-depth table  */
#define MI3D_CNT_FLUX_TALLY 9   /* flux plane crossings tallied                            */
#define MI3D_CNT_ROULETTE 10    /* Russian-roulette games played                           */
#define MI3D_CNT_KILLED 11      /* histories ended by roulette                             */
#define MI3D_CNT_ESCAPED 12     /* histories that left through the top                     */
#define MI3D_CNT_ABSORBED 13    /* histories ended with zero weight (black surface/voxel)  */
#define MI3D_CNT_SCHED_A_LANES 14 /* scheduler diagnostics: lanes that stepped / lane slots offered */
#define MI3D_CNT_SCHED_A_SLOTS 15
#define MI3D_CNT_SCHED_B_LANES 16 /* lanes with an event pending / lane slots of event passes       */
#define MI3D_CNT_SCHED_B_SLOTS 17
#define MI3D_CNT_TICKS_A 18     /* wave clock ticks / 64, summed over lanes, spent in: voxel steps,     */
#define MI3D_CNT_TICKS_B0 19    /* uniform-layer runs,                                                  */
#define MI3D_CNT_TICKS_B12 20   /* events and their tallies,                                            */
#define MI3D_CNT_TICKS_B34 21   /* starting marched views and handing out photon ids,                   */
#define MI3D_CNT_TICKS_B5 22    /* the finish block (new direction),                                    */
#define MI3D_CNT_TICKS_B6 23    /* the Philox block                                                     */

typedef struct mi3d_solver mi3d_solver;

int mi3d_version(void);
const char *mi3d_last_error(void);

/* Number of visible HIP devices (0 if none / runtime unusable). Does not create a context. */
int mi3d_device_count(void);

/* Create a solver bound to HIP device `device`.  Replaces process start-up of the reference's
 * solver executable (mca_run.py:179-181).  Fails with MI3D_EDEVICE when no GPU is usable: there
 * is no CPU fallback. */
int mi3d_create(int device, mi3d_solver **out);
int mi3d_destroy(mi3d_solver *h);

/* 1-D background atmosphere = namelist keys Atm_nz, Atm_zgrd0, Atm_np1d, Atm_ext1d(1:,ip),
 * Atm_omg1d(1:,ip), Atm_apf1d(1:,ip), Atm_abs1d(1:,1)   (er3t/rtm/mca/mca_atm.py:68-139).
 *   zgrd[nz+1]  level heights, ascending, zgrd[0] is the surface
 *   ext/omg/apf [np1d][nz] (component-major, layer index fastest), abs[nz]
 * apf selects the phase function of a component (mca_atm.py:101,262,276; rtm/mca/util.py:153):
 *   apf <= -1.5 isotropic; -1.5 < apf <= -1 Rayleigh; -1 < apf < 1 Henyey-Greenstein with g=apf;
 *   apf >= 1 tabulated, 1-based real table index (fraction = mix of the two neighbours). */
int mi3d_set_atm1d(mi3d_solver *h, int nz, const double *zgrd, int np1d, const float *ext,
                   const float *omg, const float *apf, const float *abs);

/* 3-D region = keys Atm_nx, Atm_ny, Atm_dx, Atm_dy, Atm_nz3, Atm_iz3l, Atm_np3d and the side file
 * Atm_inpfile (er3t/rtm/mca/mca_atm.py:231-337,373-389).  Arrays are in the FILE layout: x
 * fastest, then y, then z; component blocks one after another:
 *   abst[nz3][ny][nx]  gas-absorption perturbation added to abs1d of the layer (may be NULL = 0)
 *   extp/omgp/apfp [np3d][nz3][ny][nx]
 * iz3l is the 1-based index of the lowest 3-D layer exactly as the namelist carries it.
 * Atm_tmpa3d (temperature perturbation) is not needed for solar transport and is not passed here: a thermal job hands it
 * to mi3d_set_thermal.
 * nz3 == 0 removes the 3-D region (then nx, ny give the horizontal tally grid only). */
int mi3d_set_atm3d(mi3d_solver *h, int nx, int ny, int nz3, int iz3l, int np3d, double dx,
                   double dy, const float *abst, const float *extp, const float *omgp,
                   const float *apfp);

/* Tabulated phase functions = keys Sca_npf, Sca_nangi and the side file Sca_inpfile
 * (er3t/rtm/mca/mca_sca.py:72-92): ang[nang] degrees ascending from 0 to 180, pha[npf][nang].
 * Tables are renormalised to (1/2)∫P dμ = 1 and treated as piecewise linear in μ = cos(angle).
 * npf == 0 clears the tables. */
int mi3d_set_phase(mi3d_solver *h, int nang, int npf, const float *ang, const float *pha);

/* Uniform surface = keys Sfc_mtype, Sfc_param(1:5) (er3t/rtm/mca/mcarats.py:393-399). */
int mi3d_set_surface(mi3d_solver *h, int mtype, const float param[5]);

/* 2-D surface = keys Sfc_nxb, Sfc_nyb and the side file Sfc_inpfile
 * (er3t/rtm/mca/mca_sfc.py:81-146), file layout: tmps[nyb][nxb] (ignored, may be NULL: a thermal job hands it to mi3d_set_thermal),
 * jsfc[nyb][nxb] (model id stored as float), psfc[5][nyb][nxb]. */
int mi3d_set_surface2d(mi3d_solver *h, int nxb, int nyb, const float *tmps, const float *jsfc,
                       const float *psfc);

/* Solar source = keys Src_flx, Src_qmax, Src_the, Src_phi (er3t/rtm/mca/mcarats.py:374-383). */
int mi3d_set_source(mi3d_solver *h, double flx, double qmax_deg, double the_deg, double phi_deg);

/* Thermal source = keys Src_mtype, Src_wlen, Atm_tmp1d, the Atm_tmpa3d block of Atm_inpfile and the Sfc_tmps2d block of
 * Sfc_inpfile (er3t/rtm/mca/mca_inp.py:287 "0:local 1:solar 2:solar+thermal 3:thermal"; mca_atm.py:73,175-214; mca_sfc.py:74).
 * Src_wlen, the band-centre wavelength in micrometres, is a key of THIS project in the Src group: MCARaTS' own thermal inputs cannot
 * be confirmed, its source is not in the reference.  Src_dwlen is accepted and ignored: the source is monochromatic at Src_wlen.
 *   mtype    3 thermal; 2 solar+thermal, with the arguments of 3 (see mi3d_set_solar_irradiance below); 1 switches the handle back
 *            to the solar source (the other arguments are then ignored); 0 (local): MI3D_EUNSUP
 *   wlen_um  Src_wlen [um], > 0
 *   nlev     must be nz+1: tmp1d[nz+1] holds the INTERFACE temperatures [K] from the surface up (MCARaTS: Atm_tmp1d(KNZ+1))
 *   tmpa3d   [nz3][ny][nx] voxel temperature anomalies [K] in the file layout of mi3d_set_atm3d, or NULL (0)
 *   tmps2d   [nyb][nxb] surface temperature anomalies [K] of the 2-D surface of mi3d_set_surface2d, or NULL (0)
 * Call after mi3d_set_atm1d / mi3d_set_atm3d / mi3d_set_surface2d of the scene: mi3d_prepare checks the sizes again.
 * Physics contract ("Thermal source"):
 *   B(wl, T) = 2 h c^2 / wl^5 / (exp(h c / (wl k T)) - 1) in W m-2 sr-1 um-1 (CODATA 2018 h, c, k), times Src_flx;
 *            B(10 um, 300 K) = 9.92403, B(11 um, 288 K) = 7.96577, B(4 um, 250 K) = 0.0656295
 *   a 1-D layer emits at the mean of its two interface temperatures, a voxel at that mean plus its anomaly, the surface at
 *   tmp1d[0] (plus its anomaly).  Emitted power: 4 pi ka B(T) V per cell, ka = gas absorption (abs1d + abst3d) + ext (1 - omega)
 *   summed over every constituent; pi (1 - albedo) B(Ts) A per surface cell, Lambertian surfaces only (else MI3D_EUNSUP at
 *   mi3d_prepare).  Volume emission is isotropic, surface emission follows the cosine law.
 *   Results: radiance (Rad_mrkind = 2) in W m-2 sr-1 um-1, fluxes in W m-2 um-1 (mi3d_get_radiance / mi3d_get_flux /
 *   mi3d_stats_add: the normalisation is Src_flx P_tot / N in place of Src_flx mu0 Lx Ly / N).  No direct beam: the direct-down
 *   plane is 0 and the analytic direct-beam levels are off.  A thermal job runs on the general photon loop
 *   (mi3d_last_kernel: "k_transport<...> [thermal]", followed by " [heating: path length]" under that estimator); its cameras
 *   (Rad_mrkind = 1) are served as stated at mi3d_set_cameras, "Thermal cameras".  Under MI3D_SOLVER_P3D every thermal photon stays
 *   in its column (no photon is direct).
 *   Heating rates (MI3D_TARGET_FLUX | MI3D_TARGET_HEAT, the project's key Flx_mhrt = 2): the NET, absorbed minus emitted --
 *   longwave cooling where negative; see mi3d_get_heating and mi3d_get_emission.  The emission event deposits nothing; the first
 *   flight is tallied from the emission point (path-length estimator: the part of the cell from that point to the first face or
 *   collision).  A source that emits nothing (P_tot = 0) runs no photon: every result is 0. */
int mi3d_set_thermal(mi3d_solver *h, int mtype, double wlen_um, int nlev, const float *tmp1d, const float *tmpa3d,
                     const float *tmps2d);

/* Solar+thermal source (Src_mtype = 2, mi3d_set_thermal 2) = the keys of the thermal source, the sun's direction Src_the, Src_phi, Src_qmax
 * of mi3d_set_source, and Src_fsol: the solar spectral irradiance on a plane normal to the beam at the top of the atmosphere in
 * W m-2 um-1, >= 0.  Src_fsol is a key of THIS project in the Src group (as Src_wlen), written only when Src_mtype = 2.  For the
 * 3-5 um channels, where reflected sunlight and emission are the same size.
 *   fsol     negative or not finite: MI3D_EINVAL.  The handle keeps the value; it is ignored under mtype 1 and 3.  With mtype 2 and no
 *            irradiance set, mi3d_prepare and mi3d_run return MI3D_ESTATE.
 * Contract: one job, two sources, equal-weight photons.
 *   P_tot    the emitted power of the thermal source [W um-1]; P_sol = Src_fsol mu0 Lx Ly, mu0 = |cos Src_the|, in float64.
 *   A photon is thermal with probability P_tot / (P_tot + P_sol), otherwise solar; every photon starts with weight 1 and stands for
 *   Src_flx (P_tot + P_sol) / N.  mi3d_get_radiance, _flux, _heating and mi3d_stats_add normalise with that amplitude, so a result is
 *   Src_flx x (thermal result + Src_fsol x solar result per unit irradiance): absolute W m-2 (sr-1) um-1 for Src_flx = 1.
 *   Sampling: (seed, id) -> history stays a function.  Draw 0 is the launch block; the 46-bit number u of draw 1 (the block a
 *   thermal launch draws for its cell) gives target = u (P_tot + P_sol).  target < P_tot: a thermal photon, launched as
 *   mi3d_set_thermal 3 launches it for that very target -- with Src_fsol = 0 a mixed job walks the thermal job's histories id for
 *   id.  Otherwise a solar photon, launched from draw 0 as a solar job launches it (position at the top, cone jitter); it has spent
 *   one more block than a solar job's and agrees with it statistically, not id by id.  No stratification by id: id ranges add
 *   and ranks shard as for every other job.
 *   Direct beam: the analytic direct-beam levels are off (they are per unit Src_flx mu0): the solar photons tally the direct-down
 *   plane at every level, the top included.  Under MI3D_SOLVER_P3D a solar photon is direct (3-D) until its first event, a
 *   thermal photon never is.
 *   Heating rates (Flx_mhrt = 2): the net, absorbed from both sources under either estimator minus emitted; mi3d_get_emission works.
 *   As for the thermal source: Lambertian surfaces only, cameras MI3D_EUNSUP, the general photon loop in id order
 *   (mi3d_last_kernel: "k_transport<...> [solar+thermal]", followed by " [heating: path length]" under that estimator).
 *   P_tot = 0 and P_sol = 0: no photon runs, every result is 0 and mi3d_last_kernel says so.  P_tot = 0, Src_fsol > 0: every
 *   photon is solar. */
int mi3d_set_solar_irradiance(mi3d_solver *h, double fsol);
/* The two powers of a thermal or solar+thermal job [W um-1, per unit Src_flx]: *ptot = P_tot, *psol = P_sol (0 for a thermal job);
 * either pointer may be NULL.  Builds the source first if needed (mi3d_prepare); needs no run.  MI3D_ESTATE for a solar job. */
int mi3d_get_source_power(mi3d_solver *h, double *ptot, double *psol);

/* Radiance views = keys Rad_nrad, Rad_the, Rad_phi, Rad_zloc, Rad_zref, Rad_nxr, Rad_nyr for
 * Rad_mrkind = 2 (pixel-averaged radiance; er3t/rtm/mca/mcarats.py:285-307,360-367).  The
 * reference passes one view per solver process; this library takes up to MI3D_MAX_VIEW per
 * launch.  the_deg > 90: down-looking sensor (180 = nadir; Rad_the = 180 - sensor_zenith_angle,
 * mcarats.py:305): zloc[] is the sensor height, radiance is collected where the line of sight
 * crosses min(zloc, top of atmosphere) and registered to the pixel where it meets z = zref.
 * the_deg < 90: up-looking sensor (0 = zenith; "looking up, 180 deg straight up",
 * mcarats.py:499-502): light travelling down to a plane of sensors at max(zloc, surface), from
 * events above it only, registered where the line of sight meets that plane.  the_deg = 90
 * (horizontal) is rejected. */
int mi3d_set_views(mi3d_solver *h, int nview, const double *the_deg, const double *phi_deg,
                   const double *zloc, double zref, int nxr, int nyr);

/* All-sky cameras: Rad_mrkind = 1, "local radiance averaged over solid angle" (er3t/rtm/mca/mca_inp.py:141-144; set by
 * er3t/rtm/mca/mcarats.py:291-296, 369-372 for sensor_type = 'all-sky': Rad_qmax = 178, Rad_apsize = 0.05, Rad_xpos/ypos,
 * a 500 x 500 image).  Replaces mi3d_set_views for the job (a job has one kind of radiance).  Camera i stands at
 * (xpos[i] Lx, ypos[i] Ly, zloc[i]); its axes are the world axes turned by the Z-Y-Z rotations phi, the, psi (Rad_phi,
 * Rad_the, Rad_psi, mca_inp.py:324-330) and it looks along its z axis (the = 180: straight down, the = 0: straight up, as
 * for the satellite views); it sees directions within qmax/2 degrees of that axis (Rad_qmax: full angle of the cone).  Pixel
 * map: polar, Rad_mpmap = 1: a direction at angle theta from the axis and azimuth phi about it falls at U = theta cos(phi),
 * V = theta sin(phi), the image spanning umax x vmax degrees (Rad_umax, Rad_vmax) in nxr x nyr pixels.  Estimator: every
 * collision and reflection sends w P / (4 pi) exp(-tau) / r^2 (surface: w R cos / pi ...) to the nearest periodic image of
 * the camera, r not counted below apsize metres (Rad_apsize); 3-D solver only.  MCARaTS' own regularisation of the 1/r^2
 * estimator (Rad_difr*, Rad_rmin0 ...) is not in the reference tree and not applied: see DESIGN.md.
 * Thermal cameras (mi3d_set_thermal 3 with cameras): a pyrgeometer, an up- or down-looking IR radiometer, a thermal
 * sky imager.  Served: the 3-D solver over Lambertian surfaces (what a thermal job needs anyway), the polar map (all-sky images) and
 * the rectangular map with Rad_mrproj 0 or 1 (actinic and irradiance radiometers), up to MI3D_MAX_VIEW sensors anywhere in the scene
 * in any orientation.
 *   Units      pixel values are absolute mean radiances over the pixel's (weighted) solid angle in W m-2 sr-1 um-1 per unit Src_flx,
 *              the unit of a thermal satellite view's pixels: mi3d_get_radiance and mi3d_stats_add normalise the tallies with
 *              src_amp Lx Ly / N, src_amp = Src_flx P_tot / (Lx Ly).
 *   Estimator  every event of a thermal photon sends its local estimate to every image of every sensor within cam_images domain
 *              lengths of the nearest one: its emission (a volume cell: w / (4 pi r^2); the surface: w cos(theta) / (pi r^2), never
 *              seen from below) and every later scattering or Lambertian reflection.  The Russian roulettes on farther images, on
 *              the optical depth and on the weight are the solar camera's, with the same hashes of (photon id, index of the
 *              photon's Philox block, view, image): (seed, id) -> contributions is a function whichever kernels serve the job.
 *   No direct term: a thermal job has no sun.  mi3d_get_camera_direct returns zeros (nothing is marched towards Src_the) and
 *              mi3d_stats_add adds nothing.
 *   Route      where the lean loops' limits hold (at most two 3-D constituents, phase tables that fit the LDS, 16-bit cell
 *              numbers, voxel records below 4 GB, no mi3d_set_kernel 1): builds of the general loop that write an event record per
 *              emission, collision and reflection, and the thermal camera build of the ray kernel behind them
 *              (mi3d_last_kernel: "k_transport<C,2,0,0> [thermal] + k_rays"), cam_images -1 standing for 2.  Anything else: the
 *              general loop with the rays in the photons' lanes ("k_transport<...> [thermal]") serves the NEAREST image alone, as
 *              for a solar camera: cam_images > 0 is then refused (MI3D_EUNSUP), the default -1 warned about once per handle.
 *   Solar+thermal jobs (mi3d_set_thermal 2) with cameras: MI3D_EUNSUP from mi3d_run -- their direct sun would need a second
 *              normalisation.
 *   The 1 / r^2 of an event inside the medium around a sensor is bounded by the Rad_apsize clamp alone: a sensor inside an
 *              absorbing layer reads low by the order of ka x apsize x B (what the clamp removes) and its noise is heavy-tailed.
 *              mi3d_set_camera_method 1 serves the same sensors backwards, without the clamp and without cam_images. */
int mi3d_set_cameras(mi3d_solver *h, int ncam, const double *the_deg, const double *phi_deg, const double *psi_deg,
                     const double *xpos, const double *ypos, const double *zloc, const double *qmax_deg,
                     const double *umax_deg, const double *vmax_deg, const double *apsize, int nxr, int nyr);
/* Pixel map and weighting of the cameras = keys Rad_mpmap, Rad_mrproj (er3t/rtm/mca/mca_inp.py:306-311: a camera with the
 * rectangular map, one pixel, Rad_umax = 90 is an irradiance (mrproj = 1) or actinic-flux (mrproj = 0) sensor).  Default (1, 0): the
 * polar map above, the mean radiance over the pixel -- what mi3d_set_cameras alone gives.
 *   mpmap 2  rectangular map: U = theta in [0, umax] over nxr columns, V = phi in [-vmax, vmax] over nyr rows, theta measured from the
 *            camera's axis and phi about it from the image x axis.  MCARaTS' own convention for this map is not in the reference
 *            tree; this reading (a key value of THIS project's choosing, like Src_wlen) makes the documented sensor, Rad_umax = 90 with
 *            the default Rad_vmax = 180, a full hemisphere.  Needs umax, vmax <= 180 (MI3D_EINVAL from the next run otherwise).
 *            Pixel value = (sum of w L dOmega over the pixel) / W, W its exact weighted solid angle: (cos t_i - cos t_i+1) dphi
 *            (mrproj 0, w = 1) or (sin^2 t_i+1 - sin^2 t_i) dphi / 2 (mrproj 1, w = cos theta; needs umax <= 90).
 *   mrproj 1 on the polar map: the same weight; its per-direction solid angle times cos theta is the denominator, so the weight
 *            cancels direction by direction and the image equals that of mrproj 0.
 * mi3d_get_radiance holds the scattered light only, for every map: the direct sun is mi3d_get_camera_direct. */
int mi3d_set_camera_map(mi3d_solver *h, int mpmap, int mrproj);

/* How the cameras and point radiometers of a THERMAL job are served: 0 (default) the forward route above, 1 backward (adjoint) Monte
 * Carlo (er3t_amd/csrc/mi3d_kernel_backward.hip; the project's namelist key Rad_mbwd = 1).  A history starts at the
 * sensor and flies backwards along a line of sight; it collects ka B(T) along its path and eps B(Ts) at the surface.  No 1 / r^2, no
 * Rad_apsize clamp -- a sensor may stand inside an absorbing or cloudy cell --, and no cam_images / Rad_nimg: a line of sight wraps
 * through the cyclic domain, all of which is seen.  The forward route is untouched by the choice.
 *   Served     Src_mtype = 3, cameras (Rad_mrkind = 1), the 3-D solver, Lambertian surfaces (uniform or 2-D, Sfc_tmps2d included): the
 *              limits of the forward thermal cameras.  Solar and solar+thermal jobs, satellite views, flux jobs, independent columns,
 *              partial 3-D and non-Lambertian surfaces: MI3D_EUNSUP from mi3d_run, with the reason.  A sensor on or below the surface:
 *              MI3D_EINVAL.  mi3d_last_kernel: "k_backward<C> [thermal]".
 *   Pixel      npix = nview nyr nxr; history id belongs to the flat pixel p = id mod npix in the layout of the radiance tally: stratified,
 *              so that a near-uniform radiance field keeps its near-zero variance.  The ids of a job are expected to cover
 *              [0, nphoton_total): mi3d_get_radiance and mi3d_stats_add divide pixel p, on the device, by the exact number of ids in
 *              that range that map to it, floor(N / npix) + (p < N mod npix); a pixel with none reads 0.  Raw tallies add over id
 *              ranges and ranks as for every other job.
 *   Direction  Philox block 0 of (seed, id): u0, u1 place the line of sight inside the pixel with the pixel's own weight, so that a score
 *              is an unbiased sample of the pixel value as the forward route defines it.  Polar map: (U, V) uniform over the pixel's
 *              square, theta = hypot(U, V), phi = atan2(V, U).  Rectangular map: phi uniform over the row; cos(theta) uniform over the
 *              column (Rad_mrproj = 0) or sin^2(theta) (Rad_mrproj = 1).  Outside the cone Rad_qmax / 2 or theta > pi: the score is 0.
 *   Start      at the sensor, in the cell that contains it (on a level or a cell face the direction decides); a sensor above the top
 *              starts where its line enters the top, folded into the domain, and scores 0 if it never enters.
 *   Flight     the free path is sampled from the SCATTERING coefficient alone (block c: u0 -> -ln u0); absorption is continuous: a
 *              segment of length l inside one cell adds w B (1 - exp(-ka l)) and then w *= exp(-ka l), with exactly the ka and T of the
 *              forward source (total extinction - total scattering of the float32 records; layer-mean temperature + Atm_tmpa3d), rounded
 *              to float32 once.  Segments end at voxel faces inside the 3-D region (its uniform layers included: Atm_tmpa3d may vary),
 *              at levels outside it.
 *   Events     scattering: the constituent in proportion to k_s (u1), cos of the angle from its phase function (u2), azimuth (u3).
 *              Surface: the score gets w eps B(Ts), w *= albedo, the new direction follows the cosine law and comes from the NEXT block
 *              (u0, u1; u2 its roulette).  Top: the history ends, space is cold.  The roulette after a scattering takes u0 of a block
 *              of its own, drawn only when it is played.  Blocks are consumed in sequence; (seed, id) -> score depends on nothing else.
 *   Ending     the weight roulette (Pho_wmin, Pho_wfac) is played after a scattering or a reflection only: a scene that never scatters over
 *              a black surface is deterministic given the direction.  A history whose weight falls below 1e-7 ends: a bias of at most
 *              1e-7 max B, below float32 resolution.  A history that has taken 2^20 cell steps ends and is counted as CAPPED
 *              (mi3d_debug_backward): a near-horizontal line through an empty layer would not end otherwise; for a hemispheric sensor in a
 *              gap of height dz the share lost is of the order of (dz / (2^20 dx))^2 of an irradiance.
 *   Units      those of the forward thermal cameras: absolute pixel-mean radiance in W m-2 sr-1 um-1 (the score carries Src_flx).
 *              mi3d_get_camera_direct stays zeros.  Counters (counting builds): photons = histories, steps, steps3d, scatter, surface. */
int mi3d_set_camera_method(mi3d_solver *h, int method);

/* How the satellite views (mi3d_set_views, Rad_mrkind = 2) of a THERMAL job are served: 0 (default) the forward route -- local estimates
 * from every emission and collision --, 1 backward (adjoint) Monte Carlo (er3t_amd/csrc/mi3d_kernel_backward.hip; the
 * project's namelist key Rad_mvbwd = 1).  A history starts on the sensor plane of its pixel's view and flies backwards along the view's
 * line of sight; from its first flight on it is the history of mi3d_set_camera_method 1.  Every pixel gets the same number of
 * histories.  The forward route, and mi3d_set_camera_method with every refusal it has, are untouched by the choice; anything but 0 or 1
 * is MI3D_EINVAL.
 *   Served     Src_mtype = 3, the views of mi3d_set_views, a radiance job of the 3-D solver, Lambertian surfaces (uniform or 2-D, Sfc_tmps2d
 *              included).  Solar and solar+thermal jobs, flux jobs, independent columns, partial 3-D, non-Lambertian surfaces, and
 *              mi3d_set_emission_weights 1 (an image times the cells): MI3D_EUNSUP from mi3d_run, with the reason.  (Solar+thermal jobs
 *              have a switch of their own, mi3d_set_view_sunlight; independent columns and partial 3-D have one too, mi3d_set_view_columns.)
 *              The switch is
 *              accepted while cameras are set (mi3d_set_cameras); mi3d_run then returns MI3D_EUNSUP and names it.  A down-looking view
 *              whose sensor plane lies on or below the surface: MI3D_EINVAL.  mi3d_last_kernel: "k_backward<C,V> [thermal]".
 *   Pixel      as for mi3d_set_camera_method 1: npix = nview nyr nxr, history id belongs to the flat pixel p = id mod npix in the tally
 *              layout [view][jr][ir]; mi3d_get_radiance, mi3d_stats_add and the fused statistics divide pixel p by the exact number of
 *              ids of [0, nphoton_total) that map to it.
 *   Sample     Philox block 0 of (seed, id): u0, u1.  The point (xr, yr) = ((ir + u0) Lx / nxr, (jr + u1) Ly / nyr) lies on the view's
 *              registration level z = zreg, the level on which the forward route finds a line of sight's pixel: Rad_zref for a
 *              down-looking view, the sensor plane for an up-looking one.  v = (-sin the cos phi, -sin the sin phi, -cos the) is the unit
 *              vector towards the sensor, an all but vertical one snapped to (0, 0, +-1) as the forward route snaps it; the sensor plane is
 *              zs = min(Rad_zloc, top), raised to the surface for an up-looking view.  The pixel value is the radiance along v averaged
 *              over the pixel's footprint on z = zreg: what the forward route's tally estimates.
 *   Start      down-looking (vz > 0): (xr, yr) + (vx, vy) / vz (zs - Rad_zref), folded into the cyclic domain, at z = zs; up-looking:
 *              (xr, yr, zs).  The history flies along -v; an up-looking plane at or above the top scores 0.  On a level or a cell face
 *              the direction decides the cell.
 *   Flight, events, ending, units   those of mi3d_set_camera_method 1 from the first flight on, with the same sequence of Philox blocks
 *              (block 0 places the line, the first flight takes block 1): absolute radiance in W m-2 sr-1 um-1, the score carries Src_flx.
 *   Hand-out   mi3d_set_tuning "bwd_chunk" n >= 1: every view's image is cut into tiles of 8 x 8 pixels; a wave takes (tile, chunk of up
 *              to n consecutive histories of each of its pixels) by a fixed stride, lane L owns pixel L of the tile and sums its scores
 *              in a register, one atomic per pixel change.  0: the stride of the camera route, an atomic per history.  -1 (default): the
 *              tile hand-out with a chunk chosen per launch, at most 4: a launch whose tiles x chunks would leave resident waves
 *              without an item takes a smaller one.  Results differ by the order of float64 sums only.  "batch_log2" is read as by the
 *              camera route.  mi3d_debug_backward_chunk: the chunk of the launch made last (0: the stride).  No view set: MI3D_ESTATE. */
int mi3d_set_view_method(mi3d_solver *h, int method);
int mi3d_debug_backward_chunk(mi3d_solver *h);

/* Per-cell emission weights of the backward route (the project's namelist key Rad_mwgt = 1).  The path of a backward
 * history, its weight w and ka do not depend on any temperature, so a pixel's reading is exactly linear in the cells' Planck radiances:
 *     R_p = Src_flx  sum_c K[p][c] B_c,    K[p][c] = (1 / N_p) sum over p's histories and their segments in c of  w (1 - exp(-ka l))
 * (a surface cell: w eps).  K is dimensionless: the share of the reading that comes from cell c per unit Planck radiance there.  It
 * gives the attribution of a reading, its temperature Jacobian dR_p / dT_c = Src_flx K[p][c] dB/dT(T_c), and the reading for any other
 * temperature field over the same optical properties.
 *   Switch     mi3d_set_emission_weights: 0 (default) nothing of this runs -- kernels, names and results are those of the route without
 *              it; 1: mi3d_run serves what the backward route serves and tallies K beside the radiance; with the forward method
 *              (mi3d_set_camera_method 0) mi3d_run returns MI3D_EUNSUP and names the switch.  mi3d_last_kernel: "k_backward<C,W> [thermal]".
 *              mi3d_debug_backward ignores the switch.  Switching off frees the library's tally.
 *   Cells      ncell = nvox + nz + nxb nyb (1 x 1 for a uniform surface) in the order of the thermal source's CDF: voxels in file order
 *              [nz3][ny][nx], then the nz layers, then the surface cells [nyb][nxb].  Layers inside the 3-D region carry nothing:
 *              their voxels do.
 *   Tally      K_raw[npix][ncell], float64 on the device, npix = nview nyr nxr in the layout of the radiance tally.  Every cell step with
 *              a = w (1 - exp(-ka l)) != 0 (the float32 product) adds a to K_raw[pixel][cell]; the surface adds w eps.  No Src_flx.  The
 *              score itself is formed as before, so the radiance of a run is that of the route without the switch up to the order of
 *              its float64 sums.  Raw tallies add over id ranges and ranks; mi3d_reset zeroes them.  mi3d_bind_weights_buffer: a
 *              caller-owned device buffer [npix][ncell] float64 for an all-reduce (NULL: the library's own).
 *   Read-out   mi3d_get_emission_weights: row p divided, on the device, by the number of ids in [0, nphoton_total) that map to p (the
 *              rule of mi3d_get_radiance on this route; a pixel without a history reads 0), rounded to float32 once.  weights
 *              [npix][ncell]; planck [ncell] (may be NULL): the very float32 B the kernel multiplied with.
 *   Size       npix ncell above 2^31 elements: MI3D_EUNSUP with both numbers; all index arithmetic is 64-bit.
 *   Tuning     mi3d_set_tuning "wgt_stage" 0: the layer and surface part of the tally goes to global atomics always (default: summed per
 *              workgroup in LDS where the launch's LDS stays within 32 KB); mi3d_debug_weights_staged: what the last launch did. */
int mi3d_set_emission_weights(mi3d_solver *h, int on);
int mi3d_bind_weights_buffer(mi3d_solver *h, void *wgt_sum);
int mi3d_get_emission_weights(mi3d_solver *h, uint64_t nphoton_total, float *weights, float *planck);
int mi3d_debug_weights_staged(mi3d_solver *h);

/* Per-layer profiles of the backward route's satellite views: the vertical weighting function of every pixel (the
 * project's namelist key Rad_mvprf = 1).  An image times the cells is out of scope (mi3d_set_view_method); summed over every layer's
 * voxels and over the surface's cells it is an image times nrow = nz + 1 rows: rows 0 ... nz - 1 the layers from the surface up (a layer
 * inside the 3-D region: the sum over its voxels), row nz the surface.  Two profiles per pixel:
 *     weight        K[p][k] = (1 / N_p) sum over p's histories and their segments in layer k of  w (1 - exp(-ka l))   (surface: w eps)
 *     contribution  C[p][k] = (1 / N_p) sum of the very float32 terms the histories add to their score there: w B ka-term (surface: w eps B)
 * Neither carries Src_flx.  A history's path and weight depend on no temperature, so  R_p = Src_flx sum_k C[p][k]  for any temperature
 * field -- an exact partition of the radiance the route returns --, C / K is the layer's effective Planck radiance as pixel p sees it, and
 * Src_flx K[p][k] dB/dT is the Jacobian of R_p to the temperature of layer k where that temperature is horizontally uniform.
 *   Switch     mi3d_set_view_profiles: 0 (default) nothing of this runs -- kernels, names and results are those of the route without it,
 *              and the library's tally is freed; 1: mi3d_run serves what mi3d_set_view_method 1 serves, every refusal of that route
 *              included, and tallies the profiles beside the radiance.  With 1 and the route not selected (mi3d_set_view_method 0,
 *              cameras set, mi3d_set_camera_method 1 or mi3d_set_emission_weights 1) mi3d_run returns MI3D_EUNSUP and names this
 *              switch.  Anything but 0 or 1 is MI3D_EINVAL.  mi3d_last_kernel: "k_backward<C,V,P> [thermal]".
 *              mi3d_debug_backward_views ignores the switch.
 *   Tally      P_raw[npix][nrow][2], float64 on the device, the pair {K, C} per row, npix = nview nyr nxr in the layout of the radiance
 *              tally.  Every cell step with a = w (1 - exp(-ka l)) != 0 (the float32 product) adds a and its score term to the row of
 *              its layer, the surface w eps and w eps B to row nz.  A lane sums the terms of one (pixel, row) in registers and adds
 *              them when either changes.  The score, the Philox sequence, the hand-out and the image tally are those of the route: the
 *              radiance of a run is that of the run without the switch up to the order of its float64 sums.  Raw tallies add over id
 *              ranges and ranks; mi3d_reset zeroes them.  mi3d_bind_view_profiles_buffer: a caller-owned device buffer
 *              [npix][nz + 1][2] float64 for an all-reduce (NULL: the library's own).
 *   Read-out   mi3d_get_view_profiles: row block p divided, on the device, by the number of ids in [0, nphoton_total) that map to p (the
 *              rule of mi3d_get_radiance on this route; a pixel without a history reads 0), rounded to float32 once.  weight and
 *              contribution are [npix][nz + 1]; either may be NULL.  MI3D_ESTATE while the switch is off or nothing has run.
 *   Size       npix nrow 2 above 2^31 elements: MI3D_EUNSUP with the numbers; all index arithmetic is 64-bit. */
int mi3d_set_view_profiles(mi3d_solver *h, int on);
int mi3d_bind_view_profiles_buffer(mi3d_solver *h, void *raw);
int mi3d_get_view_profiles(mi3d_solver *h, uint64_t nphoton_total, float *weight, float *contribution);

/* Per-pixel standard errors of the backward route, from one run (the project's namelist key Rad_mserr = 1).  Every
 * history of the backward route scores in exactly one pixel, pixel id mod npix, and the histories of a pixel are independent and
 * identically distributed: the standard error of a pixel's mean follows from the sum of its scores and the sum of their squares.
 *   Switch     mi3d_set_pixel_errors: 0 (default) nothing of this runs -- kernels, names and results are those of the route without
 *              it, and the library's tally is freed; 1: mi3d_run serves thermal radiance jobs that run backwards through the plain
 *              camera build (mi3d_set_camera_method 1) or the plain satellite-view build (mi3d_set_view_method 1), every refusal of
 *              those routes included.  With 1, mi3d_run returns MI3D_EUNSUP and names this switch together with
 *              mi3d_set_emission_weights 1 or mi3d_set_view_profiles 1 (their builds are at their register limits), on a flux or
 *              heating-rate job, and on every forward route (mi3d_set_camera_method 0 and mi3d_set_view_method 0: one photon's local
 *              estimates land in many pixels, so a pixel's contributions are not independent samples).  Anything but 0 or 1 is
 *              MI3D_EINVAL.  mi3d_last_kernel: "k_backward<C,S> [thermal]" (cameras), "k_backward<C,V,S> [thermal]" (views).  The
 *              debug entries ignore the switch.
 *   Tally      When a history ends, the kernel forms s = score * Src_flx (float64: the float32 terms of the score summed in float64,
 *              times the float32 Src_flx) and adds it to rad[pixel]; mi3d_debug_backward and mi3d_debug_backward_views write the same
 *              number to score_out.  With the switch on the same place also adds s * s to rad2[pixel], float64, a tally of the shape
 *              of rad.  It takes the path s takes: summed per workgroup in LDS for images of up to 1024 pixels (half the plain build's
 *              2048: two sums per pixel in the same bytes), in a register beside the tile hand-out's, or by a global atomic.  The
 *              score, the Philox sequence, the hand-out and rad are those of the route: the radiance of a run is that of the run
 *              without the switch up to the order of its float64 sums.  Raw sums add over id ranges, launches and ranks exactly as
 *              rad does; mi3d_reset zeroes rad2.  mi3d_bind_pixel_errors_buffer: a caller-owned device buffer [npix] float64 for an
 *              all-reduce (NULL: the library's own, made and zeroed by the next run).
 *   Read-out   mi3d_get_radiance_se: for pixel p with n = the number of ids in [0, nphoton_total) that map to p (the rule of
 *              mi3d_get_radiance on this route)
 *                  se[p] = sqrt( max(rad2[p] - rad[p]^2 / n, 0) / (n (n - 1)) )
 *              the standard error of the mean mi3d_get_radiance returns, in its units; float64 on the device, rounded to float32
 *              once; 0 where n < 2.  out is [npix].  The difference cancels where a pixel's scores hardly differ: rounding may
 *              turn it negative, hence the clamp at 0, and with float64 sums of float32-born scores an se below about 1e-6 |mean| is
 *              rounding, not noise.  MI3D_ESTATE while the switch is off or when no run with the switch on has happened since the
 *              last mi3d_reset.  mi3d_get_radiance and mi3d_stats_add are untouched: they see rad alone. */
int mi3d_set_pixel_errors(mi3d_solver *h, int on);
int mi3d_bind_pixel_errors_buffer(mi3d_solver *h, void *rad2_sum);
int mi3d_get_radiance_se(mi3d_solver *h, uint64_t nphoton_total, float *out);

/* The sunlight term of the backward route's satellite views: solar+thermal jobs (Src_mtype = 2, the 3-5 um channels) served backwards
 * (er3t_amd/csrc/mi3d_kernel_backward.hip; the project's namelist key Rad_mvsun = 1).
 *   Switch     mi3d_set_view_sunlight: 0 (default) nothing of this runs -- kernels, names, refusals and results are those of the library
 *              without it; 1: mi3d_run serves Src_mtype = 2 under mi3d_set_view_method 1 with the views of mi3d_set_views.  Anything but
 *              0 or 1 is MI3D_EINVAL.  mi3d_last_kernel: "k_backward<C,V,N> [solar+thermal]", with mi3d_set_pixel_errors 1
 *              "k_backward<C,V,N,S> [solar+thermal]".  mi3d_debug_backward_views runs the same code for single histories.
 *   Refused    with the switch on, MI3D_EUNSUP from mi3d_run in words that name it: Src_mtype = 1 and 3 (the switch belongs to the mixed
 *              source; a pure solar image is a mixed job with a cold atmosphere), mi3d_set_view_method 0 or mi3d_set_camera_method 1,
 *              cameras and point radiometers (Rad_mrkind = 1), mi3d_set_view_profiles 1 (the weighting functions are per unit Planck
 *              radiance: the sun has no row), mi3d_set_emission_weights 1, a sun from below or on the horizon (Src_the - Src_qmax / 2
 *              <= 90).  Flux jobs, independent columns, partial 3-D and non-Lambertian surfaces are refused as mi3d_set_view_method 1
 *              refuses them (independent columns and partial 3-D are served with mi3d_set_view_columns 1 beside this switch).  mi3d_set_pixel_errors 1 is served: the sun's terms enter the score like every other.
 *   History    that of mi3d_set_view_method 1, untouched: free paths by the scattering coefficient, w *= exp(-ka l), emission scored per
 *              cell step, Lambert reflection with w *= 1 - eps, the same Philox blocks.  The path and the weight of history (seed, id) are
 *              those of the thermal job (Src_mtype = 3) whatever the sun does.
 *   Estimator  d = (sin the cos phi, sin the sin phi, cos the) of (Src_the, Src_phi) is the direction in which sunlight travels (d_z < 0),
 *              mu0 = |d_z|, F = Src_fsol the irradiance on a plane normal to the beam, -u the direction in which the history's light
 *              travels towards the sensor.  At a scattering, after the step's w *= exp(-ka l):
 *                  score += w P_q(d' . (-u)) / (4 pi)  F (mu0 / |d'_z|)  T(r -> top along -d')
 *              P_q the phase function of the constituent the event selected (1/2 int P dmu = 1; a mix of two tables: their mix).  At the
 *              surface, after w eps B and before w *= 1 - eps:
 *                  score += w (1 - eps) / pi  F mu0  T(r -> top along -d')
 *              T = exp(-int (ka + ks)) over every constituent along the ray, through the cyclic domain.  A history that ends at the
 *              event (roulette, weight) still scores the event's term, with the weight before the roulette.  Unscattered sunlight
 *              reaches no view: a line of sight that looks into the sun has measure zero, as on the forward route.
 *   Cone       Src_qmax <= 0: d' = d.  Otherwise d' is drawn per event, uniformly in solid angle inside the cone of half angle Src_qmax / 2
 *              about d, the forward launch's distribution: mu = 1 - u0 (1 - cos(Src_qmax / 2)), azimuth u1, from Philox block
 *              2^31 + j of (seed, id), j = 0, 1, ... counting the history's events: blocks the walk never reaches.  Forward photons
 *              cross the top with equal weight per horizontal area, hence mu0 / |d'_z|; it cancels against the cosine at the surface.
 *   Ray        above the 3-D region the ray ends in closed form, exp(-(tau so far + rest of the layer + tau above) / |d'_z|), from the
 *              layer table's vertical optical depths: no steps.  Inside and below it the ray takes cell steps with the walk's own
 *              reads and DDA, one per trip of the history loop, and ends early -- its term dropped -- once g exp(-tau) falls below
 *              1e-7, g = c / F the coefficient in front of T without the irradiance: the weight the history has on the ray, under
 *              the bound at which the walk itself ends a history (a bias of at most 1e-7 F per event).  The rule does not look at
 *              F, so rad is exactly affine in F on the same ids.  With F = 0 no ray is flown and the raw tally is that of the
 *              Src_mtype = 3 job bit for bit, under any Src_qmax.  An exactly vertical sun keeps its column.  A ray that has taken 2^20 steps is dropped and counted as
 *              CAPPED.  Counting builds add the rays' steps to MI3D_CNT_STEPS and MI3D_CNT_STEPS3D.
 *   Result     that of mi3d_set_view_method 1: every pixel divided by its own count of histories, absolute W m-2 sr-1 um-1, the score
 *              carries Src_flx; the brightness temperature of such an image includes the sun, as the forward mixed job's does. */
int mi3d_set_view_sunlight(mi3d_solver *h, int on);

/* The backward route's satellite views under independent columns and partial 3-D: the IPA twin of a backward 3-D image, with the same
 * error bars and weighting functions (er3t_amd/csrc/mi3d_kernel_backward.hip; the project's namelist key Rad_mvcol = 1).
 *   Switch     mi3d_set_view_columns: 0 (default) nothing of this runs -- kernels, names, refusals and results are those of the library
 *              without it; 1: mi3d_run serves solver MI3D_SOLVER_IPA and MI3D_SOLVER_P3D under mi3d_set_view_method 1 with the views of
 *              mi3d_set_views.  Anything but 0 or 1 is MI3D_EINVAL.  mi3d_last_kernel: "k_backward<C,V,I> [thermal]", with
 *              mi3d_set_pixel_errors 1 "k_backward<C,V,I,S> [thermal]", with mi3d_set_view_profiles 1 "k_backward<C,V,I,P> [thermal]",
 *              with mi3d_set_view_sunlight 1 "k_backward<C,V,I,N> [solar+thermal]" and "k_backward<C,V,I,N,S> [solar+thermal]".
 *              mi3d_debug_backward_views runs the same code for single histories.
 *   Refused    with the switch on, MI3D_EUNSUP from mi3d_run in words that name it: the 3-D solver (the switch belongs to independent
 *              columns and partial 3-D), mi3d_set_view_method 0 or mi3d_set_camera_method 1, cameras and point radiometers
 *              (Rad_mrkind = 1), mi3d_set_emission_weights 1.  Everything else is refused as mi3d_set_view_method 1 refuses it.
 *              Served: the plain route, mi3d_set_pixel_errors 1, mi3d_set_view_profiles 1, mi3d_set_view_sunlight 1 with or without
 *              pixel errors.
 *   Start      Philox block 0 of (seed, id) is read as under the 3-D solver: u0, u1 place (xr, yr) inside pixel id mod npix,
 *              xr = (ir + u0) Lx / nxr, yr = (jr + u1) Ly / nyr.  The history belongs to the column that contains (xr, yr):
 *              ix = floor(xr / dx), iy = floor(yr / dy), clipped to the grid; the face rule of the 3-D start, by which the direction
 *              chooses between two cells, does not apply.  There is no parallax shift to the sensor plane: the history starts at
 *              (xr, yr, zs), or enters at the top of the atmosphere above (xr, yr), and flies along -v.  (The forward route under
 *              independent columns registers an event in its own column without that shift too.)
 *   Walk       the history never changes ix, iy.  Every layer is crossed level to level, whether or not it lies in the 3-D region.
 *              {ka, B}, ks and the phase function come from the column's own voxel in the layers of the 3-D region and from the layer's
 *              record elsewhere.  The horizontal position inside the column folds cyclically with period (dx, dy) and leaves the column
 *              where it is, so a 2-D surface grid is read at (ix dx + px, iy dy + py) as the forward route under independent columns
 *              reads it.  Scattering, reflection, the weight roulette, the end below a weight of 1e-7, the cap of 2^20 cell steps and
 *              the order of the Philox blocks are those of mi3d_set_view_method 1.
 *   Partial 3-D   a thermal job has no direct beam, so MI3D_SOLVER_P3D is MI3D_SOLVER_IPA: the same build, the same ids, the same tallies
 *              bit for bit.
 *   Sunlight   with mi3d_set_view_sunlight 1 (Src_mtype = 2) the walk is as above and the sun ray of an event differs by solver.
 *              Independent columns: the ray stays in the event's column, steps level to level and ends in closed form above the 3-D
 *              region.  Partial 3-D: the ray is the direct beam; it is flown through the cyclic 3-D grid exactly as under the 3-D
 *              solver, from the event's folded position in its column, and the history then resumes in its column.  One build serves
 *              both.
 *   Expectation   the image equals the forward job's of the same solver wherever a pixel covers whole columns, or the surface grid is no
 *              finer than the columns.  Otherwise the registration inside a column differs under slant views: a backward history starts
 *              at its pixel's point of the column and drifts from there, a forward photon's event lands in the pixel under the event.
 *              Both are independent-column answers; they differ by how a column's radiance is spread over the pixels that cut it.
 *   Result     that of mi3d_set_view_method 1: every pixel divided by its own count of histories, absolute W m-2 sr-1 um-1. */
int mi3d_set_view_columns(mi3d_solver *h, int on);

/* Job options = 1st/2nd CLI arguments and keys Wld_mtarget, Flx_mflx, Pho_wmin
 * (er3t/rtm/mca/mcarats.py:267-287,450-454; er3t/rtm/mca/mca_inp.py:196-198).
 *   target   MI3D_TARGET_FLUX | MI3D_TARGET_RADIANCE (bit-or of both is allowed); MI3D_TARGET_FLUX | MI3D_TARGET_HEAT is the
 *            reference's target='heating rate' (Flx_mflx = 3, Flx_mhrt = 1): the weight every collision takes from a photon --
 *            gas absorption and the absorbing part of every constituent -- is tallied in the cell of the collision
 *   solver   MI3D_SOLVER_3D | MI3D_SOLVER_P3D | MI3D_SOLVER_IPA
 *   wmin     Russian-roulette weight threshold (Pho_wmin, default 0.2)
 *   wfac     weight survivors of the roulette continue with (Pho_wfac, default 1); survival probability w/wfac
 *   column_le  1: answer exactly vertical views from a per-column optical-depth table (exact,
 *              one read per event); 0: always march the local-estimate ray cell by cell. */
int mi3d_set_options(mi3d_solver *h, int target, int solver, double wmin, double wfac, int column_le);

/* Russian roulette on marched local-estimate rays (a variance-reduction option of this solver, unbiased; no namelist key:
 * MCARaTS' own `Rad_difr*` / truncation options are different devices).  tau1 > 0: a ray survives to optical depth
 * tau > tau1 with probability exp(-(tau - tau1)) and then contributes exp(-tau1) instead of exp(-tau), so that rays from
 * deep inside a cloud stop after about tau1 + 1 optical depths instead of being marched to the cut-off at 16.  Exactly
 * vertical views of a sensor above the atmosphere (answered from the column table) are never affected.  tau1 = 0
 * (default): off. */
int mi3d_set_le_roulette(mi3d_solver *h, double tau1);
/* Russian roulette on the WEIGHT of marched local-estimate rays of satellite views (Rad_mrkind = 2; unbiased; no namelist key).  A
 * local estimate carries c = w P(angle towards the sensor) / 4 pi (a reflection: w R cos / pi); with a forward-peaked phase function
 * (Henyey-Greenstein g = 0.85: P between 0.05 and 80) most of them carry a few per cent of what the few near the peak carry, and
 * the noise of a pixel is made by the latter.  cmin > 0: a ray with c < cmin is marched with probability c / cmin and then carries
 * cmin.  The mean is untouched; fewer than half the rays are marched.  Views answered from the column table (mi3d_set_options
 * column_le) are never affected: their estimates cost nothing.  cmin = 0 (default): off. */
int mi3d_set_le_weight_roulette(mi3d_solver *h, double cmin);

/* Select the instrumented build of the transport kernel, which fills every MI3D_CNT_* counter
 * (the default build only counts MI3D_CNT_PHOTONS and is the one to time).  The counters are a
 * deterministic function of (scene, seed, photon ids), so measuring them on a sub-sample of the
 * job's photon ids gives the job's per-photon averages. */
int mi3d_set_counting(mi3d_solver *h, int on);

/* Bind caller-owned DEVICE buffers for the raw tallies (so that a host framework can all-reduce
 * them in place with RCCL) and the HIP stream to launch on.  Any pointer may be NULL: the library
 * then keeps its own buffer / uses the null stream.  Sizes (FLOAT64 elements: a float32 accumulator
 * stops growing once it exceeds 2^24 contributions' worth, which one pixel of a small grid reaches within
 * a few million photons):
 *   rad_sum  [nview][nyr][nxr]
 *   flux_sum [3][nz+1][ny][nx]      RAW planes: direct-down, DIFFUSE-down, up (one atomic per level
 *                                    crossing); mi3d_get_flux / mi3d_stats_add form total-down = direct +
 *                                    diffuse, so only sums of raw buffers (an all-reduce) are meaningful */
int mi3d_bind_device_buffers(mi3d_solver *h, void *rad_sum, void *flux_sum, void *stream);
/* ... and for the heating-rate tally (MI3D_TARGET_HEAT): heat_sum [nz][ny][nx] float64, weight absorbed per cell; NULL: the
 * library's own buffer. */
int mi3d_bind_heating_buffer(mi3d_solver *h, void *heat_sum);

/* The estimator of the heating-rate tally (MI3D_TARGET_HEAT; a key of this project, Flx_mhest).  Same tally, same normalisation
 * (mi3d_get_heating), same output variable and units under both:
 *   0 (default)  collision: a collision leaves w (bt - sum ks) / bt in its cell.
 *   1            path length: every flight segment inside ONE cell -- it ends at a cell face, a level, the collision site, the surface
 *                or the top -- leaves w kappa_a l there, w the weight the photon flies with, kappa_a = max(bt - sum ks, 0) from the
 *                float32 records and the sum of scattering coefficients a collision in that cell uses: both estimators mean the same
 *                absorber and have the same expectation segment by segment.  The collision itself leaves nothing; cells with
 *                kappa_a = 0 get nothing.  The cell is the one the walk is in (independent columns, partial 3-D: the photon's
 *                column).  Layers the walk crosses without x / y faces (the 1-D layers outside the 3-D region, horizontally
 *                uniform layers inside it) are cut at the LEVELS only: a layer's piece goes to the column of the piece's midpoint,
 *                folded cyclically -- layer means stay unbiased; within such a layer the columns are smoothed over the piece's
 *                horizontal extent, where the optical properties do not vary.
 * The estimator draws no random number: (seed, photon id) -> history is what it is, and the flux planes of a job do not depend on the
 * choice beyond the order of their float64 sums.  The weight roulette is unchanged.  Thermal jobs take either estimator for the
 * absorbed part of their net heating rate.  Anything but 0 / 1: MI3D_EINVAL.  A change marks the tallies dirty (the handle's own buffers are cleared by the next
 * mi3d_prepare: sums of two estimators do not mix). */
int mi3d_set_heating_estimator(mi3d_solver *h, int estimator);

/* Build the device-side scene (layout transform, total extinction, column optical depth,
 * phase-function CDFs).  Called implicitly by mi3d_run when inputs changed; exposed so that
 * set-up can be excluded from the timed region. */
int mi3d_prepare(mi3d_solver *h);

/* Zero tallies and counters. */
int mi3d_reset(mi3d_solver *h);

/* Transport `nphoton` photon histories with global ids [photon_offset, photon_offset+nphoton)
 * of the random stream keyed by `seed` (Wld_jseed), accumulating into the tallies.  Asynchronous.
 * COMPLETION RULE (one, since round 6): when mi3d_run returns, everything it has started is queued on the handle's main stream -- the stream
 * bound with mi3d_bind_device_buffers, else the handle's own -- or joined to it.  Work the caller queues on that stream afterwards (a copy out
 * of a bound buffer, an all-reduce) and every mi3d call finds the tallies complete in stream order; hipStreamSynchronize of that stream, or
 * mi3d_sync, makes the host wait.  (tests/test_lib_abi.py holds it with a raw copy out of a bound buffer.)  The only exception is asked for
 * by name: mi3d_set_tuning "overlap_sort" 2, flux jobs on the handle's own buffers and stream -- the last record sort of a run may then still
 * be on its way on a stream of the handle's own; every mi3d call that reads, clears or re-homes tallies joins it first.
 * Replaces the reference solver's main loop ("<exe> <Nphoton> <solver> <inp> <out>", mca_run.py:113). */
int mi3d_run(mi3d_solver *h, uint64_t nphoton, uint64_t seed, uint64_t photon_offset);

/* Wait for outstanding launches.  A job whose marched views go through event lists (mi3d_last_kernel: "... + k_rays") does not
 * make mi3d_run wait for its last launches: whether one of their lists ran full -- the run's tallies are then incomplete,
 * MI3D_ESTATE -- is reported by the call that looks at the tallies next: mi3d_sync, mi3d_get_radiance, mi3d_get_counters,
 * mi3d_stats_add (it reads the job's tallies into the run field), mi3d_stats_end_run, mi3d_stats_get, or the next mi3d_run.  A caller that reads bound device buffers
 * itself calls mi3d_sync first and checks its return value.  mi3d_reset forgets the runs before it. */
int mi3d_sync(mi3d_solver *h);
/* Name of the transport kernel build that served the last mi3d_run of this handle ("k_transport_lean<COUNT,P3D,0,MIX>": the lean
 * build for radiance answered from the column table, "k_transport_lean<COUNT,P3D,2,MIX> + k_rays": marched views through event
 * records, "k_transport_flux<COUNT,P3D,MIX> + k_tl_scatter + k_tl_sum": flux jobs -- MIX 0: one 1-D and one 3-D constituent with
 * analytic phase functions (er3t's default scene), 1: a second 3-D constituent, 2: the general mixture (several 1-D constituents,
 * tabulated phase functions staged in LDS) --, "k_transport<COUNT,MARCH,FLUX,P3D>": the general kernel (flux together with radiance,
 * more than two 3-D constituents, tables too large for the LDS, kernel choice 1); "k_backward<COUNT> [thermal]": the backward route of
 * mi3d_set_camera_method 1 ("k_backward<COUNT,V> [thermal]": of mi3d_set_view_method 1; "k_backward<COUNT,V,P> [thermal]": with mi3d_set_view_profiles 1; "k_backward<COUNT,S> [thermal]" and "k_backward<COUNT,V,S> [thermal]": either with mi3d_set_pixel_errors 1), whatever mi3d_set_kernel says -- "batch_log2" is the one tuning knob it reads (ids per launch; a launch is
 * min(ids / 256, what is resident at once: 5 per CU, 4 in the counting build) workgroups of 256 lanes, every lane walks its ids with a fixed stride); "" before the first launch).  For logs and
 * measurements (bench.py, profiles/): results do not depend on it. */
const char *mi3d_last_kernel(mi3d_solver *h);
/* Which build of the transport kernel may serve a launch: 0 (default) the lean ones wherever they apply -- marched satellite
 * views through the ray kernel (k_transport_lean<.,.,2> + k_rays) --, 1 always the general one (k_transport).  Both implement the
 * same function photon id -> history and the same estimator; the choice is for A/B measurements and for the parity tests, which
 * hold every build against the oracle on the same scene.  The environment variable MI3D_KERNEL=generic sets the
 * default of new handles.  (The ray kernel keeps one event list per XCD in device memory, sized from a pilot launch and never
 * beyond a quarter of the memory free at the time -- launches are sized to the lists, so small lists cost launches, not results; when
 * not even 65 536 records per list are to be had the library warns and the general kernel serves the job.  Choice 2 of rounds 2-4, the
 * lean loop with the rays of marched views walked inside it, was retired in round 5: MI3D_EINVAL.) */
int mi3d_set_kernel(mi3d_solver *h, int choice);
/* Tuning knobs of the launch machinery, for measurements and for tests that must reach its corners at small sizes.  None changes a
 * result beyond the order of float64 sums; a caller of the drop-in path needs none of them.  Unknown key or value out of range: MI3D_EINVAL.
 * An environment variable of the same name in capitals with the prefix MI3D_ (MI3D_TILE_COLS ...) sets the default of new handles where
 * the last column says so.
 *
 *   key            default  range      what                                                                          set by (log)                        env
 *   -------------  -------  ---------  ----------------------------------------------------------------------------  ----------------------------------  ---
 *   tile_cols      -1       -1..4096   tile edge of the photon order in columns; 0: id order, -1: chosen from scene   profiles/r02/tile_sweep_les480.log  yes
 *   batch_log2     30       8..30      most photons per launch                                                       profiles/r05/ab_batch_2p30.log      yes
 *   evcap_log2     28       10..28     records per event list (marched views); never > 1/4 of the free memory         profiles/r05/ab_evcap.log           yes
 *   tlcap_log2     31       16..31     records per tally-record list (flux jobs); small values: tests of full lists   tests/test_gpu_parity.py            no
 *   rad_spread     -1       -1, 0, 1   accumulation image with one pixel per 128-byte line; -1: where the photon     profiles/r04/ab_rad_line_density    yes
 *                                      loop itself tallies by atomics
 *   rad_row_pad    -1       -1..4096   padding of that image's rows in pixels; -1: rows an odd number of 4 KiB pages   profiles/r04/stride_probe4-6.log    yes
 *   tally_window   1        0, 1       column-view tallies summed per workgroup in LDS around its photons' tile       profiles/r04/ab_no_tally_ablation   yes
 *   tally_lists    1        0, 1       flux tallies as sorted records (0: an atomic per level crossing)               profiles/r03/flux_tally_routes.log  yes
 *   tally_runs     1        0, 1       ... a flight through uniform layers as ONE run record, expanded by k_tl_runs   profiles/r06/ab_flux_run_records    yes
 *   entry_records  1        0..2       new photons from a pre-pass kernel (never > 1/2 of free memory): 0 none; 1 the   profiles/r04/ab_block_c_entry_*     yes
 *                                      32-byte form where source and build allow, else 48 bytes; 2 always 48   profiles/r11/README.md
 *   cam_images     -1       -1..8      cameras: periodic images of the camera served within this many domain lengths  profiles/r04/camera_images.log      no
 *                                      (-1: 2 where the ray kernel serves the job, else the nearest with a warning)
 *   vpad_col/_row  0        0..4096    unused 16-byte records after every column / row of the voxel records           profiles/r04/stride_probe*.log      yes
 *   overlap_rays   0        0, 1       two sets of event lists, ray kernels beside the next photon loop (-2.4 %: off)  profiles/r05/ab_overlap_rays.log    yes
 *   overlap_sort   1        0, 1, 2    flux jobs: two sets of record lists, the sort of launch i on a stream of its   profiles/r06/ab_flux_schedule.log   yes
 *                                      own beside the photon loop of launch i + 1; 0: one stream; 2: also across runs
 *                                      (see mi3d_run: the one case in which a run returns before its last sort joins)
 *   overlap_pre    1        0, 1, 2    photon order / entry records of launch i + 1 beside the photon loop of          profiles/r05/ab_overlap_pre.log     yes
 *                                      launch i (flux loop, event-writing loop); 2: also for small runs read one by one
 *   tl_split       4        1..64      with overlap_sort a run is worked off in at least this many launches            profiles/r05/ab_flux_sort_overlap   yes
 *   rays_wg        0        0..8       workgroups per CU of the ray kernel's light build (0: its own figure, 6)        profiles/r05/ab_knobs_after_nt.log  yes
 *   emit_wg        0        0..8       ... of the event-writing photon loop (0: 5)                                     profiles/r05/ab_knobs_after_nt.log  yes
 *   own_stream     0        0, 1       a non-blocking stream of the handle's own instead of the NULL stream            tools/time_dropin.py                no
 *   wgt_stage      1        0, 1       emission weights: layer and surface part summed per workgroup in LDS where it     tests/test_gpu_emission_weights.py  no
 *                                      fits 32 KB (0: global atomics always)
 *   bwd_chunk      -1       -1..65536  mi3d_set_view_method 1: consecutive histories of a pixel in an item of the tile       profiles/r17/thermal_rate_sat.log   no
 *                                      hand-out (0: the camera route's stride, an atomic per history; -1: per launch, at most 4)
 */
int mi3d_set_tuning(mi3d_solver *h, const char *key, int value);

/* Milliseconds spent in transport kernels since the last reset (HIP events on the launch
 * stream) and the number of launches.  Runs whose kernels use two streams (overlap_rays, overlap_sort) are timed as a whole, from their
 * first kernel to their last; under overlap_sort consecutive runs overlap (the next run's photon loop beside this run's last sort), so
 * the sum over runs can exceed the wall time. */
int mi3d_get_timing(mi3d_solver *h, double *kernel_ms, uint64_t *launches);

/* Normalised results.  `nphoton_total` is the number of histories the tallies hold (for a
 * photon-sharded job: the sum over all shards, after the all-reduce).
 *   radiance out[nview][nyr][nxr]   per unit Src_flx, i.e. the content of the reference's
 *                                    radiance out.bin (mca_out.py:467-481 then scales it)
 *   flux     out[3][nz+1][ny][nx]   direct-down, total-down, up */
int mi3d_get_radiance(mi3d_solver *h, uint64_t nphoton_total, float *out);
int mi3d_get_flux(mi3d_solver *h, uint64_t nphoton_total, float *out);
/* The part of the direct-down and total-down flux the kernels do not tally because it is known (the direct beam above the 3-D
 * region and in the horizontally uniform layers at its top: DESIGN.md §3): out[nz+1], per level, in the units of mi3d_get_flux
 * (Src_flx mu0 exp(-tau/mu0); 0 at the levels where every crossing is tallied), for the job that ran last on this handle.
 * mi3d_get_flux adds it by itself; a caller that normalises all-reduced RAW tallies of several jobs at once (one exchange per
 * batch of jobs instead of one per job) takes it from here, job by job. */
int mi3d_get_direct_levels(mi3d_solver *h, double *out);
/* The direct sun in the cameras (mi3d_set_cameras, solar source; a thermal job has no sun: zeros): out[nview][nyr][nxr] in the units of mi3d_get_radiance, known
 * rather than tallied and so free of noise, for the scene and source set now (worked out once per job by mi3d_prepare, k_cam_direct).
 * The optical depth tau from the camera to the top of the atmosphere is integrated in float64 along the sun's CENTRAL direction
 * through the voxels (cyclic in x and y) and the 1-D layers; Src_qmax is ignored for this term.  Where that direction lies in a
 * camera's cone of view and image, its pixel holds Src_flx exp(-tau) w(theta_sun) / W (mi3d_set_camera_map), every other pixel 0
 * (also where tau > 100: the march stops there).  mi3d_get_radiance never includes it.  mi3d_stats_add adds it to the radiance run
 * field (times the analytic share) for cameras with the RECTANGULAR map only -- point radiometers, whose reader separates it again;
 * the run field of a polar camera stays diffuse only, like its mi3d_get_radiance.  A caller that normalises all-reduced RAW tallies
 * takes it from here, job by job, as mi3d_get_direct_levels.  One thread marches each camera: a sun so close to the horizon that the
 * march could cross more than 2^20 voxels is not marched, and this call (and mi3d_stats_add of a rectangular-map job) fails with
 * MI3D_EUNSUP; other jobs are not affected. */
int mi3d_get_camera_direct(mi3d_solver *h, double *out);
/*   heating  out[nz][ny][nx]        absorbed radiant power per unit volume of every cell, per unit Src_flx [1/m x the unit of
 *                                    Src_flx]: (weight absorbed in the cell) x Src_flx mu0 nx ny / N / layer thickness.  The
 *                                    fourth variable ("hrt", nz layers) of the flux out.bin of a job with Flx_mhrt = 1; divided by
 *                                    (air density x c_p) it is the heating rate in K/s.  (The reference's reader has no branch for
 *                                    it, er3t/rtm/mca/mca_out.py:202-205; MCARaTS' own unit for the variable is not in the tree.)
 *   THERMAL or SOLAR+THERMAL job (mi3d_set_thermal 3 or 2; Flx_mhrt = 2; for 2 read P_tot + P_sol where P_tot scales the tally): the NET absorbed power per unit volume, absorbed - emitted, same array, same "hrt"
 *   variable, W m-3 um-1 per unit Src_flx; negative values are cooling.
 *     absorbed  the same float64 tally under either estimator, normalised with the thermal photon power Src_flx P_tot / N:
 *               (weight absorbed in the cell) x Src_flx P_tot / (N dx dy dz).
 *     emitted   known, not tallied (as the analytic direct beam of mi3d_get_flux): Src_flx 4 pi ka B(T), with exactly the ka and
 *               T the source's CDF was built from (ka = total extinction - total scattering of the float32 records, T = mean of the
 *               two interface temperatures + Atm_tmpa3d); in a 1-D layer outside the 3-D region every column gets the layer's value.
 *               Subtracted here, in float64 on the device, rounded to float32 once.  The raw tally (mi3d_bind_heating_buffer) stays
 *               a pure sum over photons: photon-id ranges add and ranks all-reduce as for a solar job, and the emission comes off once.
 *   The surface is not part of the heating grid: its net gain is fdn - fup at level 0 of the same job's mi3d_get_flux. */
int mi3d_get_heating(mi3d_solver *h, uint64_t nphoton_total, float *out);
/* The emitted power per unit volume of a thermal or solar+thermal job, out[nz][ny][nx], in the units of mi3d_get_heating: Src_flx 4 pi ka B(T), the term
 * mi3d_get_heating subtracts, so that absorbed = net + emitted.  Builds the source first if needed (mi3d_prepare); needs no run and
 * no MI3D_TARGET_HEAT.  MI3D_ESTATE for a solar job, where nothing emits. */
int mi3d_get_emission(mi3d_solver *h, float *out);
int mi3d_get_counters(mi3d_solver *h, uint64_t out[MI3D_NCOUNTER]);

/* ---- Run statistics on the device -------------------------------------------------------------
 * What the reference's reader does on the host with one file per (run, g) job
 * (er3t/rtm/mca/mca_out.py:313-352 flux, 438-500 radiance): every job's result is scaled by a
 * per-g factor (per level: the slit function varies with altitude) and summed over g; mean and
 * population standard deviation are then taken over the runs.  Here the normalised tallies of the
 * job that just ran are folded into a per-run field, and closed runs into float64 sums of x and
 * x*x per pixel, so that no per-job result has to leave the device.
 *
 *   mi3d_stats_begin    allocate and zero.  `rad_run` / `flux_run` are optional caller-owned
 *                       DEVICE buffers (float32, shapes of mi3d_get_radiance / mi3d_get_flux) for
 *                       the per-run fields: a photon-sharded job all-reduces them once per run
 *                       before mi3d_stats_end_run instead of once per job.
 *   mi3d_stats_add      run field += factor[level] * normalised tally of the current job (then
 *                       call mi3d_reset before the next job).  factor_rad[nview],
 *                       factor_flux[nz+1]; NULL = 1.  `nphoton_total` as in mi3d_get_radiance.
 *   mi3d_stats_end_run  close the run; optionally copy its field to the host (mode='all').
 *   mi3d_stats_get      mean and standard deviation over the closed runs; `which` is
 *                       MI3D_TARGET_RADIANCE or MI3D_TARGET_FLUX; any output may be NULL. */
int mi3d_stats_begin(mi3d_solver *h, void *rad_run, void *flux_run);
/* Two handles on one device sharing the jobs of a run (each transports every other job: the tail of one job's launch runs
 * beside the next job's).  mi3d_stats_join(h, owner): h adds its jobs (mi3d_stats_add) into the run fields of `owner`, which has
 * called mi3d_stats_begin; the run is closed and read on the owner.  mi3d_stats_chain(h, after): h's next statistics kernel
 * (mi3d_stats_add, mi3d_stats_end_run) waits for the last one of `after`; called before each of them, the run field is summed
 * in job order, as one handle sums it (er3t/rtm/mca/mca_out.py:313-352: the reader's g loop). */
int mi3d_stats_join(mi3d_solver *h, mi3d_solver *owner);
int mi3d_stats_chain(mi3d_solver *h, mi3d_solver *after);
/* Photon-sharded jobs (one process per GPU, each transporting a share of a job's photon ids and the run fields summed by
 * one all-reduce per run): the direct beam above the 3-D region is not tallied but known and joins the run
 * field in mi3d_stats_add -- on ONE rank only, or the sum over ranks would hold it world-size times.  share = 1 (default):
 * this handle adds the analytic term; share = 0: it does not (ranks > 0). */
int mi3d_stats_set_analytic_share(mi3d_solver *h, double share);
int mi3d_stats_add(mi3d_solver *h, uint64_t nphoton_total, const float *factor_rad, const float *factor_flux);
int mi3d_stats_end_run(mi3d_solver *h, float *rad_run_out, float *flux_run_out);
int mi3d_stats_get(mi3d_solver *h, int which, float *mean, float *sdev, int *nrun);

/* Test hook: fill out[4*n] with Philox4x32-10 words for counters (id0+i, draw) under `seed`,
 * computed on the device.  Lets the tests prove the device and oracle streams are bit-identical. */
int mi3d_debug_philox(mi3d_solver *h, uint64_t seed, uint64_t id0, uint32_t draw, int n,
                      uint32_t *out);
/* Test hook: the photon order of the LAST launch of the last mi3d_run (indices into the launch's id range sorted by start tile,
 * k_bin_*: a permutation of 0 .. n-1 for a launch of n photons) and, optionally, where each tile's piece of it ends (the cursors
 * k_bin_scatter leaves behind, which the lean loop's tally window reads; up to ntile_max words, 1024 at most).  MI3D_ESTATE when the
 * launch ran in id order (a small domain, fewer than 4096 photons, "tile_cols" 0).  The order is the same whenever the same launch
 * is sorted again (same photons, seed, offset and tiles): the sort takes no atomic on global memory. */
int mi3d_debug_order(mi3d_solver *h, uint64_t n, uint32_t *order_out, uint32_t *tile_end_out, int ntile_max);
/* Test hook: the entry records of the LAST launch of the last mi3d_run (k_entry -> the photon loop).  Returns their
 * form -- 3: the long records, 48 bytes a photon; 2: the short ones, 32 bytes, written where the source has no cone and shines from
 * above, the job is solar and the loop's build reads them ("entry_records" 1) -- or a negative error code: MI3D_ESTATE when the
 * launch had no entry records.  n > 0: also copies the first n records to records_out as they lie in memory, in blocks of 64
 * photons, part by part: float32 [ceil(n / 64)][form][64][4]; photon i of the launch's order is [i / 64][.][i % 64][.].
 *   long:  part 0 px, py, pz, rem;  part 1 ux, uy, uz, r1;  part 2 r2, r3, ix | iy << 16, k | mode << 16 | ran << 31
 *   short: part 0 px, py, rem, r1;  part 1 r2, r3, ix | iy << 16, k | mode << 16 | ran << 31
 * n larger than the launch: MI3D_EINVAL. */
int mi3d_debug_entry(mi3d_solver *h, uint64_t n, float *records_out);
/* Test hook: the thermal source as mi3d_prepare built it.  *ptot (if not NULL) = P_tot; cdf_out (if not NULL) [n] = the device's
 * inclusive CDF of the cells' emitted power in float64, n = its number of cells (voxels, 1-D layers, surface cells: otherwise
 * MI3D_EINVAL).  MI3D_ESTATE when the job is not thermal or its source is not built yet. */
int mi3d_debug_thermal(mi3d_solver *h, double *ptot, double *cdf_out, uint64_t n);
/* Test hook of the backward route (mi3d_set_camera_method 1; MI3D_ESTATE otherwise): single histories.  For ids id0 .. id0 + n - 1 under
 * `seed`: dir_out [n][3] the world-space direction of the line of sight AWAY from the sensor (also where the score is 0: outside the
 * cone), score_out [n] what the history adds to the raw tally of pixel id mod npix (Src_flx x the sum, not divided by anything).  Nothing
 * is tallied.  capped_out (if not NULL): the histories of this handle's runs since the last mi3d_reset that ended at 2^20 cell steps;
 * n = 0 asks for it alone. */
int mi3d_debug_backward(mi3d_solver *h, uint64_t seed, uint64_t id0, int n, float *dir_out, double *score_out, uint64_t *capped_out);
/* Test hook of the backward route for satellite views (mi3d_set_view_method 1 with mi3d_set_camera_method 0; MI3D_ESTATE otherwise): the
 * same for ids id0 .. id0 + n - 1, through the hand-out "bwd_chunk" selects.  start_out [n][3] where history id starts (folded into the
 * domain, z = the sensor plane), dir_out [n][3] its direction -v, score_out [n] what it adds to the raw tally of pixel id mod npix. */
int mi3d_debug_backward_views(mi3d_solver *h, uint64_t seed, uint64_t id0, int n, float *start_out, float *dir_out, double *score_out,
                              uint64_t *capped_out);
/* Test hook: the phase tables as they stand on the device after mi3d_set_phase + mi3d_prepare (each pointer may be NULL): mu [nang]
 * ascending, p and cdf [npf][nang] (float32, normalised), the bucket index of mu [MI3D_TAB_IDX_N] and those of the CDFs
 * [npf][MI3D_TAB_IDX_N] (uint16).  nang / npf must be the loaded ones (otherwise MI3D_EINVAL); MI3D_ESTATE when no table is loaded or
 * mi3d_prepare has not built it. */
#define MI3D_TAB_IDX_N 514
int mi3d_debug_phase_tables(mi3d_solver *h, int nang, int npf, float *mu, float *p, float *cdf, uint16_t *mu_idx, uint16_t *cdf_idx);
/* Test hook: the device's own phase-function routines (er3t_amd/csrc/mi3d_device.h) on n points: p_out[i] = P(apf[i], mu = x[i]) and
 * mu_out[i] = the cosine drawn from apf[i] with the uniform number x[i] (usel[i]: which of two mixed tables).  path:
 *   0  phase_eval / phase_sample, tables in global memory          1  the same through an LDS copy of tables tab_lo .. tab_lo + tab_n - 1
 *   2  lean_phase_eval / lean_phase_sample on the staged tables    3  phase_eval_analytic / phase_sample_analytic (apf < 1 only)
 * Paths 1 and 2 take the staged range from the caller (1 <= tab_n, tab_lo + tab_n <= npf; it must fit the LDS of a launch, and every
 * selector >= 1 must refer to staged tables only: otherwise MI3D_EINVAL); paths 0 and 3 ignore it.  No photon kernel is involved. */
int mi3d_debug_phase(mi3d_solver *h, int path, int tab_lo, int tab_n, int n, const float *apf, const float *x, const float *usel,
                     float *p_out, float *mu_out);
/* Test hook: the device's rotate_dir and sincos_turns (er3t_amd/csrc/mi3d_device.h) on n points.  dir [n][3] the direction before the
 * collision (as the caller gives it: not normalised here), mu [n] the cosine of the scattering angle, uphi [n] the azimuth in turns;
 * dir_out [n][3] the direction rotate_dir leaves, sincos_out [n][2] = sincos_turns(uphi[i]): sine, cosine.  Needs no scene.  n <= 0, n > 2^26 or a
 * NULL pointer: MI3D_EINVAL.  No photon kernel is involved. */
int mi3d_debug_rotate(mi3d_solver *h, int n, const float *dir, const float *mu, const float *uphi, float *dir_out, float *sincos_out);
/* Test hook: the device's surface routines (er3t_amd/csrc/mi3d_device.h) on n points; needs no scene.  path:
 *   0  out[i] = surface_R(Sfc{type, param[0..4]}, din[i], dout[i]): the reflectance factor for light travelling along din[i] (downward)
 *      that leaves along dout[i] (upward); MI3D_SFC_LSRT and MI3D_SFC_DSM take their routines, every other type code the Lambertian branch
 *   1  out[i] = fresnel_unpolarised(param[2], param[3], din[i][0])        2  out[i] = dsm_shadow_lambda(din[i][0], param[0])
 * Paths 1 and 2 read din[i][0] alone and ignore type; dout may be NULL for them.  A path outside 0 .. 2, n <= 0, n > 2^26 or a missing
 * pointer: MI3D_EINVAL.  No photon kernel is involved. */
int mi3d_debug_surface(mi3d_solver *h, int path, int n, int type, const float *param, const float *din, const float *dout, float *out);

#ifdef __cplusplus
}
#endif
#endif /* MI3D_H */
