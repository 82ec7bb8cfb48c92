// mi3d_api.hip — host side of libmi3drt.so: the C-ABI declared in include/mi3d.h.
//
// Plays the role of the reference solver's start-up and I/O phases (reading the namelist and the
// three side files, er3t/rtm/mca/mca_inp.py:636-697, mca_atm.py:373-389, mca_sca.py:82-92,
// mca_sfc.py:136-146; writing out.bin, mca_out.py:94-103) with in-memory hand-off instead of
// files.  There is NO CPU fallback: every compute entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "mi3d_kernels.hip"
#include "mi3d_kernel_lean.hip"
#include "mi3d_kernel_rays.hip"
#include "mi3d_kernel_flux.hip"
#include "mi3d_kernel_backward.hip"

using namespace mi3d;

#include <algorithm>

static constexpr size_t kTabLdsBudget = 24 * 1024; // LDS bytes a workgroup may spend on phase tables
constexpr int kEvSlots = 4;   // launches whose fill counters may be on their way to the host at once

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(MI3D_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),       \
                        __FILE__, __LINE__);                                                       \
    } while (0)

template <typename T>
int dev_realloc(T *&p, size_t &cap, size_t n) {
    if (n <= cap && p) return MI3D_OK;
    if (p) { HIPCHK(hipFree(p)); p = nullptr; cap = 0; }
    if (n == 0) return MI3D_OK;
    HIPCHK(hipMalloc((void **)&p, n * sizeof(T)));
    cap = n;
    return MI3D_OK;
}

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    int alloc(size_t n) { return dev_realloc(p, cap, n); }
    int upload(const T *src, size_t n) {
        int rc = alloc(n);
        if (rc) return rc;
        if (n) HIPCHK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        return MI3D_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};

constexpr double kWgtMaxElems = 2147483648.0;   // elements of the emission weights' tally npix x ncell served (mi3d_set_emission_weights)
constexpr double kPrfMaxElems = 2147483648.0;   // elements of the view profiles' tally npix x (nz + 1) x 2 served (mi3d_set_view_profiles)

// The six builds of the backward route (mi3d_kernel_backward.hip): k_backward, k_backward_w, k_backward_v, k_backward_vp, k_backward_s,
// k_backward_vs ... and the two with sunlight (mi3d_set_view_sunlight 1): k_backward_vn, k_backward_vns ... and the five of the satellite
// views under independent columns and partial 3-D (mi3d_set_view_columns 1): k_backward_vc, k_backward_vcs, k_backward_vcp, k_backward_vcn,
// k_backward_vcns
enum class BwdRoute { Camera = 0, Weights = 1, Views = 2, Profiles = 3, CameraErrors = 4, ViewsErrors = 5, ViewsSun = 6, ViewsSunErrors = 7,
                      Columns = 8, ColumnsErrors = 9, ColumnsProfiles = 10, ColumnsSun = 11, ColumnsSunErrors = 12 };
// the column build that stands for a build of the satellite views (col: mi3d_solver::col_backward)
static BwdRoute backward_column_route(BwdRoute r, bool col) {
    if (!col) return r;
    return r == BwdRoute::Views ? BwdRoute::Columns : r == BwdRoute::ViewsErrors ? BwdRoute::ColumnsErrors : r == BwdRoute::Profiles ? BwdRoute::ColumnsProfiles
           : r == BwdRoute::ViewsSun ? BwdRoute::ColumnsSun : r == BwdRoute::ViewsSunErrors ? BwdRoute::ColumnsSunErrors : r;
}
// ... and what the runtime said of one of them: workgroups resident per CU for `lds` bytes of dynamic LDS (0: not asked yet)
struct BwdCap { int blocks = 0, counting = -1; size_t lds = 0; };

} // namespace

struct mi3d_solver {
    int device = 0;
    int num_cu = 256;
    hipStream_t stream = nullptr;      // the stream every launch and asynchronous copy of this handle goes to: the caller's (NULL: the null stream) or own_stream
    hipStream_t own_stream = nullptr;  // mi3d_set_tuning "own_stream": non-blocking, so that two handles on one device do not serialise through the null stream
    bool use_own_stream = false;

    // ---- host copies of the small inputs
    int nz = 0, np1d = 0;
    std::vector<double> zgrd;
    std::vector<float> ext1d, omg1d, apf1d, abs1d;
    int nx = 1, ny = 1, nz3 = 0, iz3l = 1, np3d = 0;
    double dx = 1.0e4, dy = 1.0e4;
    bool has_abst = false;
    int nang = 0, npf = 0;
    std::vector<float> ang, pha;
    int sfc_mtype = MI3D_SFC_LAMBERT, nxb = 0, nyb = 0;
    bool sfc_lambert_only = true;   // no LSRT or DSM surface anywhere: the ray kernel's light build serves
    float sfc_param[5] = {0, 0, 0, 0, 0};
    std::vector<float> sfc2d_host;
    double src_flx = 1.0, src_qmax = 0.0, src_the = 180.0, src_phi = 0.0;
    // thermal source (mi3d_set_thermal): Src_mtype 3, band-centre wavelength, interface / voxel / surface temperatures; the
    // emitted power of every cell as a CDF on the device (k_thermal_power, k_scan_*), rebuilt by mi3d_prepare when dirty
    int src_mtype = 1;
    double th_wlen = 0.0, th_ptot = 0.0, th_ms = 0.0;
    // solar+thermal source (Src_mtype 2): the thermal source plus the sun's irradiance Src_fsol (mi3d_set_solar_irradiance; < 0: not set);
    // th_psol = Src_fsol mu0 Lx Ly is worked out with P_tot by build_thermal
    double src_fsol = -1.0, th_psol = 0.0;
    bool thermal() const { return src_mtype == 3 || src_mtype == 2; }   // does the job emit (either of the two sources with a CDF)?
    std::vector<float> th_tlev;
    size_t th_ntmpa = 0, th_ntmps = 0;   // elements of the anomalies handed over (0: none)
    size_t th_ncell = 0;                 // cells of the CDF build_thermal made last (mi3d_debug_thermal)
    DevBuf<float> d_th_tlev, d_th_tmpa, d_th_tmps;
    DevBuf<double> d_th_cdf, d_th_bsum;
    DevBuf<DevThermal> d_th;
    bool dirty_thermal = false;
    // backward Monte Carlo for the cameras of a thermal job (mi3d_set_camera_method 1; mi3d_kernel_backward.hip): {ka, B} of every cell
    // (k_backward_cells, rebuilt with the thermal source), the count of capped histories, the read-out's normalised tally
    int cam_method = 0;
    bool dirty_bwd = true;
    DevBuf<float2> d_bwd_cells;
    DevBuf<unsigned long long> d_bwd_capped;
    DevBuf<double> d_bwd_norm, d_bwd_score;
    DevBuf<float> d_bwd_dir;
    // ... and for the satellite views of a thermal job (mi3d_set_view_method 1): the switch, the tile hand-out's chunk
    // (mi3d_set_tuning "bwd_chunk"; -1: chosen per launch, at most kBwdChunkAuto; 0: the camera route's stride; n >= 1: exactly n), the chunk
    // of the launch made last
    int view_method = 0;
    int bwd_chunk = -1;
    int bwd_chunk_last = 0;
    DevBuf<float> d_bwd_start;
    BwdCap bwd_cap[13];              // per BwdRoute: the resident workgroups per CU of the build launched last (backward_resident)
    bool sat_backward() const { return view_method == 1 && cam_method == 0 && rad_kind == 2; }           // is the job sent to k_backward_v?
    // ... and the sunlight term of a solar+thermal job's satellite views (mi3d_set_view_sunlight 1): the switch
    int view_sunlight = 0;
    bool sun_backward() const { return view_sunlight == 1 && src_mtype == 2 && sat_backward(); }         // is the job sent to k_backward_vn?
    // ... and the satellite views under independent columns and partial 3-D (mi3d_set_view_columns 1): the switch
    int view_columns = 0;
    bool col_backward() const { return view_columns == 1 && solver != MI3D_SOLVER_3D && sat_backward(); }  // is the job sent to a column build (k_backward_vc...)?
    bool backward() const {                                                                               // does the read-out divide by the pixels' own counts?
        if (sun_backward() && nview > 0) return true;
        return src_mtype == 3 && nview > 0 && ((cam_method == 1 && rad_kind == 1) || sat_backward());
    }
    // per-cell emission weights of the backward route (mi3d_set_emission_weights 1): K_raw[npix][ncell], the library's own
    // buffer (wgt_n elements, zeroed when it is made; 0: to be made or cleared by the next run) or the caller's (mi3d_bind_weights_buffer)
    int emis_weights = 0;
    int wgt_stage = -1;              // mi3d_set_tuning "wgt_stage": -1 the layer and surface part is summed in LDS where it fits, 0 never
    int wgt_staged_last = 0;         // what the last launch of the weights build did
    DevBuf<double> d_wgt_own;
    DevBuf<float> d_wgt_out;         // the read-out's staging buffer
    double *wgt_ext = nullptr;
    size_t wgt_n = 0;
    double *wgt_ptr() { return wgt_ext ? wgt_ext : d_wgt_own.p; }
    // per-layer profiles of the backward route's satellite views (mi3d_set_view_profiles 1): P_raw[npix][nz + 1][2], pairs
    // {K, C}; the library's own buffer (prf_n elements, zeroed when it is made; 0: to be made by the next run) or the caller's
    // (mi3d_bind_view_profiles_buffer); prf_ran: a run has tallied them since the switch was set and the scene laid out
    int view_profiles = 0;
    DevBuf<double> d_prf_own;
    DevBuf<float> d_prf_out;         // the read-out's staging buffer
    double *prf_ext = nullptr;
    size_t prf_n = 0;
    bool prf_ran = false;
    double *prf_ptr() { return prf_ext ? prf_ext : d_prf_own.p; }
    // per-pixel standard errors of the backward route (mi3d_set_pixel_errors 1): rad2[npix], the sums of the squared
    // scores; the library's own buffer (err_n elements, zeroed when it is made; 0: to be made by the next run) or the caller's
    // (mi3d_bind_pixel_errors_buffer); err_ran: a run has tallied them since the last reset
    int pixel_errors = 0;
    DevBuf<double> d_err_own;
    DevBuf<float> d_err_out;         // the read-out's staging buffer
    double *err_ext = nullptr;
    size_t err_n = 0;
    bool err_ran = false;
    double *err_ptr() { return err_ext ? err_ext : d_err_own.p; }
    double prf_elems() const { return (double)nview * nxr * nyr * ((double)nz + 1.0) * 2.0; }
    size_t wgt_ncell() const { return (size_t)nx * ny * nz3 + (size_t)nz + (sfc2d_host.empty() ? (size_t)1 : (size_t)nxb * nyb); }
    int nview = 0, nxr = 1, nyr = 1;
    double view_the[MI3D_MAX_VIEW], view_phi[MI3D_MAX_VIEW], view_zloc[MI3D_MAX_VIEW], zref = 0.0;
    // cameras (mi3d_set_cameras): rad_kind 1, the views are point sensors
    int rad_kind = 2;
    double cam_psi[MI3D_MAX_VIEW], cam_xpos[MI3D_MAX_VIEW], cam_ypos[MI3D_MAX_VIEW], cam_qmax[MI3D_MAX_VIEW], cam_umax[MI3D_MAX_VIEW],
           cam_vmax[MI3D_MAX_VIEW], cam_apsize[MI3D_MAX_VIEW];
    DevBuf<CamRec> d_cams;            // [nview] CamRec, then the float table [nview][nxr] of the rectangular map (cam_pixel)
    int cam_mpmap = 1, cam_mrproj = 0;   // mi3d_set_camera_map: Rad_mpmap, Rad_mrproj
    // the direct sun in the cameras (k_cam_direct): [nview][nyr][nxr] per unit Src_flx, rebuilt by mi3d_prepare when dirty
    DevBuf<double> d_camdir, d_zgrd;
    bool dirty_camdir = true;
    bool camdir_ok = false;           // d_camdir holds the direct sun of the scene and source set now (false: the march was too long, see build_camdir)
    int target = MI3D_TARGET_FLUX, solver = MI3D_SOLVER_3D, column_le = 1, counting = 0;
    double wmin = 0.2, wfac = 1.0, le_tau1 = 0.0, le_cmin = 0.0;
    std::vector<LayerRec> lay_host;  // the layer table as uploaded (mi3d_prepare)
    std::vector<double> dir_level;   // [nz+1] analytic direct-beam flux per unit Src_flx*mu0 at the levels >= kdir, 0 below
    int kdir = 0;
    DevBuf<double> d_dir_level;

    // ---- device data
    DevBuf<float> d_abst, d_extp, d_omgp, d_apfp;        // file-layout inputs
    DevBuf<LayerRec> d_lay;
    DevBuf<ViewRec> d_views;
    DevBuf<DevCold> d_cold;
    DevBuf<float> d_bt1d, d_dz, d_bmin, d_bmax;
    DevBuf<float4> d_vrec;
    DevBuf<float> d_bext3;           // the total extinction alone, for the ray kernel's walk (DevScene::bext3)
    double z_cloud = -1.0;               // height [m] around which the 3-D layers' extinction varies most (the tally window is centred where the direct beam gets there), -1: none
    int tally_window = 1;                // mi3d_set_tuning "tally_window": 0: every radiance tally of the lean loop is an atomic on the image
    unsigned vcol_f4 = 0, vrow_f4 = 0;   // strides of the voxel records (DevScene), set by mi3d_prepare
    int vpad_col = 0, vpad_row = 0;      // padding of a column / a row in records (MI3D_VPAD_COL, MI3D_VPAD_ROW)
    DevBuf<float> d_tcol0, d_tmu, d_tp, d_tcdf, d_sfc2d;
    DevBuf<uint16_t> d_tmuidx, d_tcdfidx;   // bucket indices into the tables (DevCold::tmu_idx, tcdf_idx)
    int nmarch = 0, n_step3d = 0, col0 = 0;
    int tab3d_lo = 1 << 30, tab3d_hi = -1; // table range referenced by the 3-D constituents
    bool hg3d = true;                      // every 3-D constituent with extinction is Henyey-Greenstein (-1 < apf < 1)
    int tab_lo = 0, tab_n = 0;             // tables staged in LDS
    DevBuf<int> d_tabrange;
    DevBuf<float2> d_csca;
    DevBuf<tally_t> d_rad_own, d_flux_own;
    DevBuf<tally_t> d_rad_acc;       // accumulation image of the radiance tally: one pixel per 128-byte line (kRadLine), see mi3d_run
    int rad_row_pad = -1;            // pixels of padding per row of the accumulation image (-1: chosen from its row length; MI3D_RAD_ROW_PAD)
    int rad_spread = -1;             // -1: spread the image when it stays below 1 GB, 0: never (MI3D_RAD_SPREAD overrides)
    tally_t *rad_ext = nullptr, *flux_ext = nullptr;
    DevBuf<double> d_heat_own;       // heating rates (MI3D_TARGET_HEAT): weight absorbed per cell [nz][ny][nx]
    double *heat_ext = nullptr;
    int heat_estimator = 0;          // mi3d_set_heating_estimator: 0 collision, 1 path length
    size_t heat_elems() const { return (size_t)nz * nx * ny; }
    double *heat_ptr() { return heat_ext ? heat_ext : d_heat_own.p; }
    DevBuf<unsigned long long> d_counters, d_next;
    // photon order of a launch (k_bin_*): indices sorted by start tile, the tile of every index (shared by both pre-pass sets), histogram
    DevBuf<uint32_t> d_hist;
    DevBuf<uint16_t> d_tile;
    size_t bin_lds_set = 0;          // the dynamic LDS k_bin_scatter has been allowed on this handle's device (launch_bins; above 64 KB only)
    // What the pre-pass kernels of a launch write: photon order, tiles' ends (the cursors, which are also the tally window's tile_end) and
    // entry records (k_entry -> k_transport_lean, 48 or 32 bytes per photon: entry_form).  Set 1: the pre-pass of launch i + 1 runs on a stream of its own
    // beside the photon loop of launch i (28 registers against the loop's 80 x 6: one more wave per SIMD fits).  release(): the large
    // buffers (set 0's cursor is allocated by mi3d_create)
    struct PreSet {
        DevBuf<uint32_t> order, cursor;
        DevBuf<float4> entry;
        hipEvent_t done = nullptr, loop = nullptr; bool used = false;   // pre-pass written / photon loop through with the set
        void release() { order.release(); entry.release(); }
    };
    PreSet pre[2];
    hipStream_t pre_stream = nullptr;
    hipEvent_t pre_main = nullptr;   // the last pre-pass that ran on the MAIN stream (a one-stream launch): the pre-pass stream waits for it (shared d_hist / d_tile)
    bool pre_main_used = false;
    uint64_t pre_no = 0;             // launches so far: launch n uses set n & 1
    int pre_last = 0;                // the set of the last launch (mi3d_debug_order)
    int overlap_pre = 1;             // mi3d_set_tuning "overlap_pre" (MI3D_OVERLAP_PRE): 1 two sets, the pre-pass beside the previous photon loop; 0 one stream
    int cam_images = -1;             // mi3d_set_tuning "cam_images": periodic images of a camera an event contributes to, in domain lengths around the nearest one;
                                     // -1 (default): 2 where the ray kernel serves the job, the nearest image alone (with a warning) where it cannot
    bool cam_warned = false;         // the warning of that fall-back has been printed for this handle
    bool general_warned = false;     // ... and the one that says a job has landed on the general photon loop without having asked for it
    int entry_records = 1;           // mi3d_set_tuning "entry_records": 0: new photons are launched inside the photon loop; 1: entry records, the short
                                     // form where the launch and the build allow (entry_form); 2: entry records, always the long form
    int entry_form_run = 0;          // the form of the current run's entry records (kEntryF4, kEntryF4Short; 0: none)
    int entry_form_last = 0;         // ... of the last launch of the last mi3d_run, and that launch's photons (mi3d_debug_entry)
    uint64_t entry_n_last = 0;
    // marched views served by k_rays: event lists (one per XCD), their counters and the list of reflections off LSRT / DSM surfaces.  Set 1
    // (round 5): the ray kernel of launch i works through set i & 1 on a stream of its own while the photon loop of launch i + 1 fills the
    // other set -- the tail of either kernel (a tenth of a launch) no longer leaves the chip half empty.  release(): the lists
    struct EvSet {
        DevBuf<float4> events;
        DevBuf<unsigned long long> evctr, hvlist;
        hipEvent_t emit = nullptr, rays = nullptr; bool used = false;   // photon loop / ray kernels of the launch that used the set last
        void release() { events.release(); hvlist.release(); }
    };
    EvSet ev[2];
    DevCold cold_host2;              // the DevCold at d_cold.p + 1: cold_host with set 1's event lists OR set 1's pre-pass buffers (one spare: never both)
    hipStream_t rays_stream = nullptr;
    int overlap_rays = 0;            // mi3d_set_tuning "overlap_rays" (MI3D_OVERLAP_RAYS): 0 (default): one stream, one set; 1: measured 2.4 % SLOWER on the nine-view
                                     // workload (profiles/r05/ab_overlap_rays.log): both kernels wait on memory, side by side they wait more
    int rays_wg = 0, emit_wg = 0;    // mi3d_set_tuning "rays_wg" / "emit_wg": workgroups per CU of the ray kernel's light build / of the event-writing
                                     // photon loop (0: the builds' own figures) -- what share of a CU each takes while the two run side by side
    double ev_per_photon = 0.0;      // 0: nothing known, the next run with marched views starts with a pilot launch
    int n_xcd = 8;                   // XCDs workgroups of this device land on (k_xcc_census): that many event lists fill
    unsigned long long *h_evctr = nullptr;   // pinned: [kEvSlots][9 * kCtrStride] fill counters of the last launches, copied out in stream order
    // a launch whose fill counters are on their way to the host (ev_note): its photons, the capacity of the lists it wrote to, ev_epoch at
    // its launch; cleared: its tallies have been cleared since (mi3d_reset), a full list no longer matters
    struct EvSlot { hipEvent_t done = nullptr; uint64_t nb = 0, cap = 0; unsigned epoch = 0; bool busy = false, cleared = false; };
    EvSlot ev_slot[kEvSlots];
    unsigned ev_epoch = 0;           // what ev_per_photon is an estimate FOR changes with the scene: a launch of an earlier epoch says nothing about it (ev_forget)
    int ev_cap_log2 = 28;            // records per XCD list at most, log2 (and never more than a quarter of the free memory in all: 1.5e8 per list on an otherwise empty
                                     // MI355X): 2^26 / 2^27 / 2^28 -> 3.53 / 3.73 / 3.76e8 photons/s with nine views (launch tails; profiles/r05/ab_evcap.log)
    // Flux jobs served by k_transport_flux: tally records, sorted into bins and summed after every launch (mi3d_kernel_flux.hip).  Set 1: the
    // sort and the sums of launch i run on a stream of their own (memory-bound, a few waves per CU) while the photon loop of launch i + 1
    // (issue-bound) fills the other set.
    // The sums of a launch on two streams (k_tl_sum: 128 KB of LDS, no room on a CU the photon loop holds) are not queued behind its sort: on the
    // sort stream they crept along in the loop's tails and kept the NEXT launch's sort waiting for as long as the loop beside them ran.  They
    // are launched on the MAIN stream, between two photon loops: in front of the next launch of their set, or by whoever joins (tl_join).
    struct PendingSum { bool on = false; TallyList TL; double *flux = nullptr; unsigned nflux = 0; double *heat = nullptr; unsigned nheat = 0; int split = 1; };
    struct TlSet {
        DevBuf<uint2> rec, binned;   // the records the loop writes, their sorted copy
        DevBuf<uint32_t> words;      // chunk fills, histogram, bin starts, placement cursors
        DevBuf<unsigned long long> cursor;
        DevBuf<float4> runs;         // run records (round 6: one 32-byte record per flight through uniform layers, expanded by k_tl_runs)
        // photon loop / sums of the launch that used the set last; its sort is through the lists (its sums may still run)
        hipEvent_t filled = nullptr, sorted = nullptr, scattered = nullptr; bool used = false;
        PendingSum pend;             // that launch's sums, where they are still to come
        void release() { rec.release(); binned.release(); words.release(); runs.release(); }
    };
    TlSet tl[2];
    DevBuf<unsigned long long> d_tl_stats;   // [64][4] the counters of each launch in flight, copied there by its k_tl_prefix (tl_note reads them; slots as d_tldesc)
    hipStream_t tl_stream = nullptr;
    unsigned runs_unread = 0;        // runs since a call last looked at the tallies (sync_main): > 0 -- runs are queued back to back
    bool tl_unjoined = false;        // the main stream has not been made to wait for the last sorts yet (tl_join)
    uint64_t tl_launch_no = 0;       // launches with record lists so far: launch n uses set n & 1
    int overlap_sort = 1;            // mi3d_set_tuning "overlap_sort" (MI3D_OVERLAP_SORT): 1 two sets, the sort beside the next photon loop, where a run is long enough or
                                     // queued behind another (mi3d_run); 2: always; 0 one stream
    int tl_split = 4;                // mi3d_set_tuning "tl_split": a run with overlap_sort is worked off in at least this many launches (the last sort is not hidden)
    double tl_per_photon = 0.0;      // tally records per photon the photon loop reserved in its lists, seen so far (0: nothing known)
    double tl_total_pp = 0.0, tl_runs_pp = 0.0;   // ... records per photon in all (expanded runs included: what the sorted copy holds), run records per photon
    int tally_runs = 1;              // mi3d_set_tuning "tally_runs" (MI3D_TALLY_RUNS): 1 flights through uniform layers leave run records (k_tl_runs expands them); 0 a record per level
    int tl_cap_log2 = 31;            // most records the lists may hold, log2 (mi3d_set_tuning "tlcap_log2": tests of the full-list path)
    int tally_lists = 1;             // mi3d_set_tuning "tally_lists": 0: every flux tally is an atomic (MI3D_TALLY_LISTS overrides)
    int lds_max = 65536;             // bytes of LDS a workgroup may ask for
    unsigned long long *h_tlctr = nullptr;   // pinned: [kEvSlots] records reserved by the last launches
    DevBuf<char> d_tldesc;           // [64] TallyList: the description the photon loop of each launch in flight reads
    char *h_tldesc = nullptr;        // pinned source of those copies
    hipEvent_t tldesc_ev[64] = {};   // the photon loop that read slot i is through: the host waits for it before it fills the slot again (it may be dozens of small launches ahead)
    bool tldesc_used[64] = {};
    // a launch whose record counters are on their way to the host (tl_note): its photons, the capacities of the three lists it wrote to
    struct TlSlot { hipEvent_t done = nullptr; uint64_t nb = 0, cap = 0, bcap = 0, rcap = 0; bool busy = false; };
    TlSlot tl_slot[kEvSlots];
    int kernel_choice = 0;           // 0: the lean kernels where they apply (marched views through k_rays), 1: always k_transport
                                     // (MI3D_KERNEL=generic); A/B and tests
    int tile_cols = -1;              // tile edge in columns: -1 choose from the scene, 0 no sorting (MI3D_TILE_COLS overrides)
    uint64_t batch = (uint64_t)1 << 30; // most photons per kernel launch (order and tile buffers hold one launch: 4 GB + 2 GB; entry records 32 or 48 B per photon, where half
                                        // of the free memory holds them).  Every launch ends with a tail in which the chip runs empty: 2^27 -> 2^29 is worth 2.8 %
                                        // (profiles/r02/launch_batch_size.log), 2^29 -> 2^30 another 1.4 % (profiles/r05/ab_batch_2p30.log)
    DevCold cold_host;               // source of the asynchronous upload in fill_scene: must outlive the call

    bool dirty_grid = true, dirty_phase = true, dirty_sfc = true, dirty_tally = true, dirty_views = true;
    bool have_1d = false;

    // ---- run statistics (mi3d_stats_*): index 0 radiance, 1 flux
    DevBuf<float> d_run_own[2], d_stat_out;
    DevBuf<float> d_get_out;         // mi3d_get_flux / mi3d_get_heating: the normalised float32 field on its way to the host
    DevBuf<double> d_get_add;        // ... and its per-level term (the analytic direct beam, the layers' thickness)
    float *run_ext[2] = {nullptr, nullptr};
    DevBuf<double> d_sum[2], d_sumsq[2];
    DevBuf<float> d_factor[2];
    bool stats_on = false, stats_joined = false;   // joined: this handle adds into another handle's run fields (mi3d_stats_join)
    hipEvent_t stats_ev = nullptr;   // recorded after every statistics kernel of this handle (mi3d_stats_chain)
    int stats_nrun = 0;
    double analytic_share = 1.0;     // mi3d_stats_set_analytic_share
    float *run_ptr(int w) { return run_ext[w] ? run_ext[w] : d_run_own[w].p; }
    size_t stat_elems(int w) const { return w == 0 ? (size_t)nview * nxr * nyr : flux_elems(); }

    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double kernel_ms = 0.0;
    uint64_t launches = 0;
    std::string last_kernel;

    size_t rad_elems() const { return (size_t)(nview > 0 ? nview : 1) * nxr * nyr; }
    size_t flux_elems() const { return (size_t)3 * (nz + 1) * nx * ny; }
    tally_t *rad_ptr() { return rad_ext ? rad_ext : d_rad_own.p; }
    tally_t *flux_ptr() { return flux_ext ? flux_ext : d_flux_own.p; }
};

namespace {

int drain_events(mi3d_solver *h) {
    for (auto &pr : h->pending) {
        HIPCHK(hipEventSynchronize(pr.second));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, pr.first, pr.second));
        h->kernel_ms += ms;
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    h->pending.clear();
    return MI3D_OK;
}

// Host part of the layer table: 1-D optical properties, optical depth above, uniform-layer runs.
// `uniform3d[k3]` / `bt3d[k3]` come from k_layer_uniform (total extinction of a 3-D layer that does
// not vary horizontally).
int build_layers(mi3d_solver *h, const std::vector<int> &uniform3d, const std::vector<float> &bt3d,
                 std::vector<LayerRec> &lay) {
    const int nz = h->nz;
    const int k3lo = h->nz3 > 0 ? h->iz3l - 1 : 0;
    const int k3hi = h->nz3 > 0 ? k3lo + h->nz3 : 0;
    lay.assign(nz, LayerRec{});
    std::vector<double> bt(nz);
    h->n_step3d = 0;
    for (int k = 0; k < nz; ++k) {
        LayerRec &L = lay[k];
        double b = h->abs1d[k];
        for (int ip = 0; ip < h->np1d; ++ip) {
            const double e = h->ext1d[(size_t)ip * nz + k];
            b += e;
            L.ks1d[ip] = (float)(e * (double)h->omg1d[(size_t)ip * nz + k]);
            L.apf1d[ip] = h->apf1d[(size_t)ip * nz + k];
        }
        bt[k] = b > 0.0 ? b : 0.0;
        L.zlo = (float)h->zgrd[k];
        L.dz = (float)(h->zgrd[k + 1] - h->zgrd[k]);
        L.bt = (float)bt[k];
        L.flags = 0;
        if (k >= k3lo && k < k3hi) {
            L.flags |= kLayIn3d;
            if (uniform3d[k - k3lo]) L.bt = bt3d[k - k3lo];
            else { L.flags |= kLayStep3d; L.bt = 0.0f; h->n_step3d++; }
        }
    }
    // vertical optical depth above each 1-D layer (to TOA, or to the bottom of the 3-D region)
    double acc = 0.0;
    for (int k = nz - 1; k >= k3hi; --k) { lay[k].tabove = (float)acc; acc += bt[k] * (h->zgrd[k + 1] - h->zgrd[k]); }
    acc = 0.0;
    for (int k = k3lo - 1; k >= 0; --k) { lay[k].tabove = (float)acc; acc += bt[k] * (h->zgrd[k + 1] - h->zgrd[k]); }
    // runs of consecutive uniform layers and the vertical optical depth below each layer
    acc = 0.0;
    for (int k = 0; k < nz; ++k) {
        lay[k].tauz = (float)acc;
        if (!(lay[k].flags & kLayStep3d)) acc += (double)lay[k].bt * (double)lay[k].dz;
    }
    for (int k = 0; k < nz;) {
        if (lay[k].flags & kLayStep3d) { lay[k].run_lo = k + 1; lay[k].run_hi = k; ++k; continue; }
        int e = k;
        while (e + 1 < nz && !(lay[e + 1].flags & kLayStep3d)) ++e;
        for (int j = k; j <= e; ++j) { lay[j].run_lo = k; lay[j].run_hi = e; }
        k = e + 1;
    }
    return MI3D_OK;
}

int build_tables(mi3d_solver *h) {
    if (h->npf <= 0) return MI3D_OK;
    const int n = h->nang;
    std::vector<double> mu(n), p(n), cdf(n);
    std::vector<float> fmu(n), fp((size_t)n * h->npf), fcdf((size_t)n * h->npf);
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < n; ++j) mu[j] = std::cos((double)h->ang[n - 1 - j] * pi / 180.0);
    mu[0] = -1.0; mu[n - 1] = 1.0;
    for (int j = 1; j < n; ++j)
        if (!(mu[j] > mu[j - 1])) return fail(MI3D_EINVAL, "phase-function angles must ascend strictly from 0 to 180");
    for (int j = 0; j < n; ++j) fmu[j] = (float)mu[j];
    for (int t = 0; t < h->npf; ++t) {
        for (int j = 0; j < n; ++j) p[j] = h->pha[(size_t)t * n + (n - 1 - j)];
        double tot = 0.0;
        for (int j = 1; j < n; ++j) tot += 0.25 * (p[j] + p[j - 1]) * (mu[j] - mu[j - 1]);
        if (!(tot > 0.0)) return fail(MI3D_EINVAL, "phase function %d integrates to %g", t + 1, tot);
        cdf[0] = 0.0;
        for (int j = 0; j < n; ++j) p[j] /= tot;
        for (int j = 1; j < n; ++j) cdf[j] = cdf[j - 1] + 0.25 * (p[j] + p[j - 1]) * (mu[j] - mu[j - 1]);
        cdf[n - 1] = 1.0;
        for (int j = 0; j < n; ++j) { fp[(size_t)t * n + j] = (float)p[j]; fcdf[(size_t)t * n + j] = (float)cdf[j]; }
    }
    int rc;
    if ((rc = h->d_tmu.upload(fmu.data(), n))) return rc;
    if ((rc = h->d_tp.upload(fp.data(), fp.size()))) return rc;
    if ((rc = h->d_tcdf.upload(fcdf.data(), fcdf.size()))) return rc;
    // bucket indices for the lean kernels' look-ups (lean_tab_find): per bucket edge the largest node whose (float) value does not exceed it
    if (n > 65535) return fail(MI3D_EINVAL, "phase tables of more than 65 535 angles");
    // (entry b: the last node whose bucket -- tab_bucket_mu / tab_bucket_u of its float value, the kernels' own arithmetic -- is below b)
    auto build_idx = [n](const float *a, bool is_mu, uint16_t *out) {
        int i = -1;
        for (int b = 0; b <= kTabNB; ++b) {
            while (i + 1 < n && (is_mu ? tab_bucket_mu(a[i + 1]) : tab_bucket_u(a[i + 1])) < b) ++i;
            out[b] = (uint16_t)std::min(std::max(i, 0), n - 2);
        }
        for (int b = kTabNB + 1; b < kTabIdxN; ++b) out[b] = out[kTabNB];
    };
    std::vector<uint16_t> mi(kTabIdxN), ci((size_t)h->npf * kTabIdxN);
    build_idx(fmu.data(), true, mi.data());
    for (int t = 0; t < h->npf; ++t) build_idx(fcdf.data() + (size_t)t * n, false, ci.data() + (size_t)t * kTabIdxN);
    if ((rc = h->d_tmuidx.upload(mi.data(), mi.size()))) return rc;
    if ((rc = h->d_tcdfidx.upload(ci.data(), ci.size()))) return rc;
    return MI3D_OK;
}

int needs_tables(const mi3d_solver *h) {
    for (float a : h->apf1d)
        if (a >= 1.0f) return 1;
    return 0; // 3-D apf values are not scanned on the host; the kernel falls back to isotropic if npf == 0
}

int build_views(mi3d_solver *h) {
    std::vector<ViewRec> v(h->nview > 0 ? h->nview : 1);
    const double pi = 3.14159265358979323846;
    const double ztoa = h->zgrd[h->nz];
    h->nmarch = 0;
    h->col0 = -1;
    if (h->rad_kind == 1) {
        // cameras: axes = world axes turned by Rz(phi) Ry(the) Rz(psi) (er3t/rtm/mca/mca_inp.py:324-330)
        // the CamRec records, then the rectangular map's table [nview][nxr] (cam_pixel) in the same buffer
        const size_t ncr = h->nview > 0 ? h->nview : 1, ntab = ((size_t)ncr * h->nxr * sizeof(float) + sizeof(CamRec) - 1) / sizeof(CamRec);
        std::vector<CamRec> cams(ncr + ntab);
        std::memset(cams.data(), 0, cams.size() * sizeof(CamRec));
        float *rowf = reinterpret_cast<float *>(cams.data() + (h->nview > 0 ? h->nview : 0));
        const double Lx = h->dx * h->nx, Ly = h->dy * h->ny;
        for (int iv = 0; iv < h->nview; ++iv) {
            const double t = h->view_the[iv] * pi / 180.0, p = h->view_phi[iv] * pi / 180.0, q = h->cam_psi[iv] * pi / 180.0;
            const double ct = std::cos(t), st = std::sin(t), cp = std::cos(p), sp = std::sin(p), cq = std::cos(q), sq = std::sin(q);
            const double Z[3] = {st * cp, st * sp, ct};
            const double X[3] = {cp * ct * cq - sp * sq, sp * ct * cq + cp * sq, -st * cq};
            const double Y[3] = {Z[1] * X[2] - Z[2] * X[1], Z[2] * X[0] - Z[0] * X[2], Z[0] * X[1] - Z[1] * X[0]};
            CamRec &C = cams[iv];
            C.cx = (float)(h->cam_xpos[iv] * Lx); C.cy = (float)(h->cam_ypos[iv] * Ly); C.cz = (float)h->view_zloc[iv];
            C.r2min = (float)(h->cam_apsize[iv] * h->cam_apsize[iv]);
            C.zx = (float)Z[0]; C.zy = (float)Z[1]; C.zz = (float)Z[2];
            C.xx = (float)X[0]; C.xy = (float)X[1]; C.xz = (float)X[2];
            C.yx = (float)Y[0]; C.yy = (float)Y[1]; C.yz = (float)Y[2];
            C.cos_half = (float)std::cos(0.5 * h->cam_qmax[iv] * pi / 180.0);
            const bool rect = h->cam_mpmap == 2;
            if (rect && !(h->cam_umax[iv] <= 180.0 && h->cam_vmax[iv] <= 180.0))
                return fail(MI3D_EINVAL, "camera %d: the rectangular map (Rad_mpmap=2) needs Rad_umax <= 180 and Rad_vmax <= 180 (%g, %g)", iv + 1,
                            h->cam_umax[iv], h->cam_vmax[iv]);
            if (rect && h->cam_mrproj == 1 && !(h->cam_umax[iv] <= 90.0))
                return fail(MI3D_EINVAL, "camera %d: cosine weighting (Rad_mrproj=1) on the rectangular map needs Rad_umax <= 90 (%g)", iv + 1, h->cam_umax[iv]);
            C.inv_du = (float)(h->nxr / (h->cam_umax[iv] * pi / 180.0));
            C.inv_dv = (float)(h->nyr / ((rect ? 2.0 : 1.0) * h->cam_vmax[iv] * pi / 180.0));   // (rectangular: V spans [-vmax, vmax])
            if (rect) {
                // 1 / W: the exact weighted solid angle of a pixel of column ir, (cos t0 - cos t1) dphi or (sin^2 t1 - sin^2 t0) dphi / 2
                const double du = h->cam_umax[iv] * pi / 180.0 / h->nxr, dphi = 2.0 * h->cam_vmax[iv] * pi / 180.0 / h->nyr;
                for (int ir = 0; ir < h->nxr; ++ir) {
                    const double t0 = ir * du, t1 = (ir + 1) * du;
                    const double W = h->cam_mrproj == 1 ? 0.5 * (std::sin(t1) * std::sin(t1) - std::sin(t0) * std::sin(t0)) * dphi
                                                        : 2.0 * std::sin(0.5 * (t0 + t1)) * std::sin(0.5 * (t1 - t0)) * dphi;
                    rowf[(size_t)iv * h->nxr + ir] = W > 0.0 ? (float)(1.0 / W) : 0.0f;
                }
            }
            ViewRec &V = v[iv];
            std::memset(&V, 0, sizeof(V));
            V.vx = C.zx; V.vy = C.zy; V.vz = C.zz; V.zs = C.cz; V.zreg = C.cz;
            V.column = 0;
            V.point = kCamPoint | (rect ? kCamRect : 0) | (h->cam_mrproj == 1 ? kCamCos : 0) | (rect && h->cam_vmax[iv] >= 180.0 ? kCamWrap : 0);
            V.roulette = h->le_tau1 > 0.0 ? 1 : 0;
            h->nmarch++;
        }
        int rc = h->d_cams.upload(cams.data(), cams.size());
        if (rc) return rc;
        return h->d_views.upload(v.data(), v.size());
    }
    for (int iv = 0; iv < h->nview; ++iv) {
        const double t = h->view_the[iv] * pi / 180.0, p = h->view_phi[iv] * pi / 180.0;
        const double vx = -std::sin(t) * std::cos(p), vy = -std::sin(t) * std::sin(p), vz = -std::cos(t);
        const bool vertical = std::fabs(vx) < 1e-7 && std::fabs(vy) < 1e-7;
        ViewRec &V = v[iv];
        std::memset(&V, 0, sizeof(V));
        const bool down = vz > 0.0;   // down-looking sensor: the light travels up to it
        V.vx = vertical ? 0.0f : (float)vx; V.vy = vertical ? 0.0f : (float)vy; V.vz = vertical ? (down ? 1.0f : -1.0f) : (float)vz;
        double zs = h->view_zloc[iv] < ztoa ? h->view_zloc[iv] : ztoa;
        if (!down && zs < h->zgrd[0]) zs = h->zgrd[0];
        V.zs = (float)zs;
        V.zreg = (float)(down ? h->zref : zs);
        V.column = (h->column_le && down && vertical && h->view_zloc[iv] >= ztoa) ? 1 : 0;
        const bool free_of_charge = down && vertical && h->view_zloc[iv] >= ztoa;   // answered from the column table (or could be): no roulette
        V.roulette = ((h->le_tau1 > 0.0 && !free_of_charge) ? 1 : 0) | ((h->le_cmin > 0.0 && !free_of_charge) ? 2 : 0);
        if (!V.column) h->nmarch++;
        else if (h->col0 < 0) h->col0 = iv;
    }
    return h->d_views.upload(v.data(), v.size());
}

// er3t's default 1-D part: Rayleigh scattering as the one 1-D constituent
static bool rayleigh_1d(const mi3d_solver *h) {
    bool ray1 = h->np1d == 1;
    for (float a : h->apf1d) ray1 = ray1 && (a > -1.5f && a <= -1.0f);
    return ray1;
}

int fill_scene(mi3d_solver *h, DevScene &S) {
    std::memset(&S, 0, sizeof(S));
    DevCold &C = h->cold_host;
    std::memset(&C, 0, sizeof(C));
    const double Lx = h->dx * h->nx, Ly = h->dy * h->ny;
    S.nz = h->nz;
    S.k3lo = h->nz3 > 0 ? h->iz3l - 1 : 0;
    S.nx = h->nx; S.ny = h->ny; S.nz3 = h->nz3; S.np1d = h->np1d; S.np3d = h->np3d;
    S.kdir = h->kdir;
    S.dx = (float)h->dx; S.dy = (float)h->dy;
    C.Lx = (float)Lx; C.Ly = (float)Ly;
    C.inv_dx = (float)(1.0 / h->dx); C.inv_dy = (float)(1.0 / h->dy);
    C.inv_nx = (float)(1.0 / h->nx); C.inv_ny = (float)(1.0 / h->ny);
    S.pix_sx = (float)(h->nxr / Lx); S.pix_sy = (float)(h->nyr / Ly);
    S.bext3 = h->d_bext3.p; S.vrec = h->d_vrec.p; S.vcol_f4 = h->vcol_f4; S.vrow_f4 = h->vrow_f4; C.csca = h->d_csca.p; C.tcol0 = h->d_tcol0.p;
    const double pi = 3.14159265358979323846;
    const double th = h->src_the * pi / 180.0, ph = h->src_phi * pi / 180.0;
    C.sdx = (float)(std::sin(th) * std::cos(ph));
    C.sdy = (float)(std::sin(th) * std::sin(ph));
    C.sdz = (float)std::cos(th);
    C.cos_cone = (float)std::cos(0.5 * h->src_qmax * pi / 180.0);
    if (h->src_qmax <= 0.0) C.cos_cone = 1.0f;
    S.nview = h->nview; S.nmarch = h->nmarch; S.nxr = h->nxr; S.nyr = h->nyr; S.rad_row = h->nxr; S.col0 = h->col0 > 0 ? h->col0 : 0;
    S.target = h->target; S.solver = h->solver; S.wmin = (float)h->wmin; S.wfac = (float)h->wfac;
    // er3t's default mixture (mca_atm.py:95-102,299-303): Rayleigh as the one 1-D constituent, Henyey-Greenstein in every voxel:
    // the lean kernels then evaluate the two phase functions without looking at their selectors (bit 8 of the target word)
    if (rayleigh_1d(h)) S.target |= kTargetRayleigh1d | (h->hg3d ? kTargetPlainPhase : 0);
    if ((h->target & MI3D_TARGET_HEAT) && h->heat_estimator == 1) S.target |= kTargetHeatPath;
    S.rad = h->rad_ptr(); S.flux = h->flux_ptr(); S.rad_stride = 1;
    C.next_photon = h->d_next.p;
    C.le_tau1 = (float)h->le_tau1;
    C.le_cmin = (float)h->le_cmin;

    {   // direct beam above the 3-D region (everything, without one): horizontally uniform, known analytically
        const int nz = h->nz;
        h->kdir = h->nz3 > 0 ? (h->iz3l - 1) + h->nz3 : 0;
        // ... and so it is in the horizontally uniform layers at the top of the 3-D region (clear air above the highest cloud
        // top: 15 of the 50 layers of BASELINE config 3): nothing the beam has met so far varies from column to column
        while (h->kdir > 0 && h->kdir <= nz && (int)h->lay_host.size() == nz && (h->lay_host[h->kdir - 1].flags & kLayIn3d) &&
               !(h->lay_host[h->kdir - 1].flags & kLayStep3d))
            h->kdir--;
        // (a source cone much wider than the solar disc -- er3t hard-wires 0.533 deg, mcarats.py:378 -- spreads the path
        //  lengths of the direct beam: then every crossing is tallied like anywhere else)
        if (h->src_qmax > 1.0) h->kdir = nz + 1;
        // (thermal: there is no direct beam.  Solar+thermal: dir_level is per unit Src_flx mu0, a mixed job's amplitude is another: its
        //  solar photons tally the direct-down plane at every level, the top included)
        if (h->thermal()) h->kdir = nz + 1;
        S.kdir = h->kdir;
        h->dir_level.assign(nz + 1, 0.0);
        const double mu0 = std::fabs(std::cos(th));
        double tau = 0.0;
        for (int L = nz; L >= h->kdir; --L) {
            if (L < nz) {
                double b = h->abs1d[L];
                for (int ip = 0; ip < h->np1d; ++ip) b += h->ext1d[(size_t)ip * nz + L];
                if ((int)h->lay_host.size() == nz && (h->lay_host[L].flags & kLayIn3d)) b = h->lay_host[L].bt;   // uniform layer of the 3-D region
                tau += (b > 0.0 ? b : 0.0) * (h->zgrd[L + 1] - h->zgrd[L]);
            }
            h->dir_level[L] = mu0 > 0.0 ? std::exp(-tau / mu0) : 0.0;
        }
    }
    C.ztoa = (float)h->zgrd[h->nz]; C.zref = (float)h->zref;
    C.inv_Lx = (float)(1.0 / Lx); C.inv_Ly = (float)(1.0 / Ly);
    C.nang = h->nang; C.npf = h->npf; C.tmu = h->d_tmu.p; C.tp = h->d_tp.p; C.tcdf = h->d_tcdf.p;
    C.tmu_idx = h->d_tmuidx.p; C.tcdf_idx = h->d_tcdfidx.p;
    {   // which tables does the scene refer to?  (1-D selectors scanned here, 3-D ones by k_apf_range)
        int lo = h->tab3d_lo, hi = h->tab3d_hi;
        for (float a : h->apf1d)
            if (a >= 1.0f) {
                const float t = a - 1.0f;
                const int i0 = (int)std::floor(t);
                lo = std::min(lo, i0);
                hi = std::max(hi, t > (float)i0 ? i0 + 1 : i0);
            }
        h->tab_lo = 0; h->tab_n = 0;
        if (h->npf > 0 && hi >= 0) {
            lo = std::max(lo, 0); hi = std::min(hi, h->npf - 1);
            // what staging costs the largest consumer: mu, p, cdf AND the bucket indices of the lean kernels (many short tables: the indices
            // dominate -- ADVICE r5), on top of the largest fixed part (the ray kernels' pools, the general kernel's per-lane stash)
            const size_t bytes = std::max((size_t)(1 + 2 * (hi - lo + 1)) * h->nang * sizeof(float), lean_tab_floats(h->nang, hi - lo + 1) * sizeof(float));
            const size_t fixed = std::max((size_t)h->nz * sizeof(LayerRec) + MI3D_MAX_VIEW * sizeof(ViewRec) + sizeof(DevCold) + (size_t)9 * 256 * sizeof(float),
                                          (size_t)(h->nz + 2) * sizeof(LayerRec) + MI3D_MAX_VIEW * sizeof(ViewRec) + sizeof(DevCold) + rays_lds_extra(h->nz, true));
            const size_t room = fixed < 64 * 1024 ? 64 * 1024 - fixed : 0; // default dynamic-LDS limit of a launch
            if (hi >= lo && bytes <= kTabLdsBudget + (size_t)(1 + (hi - lo + 1)) * kTabIdxN * sizeof(uint16_t) && bytes <= room) { h->tab_lo = lo; h->tab_n = hi - lo + 1; }
        }
        C.tab_lo = h->tab_lo; C.tab_n = h->tab_n;
    }
    C.sfc_mtype = h->sfc_mtype; C.nxb = h->nxb; C.nyb = h->nyb;
    C.sfc_p0 = h->sfc_param[0]; C.sfc_p1 = h->sfc_param[1]; C.sfc_p2 = h->sfc_param[2];
    C.sfc_p3 = h->sfc_param[3]; C.sfc_p4 = h->sfc_param[4];
    C.sfc_sx = (float)(h->nxb / Lx); C.sfc_sy = (float)(h->nyb / Ly);
    C.sfc2d = h->sfc2d_host.empty() ? nullptr : h->d_sfc2d.p;
    C.lay = h->d_lay.p; C.views = h->d_views.p; C.counters = h->d_counters.p;
    C.cams = h->rad_kind == 1 ? h->d_cams.p : nullptr;
    C.heat = (h->target & MI3D_TARGET_HEAT) ? h->heat_ptr() : nullptr;
    int rc = h->d_cold.alloc(2);     // ([1]: the second set of event lists)
    if (rc) return rc;
    S.cold = h->d_cold.p;     // (uploaded by mi3d_run from h->cold_host, which outlives the asynchronous copy)
    return MI3D_OK;
}

// The sorts and sums of a flux run's last launches may still be on their way on the sort stream when mi3d_run returns (the next run's
// photon loops then start beside them): whoever reads the tallies, clears them or changes what the kernels work on makes the main
// stream wait for them first.
// the sums of the launch that used set q last (mi3d_solver::TlSet::pend), on stream st
static hipError_t launch_sum(mi3d_solver *h, int q, hipStream_t st) {
    mi3d_solver::PendingSum &P = h->tl[q].pend;
    P.on = false;
    if ((sizeof(double) << P.TL.shift) > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_tl_sum), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) << P.TL.shift));
    hipLaunchKernelGGL(k_tl_sum, dim3((unsigned)(P.TL.nbins * P.split)), dim3(1024), sizeof(double) << P.TL.shift, st, P.TL, P.flux, P.nflux, P.heat, P.nheat, P.split);
    return hipGetLastError();
}

static hipError_t tl_join(mi3d_solver *h) {
    if (!h->tl_unjoined) return hipSuccess;
    for (int q = 0; q < 2; ++q) {
        // (the main stream behind the sort of the set's last launch; that launch's sums, if they are still to come, on the main stream now)
        if (h->tl[q].used && h->tl[q].scattered) { const hipError_t e = hipStreamWaitEvent(h->stream, h->tl[q].scattered, 0); if (e != hipSuccess) return e; }
        if (h->tl[q].pend.on) { const hipError_t e = launch_sum(h, q, h->stream); if (e != hipSuccess) return e; }
    }
    h->tl_unjoined = false;
    return hipSuccess;
}
static hipError_t sync_main(mi3d_solver *h) {
    h->runs_unread = 0;
    const hipError_t e = tl_join(h);
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

// both streams of a handle (the ray kernels of launches with two sets of event lists run on a stream of their own)
static hipError_t sync_streams(mi3d_solver *h) {
    hipError_t e = tl_join(h);     // (sums that are still to come: on the main stream, before it is waited for)
    h->tl_unjoined = false;
    { const hipError_t e2 = hipStreamSynchronize(h->stream); if (e == hipSuccess) e = e2; }
    for (hipStream_t st : {h->rays_stream, h->tl_stream, h->pre_stream})
        if (st) { const hipError_t e2 = hipStreamSynchronize(st); if (e == hipSuccess) e = e2; }
    return e;
}

// the launch's DevCold goes to the device: [0] with the first set of event lists, [1] the same with the second set
static hipError_t upload_cold(mi3d_solver *h, bool two_sets, bool pre_two) {
    hipError_t e = hipMemcpyAsync(h->d_cold.p, &h->cold_host, sizeof(DevCold), hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess || !(two_sets || pre_two)) return e;
    h->cold_host2 = h->cold_host;
    if (two_sets) {
        h->cold_host2.ev_list = h->ev[1].events.p; h->cold_host2.ev_ctr = h->ev[1].evctr.p;
        h->cold_host2.hv_list = h->cold_host.hv_list ? h->ev[1].hvlist.p : nullptr;
    }
    if (pre_two) {   // (the second set of what the pre-pass writes; its cursors are its tiles' ends)
        if (h->cold_host.order) h->cold_host2.order = h->pre[1].order.p;
        if (h->cold_host.entry) h->cold_host2.entry = h->pre[1].entry.p;
        if (h->cold_host.tile_end) h->cold_host2.tile_end = h->pre[1].cursor.p;
    }
    return hipMemcpyAsync(h->d_cold.p + 1, &h->cold_host2, sizeof(DevCold), hipMemcpyHostToDevice, h->stream);
}

// Nothing is known about the events per photon any more (another scene, surface, source, solver): the next run with marched views
// starts with a pilot launch, and launches still on their way no longer count (mi3d_run does not wait for its last ones).
static inline void ev_forget(mi3d_solver *h) { h->ev_per_photon = 0.0; h->ev_epoch++; }

int check_handle(mi3d_solver *h) {
    if (!h) return fail(MI3D_EINVAL, "null solver handle");
    HIPCHK(hipSetDevice(h->device));
    return MI3D_OK;
}

// The power per unit domain area a job's photons stand for in all: Src_flx mu0 (solar), Src_flx P_tot / (Lx Ly) (thermal),
// Src_flx (P_tot + P_sol) / (Lx Ly) (solar+thermal)
double src_amp(const mi3d_solver *h) {
    if (h->src_mtype == 3) return h->src_flx * h->th_ptot / ((h->dx * h->nx) * (h->dy * h->ny));
    if (h->src_mtype == 2) return h->src_flx * (h->th_ptot + h->th_psol) / ((h->dx * h->nx) * (h->dy * h->ny));
    return h->src_flx * std::fabs(std::cos(h->src_the * 3.14159265358979323846 / 180.0));
}

// The atmosphere as cell_emission reads it (k_thermal_power, k_get_net_heating): valid once build_thermal has uploaded the temperatures
static ThermalGrid thermal_grid(const mi3d_solver *h) {
    ThermalGrid G;
    G.nx = h->nx; G.ny = h->ny; G.nz = h->nz; G.nz3 = h->nz3; G.k3lo = h->nz3 > 0 ? h->iz3l - 1 : 0; G.np1d = h->np1d; G.np3d = h->np3d;
    G.wl_um = h->th_wlen;
    G.lay = (const LayerRec *)h->d_lay.p;
    G.vrec = (const float4 *)(h->nz3 > 0 ? h->d_vrec.p : nullptr); G.vcol_f4 = h->vcol_f4; G.vrow_f4 = h->vrow_f4;
    G.csca = (const float2 *)h->d_csca.p;
    G.tlev = (const float *)h->d_th_tlev.p; G.tmpa3d = (const float *)(h->th_ntmpa ? h->d_th_tmpa.p : nullptr);
    return G;
}

// Thermal source: emitted power of every cell (k_thermal_power), its CDF and P_tot (k_scan_*), the photon loop's DevThermal.
int build_thermal(mi3d_solver *h) {
    if (h->src_mtype == 2 && !(h->src_fsol >= 0.0))
        return fail(MI3D_ESTATE, "solar+thermal source (Src_mtype=2): no solar irradiance set (mi3d_set_solar_irradiance)");
    if ((int)h->th_tlev.size() != h->nz + 1)
        return fail(MI3D_ESTATE, "thermal source: %d interface temperatures for Atm_nz=%d (call mi3d_set_thermal again)", (int)h->th_tlev.size(), h->nz);
    const size_t nvox = (size_t)h->nx * h->ny * h->nz3;
    if (h->th_ntmpa && h->th_ntmpa != nvox)
        return fail(MI3D_ESTATE, "thermal source: Atm_tmpa3d holds %zu voxels, the 3-D region %zu (call mi3d_set_thermal again)", h->th_ntmpa, nvox);
    const bool sfc2d = !h->sfc2d_host.empty();
    const size_t nsfc = sfc2d ? (size_t)h->nxb * h->nyb : 1;
    if (h->th_ntmps && (!sfc2d || h->th_ntmps != nsfc))
        return fail(MI3D_ESTATE, "thermal source: Sfc_tmps2d holds %zu cells, the surface %zu (call mi3d_set_thermal again)", h->th_ntmps, sfc2d ? nsfc : 0);
    if (!h->sfc_lambert_only) return fail(MI3D_EUNSUP, "thermal source: only Lambertian surfaces emit (Sfc_mtype / jsfc2d = 1)");
    const size_t ncell = nvox + (size_t)h->nz + nsfc;
    if (ncell > 4294967295ull) return fail(MI3D_EUNSUP, "thermal source: more than 2^32 cells");
    const size_t nblk = (ncell + kScanChunk - 1) / kScanChunk;
    int rc;
    if ((rc = h->d_th_cdf.alloc(ncell)) || (rc = h->d_th_bsum.alloc(nblk)) || (rc = h->d_th.alloc(1))) return rc;
    if ((rc = h->d_th_tlev.upload(h->th_tlev.data(), h->th_tlev.size()))) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, h->stream));
    hipLaunchKernelGGL(k_thermal_power, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, h->stream, thermal_grid(h), h->dx, h->dy,
                       sfc2d ? h->nxb : 1, sfc2d ? h->nyb : 1, (const float *)(sfc2d ? h->d_sfc2d.p : nullptr), h->sfc_param[0],
                       (const float *)(h->th_ntmps ? h->d_th_tmps.p : nullptr), h->d_th_cdf.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_scan_chunk, dim3((unsigned)nblk), dim3(kScanT), 0, h->stream, h->d_th_cdf.p, (unsigned long)ncell, h->d_th_bsum.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, h->stream, h->d_th_bsum.p, (unsigned long)nblk);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nblk), dim3(256), 0, h->stream, h->d_th_cdf.p, (unsigned long)ncell, (const double *)h->d_th_bsum.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, h->stream));
    double ptot = 0.0;
    HIPCHK(hipMemcpyAsync(&ptot, h->d_th_cdf.p + (ncell - 1), sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    h->th_ms = ms;
    if (!(ptot >= 0.0) || !std::isfinite(ptot)) return fail(MI3D_EINVAL, "thermal source: total emitted power %g", ptot);
    h->th_ptot = ptot;
    h->th_ncell = ncell;
    h->th_psol = 0.0;
    if (h->src_mtype == 2)
        h->th_psol = h->src_fsol * std::fabs(std::cos(h->src_the * 3.14159265358979323846 / 180.0)) * (h->dx * h->nx) * (h->dy * h->ny);
    DevThermal T;
    T.cdf = h->d_th_cdf.p; T.ptot = ptot; T.psol = h->th_psol; T.ncell = (unsigned)ncell; T.nvox = (unsigned)nvox;
    T.nxb = sfc2d ? h->nxb : 1; T.nyb = sfc2d ? h->nyb : 1;
    if ((rc = h->d_th.upload(&T, 1))) return rc;
    return MI3D_OK;
}

// Backward route (mi3d_set_camera_method 1): {ka, B(T)} of every cell of the thermal source, in the order of its CDF (k_backward_cells)
int build_backward_cells(mi3d_solver *h) {
    const size_t nvox = (size_t)h->nx * h->ny * h->nz3;
    const bool sfc2d = !h->sfc2d_host.empty();
    const size_t nsfc = sfc2d ? (size_t)h->nxb * h->nyb : 1;
    const size_t ncell = nvox + (size_t)h->nz + nsfc;
    int rc;
    if ((rc = h->d_bwd_cells.alloc(ncell))) return rc;
    if (!h->d_bwd_capped.p) {
        if ((rc = h->d_bwd_capped.alloc(1))) return rc;
        HIPCHK(hipMemsetAsync(h->d_bwd_capped.p, 0, sizeof(unsigned long long), h->stream));
    }
    hipLaunchKernelGGL(k_backward_cells, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, h->stream, thermal_grid(h),
                       sfc2d ? h->nxb : 1, sfc2d ? h->nyb : 1, (const float *)(sfc2d ? h->d_sfc2d.p : nullptr), h->sfc_param[0],
                       (const float *)(h->th_ntmps ? h->d_th_tmps.p : nullptr), h->d_bwd_cells.p);
    HIPCHK(hipGetLastError());
    return MI3D_OK;
}

// The direct sun in the cameras (k_cam_direct), per unit Src_flx; thermal jobs have none (zeros).
constexpr double kCamDirMaxCells = 1048576.0;   // voxels one march may cross (a few hundred milliseconds of one thread at most)
int build_camdir(mi3d_solver *h) {
    const size_t n = (size_t)h->nview * h->nxr * h->nyr;
    HIPCHK(sync_streams(h));   // (the uploads are synchronous copies; a statistics kernel of the last job may still read the image)
    int rc;
    if ((rc = h->d_camdir.alloc(n)) || (rc = h->d_zgrd.upload(h->zgrd.data(), h->zgrd.size()))) return rc;
    HIPCHK(hipMemsetAsync(h->d_camdir.p, 0, n * sizeof(double), h->stream));
    h->camdir_ok = true;
    if (h->src_mtype == 1) {
        const double pi = 3.14159265358979323846;
        const double th = h->src_the * pi / 180.0, ph = h->src_phi * pi / 180.0;
        const int k3lo = h->nz3 > 0 ? h->iz3l - 1 : 0;
        // the most voxels a march through the 3-D region can cross: one thread walks them, so a sun within a few thousandths of a degree
        // of the horizon (cells in proportion to 1 / cos) is not marched -- mi3d_get_camera_direct then fails; no job has to read it
        if (h->nz3 > 0) {
            const double h3 = h->zgrd[k3lo + h->nz3] - h->zgrd[k3lo], sz = -std::cos(th);
            const double cells = h->nz3 + 2.0 + h3 / sz * (std::fabs(std::sin(th) * std::cos(ph)) / h->dx + std::fabs(std::sin(th) * std::sin(ph)) / h->dy);
            if (!(cells <= kCamDirMaxCells)) { h->camdir_ok = false; return MI3D_OK; }
        }
        // (towards the sun: against the direction the photons of the direct beam travel in)
        hipLaunchKernelGGL(k_cam_direct, dim3((unsigned)((h->nview + 63) / 64)), dim3(64), 0, h->stream, h->nview, h->nxr, h->nyr,
                           (const CamRec *)h->d_cams.p, (const ViewRec *)h->d_views.p, (const double *)h->d_zgrd.p, (const LayerRec *)h->d_lay.p,
                           h->nz, h->nx, h->ny, h->nz3, k3lo, h->dx, h->dy, (const float *)(h->nz3 > 0 ? h->d_bext3.p : nullptr),
                           -std::sin(th) * std::cos(ph), -std::sin(th) * std::sin(ph), -std::cos(th), h->d_camdir.p);
        HIPCHK(hipGetLastError());
    }
    return MI3D_OK;
}

// ---- what the selectors and launchers of the forward routes' builds are made of (below: entry_build ... launch_general, launch_flux) -----
// Run-time flags as compile-time ones: f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...).  f is instantiated for every
// combination of its flags, so a selector names a kernel with flags only where the family has all of them
template <class F, bool... Bs>
static auto with_flags(F &&f, std::integer_sequence<bool, Bs...>) { return f(std::bool_constant<Bs>{}...); }
template <class F, bool... Bs, class... Rest>
static auto with_flags(F &&f, std::integer_sequence<bool, Bs...>, bool b, Rest... rest) {
    return b ? with_flags(f, std::integer_sequence<bool, Bs..., true>{}, rest...) : with_flags(f, std::integer_sequence<bool, Bs..., false>{}, rest...);
}
template <class F, class... Flags>
static auto with_flags(F &&f, bool b, Flags... rest) { return with_flags(f, std::integer_sequence<bool>{}, b, rest...); }

// One launch of a build.  More than the default 64 KB of dynamic LDS: the runtime is told first, for that kernel, on every such launch.
// No build (the selector knows none for what it was asked): an error, never another kernel.  The arguments go through the typed pointer:
// the compiler checks them against the family's signature
template <class... Params, class... Args>
static hipError_t launch_build(void (*kernel)(Params...), unsigned grid, unsigned threads, size_t lds, hipStream_t st, Args &&...args) {
    if (!kernel) return hipErrorInvalidValue;
    if (lds > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, std::forward<Args>(args)...);
    return hipGetLastError();
}

} // namespace

// =================================================================================================
extern "C" {

int mi3d_version(void) { return MI3D_VERSION; }

const char *mi3d_last_error(void) { return g_err.c_str(); }

int mi3d_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mi3d_create(int device, mi3d_solver **out) {
    if (!out) return fail(MI3D_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(MI3D_EDEVICE, "no HIP device available (%s); this solver has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(MI3D_EINVAL, "device %d out of range [0,%d)", device, n);
    HIPCHK(hipSetDevice(device));
    mi3d_solver *h = new mi3d_solver();
    h->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        h->num_cu = prop.multiProcessorCount;
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && v >= 32768) h->lds_max = v; else (void)hipGetLastError(); }
    int rc;
    if ((rc = h->d_counters.alloc(MI3D_NCOUNTER)) || (rc = h->d_next.alloc(8 * kCtrStride)) ||
        (rc = h->pre[0].cursor.alloc(kMaxTiles))) { delete h; return rc; }
    HIPCHK(hipMemset(h->d_counters.p, 0, MI3D_NCOUNTER * sizeof(unsigned long long)));
    HIPCHK(hipMemset(h->d_next.p, 0, 8 * kCtrStride * sizeof(unsigned long long)));
    {   // XCDs in use (eight on an MI355X in SPX mode; fewer in CPX / QPX partitions)
        DevBuf<unsigned> fl;
        unsigned host[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (fl.alloc(8) == MI3D_OK && hipMemset(fl.p, 0, sizeof(host)) == hipSuccess) {
            hipLaunchKernelGGL(k_xcc_census, dim3(4096), dim3(64), 0, nullptr, fl.p);
            if (hipMemcpy(host, fl.p, sizeof(host), hipMemcpyDeviceToHost) == hipSuccess) {
                int n = 0;
                for (unsigned f : host) n += f ? 1 : 0;
                if (n >= 1) h->n_xcd = n;
            }
        }
        (void)hipGetLastError();
        fl.release();
    }
    if (const char *e = getenv("MI3D_TILE_COLS")) h->tile_cols = atoi(e);          // tuning knobs, not part of the C-ABI
    if (const char *e = getenv("MI3D_RAD_SPREAD")) h->rad_spread = atoi(e);
    if (const char *e = getenv("MI3D_RAD_ROW_PAD")) h->rad_row_pad = atoi(e);
    if (const char *e = getenv("MI3D_TALLY_WINDOW")) h->tally_window = atoi(e) ? 1 : 0;
    if (const char *e = getenv("MI3D_TALLY_LISTS")) h->tally_lists = atoi(e) ? 1 : 0;
    if (const char *e = getenv("MI3D_TALLY_RUNS")) h->tally_runs = atoi(e) ? 1 : 0;
    if (const char *e = getenv("MI3D_ENTRY_RECORDS")) { const int v = atoi(e); h->entry_records = v == 2 ? 2 : (v ? 1 : 0); }
    if (const char *e = getenv("MI3D_OVERLAP_RAYS")) h->overlap_rays = atoi(e) ? 1 : 0;
    if (const char *e = getenv("MI3D_OVERLAP_SORT")) h->overlap_sort = std::max(0, std::min(2, atoi(e)));
    if (const char *e = getenv("MI3D_OVERLAP_PRE")) h->overlap_pre = std::max(0, std::min(2, atoi(e)));
    if (const char *e = getenv("MI3D_TL_SPLIT")) h->tl_split = std::max(1, std::min(64, atoi(e)));
    if (const char *e = getenv("MI3D_RAYS_WG")) h->rays_wg = std::max(0, std::min(8, atoi(e)));
    if (const char *e = getenv("MI3D_EMIT_WG")) h->emit_wg = std::max(0, std::min(8, atoi(e)));
    if (const char *e = getenv("MI3D_VPAD_COL")) h->vpad_col = std::max(0, atoi(e));
    if (const char *e = getenv("MI3D_VPAD_ROW")) h->vpad_row = std::max(0, atoi(e));
    if (const char *e = getenv("MI3D_KERNEL")) h->kernel_choice = std::strcmp(e, "generic") == 0 ? 1 : 0;
    if (const char *e = getenv("MI3D_EVCAP_LOG2")) { const int b = atoi(e); if (b >= 12 && b <= 28) h->ev_cap_log2 = b; }
    if (const char *e = getenv("MI3D_BATCH_LOG2")) { const int b = atoi(e); if (b >= 8 && b <= 30) h->batch = (uint64_t)1 << b; }
    *out = h;
    return MI3D_OK;
}

int mi3d_destroy(mi3d_solver *h) {
    if (!h) return MI3D_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    auto destroy_event = [](hipEvent_t e) { if (e) (void)hipEventDestroy(e); };
    for (auto &pr : h->pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    destroy_event(h->stats_ev);
    for (auto &S : h->ev_slot) destroy_event(S.done);
    for (auto &S : h->tl_slot) destroy_event(S.done);
    for (hipEvent_t e : h->tldesc_ev) destroy_event(e);
    destroy_event(h->pre_main);
    for (auto &P : h->pre) { destroy_event(P.done); destroy_event(P.loop); P.release(); P.cursor.release(); }
    for (auto &E : h->ev) { destroy_event(E.emit); destroy_event(E.rays); E.release(); E.evctr.release(); }
    for (auto &T : h->tl) { destroy_event(T.filled); destroy_event(T.sorted); destroy_event(T.scattered); T.release(); T.cursor.release(); }
    for (hipStream_t st : {h->own_stream, h->rays_stream, h->tl_stream, h->pre_stream}) if (st) (void)hipStreamDestroy(st);
    for (void *p : {(void *)h->h_evctr, (void *)h->h_tlctr, (void *)h->h_tldesc}) if (p) (void)hipHostFree(p);
    h->d_abst.release(); h->d_extp.release(); h->d_omgp.release(); h->d_apfp.release();
    h->d_lay.release(); h->d_vrec.release(); h->d_bext3.release(); h->d_tcol0.release(); h->d_tmu.release(); h->d_tp.release();
    h->d_tcdf.release(); h->d_tmuidx.release(); h->d_tcdfidx.release(); h->d_sfc2d.release(); h->d_csca.release(); h->d_rad_own.release();
    h->d_flux_own.release(); h->d_heat_own.release(); h->d_counters.release(); h->d_next.release();
    h->d_rad_acc.release(); h->d_cams.release(); h->d_camdir.release(); h->d_zgrd.release();
    h->d_hist.release(); h->d_tile.release(); h->d_tldesc.release(); h->d_tl_stats.release();
    for (int w = 0; w < 2; ++w) { h->d_run_own[w].release(); h->d_sum[w].release(); h->d_sumsq[w].release(); h->d_factor[w].release(); }
    h->d_stat_out.release(); h->d_dir_level.release(); h->d_get_out.release(); h->d_get_add.release();
    h->d_th_tlev.release(); h->d_th_tmpa.release(); h->d_th_tmps.release(); h->d_th_cdf.release(); h->d_th_bsum.release(); h->d_th.release();
    h->d_wgt_own.release(); h->d_wgt_out.release();
    h->d_prf_own.release(); h->d_prf_out.release();
    h->d_err_own.release(); h->d_err_out.release();
    h->d_bwd_cells.release(); h->d_bwd_capped.release(); h->d_bwd_norm.release(); h->d_bwd_score.release(); h->d_bwd_dir.release(); h->d_bwd_start.release();
    h->d_views.release(); h->d_cold.release(); h->d_tabrange.release(); h->d_bt1d.release(); h->d_dz.release(); h->d_bmin.release(); h->d_bmax.release();
    delete h;
    return MI3D_OK;
}

int mi3d_set_atm1d(mi3d_solver *h, int nz, const double *zgrd, int np1d, const float *ext, const float *omg,
                   const float *apf, const float *abs) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (nz < 1 || nz > kMaxLayers) return fail(MI3D_EINVAL, "Atm_nz=%d outside [1,%d]", nz, kMaxLayers);
    if (np1d < 1 || np1d > MI3D_MAX_NP1D) return fail(MI3D_EINVAL, "Atm_np1d=%d outside [1,%d]", np1d, MI3D_MAX_NP1D);
    if (!zgrd || !ext || !omg || !apf) return fail(MI3D_EINVAL, "NULL 1-D profile");
    for (int k = 0; k < nz; ++k)
        if (!(zgrd[k + 1] > zgrd[k])) return fail(MI3D_EINVAL, "Atm_zgrd0 must ascend strictly (level %d)", k + 1);
    const size_t n = (size_t)nz * np1d;
    for (size_t i = 0; i < n; ++i)
        if (!(ext[i] >= 0.0f) || !(omg[i] >= 0.0f)) return fail(MI3D_EINVAL, "negative or NaN 1-D extinction / albedo");
    if (h->nz != nz) h->dirty_tally = true;
    h->nz = nz; h->np1d = np1d;
    h->zgrd.assign(zgrd, zgrd + nz + 1);
    h->ext1d.assign(ext, ext + n); h->omg1d.assign(omg, omg + n); h->apf1d.assign(apf, apf + n);
    if (abs) h->abs1d.assign(abs, abs + nz); else h->abs1d.assign(nz, 0.0f);
    h->have_1d = true;
    h->dirty_grid = true;
    return MI3D_OK;
}

int mi3d_set_atm3d(mi3d_solver *h, int nx, int ny, int nz3, int iz3l, int np3d, double dx, double dy,
                   const float *abst, const float *extp, const float *omgp, const float *apfp) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (nx < 1 || ny < 1 || nz3 < 0) return fail(MI3D_EINVAL, "bad grid %d x %d x %d", nx, ny, nz3);
    if (!(dx > 0.0) || !(dy > 0.0)) return fail(MI3D_EINVAL, "Atm_dx / Atm_dy must be positive");
    if (nz3 > 0) {
        if (np3d < 1 || np3d > MI3D_MAX_NP3D) return fail(MI3D_EINVAL, "Atm_np3d=%d outside [1,%d]", np3d, MI3D_MAX_NP3D);
        if (!extp || !omgp || !apfp) return fail(MI3D_EINVAL, "NULL 3-D array");
        if (iz3l < 1) return fail(MI3D_EINVAL, "Atm_iz3l=%d must be >= 1", iz3l);
    }
    if (h->nx != nx || h->ny != ny) h->dirty_tally = true;
    h->nx = nx; h->ny = ny; h->nz3 = nz3; h->iz3l = nz3 > 0 ? iz3l : 1; h->np3d = nz3 > 0 ? np3d : 0;
    h->dx = dx; h->dy = dy;
    h->has_abst = false;
    if (nz3 > 0) {
        const size_t nvox = (size_t)nx * ny * nz3;
        if (abst) { if ((rc = h->d_abst.upload(abst, nvox))) return rc; h->has_abst = true; }
        if ((rc = h->d_extp.upload(extp, nvox * np3d))) return rc;
        if ((rc = h->d_omgp.upload(omgp, nvox * np3d))) return rc;
        if ((rc = h->d_apfp.upload(apfp, nvox * np3d))) return rc;
    }
    h->dirty_grid = true;
    return MI3D_OK;
}

int mi3d_set_phase(mi3d_solver *h, int nang, int npf, const float *ang, const float *pha) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (npf <= 0) { h->npf = 0; h->nang = 0; h->ang.clear(); h->pha.clear(); h->dirty_phase = true; return MI3D_OK; }
    if (nang < 2 || !ang || !pha) return fail(MI3D_EINVAL, "bad phase table (Sca_nangi=%d)", nang);
    for (size_t i = 0; i < (size_t)nang * npf; ++i)
        if (!(pha[i] >= 0.0f)) return fail(MI3D_EINVAL, "negative or NaN phase-function value");
    h->nang = nang; h->npf = npf;
    h->ang.assign(ang, ang + nang);
    h->pha.assign(pha, pha + (size_t)nang * npf);
    h->dirty_phase = true;
    return MI3D_OK;
}

int mi3d_set_surface(mi3d_solver *h, int mtype, const float param[5]) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (mtype != MI3D_SFC_LAMBERT && mtype != MI3D_SFC_LSRT && mtype != MI3D_SFC_DSM) return fail(MI3D_EINVAL, "unknown Sfc_mtype=%d", mtype);
    if (!param) return fail(MI3D_EINVAL, "NULL Sfc_param");
    h->sfc_mtype = mtype;
    h->sfc_lambert_only = (mtype == MI3D_SFC_LAMBERT);
    for (int i = 0; i < 5; ++i) h->sfc_param[i] = param[i];
    h->sfc2d_host.clear(); h->nxb = h->nyb = 0;
    h->dirty_sfc = true;
    h->dirty_thermal = true;
    ev_forget(h);   // (a brighter surface: more events per photon; the next run with marched views starts with a pilot launch)
    return MI3D_OK;
}

int mi3d_set_surface2d(mi3d_solver *h, int nxb, int nyb, const float *tmps, const float *jsfc, const float *psfc) {
    (void)tmps;
    int rc = check_handle(h);
    if (rc) return rc;
    if (nxb < 1 || nyb < 1 || !jsfc || !psfc) return fail(MI3D_EINVAL, "bad 2-D surface (%d x %d)", nxb, nyb);
    const size_t n = (size_t)nxb * nyb;
    std::vector<float> packed(n * 8, 0.0f);
    bool lambert_only = true;
    for (size_t i = 0; i < n; ++i) {
        const int t = (int)std::lround(jsfc[i]);
        lambert_only = lambert_only && t == MI3D_SFC_LAMBERT;
        if (t != MI3D_SFC_LAMBERT && t != MI3D_SFC_LSRT && t != MI3D_SFC_DSM) return fail(MI3D_EINVAL, "unknown surface model id %d in jsfc2d", t);
        packed[i * 8 + 0] = (float)t;
        for (int q = 0; q < 5; ++q) packed[i * 8 + 1 + q] = psfc[q * n + i];
    }
    h->sfc2d_host.swap(packed);
    h->sfc_lambert_only = lambert_only;
    h->nxb = nxb; h->nyb = nyb;
    h->dirty_sfc = true;
    h->dirty_thermal = true;
    ev_forget(h);
    return MI3D_OK;
}

int mi3d_set_source(mi3d_solver *h, double flx, double qmax_deg, double the_deg, double phi_deg) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!(the_deg > 90.0 && the_deg <= 180.0)) return fail(MI3D_EINVAL, "Src_the=%g: the sun must shine downwards (90 < the <= 180)", the_deg);
    if (!(qmax_deg >= 0.0 && qmax_deg < 90.0)) return fail(MI3D_EINVAL, "Src_qmax=%g out of range", qmax_deg);
    if (h->src_the != the_deg || h->src_phi != phi_deg || h->src_qmax != qmax_deg) ev_forget(h);
    h->src_flx = flx; h->src_qmax = qmax_deg; h->src_the = the_deg; h->src_phi = phi_deg;
    h->dirty_camdir = true;
    if (h->src_mtype == 2) h->dirty_thermal = true;   // (P_sol holds mu0)
    return MI3D_OK;
}

int mi3d_set_thermal(mi3d_solver *h, int mtype, double wlen_um, int nlev, const float *tmp1d, const float *tmpa3d,
                     const float *tmps2d) {
    int rc = check_handle(h);
    if (rc) return rc;
    h->dirty_camdir = true;
    if (mtype == 1) {
        if (h->src_mtype != 1) ev_forget(h);
        h->src_mtype = 1; h->th_ptot = 0.0; h->dirty_thermal = false;
        return MI3D_OK;
    }
    if (mtype == 0) return fail(MI3D_EUNSUP, "Src_mtype=0: only the solar (1), the solar+thermal (2) and the thermal (3) source are supported");
    if (mtype != 3 && mtype != 2) return fail(MI3D_EINVAL, "unknown Src_mtype=%d", mtype);
    if (!h->have_1d) return fail(MI3D_ESTATE, "mi3d_set_atm1d has not been called");
    if (!(wlen_um > 0.0) || !std::isfinite(wlen_um)) return fail(MI3D_EINVAL, "Src_wlen=%g um must be positive", wlen_um);
    if (nlev != h->nz + 1) return fail(MI3D_EINVAL, "Atm_tmp1d: %d values for Atm_nz=%d -- the thermal source needs the nz+1 INTERFACE temperatures", nlev, h->nz);
    if (!tmp1d) return fail(MI3D_EINVAL, "NULL Atm_tmp1d");
    for (int i = 0; i < nlev; ++i)
        if (!(tmp1d[i] > 0.0f) || !std::isfinite(tmp1d[i])) return fail(MI3D_EINVAL, "Atm_tmp1d(%d)=%g K must be positive", i + 1, tmp1d[i]);
    const size_t nvox = (size_t)h->nx * h->ny * h->nz3;
    h->th_ntmpa = 0; h->th_ntmps = 0;
    if (tmpa3d && nvox > 0) {
        for (size_t i = 0; i < nvox; ++i) if (!std::isfinite(tmpa3d[i])) return fail(MI3D_EINVAL, "non-finite Atm_tmpa3d");
        if ((rc = h->d_th_tmpa.upload(tmpa3d, nvox))) return rc;
        h->th_ntmpa = nvox;
    }
    if (tmps2d) {
        if (h->sfc2d_host.empty()) return fail(MI3D_EINVAL, "Sfc_tmps2d given for a uniform surface (mi3d_set_surface2d first)");
        const size_t nsfc = (size_t)h->nxb * h->nyb;
        for (size_t i = 0; i < nsfc; ++i) if (!std::isfinite(tmps2d[i])) return fail(MI3D_EINVAL, "non-finite Sfc_tmps2d");
        if ((rc = h->d_th_tmps.upload(tmps2d, nsfc))) return rc;
        h->th_ntmps = nsfc;
    }
    if (h->src_mtype != mtype) ev_forget(h);
    h->src_mtype = mtype; h->th_wlen = wlen_um;
    h->th_tlev.assign(tmp1d, tmp1d + nlev);
    h->dirty_thermal = true;
    return MI3D_OK;
}

int mi3d_set_solar_irradiance(mi3d_solver *h, double fsol) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!(fsol >= 0.0) || !std::isfinite(fsol)) return fail(MI3D_EINVAL, "Src_fsol=%g W m-2 um-1 must be finite and >= 0", fsol);
    h->src_fsol = fsol;
    if (h->src_mtype == 2) h->dirty_thermal = true;
    return MI3D_OK;
}

int mi3d_get_source_power(mi3d_solver *h, double *ptot, double *psol) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!h->thermal()) return fail(MI3D_ESTATE, "mi3d_get_source_power: the job is solar (Src_mtype=1): its photons stand for Src_flx mu0 Lx Ly");
    if ((rc = mi3d_prepare(h))) return rc;
    if (ptot) *ptot = h->th_ptot;
    if (psol) *psol = h->th_psol;
    return MI3D_OK;
}

int mi3d_set_views(mi3d_solver *h, int nview, const double *the_deg, const double *phi_deg, const double *zloc,
                   double zref, int nxr, int nyr) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (nview < 0 || nview > MI3D_MAX_VIEW) return fail(MI3D_EINVAL, "Rad_nrad=%d outside [0,%d]", nview, MI3D_MAX_VIEW);
    if (nxr < 1 || nyr < 1) return fail(MI3D_EINVAL, "bad Rad_nxr/Rad_nyr");
    for (int i = 0; i < nview; ++i) {
        if (!(the_deg[i] >= 0.0 && the_deg[i] <= 180.0) || std::fabs(std::cos(the_deg[i] * 3.14159265358979323846 / 180.0)) <= 1e-6)
            return fail(MI3D_EINVAL, "Rad_the=%g: the line of sight must not be horizontal (0 <= the <= 180, the != 90)", the_deg[i]);
        h->view_the[i] = the_deg[i]; h->view_phi[i] = phi_deg[i]; h->view_zloc[i] = zloc[i];
    }
    if (h->nview != nview || h->nxr != nxr || h->nyr != nyr) h->dirty_tally = true;
    h->nview = nview; h->zref = zref; h->nxr = nxr; h->nyr = nyr;
    h->rad_kind = 2;
    h->dirty_views = true;
    return MI3D_OK;
}

int mi3d_set_cameras(mi3d_solver *h, int ncam, const double *the_deg, const double *phi_deg, const double *psi_deg,
                     const double *xpos, const double *ypos, const double *zloc, const double *qmax_deg,
                     const double *umax_deg, const double *vmax_deg, const double *apsize, int nxr, int nyr) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (ncam < 1 || ncam > MI3D_MAX_VIEW) return fail(MI3D_EINVAL, "Rad_nrad=%d outside [1,%d]", ncam, MI3D_MAX_VIEW);
    if (nxr < 1 || nyr < 1) return fail(MI3D_EINVAL, "bad Rad_nxr/Rad_nyr");
    if (!the_deg || !phi_deg || !psi_deg || !xpos || !ypos || !zloc || !qmax_deg || !umax_deg || !vmax_deg || !apsize)
        return fail(MI3D_EINVAL, "NULL camera array");
    for (int i = 0; i < ncam; ++i) {
        if (!(qmax_deg[i] > 0.0 && qmax_deg[i] <= 360.0) || !(umax_deg[i] > 0.0) || !(vmax_deg[i] > 0.0) || !(apsize[i] >= 0.0))
            return fail(MI3D_EINVAL, "camera %d: Rad_qmax=%g, Rad_umax=%g, Rad_vmax=%g, Rad_apsize=%g", i + 1, qmax_deg[i], umax_deg[i], vmax_deg[i], apsize[i]);
        h->view_the[i] = the_deg[i]; h->view_phi[i] = phi_deg[i]; h->view_zloc[i] = zloc[i];
        h->cam_psi[i] = psi_deg[i]; h->cam_xpos[i] = xpos[i]; h->cam_ypos[i] = ypos[i];
        h->cam_qmax[i] = qmax_deg[i]; h->cam_umax[i] = umax_deg[i]; h->cam_vmax[i] = vmax_deg[i]; h->cam_apsize[i] = apsize[i];
    }
    if (h->nview != ncam || h->nxr != nxr || h->nyr != nyr) h->dirty_tally = true;
    h->nview = ncam; h->nxr = nxr; h->nyr = nyr; h->zref = 0.0;
    h->rad_kind = 1;
    h->dirty_views = true;
    return MI3D_OK;
}

int mi3d_set_camera_method(mi3d_solver *h, int method) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (method != 0 && method != 1) return fail(MI3D_EINVAL, "camera method %d (0: forward local estimates, 1: backward Monte Carlo)", method);
    if (method == h->cam_method) return MI3D_OK;
    HIPCHK(sync_main(h));   // (as every call that changes what the kernels work on)
    h->cam_method = method;
    return MI3D_OK;
}

int mi3d_set_view_method(mi3d_solver *h, int method) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (method != 0 && method != 1) return fail(MI3D_EINVAL, "view method %d (0: forward local estimates, 1: backward Monte Carlo)", method);
    if (method == h->view_method) return MI3D_OK;
    HIPCHK(sync_main(h));   // (as every call that changes what the kernels work on)
    h->view_method = method;
    return MI3D_OK;
}

int mi3d_set_view_sunlight(mi3d_solver *h, int on) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (on != 0 && on != 1) return fail(MI3D_EINVAL, "view sunlight %d (0: off, 1: the sunlight term of the backward route's satellite views)", on);
    if (on == h->view_sunlight) return MI3D_OK;
    HIPCHK(sync_main(h));   // (as every call that changes what the kernels work on)
    h->view_sunlight = on;
    h->dirty_bwd = true;
    return MI3D_OK;
}

int mi3d_set_view_columns(mi3d_solver *h, int on) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (on != 0 && on != 1) return fail(MI3D_EINVAL, "view columns %d (0: off, 1: the backward route's satellite views under independent columns and partial 3-D)", on);
    if (on == h->view_columns) return MI3D_OK;
    HIPCHK(sync_main(h));   // (as every call that changes what the kernels work on)
    h->view_columns = on;
    h->dirty_bwd = true;
    return MI3D_OK;
}

int mi3d_set_emission_weights(mi3d_solver *h, int on) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (on != 0 && on != 1) return fail(MI3D_EINVAL, "emission weights %d (0: off, 1: per-cell weights of the backward route)", on);
    if (on == h->emis_weights) return MI3D_OK;
    HIPCHK(sync_main(h));   // (as every call that changes what the kernels work on)
    h->emis_weights = on;
    if (!on) { h->d_wgt_own.release(); h->d_wgt_out.release(); h->wgt_n = 0; }   // (gigabytes, for a large job)
    return MI3D_OK;
}

int mi3d_bind_weights_buffer(mi3d_solver *h, void *wgt_sum) {
    int rc = check_handle(h);
    if (rc) return rc;
    if ((double *)wgt_sum == h->wgt_ext) return MI3D_OK;
    HIPCHK(sync_main(h));
    h->wgt_ext = (double *)wgt_sum;
    if (!wgt_sum) h->wgt_n = 0;   // (the library's own buffer is made anew, and zeroed, by the next run)
    return MI3D_OK;
}

int mi3d_set_view_profiles(mi3d_solver *h, int on) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (on != 0 && on != 1) return fail(MI3D_EINVAL, "view profiles %d (0: off, 1: per-layer weighting functions of the backward route's satellite views)", on);
    if (on == h->view_profiles) return MI3D_OK;
    HIPCHK(sync_main(h));   // (as every call that changes what the kernels work on)
    h->view_profiles = on;
    h->prf_ran = false;
    if (!on) { h->d_prf_own.release(); h->d_prf_out.release(); h->prf_n = 0; }
    return MI3D_OK;
}

int mi3d_bind_view_profiles_buffer(mi3d_solver *h, void *raw) {
    int rc = check_handle(h);
    if (rc) return rc;
    if ((double *)raw == h->prf_ext) return MI3D_OK;
    HIPCHK(sync_main(h));
    h->prf_ext = (double *)raw;
    if (!raw) h->prf_n = 0;   // (the library's own buffer is made anew, and zeroed, by the next run)
    return MI3D_OK;
}

int mi3d_set_pixel_errors(mi3d_solver *h, int on) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (on != 0 && on != 1) return fail(MI3D_EINVAL, "pixel errors %d (0: off, 1: per-pixel standard errors of the backward route)", on);
    if (on == h->pixel_errors) return MI3D_OK;
    HIPCHK(sync_main(h));   // (as every call that changes what the kernels work on)
    h->pixel_errors = on;
    h->err_ran = false;
    if (!on) { h->d_err_own.release(); h->d_err_out.release(); h->err_n = 0; }
    return MI3D_OK;
}

int mi3d_bind_pixel_errors_buffer(mi3d_solver *h, void *rad2_sum) {
    int rc = check_handle(h);
    if (rc) return rc;
    if ((double *)rad2_sum == h->err_ext) return MI3D_OK;
    HIPCHK(sync_main(h));
    h->err_ext = (double *)rad2_sum;
    if (!rad2_sum) h->err_n = 0;   // (the library's own buffer is made anew, and zeroed, by the next run)
    return MI3D_OK;
}

int mi3d_set_camera_map(mi3d_solver *h, int mpmap, int mrproj) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (mpmap != 1 && mpmap != 2) return fail(MI3D_EINVAL, "Rad_mpmap=%d: 1 (polar) or 2 (rectangular)", mpmap);
    if (mrproj != 0 && mrproj != 1) return fail(MI3D_EINVAL, "Rad_mrproj=%d: 0 (mean radiance) or 1 (cosine-weighted)", mrproj);
    if (h->cam_mpmap != mpmap || h->cam_mrproj != mrproj) h->dirty_views = true;
    h->cam_mpmap = mpmap; h->cam_mrproj = mrproj;
    return MI3D_OK;
}

int mi3d_set_options(mi3d_solver *h, int target, int solver, double wmin, double wfac, int column_le) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (target < 1 || target > 7) return fail(MI3D_EINVAL, "target=%d", target);
    if ((target & MI3D_TARGET_HEAT) && !(target & MI3D_TARGET_FLUX))
        return fail(MI3D_EINVAL, "target=%d: heating rates (Flx_mhrt=1) come with the fluxes (MI3D_TARGET_FLUX | MI3D_TARGET_HEAT)", target);
    if ((target & MI3D_TARGET_HEAT) != (h->target & MI3D_TARGET_HEAT)) h->dirty_tally = true;
    if (solver != MI3D_SOLVER_3D && solver != MI3D_SOLVER_P3D && solver != MI3D_SOLVER_IPA) return fail(MI3D_EINVAL, "solver=%d", solver);
    if (!(wmin >= 0.0 && wmin <= 1.0)) return fail(MI3D_EINVAL, "Pho_wmin=%g outside [0,1]", wmin);
    if (!(wfac >= wmin && wfac > 0.0)) return fail(MI3D_EINVAL, "Pho_wfac=%g must be positive and not below Pho_wmin=%g", wfac, wmin);
    if (h->solver != solver || h->wmin != wmin || h->wfac != wfac) ev_forget(h);
    h->target = target; h->solver = solver; h->wmin = wmin; h->wfac = wfac; h->column_le = column_le ? 1 : 0;
    h->dirty_views = true;
    return MI3D_OK;
}

int mi3d_set_le_roulette(mi3d_solver *h, double tau1) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!(tau1 >= 0.0) || tau1 > 16.0) return fail(MI3D_EINVAL, "le roulette threshold %g outside [0, 16]", tau1);
    h->le_tau1 = tau1;
    h->dirty_views = true;
    return MI3D_OK;
}

int mi3d_set_le_weight_roulette(mi3d_solver *h, double cmin) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!(cmin >= 0.0) || cmin > 1.0) return fail(MI3D_EINVAL, "le weight roulette threshold %g outside [0, 1]", cmin);
    h->le_cmin = cmin;
    h->dirty_views = true;
    return MI3D_OK;
}

int mi3d_set_counting(mi3d_solver *h, int on) {
    int rc = check_handle(h);
    if (rc) return rc;
    h->counting = on ? 1 : 0;
    return MI3D_OK;
}

int mi3d_bind_device_buffers(mi3d_solver *h, void *rad_sum, void *flux_sum, void *stream) {
    int rc = check_handle(h);
    if (rc) return rc;
    h->rad_ext = (tally_t *)rad_sum;
    h->flux_ext = (tally_t *)flux_sum;
    const hipStream_t st = stream ? (hipStream_t)stream : (h->use_own_stream ? h->own_stream : nullptr);
    if (st != h->stream) {
        (void)sync_streams(h);                            // nothing of this handle is left behind on the stream it leaves (a caller's stream
                                                          // that no longer exists is the caller's business: not an error here)
        (void)hipGetLastError();
        h->stream = st;
    }
    if (!rad_sum || !flux_sum) h->dirty_tally = true;     // own buffers are (re)created on demand by mi3d_prepare
    return MI3D_OK;
}

int mi3d_set_heating_estimator(mi3d_solver *h, int estimator) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (estimator != 0 && estimator != 1) return fail(MI3D_EINVAL, "heating estimator %d (0: collision, 1: path length)", estimator);
    if (estimator == h->heat_estimator) return MI3D_OK;
    HIPCHK(sync_main(h));   // (as every call that changes what the kernels work on)
    h->heat_estimator = estimator;
    // (another estimator, other records per photon: the lists are sized anew; its sums and the other one's do not mix in one tally)
    h->tl_per_photon = 0.0; h->tl_total_pp = 0.0; h->tl_runs_pp = 0.0;
    for (auto &S : h->tl_slot) S.busy = false;
    if (h->target & MI3D_TARGET_HEAT) h->dirty_tally = true;
    return MI3D_OK;
}

int mi3d_bind_heating_buffer(mi3d_solver *h, void *heat_sum) {
    int rc = check_handle(h);
    if (rc) return rc;
    h->heat_ext = (double *)heat_sum;
    if (!heat_sum && (h->target & MI3D_TARGET_HEAT)) h->dirty_tally = true;
    return MI3D_OK;
}

int mi3d_prepare(mi3d_solver *h) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!h->have_1d) return fail(MI3D_ESTATE, "mi3d_set_atm1d has not been called");
    // the uploads below are synchronous copies that do not wait for this handle's (non-blocking) stream: nothing still running
    // there may read what they overwrite
    if (h->dirty_grid || h->dirty_views || h->dirty_phase || h->dirty_sfc || h->dirty_tally) HIPCHK(sync_streams(h));
    if (h->dirty_grid) {
        const int nz = h->nz;
        const int k3lo = h->nz3 > 0 ? h->iz3l - 1 : 0, k3hi = h->nz3 > 0 ? k3lo + h->nz3 : 0;
        if (h->nz3 > 0 && (k3lo < 0 || k3hi > nz))
            return fail(MI3D_EINVAL, "3-D layers %d..%d (Atm_iz3l=%d, Atm_nz3=%d) do not fit Atm_nz=%d", k3lo + 1,
                        k3hi, h->iz3l, h->nz3, nz);
        std::vector<float> bt1d(nz), dz(nz);
        for (int k = 0; k < nz; ++k) {
            double b = h->abs1d[k];
            for (int ip = 0; ip < h->np1d; ++ip) b += h->ext1d[(size_t)ip * nz + k];
            bt1d[k] = (float)(b > 0.0 ? b : 0.0);
            dz[k] = (float)(h->zgrd[k + 1] - h->zgrd[k]);
        }
        h->tab3d_lo = 1 << 30; h->tab3d_hi = -1; h->hg3d = true;
        std::vector<int> uniform3d(h->nz3, 0);
        std::vector<float> bt3d(h->nz3, 0.0f);
        if (h->nz3 > 0) {
            const size_t nvox = (size_t)h->nx * h->ny * h->nz3, ncol = (size_t)h->nx * h->ny;
            if ((rc = h->d_bt1d.upload(bt1d.data(), nz)) || (rc = h->d_dz.upload(dz.data(), nz))) return rc;
            h->vcol_f4 = (unsigned)(h->nz3 + h->vpad_col); h->vrow_f4 = (unsigned)h->nx * h->vcol_f4 + (unsigned)h->vpad_row;
            if ((rc = h->d_bext3.alloc(nvox)) || (rc = h->d_vrec.alloc((size_t)h->ny * h->vrow_f4)) || (rc = h->d_csca.alloc(h->np3d > 1 ? nvox * h->np3d : 1)) ||
                (rc = h->d_tcol0.alloc(ncol)) || (rc = h->d_bmin.alloc(h->nz3)) ||
                (rc = h->d_bmax.alloc(h->nz3)))
                return rc;
            const int tb = 256;
            const float *abst = h->has_abst ? h->d_abst.p : nullptr;
            hipLaunchKernelGGL(k_build_grid, dim3((unsigned)((nvox + tb - 1) / tb)), dim3(tb), 0, h->stream, h->nx,
                               h->ny, h->nz3, k3lo, h->np3d, h->d_bt1d.p, abst, h->d_extp.p, h->d_omgp.p,
                               h->d_apfp.p, h->d_vrec.p, h->d_csca.p, h->vcol_f4, h->vrow_f4, h->d_bext3.p);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_layer_uniform, dim3(h->nz3), dim3(tb), 0, h->stream, h->nx, h->ny, h->nz3, k3lo,
                               h->np3d, h->d_bt1d.p, abst, h->d_extp.p, h->d_bmin.p, h->d_bmax.p);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_build_column, dim3((unsigned)((ncol + tb - 1) / tb)), dim3(tb), 0, h->stream,
                               (int)ncol, h->nz3, k3lo, nz, h->d_bt1d.p, h->d_dz.p, h->d_vrec.p, h->d_tcol0.p, h->nx, h->vcol_f4, h->vrow_f4);
            HIPCHK(hipGetLastError());
            int init[3] = {1 << 30, -1, 0};
            if ((rc = h->d_tabrange.upload(init, 3))) return rc;
            hipLaunchKernelGGL(k_apf_range, dim3(1024), dim3(tb), 0, h->stream, (long)(nvox * h->np3d), h->d_extp.p,
                               h->d_apfp.p, h->d_tabrange.p);
            HIPCHK(hipGetLastError());
            std::vector<float> bmin(h->nz3), bmax(h->nz3);
            HIPCHK(sync_main(h));
            HIPCHK(hipMemcpy(init, h->d_tabrange.p, sizeof(init), hipMemcpyDeviceToHost));
            h->tab3d_lo = init[0]; h->tab3d_hi = init[1]; h->hg3d = (init[2] == 0) && (init[1] < 0);
            HIPCHK(hipMemcpy(bmin.data(), h->d_bmin.p, h->nz3 * sizeof(float), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(bmax.data(), h->d_bmax.p, h->nz3 * sizeof(float), hipMemcpyDeviceToHost));
            double wsum = 0.0, wz = 0.0;
            for (int k3 = 0; k3 < h->nz3; ++k3) {
                uniform3d[k3] = (bmin[k3] == bmax[k3]) ? 1 : 0;
                bt3d[k3] = bmin[k3];
                const double wgt = (double)bmax[k3] - (double)bmin[k3];
                wsum += wgt; wz += wgt * 0.5 * (h->zgrd[k3lo + k3] + h->zgrd[k3lo + k3 + 1]);
            }
            h->z_cloud = wsum > 0.0 ? wz / wsum : -1.0;
        }
        std::vector<LayerRec> lay;
        if ((rc = build_layers(h, uniform3d, bt3d, lay))) return rc;
        if ((rc = h->d_lay.upload(lay.data(), lay.size()))) return rc;
        h->lay_host = lay;
        h->dirty_grid = false;
        h->dirty_thermal = true;
        h->dirty_views = true;
        // another scene (or another g of it: the gas absorption moves the events per photon too): the next run with marched views
        // starts with a pilot launch again -- an event list that runs full fails the run.  The tally-record lists of flux jobs KEEP what
        // earlier launches reported (round 6): a list of theirs that runs full loses nothing but speed, the next launch is sized by what this
        // one needed, and er3t's jobs -- sixteen g of one scene, a few million photons each -- are not cut in two by a pilot launch and a
        // wait each
        ev_forget(h);
        for (auto &S : h->tl_slot) S.busy = false;
    }
    if (h->dirty_views) {
        if ((rc = build_views(h))) return rc;
        h->dirty_views = false;
        h->dirty_camdir = true;
    }
    if (h->dirty_phase) {
        if ((rc = build_tables(h))) return rc;
        h->dirty_phase = false;
    }
    if (h->npf <= 0 && needs_tables(h))
        return fail(MI3D_ESTATE, "a 1-D component selects a tabulated phase function (apf >= 1) but no table is loaded");
    if (h->dirty_sfc) {
        if (!h->sfc2d_host.empty())
            if ((rc = h->d_sfc2d.upload(h->sfc2d_host.data(), h->sfc2d_host.size()))) return rc;
        h->dirty_sfc = false;
    }
    if (h->dirty_tally) {
        if (!h->rad_ext) {
            if ((rc = h->d_rad_own.alloc(h->rad_elems()))) return rc;
            HIPCHK(hipMemsetAsync(h->d_rad_own.p, 0, h->rad_elems() * sizeof(tally_t), h->stream));
        }
        if (!h->flux_ext) {
            if ((rc = h->d_flux_own.alloc(h->flux_elems()))) return rc;
            HIPCHK(hipMemsetAsync(h->d_flux_own.p, 0, h->flux_elems() * sizeof(tally_t), h->stream));
        }
        if ((h->target & MI3D_TARGET_HEAT) && !h->heat_ext) {
            if ((rc = h->d_heat_own.alloc(h->heat_elems()))) return rc;
            HIPCHK(hipMemsetAsync(h->d_heat_own.p, 0, h->heat_elems() * sizeof(double), h->stream));
        }
        h->wgt_n = 0;   // (the emission weights' own buffer: made and zeroed by the next run that tallies them, run_backward)
        h->prf_n = 0; h->prf_ran = false;   // (likewise the view profiles')
        h->err_n = 0; h->err_ran = false;   // (and the pixel errors')
        h->dirty_tally = false;
    }
    if (h->thermal() && h->dirty_thermal) {
        if ((rc = build_thermal(h))) return rc;
        h->dirty_thermal = false;
        h->dirty_bwd = true;
    }
    if ((h->cam_method == 1 || h->view_method == 1) && (h->src_mtype == 3 || (h->src_mtype == 2 && h->view_sunlight)) && h->dirty_bwd) {
        if ((rc = build_backward_cells(h))) return rc;
        h->dirty_bwd = false;
    }
    if (h->rad_kind == 1 && h->nview > 0 && h->dirty_camdir) {
        if ((rc = build_camdir(h))) return rc;
        h->dirty_camdir = false;
    }
    return MI3D_OK;
}

int mi3d_reset(mi3d_solver *h) {
    int rc = check_handle(h);
    if (rc) return rc;
    if ((rc = mi3d_prepare(h))) return rc;
    // (a run that failed half way may have left ray kernels on their own stream: the tallies are cleared after them)
    for (const auto &E : h->ev) if (E.used && E.rays) HIPCHK(hipStreamWaitEvent(h->stream, E.rays, 0));
    HIPCHK(tl_join(h));
    HIPCHK(hipMemsetAsync(h->rad_ptr(), 0, h->rad_elems() * sizeof(tally_t), h->stream));
    HIPCHK(hipMemsetAsync(h->flux_ptr(), 0, h->flux_elems() * sizeof(tally_t), h->stream));
    if ((h->target & MI3D_TARGET_HEAT) && h->heat_ptr()) HIPCHK(hipMemsetAsync(h->heat_ptr(), 0, h->heat_elems() * sizeof(double), h->stream));
    HIPCHK(hipMemsetAsync(h->d_counters.p, 0, MI3D_NCOUNTER * sizeof(unsigned long long), h->stream));
    if (h->d_bwd_capped.p) HIPCHK(hipMemsetAsync(h->d_bwd_capped.p, 0, sizeof(unsigned long long), h->stream));
    if (h->emis_weights) {
        const double ne = (double)h->nview * h->nxr * h->nyr * (double)h->wgt_ncell();
        if (h->wgt_ext) { if (h->backward() && ne <= kWgtMaxElems) HIPCHK(hipMemsetAsync(h->wgt_ext, 0, (size_t)ne * sizeof(double), h->stream)); }
        else if (h->wgt_n) HIPCHK(hipMemsetAsync(h->d_wgt_own.p, 0, h->wgt_n * sizeof(double), h->stream));
    }
    if (h->view_profiles) {
        const double ne = h->prf_elems();
        if (h->prf_ext) { if (h->sat_backward() && ne <= kPrfMaxElems) HIPCHK(hipMemsetAsync(h->prf_ext, 0, (size_t)ne * sizeof(double), h->stream)); }
        else if (h->prf_n) HIPCHK(hipMemsetAsync(h->d_prf_own.p, 0, h->prf_n * sizeof(double), h->stream));
    }
    if (h->pixel_errors) {
        if (h->err_ext) { if (h->backward()) HIPCHK(hipMemsetAsync(h->err_ext, 0, (size_t)h->nview * h->nxr * h->nyr * sizeof(double), h->stream)); }
        else if (h->err_n) HIPCHK(hipMemsetAsync(h->d_err_own.p, 0, h->err_n * sizeof(double), h->stream));
    }
    h->err_ran = false;
    // (the accumulation image is folded and zeroed at the end of a successful mi3d_run; a run that failed half way -- an event
    //  list ran full, a launch failed -- leaves its partial tallies there)
    if (h->d_rad_acc.p) HIPCHK(hipMemsetAsync(h->d_rad_acc.p, 0, h->d_rad_acc.cap * sizeof(tally_t), h->stream));
    if ((rc = drain_events(h))) return rc;
    for (auto &S : h->ev_slot) if (S.busy) S.cleared = true;   // (launches still on their way: their tallies are gone)
    h->kernel_ms = 0.0;
    h->launches = 0;
    return MI3D_OK;
}

// ---- launchers shared by mi3d_run and its pipelined form -------------------------------------------------------------------
// The photon order of a launch (mi3d_kernels.hip: k_bin_count, k_bin_scan, k_bin_scatter).  The blocks of the first and the third kernel
// own the same slabs of the indices; d_hist: [ntile][nblk] counts, then first slots, per tile and block, followed by the tiles' photons [ntile].
static hipError_t launch_bins(mi3d_solver *h, hipStream_t st, const BinGeom &G, int ntile, uint64_t seed, uint64_t off, uint64_t nb, uint32_t *order, uint32_t *cursor) {
    const unsigned nblk = (unsigned)std::min<uint64_t>((nb + 4095) / 4096, 4096);
    const uint32_t slab = (uint32_t)(((nb + nblk - 1) / nblk + 7) / 8 * 8);     // (a multiple of 8: the scatter reads tile[] 16 bytes at a time)
    uint32_t *bhist = h->d_hist.p, *hist = h->d_hist.p + (size_t)ntile * nblk;
    const size_t lds = bin_scatter_lds(ntile);
    if (lds > 65536 && lds > h->bin_lds_set) {     // (above 819 tiles; once per handle and size, not per launch)
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_bin_scatter), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return hipGetLastError();
        h->bin_lds_set = lds;
    }
    hipLaunchKernelGGL(k_bin_count, dim3(nblk), dim3(256), 0, st, G, seed, off, (uint32_t)nb, slab, h->d_tile.p, bhist);
    hipLaunchKernelGGL(k_bin_scan, dim3((unsigned)ntile), dim3(256), 0, st, (int)nblk, bhist, hist);
    hipLaunchKernelGGL(k_bin_scatter, dim3(nblk), dim3(256), lds, st, ntile, (uint32_t)nb, slab, h->d_tile.p, bhist, hist, cursor, order);
    return hipGetLastError();
}

// ---- the forward routes' builds: one selector per kernel family, one launch path ---------------------------------
// What a run fixes of its builds, stated once (plan_run): the instrumented build, the partial 3-D solver, k_transport's SRC (0 the sun,
// 1 thermal emission, 2 both) and the path-length estimator of the heating rates (k_transport_flux's HEST, kTargetHeatPath of the scene)
struct RunBuild { bool counting = false, p3d = false, hpath = false; int src = 0; };

using EntryFn = void (*)(EntryArgs, uint64_t, uint64_t, uint64_t, const uint32_t *, float4 *);
using LeanFn = void (*)(DevScene, uint64_t, uint64_t, uint64_t);
using RaysFn = void (*)(DevScene, uint64_t);
using GeneralFn = void (*)(DevScene, uint64_t, uint64_t, uint64_t, const DevThermal *);
using FluxFn = void (*)(DevScene, const TallyList *, uint64_t, uint64_t, uint64_t);
using TlRunsFn = void (*)(TallyList, RunGeom, tally_t *);
using TlScatterFn = void (*)(TallyList, tally_t *, unsigned, double *, unsigned);

// k_entry<EF> (mi3d_kernel_lean.hip): the build that writes long records or the one that writes short ones (entry_form)
static EntryFn entry_build(int form) { return form == kEntryF4Short ? k_entry<kEntryF4Short> : form == kEntryF4 ? k_entry<kEntryF4> : nullptr; }

// The builds of the lean loop that read short entry records (mi3d_kernel_lean.hip: k_transport_lean<., ., 0, 0, 256, kEntryF4Short>)
static bool lean_short_build(bool emit, int mix, int nt) { return !emit && mix == 0 && nt == 256; }

// k_transport_lean<C, P, MARCH, MIX, NT, EF> (mi3d_kernel_lean.hip), ten builds for each (C, P).  emit: MARCH 2, the loop that writes event
// records for k_rays; mix: 0 er3t's default scene, 1 a second 3-D constituent, 2 the general mixture (several 1-D constituents, tables), 3
// its common scene in the column view (plan_run: mix_lean); nt: threads per workgroup; short_rec: the run's entry records are short ones.
// Workgroups of 512 and mix 3 belong to the column view (never emit), and 512 to mix 2 and 3
static LeanFn lean_build(bool counting, bool p3d, bool emit, int mix, int nt, bool short_rec) {
    return with_flags([=](auto C, auto P) -> LeanFn {
        constexpr bool c = decltype(C)::value, p = decltype(P)::value;
        if (short_rec) return lean_short_build(emit, mix, nt) ? k_transport_lean<c, p, 0, 0, 256, kEntryF4Short> : nullptr;
        if (nt == 512 && !emit) return mix == 2 ? k_transport_lean<c, p, 0, 2, 512> : mix == 3 ? k_transport_lean<c, p, 0, 3, 512> : nullptr;
        if (nt != 256) return nullptr;
        switch (mix) {
        case 0: return emit ? k_transport_lean<c, p, 2, 0> : k_transport_lean<c, p, 0, 0>;
        case 1: return emit ? k_transport_lean<c, p, 2, 1> : k_transport_lean<c, p, 0, 1>;
        case 2: return emit ? k_transport_lean<c, p, 2, 2> : k_transport_lean<c, p, 0, 2>;
        case 3: return emit ? nullptr : k_transport_lean<c, p, 0, 3>;
        }
        return nullptr;
    }, counting, p3d);
}

// k_rays<C, P, HEAVY, CAM, PLAIN, THERM> (mi3d_kernel_rays.hip).  Satellite views: the light build, its form for scenes of analytic
// phase functions alone (plain) and the heavy one (reflections off LSRT / DSM surfaces), each for (C, P).  Cameras: the 3-D solver's
// build whose rays carry their own direction, and the one of a thermal job, each for C
static RaysFn rays_build(bool counting, bool p3d, bool heavy, bool camera, bool plain, bool thermal) {
    return with_flags([=](auto C, auto P) -> RaysFn {
        constexpr bool c = decltype(C)::value, p = decltype(P)::value;
        if (camera) {
            if (p || heavy || plain) return nullptr;
            return thermal ? k_rays<c, false, false, true, false, true> : k_rays<c, false, false, true>;
        }
        if (thermal || (heavy && plain)) return nullptr;
        return plain ? k_rays<c, p, false, false, true> : heavy ? k_rays<c, p, true, false, false> : k_rays<c, p, false, false, false>;
    }, counting, p3d);
}

// k_transport<C, MARCHK, F, P, SRC> (mi3d_kernels.hip).  march: 0 / 1 the photon loop without / with the rays of marched views inside it,
// every (C, F, P, SRC); 2 the thermal radiance builds of the 3-D solver that write event records for k_rays' thermal camera build
static GeneralFn general_build(bool counting, int march, bool flux, bool p3d, int src) {
    if (march < 0 || march > 2 || src < 0 || src > 2) return nullptr;
    if (march == 2) {
        if (flux || p3d || src != 1) return nullptr;
        return counting ? k_transport<true, 2, false, false, 1> : k_transport<false, 2, false, false, 1>;
    }
    return with_flags([=](auto C, auto M, auto F, auto P) -> GeneralFn {
        constexpr bool c = decltype(C)::value, f = decltype(F)::value, p = decltype(P)::value;
        constexpr int m = decltype(M)::value ? 1 : 0;
        return src == 2 ? k_transport<c, m, f, p, 2> : src == 1 ? k_transport<c, m, f, p, 1> : k_transport<c, m, f, p, 0>;
    }, counting, march == 1, flux, p3d);
}

// k_transport_flux<C, P, MIX, HEST> (mi3d_kernel_flux.hip): every combination.  mix: 0, 1, 2 as the lean loop's; hpath: the path-length
// estimator of the heating rates
static FluxFn flux_build(bool counting, bool p3d, int mix, bool hpath) {
    return with_flags([=](auto C, auto P, auto H) -> FluxFn {
        constexpr bool c = decltype(C)::value, p = decltype(P)::value, hp = decltype(H)::value;
        return mix == 0 ? k_transport_flux<c, p, 0, hp> : mix == 1 ? k_transport_flux<c, p, 1, hp> : mix == 2 ? k_transport_flux<c, p, 2, hp> : nullptr;
    }, counting, p3d, hpath);
}

// k_tl_runs<W, G, NTR> (mi3d_kernel_flux.hip).  write: the pass that writes the runs' records (the other counts them); hist_wg: one
// workgroup per workgroup of the photon loop, not per wave; wide: 512 threads, with hist_wg only
static TlRunsFn tl_runs_build(bool write, bool hist_wg, bool wide) {
    return with_flags([=](auto W) -> TlRunsFn {
        constexpr bool w = decltype(W)::value;
        if (!hist_wg) return wide ? nullptr : k_tl_runs<w, 1, 256>;
        return wide ? k_tl_runs<w, 4, 512> : k_tl_runs<w, 4, 256>;
    }, write);
}

// k_tl_scatter<NT, R, G> (mi3d_kernel_flux.hip): the sort of one wave's records, or (hist_wg) of a workgroup's in 64-KB tiles
static TlScatterFn tl_scatter_build(bool hist_wg) { return hist_wg ? k_tl_scatter<1024, 8, 4> : k_tl_scatter<MI3D_TLS_NT, MI3D_TLS_R, 1>; }

// The photons of a launch up to their first voxel walk (k_entry, mi3d_kernel_lean.hip); one photon per thread: the stream of records
// leaves at the rate a plain copy reaches.  form: the build that writes long records or the one that writes short ones (entry_form).
static hipError_t launch_entry(mi3d_solver *h, hipStream_t st, const DevScene &S, int form, uint64_t nb, uint64_t seed, uint64_t off, const uint32_t *order, float4 *entry) {
    const DevCold &C = h->cold_host;
    EntryArgs A;
    A.lay = C.lay;
    A.Lx = C.Lx; A.Ly = C.Ly; A.dx = S.dx; A.dy = S.dy; A.inv_dx = C.inv_dx; A.inv_dy = C.inv_dy; A.inv_nx = C.inv_nx; A.inv_ny = C.inv_ny;
    A.sdx = C.sdx; A.sdy = C.sdy; A.sdz = C.sdz; A.cos_cone = C.cos_cone;
    A.nx = S.nx; A.ny = S.ny; A.nz = S.nz; A.solver = S.solver; A.target = S.target; A.kdir = S.kdir;
    return launch_build(entry_build(form), (unsigned)((nb + 255) / 256), 256, 0, st, A, nb, seed, off, order, entry);
}

// The lean loop of a launch.  The build that reads short entry records where the run writes them: entry_form has asked lean_short_build,
// and a run that wrote short records for any other build finds none here
static hipError_t launch_lean(mi3d_solver *h, const RunBuild &B, hipStream_t st, const DevScene &S, bool emit, int mix, int nt, unsigned grid, size_t lds, uint64_t nb, uint64_t seed, uint64_t off) {
    return launch_build(lean_build(B.counting, B.p3d, emit, mix, nt, h->entry_form_run == kEntryF4Short), grid, (unsigned)nt, lds, st, S, nb, seed, off);
}

// The ray kernel behind the event-writing loops (LDS beyond 64 KB: staged tables behind the pools)
static hipError_t launch_rays(mi3d_solver *h, const RunBuild &B, hipStream_t st, const DevScene &S, bool heavy, size_t lds, uint64_t seed) {
    const bool camera = h->rad_kind == 1;   // cameras: the build whose rays carry their own direction (3-D solver: mi3d_run has checked)
    const bool thermal = camera && h->src_mtype == 3;   // (a thermal job's events: emissions among them)
    const bool plain = (S.target & kTargetPlainPhase) != 0 && !heavy && !camera;     // (the heavy build evaluates surface models only)
    const int waves = camera ? 4 : (h->rays_wg > 0 && !heavy) ? std::min(h->rays_wg, MI3D_RAYS_WAVES(B.counting, heavy)) : MI3D_RAYS_WAVES(B.counting, heavy);
    return launch_build(rays_build(B.counting, B.p3d, heavy, camera, plain, thermal), (unsigned)h->num_cu * (unsigned)waves, 256, lds, st, S, seed);
}

// The general photon loop (mi3d_kernels.hip): every job the lean loops do not serve, the thermal source's among them
// (emit: the thermal builds that write event records for k_rays instead of marching the rays of the cameras themselves, k_transport<.,2,...>)
static hipError_t launch_general(mi3d_solver *h, const RunBuild &B, hipStream_t st, const DevScene &S, int march, bool flux, unsigned grid, uint64_t nb, uint64_t seed, uint64_t off) {
    const int tb = 256;
    const size_t lds = (size_t)h->nz * sizeof(LayerRec) + MI3D_MAX_VIEW * sizeof(ViewRec) + sizeof(DevCold) + (size_t)9 * tb * sizeof(float) +
                       (size_t)(h->tab_n > 0 ? (1 + 2 * h->tab_n) * h->nang * sizeof(float) : 0);
    const DevThermal *th = B.src ? h->d_th.p : nullptr;
    return launch_build(general_build(B.counting, march, flux, B.p3d, B.src), grid, tb, lds, st, S, nb, seed, off, th);
}

// Photons a launch may have so that its events fit the lists, at `per_photon` events per photon (0: nothing known yet, a
// pilot).  A launch of a few million photons fills the lists of the XCDs in use evenly (twice the room asked for); a smaller one is
// taken by whichever workgroups start first, all on one XCD in the worst case: then ONE list must hold it.
static uint64_t photons_that_fit(uint64_t ev_cap, double per_photon, int n_xcd) {
    if (!(per_photon > 0.0)) return std::min<uint64_t>(16384, std::max<uint64_t>(ev_cap / 256, 16));   // pilot: room for 256 events per photon on one list
    const double even = 0.5 * n_xcd * (double)ev_cap / per_photon;
    return (uint64_t)(even >= 2.0e6 ? even : std::max(16.0, (double)ev_cap / (1.5 * per_photon)));
}

// The fill counters of a launch that has ended, as copied out in stream order (ev_note): how full the lists got sizes the
// launches still to come; a list that ran full has dropped events.  wait: also for launches still running.
static int ev_collect(mi3d_solver *h, bool wait) {
    for (int s = 0; s < kEvSlots; ++s) {
        mi3d_solver::EvSlot &S = h->ev_slot[s];
        if (!S.busy) continue;
        const hipError_t q = wait ? hipEventSynchronize(S.done) : hipEventQuery(S.done);
        if (q == hipErrorNotReady) continue;
        HIPCHK(q);
        S.busy = false;
        const unsigned long long *c = h->h_evctr + (size_t)s * 9 * kCtrStride;
        unsigned long long mx = 0, sum = 0;
        for (int x = 0; x < 8; ++x) { mx = std::max(mx, c[x * kCtrStride]); sum += c[x * kCtrStride]; }
        if ((c[8 * kCtrStride] != 0ull || mx > S.cap) && !S.cleared) {
            (void)sync_streams(h);   // what is still queued of this run ends; its counters are of no interest any more
            for (auto &T : h->ev_slot) T.busy = false;
            return fail(MI3D_ESTATE, "an event list of the marched views ran full (%llu events on one XCD from %llu photons, room for %llu): "
                                     "the tallies of this run are incomplete; call mi3d_reset and run it again (MI3D_KERNEL=generic needs no lists)",
                        mx, (unsigned long long)S.nb, (unsigned long long)S.cap);
        }
        // (records reserved, unused ones included: what the lists must hold)
        if (S.epoch == h->ev_epoch) h->ev_per_photon = std::max(0.5 * h->ev_per_photon, (double)sum / (double)S.nb);
    }
    return MI3D_OK;
}

// The launches of a run that has returned may still be on their way (mi3d_run does not wait for its last ones): whoever is about to
// look at the tallies -- mi3d_sync, the read-outs, the end of a statistics run -- settles them first.  A list that ran full fails
// THAT call: never silently short.
static int ev_settle(mi3d_solver *h) {
    for (const auto &S : h->ev_slot) if (S.busy) return ev_collect(h, true);
    return MI3D_OK;
}

// after the kernels of a launch: its fill counters go to a pinned slot (the next launch zeroes them on the device)
static int ev_note(mi3d_solver *h, uint64_t ev_cap, uint64_t nb, hipStream_t st, const unsigned long long *ctr) {
    int s = -1;
    for (int i = 0; i < kEvSlots; ++i) if (!h->ev_slot[i].busy) { s = i; break; }
    if (s < 0) { const int rc = ev_collect(h, true); if (rc) return rc; s = 0; }   // (every slot is on its way: wait for them)
    mi3d_solver::EvSlot &S = h->ev_slot[s];
    if (!S.done) HIPCHK(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    HIPCHK(hipMemcpyAsync(h->h_evctr + (size_t)s * 9 * kCtrStride, ctr, 9 * kCtrStride * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(S.done, st));
    S.busy = true; S.nb = nb; S.cap = ev_cap; S.cleared = false; S.epoch = h->ev_epoch;
    return MI3D_OK;
}

// the photon loop of a flux job and, with record lists, their sort (tset: the set of lists; two_streams: the sort on the sort stream)
static hipError_t launch_flux(mi3d_solver *h, const RunBuild &B, int tset, bool two_streams, const DevScene &S, const TallyList &TL0, int mix, unsigned grid, size_t lds, uint64_t nb, uint64_t seed, uint64_t off) {
    hipStream_t st = h->stream;
    mi3d_solver::TlSet &T = h->tl[tset];
    TallyList TL = TL0;
    TL.nwave = (int)grid * 4;   // (256-thread workgroups)
    TL.stats = (TL.cap && h->d_tl_stats.p) ? h->d_tl_stats.p + 4 * (h->launches % 64) : nullptr;
    // the photon loop reads the description from memory (one slot per launch in flight: the copy is asynchronous)
    static_assert(sizeof(TallyList) % 8 == 0, "TallyList slots");
    const int slot = (int)(h->launches % 64);
    // (the pinned copy of a slot is read by an ASYNCHRONOUS copy: a host that is 64 launches ahead of the device -- runs of dozens of small launches
    //  queued back to back -- must not overwrite it before that copy and the loop that reads the slot are through.  Until round 6 the host happened
    //  to wait every fourth launch for its record counters; without that wait launches read the description of launch + 64: another set of lists
    //  where one-stream and two-stream runs follow each other, test_record_sort_beside_the_next_photon_loop_changes_no_result[b2b_auto])
    if (h->tldesc_used[slot]) { const hipError_t ew = hipEventSynchronize(h->tldesc_ev[slot]); if (ew != hipSuccess) return ew; }
    std::memcpy(h->h_tldesc + (size_t)slot * sizeof(TallyList), &TL, sizeof(TallyList));
    hipError_t e0 = hipMemcpyAsync(h->d_tldesc.p + (size_t)slot * sizeof(TallyList), h->h_tldesc + (size_t)slot * sizeof(TallyList), sizeof(TallyList), hipMemcpyHostToDevice, st);
    if (e0 != hipSuccess) return e0;
    const TallyList *TLd = reinterpret_cast<const TallyList *>(h->d_tldesc.p + (size_t)slot * sizeof(TallyList));
    // (two sets of lists: the set is free once the sort of the launch that used it last is through it -- that launch's sums read the sorted
    //  copy and the bins' starts, which this photon loop does not touch: they may still run beside it)
    if (two_streams && T.used && (e0 = hipStreamWaitEvent(st, T.scattered, 0)) != hipSuccess) return e0;
    // (the sums of that launch, if they are still to come: here, on the main stream, between two photon loops -- they read the set's sorted copy
    //  and bins' starts, which this launch's sort writes again)
    if (T.pend.on && (e0 = launch_sum(h, tset, st)) != hipSuccess) return e0;
    // (the set's cursors: behind the wait -- the sort of the launch that used the set last writes one of them and copies them out on its stream)
    if (TL.cap && (e0 = hipMemsetAsync(TL.cursor, 0, 3 * sizeof(unsigned long long), st)) != hipSuccess) return e0;
    hipError_t err = launch_build(flux_build(B.counting, B.p3d, mix, B.hpath), grid, 256, lds, st, S, TLd, nb, seed, off);
    if (err == hipSuccess) {
        if (!h->tldesc_ev[slot]) err = hipEventCreateWithFlags(&h->tldesc_ev[slot], hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventRecord(h->tldesc_ev[slot], st);
        h->tldesc_used[slot] = (err == hipSuccess);
    }
    if (err != hipSuccess || TL.cap == 0) return err;
    if (two_streams) {   // (two sets of lists: the sort on its own stream, behind this photon loop)
        // The sums of the launch BEFORE this one (the other set), whose sort has run beside this photon loop: on the main stream straight behind
        // the loop, alone on the chip for the millisecond or two they take -- this launch's sort waits for them too (`filled` below), so it does
        // not take their CUs, and starts together with the next launch's photon loop, beside which it runs.  (Queued behind their own sort they
        // crept along in the loop's tails -- 13 ms for 1.6 ms of work -- and held up every sort behind them.)
        const int other = tset ^ 1;
        if (h->tl[other].pend.on) {
            if (h->tl[other].used && h->tl[other].scattered) err = hipStreamWaitEvent(st, h->tl[other].scattered, 0);
            if (err == hipSuccess) err = launch_sum(h, other, st);
            if (err != hipSuccess) return err;
        }
        err = hipEventRecord(T.filled, st);
        if (err == hipSuccess) err = hipStreamWaitEvent(h->tl_stream, T.filled, 0);
        if (err != hipSuccess) return err;
        st = h->tl_stream;
    }
    // the records of this launch: where every wave's share of every bin goes, counting sort, one LDS sum per bin
    double *heat = (h->target & MI3D_TARGET_HEAT) ? h->heat_ptr() : nullptr;
    // (round 6) the run records first: how many records of every bin each row's runs expand to -- the runs' rows of the histogram
    RunGeom Gm;
    Gm.lay = h->d_lay.p; Gm.ztoa = h->cold_host.ztoa; Gm.inv_dx = h->cold_host.inv_dx; Gm.inv_dy = h->cold_host.inv_dy;
    Gm.inv_nx = h->cold_host.inv_nx; Gm.inv_ny = h->cold_host.inv_ny; Gm.nz = h->nz; Gm.nx = h->nx; Gm.ny = h->ny; Gm.diag = h->d_counters.p;
    const size_t lds_runs = tl_runs_lds(TL.nbins, h->nz);
    // (large tables of bins: workgroups of 512 threads -- twice the waves on the same LDS)
    const bool hist_wg = TL.hist_wg != 0, runs_wide = hist_wg && lds_runs > 40960;
    const unsigned sort_grid = hist_wg ? (unsigned)TL.nwave / 4u : (unsigned)TL.nwave;   // (a workgroup of the sort per workgroup of the loop, or per wave)
    const unsigned nflux = (unsigned)h->flux_elems(), nheat = (unsigned)(heat ? h->heat_elems() : 0);
    if (TL.run_cap && (err = launch_build(tl_runs_build(false, hist_wg, runs_wide), sort_grid, runs_wide ? 512 : 256, lds_runs, st, TL, Gm, S.flux)) != hipSuccess) return err;
    hipLaunchKernelGGL(k_tl_wavescan<256>, dim3((unsigned)TL.nbins), dim3(256), 0, st, TL);
    hipLaunchKernelGGL(k_tl_prefix<256>, dim3(1), dim3(256), 0, st, TL);
    // One wave's records: workgroups of 256 threads with 16-KB tiles -- eight records per thread --, up to eight to a CU: 8.9e8 photons/s on the
    // 128 x 128 flux scene; 16 / 32 records per thread 8.7e8 / 6.7e8, 4: 8.5e8; 128 / 512 / 1024 threads 8.7e8 / 7.5e8 / 7.9e8:
    // profiles/r03/flux_records_experiments.log.
    // Tallies of more than 1024 bins (hist_wg): one workgroup of the sort per workgroup of the photon loop (four waves' chunk lists, one
    // histogram), 1024 threads and 64-KB tiles -- the tables over the bins (60 KB at 5000 bins) leave room for one workgroup per CU,
    // and every tile pays for a pass over them: 5.4e8 photons/s on 480 x 480 x 100 against 4.0e8 with 256 threads (atomics: 3.35e8)
    const size_t lds_sc = hist_wg ? ((size_t)3 * TL.nbins + 16 + 2 * kTlIds) * sizeof(uint32_t) + (size_t)8 * 1024 * sizeof(uint2)
                                  : ((size_t)4 * TL.nbins + 16 + 2 * kTlIds) * sizeof(uint32_t) + (size_t)MI3D_TLS_R * MI3D_TLS_NT * sizeof(uint2);
    if ((err = launch_build(tl_scatter_build(hist_wg), sort_grid, hist_wg ? 1024 : MI3D_TLS_NT, lds_sc, st, TL, S.flux, nflux, heat, nheat)) != hipSuccess) return err;
    // ... and the runs' records, level by level, behind each row's share of every bin
    if (TL.run_cap && (err = launch_build(tl_runs_build(true, hist_wg, runs_wide), sort_grid, runs_wide ? 512 : 256, lds_runs, st, TL, Gm, S.flux)) != hipSuccess) return err;
    if (two_streams && (err = hipEventRecord(T.scattered, st)) != hipSuccess) return err;
    const int split = std::max(1, std::min(64, (h->num_cu * 8) / TL.nbins));
    mi3d_solver::PendingSum &P = T.pend;
    P.on = true; P.TL = TL; P.flux = S.flux; P.nflux = nflux; P.heat = heat; P.nheat = nheat; P.split = split;
    // one stream: the sums straight behind the sort.  Two: they wait for the main stream's next pause -- the next launch of this set, or a join
    if (!two_streams) return launch_sum(h, tset, st);
    return hipGetLastError();
}

// Records reserved by the launches that have ended, as copied out in stream order (tl_note): they size the launches to come.
// A list that ran full has lost nothing (the tallies went out as atomics from there on), only speed.
static int tl_collect(mi3d_solver *h, bool wait) {
    for (int s = 0; s < kEvSlots; ++s) {
        mi3d_solver::TlSlot &S = h->tl_slot[s];
        if (!S.busy) continue;
        const hipError_t q = wait ? hipEventSynchronize(S.done) : hipEventQuery(S.done);
        if (q == hipErrorNotReady) continue;
        HIPCHK(q);
        S.busy = false;
        // ([0] records the loop reserved, [1] records in all with the runs expanded (k_tl_prefix), [2] run records reserved)
        auto upd = [&S](double &pp, unsigned long long got, uint64_t cap) {
            const double seen = (double)got / (double)S.nb;
            if (got > cap) pp = std::max(1.5 * pp, seen);   // ran full: what it needed is not known
            else pp = pp > 0.0 ? std::max(0.7 * pp, seen) : seen;
        };
        upd(h->tl_per_photon, h->h_tlctr[4 * s], S.cap);
        upd(h->tl_total_pp, h->h_tlctr[4 * s + 1], S.bcap);
        if (S.rcap) upd(h->tl_runs_pp, h->h_tlctr[4 * s + 2], S.rcap);
    }
    return MI3D_OK;
}

// (st: the stream behind whose work the counters are complete -- the sort stream where the sort runs on one of its own)
static int tl_note(mi3d_solver *h, uint64_t cap, uint64_t bcap, uint64_t rcap, uint64_t nb, const unsigned long long *cursor, hipStream_t st) {
    int s = -1;
    for (int i = 0; i < kEvSlots; ++i) if (!h->tl_slot[i].busy) { s = i; break; }
    if (s < 0) {
        // (every slot on its way: this launch's counters are not looked at -- the host does not wait here: the copies follow the SORT of their
        //  launch, and a host that waited for them could queue the next photon loop only when the sort before it was through, beside nothing)
        if (const int rc = tl_collect(h, false)) return rc;
        for (int i = 0; i < kEvSlots; ++i) if (!h->tl_slot[i].busy) { s = i; break; }
        if (s < 0) return MI3D_OK;
    }
    mi3d_solver::TlSlot &S = h->tl_slot[s];
    if (!S.done) HIPCHK(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    HIPCHK(hipMemcpyAsync(h->h_tlctr + 4 * s, cursor, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(S.done, st));
    S.busy = true; S.nb = nb; S.cap = cap; S.bcap = bcap; S.rcap = rcap;
    return MI3D_OK;
}

// Tile edge (in columns) of the photon order.  Two things pull in opposite directions (profiles/r02/tile_sweep_les480.log):
// the voxel records of a tile plus a margin of ten columns on every side (a photon wanders about a kilometre from where
// it enters the cloud) must fit an XCD's 4 MiB L2 with room to spare, counting the layers that are walked voxel by voxel;
// but the smaller the tile, the fewer cache lines of the radiance image take the tally atomics of the 41 000 photons an
// XCD has in flight, and float atomics to one line are served one after the other at the memory side (16-column tiles ran
// 17 % slower than 64-column ones at the same 84 % L2 hit rate).  So: as large as 3 MB of records allow, at most 64.
// Does the job keep a tally window (DevCold::tile_end ...)?  One predicate for the tile edge chosen here and for mi3d_run, which gives the
// kernel the LDS for it: the lean loop's column view of a satellite image with one pixel per column -- the build without marched views
// (k_transport_lean<.,.,0,.>), or the event-writing one when it is built with MI3D_LEAN_WIN_EMIT.  (mi3d_run adds what only it knows: the
// launch is sorted by tile, the lean loop serves the job.)
static bool window_wanted(const mi3d_solver *h) {
    return h->tally_window && !(h->target & MI3D_TARGET_FLUX) && h->rad_kind == 2 && h->kernel_choice == 0 && h->nview > 0 && h->nxr == h->nx && h->nyr == h->ny &&
           (h->nmarch == 0 || (MI3D_LEAN_WIN_EMIT && h->nmarch < h->nview));
}

static int choose_tile_cols(const mi3d_solver *h) {
    if (h->tile_cols >= 0) return h->tile_cols;
    if (h->nz3 <= 0 || h->n_step3d <= 0 || (long)h->nx * h->ny < 4096) return 0;   // nothing to gain: one tile
    // a tile's voxel records (16 bytes x the layers walked voxel by voxel) in three quarters of an XCD's 4 MiB L2, less a margin
    // of 20 columns.  Swept again in round 4 (profiles/r04/ab_tile_cols*.log): on the 480 x 480 scene 16 / 32 / 48 columns lose
    // 20 / 8 / 3 %, 240 lose 4 %, and between 60 and 120 the rates lie within what two processes with the same tile differ by (1.7 %).
    const double cols = std::sqrt(3.0e6 / (16.0 * h->n_step3d)) - 20.0;
    // (where the lean loop keeps its tally window -- a column view, one pixel per column -- a tile is narrower than the window by a
    //  margin: 40-56 columns 2.755e9 photons/s on the 480 x 480 scene against 2.725e9 at 64; ab_window_tile_cols.log)
    return (int)std::min(window_wanted(h) ? 48.0 : 64.0, std::max(24.0, cols));
}

// ---- mi3d_run: the route of a job, the room it needs, its launches -----------------------------------------------------------------

// The photon loop a job takes.  The lean kernels (mi3d_kernel_lean.hip): radiance only, satellite views (Column: the column table;
// ColumnRays: marched views and cameras, Rad_mrkind = 1 under the 3-D solver, through event lists and the ray kernel), at most two 3-D
// constituents, byte offsets of the voxel records within 32 bits.  The lean flux kernel (mi3d_kernel_flux.hip, Flux): flux / heating
// rates without radiance, the same scenes.  Everything else: the general loop, k_transport.
enum class Loop { General, Column, ColumnRays, Flux, Backward };

struct RunPlan {
    Loop loop = Loop::General;
    bool march = false, flux = false, thermal = false;
    RunBuild build;              // what the run fixes of its kernels' builds, for the launchers and name_route
    // builds of the lean loops (`mix`): 0 er3t's default scene -- one 1-D and one 3-D constituent, analytic phase functions --, 1 a second
    // 3-D constituent, 2 (round 5) the general mixture: several 1-D constituents and / or TABULATED phase functions, in 1-D layers
    // (func_ref_vs_cot's cloud slab, rtm/mca/util.py:153) or in voxels (the Mie branch as mca_atm.py:275-277 would write it).  mix_lean: the
    // column view's build, where the general mixture's common scene -- one Rayleigh 1-D constituent, one 3-D constituent with tables -- has
    // one of its own (3)
    int mix = 0, mix_lean = 0;
    size_t lds_tab = 0;          // the phase tables the scene refers to, staged in LDS by the lean kernels (mu, p, cdf, bucket indices)
    const char *why = nullptr;   // why the lean route was not taken (set where it was not, or where a camera job goes without the ray kernel)
    BinGeom G = {}; int ntile = 1; bool sorted = false;   // photon order: tiles of the domain (ntile 1: the launch runs in id order)
};

static RunPlan plan_run(const mi3d_solver *h, uint64_t nphoton) {
    RunPlan plan;
    plan.thermal = h->thermal();   // (a mixed job's photons start anywhere too: id order, the general loop)
    plan.build.counting = h->counting != 0;
    plan.build.p3d = h->solver == MI3D_SOLVER_P3D;
    plan.build.src = h->src_mtype == 3 ? 1 : h->src_mtype == 2 ? 2 : 0;
    plan.build.hpath = (h->target & MI3D_TARGET_HEAT) && h->heat_estimator == 1;   // (fill_scene: kTargetHeatPath)
    plan.march = (h->target & MI3D_TARGET_RADIANCE) && h->nmarch > 0;
    plan.flux = (h->target & MI3D_TARGET_FLUX) != 0;
    int tc = plan.thermal ? 0 : choose_tile_cols(h);   // (a thermal photon does not start at the top: id order)
    if (tc > 0) {
        while ((long)((h->nx + tc - 1) / tc) * ((h->ny + tc - 1) / tc) > kMaxTiles) tc *= 2;
        BinGeom &G = plan.G;
        G.Lx = (float)(h->dx * h->nx); G.Ly = (float)(h->dy * h->ny);
        G.inv_tx = (float)(1.0 / (h->dx * tc)); G.inv_ty = (float)(1.0 / (h->dy * tc));
        G.nx = h->nx; G.ny = h->ny; G.tcols = tc; G.ntx = (h->nx + tc - 1) / tc; G.nty = (h->ny + tc - 1) / tc;
        plan.ntile = G.ntx * G.nty;
    }
    plan.sorted = plan.ntile > 1 && nphoton >= 4096;

    bool gen = h->np1d > 1 || h->tab3d_hi >= 0, tabs = h->tab3d_hi >= 0;
    for (float a : h->apf1d) if (a >= 1.0f) { gen = true; tabs = true; }
    plan.mix = gen ? 2 : (h->np3d > 1 ? 1 : 0);
    // (tables that do not fit the LDS budget of fill_scene, or none loaded where a selector asks for one: the general kernel, which reads them from global memory)
    const bool tabs_ok = !tabs || h->tab_n > 0;
    plan.lds_tab = (gen && h->tab_n > 0) ? lean_tab_floats(h->nang, h->tab_n) * sizeof(float) : 0;
    const bool rad_job = (h->target & MI3D_TARGET_RADIANCE) && h->nview > 0;
    const bool vox32 = (double)h->ny * h->vrow_f4 * 16.0 < 4.0e9;
    const bool cells16 = h->nx < 65536 && h->ny < 65536 && h->nz < 65536;   // (cell numbers of the event records)
    const bool lean = !plan.thermal && h->kernel_choice == 0 && h->np3d <= 2 && tabs_ok && vox32;
    if (lean && plan.flux && !rad_job && h->nx < 65536 && h->ny < 65536 && h->nz < 65535) plan.loop = Loop::Flux;
    else if (lean && !plan.flux && h->nview > 0 && (plan.march ? cells16 && (h->rad_kind == 2 || h->solver == MI3D_SOLVER_3D) : h->rad_kind == 2))
        plan.loop = plan.march ? Loop::ColumnRays : Loop::Column;
    // Thermal cameras (Src_mtype = 3, Rad_mrkind = 1): where the lean loops' limits hold, the general loop's builds that write
    // event records, and k_rays' thermal camera build behind them -- the ColumnRays machinery with another photon loop in front
    if (h->src_mtype == 3 && h->kernel_choice == 0 && h->np3d <= 2 && tabs_ok && vox32 && !plan.flux && h->nview > 0 && plan.march && cells16 &&
        h->rad_kind == 1 && h->solver == MI3D_SOLVER_3D)
        plan.loop = Loop::ColumnRays;
    // Backward Monte Carlo for the cameras of a thermal job (mi3d_set_camera_method 1): a kernel of its own; what it does
    // not serve is refused by mi3d_run (backward_unsupported)
    if (h->cam_method == 1 || h->sat_backward()) plan.loop = Loop::Backward;
    plan.mix_lean = (plan.mix == 2 && plan.loop != Loop::ColumnRays && rayleigh_1d(h) && h->np3d == 1) ? 3 : plan.mix;
    if (plan.loop != Loop::Backward && (plan.loop == Loop::General || (h->rad_kind == 1 && plan.loop != Loop::ColumnRays)))
        plan.why = h->kernel_choice != 0 ? "kernel choice 1"
                   : h->rad_kind == 1 && h->solver != MI3D_SOLVER_3D ? "cameras are served under the 3-D solver only"
                   : plan.flux && rad_job ? "flux (or heating rates) TOGETHER with radiance: two jobs, one per target, as er3t's mcarats_ng submits them (mcarats.py:238-245), each take a lean loop"
                   : h->np3d > 2 ? "more than two 3-D constituents"
                   : !tabs_ok ? "phase tables too large for the LDS (or none loaded where a selector asks for one)"
                   : !vox32 ? "voxel records beyond 4 GB"
                   : plan.march && !cells16 ? "cell numbers beyond the event records' 16 bits"
                   : "a scene the lean photon loops do not serve";
    return plan;
}

// Cameras in the cyclic domain: the periodic images of a camera are served by the ray kernel's camera build.  A camera job that cannot
// use it (plan.why), asked for explicitly ("cam_images" > 0), is refused; left to the default (-1) it runs with the nearest image alone and
// says so.
static int cam_fallback(mi3d_solver *h, const char *why) {
    if (h->cam_images > 0)
        return fail(MI3D_EUNSUP, "cam_images=%d: the periodic images of a camera are served by the ray kernel only, and this job cannot use it (%s)", h->cam_images, why);
    if (h->cam_images < 0 && !h->cam_warned) {
        fprintf(stderr, "Warning [mi3d_run]: this camera job cannot use the ray kernel (%s): the NEAREST periodic image of the camera alone is served -- "
                        "lines of sight that leave the domain sideways miss what its continuation adds (set \"cam_images\" to 0 to say so yourself).\n", why);
        h->cam_warned = true;
    }
    return MI3D_OK;
}

// The route's name (mi3d_last_kernel) and, once per handle, the warning of a job that was not sent to the general loop by its caller
// (mi3d_set_kernel 1) but landed there: the loop of round 1 serves it correctly and at a fraction of the lean loops' speed (bench.py's
// `general_kernel` leg has the figure).  Thermal jobs take the general loop by design.
static void name_route(mi3d_solver *h, const RunPlan &plan, bool lists, uint64_t nphoton) {
    const int c = plan.build.counting ? 1 : 0, p3d = plan.build.p3d ? 1 : 0;
    char nm[96];
    const bool hpath = plan.build.hpath;
    if (plan.loop == Loop::Backward && h->col_backward())
        snprintf(nm, sizeof(nm), h->sun_backward() ? (h->pixel_errors ? "k_backward<%d,V,I,N,S> [solar+thermal]" : "k_backward<%d,V,I,N> [solar+thermal]")
                                 : h->pixel_errors ? "k_backward<%d,V,I,S> [thermal]" : h->view_profiles ? "k_backward<%d,V,I,P> [thermal]" : "k_backward<%d,V,I> [thermal]", c);
    else if (plan.loop == Loop::Backward && h->sun_backward()) snprintf(nm, sizeof(nm), h->pixel_errors ? "k_backward<%d,V,N,S> [solar+thermal]" : "k_backward<%d,V,N> [solar+thermal]", c);
    else if (plan.loop == Loop::Backward && h->sat_backward() && h->pixel_errors) snprintf(nm, sizeof(nm), "k_backward<%d,V,S> [thermal]", c);
    else if (plan.loop == Loop::Backward && h->pixel_errors) snprintf(nm, sizeof(nm), "k_backward<%d,S> [thermal]", c);
    else if (plan.loop == Loop::Backward && h->sat_backward() && h->view_profiles) snprintf(nm, sizeof(nm), "k_backward<%d,V,P> [thermal]", c);
    else if (plan.loop == Loop::Backward && h->sat_backward()) snprintf(nm, sizeof(nm), "k_backward<%d,V> [thermal]", c);
    else if (plan.loop == Loop::Backward && h->emis_weights) snprintf(nm, sizeof(nm), "k_backward<%d,W> [thermal]", c);
    else if (plan.loop == Loop::Backward) snprintf(nm, sizeof(nm), "k_backward<%d> [thermal]", c);
    else if (plan.loop == Loop::Flux && hpath) snprintf(nm, sizeof(nm), lists ? "k_transport_flux<%d,%d,%d,1> + k_tl_scatter + k_tl_sum" : "k_transport_flux<%d,%d,%d,1>", c, p3d, plan.mix);
    else if (plan.loop == Loop::Flux) snprintf(nm, sizeof(nm), lists ? "k_transport_flux<%d,%d,%d> + k_tl_scatter + k_tl_sum" : "k_transport_flux<%d,%d,%d>", c, p3d, plan.mix);
    else if (plan.loop == Loop::ColumnRays && plan.thermal) snprintf(nm, sizeof(nm), "k_transport<%d,2,0,0> [thermal] + k_rays", c);
    else if (plan.loop == Loop::ColumnRays) snprintf(nm, sizeof(nm), "k_transport_lean<%d,%d,2,%d> + k_rays", c, p3d, plan.mix_lean);
    else if (plan.loop == Loop::Column) snprintf(nm, sizeof(nm), "k_transport_lean<%d,%d,0,%d>", c, p3d, plan.mix_lean);
    else if (plan.build.src == 2) snprintf(nm, sizeof(nm), hpath ? "k_transport<%d,%d,%d,%d> [solar+thermal] [heating: path length]" : "k_transport<%d,%d,%d,%d> [solar+thermal]", c, plan.march ? 1 : 0, plan.flux ? 1 : 0, p3d);
    else snprintf(nm, sizeof(nm), plan.thermal ? (hpath ? "k_transport<%d,%d,%d,%d> [thermal] [heating: path length]" : "k_transport<%d,%d,%d,%d> [thermal]") : hpath ? "k_transport<%d,%d,%d,%d> [heating: path length]" : "k_transport<%d,%d,%d,%d>", c, plan.march ? 1 : 0, plan.flux ? 1 : 0, p3d);
    h->last_kernel = nm;
    if (plan.loop == Loop::General && h->kernel_choice == 0 && !h->general_warned && nphoton >= 4096 && !plan.thermal) {
        fprintf(stderr, "Warning [mi3d_run]: this job runs on the general photon loop (k_transport), not on a lean one: %s.  Same results, a third to a half of the speed.\n", plan.why);
        h->general_warned = true;
    }
}

static bool new_event(hipEvent_t &e) { return e || hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess; }
static size_t free_bytes(size_t unknown) { size_t f = 0, t = 0; if (hipMemGetInfo(&f, &t) == hipSuccess) return f; (void)hipGetLastError(); return unknown; }

// Tally records per photon with a margin: records in all (what the sorted copy holds), records the loop writes one by one, run records.
// Nothing known yet: a record per level and a half, every one of them written by the loop, a run for every kRunMin of them.
struct TlRates { double tpp, dpp, rpp; };
static TlRates tl_rates(const mi3d_solver *h, bool runs) {
    // (the path-length estimator of the heating rates: a record per cell and layer flown through beside the one per level -- twice the guess)
    const double guess = ((h->target & MI3D_TARGET_HEAT) && h->heat_estimator == 1 ? 3.0 : 1.5) * (h->nz + 1);
    const double tpp = h->tl_total_pp > 0.0 ? 1.15 * h->tl_total_pp : (h->tl_per_photon > 0.0 && !runs ? 1.15 * h->tl_per_photon : guess);
    return {tpp, h->tl_per_photon > 0.0 ? 1.15 * h->tl_per_photon : tpp, !runs ? 0.0 : h->tl_runs_pp > 0.0 ? 1.15 * h->tl_runs_pp + 0.05 : tpp / kRunMin};
}

// The compact histogram of a workgroup of the photon loop (hist_wg, with run records): the bins of the levels around the layers that are
// walked voxel by voxel, for the three planes and the heating cells -- merged where they touch; without run records: all bins
static void tl_compact_hist(const mi3d_solver *h, TallyList &T) {
    const int nbins = T.nbins, shift = T.shift;
    T.run_min = kRunMin;
    for (int r = 0; r < 4; ++r) { T.cb_lo[r] = 1; T.cb_hi[r] = 0; T.cb_off[r] = 0; }
    T.cb_lo[0] = 0; T.cb_hi[0] = nbins - 1; T.ncb = nbins;
    int ks_lo = h->nz, ks_hi = -1;
    for (int kq = 0; kq < h->nz && kq < (int)h->lay_host.size(); ++kq) if (h->lay_host[kq].flags & kLayStep3d) { ks_lo = std::min(ks_lo, kq); ks_hi = std::max(ks_hi, kq); }
    if (!T.hist_wg || !T.run_cap || ks_hi < ks_lo) return;
    const size_t ncol_ = (size_t)h->nx * h->ny, nlev_ = (size_t)h->nz + 1, nflux_ = 3 * nlev_ * ncol_;
    std::vector<std::pair<int, int>> rg;
    for (size_t pl = 0; pl < 3; ++pl) rg.emplace_back((int)(((pl * nlev_ + ks_lo) * ncol_) >> shift), (int)((((pl * nlev_ + ks_hi + 2) * ncol_) - 1) >> shift));
    // (the path-length estimator leaves records in the heating cells of EVERY layer, the uniform ones too: all of their bins)
    if ((h->target & MI3D_TARGET_HEAT) && h->heat_estimator == 1) rg.emplace_back((int)(nflux_ >> shift), nbins - 1);
    else if (h->target & MI3D_TARGET_HEAT) rg.emplace_back((int)((nflux_ + (size_t)ks_lo * ncol_) >> shift), (int)((nflux_ + ((size_t)ks_hi + 1) * ncol_ - 1) >> shift));
    std::sort(rg.begin(), rg.end());
    std::vector<std::pair<int, int>> mg;
    for (auto &q : rg) { if (!mg.empty() && q.first <= mg.back().second + 1) mg.back().second = std::max(mg.back().second, q.second); else mg.push_back(q); }
    int off = 0;   // (at least one range: the ones after it stay unused)
    for (size_t r = 0; r < 4 && r < mg.size(); ++r) { T.cb_lo[r] = mg[r].first; T.cb_hi[r] = std::min(mg[r].second, nbins - 1); T.cb_off[r] = off; off += T.cb_hi[r] - T.cb_lo[r] + 1; }
    T.ncb = std::max(off, 1);
    T.run_min = 1;
}

// A set's buffers in the description of its lists (the sizes are in T already): the words are chunk fills, the waves' chunk lists, the
// rows of the histograms, bin starts, then the same for the run records
static void tl_lay_out(TallyList &T, const mi3d_solver::TlSet &S) {
    const size_t nwave = (size_t)T.nwave, nrow = (size_t)tl_nrow(T);
    T.rec = S.rec.p; T.binned = S.binned.p; T.cursor = S.cursor.p;
    T.runs = T.run_cap ? S.runs.p : nullptr;
    T.chunk_fill = S.words.p;
    T.wave_chunks = T.chunk_fill + T.cap / kTlChunk; T.wave_nchunk = T.wave_chunks + nwave * T.wcap;
    T.whist = T.wave_nchunk + nwave; T.wbase = T.whist + nrow * T.nbins;
    T.hist = T.wbase + nrow * T.nbins; T.bin_start = T.hist + T.nbins;
    T.run_fill = T.bin_start + T.nbins + 1; T.run_chunks = T.run_fill + T.run_cap / kRunChunk; T.run_nchunk = T.run_chunks + nwave * T.run_wcap;
}

// Tally records instead of atomics: bins of 2^shift tally cells, as many as one workgroup can sum in LDS in float64; the record lists
// of nset sets take what launches of nb_max photons need at the records per photon seen so far, at most 2^31 records and a quarter of the
// memory that is free (two lists of 8 bytes per record).  Not for tallies of more than 8192 bins (134 million tally cells).  Returns the
// records a list holds and the sets' descriptions in TL; 0: no lists (TL as it was).
static uint64_t size_tally_lists(mi3d_solver *h, uint64_t nb_max, int nset, TallyList TL[2]) {
    TallyList T = {};
    T.shift = 10;
    while (T.shift < 14 && ((size_t)16 << T.shift) <= (size_t)h->lds_max) ++T.shift;
    const size_t ncell = h->flux_elems() + ((h->target & MI3D_TARGET_HEAT) ? h->heat_elems() : 0);   // (heating-rate cells follow the flux cells)
    if ((double)ncell > 4.0e9) return 0;
    T.nbins = (int)((ncell + ((size_t)1 << T.shift) - 1) >> T.shift);
    if (T.nbins > 8192 || ((size_t)3 * T.nbins + 16 + 2 * kTlIds) * sizeof(uint32_t) + (size_t)8 * 1024 * sizeof(uint2) > (size_t)h->lds_max) return 0;
    T.hist_wg = T.nbins > 1024 ? 1 : 0;   // (four histograms per workgroup of the photon loop would not fit its LDS any more)
    const bool runs = h->tally_runs != 0 && h->nz <= 1022;   // (a run record holds its first level and its count in ten bits each)
    size_t free_b = free_bytes((size_t)8 << 30);
    for (const auto &S : h->tl) free_b += (S.rec.cap + S.binned.cap) * sizeof(uint2) + S.runs.cap * sizeof(float4);
    const TlRates r = tl_rates(h, runs);
    const uint64_t waves = (uint64_t)h->num_cu * MI3D_FLUX_WAVES(h->counting != 0) * 4;
    const uint64_t lim = ((uint64_t)1 << h->tl_cap_log2) - kTlChunk;
    // the lists in all: a quarter of the memory that is free (the sorted copy once, records and runs once per set)
    const double nb = std::min((double)nb_max, 0.25 * (double)free_b / (nset * (8.0 * r.tpp + 8.0 * r.dpp + 32.0 * r.rpp)));
    auto cap_of = [nb, waves, lim](double pp, uint64_t chunk, uint64_t have, double item_bytes) -> uint64_t {
        uint64_t c = (uint64_t)(pp * nb) + (waves + 1) * chunk;
        // (lists only grow, and by a quarter at least: the rates per photon creep upwards by a per cent from launch to launch, and every
        //  step of a list that is not at its limit would free and allocate gigabytes -- seen as one run in three taking seconds.
        //  A LARGE list that is near enough stays where it is: a launch more per run costs less than moving sixteen gigabytes.  A small one
        //  moves: er3t's jobs of a few million photons come by the dozen, one size, and a list 30 % short made two launches of every one
        //  of them -- 7.3 instead of 5.6 ms per job of 6e6 photons, profiles/r06/small_flux_jobs_one_launch.log)
        if (have > 0 && (double)have >= (double)c) c = have;
        else if (have > 0 && (double)have >= 0.7 * (double)c && (double)have * item_bytes >= 1.6e10) c = have;
        else if (c > have && have > 0) c = std::max<uint64_t>(c, have + have / 4);
        c = std::min<uint64_t>(c, lim);
        c = std::max<uint64_t>(c, std::min<uint64_t>(have, lim));
        return c / chunk * chunk;
    };
    const mi3d_solver::TlSet &S0 = h->tl[0];
    const uint64_t want_cap = cap_of(r.dpp, kTlChunk, S0.rec.cap, 8.0 * nset);
    const uint64_t want_bcap = cap_of(r.tpp, kTlChunk, S0.binned.cap, 8.0 * nset);
    const uint64_t want_rcap = runs ? std::max<uint64_t>(cap_of(r.rpp, kRunChunk, S0.runs.cap / 2, 32.0 * nset), 64 * kRunChunk) : 0;
    if (want_cap < 64 * kTlChunk) return 0;
    T.cap = (unsigned)want_cap; T.bcap = (unsigned)want_bcap; T.run_cap = (unsigned)want_rcap;
    T.nwave = (int)waves;
    T.wcap = (int)std::max<size_t>(64, 4 * (size_t)(want_cap / kTlChunk) / waves);
    T.run_wcap = runs ? (int)std::max<size_t>(64, 4 * (size_t)(want_rcap / kRunChunk) / waves) : 0;
    const size_t nrow = (size_t)tl_nrow(T);
    const size_t nwords = (size_t)(want_cap / kTlChunk) + waves * T.wcap + waves + 2 * nrow * T.nbins + 2 * (size_t)T.nbins + 1 +
                          (runs ? (size_t)(want_rcap / kRunChunk) + waves * T.run_wcap + waves : 0);
    // (a list that moves: nothing may still be on its way that reads the old one -- launches, sorts, and the sums that are kept back for the main
    //  stream's next pause, whose description holds the old pointers: everything joined and waited for first)
    bool moves = false;
    for (int q = 0; q < nset; ++q) moves = moves || want_cap > h->tl[q].rec.cap || want_bcap > h->tl[q].binned.cap || nwords > h->tl[q].words.cap || 2 * want_rcap > h->tl[q].runs.cap;
    if (moves && sync_streams(h) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int rc = MI3D_OK;
    for (int q = 0; q < nset && !rc; ++q) {
        mi3d_solver::TlSet &S = h->tl[q];
        rc = S.rec.alloc(want_cap);
        if (!rc) rc = S.binned.alloc(want_bcap);
        if (!rc) rc = S.words.alloc(nwords);
        if (!rc) rc = S.cursor.alloc(kCtrStride);
        if (!rc && q == 0) rc = h->d_tl_stats.alloc(64 * 4);
        if (!rc && runs) rc = S.runs.alloc(2 * want_rcap);
    }
    if (!rc && !h->h_tlctr && hipHostMalloc((void **)&h->h_tlctr, (size_t)4 * kEvSlots * sizeof(unsigned long long)) != hipSuccess) rc = MI3D_EDEVICE;
    if (rc) {
        (void)hipGetLastError();
        for (auto &S : h->tl) S.release();
        fprintf(stderr, "Warning [mi3d_run]: no device memory for the tally-record lists of this flux job (%.1f GB free); an atomic per level crossing instead (same results, slower).\n", (double)free_b / 1.0e9);
        return 0;
    }
    tl_compact_hist(h, T);
    // (each set: lists, counters, cursor and sorted copy of its own)
    for (int q = 0; q < 2; ++q) { TL[q] = T; tl_lay_out(TL[q], h->tl[q < nset ? q : 0]); }
    return want_cap;
}

// Capacity of each XCD's event list.  Nothing known about the scene yet: room for a pilot launch.  A short run: room for every
// event of the run on ONE list (64 per photon: the workgroups that start first take most of its photons).  A long one: what
// the run's events need at the number per photon seen so far, twice over (the lists fill unevenly), at most 2^ev_cap_log2
// records -- and never more than a quarter of the memory that is free now (other handles, a host framework and smaller parts
// share the device).  Lists only grow (mi3d_set_tuning "evcap_log2" and a job without marched views release them).  Returns the
// capacity, with cold_host pointing at set 0's lists (0: no room).
static uint64_t size_ev_lists(mi3d_solver *h, uint64_t nphoton, bool two_sets) {
    const double per_rec = (double)kEvBlockF4 * 16.0 / 64.0 + (h->sfc_lambert_only ? 0.0 : 8.0);
    size_t free_b = free_bytes((size_t)8 << 30);
    for (const auto &E : h->ev) free_b += E.events.cap * sizeof(float4) + E.hvlist.cap * sizeof(unsigned long long);   // (what this handle holds already is reused)
    const int nset = two_sets ? 2 : 1;
    const uint64_t cap_mem = (uint64_t)(0.25 * (double)free_b / (8.0 * per_rec * nset));
    const uint64_t cap_max = (uint64_t)1 << h->ev_cap_log2;
    uint64_t want_cap = std::min<uint64_t>(cap_max, 64 * nphoton + 65536);
    if (h->ev_per_photon > 0.0)
        want_cap = std::min<uint64_t>(want_cap, std::max<uint64_t>((uint64_t)(4.0 * h->ev_per_photon * (double)nphoton / h->n_xcd), 65536));
    else want_cap = std::min<uint64_t>(want_cap, (uint64_t)1 << 22);
    want_cap = std::max<uint64_t>(want_cap, std::min<uint64_t>(h->ev[0].events.cap / ((size_t)8 * kEvBlockF4) * 64, cap_max));
    want_cap = std::min<uint64_t>(want_cap, cap_mem);
    want_cap &= ~(uint64_t)63;      // (the records stand in blocks of 64: ev_index)
    // (an allocation that fails although the device reported the room -- fragmentation, another process -- is tried again at half the
    //  size: launches are sized to the lists, so small lists cost launches, not results; below 65 536 records per list: the general kernel)
    int r = MI3D_OK;
    for (;;) {
        r = want_cap < 65536 ? fail(MI3D_EDEVICE, "no memory for event lists") : MI3D_OK;
        for (int q = 0; q < nset && !r; ++q) {
            mi3d_solver::EvSet &E = h->ev[q];
            r = E.events.alloc((size_t)8 * ev_list_f4(want_cap));
            if (!r) r = E.evctr.alloc(kCtrWords * kCtrStride);
            if (!r && !h->sfc_lambert_only) r = E.hvlist.alloc((size_t)8 * want_cap);
        }
        if (!r && !h->h_evctr && hipHostMalloc((void **)&h->h_evctr, (size_t)kEvSlots * 9 * kCtrStride * sizeof(unsigned long long)) != hipSuccess) r = MI3D_EDEVICE;
        if (!r || want_cap < 65536) break;
        (void)hipGetLastError();
        for (auto &E : h->ev) E.release();
        want_cap = (want_cap / 2) & ~(uint64_t)63;
    }
    if (r) {
        (void)hipGetLastError();
        fprintf(stderr, "Warning [mi3d_run]: no device memory for the event lists of the marched views (%.1f GB free); the general kernel marches them inside its photon loop (same results, slower).\n", (double)free_b / 1.0e9);
        return 0;
    }
    h->cold_host.ev_list = h->ev[0].events.p; h->cold_host.ev_ctr = h->ev[0].evctr.p; h->cold_host.ev_cap = (int)want_cap;
    h->cold_host.hv_list = h->sfc_lambert_only ? nullptr : h->ev[0].hvlist.p;
    return want_cap;
}

// Entry records (k_entry, mi3d_kernel_lean.hip): the lean loop's builds without rays inside them take new photons where their
// first voxel walk begins.  48 bytes per photon of a launch (32 in the short form), never more than half of the memory that is free:
// without them (no room, "entry_records" 0) the photons are launched inside the loop as before.  Points cold_host at the records and
// notes their form in h->entry_form_run.
// The form (mi3d_device.h): short where direction and pz are the same for every photon of the launch and the loop's build can do
// without them -- a solar source without a cone from above, served by the column-view build of er3t's default scene
// (lean_short_build; MIX 0 is never run in workgroups of 512) -- unless "entry_records" 2 asks for the long form everywhere.
static int entry_form(const mi3d_solver *h, const RunPlan &plan) {
    const DevCold &C = h->cold_host;
    const bool launch_ok = C.cos_cone >= 1.0f && C.sdz < 0.0f && !plan.thermal && !h->thermal();
    const bool build_ok = plan.loop == Loop::Column && lean_short_build(false, plan.mix_lean, 256);
    return (h->entry_records == 1 && launch_ok && build_ok) ? kEntryF4Short : kEntryF4;
}

static bool use_entry_records(mi3d_solver *h, const RunPlan &plan, uint64_t nphoton) {
    h->entry_form_run = 0;
#if MI3D_LEAN_FAST
    // (the path-length estimator of the heating rates tallies the first flight too: its photons are launched inside the loop)
    if (plan.build.hpath) return false;
    if (plan.loop == Loop::General || plan.thermal || !h->entry_records || h->nx >= 65536 || h->ny >= 65536 || h->nz >= 32768) return false;
    DevBuf<float4> &E = h->pre[0].entry;
    const int form = entry_form(h, plan);
    const size_t need = entry_f4((size_t)std::min<uint64_t>(nphoton, h->batch), form);
    size_t free_b = free_bytes((size_t)8 << 30);
    free_b += E.cap * sizeof(float4);
    if (need > E.cap && need * sizeof(float4) > free_b / 2) return false;
    if (E.alloc(need) == MI3D_OK) { h->cold_host.entry = E.p; h->entry_form_run = form; return true; }
    (void)hipGetLastError();
#endif
    return false;
}

// The pre-pass of a launch (photon order, entry records) on a stream of its own beside the photon loop of the launch before: a second set
// of what it writes.  (Not together with the second set of event lists of "overlap_rays": one spare DevCold.)
// Where the loop leaves room on a CU: the flux loop (four waves per SIMD) and the event-writing loop of jobs with marched views (+4 % for a flux
// run alone, +2.6 % with nine views).  The column / tally-window loop holds six waves per SIMD and most of the LDS: there the pre-pass only finds
// room in the loop's tail, and what runs beside it costs the loop more than it saves (-4 % on the 480 x 480 nadir bench, -3 % on 128 x 128:
// profiles/r05/ab_overlap_pre.log; -4 % on a stream of its own of the lowest priority, profiles/r06/ab_pre_nadir_priority.log).
// A run of a few million photons that is read before the next one has no loop before it to hide behind and pays for the hop between the streams.
// Returns whether the run uses the second set ("overlap_pre" 2: whatever the run).
static bool pre_second_set(mi3d_solver *h, const RunPlan &plan, bool use_entry, bool two_sets, uint64_t nphoton) {
    mi3d_solver::PreSet &P0 = h->pre[0], &P1 = h->pre[1];
    bool two = h->overlap_pre && !two_sets && (plan.sorted || use_entry) && (plan.loop == Loop::Flux || plan.loop == Loop::ColumnRays) &&
               (h->overlap_pre > 1 || nphoton >= ((uint64_t)1 << 22) || h->runs_unread > 0);
    if (two && !h->pre_stream && hipStreamCreateWithFlags(&h->pre_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); two = false; }
    for (auto &S : h->pre) two = two && new_event(S.done) && new_event(S.loop);
    if (two && plan.sorted && (P1.order.alloc(P0.order.cap) != MI3D_OK || P1.cursor.alloc(kMaxTiles) != MI3D_OK)) { (void)hipGetLastError(); two = false; }
    if (two && use_entry && P1.entry.cap < P0.entry.cap) {   // (a second set of the same size, where half of the free memory holds it)
        const size_t free_b = free_bytes(0) + P1.entry.cap * sizeof(float4);
        if (P0.entry.cap * sizeof(float4) > free_b / 2 || P1.entry.alloc(P0.entry.cap) != MI3D_OK) { (void)hipGetLastError(); two = false; }
    }
    // (a job that does not use the second set gives back what is large: a hipFree waits for the device -- not for every small job)
    if (!two && (P1.entry.cap * sizeof(float4) + P1.order.cap * sizeof(uint32_t)) > ((size_t)256 << 20)) P1.release();
    return two;
}

// The tally window of the lean loop (DevCold::tile_end ...): for the column view of a satellite image with one pixel per column,
// when the launch is worked through tile by tile.  Its place relative to a tile: where the direct beam that enters the top of
// the atmosphere above the tile reaches the height of the clouds, centred.
static void set_tally_window(mi3d_solver *h, const RunPlan &plan) {
    DevCold &C = h->cold_host;
    C.tile_end = nullptr; C.win_tc = 0; C.win_ntx = 0; C.win_ntile = 0; C.win_off = 0u;
    if (!(plan.loop == Loop::Column || plan.loop == Loop::ColumnRays) || !window_wanted(h) || !plan.sorted || h->nx >= 32768 || h->ny >= 32768 ||
        h->nx < kWin || h->ny < kWin || !(h->z_cloud >= 0.0) || !(C.sdz < 0.0f))
        return;
    const double ztoa = h->zgrd[h->nz];
    // (under the independent-pixel approximation a photon never leaves the column it was launched above)
    const double way = h->solver == MI3D_SOLVER_IPA ? 0.0 : (ztoa - h->z_cloud) / std::fabs((double)C.sdz);
    const int tcols = plan.G.tcols;
    const int margin = (kWin - std::min(tcols, kWin)) / 2 - std::max(0, tcols - kWin) / 2;   // (a tile wider than the window: its middle)
    auto wrap = [](long v, int n) { v %= n; if (v < 0) v += n; return (unsigned)v; };
    // (the centring was checked by moving the window about: ±12 columns change the share of the tallies it catches by less than a
    //  point, ±24 cost ten -- profiles/r04/win_offset_probe.log)
    const unsigned ox = wrap(std::lround(C.sdx * way / h->dx) - margin, h->nx);
    const unsigned oy = wrap(std::lround(C.sdy * way / h->dy) - margin, h->ny);
    C.tile_end = h->pre[0].cursor.p;   // (the tiles' ends: each pre-pass set's cursors, upload_cold)
    C.win_tc = tcols; C.win_ntx = plan.G.ntx; C.win_ntile = plan.ntile;
    C.win_off = ox | (oy << 16);
}

// Radiance tallies go to an accumulation image with one pixel per 128-byte line and are folded into the tally buffer (the
// library's own or the caller's) after the last launch of this call -- where the tallies are atomics from the photon loop itself
// ("rad_spread" -1, the default).  Not where the ray kernel makes them (marched views, cameras): its tallies spread over the images
// of several views or a wide camera image, and the compact image (8 bytes per pixel: 1.8 MB per view on the 480 x 480 scene, at home
// in the L2s) serves them better than 29 MB per view -- nine views 2.83 -> 3.11e8 photons/s, the camera +1 %
// (profiles/r04/ab_rad_line_density.log).  With the tally window either image does (2.79 / 2.78e9): the accumulation image stays.
// Rows of the accumulation image an ODD number of 4 KiB pages apart (32 pixels of kRadLine * 8 bytes a page).  The atomics of an
// XCD go to the pixels of one tile of columns, a few rows of which are busy at any time; with rows a multiple of four pages
// apart they meet in a few of the L2's sixteen channels: 128 pixels per row (4 pages) 1.93e9 photons/s against 2.47e9 at 5 pages
// and 2.52 at 4.5; 256 (8 pages) 1.63 against 2.25 at 9; 64 pixels padded to 4 pages 1.19 against 2.5; 512 (16) 2.11 against 2.25
// at 17.  Odd page counts came within 2 % of the best stride on every size tried (192 ... 512 pixels: 7, 9, 11, 13, 15, 17
// pages); half pages are good on some sizes and the worst choice on others (15.5 and 16.5 pages: 1.96 and 2.00 against 2.28).
// profiles/r04/stride_probe4.log ... stride_probe6.log, ab_rad_row_pad*.log; tools/stride_probe*.py
// rad_row: pixels per row of the image the run tallies into (0: none, the tally buffer itself)
static int rad_acc_image(mi3d_solver *h, const RunPlan &plan, DevScene &S, int &rad_row) {
    rad_row = 0;
    const int row = h->rad_row_pad >= 0 ? h->nxr + h->rad_row_pad : 32 * (((h->nxr + 31) / 32) | 1);
    const size_t acc_elems = (size_t)h->nview * h->nyr * row;
    // (the point radiometers of a thermal job, DESIGN.md §5.10: sixteen one-pixel images are ONE 128-byte line of the compact image, and the ray
    //  kernel's atomics to it run one after the other -- spread they are sixteen lines: 1.87 -> 6.63e7 photons/s for sixteen sensors on 128 x 128,
    //  profiles/r10/spread_probe.log)
    const bool few_pixels = plan.thermal && h->rad_kind == 1 && (size_t)h->nview * h->nyr * h->nxr <= 1024;
    const bool spread = (h->target & MI3D_TARGET_RADIANCE) && h->nview > 0 && h->rad_spread != 0 && !(h->rad_spread < 0 && plan.loop == Loop::ColumnRays && !few_pixels) &&
                        (double)acc_elems * kRadLine * sizeof(tally_t) <= 1.0e9 && (double)acc_elems * kRadLine < 2147483647.0;
    if (!spread) return MI3D_OK;
    const size_t need = acc_elems * kRadLine;
    if (h->d_rad_acc.cap < need || !h->d_rad_acc.p) {
        int rc = h->d_rad_acc.alloc(need);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(h->d_rad_acc.p, 0, need * sizeof(tally_t), h->stream));
    }
    S.rad = h->d_rad_acc.p; S.rad_stride = kRadLine; S.rad_row = row;
    rad_row = row;
    return MI3D_OK;
}

// Photons of the next launch (per: those of the last one, in and out).  Equal launches (a short last one would be mostly tail).  With
// k_rays a launch is as many photons as the event lists hold at the number of events per photon seen so far (twice the room: the lists
// fill unevenly); with tally-record lists as many as the lists hold at the records per photon seen so far.
static int launch_photons(mi3d_solver *h, const RunPlan &plan, uint64_t ev_cap, const TallyList &TL, bool tl_two, uint64_t nphoton, uint64_t done, uint64_t &per) {
    const uint64_t left = nphoton - done;
    int rc;
    if (plan.loop == Loop::ColumnRays) {
        if ((rc = ev_collect(h, false))) return rc;
        const uint64_t room = photons_that_fit(ev_cap, h->ev_per_photon, h->n_xcd);
        const uint64_t want_n = std::max<uint64_t>(std::min<uint64_t>(room, h->batch), 64);
        const uint64_t nl = (left + want_n - 1) / want_n;
        per = (left + nl - 1) / nl;
    }
    if (TL.cap) {
        if ((rc = tl_collect(h, false))) return rc;
        const uint64_t waves = (uint64_t)h->num_cu * MI3D_FLUX_WAVES(h->counting != 0) * 4;
        // (what each of the three lists holds at its rate per photon seen so far: the loop's records, the sorted copy, the run records)
        auto room_of = [waves](uint64_t cap_, uint64_t chunk, double pp_) -> uint64_t {
            return (uint64_t)((double)(cap_ > 2 * waves * chunk ? cap_ - waves * chunk : cap_ / 2) / pp_);
        };
        const TlRates r = tl_rates(h, TL.run_cap != 0);
        uint64_t room = std::min(room_of(TL.cap, kTlChunk, r.dpp), room_of(TL.bcap, kTlChunk, r.tpp));
        if (TL.run_cap) room = std::min(room, room_of(TL.run_cap, kRunChunk, r.rpp));
        const uint64_t want_n = std::max<uint64_t>(std::min<uint64_t>(room, h->batch), 4096);
        uint64_t nl = (left + want_n - 1) / want_n;
        // (the sort beside the next photon loop: a run in tl_split launches at least, of eight million photons or more -- all but the last sort are hidden)
        if (tl_two && done == 0) nl = std::max<uint64_t>(nl, std::min<uint64_t>((uint64_t)h->tl_split, nphoton >> 23));
        else if (tl_two) nl = std::max<uint64_t>(nl, std::min<uint64_t>((left + per - 1) / std::max<uint64_t>(per, 1), (uint64_t)h->tl_split));
        nl = std::max<uint64_t>(nl, 1);
        per = (left + nl - 1) / nl;
    }
    return MI3D_OK;
}

// The column-view loop of a launch (set: its event lists) and, with marched views, the ray kernels of the events it has written: on their
// own stream rs beside the next launch's photon loop where there are two sets
static hipError_t launch_column(mi3d_solver *h, const RunPlan &plan, const DevScene &Sl, int set, bool two_sets, hipStream_t rs, unsigned grid, uint64_t nb, uint64_t seed, uint64_t off) {
    const bool split = plan.loop == Loop::ColumnRays, counting = plan.build.counting;
    mi3d_solver::EvSet &E = h->ev[set];
    const size_t lds_col = (size_t)(h->nz + 2) * sizeof(LayerRec) + MI3D_MAX_VIEW * sizeof(ViewRec) + sizeof(DevCold);   // (+2: the lean loop's end records)
    const int emit_wg = counting ? 4 : (h->emit_wg > 0 ? std::min(h->emit_wg, MI3D_LEAN_EMIT_GRID) : MI3D_LEAN_EMIT_GRID);
    const unsigned gridp = split ? (unsigned)std::min<uint64_t>((nb + 255) / 256, (uint64_t)h->num_cu * emit_wg) : grid;
    DevScene Sx = Sl;
    if (set) Sx.cold = h->d_cold.p + 1;       // (this launch's set of event lists)
    hipError_t err = hipSuccess;
    // (the set is free once the ray kernels of the launch that used it last are through it)
    if (two_sets && E.used) err = hipStreamWaitEvent(h->stream, E.rays, 0);
    if (err == hipSuccess && split) err = hipMemsetAsync(E.evctr.p, 0, kCtrWords * kCtrStride * sizeof(unsigned long long), h->stream);
    if (err == hipSuccess && plan.thermal) err = launch_general(h, plan.build, h->stream, Sx, 2, false, gridp, nb, seed, off);   // (thermal cameras: the general loop writes the records)
    else if (err == hipSuccess) {
        // (the general mixture with staged tables AND a tally window: three workgroups of 512 threads keep six waves per SIMD where
        //  six of 256 would not find the LDS)
        const size_t lds_lean = lds_col + (h->cold_host.tile_end ? kWinLds : 0) + plan.lds_tab;
        const bool wide = plan.mix >= 2 && !split && !counting && lds_lean * 3 <= (size_t)160 * 1024 && lds_lean * 6 > (size_t)160 * 1024;
        unsigned gridw = wide ? (unsigned)std::min<uint64_t>((nb + 511) / 512, (uint64_t)h->num_cu * 3) : gridp;
        // (the general mixture in workgroups of 256: as many as its registers -- five waves per SIMD -- and its LDS let a CU hold)
        if (plan.mix >= 2 && !wide && !split && !counting) gridw = std::min<unsigned>(gridw, (unsigned)h->num_cu * (unsigned)std::max<size_t>(1, std::min<size_t>(MI3D_GEN_NARROW_WAVES, ((size_t)160 * 1024) / lds_lean)));
        err = launch_lean(h, plan.build, h->stream, Sx, split, plan.mix_lean, wide ? 512 : 256, gridw, lds_lean, nb, seed, off);
    }
    if (err != hipSuccess || !split) return err;
    if (two_sets) {
        err = hipEventRecord(E.emit, h->stream);
        if (err == hipSuccess) err = hipStreamWaitEvent(rs, E.emit, 0);
    }
    const bool plain_scene = (Sl.target & kTargetPlainPhase) != 0 && h->rad_kind != 1;
    if (err == hipSuccess) err = launch_rays(h, plan.build, rs, Sx, false, lds_col + rays_lds_extra(h->nz, h->rad_kind == 1) + (plain_scene ? 0 : plan.lds_tab), seed);
    if (err == hipSuccess && !h->sfc_lambert_only && h->rad_kind != 1)   // the reflections off LSRT / DSM surfaces it left aside
        err = launch_rays(h, plan.build, rs, Sx, true, lds_col + rays_lds_extra(h->nz) + plan.lds_tab, seed);
    return err;
}

// The flux loop's tally-record lists (TL; tl_two: a second set, sorted on a stream of its own beside the next photon loop) and the LDS its
// workgroups take (lds_fl)
static int flux_lists(mi3d_solver *h, const RunPlan &plan, uint64_t nphoton, TallyList TL[2], bool &tl_two, size_t &lds_fl) {
    int rc;
    if ((rc = h->d_tldesc.alloc((size_t)64 * sizeof(TallyList)))) return rc;
    if (!h->h_tldesc && hipHostMalloc((void **)&h->h_tldesc, (size_t)64 * sizeof(TallyList)) != hipSuccess) return fail(MI3D_EDEVICE, "no pinned memory for the tally-list descriptions");
    // Two streams pay where something runs beside the sort: a run long enough for four launches of eight million photons (a run of 4e7 alone: +7 %;
    // 1e7 / 2e7 in two or three launches: -2.5 %, tools/small_runs.py), or a run that follows another whose tallies nobody has looked at in between
    // (runs queued back to back: +19 % at 5e6 photons a run).  A small run whose tallies are read before the next one -- er3t's jobs of a few
    // million photons, one by one -- only pays for the launches' tails and the hops between the streams: one stream ("overlap_sort" 2: two
    // streams whatever the run).
    tl_two = h->overlap_sort != 0 && (h->overlap_sort == 2 || nphoton >= ((uint64_t)1 << 25) || h->runs_unread > 0);
    // (the stream and its events only where they are used: every stream more of a process shares the device's few hardware queues with the
    //  others -- two handles that each kept an idle sort stream ran their jobs 12 % slower side by side, tools/time_dropin.py)
    if (tl_two && !h->tl_stream && hipStreamCreateWithFlags(&h->tl_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); tl_two = false; }
    for (auto &T : h->tl) tl_two = tl_two && new_event(T.filled) && new_event(T.sorted) && new_event(T.scattered);
    // (nothing known about the scene's records per photon: lists for a pilot launch of two million photons -- sized by the guess "a record and a half
    //  per level, a run for every three" they would take tens of gigabytes -- and the right size after it, below.  Not for short runs: the sort has
    //  a fixed cost)
    const bool tl_pilot = !(h->tl_total_pp > 0.0) && nphoton > ((uint64_t)1 << 21);
    lds_fl = (size_t)(h->nz + 2) * sizeof(LayerRec) + sizeof(DevCold);
    if (h->tally_lists && nphoton >= 4096 && size_tally_lists(h, tl_pilot ? (uint64_t)1 << 21 : std::min<uint64_t>(nphoton, h->batch), tl_two ? 2 : 1, TL))
        lds_fl += TL[0].hist_wg ? ((size_t)TL[0].ncb + 3) / 4 * 16 : (size_t)TL[0].nbins * 16;   // (a histogram per wave, or one for the workgroup)
    lds_fl += (size_t)4 * 128 * sizeof(float4) + (size_t)4 * kTlStage * sizeof(uint2);   // the waves' run records and staged tallies
    lds_fl += plan.lds_tab;                                                              // ... and the phase tables behind them
    if (!TL[0].cap) tl_two = false;
    // (one stream after runs on two: the shared sorted copy and the first set of lists are free once the sorts before are through)
    if (!tl_two && TL[0].cap) HIPCHK(tl_join(h));
    return MI3D_OK;
}

// The event lists of a job with marched views (ev_cap: the records of each; two_sets: a second set, the ray kernels on a stream of their own
// beside the next launch's photon loop).  No room for them: the general loop serves the job
static int event_lists(mi3d_solver *h, RunPlan &plan, uint64_t nphoton, uint64_t &ev_cap, bool &two_sets) {
    if (plan.loop == Loop::ColumnRays) {
        two_sets = h->overlap_rays != 0;
        if (two_sets && !h->rays_stream && hipStreamCreateWithFlags(&h->rays_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); two_sets = false; }
        for (auto &E : h->ev) two_sets = two_sets && new_event(E.emit) && new_event(E.rays);
        if (!(ev_cap = size_ev_lists(h, nphoton, two_sets))) {
            // no room for the lists: the general kernel marches the rays inside its photon loop instead (same results, slower) -- except for
            // a camera that was to see its periodic images: the general kernel serves the nearest one only
            for (auto &E : h->ev) E.release();
            plan.loop = Loop::General; plan.why = "no device memory for its event lists"; two_sets = false;
            if (h->rad_kind == 1) {
                if (h->cam_images > 0) return fail(MI3D_EDEVICE, "no device memory for the event lists of a camera job with cam_images=%d (the general kernel serves the nearest image only)", h->cam_images);
                return cam_fallback(h, plan.why);
            }
        }
    } else if (h->ev[0].events.p) {   // this job needs no lists: what an earlier one held goes back to the device
        HIPCHK(sync_streams(h));
        for (auto &E : h->ev) E.release();
    }
    return MI3D_OK;
}

// The pre-pass of a launch: its photon order and entry records, into set pset (with two sets on the pre-pass stream, behind the photon loop
// that read the set last and beside the one that is running)
static hipError_t launch_pre(mi3d_solver *h, const RunPlan &plan, int pset, bool pre_two, bool pre_track, bool use_entry, const DevScene &S, uint64_t nb, uint64_t seed, uint64_t off) {
    mi3d_solver::PreSet &PS = h->pre[pset];
    hipStream_t const ps = pre_two ? h->pre_stream : h->stream;
    hipError_t eb = hipSuccess;
    // (set pset is free once the photon loop of the launch that read it last is through -- whichever stream arrangement that launch
    //  had: a one-stream launch records set 0's loop event too, below -- and the histogram / tile scratch the two sets share once the last
    //  pre-pass on the main stream is: ADVICE r5, a two-stream run queued straight behind a one-stream run)
    if (pre_two && PS.used) eb = hipStreamWaitEvent(ps, PS.loop, 0);
    if (eb == hipSuccess && pre_two && h->pre_main_used) { eb = hipStreamWaitEvent(ps, h->pre_main, 0); h->pre_main_used = false; }
    if (eb == hipSuccess && plan.sorted) eb = launch_bins(h, ps, plan.G, plan.ntile, seed, off, nb, PS.order.p, PS.cursor.p);
    if (eb == hipSuccess && use_entry)   // the photons of this launch up to their first voxel walk
        eb = launch_entry(h, ps, S, h->entry_form_run, nb, seed, off, plan.sorted ? (const uint32_t *)PS.order.p : (const uint32_t *)nullptr, PS.entry.p);
    if (eb == hipSuccess && pre_two) eb = hipEventRecord(PS.done, ps);
    if (eb == hipSuccess && pre_track && !pre_two) {
        if (!h->pre_main) eb = hipEventCreateWithFlags(&h->pre_main, hipEventDisableTiming);
        if (eb == hipSuccess) { eb = hipEventRecord(h->pre_main, h->stream); h->pre_main_used = true; }
    }
    if (eb == hipSuccess && pre_two) eb = hipStreamWaitEvent(h->stream, PS.done, 0);
    return eb;
}

// ---- the backward route (mi3d_set_camera_method 1; mi3d_kernel_backward.hip) ------------------------------------
// What it serves: Src_mtype = 3, a radiance job of the 3-D solver over Lambertian surfaces.  The switch of the cameras
// (mi3d_set_camera_method 1) serves cameras and point radiometers (Rad_mrkind = 1), with or without emission weights; the switch of the
// satellite views (sat: mi3d_set_view_method 1) the views of mi3d_set_views (Rad_mrkind = 2), without them.
// With mi3d_set_view_sunlight 1 the satellite views' route serves Src_mtype = 2 instead, and nothing else.
// With mi3d_set_view_columns 1 it serves independent columns and partial 3-D instead of the 3-D solver.
// Everything else: MI3D_EUNSUP, with the reason.
static int backward_unsupported(const mi3d_solver *h, bool sat) {
    if (h->view_columns) {
        // the satellite views under independent columns and partial 3-D (mi3d_set_view_columns 1, Rad_mvcol=1)
        const char *no = h->rad_kind != 2 ? "cameras and point radiometers (Rad_mrkind=1): a camera's lines of sight fan out over the columns, the switch belongs to the satellite views (Rad_mrkind=2)"
                         : !sat || h->view_method != 1 ? "mi3d_set_view_method 0 or mi3d_set_camera_method 1 (it needs Rad_mvbwd=1): the switch belongs to the backward route for satellite views"
                         : h->solver == MI3D_SOLVER_3D ? "the 3-D solver: the switch belongs to independent columns and partial 3-D (solver 2 / 1), run the 3-D job without it"
                         : h->emis_weights ? "emission weights (mi3d_set_emission_weights 1): an image times the cells is out of its scope"
                         : nullptr;
        if (no) return fail(MI3D_EUNSUP, "the column histories of the backward satellite views (mi3d_set_view_columns 1, Rad_mvcol=1) do not serve %s", no);
    }
    if (h->view_sunlight) {
        // the sunlight term (mi3d_set_view_sunlight 1, Rad_mvsun=1) belongs to the satellite views of a solar+thermal job
        const char *no = h->src_mtype == 1 ? "a solar job (Src_mtype=1): the switch belongs to the mixed source, a pure solar image is a solar+thermal job with a cold atmosphere"
                         : h->src_mtype == 3 ? "a thermal job (Src_mtype=3): there is no sun, run it without the switch"
                         : h->rad_kind != 2 ? "cameras and point radiometers (Rad_mrkind=1): the term belongs to the satellite views (Rad_mrkind=2)"
                         : !sat || h->view_method != 1 ? "mi3d_set_view_method 0 or mi3d_set_camera_method 1 (it needs Rad_mvbwd=1): the term belongs to the backward route for satellite views"
                         : h->view_profiles ? "view profiles (mi3d_set_view_profiles 1): the weighting functions are per unit Planck radiance, and the sun has no row"
                         : h->emis_weights ? "emission weights (mi3d_set_emission_weights 1): the sun is no cell"
                         : !(h->src_the - 0.5 * std::max(h->src_qmax, 0.0) > 90.0) ? "a sun from below or on the horizon (Src_the - Src_qmax / 2 <= 90)"
                         : nullptr;
        if (no) return fail(MI3D_EUNSUP, "the sunlight term of the backward satellite views (mi3d_set_view_sunlight 1, Rad_mvsun=1) does not serve %s", no);
    }
    const char *why = h->src_mtype == 1 ? "a solar job (Src_mtype=1): the sun needs a local estimate of its own"
                      : h->src_mtype == 2 && !h->view_sunlight ? "a solar+thermal job (Src_mtype=2): the sun needs a local estimate of its own (satellite views have one: mi3d_set_view_sunlight 1, Rad_mvsun=1)"
                      : !(h->target & MI3D_TARGET_RADIANCE) || (h->target & MI3D_TARGET_FLUX) ? (sat ? "a flux or heating-rate job: the route serves radiance (satellite images) alone"
                                                                                                      : "a flux or heating-rate job: the route serves radiance (cameras) alone")
                      : h->rad_kind != (sat ? 2 : 1) ? (sat ? "cameras and point radiometers (Rad_mrkind=1): their switch is mi3d_set_camera_method (Rad_mbwd)"
                                                            : "satellite views (Rad_mrkind=2): the route serves cameras and point radiometers (Rad_mrkind=1)")
                      : h->solver != MI3D_SOLVER_3D && !(sat && h->view_columns) ? (sat ? "independent columns or partial 3-D: a line of sight crosses columns, it needs the 3-D solver"
                                                           : "independent columns or partial 3-D: cameras need the 3-D solver")
                      : !h->sfc_lambert_only ? "a non-Lambertian surface (only Lambertian surfaces emit)"
                      : sat && h->emis_weights ? "emission weights (mi3d_set_emission_weights 1): an image times the cells is out of its scope"
                      : nullptr;
    if (why)
        return fail(MI3D_EUNSUP, sat ? "backward Monte Carlo for satellite views (mi3d_set_view_method 1, Rad_mvbwd=1) does not serve %s"
                                     : "backward Monte Carlo (mi3d_set_camera_method 1) does not serve %s", why);
    return MI3D_OK;
}

static int fill_backward(mi3d_solver *h, DevBackward &A, bool sat) {
    std::memset(&A, 0, sizeof(A));
    const double Lx = h->dx * h->nx, Ly = h->dy * h->ny;
    const bool sfc2d = !h->sfc2d_host.empty();
    A.nx = h->nx; A.ny = h->ny; A.nz = h->nz; A.nz3 = h->nz3; A.k3lo = h->nz3 > 0 ? h->iz3l - 1 : 0; A.np1d = h->np1d; A.np3d = h->np3d;
    A.nxb = sfc2d ? h->nxb : 1; A.nyb = sfc2d ? h->nyb : 1;
    A.nview = h->nview; A.nxr = h->nxr; A.nyr = h->nyr;
    A.cam_mode = sat ? 0 : kCamPoint | (h->cam_mpmap == 2 ? kCamRect : 0) | (h->cam_mrproj == 1 ? kCamCos : 0);
    A.dx = (float)h->dx; A.dy = (float)h->dy; A.inv_dx = (float)(1.0 / h->dx); A.inv_dy = (float)(1.0 / h->dy);
    A.ztoa = (float)h->zgrd[h->nz];
    A.sfc_sx = (float)(A.nxb / Lx); A.sfc_sy = (float)(A.nyb / Ly);
    A.wmin = (float)h->wmin; A.wfac = (float)h->wfac; A.src_flx = (float)h->src_flx;
    A.nvox = (unsigned)((size_t)h->nx * h->ny * h->nz3); A.vcol_f4 = h->vcol_f4; A.vrow_f4 = h->vrow_f4;
    A.lay = h->d_lay.p; A.vrec = h->d_vrec.p; A.csca = h->d_csca.p; A.cells = h->d_bwd_cells.p;
    A.cams = sat ? nullptr : h->d_cams.p;          // (the views travel in BwdSat)
    A.tab.tmu = h->d_tmu.p; A.tab.tp = h->d_tp.p; A.tab.tcdf = h->d_tcdf.p; A.tab.nang = h->nang; A.tab.npf = h->npf;
    A.rad = h->rad_ptr(); A.counters = h->d_counters.p; A.capped = h->d_bwd_capped.p;
    for (int iv = 0; iv < h->nview; ++iv) {
        if (sat && !(std::cos(h->view_the[iv] * 3.14159265358979323846 / 180.0) < 0.0)) continue;   // (an up-looking view's plane is raised to the surface)
        if (!(h->view_zloc[iv] > h->zgrd[0]))
            return fail(MI3D_EINVAL, sat ? "backward Monte Carlo: the sensor plane of view %d lies on or below the surface (Rad_zloc=%g, surface at %g)"
                                         : "backward Monte Carlo: sensor %d stands on or below the surface (Rad_zloc=%g, surface at %g)", iv + 1, h->view_zloc[iv], h->zgrd[0]);
    }
    if ((double)h->nview * h->nxr * h->nyr > 2147483647.0) return fail(MI3D_EUNSUP, "image too large for the 32-bit pixel numbers of the backward kernel");
    return MI3D_OK;
}

// What k_backward_v receives beside DevBackward
static void fill_backward_views(const mi3d_solver *h, BwdSat &S, float *start_out) {
    const double Lx = h->dx * h->nx, Ly = h->dy * h->ny;
    std::memset(&S, 0, sizeof(S));
    S.views = h->d_views.p;
    S.pix_dx = (float)(Lx / h->nxr); S.pix_dy = (float)(Ly / h->nyr);
    S.Lx = (float)Lx; S.Ly = (float)Ly; S.inv_Lx = (float)(1.0 / Lx); S.inv_Ly = (float)(1.0 / Ly);
    S.jch = h->bwd_chunk < 0 ? kBwdChunkAuto : h->bwd_chunk;
    S.start_out = start_out;
}

// What the builds with sunlight receive beside that (mi3d_set_view_sunlight 1): the sun of fill_scene
static void fill_backward_sun(const mi3d_solver *h, BwdSun &N) {
    const double pi = 3.14159265358979323846, th = h->src_the * pi / 180.0, ph = h->src_phi * pi / 180.0;
    std::memset(&N, 0, sizeof(N));
    N.sdx = (float)(std::sin(th) * std::cos(ph)); N.sdy = (float)(std::sin(th) * std::sin(ph)); N.sdz = (float)std::cos(th);
    N.mu0 = std::fabs(N.sdz);
    N.F = (float)h->src_fsol;
    N.cos_cone = h->src_qmax <= 0.0 ? 1.0f : (float)std::cos(0.5 * h->src_qmax * pi / 180.0);
    N.ray3d = h->solver == MI3D_SOLVER_P3D ? 1 : 0;      // (read by the column builds alone: the direct beam of partial 3-D flies in 3-D)
}

// The one place that names the builds of the histories: the kernel of (route, counting, debug), as the runtime takes it for a launch and
// for an occupancy query.  The weights, profiles and errors builds have no debug form (nullptr); the debug forms do not count
static const void *backward_build(BwdRoute route, bool counting, bool debug) {
    switch (route) {
    case BwdRoute::Camera:
        if (debug) return (const void *)k_backward<false, true>;
        return counting ? (const void *)k_backward<true, false> : (const void *)k_backward<false, false>;
    case BwdRoute::Weights:
        if (debug) return nullptr;
        return counting ? (const void *)k_backward_w<true> : (const void *)k_backward_w<false>;
    case BwdRoute::Views:
        if (debug) return (const void *)k_backward_v<false, true>;
        return counting ? (const void *)k_backward_v<true, false> : (const void *)k_backward_v<false, false>;
    case BwdRoute::Profiles:
        if (debug) return nullptr;
        return counting ? (const void *)k_backward_vp<true> : (const void *)k_backward_vp<false>;
    case BwdRoute::CameraErrors:
        if (debug) return nullptr;
        return counting ? (const void *)k_backward_s<true> : (const void *)k_backward_s<false>;
    case BwdRoute::ViewsErrors:
        if (debug) return nullptr;
        return counting ? (const void *)k_backward_vs<true> : (const void *)k_backward_vs<false>;
    case BwdRoute::ViewsSun:
        if (debug) return (const void *)k_backward_vn<false, true>;
        return counting ? (const void *)k_backward_vn<true, false> : (const void *)k_backward_vn<false, false>;
    case BwdRoute::ViewsSunErrors:
        if (debug) return nullptr;
        return counting ? (const void *)k_backward_vns<true> : (const void *)k_backward_vns<false>;
    case BwdRoute::Columns:
        if (debug) return (const void *)k_backward_vc<false, true>;
        return counting ? (const void *)k_backward_vc<true, false> : (const void *)k_backward_vc<false, false>;
    case BwdRoute::ColumnsErrors:
        if (debug) return nullptr;
        return counting ? (const void *)k_backward_vcs<true> : (const void *)k_backward_vcs<false>;
    case BwdRoute::ColumnsProfiles:
        if (debug) return nullptr;
        return counting ? (const void *)k_backward_vcp<true> : (const void *)k_backward_vcp<false>;
    case BwdRoute::ColumnsSun:
        if (debug) return (const void *)k_backward_vcn<false, true>;
        return counting ? (const void *)k_backward_vcn<true, false> : (const void *)k_backward_vcn<false, false>;
    case BwdRoute::ColumnsSunErrors:
        if (debug) return nullptr;
        return counting ? (const void *)k_backward_vcns<true> : (const void *)k_backward_vcns<false>;
    }
    return nullptr;
}

// One launch.  The kernel arguments in the order of the entry points: (A, seed, id0, n), then (dir_out, score_out) for the cameras,
// (W) for the weights build, (dir_out, score_out, S) for the views, (S, P) for the views' profiles build, (E) and (S, E) for the cameras'
// and the views' errors builds, (dir_out, score_out, S, N) and (S, E, N) for the views with sunlight; a column build takes the arguments of
// the views' build it stands for
static hipError_t backward_launch(BwdRoute route, bool counting, bool debug, unsigned grid, size_t lds, hipStream_t stream, DevBackward A, uint64_t seed,
                                  uint64_t id0, uint64_t n, float *dir_out, double *score_out, BwdWeights W, BwdSat S, BwdProfiles P,
                                  BwdErrors E = BwdErrors{}, BwdSun N = BwdSun{}) {
    const void *kernel = backward_build(route, counting, debug);
    if (!kernel) return hipErrorInvalidValue;
    void *cam[] = {&A, &seed, &id0, &n, &dir_out, &score_out}, *wgt[] = {&A, &seed, &id0, &n, &W}, *sat[] = {&A, &seed, &id0, &n, &dir_out, &score_out, &S},
         *prf[] = {&A, &seed, &id0, &n, &S, &P}, *cerr[] = {&A, &seed, &id0, &n, &E}, *verr[] = {&A, &seed, &id0, &n, &S, &E},
         *vsun[] = {&A, &seed, &id0, &n, &dir_out, &score_out, &S, &N}, *vsune[] = {&A, &seed, &id0, &n, &S, &E, &N};
    return hipLaunchKernel(kernel, dim3(grid), dim3(256),
                           route == BwdRoute::Camera ? cam : route == BwdRoute::Weights ? wgt : route == BwdRoute::Views || route == BwdRoute::Columns ? sat
                           : route == BwdRoute::Profiles || route == BwdRoute::ColumnsProfiles ? prf : route == BwdRoute::CameraErrors ? cerr
                           : route == BwdRoute::ViewsErrors || route == BwdRoute::ColumnsErrors ? verr
                           : route == BwdRoute::ViewsSun || route == BwdRoute::ColumnsSun ? vsun : vsune, lds, stream);
}

// Workgroups of the build that are resident on the device at once.  The weights, view, profiles and errors builds ask the runtime, once per (route, LDS
// bytes, counting).  The camera build takes five waves per SIMD, four in the counting build (the register report in DESIGN.md §5.11),
// the grid it has always had: asking the runtime instead could change that grid where LDS limits residency, a change of behaviour
// that belongs to a pull request of its own.
static int backward_resident(mi3d_solver *h, BwdRoute route, size_t lds, uint64_t &cap) {
    BwdCap &c = h->bwd_cap[(int)route];
    if (route == BwdRoute::Camera) c.blocks = h->counting ? 4 : 5;
    else if (!c.blocks || c.lds != lds || c.counting != h->counting) {
        int nb = 0;
        const hipError_t eo = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, backward_build(route, h->counting != 0, false), 256, lds);
        if (eo != hipSuccess || nb < 1) {
            if (route == BwdRoute::Weights) return fail(MI3D_EDEVICE, "emission weights: no workgroup of the weights build fits a CU with %zu bytes of LDS", lds);
            if (route == BwdRoute::Profiles || route == BwdRoute::ColumnsProfiles) return fail(MI3D_EDEVICE, "view profiles: no workgroup of the profiles build fits a CU with %zu bytes of LDS", lds);
            if (route == BwdRoute::CameraErrors || route == BwdRoute::ViewsErrors || route == BwdRoute::ViewsSunErrors || route == BwdRoute::ColumnsErrors ||
                route == BwdRoute::ColumnsSunErrors)
                return fail(MI3D_EDEVICE, "pixel errors: no workgroup of the errors build fits a CU with %zu bytes of LDS", lds);
            return fail(MI3D_EDEVICE, "backward Monte Carlo for satellite views: no workgroup fits a CU with %zu bytes of LDS", lds);
        }
        c.blocks = nb; c.lds = lds; c.counting = h->counting;
    }
    cap = (uint64_t)h->num_cu * (uint64_t)c.blocks;
    return MI3D_OK;
}

static int run_backward(mi3d_solver *h, uint64_t nphoton, uint64_t seed, uint64_t photon_offset) {
    const bool sat = h->sat_backward(), wgt = h->emis_weights != 0;
    const bool prf = sat && h->view_profiles != 0;
    const bool var = h->pixel_errors != 0;     // (never with wgt or prf: mi3d_run refuses)
    const bool sun = h->sun_backward();        // (never with wgt or prf: backward_unsupported refuses)
    const BwdRoute route = backward_column_route(sun ? (var ? BwdRoute::ViewsSunErrors : BwdRoute::ViewsSun)
                                                 : prf ? BwdRoute::Profiles : sat ? (var ? BwdRoute::ViewsErrors : BwdRoute::Views) : wgt ? BwdRoute::Weights
                                                 : var ? BwdRoute::CameraErrors : BwdRoute::Camera, h->col_backward());
    int rc = backward_unsupported(h, sat);
    if (rc) return rc;
    if (h->nview == 0) return fail(MI3D_ESTATE, "radiance requested but no view is set (%s)", sat ? "mi3d_set_views" : "mi3d_set_cameras");
    if (nphoton == 0) return MI3D_OK;
    DevBackward A;
    if ((rc = fill_backward(h, A, sat))) return rc;
    RunPlan plan = plan_run(h, nphoton);
    name_route(h, plan, false, nphoton);
    h->entry_form_last = 0;
    h->runs_unread++;
    const int npix = h->nview * h->nxr * h->nyr;
    BwdWeights W{};
    if (wgt) {
        // the weights build: its tally, made and zeroed here when it is the library's own
        W.ncell = (unsigned long long)h->wgt_ncell();
        W.nls = (int)(W.ncell - A.nvox);
        const double ne = (double)npix * (double)W.ncell;
        if (ne > kWgtMaxElems)
            return fail(MI3D_EUNSUP, "emission weights (mi3d_set_emission_weights 1): %d pixels x %llu cells are more than the 2^31 elements served", npix, W.ncell);
        if (!h->wgt_ext && h->wgt_n != (size_t)ne) {
            if ((rc = h->d_wgt_own.alloc((size_t)ne))) return rc;
            HIPCHK(hipMemsetAsync(h->d_wgt_own.p, 0, (size_t)ne * sizeof(double), h->stream));
            h->wgt_n = (size_t)ne;
        }
        W.K = h->wgt_ptr();
    }
    BwdProfiles P{};
    if (prf) {
        // the profiles build: its tally, made and zeroed here when it is the library's own
        P.nrow = h->nz + 1;
        const double ne = h->prf_elems();
        if (ne > kPrfMaxElems)
            return fail(MI3D_EUNSUP, "view profiles (mi3d_set_view_profiles 1): %d pixels x %d rows x 2 are more than the 2^31 elements served", npix, P.nrow);
        if (!h->prf_ext && h->prf_n != (size_t)ne) {
            if ((rc = h->d_prf_own.alloc((size_t)ne))) return rc;
            HIPCHK(hipMemsetAsync(h->d_prf_own.p, 0, (size_t)ne * sizeof(double), h->stream));
            h->prf_n = (size_t)ne;
        }
        P.raw = h->prf_ptr();
        h->prf_ran = true;
    }
    BwdErrors E{};
    if (var) {
        // the errors builds: the tally of the squared scores, made and zeroed here when it is the library's own
        if (!h->err_ext && h->err_n != (size_t)npix) {
            if ((rc = h->d_err_own.alloc((size_t)npix))) return rc;
            HIPCHK(hipMemsetAsync(h->d_err_own.p, 0, (size_t)npix * sizeof(double), h->stream));
            h->err_n = (size_t)npix;
        }
        E.rad2 = h->err_ptr();
        h->err_ran = true;
    }
    BwdSun N{};
    if (sun) fill_backward_sun(h, N);
    BwdSat S{};
    uint64_t ntile = 0;
    if (sat) {
        fill_backward_views(h, S, nullptr);
        ntile = (uint64_t)h->nview * (uint64_t)((h->nxr + 7) / 8) * (uint64_t)((h->nyr + 7) / 8);
    }
    // the launch's LDS (backward_lds).  The weights build stages its layer and surface weights there
    // where the image's sums are and the whole stays within kBwdWgtLds
    const bool lds_sums = backward_lds_sums(npix, false, S.jch > 0, var);
    if (wgt) {
        W.stage = h->wgt_stage != 0 && lds_sums && backward_lds(npix, h->nz, h->nview, W.nls, lds_sums, true, false) <= kBwdWgtLds ? 1 : 0;
        h->wgt_staged_last = W.stage;
    }
    const size_t lds = backward_lds(npix, h->nz, h->nview, W.nls, lds_sums, W.stage != 0, sat, var);
    // workgroups of 256 lanes, as many as are resident at once: every lane walks its ids with a fixed stride, and a workgroup that had to
    // queue would start when the others are through
    uint64_t cap = 0;
    if ((rc = backward_resident(h, route, lds, cap))) return rc;
    for (uint64_t done = 0; done < nphoton; done += h->batch) {
        const uint64_t nb = std::min<uint64_t>(h->batch, nphoton - done), off = photon_offset + done;
        if (h->pending.size() >= 64 && (rc = drain_events(h))) return rc;
        uint64_t want = (nb + 255) / 256;
        BwdSat Sl = S;
        if (sat && S.jch > 0) {
            // a wave per item of the tile hand-out, four to a workgroup.  A chunk the caller set is taken as it is; the default (-1) is at most
            // kBwdChunkAuto: where tiles x chunks would leave resident waves without an item (a small image, few histories per pixel) the
            // launch takes a smaller one
            const uint64_t jmax = (nb + (uint64_t)npix - 1) / (uint64_t)npix, per_tile = (cap * 4 + ntile - 1) / ntile;
            uint64_t jch = (uint64_t)S.jch;
            if (h->bwd_chunk < 0 && per_tile > 1) jch = std::min<uint64_t>(jch, std::max<uint64_t>(1, jmax / per_tile));
            Sl.jch = (int)jch;
            want = (ntile * ((jmax + jch - 1) / jch) + 3) / 4;
        }
        const unsigned grid = (unsigned)(want < cap ? want : cap);
        if (sat) h->bwd_chunk_last = Sl.jch;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        HIPCHK(hipEventCreate(&e0));
        hipError_t err = hipEventCreate(&e1);
        if (err == hipSuccess) err = hipEventRecord(e0, h->stream);
        if (err == hipSuccess) err = backward_launch(route, h->counting != 0, false, grid, lds, h->stream, A, seed, off, nb, nullptr, nullptr, W, Sl, P, E, N);
        if (err == hipSuccess) err = hipEventRecord(e1, h->stream);
        if (err != hipSuccess) {
            (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            return fail(MI3D_EDEVICE, "backward launch failed: %s", hipGetErrorString(err));
        }
        h->pending.emplace_back(e0, e1);
        h->launches++;
    }
    return MI3D_OK;
}

// The tally a read-out scales: the raw one, or -- backward route -- the raw one divided pixel by pixel by the number of ids in
// [0, nphoton_total) that map to the pixel (k_backward_norm), whose scale is then 1
static int readout_tally(mi3d_solver *h, uint64_t nphoton_total, const tally_t *&tally, double &norm) {
    tally = h->rad_ptr();
    if (!h->backward()) return MI3D_OK;
    const size_t n = (size_t)h->nview * h->nxr * h->nyr;
    int rc = h->d_bwd_norm.alloc(n);
    if (rc) return rc;
    hipLaunchKernelGGL(k_backward_norm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const double *)h->rad_ptr(), h->d_bwd_norm.p,
                       (unsigned long long)nphoton_total, (unsigned)n);
    HIPCHK(hipGetLastError());
    tally = h->d_bwd_norm.p; norm = 1.0;
    return MI3D_OK;
}

int mi3d_run(mi3d_solver *h, uint64_t nphoton, uint64_t seed, uint64_t photon_offset) {
    int rc = check_handle(h);
    if (rc) return rc;
    if ((rc = mi3d_prepare(h))) return rc;
    if (h->pixel_errors) {
        const char *why = h->emis_weights ? "emission weights (mi3d_set_emission_weights 1): the weights build is at its register limit"
                          : h->view_profiles ? "view profiles (mi3d_set_view_profiles 1): the profiles build is at its register limit"
                          : !(h->target & MI3D_TARGET_RADIANCE) || (h->target & MI3D_TARGET_FLUX) ? "a flux or heating-rate job: only the pixels of a backward image have histories of their own"
                          : !(h->cam_method == 1 || h->view_method == 1)
                              ? "a forward route (mi3d_set_camera_method 0, mi3d_set_view_method 0): one photon's contributions land in many pixels, so no pixel has "
                                "independent histories of its own"
                              : nullptr;
        if (why)
            return fail(MI3D_EUNSUP, "per-pixel standard errors (mi3d_set_pixel_errors 1) are tallied by the plain backward builds alone "
                                     "(mi3d_set_camera_method 1 or mi3d_set_view_method 1): not with %s", why);
    }
    if (h->view_profiles && (h->view_method != 1 || h->rad_kind != 2 || h->cam_method != 0 || h->emis_weights))
        return fail(MI3D_EUNSUP, "view profiles (mi3d_set_view_profiles 1) are tallied by the backward route for satellite views alone (mi3d_set_view_method 1 "
                                 "with mi3d_set_views, mi3d_set_camera_method 0, mi3d_set_emission_weights 0): not with %s",
                    h->view_method != 1 ? "mi3d_set_view_method 0" : h->rad_kind != 2 ? "cameras (mi3d_set_cameras)" : h->cam_method != 0 ? "mi3d_set_camera_method 1"
                                                                                                                      : "mi3d_set_emission_weights 1");
    if (h->view_sunlight && (rc = backward_unsupported(h, h->sat_backward()))) return rc;   // (names mi3d_set_view_sunlight where the refusal is its own)
    if (h->view_columns && (rc = backward_unsupported(h, h->sat_backward()))) return rc;    // (likewise mi3d_set_view_columns)
    if (h->view_method == 1 && h->rad_kind != 2) return backward_unsupported(h, true);   // (names the switch: it belongs to the views of mi3d_set_views)
    if (h->cam_method == 1 || h->view_method == 1) return run_backward(h, nphoton, seed, photon_offset);
    if (h->emis_weights)
        return fail(MI3D_EUNSUP, "emission weights (mi3d_set_emission_weights 1) are tallied by the backward route alone (mi3d_set_camera_method 1)");
    if ((h->target & MI3D_TARGET_RADIANCE) && h->nview == 0)
        return fail(MI3D_ESTATE, "radiance requested but no view is set (mi3d_set_views)");
    if ((h->target & MI3D_TARGET_RADIANCE) && h->rad_kind == 1 && h->solver != MI3D_SOLVER_3D)
        return fail(MI3D_EUNSUP, "cameras (Rad_mrkind=1) need the 3-D solver");
    const bool thermal = h->thermal();
    // (thermal cameras, Src_mtype = 3: served; the direct sun of a mixed job's cameras would need a normalisation of its own)
    if (h->src_mtype == 2 && (h->target & MI3D_TARGET_RADIANCE) && h->rad_kind == 1)
        return fail(MI3D_EUNSUP, "solar+thermal source (Src_mtype=2): all-sky cameras (Rad_mrkind=1) are not supported");
    if (nphoton == 0) return MI3D_OK;
    if (thermal && !(h->th_ptot + h->th_psol > 0.0)) {   // (the tallies stay 0)
        h->last_kernel = h->src_mtype == 2 ? "k_transport [solar+thermal: nothing emits, no sunlight]" : "k_transport [thermal: nothing emits]";
        return MI3D_OK;
    }
    {   // the kernels index every table with 32-bit arithmetic
        const double lim = 2147483647.0;
        const double nvox = (double)h->nx * h->ny * (h->nz3 + 1) * (h->np3d > 0 ? h->np3d : 1);
        if (nvox > lim || (double)h->flux_elems() > lim || (double)h->rad_elems() > lim || (double)h->heat_elems() > lim)
            return fail(MI3D_EUNSUP, "grid too large for the 32-bit table indices of the transport kernel");
    }
    h->entry_form_last = 0;
    DevScene S;
    if ((rc = fill_scene(h, S))) return rc;
    RunPlan plan = plan_run(h, nphoton);
    if (plan.sorted) {
        const size_t cap = (size_t)std::min<uint64_t>(nphoton, h->batch);
        const size_t nblk = std::min<size_t>((cap + 4095) / 4096, 4096);     // (launch_bins: counts per tile and block, and per tile)
        if ((rc = h->pre[0].order.alloc(cap)) || (rc = h->d_tile.alloc(cap)) || (rc = h->d_hist.alloc((size_t)plan.ntile * (nblk + 1)))) return rc;
    }
    h->cold_host.order = plan.sorted ? h->pre[0].order.p : nullptr;

    // ---- the room the route needs: tally-record lists (flux loop), event lists (marched views), entry records, second sets
    TallyList TL[2] = {};
    bool tl_two = false, two_sets = false;
    size_t lds_fl = 0;
    uint64_t ev_cap = 0;
    if (plan.loop == Loop::Flux && (rc = flux_lists(h, plan, nphoton, TL, tl_two, lds_fl))) return rc;
    if (h->rad_kind == 1 && plan.loop != Loop::ColumnRays && (rc = cam_fallback(h, plan.why))) return rc;
    if ((rc = event_lists(h, plan, nphoton, ev_cap, two_sets))) return rc;
    name_route(h, plan, TL[0].cap != 0, nphoton);
    const uint64_t cap = (uint64_t)h->num_cu * (plan.loop == Loop::Flux ? MI3D_FLUX_WAVES(plan.build.counting)
                                                : plan.loop == Loop::General ? MI3D_WAVES(plan.march, plan.build.counting)
                                                                             : MI3D_LEAN_WAVES(plan.build.counting, plan.march));
    const bool use_entry = use_entry_records(h, plan, nphoton);   // (fill_scene has cleared cold_host.entry)
    const bool pre_two = pre_second_set(h, plan, use_entry, two_sets, nphoton);
    // (a launch of a kind that MAY be followed by a two-stream launch on this handle leaves the events the latter waits for, also when it runs on one stream itself)
    const bool pre_track = h->overlap_pre && (plan.sorted || use_entry);
    h->runs_unread++;
    set_tally_window(h, plan);
    int rad_row = 0;
    if ((rc = rad_acc_image(h, plan, S, rad_row))) return rc;
    h->cold_host.cam_images = (unsigned)(plan.loop == Loop::ColumnRays ? (h->cam_images < 0 ? 2 : h->cam_images) : 0);
    HIPCHK(upload_cold(h, two_sets, pre_two));

    // ---- the launches.  With two sets the time of a run is the span from its first launch to the end of its last ray kernel (one pair of
    // events on the main stream, which joins the rays' stream at the end); launches that overlap cannot be timed one by one
    hipEvent_t run_e0 = nullptr;
    // (every way out of this function that still owns run_e0 is an error exit of a run on two streams: the event goes, and what is queued on
    //  the sort / pre-pass / rays streams is waited for -- ADVICE r5: several early returns left both behind)
    struct RunGuard { hipEvent_t &e; mi3d_solver *h; ~RunGuard() { if (e) { (void)hipEventDestroy(e); e = nullptr; (void)sync_streams(h); } } } run_guard{run_e0, h};
    const bool run_timed = two_sets || tl_two;   // (kernels on two streams: the run is timed as a whole, not launch by launch)
    if (run_timed) { HIPCHK(hipEventCreate(&run_e0)); HIPCHK(hipEventRecord(run_e0, h->stream)); }
    uint64_t ilaunch = 0;
    const uint64_t nlaunch = (nphoton + h->batch - 1) / h->batch;
    uint64_t per = (nphoton + nlaunch - 1) / nlaunch;
    for (uint64_t done = 0; done < nphoton; done += per) {
        if ((rc = launch_photons(h, plan, ev_cap, TL[0], tl_two, nphoton, done, per))) return rc;
        const uint64_t nb = std::min<uint64_t>(per, nphoton - done), off = photon_offset + done;
        if (h->pending.size() >= 64 && (rc = drain_events(h))) return rc;
        HIPCHK(hipMemsetAsync(h->d_next.p, 0, 8 * kCtrStride * sizeof(unsigned long long), h->stream));
        const int pset = pre_two ? (int)(h->pre_no & 1) : 0;
        mi3d_solver::PreSet &PS = h->pre[pset];
        const hipError_t eb = launch_pre(h, plan, pset, pre_two, pre_track, use_entry, S, nb, seed, off);
        if (eb != hipSuccess) { (void)sync_streams(h); return fail(MI3D_EDEVICE, "photon order / entry records: %s", hipGetErrorString(eb)); }
        DevScene Sl = S;
        if (pset) Sl.cold = h->d_cold.p + 1;   // (this launch's set of pre-pass buffers)
        const uint64_t want = (nb + 255) / 256;
        const unsigned grid = (unsigned)(want < cap ? want : cap);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        hipError_t err = run_timed ? hipSuccess : hipEventCreate(&e0);
        if (err == hipSuccess && !run_timed && (err = hipEventCreate(&e1)) == hipSuccess) err = hipEventRecord(e0, h->stream);
        const int set = two_sets ? (int)(ilaunch & 1) : 0;
        const int tset = tl_two ? (int)(h->tl_launch_no & 1) : 0;
        hipStream_t const rs = two_sets ? h->rays_stream : h->stream;
        if (err == hipSuccess && plan.loop == Loop::Flux) {
            err = launch_flux(h, plan.build, tset, tl_two, Sl, TL[tset], plan.mix, grid, lds_fl, nb, seed, off);
            if (err == hipSuccess && tl_two) { err = hipEventRecord(h->tl[tset].sorted, h->tl_stream); h->tl[tset].used = true; h->tl_unjoined = true; }
        } else if (err == hipSuccess && plan.loop == Loop::General) err = launch_general(h, plan.build, h->stream, Sl, plan.march ? 1 : 0, plan.flux, grid, nb, seed, off);
        else if (err == hipSuccess) err = launch_column(h, plan, Sl, set, two_sets, rs, grid, nb, seed, off);
        if (err == hipSuccess && !run_timed) err = hipEventRecord(e1, h->stream);
        h->pre_last = pset;
        h->entry_form_last = use_entry ? h->entry_form_run : 0; h->entry_n_last = nb;
        if (err == hipSuccess && (pre_two || pre_track)) {   // (the set may be written again once this launch's photon loop is through it)
            if (!PS.loop) err = hipEventCreateWithFlags(&PS.loop, hipEventDisableTiming);
            if (err == hipSuccess) err = hipEventRecord(PS.loop, h->stream);
            PS.used = true;
            if (pre_two) h->pre_no++;
        }
        if (err != hipSuccess) {   // (no event is left behind on the error path)
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            (void)sync_streams(h);
            return fail(MI3D_EDEVICE, "transport launch failed: %s", hipGetErrorString(err));
        }
        if (!run_timed) h->pending.emplace_back(e0, e1);
        h->launches++; ilaunch++;
        if (TL[0].cap) {
            const bool first = !(h->tl_total_pp > 0.0);
            if ((rc = tl_note(h, TL[0].cap, TL[0].bcap, TL[0].run_cap, nb, h->d_tl_stats.p + 4 * ((h->launches - 1) % 64), tl_two ? h->tl_stream : h->stream))) return rc;
            h->tl_launch_no++;
            // (nothing known about the scene's records per photon yet: the first launch is waited for -- the ones to come are then
            //  sized by what it needed instead of by a guess twice too large)
            if (first && done + nb < nphoton) {
                if ((rc = tl_collect(h, true))) return rc;
                // the pilot is through: lists for the rest of the run at the rates it has shown (every stream joined: the lists may move)
                HIPCHK(sync_streams(h));
                if (!size_tally_lists(h, std::min<uint64_t>(nphoton - done - nb, h->batch), tl_two ? 2 : 1, TL)) return fail(MI3D_EDEVICE, "no device memory to grow the tally-record lists after the pilot launch");
            }
        }
        if (plan.loop == Loop::ColumnRays) {
            // how full the lists got sizes the launches to come; read while they run (only a pilot is waited for)
            mi3d_solver::EvSet &E = h->ev[set];
            rc = ev_note(h, ev_cap, nb, rs, E.evctr.p);
            if (!rc && two_sets) {            // (after the copy of its fill counters: the set may be zeroed and filled again)
                if (hipEventRecord(E.rays, rs) != hipSuccess) rc = fail(MI3D_EDEVICE, "event record failed");
                E.used = true;
            }
            if (rc) { (void)sync_streams(h); return rc; }
            if (!(h->ev_per_photon > 0.0)) {
                // a pilot: wait for it, then give the lists the size the rest of the run needs
                if ((rc = ev_collect(h, true))) return rc;
                if (done + nb < nphoton) {
                    HIPCHK(sync_streams(h));
                    if (!(ev_cap = size_ev_lists(h, nphoton, two_sets))) return fail(MI3D_EDEVICE, "no device memory to grow the event lists of the marched views after the pilot launch");
                    HIPCHK(upload_cold(h, two_sets, pre_two));
                }
            }
        }
    }
    // (the last launches' fill counters are looked at by whoever reads the tallies next -- ev_settle -- or by the next run: the
    //  host does not wait here, so that the next run's launches queue up behind this one's)
    // ONE completion rule (round 6): when mi3d_run returns, everything it has started is queued on the handle's main stream or joined to it --
    // whatever the caller queues on that stream next, and every mi3d call, finds the tallies complete in stream order.  (Round 5 returned before
    // the last sort had joined where the tallies lived in the handle's own buffers, so that the next run's loops started beside it: worth 1-2 %
    // for runs queued back to back since the sums moved between the loops, and a rule a ctypes caller had to know.  "overlap_sort" 2 still asks
    // for it, for such runs on the handle's own buffers and stream: every reading call joins.)
    const bool tl_lazy = h->overlap_sort == 2 && tl_two && !two_sets && !h->flux_ext && !h->heat_ext && !h->rad_ext && (h->stream == nullptr || h->stream == h->own_stream);
    if (run_timed) {
        // (tl_unjoined has been set with the first sort of this run: a run that fails half way leaves it set, and the next call that looks at
        //  the tallies joins)
        if (tl_two && !tl_lazy) HIPCHK(tl_join(h));   // (... or the sort's)
        // the main stream joins the rays' stream: whatever follows on it -- the fold below, the next run, a read-out after mi3d_sync -- comes
        // after the last ray kernel; the run's time is the span up to here
        for (const auto &E : h->ev) if (two_sets && E.used) HIPCHK(hipStreamWaitEvent(h->stream, E.rays, 0));
        hipEvent_t run_e1 = nullptr;
        HIPCHK(hipEventCreate(&run_e1)); HIPCHK(hipEventRecord(run_e1, tl_two && tl_lazy ? h->tl_stream : h->stream));
        h->pending.emplace_back(run_e0, run_e1);
        run_e0 = nullptr;   // (owned by the pending list from here on)
    }
    if (plan.loop == Loop::ColumnRays && (rc = ev_collect(h, false))) { (void)sync_streams(h); return rc; }
    if (TL[0].cap && (rc = tl_collect(h, false))) return rc;
    if (rad_row) {
        const int n = (int)h->rad_elems();
        hipLaunchKernelGGL(k_fold_rad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_rad_acc.p, h->rad_ptr(), kRadLine, n, h->nxr, rad_row);
        HIPCHK(hipGetLastError());
    }
    return MI3D_OK;
}

int mi3d_sync(mi3d_solver *h) {
    int rc = check_handle(h);
    if (rc) return rc;
    HIPCHK(sync_main(h));
    return ev_settle(h);
}

int mi3d_set_kernel(mi3d_solver *h, int choice) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (choice < 0 || choice > 1) return fail(MI3D_EINVAL, "kernel choice %d (0: the lean kernels where they apply, 1: always the general one; choice 2, the lean loop with the rays of marched views inside it, was retired in round 5)", choice);
    HIPCHK(tl_join(h));   // (as every call that changes what the kernels work on: sorts still on their way join the main stream first)
    h->kernel_choice = choice;
    return MI3D_OK;
}

int mi3d_set_tuning(mi3d_solver *h, const char *key, int value) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!key) return fail(MI3D_EINVAL, "NULL key");
    const std::string k(key);
    if (k == "tile_cols") { if (value < -1 || value > 4096) return fail(MI3D_EINVAL, "tile_cols=%d", value); h->tile_cols = value; }
    else if (k == "batch_log2") { if (value < 8 || value > 30) return fail(MI3D_EINVAL, "batch_log2=%d outside [8,30]", value); h->batch = (uint64_t)1 << value; }
    else if (k == "evcap_log2") {
        if (value < 10 || value > 28) return fail(MI3D_EINVAL, "evcap_log2=%d outside [10,28]", value);
        HIPCHK(sync_streams(h));
        h->ev_cap_log2 = value; ev_forget(h);
        for (auto &E : h->ev) E.release();   // (lists only grow otherwise)
    }
    else if (k == "rad_spread") h->rad_spread = value < 0 ? -1 : (value ? 1 : 0);   // (-1: the default choice by route, mi3d_run)
    else if (k == "tally_window") h->tally_window = value ? 1 : 0;
    else if (k == "rad_row_pad") { if (value < -1 || value > 4096) return fail(MI3D_EINVAL, "rad_row_pad=%d outside [-1,4096]", value); h->rad_row_pad = value; }
    else if (k == "tlcap_log2") {
        if (value < 16 || value > 31) return fail(MI3D_EINVAL, "tlcap_log2=%d outside [16,31]", value);
        HIPCHK(sync_main(h));
        h->tl_cap_log2 = value; h->tl_per_photon = 0.0; h->tl_total_pp = 0.0; h->tl_runs_pp = 0.0;
        for (auto &S : h->tl_slot) S.busy = false;
        for (auto &T : h->tl) T.release();
    }
    else if (k == "vpad_col" || k == "vpad_row") {
        // padding of the voxel records' strides, in records of 16 bytes (DevScene::vcol_f4, vrow_f4): where a grid's strides alias in
        // the L2 -- the sorted photon order then gains little -- another stride may bring some of it back (profiles/r04/stride_probe*.log)
        if (value < 0 || value > 4096) return fail(MI3D_EINVAL, "%s=%d outside [0,4096]", key, value);
        (k == "vpad_col" ? h->vpad_col : h->vpad_row) = value;
        h->dirty_grid = true;
    }
    else if (k == "overlap_rays") { HIPCHK(sync_streams(h)); h->overlap_rays = value ? 1 : 0; }
    else if (k == "overlap_pre") { if (value < 0 || value > 2) return fail(MI3D_EINVAL, "overlap_pre=%d outside [0,2]", value); HIPCHK(sync_streams(h)); h->overlap_pre = value; if (!value) { h->pre[1].release(); h->pre_last = 0; } }
    else if (k == "overlap_sort") { if (value < 0 || value > 2) return fail(MI3D_EINVAL, "overlap_sort=%d outside [0,2]", value); HIPCHK(sync_streams(h)); h->overlap_sort = value; if (!value) h->tl[1].release(); }
    else if (k == "tl_split") { if (value < 1 || value > 64) return fail(MI3D_EINVAL, "tl_split=%d outside [1,64]", value); h->tl_split = value; }
    else if (k == "rays_wg" || k == "emit_wg") { if (value < 0 || value > 8) return fail(MI3D_EINVAL, "%s=%d outside [0,8]", key, value); (k == "rays_wg" ? h->rays_wg : h->emit_wg) = value; }
    else if (k == "bwd_chunk") {   // (the satellite views' backward route: histories of a pixel per item of the tile hand-out; 0: the camera route's stride)
        if (value < -1 || value > 65536) return fail(MI3D_EINVAL, "bwd_chunk=%d outside [-1,65536]", value);
        HIPCHK(sync_main(h)); h->bwd_chunk = value;
    }
    else if (k == "wgt_stage") { HIPCHK(sync_main(h)); h->wgt_stage = value ? -1 : 0; }   // (0: the emission weights' layer and surface part goes to global atomics always)
    else if (k == "cam_images") { if (value < -1 || value > 8) return fail(MI3D_EINVAL, "cam_images=%d outside [-1,8]", value); h->cam_images = value; }
    else if (k == "entry_records") { if (value < 0 || value > 2) return fail(MI3D_EINVAL, "entry_records=%d outside [0,2]", value); HIPCHK(sync_main(h)); h->entry_records = value; if (!value) h->pre[0].entry.release(); }
    else if (k == "tally_runs") { HIPCHK(sync_main(h)); h->tally_runs = value ? 1 : 0; h->tl_per_photon = 0.0; h->tl_total_pp = 0.0; h->tl_runs_pp = 0.0; if (!value) for (auto &T : h->tl) T.runs.release(); }
    else if (k == "tally_lists") { HIPCHK(sync_main(h)); h->tally_lists = value ? 1 : 0; if (!value) for (auto &T : h->tl) T.release(); }
    else if (k == "own_stream") {
        // a stream of the handle's own (non-blocking) wherever the caller binds none; the caller orders its own work with mi3d_sync
        HIPCHK(sync_main(h));
        const bool was_default = (h->stream == nullptr) || (h->stream == h->own_stream);
        if (value && !h->own_stream && hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess)
            return fail(MI3D_EDEVICE, "cannot create a stream");
        h->use_own_stream = value != 0;
        if (was_default) h->stream = h->use_own_stream ? h->own_stream : nullptr;
    }
    else return fail(MI3D_EINVAL, "unknown tuning key '%s'", key);
    return MI3D_OK;
}

const char *mi3d_last_kernel(mi3d_solver *h) { return h ? h->last_kernel.c_str() : ""; }

int mi3d_get_timing(mi3d_solver *h, double *kernel_ms, uint64_t *launches) {
    int rc = check_handle(h);
    if (rc) return rc;
    if ((rc = drain_events(h))) return rc;
    if (kernel_ms) *kernel_ms = h->kernel_ms;
    if (launches) *launches = h->launches;
    return MI3D_OK;
}

int mi3d_get_radiance(mi3d_solver *h, uint64_t nphoton_total, float *out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!out || nphoton_total == 0) return fail(MI3D_EINVAL, "bad arguments to mi3d_get_radiance");
    if (!h->rad_ptr()) return fail(MI3D_ESTATE, "no radiance tally (nothing has run)");
    HIPCHK(sync_main(h));
    if ((rc = ev_settle(h))) return rc;
    const size_t n = (size_t)h->nview * h->nxr * h->nyr;
    const double amp = src_amp(h);
    // satellite: radiance averaged over the pixel's share of the domain area; camera: the tallies hold 1 / (r^2 dOmega) already and
    // a photon stands for Src_flx mu0 Lx Ly / N of power (thermal: Src_flx P_tot / N)
    double fac = h->rad_kind == 1 ? amp * (h->dx * h->nx) * (h->dy * h->ny) / (double)nphoton_total
                                  : amp * (double)h->nxr * (double)h->nyr / (double)nphoton_total;
    // (scaled on the device, k_get_field: nine views of 480 x 480 pixels were 16 MB of float64 to the host and a loop over them)
    if (n == 0) return MI3D_OK;
    if ((rc = h->d_get_out.alloc(n))) return rc;
    const tally_t *rad_tally = nullptr;
    if ((rc = readout_tally(h, nphoton_total, rad_tally, fac))) return rc;   // (backward route: every pixel by its own count of histories)
    hipLaunchKernelGGL(k_get_field, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, rad_tally, h->d_get_out.p, fac,
                       1u, 1u, -1L, (const double *)nullptr, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->d_get_out.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI3D_OK;
}

int mi3d_get_flux(mi3d_solver *h, uint64_t nphoton_total, float *out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!out || nphoton_total == 0) return fail(MI3D_EINVAL, "bad arguments to mi3d_get_flux");
    if (!h->flux_ptr()) return fail(MI3D_ESTATE, "no flux tally (nothing has run)");
    HIPCHK(sync_main(h));
    const size_t n = h->flux_elems();
    const double amp = src_amp(h);
    const double fac = amp * (double)h->nx * (double)h->ny / (double)nphoton_total;
    // the raw planes are direct-down, diffuse-down, up (one atomic per crossing); the result planes direct-down, total-down, up.
    // At the levels above the 3-D region the direct beam is not tallied but known: Src_flx*mu0*exp(-tau/mu0) (thermal: none, 0).
    // (normalised on the device, k_get_field: float32 crosses to the host)
    const double *add = nullptr;
    if (!h->dir_level.empty()) {
        std::vector<double> a(h->dir_level);
        for (double &x : a) x = amp * x;
        if ((rc = h->d_get_add.upload(a.data(), a.size()))) return rc;
        add = h->d_get_add.p;
    }
    if (n == 0) return MI3D_OK;
    if ((rc = h->d_get_out.alloc(n))) return rc;
    hipLaunchKernelGGL(k_get_field, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->flux_ptr(), h->d_get_out.p, fac,
                       (unsigned)((size_t)h->nx * h->ny), (unsigned)(h->nz + 1), (long)(n / 3), add, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->d_get_out.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI3D_OK;
}

int mi3d_get_direct_levels(mi3d_solver *h, double *out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!out) return fail(MI3D_EINVAL, "out is NULL");
    if ((int)h->dir_level.size() != h->nz + 1) return fail(MI3D_ESTATE, "no job has run on this handle since its grid was set");
    const double amp = src_amp(h);
    for (int L = 0; L <= h->nz; ++L) out[L] = amp * h->dir_level[L];
    return MI3D_OK;
}

int mi3d_get_camera_direct(mi3d_solver *h, double *out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!out) return fail(MI3D_EINVAL, "out is NULL");
    if (h->rad_kind != 1) return fail(MI3D_ESTATE, "the views are not cameras (mi3d_set_cameras)");
    if ((rc = mi3d_prepare(h))) return rc;
    const size_t n = (size_t)h->nview * h->nxr * h->nyr;
    if (n == 0) return MI3D_OK;
    if (!h->camdir_ok)
        return fail(MI3D_EUNSUP, "the cameras' direct sun: Src_the=%g lies too close to the horizon (more than %.0f voxels to march)", h->src_the, kCamDirMaxCells);
    HIPCHK(hipMemcpyAsync(out, h->d_camdir.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; ++i) out[i] *= h->src_flx;
    return MI3D_OK;
}

int mi3d_get_heating(mi3d_solver *h, uint64_t nphoton_total, float *out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!out || nphoton_total == 0) return fail(MI3D_EINVAL, "bad arguments to mi3d_get_heating");
    if (!(h->target & MI3D_TARGET_HEAT) || !h->heat_ptr()) return fail(MI3D_ESTATE, "no heating-rate tally (the job's target does not include MI3D_TARGET_HEAT, or nothing has run)");
    HIPCHK(sync_main(h));
    const size_t n = h->heat_elems();
    // a photon stands for Src_flx mu0 Lx Ly / N of power (thermal: Src_flx P_tot / N; solar+thermal: Src_flx (P_tot + P_sol) / N)
    const double fac = src_amp(h) * (double)h->nx * (double)h->ny / (double)nphoton_total;
    if (h->thermal()) {
        // thermal or solar+thermal job: the NET, absorbed (from either source) - emitted.  The emission is known, not tallied: taken off here, once, in float64 on the device
        if (h->dirty_thermal || !h->d_th_tlev.p) return fail(MI3D_ESTATE, "thermal source: not built (nothing has run since the scene changed)");
        if (n == 0) return MI3D_OK;
        if ((rc = h->d_get_out.alloc(n))) return rc;
        hipLaunchKernelGGL(k_get_net_heating, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, thermal_grid(h), (const double *)h->heat_ptr(),
                           fac, h->src_flx, h->d_get_out.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, h->d_get_out.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return MI3D_OK;
    }
    // (on the device as the flux: tally * fac / layer thickness, float32 to the host)
    std::vector<double> dz((size_t)h->nz);
    for (int k = 0; k < h->nz; ++k) dz[k] = h->zgrd[k + 1] - h->zgrd[k];
    if ((rc = h->d_get_add.upload(dz.data(), dz.size()))) return rc;
    if (n == 0) return MI3D_OK;
    if ((rc = h->d_get_out.alloc(n))) return rc;
    hipLaunchKernelGGL(k_get_field, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const tally_t *)h->heat_ptr(), h->d_get_out.p, fac,
                       (unsigned)((size_t)h->nx * h->ny), (unsigned)h->nz, -1L, (const double *)h->d_get_add.p, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->d_get_out.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI3D_OK;
}

int mi3d_get_emission(mi3d_solver *h, float *out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!out) return fail(MI3D_EINVAL, "out is NULL");
    if (!h->thermal()) return fail(MI3D_ESTATE, "mi3d_get_emission: the job is not thermal (Src_mtype=%d): nothing emits", h->src_mtype);
    if ((rc = mi3d_prepare(h))) return rc;
    const size_t n = h->heat_elems();
    if (n == 0) return MI3D_OK;
    HIPCHK(sync_main(h));   // (d_get_out may still be on its way to the host for another getter's caller: one stream, in order)
    if ((rc = h->d_get_out.alloc(n))) return rc;
    hipLaunchKernelGGL(k_get_net_heating, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, thermal_grid(h), (const double *)nullptr,
                       0.0, h->src_flx, h->d_get_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->d_get_out.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI3D_OK;
}

int mi3d_get_counters(mi3d_solver *h, uint64_t out[MI3D_NCOUNTER]) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!out) return fail(MI3D_EINVAL, "out is NULL");
    HIPCHK(sync_main(h));
    if ((rc = ev_settle(h))) return rc;
    unsigned long long tmp[MI3D_NCOUNTER];
    HIPCHK(hipMemcpy(tmp, h->d_counters.p, sizeof(tmp), hipMemcpyDeviceToHost));
    for (int i = 0; i < MI3D_NCOUNTER; ++i) out[i] = tmp[i];
    return MI3D_OK;
}

// ---- run statistics --------------------------------------------------------------------------
static int stats_mark(mi3d_solver *h) {
    if (!h->stats_ev) HIPCHK(hipEventCreateWithFlags(&h->stats_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->stats_ev, h->stream));
    return MI3D_OK;
}

int mi3d_stats_begin(mi3d_solver *h, void *rad_run, void *flux_run) {
    int rc = check_handle(h);
    if (rc) return rc;
    if ((rc = mi3d_prepare(h))) return rc;
    h->run_ext[0] = (float *)rad_run;
    h->run_ext[1] = (float *)flux_run;
    for (int w = 0; w < 2; ++w) {
        const bool used = (h->target & (w == 0 ? MI3D_TARGET_RADIANCE : MI3D_TARGET_FLUX)) != 0;
        const size_t n = used ? h->stat_elems(w) : 0;
        if (!used || n == 0) continue;
        if (!h->run_ext[w] && (rc = h->d_run_own[w].alloc(n))) return rc;
        if ((rc = h->d_sum[w].alloc(n)) || (rc = h->d_sumsq[w].alloc(n))) return rc;
        HIPCHK(hipMemsetAsync(h->run_ptr(w), 0, n * sizeof(float), h->stream));
        HIPCHK(hipMemsetAsync(h->d_sum[w].p, 0, n * sizeof(double), h->stream));
        HIPCHK(hipMemsetAsync(h->d_sumsq[w].p, 0, n * sizeof(double), h->stream));
    }
    h->stats_on = true;
    h->stats_joined = false;
    h->stats_nrun = 0;
    return MI3D_OK;
}

int mi3d_stats_set_analytic_share(mi3d_solver *h, double share) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!(share >= 0.0 && share <= 1.0)) return fail(MI3D_EINVAL, "analytic share %g outside [0,1]", share);
    h->analytic_share = share;
    return MI3D_OK;
}

int mi3d_stats_add(mi3d_solver *h, uint64_t nphoton_total, const float *factor_rad, const float *factor_flux) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!h->stats_on) return fail(MI3D_ESTATE, "mi3d_stats_begin has not been called");
    if (nphoton_total == 0) return fail(MI3D_EINVAL, "nphoton_total is 0");
    const double amp = src_amp(h);
    for (int w = 0; w < 2; ++w) {
        if (!(h->target & (w == 0 ? MI3D_TARGET_RADIANCE : MI3D_TARGET_FLUX))) continue;
        const size_t n = h->stat_elems(w);
        if (n == 0) continue;
        if (!h->stats_joined && (!h->d_sum[w].p || h->d_sum[w].cap < n)) return fail(MI3D_ESTATE, "the scene changed shape since mi3d_stats_begin");
        const int nlevel = w == 0 ? h->nview : h->nz + 1;
        const int plane = w == 0 ? h->nxr * h->nyr : h->nx * h->ny;
        const float *fsrc = w == 0 ? factor_rad : factor_flux;
        std::vector<float> ones;
        if (!fsrc) { ones.assign(nlevel, 1.0f); fsrc = ones.data(); }
        // the factors are consumed by a kernel that may still be queued when the caller's buffer goes away
        if ((rc = h->d_factor[w].alloc(nlevel))) return rc;
        HIPCHK(hipMemcpyAsync(h->d_factor[w].p, fsrc, nlevel * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(sync_main(h));
        // (this call reads the tallies of the job that has just run: a launch of it whose event list ran full fails the call HERE -- the next
        //  mi3d_reset would forget it, and the short tallies would be part of the run's mean and standard deviation for good)
        if ((rc = ev_settle(h))) return rc;
        double norm = w == 0 ? (h->rad_kind == 1 ? amp * (h->dx * h->nx) * (h->dy * h->ny) / (double)nphoton_total
                                                       : amp * (double)h->nxr * (double)h->nyr / (double)nphoton_total)
                                   : amp * (double)h->nx * (double)h->ny / (double)nphoton_total; // as mi3d_get_*
        const tally_t *tally = w == 0 ? h->rad_ptr() : h->flux_ptr();
        if (w == 0 && (rc = readout_tally(h, nphoton_total, tally, norm))) return rc;   // (backward route: every pixel by its own count of histories)
        const double *dir_dev = nullptr;
        if (w == 1 && !h->dir_level.empty()) {
            std::vector<double> a(h->dir_level);
            for (double &x : a) x *= amp * h->analytic_share;
            if ((rc = h->d_dir_level.upload(a.data(), a.size()))) return rc;
            dir_dev = h->d_dir_level.p;
        }
        // (cameras with the rectangular map -- point radiometers: the direct sun joins the run field like the flux's analytic direct beam,
        //  on the ranks with an analytic share.  The polar map's run field stays diffuse only, as mi3d_get_radiance and its files are)
        const bool camdir = w == 0 && h->rad_kind == 1 && h->cam_mpmap == 2 && h->src_mtype == 1 && h->analytic_share > 0.0;
        if (camdir && !h->camdir_ok)
            return fail(MI3D_EUNSUP, "the cameras' direct sun: Src_the=%g lies too close to the horizon (more than %.0f voxels to march)", h->src_the, kCamDirMaxCells);
        hipLaunchKernelGGL(k_stats_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, tally, h->run_ptr(w),
                           h->d_factor[w].p, norm, plane, nlevel, w == 0 ? -1 : (int)(n / 3), dir_dev, (int)n,
                           camdir ? (const double *)h->d_camdir.p : (const double *)nullptr, h->src_flx * h->analytic_share);
        HIPCHK(hipGetLastError());
    }
    return stats_mark(h);
}

int mi3d_stats_end_run(mi3d_solver *h, float *rad_run_out, float *flux_run_out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!h->stats_on) return fail(MI3D_ESTATE, "mi3d_stats_begin has not been called");
    if (h->stats_joined) return fail(MI3D_ESTATE, "this handle adds into another handle's run (mi3d_stats_join): close the run on that one");
    for (int w = 0; w < 2; ++w) {
        if (!(h->target & (w == 0 ? MI3D_TARGET_RADIANCE : MI3D_TARGET_FLUX))) continue;
        const size_t n = h->stat_elems(w);
        if (n == 0) continue;
        float *out = w == 0 ? rad_run_out : flux_run_out;
        if ((rc = ev_settle(h))) return rc;   // (nothing busy after mi3d_stats_add; a handle that has only joined another's run may still have launches on their way)
        if (out) {
            HIPCHK(sync_main(h));
            HIPCHK(hipMemcpy(out, h->run_ptr(w), n * sizeof(float), hipMemcpyDeviceToHost));
        }
        hipLaunchKernelGGL(k_stats_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->run_ptr(w),
                           h->d_sum[w].p, h->d_sumsq[w].p, (int)n);
        HIPCHK(hipGetLastError());
    }
    h->stats_nrun++;
    return stats_mark(h);
}

// Two handles on one device may gather the jobs of ONE run between them (each transports every other job, so that the tail of
// one job's launch runs beside the next job's): the second one joins the first one's run fields (mi3d_stats_join), and every mi3d_stats_add / mi3d_stats_end_run is preceded by mi3d_stats_chain(h,
// other), which makes h's next statistics kernel wait for the other's last one: the run field is then summed in job order,
// exactly as one handle would have summed it.
int mi3d_stats_join(mi3d_solver *h, mi3d_solver *owner) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!owner || owner == h || !owner->stats_on || owner->stats_joined) return fail(MI3D_ESTATE, "mi3d_stats_join: the owner has not begun statistics of its own");
    if (owner->device != h->device) return fail(MI3D_EINVAL, "mi3d_stats_join: the two handles are on different devices");
    if ((rc = mi3d_prepare(h))) return rc;
    if (h->target != owner->target) return fail(MI3D_EINVAL, "mi3d_stats_join: the two handles have different targets");
    for (int w = 0; w < 2; ++w) {
        h->run_ext[w] = nullptr;
        if (!(h->target & (w == 0 ? MI3D_TARGET_RADIANCE : MI3D_TARGET_FLUX))) continue;
        if (h->stat_elems(w) != owner->stat_elems(w)) return fail(MI3D_EINVAL, "mi3d_stats_join: the two scenes have different result shapes");
        h->run_ext[w] = owner->run_ptr(w);
    }
    h->stats_on = true;
    h->stats_joined = true;
    h->stats_nrun = 0;
    return MI3D_OK;
}

int mi3d_stats_chain(mi3d_solver *h, mi3d_solver *after) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!after || after == h) return MI3D_OK;
    if (after->device != h->device) return fail(MI3D_EINVAL, "mi3d_stats_chain: the two handles are on different devices");
    if (after->stats_ev) HIPCHK(hipStreamWaitEvent(h->stream, after->stats_ev, 0));
    return MI3D_OK;
}

int mi3d_stats_get(mi3d_solver *h, int which, float *mean, float *sdev, int *nrun) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!h->stats_on) return fail(MI3D_ESTATE, "mi3d_stats_begin has not been called");
    if (which != MI3D_TARGET_RADIANCE && which != MI3D_TARGET_FLUX) return fail(MI3D_EINVAL, "which=%d", which);
    if (nrun) *nrun = h->stats_nrun;
    if (!mean && !sdev) return MI3D_OK;
    if (!(h->target & which)) return fail(MI3D_ESTATE, "no statistics of that kind were gathered");
    if (h->stats_nrun == 0) return fail(MI3D_ESTATE, "no run has been closed (mi3d_stats_end_run)");
    const int w = which == MI3D_TARGET_RADIANCE ? 0 : 1;
    const size_t n = h->stat_elems(w);
    if ((rc = h->d_stat_out.alloc(2 * n))) return rc;
    hipLaunchKernelGGL(k_stats_final, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_sum[w].p,
                       h->d_sumsq[w].p, h->d_stat_out.p, h->d_stat_out.p + n, 1.0 / (double)h->stats_nrun, (int)n);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_main(h));
    if ((rc = ev_settle(h))) return rc;   // (a run whose event lists ran full has gone into these statistics: the call fails)
    if (mean) HIPCHK(hipMemcpy(mean, h->d_stat_out.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (sdev) HIPCHK(hipMemcpy(sdev, h->d_stat_out.p + n, n * sizeof(float), hipMemcpyDeviceToHost));
    return MI3D_OK;
}

int mi3d_debug_philox(mi3d_solver *h, uint64_t seed, uint64_t id0, uint32_t draw, int n, uint32_t *out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (n <= 0 || !out) return fail(MI3D_EINVAL, "bad arguments to mi3d_debug_philox");
    DevBuf<uint32_t> d;
    if ((rc = d.alloc((size_t)4 * n))) return rc;
    hipLaunchKernelGGL(k_philox, dim3((n + 255) / 256), dim3(256), 0, h->stream, seed, id0, draw, n, d.p);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_main(h));
    HIPCHK(hipMemcpy(out, d.p, (size_t)4 * n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    d.release();
    return MI3D_OK;
}

int mi3d_debug_order(mi3d_solver *h, uint64_t n, uint32_t *order_out, uint32_t *tile_end_out, int ntile_max) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (n == 0 || !order_out) return fail(MI3D_EINVAL, "bad arguments to mi3d_debug_order");
    if (!h->pre[0].order.p || h->pre[0].order.cap < n) return fail(MI3D_ESTATE, "no photon order of that length (the last launch ran in id order, or was shorter)");
    HIPCHK(sync_main(h));
    HIPCHK(hipMemcpy(order_out, h->pre[h->pre_last].order.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (tile_end_out && ntile_max > 0)
        HIPCHK(hipMemcpy(tile_end_out, h->pre[h->pre_last].cursor.p, (size_t)std::min(ntile_max, kMaxTiles) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MI3D_OK;
}

int mi3d_debug_entry(mi3d_solver *h, uint64_t n, float *records_out) {
    int rc = check_handle(h);
    if (rc) return rc;
    const int form = h->entry_form_last;
    const mi3d_solver::PreSet &PS = h->pre[h->pre_last];
    if (form == 0 || !PS.entry.p) return fail(MI3D_ESTATE, "the last launch had no entry records (mi3d_debug_entry)");
    if (n > 0) {
        if (!records_out) return fail(MI3D_EINVAL, "bad arguments to mi3d_debug_entry");
        if (n > h->entry_n_last || entry_f4((size_t)n, form) > PS.entry.cap) return fail(MI3D_EINVAL, "mi3d_debug_entry: the last launch had %llu photons, not %llu", (unsigned long long)h->entry_n_last, (unsigned long long)n);
        HIPCHK(sync_streams(h));
        HIPCHK(hipMemcpy(records_out, PS.entry.p, entry_f4((size_t)n, form) * sizeof(float4), hipMemcpyDeviceToHost));
    }
    return form;
}

int mi3d_debug_thermal(mi3d_solver *h, double *ptot, double *cdf_out, uint64_t n) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!h->thermal()) return fail(MI3D_ESTATE, "mi3d_debug_thermal: the job is not thermal (Src_mtype=%d)", h->src_mtype);
    if (h->dirty_thermal || !h->d_th_cdf.p) return fail(MI3D_ESTATE, "mi3d_debug_thermal: the thermal source is not built (call mi3d_prepare)");
    if (cdf_out && n != h->th_ncell)
        return fail(MI3D_EINVAL, "mi3d_debug_thermal: the CDF has %zu cells, not %llu", h->th_ncell, (unsigned long long)n);
    HIPCHK(sync_main(h));
    if (ptot) *ptot = h->th_ptot;
    if (cdf_out) HIPCHK(hipMemcpy(cdf_out, h->d_th_cdf.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return MI3D_OK;
}

static_assert(MI3D_TAB_IDX_N == kTabIdxN, "include/mi3d.h states the length of a bucket index");

// The two debug entries of the backward route behind their own checks: the ids [id0, id0 + n) through the DEBUG build, and the capped
// count.  sat: the satellite views' entry, which also writes where every history starts (start_out)
static int debug_backward(mi3d_solver *h, bool sat, uint64_t seed, uint64_t id0, int n, float *start_out, float *dir_out, double *score_out, uint64_t *capped_out) {
    int rc;
    if (n > 0) {
        DevBackward A;
        BwdSat S{};
        BwdSun N{};
        const bool sun = sat && h->sun_backward();
        if (sun) fill_backward_sun(h, N);
        if ((rc = fill_backward(h, A, sat))) return rc;
        if ((sat && (rc = h->d_bwd_start.alloc((size_t)3 * n))) || (rc = h->d_bwd_dir.alloc((size_t)3 * n)) || (rc = h->d_bwd_score.alloc(n))) return rc;
        if (sat) fill_backward_views(h, S, h->d_bwd_start.p);
        // (every slot is written by the history of its id: the hand-out reaches every id of [id0, id0 + n) whatever the grid)
        const int npix = h->nview * h->nxr * h->nyr;
        const size_t lds = backward_lds(npix, h->nz, h->nview, 1, backward_lds_sums(npix, true, S.jch > 0), false, sat);
        HIPCHK(backward_launch(backward_column_route(sun ? BwdRoute::ViewsSun : sat ? BwdRoute::Views : BwdRoute::Camera, sat && h->col_backward()), false, true, (unsigned)((n + 255) / 256), lds, h->stream, A, seed, id0, (uint64_t)n,
                               h->d_bwd_dir.p, h->d_bwd_score.p, BwdWeights{}, S, BwdProfiles{}, BwdErrors{}, N));
        if (sat) HIPCHK(hipMemcpyAsync(start_out, h->d_bwd_start.p, (size_t)3 * n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(dir_out, h->d_bwd_dir.p, (size_t)3 * n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(score_out, h->d_bwd_score.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    if (capped_out) {
        *capped_out = 0;
        if (h->d_bwd_capped.p) { unsigned long long c = 0; HIPCHK(hipMemcpyAsync(&c, h->d_bwd_capped.p, sizeof(c), hipMemcpyDeviceToHost, h->stream)); HIPCHK(hipStreamSynchronize(h->stream)); *capped_out = c; }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI3D_OK;
}

int mi3d_debug_backward(mi3d_solver *h, uint64_t seed, uint64_t id0, int n, float *dir_out, double *score_out, uint64_t *capped_out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!dir_out || !score_out))) return fail(MI3D_EINVAL, "bad arguments to mi3d_debug_backward");
    if (h->cam_method != 1) return fail(MI3D_ESTATE, "mi3d_debug_backward: the backward route is not selected (mi3d_set_camera_method 1)");
    if ((rc = mi3d_prepare(h))) return rc;
    if ((rc = backward_unsupported(h, false))) return rc;
    return debug_backward(h, false, seed, id0, n, nullptr, dir_out, score_out, capped_out);
}

int mi3d_debug_backward_views(mi3d_solver *h, uint64_t seed, uint64_t id0, int n, float *start_out, float *dir_out, double *score_out, uint64_t *capped_out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!start_out || !dir_out || !score_out))) return fail(MI3D_EINVAL, "bad arguments to mi3d_debug_backward_views");
    if (h->view_method != 1 || h->cam_method != 0) return fail(MI3D_ESTATE, "mi3d_debug_backward_views: the route is not selected (mi3d_set_view_method 1, mi3d_set_camera_method 0)");
    if ((rc = mi3d_prepare(h))) return rc;
    if ((rc = backward_unsupported(h, true))) return rc;
    if (h->nview == 0) return fail(MI3D_ESTATE, "mi3d_debug_backward_views: no view is set (mi3d_set_views)");
    return debug_backward(h, true, seed, id0, n, start_out, dir_out, score_out, capped_out);
}

// Read-out of the emission weights (mi3d_set_emission_weights 1): the rows of K_raw by the rule of k_backward_norm, rounded to
// float32 on the device and brought over through a staging buffer of at most 2^26 elements; planck: cells[c].y as the kernel read it
int mi3d_get_emission_weights(mi3d_solver *h, uint64_t nphoton_total, float *weights, float *planck) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!weights) return fail(MI3D_EINVAL, "bad arguments to mi3d_get_emission_weights");
    if (!h->emis_weights) return fail(MI3D_ESTATE, "mi3d_get_emission_weights: the weights are not tallied (mi3d_set_emission_weights 1)");
    if (!h->backward()) return fail(MI3D_ESTATE, "mi3d_get_emission_weights: the backward route is not serving this job (mi3d_set_camera_method 1, Src_mtype=3, cameras)");
    if ((rc = mi3d_prepare(h))) return rc;
    const unsigned long long npix = (unsigned long long)h->nview * h->nxr * h->nyr, ncell = (unsigned long long)h->wgt_ncell();
    if ((double)npix * (double)ncell > kWgtMaxElems)
        return fail(MI3D_EUNSUP, "emission weights (mi3d_set_emission_weights 1): %llu pixels x %llu cells are more than the 2^31 elements served", npix, ncell);
    const unsigned long long ne = npix * ncell;
    HIPCHK(sync_main(h));
    const double *K = h->wgt_ptr();
    if (!K || (!h->wgt_ext && h->wgt_n != (size_t)ne)) {      // (nothing has been tallied for this scene yet)
        std::memset(weights, 0, (size_t)ne * sizeof(float));
    } else {
        const unsigned long long chunk = std::min<unsigned long long>(ne, 1ull << 26);
        if ((rc = h->d_wgt_out.alloc((size_t)chunk))) return rc;
        for (unsigned long long e0 = 0; e0 < ne; e0 += chunk) {
            const unsigned long long nn = std::min(chunk, ne - e0);
            const unsigned grid = (unsigned)std::min<unsigned long long>((nn + 255) / 256, 65536);
            hipLaunchKernelGGL(k_backward_norm_rows, dim3(grid), dim3(256), 0, h->stream, K, h->d_wgt_out.p, (unsigned long long)nphoton_total, (unsigned)npix, ncell, e0, nn);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(weights + e0, h->d_wgt_out.p, (size_t)nn * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        }
    }
    if (planck) {
        if (!h->d_bwd_cells.p) return fail(MI3D_ESTATE, "mi3d_get_emission_weights: the cells' Planck radiances have not been built");
        std::vector<float2> cells((size_t)ncell);
        HIPCHK(hipMemcpyAsync(cells.data(), h->d_bwd_cells.p, (size_t)ncell * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (size_t c = 0; c < (size_t)ncell; ++c) planck[c] = cells[c].y;
    }
    return MI3D_OK;
}

// Read-out of the view profiles (mi3d_set_view_profiles 1): the rows of P_raw by the rule of k_backward_norm, its pairs parted and
// rounded to float32 on the device and brought over through a staging buffer of at most 2 x 2^25 elements
int mi3d_get_view_profiles(mi3d_solver *h, uint64_t nphoton_total, float *weight, float *contribution) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!h->view_profiles) return fail(MI3D_ESTATE, "mi3d_get_view_profiles: the profiles are not tallied (mi3d_set_view_profiles 1)");
    if ((rc = mi3d_prepare(h))) return rc;
    if (!h->sat_backward() || !h->prf_ran || !h->prf_ptr() || (!h->prf_ext && h->prf_n != (size_t)h->prf_elems()))
        return fail(MI3D_ESTATE, "mi3d_get_view_profiles: nothing has been tallied (mi3d_run with mi3d_set_view_method 1 and mi3d_set_view_profiles 1)");
    const unsigned long long npix = (unsigned long long)h->nview * h->nxr * h->nyr, nrow = (unsigned long long)h->nz + 1;
    if (h->prf_elems() > kPrfMaxElems)
        return fail(MI3D_EUNSUP, "view profiles (mi3d_set_view_profiles 1): %llu pixels x %llu rows x 2 are more than the 2^31 elements served", npix, nrow);
    const unsigned long long ne = npix * nrow;
    HIPCHK(sync_main(h));
    const double *raw = h->prf_ptr();
    const unsigned long long chunk = std::min<unsigned long long>(ne, 1ull << 25);
    if ((rc = h->d_prf_out.alloc((size_t)chunk * 2))) return rc;
    for (unsigned long long e0 = 0; e0 < ne; e0 += chunk) {
        const unsigned long long nn = std::min(chunk, ne - e0);
        const unsigned grid = (unsigned)std::min<unsigned long long>((nn + 255) / 256, 65536);
        hipLaunchKernelGGL(k_backward_norm_profiles, dim3(grid), dim3(256), 0, h->stream, raw, h->d_prf_out.p, h->d_prf_out.p + chunk,
                           (unsigned long long)nphoton_total, (unsigned)npix, nrow, e0, nn);
        HIPCHK(hipGetLastError());
        if (weight) HIPCHK(hipMemcpyAsync(weight + e0, h->d_prf_out.p, (size_t)nn * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (contribution) HIPCHK(hipMemcpyAsync(contribution + e0, h->d_prf_out.p + chunk, (size_t)nn * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return MI3D_OK;
}

// Read-out of the per-pixel standard errors (mi3d_set_pixel_errors 1): k_backward_norm_se on the raw sums, float32
int mi3d_get_radiance_se(mi3d_solver *h, uint64_t nphoton_total, float *out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (!out) return fail(MI3D_EINVAL, "bad arguments to mi3d_get_radiance_se");
    if (!h->pixel_errors) return fail(MI3D_ESTATE, "mi3d_get_radiance_se: the squared scores are not tallied (mi3d_set_pixel_errors 1)");
    if ((rc = mi3d_prepare(h))) return rc;
    const size_t n = (size_t)h->nview * h->nxr * h->nyr;
    if (!h->backward() || !h->err_ran || !h->err_ptr() || (!h->err_ext && h->err_n != n))
        return fail(MI3D_ESTATE, "mi3d_get_radiance_se: nothing has been tallied since the last reset (mi3d_run on the backward route with mi3d_set_pixel_errors 1)");
    HIPCHK(sync_main(h));
    if ((rc = h->d_err_out.alloc(n))) return rc;
    hipLaunchKernelGGL(k_backward_norm_se, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const double *)h->rad_ptr(), (const double *)h->err_ptr(),
                       h->d_err_out.p, (unsigned long long)nphoton_total, (unsigned)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->d_err_out.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MI3D_OK;
}

int mi3d_debug_weights_staged(mi3d_solver *h) { return h ? h->wgt_staged_last : 0; }
int mi3d_debug_backward_chunk(mi3d_solver *h) { return h ? h->bwd_chunk_last : 0; }

int mi3d_debug_phase_tables(mi3d_solver *h, int nang, int npf, float *mu, float *p, float *cdf, uint16_t *mu_idx, uint16_t *cdf_idx) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (h->npf <= 0 || h->dirty_phase || !h->d_tmu.p) return fail(MI3D_ESTATE, "mi3d_debug_phase_tables: no phase table is built (mi3d_set_phase, mi3d_prepare)");
    if (nang != h->nang || npf != h->npf) return fail(MI3D_EINVAL, "mi3d_debug_phase_tables: the tables are %d x %d, not %d x %d", h->npf, h->nang, npf, nang);
    HIPCHK(sync_main(h));
    const size_t n = (size_t)nang, nt = n * (size_t)npf;
    if (mu) HIPCHK(hipMemcpy(mu, h->d_tmu.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (p) HIPCHK(hipMemcpy(p, h->d_tp.p, nt * sizeof(float), hipMemcpyDeviceToHost));
    if (cdf) HIPCHK(hipMemcpy(cdf, h->d_tcdf.p, nt * sizeof(float), hipMemcpyDeviceToHost));
    if (mu_idx) HIPCHK(hipMemcpy(mu_idx, h->d_tmuidx.p, (size_t)kTabIdxN * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (cdf_idx) HIPCHK(hipMemcpy(cdf_idx, h->d_tcdfidx.p, (size_t)npf * kTabIdxN * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return MI3D_OK;
}

int mi3d_debug_phase(mi3d_solver *h, int path, int tab_lo, int tab_n, int n, const float *apf, const float *x, const float *usel,
                     float *p_out, float *mu_out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (path < 0 || path > 3 || n <= 0 || !apf || !x || !usel || !p_out || !mu_out) return fail(MI3D_EINVAL, "bad arguments to mi3d_debug_phase");
    const bool tables = h->npf > 0;
    if (tables && (h->dirty_phase || !h->d_tmu.p)) return fail(MI3D_ESTATE, "mi3d_debug_phase: the phase tables are not built (call mi3d_prepare)");
    const bool staged = tables && (path == 1 || path == 2);
    size_t lds = sizeof(DevCold);
    if (staged) {
        if (tab_lo < 0 || tab_n < 1 || tab_n > h->npf - tab_lo)
            return fail(MI3D_EINVAL, "mi3d_debug_phase: tables %d .. %d are not among the %d loaded", tab_lo, tab_lo + tab_n - 1, h->npf);
        lds += lean_tab_floats(h->nang, tab_n) * sizeof(float);
        if (lds > 64 * 1024) return fail(MI3D_EINVAL, "mi3d_debug_phase: %d tables of %d angles do not fit the LDS (%zu bytes)", tab_n, h->nang, lds);
    }
    for (int i = 0; i < n; ++i) {
        if (path == 3 && !(apf[i] < 1.0f)) return fail(MI3D_EINVAL, "mi3d_debug_phase: path 3 takes analytic selectors only (apf[%d] = %g)", i, (double)apf[i]);
        if (staged && apf[i] >= 1.0f) {   // (the tables the routines will touch: table_pick's arithmetic)
            const float t = apf[i] - 1.0f;
            int i0 = (int)std::floor(t), i1 = t > (float)i0 ? i0 + 1 : i0;
            if (i0 >= h->npf - 1) i0 = i1 = h->npf - 1;
            if (i0 < tab_lo || i1 > tab_lo + tab_n - 1)
                return fail(MI3D_EINVAL, "mi3d_debug_phase: apf[%d] = %g refers to a table outside the staged %d .. %d", i, (double)apf[i], tab_lo, tab_lo + tab_n - 1);
        }
    }
    DevCold C;
    memset(&C, 0, sizeof(C));
    if (tables) {
        C.nang = h->nang; C.npf = h->npf; C.tmu = h->d_tmu.p; C.tp = h->d_tp.p; C.tcdf = h->d_tcdf.p;
        C.tmu_idx = h->d_tmuidx.p; C.tcdf_idx = h->d_tcdfidx.p;
        if (staged) { C.tab_lo = tab_lo; C.tab_n = tab_n; }
    }
    DevBuf<DevCold> d_cold;
    DevBuf<float> d_in, d_out;
    const size_t m = (size_t)n;
    auto done = [&](int code) { d_cold.release(); d_in.release(); d_out.release(); return code; };
    if ((rc = d_cold.upload(&C, 1)) || (rc = d_in.alloc(3 * m)) || (rc = d_out.alloc(2 * m))) return done(rc);
    if (hipMemcpy(d_in.p, apf, m * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_in.p + m, x, m * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_in.p + 2 * m, usel, m * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return done(fail(MI3D_EDEVICE, "mi3d_debug_phase: copy to the device failed"));
    const unsigned nblk = (unsigned)std::min<size_t>((m + 255) / 256, 1024);
    hipLaunchKernelGGL(k_debug_phase, dim3(nblk), dim3(256), lds, h->stream, d_cold.p, path, n, d_in.p, d_in.p + m, d_in.p + 2 * m, d_out.p, d_out.p + m);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = sync_main(h);
    if (e == hipSuccess) e = hipMemcpy(p_out, d_out.p, m * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(mu_out, d_out.p + m, m * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return done(fail(MI3D_EDEVICE, "mi3d_debug_phase: %s", hipGetErrorString(e)));
    return done(MI3D_OK);
}

constexpr int kDebugMaxPoints = 1 << 26;      // (the hooks below index [n][3] arrays with 32-bit integers)

int mi3d_debug_rotate(mi3d_solver *h, int n, const float *dir, const float *mu, const float *uphi, float *dir_out, float *sincos_out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (n <= 0 || n > kDebugMaxPoints || !dir || !mu || !uphi || !dir_out || !sincos_out) return fail(MI3D_EINVAL, "bad arguments to mi3d_debug_rotate");
    DevBuf<float> d_in, d_out;
    const size_t m = (size_t)n;
    auto done = [&](int code) { d_in.release(); d_out.release(); return code; };
    if ((rc = d_in.alloc(5 * m)) || (rc = d_out.alloc(5 * m))) return done(rc);
    if (hipMemcpy(d_in.p, dir, 3 * m * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_in.p + 3 * m, mu, m * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_in.p + 4 * m, uphi, m * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return done(fail(MI3D_EDEVICE, "mi3d_debug_rotate: copy to the device failed"));
    const unsigned nblk = (unsigned)std::min<size_t>((m + 255) / 256, 1024);
    hipLaunchKernelGGL(k_debug_rotate, dim3(nblk), dim3(256), 0, h->stream, n, d_in.p, d_in.p + 3 * m, d_in.p + 4 * m, d_out.p, d_out.p + 3 * m);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = sync_main(h);
    if (e == hipSuccess) e = hipMemcpy(dir_out, d_out.p, 3 * m * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(sincos_out, d_out.p + 3 * m, 2 * m * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return done(fail(MI3D_EDEVICE, "mi3d_debug_rotate: %s", hipGetErrorString(e)));
    return done(MI3D_OK);
}

int mi3d_debug_surface(mi3d_solver *h, int path, int n, int type, const float *param, const float *din, const float *dout, float *out) {
    int rc = check_handle(h);
    if (rc) return rc;
    if (path < 0 || path > 2 || n <= 0 || n > kDebugMaxPoints || !param || !din || (path == 0 && !dout) || !out) return fail(MI3D_EINVAL, "bad arguments to mi3d_debug_surface");
    const Sfc sf = {type, param[0], param[1], param[2], param[3], param[4]};
    DevBuf<float> d_in, d_out;
    const size_t m = (size_t)n;
    auto done = [&](int code) { d_in.release(); d_out.release(); return code; };
    if ((rc = d_in.alloc(6 * m)) || (rc = d_out.alloc(m))) return done(rc);
    if (hipMemcpy(d_in.p, din, 3 * m * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        (path == 0 && hipMemcpy(d_in.p + 3 * m, dout, 3 * m * sizeof(float), hipMemcpyHostToDevice) != hipSuccess))
        return done(fail(MI3D_EDEVICE, "mi3d_debug_surface: copy to the device failed"));
    const unsigned nblk = (unsigned)std::min<size_t>((m + 255) / 256, 1024);
    hipLaunchKernelGGL(k_debug_surface, dim3(nblk), dim3(256), 0, h->stream, path, n, sf, d_in.p, d_in.p + 3 * m, d_out.p);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = sync_main(h);
    if (e == hipSuccess) e = hipMemcpy(out, d_out.p, m * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return done(fail(MI3D_EDEVICE, "mi3d_debug_surface: %s", hipGetErrorString(e)));
    return done(MI3D_OK);
}

} // extern "C"
