// mi3d_kernel_backward_body.inc — the histories of the backward route, the one body of k_backward<COUNT, DEBUG> and k_backward_w<COUNT>
// and k_backward_v<COUNT, DEBUG> and k_backward_vp<COUNT> and k_backward_s<COUNT> and k_backward_vs<COUNT> and k_backward_vn<COUNT, DEBUG>
// and k_backward_vns<COUNT> and the column builds k_backward_vc<COUNT, DEBUG>, k_backward_vcs<COUNT>, k_backward_vcp<COUNT>,
// k_backward_vcn<COUNT, DEBUG>, k_backward_vcns<COUNT> (mi3d_kernel_backward.hip includes it inside each).  What it expects in scope:
// COUNT, DEBUG, WGT, SAT, PRF, VAR, SUN, COL (compile-time constants; COL: a history keeps its column, the satellite views under
// independent columns and partial 3-D, DESIGN.md §5.20), the arguments A, seed, id0, n, dir_out, score_out, W (BwdWeights: read where WGT
// holds, the weights build of DESIGN.md §5.12), S (BwdSat: read where SAT holds, the satellite-view build of DESIGN.md §5.14), P
// (BwdProfiles: read where PRF holds, the per-layer profiles of the satellite views, DESIGN.md §5.16) and E (BwdErrors: read where VAR
// holds, the second tally of the per-pixel standard errors, DESIGN.md §5.17) and N (BwdSun: read where SUN holds, the sunlight term of a
// solar+thermal job's satellite views, DESIGN.md §5.18).
    extern __shared__ double bwd_smem[];
    const int npix = A.nview * A.nxr * A.nyr;
    const bool tiles = SAT && S.jch > 0;                                     // the tile hand-out (mi3d_set_tuning "bwd_chunk" >= 1)
    const bool lds_sums = !DEBUG && npix <= (VAR ? kBwdLdsPixErr : kBwdLdsPix) && !tiles;
    double *sums = bwd_smem;
    double *sums2 = VAR ? bwd_smem + ((npix + 1) & ~1) : bwd_smem;           // (VAR) [npix] the workgroup's sums of squares, behind the sums
    const bool wstage = WGT && W.stage != 0;                                 // (the host sets it only where lds_sums holds)
    const int nls = WGT ? W.nls : 1, nwsum = wstage ? npix * nls : 0;
    double *wsum = bwd_smem + (lds_sums ? ((npix + 1) & ~1) : 0) + (VAR && lds_sums ? ((npix + 1) & ~1) : 0);   // [npix][nls] the workgroup's layer and surface weights
    LayerRec *slay = reinterpret_cast<LayerRec *>(bwd_smem + (lds_sums ? ((npix + 1) & ~1) : 0) + (VAR && lds_sums ? ((npix + 1) & ~1) : 0)
                                                  + (WGT ? ((nwsum + 1) & ~1) : 0));   // (16-byte aligned)
    CamRec *scam = reinterpret_cast<CamRec *>(slay + A.nz);
    const ViewRec *sview = reinterpret_cast<const ViewRec *>(scam);         // (SAT: the views stand where the cameras would)
    if (lds_sums) for (int i = threadIdx.x; i < npix; i += blockDim.x) sums[i] = 0.0;
    if (VAR && lds_sums) for (int i = threadIdx.x; i < npix; i += blockDim.x) sums2[i] = 0.0;
    if (WGT) for (int i = threadIdx.x; i < nwsum; i += blockDim.x) wsum[i] = 0.0;
    {   // layer table and cameras (SAT: views): 16-byte pieces
        const float4 *src = reinterpret_cast<const float4 *>(A.lay);
        float4 *dst = reinterpret_cast<float4 *>(slay);
        for (int i = threadIdx.x; i < A.nz * 4; i += blockDim.x) dst[i] = src[i];
        src = SAT ? reinterpret_cast<const float4 *>(S.views) : reinterpret_cast<const float4 *>(A.cams); dst = reinterpret_cast<float4 *>(scam);
        for (int i = threadIdx.x; i < A.nview * (SAT ? 2 : 4); i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();

    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t next = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;     // ids are handed out by a fixed stride
    unsigned long long c_hist = 0, c_steps = 0, c_steps3d = 0, c_scat = 0, c_sfc = 0;

    // The tile hand-out of the SAT build (DESIGN.md §5.14).  An item is (tile of 8 x 8 pixels, chunk of up to jch consecutive histories of each
    // of its pixels), number tile * nchunk + chunk; wave w of the launch takes the items w, w + nwaves, ...; lane L owns pixel (L & 7, L >> 3)
    // of the tile.  Every lane walks this sequence on its own.  Pixel p's ids in the batch [id0, id0 + n) are id0 + r + j npix with
    // r = (p - id0) mod npix, j < cnt = n / npix + (r < n mod npix): the two 64-bit remainders are the launch's, taken once.
    const int lane = threadIdx.x & 63;
    const uint64_t nwaves = stride >> 6;
    const int tiles_x = SAT ? (A.nxr + 7) >> 3 : 1, tiles_v = SAT ? tiles_x * ((A.nyr + 7) >> 3) : 1;
    const int off_m = tiles ? (int)(id0 % (uint64_t)npix) : 0, n_m = tiles ? (int)(n % (uint64_t)npix) : 0;
    const uint64_t n_q = tiles ? n / (uint64_t)npix : 0;
    const uint64_t jch = tiles ? (uint64_t)S.jch : 1;
    const uint64_t nchunk = tiles ? (n_q + (n_m ? 1 : 0) + jch - 1) / jch : 1;
    const uint64_t nitems = tiles ? (uint64_t)A.nview * (uint64_t)tiles_v * nchunk : 0;
    uint64_t item = next >> 6, idn = 0;      // the lane's next item; the next id of its chunk ...
    unsigned jn = 0;                         // ... and how many of the chunk are left
    double acc = 0.0;                        // the sum of the scores of pixel accpix since it last changed
    double acc2 = 0.0;                       // (VAR) ... and of their squares
    int accpix = 0;
    // PRF: the lane's run -- the sums of the terms of row run_e = pix nrow + k of P.raw since (pix, k) last changed.  A slant line takes
    // several cell steps inside a layer and, under the tile hand-out, a lane keeps its pixel: a run ends in two atomics, not a step
    int run_e = -1;                          // (npix nrow <= 2^30: the host refuses a tally of more than 2^31 elements)
    double accK = 0.0, accC = 0.0;
    auto prf_flush = [&]() {
        if (run_e >= 0) {
            if (accK != 0.0) atomicAdd(&P.raw[2 * (size_t)run_e], accK);
            if (accC != 0.0) atomicAdd(&P.raw[2 * (size_t)run_e + 1], accC);
        }
        accK = 0.0; accC = 0.0;
    };
    // the terms a (of K) and c (of C, the very term the score takes) of row `row` of pixel p
    auto prf_add = [&](const int p, const int row, const float a, const float c) {
        const int e = p * P.nrow + row;
        if (e != run_e) { prf_flush(); run_e = e; }
        accK += (double)a; accC += (double)c;
    };

    // the history's state
    bool have = false;
    uint64_t id = 0, slot = 0;
    int pix = 0, ix = 0, iy = 0, k = 0;
    float ux = 0.0f, uy = 0.0f, uz = 1.0f, tx = 0.0f, ty = 0.0f, tz = 0.0f, sx = 0.0f, sy = 0.0f, aiz = 0.0f;   // distances to the next x / y / z face, a cell's width along the line
    float w = 0.0f, taus = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
    double score = 0.0;
    uint32_t draw = 0;
    unsigned steps = 0;

    // SUN: the sun ray of an event, flown by the same trips of the loop as the walk (DESIGN.md §5.18).  While `sun` holds, the DDA registers
    // and ix, iy, k, ux, uy, uz are the ray's; the history's own cell, position in it and new direction wait in the s* registers
    bool sun = false, sun_end = false;       // the ray is under way; the history ends when the ray has
    int six = 0, siy = 0, sk = 0;
    float spx = 0.0f, spy = 0.0f, spz = 0.0f, snx = 0.0f, sny = 0.0f, snz = 0.0f;
    float sunc = 0.0f, sung = 0.0f;                   // the term's coefficient c in front of T, and g = c / F: what the history's weight has become on the ray
    float stau = 0.0f, staumax = 0.0f;                // the ray's optical path so far, the path beyond which the term is dropped
    float sdx = 0.0f, sdy = 0.0f, sdz = -1.0f;        // the direction d' in which the event's sunlight travels
    unsigned ssteps = 0;
    uint32_t sdraw = 0;                      // the history's cone draws: Philox blocks 2^31 + sdraw, which the walk never reaches
    const int k3hi = A.nz3 > 0 ? A.k3lo + A.nz3 : 0;  // (SUN) the layers from here up are horizontally uniform to the top: their optical depth is tabove

    // the DDA anew from a position inside the cell (px, py from the low faces, pz from the layer's bottom) and the direction
    auto set_dda = [&](const float px, const float py, const float pz, const float dzk) {
        const float aix = frcp(floor_abs(ux)), aiy = frcp(floor_abs(uy));
        aiz = frcp(floor_abs(uz));
        sx = A.dx * aix; sy = A.dy * aiy;
        tx = (ux > 0.0f ? A.dx - px : px) * aix;
        ty = (uy > 0.0f ? A.dy - py : py) * aiy;
        tz = (uz > 0.0f ? dzk - pz : pz) * aiz;
    };
    // the position inside the cell back from the DDA.  SAT: a vertical view flies with ux = uy = 0 exactly, where t * |u| would be 0 and the
    // position lost: the floor of set_dda's reciprocal gives it back (the camera builds never draw an exact 0 and keep their code)
    auto pos_x = [&]() { const float d = tx * (SAT ? floor_abs(ux) : fabsf(ux)); return fminf(fmaxf(ux > 0.0f ? A.dx - d : d, 0.0f), A.dx); };
    auto pos_y = [&]() { const float d = ty * (SAT ? floor_abs(uy) : fabsf(uy)); return fminf(fmaxf(uy > 0.0f ? A.dy - d : d, 0.0f), A.dy); };
    auto new_flight = [&]() {
        float u0;
        draw4(seed, id, draw++, u0, r1, r2, r3);
        taus = -__logf(u0);
    };
    // weight roulette (Pho_wmin, Pho_wfac) with the uniform number u: false: the history ends
    auto roulette = [&](const float u) {
        if (u * A.wfac < w) { w = A.wfac; return true; }
        return false;
    };

    // SUN: the direction d' of an event's sunlight: the sun's, or one drawn uniformly in solid angle inside the solar cone about it (the
    // forward launch's distribution: mu_cone = 1 - u (1 - cos_cone), rotate_dir)
    auto sun_dir = [&]() {
        sdx = N.sdx; sdy = N.sdy; sdz = N.sdz;
        if (N.cos_cone < 1.0f) {
            float q0, q1, q2, q3;
            draw4(seed, id, 0x80000000u | sdraw++, q0, q1, q2, q3);
            rotate_dir(sdx, sdy, sdz, 1.0f - q0 * (1.0f - N.cos_cone), q1);   // (sdz < 0 stays: the host refuses a cone that reaches the horizon)
        }
    };
    // SUN: the event's term sunc T(r -> top along -d') from the position (px, py, pz) inside cell (ix, iy, k), after the history's new
    // direction stands in ux, uy, uz.  Above the 3-D region the answer is closed and scored here; otherwise the lane goes over to the ray
    // (true: the caller leaves the next flight to the ray's end).  A ray is flown while g e^{-tau} >= kBwdWeightEnd, the weight below which
    // the walk ends a history: a rule that does not look at F, so that the tally is affine in F.  No term, no ray: none with F = 0
    auto sun_start = [&](const float px, const float py, const float pz, const bool end_after) {
        if (!(sunc > 0.0f) || !(sung > kBwdWeightEnd)) return false;
        const LayerRec &L0 = slay[k];
        if (k >= k3hi) {
            score += (double)(sunc * fexp_neg(fmaf(L0.bt, L0.dz - pz, L0.tabove) * frcp(-sdz)));
            return false;
        }
        staumax = __logf(sung * (1.0f / kBwdWeightEnd));
#ifdef MI3D_BWD_SUN_NESTED
        if (!COL) {   // the measurement build of DESIGN.md §5.18's A/B (make EXTRA=-DMI3D_BWD_SUN_NESTED): the whole ray here, in a loop of its own, with the same arithmetic
            const float vx = -sdx, vy = -sdy, vz = -sdz;
            const float bix = frcp(floor_abs(vx)), biy = frcp(floor_abs(vy)), biz = frcp(floor_abs(vz));
            const float qx = A.dx * bix, qy = A.dy * biy;
            float hx = (vx > 0.0f ? A.dx - px : px) * bix, hy = (vy > 0.0f ? A.dy - py : py) * biy, hz = (L0.dz - pz) * biz;
            int jx = ix, jy = iy, kk = k;
            float tau = 0.0f;
            unsigned ns = 0;
            bool drop = false;
            for (;;) {
                const LayerRec &L = slay[kk];
                const bool in3d = (L.flags & kLayIn3d) != 0;
                const int k3 = kk - A.k3lo;
                float ks = 0.0f;
                float2 cell;
                if (in3d) {
                    const float4 r = A.vrec[(size_t)jy * A.vrow_f4 + (size_t)jx * A.vcol_f4 + k3];
                    cell = A.cells[((size_t)k3 * A.ny + jy) * A.nx + jx];
                    ks = r.z;
                    for (int ip = 1; ip < A.np3d; ++ip) ks += A.csca[(((size_t)jy * A.nx + jx) * A.nz3 + k3) * A.np3d + ip].x;
                } else cell = A.cells[A.nvox + kk];
                for (int ip = 0; ip < A.np1d; ++ip) ks += L.ks1d[ip];
                const float ds = in3d ? fminf(fminf(hx, hy), hz) : hz;
                tau = fmaf(cell.x + ks, ds, tau); ns++;
                if (COUNT) { c_steps++; if (in3d) c_steps3d++; }
                const bool fz = !in3d || (hz <= hx && hz <= hy), fx = !fz && hx <= hy;
                hx -= ds; hy -= ds; hz -= ds;
                if (!in3d) {
                    if (hx < 0.0f) { const float nc = floorf(-hx / qx) + 1.0f; hx = fminf(fmaxf(fmaf(nc, qx, hx), 0.0f), qx); jx = bwd_wrap(jx, vx > 0.0f ? nc : -nc, A.nx); }
                    if (hy < 0.0f) { const float nc = floorf(-hy / qy) + 1.0f; hy = fminf(fmaxf(fmaf(nc, qy, hy), 0.0f), qy); jy = bwd_wrap(jy, vy > 0.0f ? nc : -nc, A.ny); }
                }
                if (tau > staumax) { drop = true; break; }
                if (ns >= kBwdMaxCells) { drop = true; atomicAdd(A.capped, 1ull); break; }
                if (fx) { hx = qx; jx += vx > 0.0f ? 1 : -1; jx = jx < 0 ? A.nx - 1 : (jx >= A.nx ? 0 : jx); }
                else if (!fz) { hy = qy; jy += vy > 0.0f ? 1 : -1; jy = jy < 0 ? A.ny - 1 : (jy >= A.ny ? 0 : jy); }
                else if (++kk >= k3hi) {
                    if (kk < A.nz) tau = fmaf(fmaf(slay[kk].bt, slay[kk].dz, slay[kk].tabove), biz, tau);
                    break;
                } else hz = slay[kk].dz * biz;
            }
            if (!drop) score += (double)(sunc * fexp_neg(tau));
            return false;
        }
#endif
        six = ix; siy = iy; sk = k; spx = px; spy = py; spz = pz; snx = ux; sny = uy; snz = uz;
        sun_end = end_after;
        ux = -sdx; uy = -sdy; uz = -sdz;
        set_dda(px, py, pz, L0.dz);
        stau = 0.0f; ssteps = 0;
        sun = true;
        return true;
    };

    for (;;) {
        bool ended = false;
        if (!have) {
            if (tiles) {
                while (jn == 0u && item < nitems) {
                    const uint64_t tile = item / nchunk, chunk = item - tile * nchunk;
                    item += nwaves;
                    const int iv = (int)tile / tiles_v, rem = (int)tile - iv * tiles_v, tj = rem / tiles_x, ti = rem - tj * tiles_x;
                    const int ir = ti * 8 + (lane & 7), jr = tj * 8 + (lane >> 3);
                    if (ir >= A.nxr || jr >= A.nyr) continue;                  // the tile is clipped at the image's edge
                    const int p = (iv * A.nyr + jr) * A.nxr + ir;
                    const int r = p - off_m + (p < off_m ? npix : 0);
                    if ((uint64_t)r >= n) continue;                             // no id of this pixel in the batch
                    const uint64_t cnt = n_q + (r < n_m ? 1u : 0u), j0 = chunk * jch;
                    if (j0 >= cnt) continue;
                    jn = (unsigned)(cnt - j0 < jch ? cnt - j0 : jch);
                    idn = id0 + (uint64_t)r + j0 * (uint64_t)npix;
                    if (p != accpix) {
                        if (!DEBUG && acc != 0.0) atomicAdd(&A.rad[accpix], acc);
                        if (VAR && acc2 != 0.0) atomicAdd(&E.rad2[accpix], acc2);
                        acc = 0.0; acc2 = 0.0; accpix = p;
                    }
                }
                if (jn == 0u) break;
                id = idn; slot = id - id0; idn += (uint64_t)npix; --jn;
                pix = accpix;
            } else {
                if (next >= n) break;
                slot = next; id = id0 + next; next += stride;
                pix = (int)(id % (uint64_t)npix);
            }
            have = true;
            score = 0.0; w = 1.0f; steps = 0; draw = 1;
            if (SUN) sdraw = 0;
            const int iv = pix / (A.nxr * A.nyr), rem = pix - iv * (A.nxr * A.nyr), jr = rem / A.nxr, ir = rem - jr * A.nxr;
            float u0, u1, u2, u3;
            draw4(seed, id, 0u, u0, u1, u2, u3);
            float x, y, z;
            if (SAT) {
                // a satellite view: the point (xr, yr) inside the pixel on the registration level, the line through it along the view
                // direction, and where that line meets the sensor plane z = zs (mi3d.h, mi3d_set_view_method)
                const ViewRec V = sview[iv];
                const float xr = ((float)ir + u0) * S.pix_dx, yr = ((float)jr + u1) * S.pix_dy;
                if (COL) { x = xr; y = yr; z = V.zs; }                        // the history belongs to the column under (xr, yr): no parallax shift
                else {
                    const float tq = (V.zs - V.zreg) / V.vz;                  // (up-looking: zreg is zs, 0)
                    x = fmaf(V.vx, tq, xr); y = fmaf(V.vy, tq, yr); z = V.zs;
                    x -= S.Lx * floorf(x * S.inv_Lx); y -= S.Ly * floorf(y * S.inv_Ly);
                    x = x >= S.Lx ? x - S.Lx : x; y = y >= S.Ly ? y - S.Ly : y;
                    x = fmaxf(x, 0.0f); y = fmaxf(y, 0.0f);
                }
                ux = -V.vx; uy = -V.vy; uz = -V.vz;
                if (DEBUG) {
                    dir_out[3 * slot] = ux; dir_out[3 * slot + 1] = uy; dir_out[3 * slot + 2] = uz;
                    S.start_out[3 * slot] = x; S.start_out[3 * slot + 1] = y; S.start_out[3 * slot + 2] = z;
                }
            } else {
                const CamRec Cm = scam[iv];
                float st, ct, ph;
                bool ok = true;
                if (!(A.cam_mode & kCamRect)) {
                    const float U = ((float)ir + u0 - 0.5f * (float)A.nxr) * frcp(Cm.inv_du), V = ((float)jr + u1 - 0.5f * (float)A.nyr) * frcp(Cm.inv_dv);
                    const float th = sqrtf(U * U + V * V);
                    ph = atan2f(V, U);
                    __sincosf(th, &st, &ct);
                    ok = th <= kPi;
                } else {
                    const float du = 1.0f / Cm.inv_du, t0 = (float)ir * du, t1 = (float)(ir + 1) * du;
                    if (A.cam_mode & kCamCos) {
                        const float s0 = sinf(t0), s1 = sinf(t1), s2 = fminf(fmaxf(fmaf(u0, s1 * s1 - s0 * s0, s0 * s0), 0.0f), 1.0f);
                        st = sqrtf(s2); ct = sqrtf(1.0f - s2);
                    } else {
                        const float c0 = cosf(t0), c1 = cosf(t1);
                        ct = fminf(fmaxf(fmaf(u0, c1 - c0, c0), -1.0f), 1.0f);
                        st = sqrtf(fmaxf(1.0f - ct * ct, 0.0f));
                    }
                    ph = ((float)jr + u1 - 0.5f * (float)A.nyr) / Cm.inv_dv;
                }
                float sp, cp;
                sincosf(ph, &sp, &cp);
                const float a = st * cp, b = st * sp;
                ux = a * Cm.xx + b * Cm.yx + ct * Cm.zx;
                uy = a * Cm.xy + b * Cm.yy + ct * Cm.zy;
                uz = a * Cm.xz + b * Cm.yz + ct * Cm.zz;
                const float nrm = 1.0f / sqrtf(ux * ux + uy * uy + uz * uz);
                ux *= nrm; uy *= nrm; uz *= nrm;
                if (DEBUG) { dir_out[3 * slot] = ux; dir_out[3 * slot + 1] = uy; dir_out[3 * slot + 2] = uz; }
                if (!ok || ct < Cm.cos_half) ended = true;       // outside the image or the cone of view: 0
                // where the history starts: the sensor, or where its line enters the top
                x = Cm.cx; y = Cm.cy; z = Cm.cz;
            }
            if (!ended && z >= A.ztoa) {
                if (uz >= 0.0f) ended = true;                 // never enters
                else if (COL) z = A.ztoa;                     // (it enters at the top of its own column)
                else { const float t = (z - A.ztoa) / -uz; x = fmaf(ux, t, x); y = fmaf(uy, t, y); z = A.ztoa; }
            }
            if (!ended) {
                k = A.nz - 1;
                if (z < A.ztoa) {
                    k = 0;
                    while (k < A.nz - 1 && z >= slay[k + 1].zlo) ++k;
                    if (z == slay[k].zlo && uz < 0.0f && k > 0) --k;        // on a level: the direction decides the cell
                }
                float cfx = floorf(x * A.inv_dx), cfy = floorf(y * A.inv_dy);
                float px = x - cfx * A.dx, py = y - cfy * A.dy;
                if (COL) {
                    // the column that contains the point, clipped: no face rule, the direction does not choose the column
                    cfx = fminf(fmaxf(cfx, 0.0f), (float)(A.nx - 1)); cfy = fminf(fmaxf(cfy, 0.0f), (float)(A.ny - 1));
                    px = x - cfx * A.dx; py = y - cfy * A.dy;
                } else {
                    if (px <= 0.0f && ux < 0.0f) { cfx -= 1.0f; px = A.dx; }    // on a face: likewise
                    if (py <= 0.0f && uy < 0.0f) { cfy -= 1.0f; py = A.dy; }
                }
                px = fminf(fmaxf(px, 0.0f), A.dx); py = fminf(fmaxf(py, 0.0f), A.dy);
                if (COL) { ix = (int)cfx; iy = (int)cfy; }
                else { ix = bwd_wrap(0, cfx, A.nx); iy = bwd_wrap(0, cfy, A.ny); }
                const float dzk = slay[k].dz;
                set_dda(px, py, fminf(fmaxf(z - slay[k].zlo, 0.0f), dzk), dzk);
                new_flight();
            }
        }
        if (!ended) {
            // ---- one cell step: the segment up to the next face (a level, outside the 3-D region) or to the end of the flight
            const LayerRec &L = slay[k];
            const bool in3d = (L.flags & kLayIn3d) != 0;
            // does this step cross x / y faces and move through the cyclic grid?  Always, but in a COL build: there the history keeps its
            // column and so does the sun ray of independent columns; the direct beam of partial 3-D (N.ray3d) alone flies in 3-D
            const bool cyc = !COL || (SUN && sun && N.ray3d != 0);
            const bool faces = cyc && in3d;
            float ks = 0.0f, ks0 = 0.0f, apf0 = 0.0f;
            float2 cell;
            const int k3 = k - A.k3lo;
            if (in3d) {
                const float4 r = A.vrec[(size_t)iy * A.vrow_f4 + (size_t)ix * A.vcol_f4 + k3];
                cell = A.cells[((size_t)k3 * A.ny + iy) * A.nx + ix];
                ks0 = r.z; apf0 = r.w; ks = ks0;
                for (int ip = 1; ip < A.np3d; ++ip) ks += A.csca[(((size_t)iy * A.nx + ix) * A.nz3 + k3) * A.np3d + ip].x;
            } else cell = A.cells[A.nvox + k];
            for (int ip = 0; ip < A.np1d; ++ip) ks += L.ks1d[ip];
            const float dface = faces ? fminf(fminf(tx, ty), tz) : tz;
            const float dsc = SUN && sun ? 3.0e38f : ks > 0.0f ? taus * frcp(ks) : 3.0e38f;    // (a sun ray has no free path: it ends at the top)
            const bool scat = dsc < dface;
            const float ds = scat ? dsc : dface;
            float e = 1.0f, em = 0.0f;
            if (SUN && sun) { stau = fmaf(cell.x + ks, ds, stau); ssteps++; }     // the ray: k_a and k_s of every constituent, no emission
            else {
                em = bwd_absorb(cell.x * ds, e);
                score += (double)(w * cell.y * em);
            }
            if (PRF) {
                const float a = w * em;
                if (a != 0.0f) prf_add(pix, k, a, w * cell.y * em);
            }
            if (WGT) {
                const float a = w * em;
                if (a != 0.0f) {
                    if (in3d) atomicAdd(&W.K[(unsigned long long)pix * W.ncell + (((size_t)k3 * A.ny + iy) * A.nx + ix)], (double)a);
                    else if (wstage) atomicAdd(&wsum[pix * nls + k], (double)a);
                    else atomicAdd(&W.K[(unsigned long long)pix * W.ncell + A.nvox + k], (double)a);
                }
            }
            w *= e;
            if (!(SUN && sun)) steps++;
            if (COUNT) { c_steps++; if (in3d) c_steps3d++; }
            const bool hitz = !scat && (!faces || (tz <= tx && tz <= ty)), hitx = !scat && !hitz && tx <= ty, hity = !scat && !hitz && !hitx;
            tx -= ds; ty -= ds; tz -= ds;
            taus = fmaxf(taus - ks * ds, 0.0f);
            if (!faces) {
                // a layer without x / y faces: the columns crossed on the way (COL: the position folds inside the column, which stays)
                if (tx < 0.0f) { const float nc = floorf(-tx / sx) + 1.0f; tx = fminf(fmaxf(fmaf(nc, sx, tx), 0.0f), sx); if (cyc) ix = bwd_wrap(ix, ux > 0.0f ? nc : -nc, A.nx); }
                if (ty < 0.0f) { const float nc = floorf(-ty / sy) + 1.0f; ty = fminf(fmaxf(fmaf(nc, sy, ty), 0.0f), sy); if (cyc) iy = bwd_wrap(iy, uy > 0.0f ? nc : -nc, A.ny); }
            }
            if (SUN && sun) {
                // ---- the sun ray: on through the next face; above the 3-D region and at the top it ends in closed form
                bool done = false, drop = false;
                if (stau > staumax) { done = true; drop = true; }                // g e^{-tau} has fallen below kBwdWeightEnd
                else if (ssteps >= kBwdMaxCells) { done = true; drop = true; atomicAdd(A.capped, 1ull); }
                else if (hitx) { tx = sx; ix += ux > 0.0f ? 1 : -1; ix = ix < 0 ? A.nx - 1 : (ix >= A.nx ? 0 : ix); }
                else if (hity) { ty = sy; iy += uy > 0.0f ? 1 : -1; iy = iy < 0 ? A.ny - 1 : (iy >= A.ny ? 0 : iy); }
                else if (++k >= k3hi) {                                         // (uz > 0 always)
                    if (k < A.nz) stau = fmaf(fmaf(slay[k].bt, slay[k].dz, slay[k].tabove), aiz, stau);
                    done = true;
                } else tz = slay[k].dz * aiz;
                if (done) {
                    if (!drop) score += (double)(sunc * fexp_neg(stau));
                    sun = false;
                    ix = six; iy = siy; k = sk; ux = snx; uy = sny; uz = snz;
                    set_dda(spx, spy, spz, slay[k].dz);
                    if (sun_end) ended = true;
                    else new_flight();
                }
            } else if (w < kBwdWeightEnd) ended = true;
            else if (steps >= kBwdMaxCells) { ended = true; atomicAdd(A.capped, 1ull); }
            else if (scat) {
                // ---- scattering: the constituent in proportion to k_s (u1), its phase function (u2), the azimuth (u3)
                if (COUNT) c_scat++;
                const float target = r1 * ks;
                float cum = 0.0f, apf = -2.0f, usel = 0.0f;
                bool found = false;
                const int ncomp = A.np1d + (in3d ? A.np3d : 0);
                for (int q = 0; q < ncomp; ++q) {
                    float kq, aq;
                    if (q < A.np1d) { kq = L.ks1d[q]; aq = L.apf1d[q]; }
                    else if (q == A.np1d) { kq = ks0; aq = apf0; }
                    else { const float2 c = A.csca[(((size_t)iy * A.nx + ix) * A.nz3 + k3) * A.np3d + (q - A.np1d)]; kq = c.x; aq = c.y; }
                    if (!found && (target < cum + kq || q == ncomp - 1)) { found = true; apf = aq; usel = kq > 0.0f ? (target - cum) * frcp(kq) : 0.0f; }
                    cum += kq;
                }
                usel = fminf(fmaxf(usel, 0.0f), 1.0f);
                const float mu = apf >= 1.0f ? phase_sample_table(A.tab, apf, r2, usel) : phase_sample_analytic(apf, r2);
                const float px = pos_x(), py = pos_y();
                const float dz0 = tz * fabsf(uz), pz = fminf(fmaxf(uz > 0.0f ? L.dz - dz0 : dz0, 0.0f), L.dz);
                if (SUN) {
                    // the sunlight this event turns into the line of sight: w P_q(d' . (-u)) / 4 pi  F mu0 / |d'_z|, P_q of the constituent chosen
                    sun_dir();
                    const float cs = fminf(fmaxf(-(sdx * ux + sdy * uy + sdz * uz), -1.0f), 1.0f);
                    const float pq = apf >= 1.0f ? phase_eval_table(A.tab, apf, cs) : phase_eval_analytic(apf, cs);
                    sung = w * pq * (0.25f / kPi) * N.mu0 * frcp(-sdz);
                    sunc = sung * N.F;
                }
                rotate_dir(ux, uy, uz, mu, r3);
                set_dda(px, py, pz, L.dz);
                if (w < A.wmin) {
                    float q0, q1, q2, q3;
                    draw4(seed, id, draw++, q0, q1, q2, q3);
                    if (!roulette(q0)) ended = true;
                }
                if (SUN && sun_start(px, py, pz, ended)) ended = false;           // (the history's end, if it has come, waits for the ray's)
                else if (!ended) new_flight();
            } else if (!COL && hitx) { tx = sx; ix += ux > 0.0f ? 1 : -1; ix = ix < 0 ? A.nx - 1 : (ix >= A.nx ? 0 : ix); }
            else if (!COL && hity) { ty = sy; iy += uy > 0.0f ? 1 : -1; iy = iy < 0 ? A.ny - 1 : (iy >= A.ny ? 0 : iy); }
            else if (uz > 0.0f) {
                if (++k >= A.nz) ended = true;                 // the top: space is cold
                else tz = slay[k].dz * aiz;
            } else if (--k >= 0) tz = slay[k].dz * aiz;
            else {
                // ---- the surface: it emits eps B(Ts) into the line of sight and reflects the rest (Lambertian)
                if (COUNT) c_sfc++;
                const float px = pos_x(), py = pos_y();
                const int ib = min((int)(((float)ix * A.dx + px) * A.sfc_sx), A.nxb - 1), jb = min((int)(((float)iy * A.dy + py) * A.sfc_sy), A.nyb - 1);
                const float2 sc = A.cells[A.nvox + A.nz + (size_t)max(jb, 0) * A.nxb + max(ib, 0)];
                score += (double)(w * sc.x * sc.y);
                if (PRF) {
                    const float a = w * sc.x;
                    if (a != 0.0f) prf_add(pix, A.nz, a, w * sc.x * sc.y);
                }
                if (WGT) {
                    const float a = w * sc.x;
                    const int s = max(jb, 0) * A.nxb + max(ib, 0);
                    if (a != 0.0f) {
                        if (wstage) atomicAdd(&wsum[pix * nls + A.nz + s], (double)a);
                        else atomicAdd(&W.K[(unsigned long long)pix * W.ncell + A.nvox + A.nz + s], (double)a);
                    }
                }
                if (SUN) {
                    // the sunlight the surface reflects into the line of sight: w (1 - eps) / pi  F mu0 (mu0 / |d'_z| cancels against the cosine)
                    sun_dir();
                    sung = w * (1.0f - sc.x) * (1.0f / kPi) * N.mu0;
                    sunc = sung * N.F;
                }
                w *= 1.0f - sc.x;
                if (w < kBwdWeightEnd) ended = true;
                else {
                    float q0, q1, q2, q3;
                    draw4(seed, id, draw++, q0, q1, q2, q3);
                    const float cz = sqrtf(q0), sz = sqrtf(fmaxf(1.0f - q0, 0.0f));
                    float sp, cp;
                    sincos_turns(q1, sp, cp);
                    ux = sz * cp; uy = sz * sp; uz = cz;
                    k = 0;
                    set_dda(px, py, 0.0f, slay[0].dz);
                    if (w < A.wmin && !roulette(q2)) ended = true;
                    if (!SUN && !ended) new_flight();
                }
                if (SUN) {
                    k = 0;
                    if (sun_start(px, py, 0.0f, ended)) ended = false;
                    else if (!ended) new_flight();
                }
            }
        }
        if (ended) {
            have = false;
            const double s = score * (double)A.src_flx;
            if (DEBUG) score_out[slot] = s;
            else if (tiles) { acc += s; if (VAR) acc2 += s * s; }
            else if (s != 0.0) {
                if (lds_sums) { atomicAdd(&sums[pix], s); if (VAR) atomicAdd(&sums2[pix], s * s); }
                else { atomicAdd(&A.rad[pix], s); if (VAR) atomicAdd(&E.rad2[pix], s * s); }
            }
            if (COUNT) c_hist++;
        }
    }
    if (tiles && !DEBUG && acc != 0.0) atomicAdd(&A.rad[accpix], acc);
    if (VAR && tiles && acc2 != 0.0) atomicAdd(&E.rad2[accpix], acc2);
    if (PRF) prf_flush();
    if (lds_sums) {
        __syncthreads();
        for (int i = threadIdx.x; i < npix; i += blockDim.x) { const double s = sums[i]; if (s != 0.0) atomicAdd(&A.rad[i], s); }
        if (VAR) for (int i = threadIdx.x; i < npix; i += blockDim.x) { const double s = sums2[i]; if (s != 0.0) atomicAdd(&E.rad2[i], s); }
        if (WGT)
            for (int i = threadIdx.x; i < nwsum; i += blockDim.x) {
                const double s = wsum[i];
                const int p = i / nls;
                if (s != 0.0) atomicAdd(&W.K[(unsigned long long)p * W.ncell + A.nvox + (i - p * nls)], s);
            }
    }
    if (COUNT && !DEBUG) {
        atomicAdd(A.counters + MI3D_CNT_PHOTONS, c_hist);
        atomicAdd(A.counters + MI3D_CNT_STEPS, c_steps);
        atomicAdd(A.counters + MI3D_CNT_STEPS3D, c_steps3d);
        atomicAdd(A.counters + MI3D_CNT_SCATTER, c_scat);
        atomicAdd(A.counters + MI3D_CNT_SURFACE, c_sfc);
    }
