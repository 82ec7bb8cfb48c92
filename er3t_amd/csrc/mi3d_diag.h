// mi3d_diag.h -- everything the photon loops carry for MEASUREMENT builds only, in one place, so that the kernels read as the algorithm
// (VERDICT r5 item 6).  None of it is compiled into the shipped library: every macro below expands to nothing unless the build asks
// for it (make EXTRA=-DMI3D_...).  What each build is for, and the log it produced, stands beside its switch.
#pragma once

// -DMI3D_MARKS: comments in the ISA listing that delimit the blocks of a loop (tools/isa_blocks.py; superseded by the line table,
// tools/isa_lines.py, but still the quickest way to find a block in a listing)
#ifdef MI3D_MARKS
#define MI3D_MARK(name) asm volatile("; MARK " name)
#else
#define MI3D_MARK(name)
#endif

// The instrumented builds (COUNT = true, mi3d_set_counting) split the wave time of a loop over six clock counters (Counters::cyc).
// -DMI3D_NO_LEAN_TICKS leaves the counters to the ray kernels, which share them (tools/sched_rays.py); -DMI3D_CENSUS keeps three
// (the census of tally addresses uses the others: tools/census.py, profiles/r04/tally_same_address_census.log).
#if defined(MI3D_NO_LEAN_TICKS)
#define MI3D_DIAG_TICK(COUNT_, cnt_, tick_, slot) do { } while (0)
#elif defined(MI3D_CENSUS)
#define MI3D_DIAG_TICK(COUNT_, cnt_, tick_, slot) do { if ((COUNT_) && (slot) < 3) { const long long t_ = clock64(); (cnt_).cyc[slot] += (uint32_t)((t_ - (tick_)) >> 6); (tick_) = t_; } } while (0)
#else
#define MI3D_DIAG_TICK(COUNT_, cnt_, tick_, slot) do { if (COUNT_) { const long long t_ = clock64(); (cnt_).cyc[slot] += (uint32_t)((t_ - (tick_)) >> 6); (tick_) = t_; } } while (0)
#endif

// -DMI3D_FULL_CENSUS=1 / 2 (round 7, tools/full_pass_census.py, profiles/r07/full_pass_census_*.log): what the full passes of the lean photon
// loop serve and what they park, in counters the column-view build leaves at zero (le_steps, le_steps3d, flux_tally) and in the six clock
// counters, whose split becomes A | B0 + B5 + B6 + B7 | C | B4 until its reads are issued | B2 | B4 from there until the records are unpacked.
//   1: le_steps   lanes in a rare mode (not flying, not done, no collision found by the walk) when phase B of a pass that is NOT full begins
//      le_steps3d lanes x full passes (64 per full pass of a wave)
//      flux_tally lanes a later block hands to an earlier one (B6 -> M_UNIF, roulette survivor -> M_DRAW): they wait for a second full pass
//   2: le_steps / le_steps3d / flux_tally  lanes served by B0 / B2 / B4 (B5 serves what B2 leaves alive, B6 those and the roulette, B7 the rest)
#ifdef MI3D_FULL_CENSUS
#define MI3D_FPC(COUNT_, cnt_, set_, field_, cond_) do { if ((COUNT_) && MI3D_FULL_CENSUS == (set_) && (cond_)) (cnt_).field_++; } while (0)
#define MI3D_FPC_TICK(COUNT_, cnt_, tick_, slot_old, slot_census) MI3D_DIAG_TICK(COUNT_, cnt_, tick_, slot_census)
#else
#define MI3D_FPC(COUNT_, cnt_, set_, field_, cond_) do { } while (0)
#define MI3D_FPC_TICK(COUNT_, cnt_, tick_, slot_old, slot_census) do { if ((slot_old) >= 0) MI3D_DIAG_TICK(COUNT_, cnt_, tick_, (slot_old) < 0 ? 0 : (slot_old)); } while (0)
#endif

// -DMI3D_WAIT_CENSUS (round 13, tools/wait_census.py, profiles/r13/wait_census_les480.log): what two waits of a pass of the lean photon loop cost.
// The six clock counters become, in wave cycles: [0] phase A | [1] the pass's count and its read of the window's origin, up to the origin in a
// scalar register | [2] block C's first wait (the records the walk's last step asked for; with MI3D_LEAN_C_EARLY the layer table with them) |
// [3] two ticks back to back, once a pass: what a tick costs (it reads the clock through the scalar memory path and waits for it) | [4] the
// rest of BSCHED + C | [5] the full pass and the loop's end.  The other ticks are off.  Exact to the cycle: a lane adds
// (cycles + its number) / 64 and the lanes are summed.  NOT the shipped order to the instruction: the empty `asm volatile` that pins block C's early
// reads is off in this build and an explicit `s_waitcnt vmcnt(0) lgkmcnt(0)` between two ticks stands where the record's first use would wait, and
// it is the counting build (four waves per SIMD, not six): the figures say where a wave is parked, not what the plain build gains.
#ifdef MI3D_WAIT_CENSUS
#ifdef MI3D_FULL_CENSUS
#error "MI3D_WAIT_CENSUS and MI3D_FULL_CENSUS share the six clock counters: build one census at a time"
#endif
#undef MI3D_DIAG_TICK
#define MI3D_DIAG_TICK(COUNT_, cnt_, tick_, slot) do { } while (0)
#define MI3D_WAIT_CENSUS_ON 1
#define MI3D_WAIT_TICK(COUNT_, cnt_, tick_, slot) do { if (COUNT_) { const long long t_ = clock64(); (cnt_).cyc[slot] += (uint32_t)((t_ - (tick_) + (long long)(threadIdx.x & 63)) >> 6); (tick_) = t_; } } while (0)
#else
#define MI3D_WAIT_CENSUS_ON 0
#define MI3D_WAIT_TICK(COUNT_, cnt_, tick_, slot) do { } while (0)
#endif

// -DMI3D_WIN_DIAG: le_steps3d counts the column-view tallies that stayed in the LDS tally window, le_steps all of them (82-90 %,
// profiles/r04/win_offset_probe.log)
#ifdef MI3D_WIN_DIAG
#define MI3D_WIN_HIT(COUNT_, cnt_) do { if (COUNT_) (cnt_).le_steps3d++; } while (0)
#define MI3D_WIN_ANY(COUNT_, cnt_) do { if (COUNT_) (cnt_).le_steps++; } while (0)
#else
#define MI3D_WIN_HIT(COUNT_, cnt_) do { } while (0)
#define MI3D_WIN_ANY(COUNT_, cnt_) do { } while (0)
#endif

// -DMI3D_CLEAR_STEPS: voxel steps through cloud-free voxels counted in le_steps, those that end the walk there in le_steps3d (12.1 of the
// 61.5 steps per photon on the bench scene: an empty-space structure would not pay)
#ifdef MI3D_CLEAR_STEPS
#define MI3D_DIAG_CLEAR_STEP(COUNT_, cnt_, ks_, ends_) do { if ((COUNT_) && (ks_) == 0.0f) { (cnt_).le_steps++; if (ends_) (cnt_).le_steps3d++; } } while (0)
#else
#define MI3D_DIAG_CLEAR_STEP(COUNT_, cnt_, ks_, ends_) do { } while (0)
#endif

// -DMI3D_ABL_NOEMITSTORE (results wrong): the event-writing loop without its stores -- what the event records cost it (21 %,
// profiles/r03, `kt_noemit`)
#ifdef MI3D_ABL_NOEMITSTORE
#define MI3D_DIAG_NOEMITSTORE 1
#define MI3D_DIAG_KEEP11(a, b, c, d, e, f, g, h, i, j, k) asm volatile("" ::"v"(a), "v"(b), "v"(c), "v"(d), "v"(e), "v"(f), "v"(g), "v"(h), "v"(i), "v"(j), "v"(k))
#else
#define MI3D_DIAG_NOEMITSTORE 0
#endif
