// pencil_launch.hpp -- the host side of the Gram walks, once: gram_pencil with its run-time and Tangent instantiations
// (gram_mfma.hpp), the patch-of-pencils walks (gram_patch.hpp, gram_patch3.hpp) and gram_p3_element behind try_gram_mfma.
// One loop over segment counts (segment_search), one LDS sum of a pencil launch (pencil_launch_lds), one plan per colour launch
// (pencil_plan: what launch_pencils launches and pencil_box_cost costs), one list of passes (assembly_passes), one switchboard from
// run-time values to the template arguments of gram_pencil, one runner of the patch walks, one place for the names and figures, and
// the Tangent's module of a built-in state form (state_pencil_module, for compute() of engine.hip).
// Host only, the main unit only: nothing here reaches the run-time compiler.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include "gram_mfma.hpp"
#include "gram_patch.hpp"
#include "gram_patch3.hpp"
#include "gram_rows3.hpp"
#include "boundary_loads.hpp"
#include "pencil_stamps.hpp"
#include "module_launch.hpp"

namespace igx {

// a run-time form's instantiation of the walk (rtc.hpp): the module function for this driver / degree / geometry, its parameters
// ... or a compiled-in instantiation for a built-in form (state_pencil: kfn, its extra LDS, flops per element for the roofline line)
typedef void (*PencilKernel)(SpaceDev, OutDev, PencilArgs, ParamsDev);
// one pass of an assembly that comes in several (the elements next to the upper faces first, a mark for the exchange after each):
// {lo, hi, blocked} of the first-touch rule on axes Y and X of the axis-0 walk (first_touch_axis), and, when the pass is a part of the
// walk axis, how its ends join the others.  The default is the one pass of an assembly.
struct PencilPass { int fty[3] = {0, 0x7fffffff, 0x7fffffff}, ftx[3] = {0, 0x7fffffff, 0x7fffffff}; int halo_lo = -1; bool open_hi = false; };
struct PencilModule { hipFunction_t fn = nullptr; ParamsDev prm; std::string name; PencilKernel kfn = nullptr; size_t extra_lds = 0; bool state = false; double flop_per_element = 0;
                      bool state_geo = false;         // state_geo: the instantiation is state_pencil_geo (evaluates the geometry itself)
                      int pack = 0;                   // pack: packed tiles, the window of band rows in the place of the hold areas (1: state_pencil_k; 2: the compact window, state_pencil_geo_k)
                      const void *patch_kfn = nullptr; };      // gram_patch.hpp: state_patch_p2<Form> of the same form (p = 2, no geometry)

constexpr size_t LDS_MAX = (size_t)160 * 1024;
static inline int nseg_min_lds(int nw) { return std::max(1, (nw + 159) / 160); }
// a launch that could not be made (the LDS of the chosen segments beyond the device's, a module launch refused): try_gram_mfma
// reports it instead of the generic "kernel launch failed" of a later call
inline const char *&pencil_launch_error() { static thread_local const char *e = nullptr; return e; }
static inline int pencil_cus() {
  static const int ncu = [] { int dev = 0; hipDeviceProp_t pr; return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256; }();
  return ncu;
}

// ------------------------------------------------------------------ segments
// Segments of one launch (`units` workgroups per segment, nw walked elements): as few as possible -- every segment re-computes P halo
// elements -- but enough workgroups for the CUs.  For n = n_first .. nw / 2 segments of len = ceil(nw / n) elements (ns = ceil(nw / len)
// of them; down to two elements per segment) whose LDS lds_at(len + 3 elements) fits, the count with the least
// cost_at(len, ns, lds, workgroups on the fullest of the ncu CUs).
// (round 6: segments down to two elements.  A pencil's elements are sequential -- 12.8 us of MFMA issue each at p = 3 -- so on a small
//  mesh, where the CUs outnumber the workgroups, the walk's LENGTH is the launch's duration: 32^3 took 365 us per launch with the old
//  floor of eight elements per segment, 250 us with four.)
// The callers differ, on record (profiles/pencil_launch.txt): where the search starts; c.n when nothing fits (past_misfits: one past
// the last count that did not fit, else what the caller put there); how much less a later count must cost to win (tie).  A second
// search over the same SegmentChoice competes with the first; returns whether it won.
struct SegmentChoice { int n; double cost = 0; bool found = false; };
template <class LdsAt, class CostAt>
static inline bool segment_search(SegmentChoice &c, int nw, long long units, int ncu, int n_first, bool past_misfits, double tie, LdsAt lds_at, CostAt cost_at) {
  bool won = false;
  for (int n = n_first; n <= std::max(n_first, nw / 2); ++n) {
    const int len = (nw + n - 1) / n, ns = (nw + len - 1) / len;
    const size_t lds = lds_at(len + 3);
    if (lds > LDS_MAX) { if (past_misfits && !c.found) c.n = n + 1; continue; }
    const double cost = cost_at(len, ns, lds, (units * ns + ncu - 1) / ncu);
    if (!c.found || cost < c.cost * (1.0 - tie)) { c.found = won = true; c.cost = cost; c.n = n; }
  }
  return won;
}
// IGX_NSEG (experiment switch): the forced count, between the search's first count and two elements per segment
static inline int segments_forced(int env_nseg, int nw, int n_first) { return std::max(n_first, std::min(env_nseg, std::max(1, nw / 2))); }

// the LDS of a pencil launch of wpb wavefronts: tables for ne elements, the hold areas of the axis-0 walk (per wavefront; they come
// last when there is no metric area), the metric area, and `extra`: the module's own plus pencil_win_extra
static inline size_t pencil_launch_lds(int ne, int P, bool geo, bool walk0, int wpb, size_t extra) {
  return pencil_lds_bytes(ne, geo, wpb) + (walk0 ? pencil_hold_bytes(P) * wpb / 8 : 0) + (geo ? pencil_geo_bytes() : 0) + extra;
}
// One 8-pencil workgroup per CU at a time (LDS; two where the tables are small), so a launch takes ceil(workgroups / slots) rounds of
// (segment length + halo + 1): the "+ 1" is a workgroup's set-up in units of a step.  Returns the count; *cost = rounds x length
// (element-steps of the launch's critical path).
// (next to the metric areas of a mapped geometry the tables of 128 + 3 elements no longer fit: 256^3 takes three segments there)
static inline int pencil_segments(long long pencils, int nw, int P, bool geo, bool walk0, size_t extra_lds, bool halo_always, int ncu, long long *cost_out = nullptr, int wpb = 8) {
  SegmentChoice c{nseg_min_lds(nw)};
  segment_search(c, nw, (pencils + wpb - 1) / wpb, ncu, c.n, true, 0.0,
                 [&](int ne) { return pencil_launch_lds(ne, P, geo, walk0, wpb, extra_lds); },
                 [&](int len, int ns, size_t lds, long long per_cu) {
                   const long long resident = std::max<long long>(1, std::min<long long>(2, (long long)LDS_MAX / (long long)lds));
                   return (double)(((per_cu + resident - 1) / resident) * (len + ((ns > 1 || halo_always) ? P : 0) + 1));
                 });
  if (cost_out) *cost_out = c.found ? (long long)c.cost : 0;
  return c.n;
}
// waves per workgroup of the axis-0 walk: twelve for the free-running p = 2 kernel on the identity geometry (gram_pencil_w6), else eight
static inline int pencil_wpb(const Space &s, int P, bool geo, bool fixt, bool has_mod) {
  static const int wpb_env = [] { const char *e = getenv("IGX_WPB"); return e ? atoi(e) : 0; }();
  const int free_run = s.env.free_run >= 0 ? s.env.free_run : ((P == 2 && !geo && !has_mod) ? 1 : 0);
  return (P == 2 && !geo && !fixt && !has_mod && free_run && wpb_env != 8) ? 12 : 8;
}
// ... and whether that kernel packs the element's 27 functions into two tiles (pencil_mfma_p2k; IGX_P2_PACK=0: the layer-pair tiles)
static inline bool pencil_p2_pack(const Space &s, int P, bool geo, bool fixt, bool has_mod) {
  return s.env.p2_pack != 0 && pencil_wpb(s, P, geo, fixt, has_mod) == 12;
}
// LDS the packed p = 2 walks take on top of the hold areas pencil_launch_lds counts: the window of band rows in their place (about
// + 28 KB at eight waves, + 43 KB at twelve)
static size_t pencil_win_extra(const Space &s, int P, bool geo, bool fixt, const PencilModule *mod, int wpb) {
  const bool pack = pencil_p2_pack(s, P, geo, fixt, mod != nullptr) || (mod && mod->pack);
  if (!pack) return 0;
  const size_t win_bytes = (mod && mod->pack == 2) ? pencil_winc_bytes(wpb) : pencil_win_bytes(wpb);
  return win_bytes - pencil_hold_bytes(P) * wpb / 8;
}

// ------------------------------------------------------------------ the plan of one colour launch
// the walk of an assembly: axis W, degree P, geo = a mapped geometry or a module (the kernel evaluates a metric), the fix table
struct PencilPlan;
typedef void (*GramKernel)(SpaceDev, OutDev, PencilArgs);
typedef GramKernel (*GramKernelPick)(const PencilPlan &);
struct PencilWalk { int W = 0, P = 3; bool geo = false, fixt = false; const PencilModule *mod = nullptr; double forcing = 0; bool first_touch = false; GramKernelPick pick = nullptr; };
struct PencilPlan {
  PencilArgs pa; size_t lds = 0; unsigned grid = 0, block = 0;
  bool sf = false, w6 = false, pack = false;      // kernel variants (with pa.alias0 and, four-wave small mesh, pa.wpb == 4)
  long long seg_cost = 0;                         // pencil_segments' figure for this launch: what pencil_box_cost sums
};
// Colour (cx, cy) of the box bx in the pass `pass`.  Returns false when the colour has no pencil in the box.
static bool pencil_plan(const Space &s, const PencilWalk &w, const Box &bx, int cx, int cy, const PencilPass &pass, int ncu, PencilPlan &pl) {
  const int W = w.W, P = w.P, X = (W == 0) ? 1 : 0, Y = (W == 2) ? 1 : 2;
  const PencilModule *mod = w.mod;
  const int nw = bx.hi[W] - bx.lo[W];
  PencilArgs &pa = pl.pa; pa.forcing = w.forcing;
  pa.first_touch = (W == 0 && w.first_touch) ? 1 : 0; pa.nelx = s.elem_width[X]; pa.nely = s.elem_width[Y];
  pa.alias0 = (W == 0 && s.lay[0].alias) ? 1 : 0;
  pa.fty_lo = pass.fty[0]; pa.fty_hi = pass.fty[1]; pa.fty_blocked = pass.fty[2];
  pa.ftx_lo = pass.ftx[0]; pa.ftx_hi = pass.ftx[1]; pa.ftx_blocked = pass.ftx[2];
  pa.w_halo_lo = pass.halo_lo >= 0 ? pass.halo_lo : bx.lo[W]; pa.open_hi = pass.open_hi ? 1 : 0;
  if (!color_range(s.lay[X], cx, bx.lo[X], bx.hi[X], pa.ex_start, pa.ex_step, pa.ex_count)) return false;
  if (!color_range(s.lay[Y], cy, bx.lo[Y], bx.hi[Y], pa.ey_start, pa.ey_step, pa.ey_count)) return false;
  const long long pencils = (long long)pa.ex_count * pa.ey_count;
  pl.sf = P == 3 && !w.geo && !mod && s.env.gram_sumfact != 0;
  // p = 2 on the identity geometry: the flush is the longer phase and the rigid ping-pong makes the MFMA wave wait for it; left to
  // the SIMD's own arbitration the walk gains 5 % (128^3: 166.7 -> 175.3 M el/s).  Everything at p = 3, mapped geometries and
  // Tangents lose 6-8 % without the barriers (256^3: 64.8 -> 59.5).  IGX_FREE_RUN=0/1 overrides.
  pa.free_run = s.env.free_run >= 0 ? s.env.free_run : ((P == 2 && !w.geo && !(mod && mod->state)) ? 1 : 0);
  // ... and free of the pairing, six-wave workgroups put three waves on every SIMD (gram_pencil_w6; IGX_WPB=8: the eight-wave kernel)
  pl.w6 = W == 0 && pencil_wpb(s, P, w.geo, w.fixt, mod != nullptr) == 12;
  pa.wpb = pl.w6 ? 12 : 8;
  pl.pack = W == 0 && (pencil_p2_pack(s, P, w.geo, w.fixt, mod != nullptr) || (mod && mod->pack));      // (p = 2 on the identity geometry: packed tiles, the band rows combined in an LDS window instead of the hold areas)
  const size_t extra = (mod ? mod->extra_lds : 0) + (W == 0 ? pencil_win_extra(s, P, w.geo, w.fixt, mod, pa.wpb) : 0);
  const bool halo_always = (W == 0 && s.lay[0].alias) || (pass.halo_lo >= 0 && pass.halo_lo < bx.lo[W]);
  int nseg = pencil_segments(pencils, nw, P, w.geo, W == 0, extra, halo_always, ncu, &pl.seg_cost, pa.wpb);
  if (s.env.nseg > 0) nseg = segments_forced(s.env.nseg, nw, nseg_min_lds(nw));
  // Launches that do not fill the chip (small and medium meshes), the plain Gram walk: segments AND workgroup size from a model of the
  // step -- measured at p = 3 (profiles/r06_small_meshes.txt): a step of the walk takes 20 us with one wavefront on the SIMD (its
  // MFMAs, then its flush), 31 us with two (the ping-pong pair), 14 us per wavefront beyond; four-wavefront workgroups (one per SIMD,
  // free-running) spread the pencils over twice the CUs.  time = rounds x (length + halo + 1) x step(wavefronts per SIMD on the
  // fullest CU).  Large meshes come out as before (eight wavefronts, the fewest segments that fit the LDS).  IGX_SMALL_WPB=0: off;
  // IGX_NSEG forces the segments and keeps the eight.
  if (W == 0 && !w.geo && !mod && pa.wpb == 8 && s.env.small_wpb && s.env.nseg <= 0) {
    SegmentChoice c{nseg};
    for (int wc = 8; wc >= 4; wc -= 4) {
      const bool won = segment_search(c, nw, (pencils + wc - 1) / wc, ncu, nseg_min_lds(nw), false, 1e-9,
                                      [&](int ne) { return pencil_launch_lds(ne, P, false, true, wc, 0); },
                                      [&](int len, int ns, size_t lds, long long per_cu) {
                                        const long long rmax = std::max<long long>(1, std::min<long long>(wc == 8 ? 2 : 4, (long long)LDS_MAX / (long long)lds));
                                        const long long rounds = (per_cu + rmax - 1) / rmax, wsimd = std::min(per_cu, rmax) * wc / 4;
                                        double step = wsimd <= 1 ? 20.0 : (wsimd == 2 ? 31.0 : 14.0 * (double)wsimd);
                                        if (wc == 4 && wsimd >= 2) step *= 1.08;      // (without the barriers the p = 3 walk loses 6-8 % once wavefronts share a SIMD)
                                        return (double)rounds * (double)(len + ((ns > 1 || halo_always) ? P : 0) + 1) * step;
                                      });
      if (won && wc == 4) { pa.wpb = 4; pa.free_run = 1; }
    }
    nseg = c.n;
  }
  pa.seg_len = (nw + nseg - 1) / nseg; pa.nseg = (nw + pa.seg_len - 1) / pa.seg_len;
  pa.w_lo = bx.lo[W]; pa.w_hi = bx.hi[W];
  pa.blocks_per_seg = (int)((pencils + pa.wpb - 1) / pa.wpb);
  pa.ne_max = pa.seg_len + 3;
  pa.debug_noflush = s.env.debug_noflush; pa.debug_noprio = s.env.debug_noprio;
  pa.debug_buf = nullptr;
  pl.lds = pencil_launch_lds(pa.ne_max, P, w.geo, W == 0, pa.wpb, extra);
  pl.grid = (unsigned)(pa.blocks_per_seg * pa.nseg);
  pl.block = (unsigned)(pa.wpb * 64);      // (a module walks eight pencils per workgroup)
  return true;
}

// the colour launches of a box of elements in a pass: f(plan) for every colour that has a pencil in the box
template <class F>
static void for_each_plan(const Space &s, const PencilWalk &w, const Box &bx, const PencilPass &pass, int ncu, F f) {
  const int X = (w.W == 0) ? 1 : 0, Y = (w.W == 2) ? 1 : 2;
  for (int d = 0; d < 3; ++d) if (bx.hi[d] <= bx.lo[d]) return;
  for (int cy = 0; cy < s.lay[Y].ncolors; ++cy) for (int cx = 0; cx < s.lay[X].ncolors; ++cx) {
    PencilPlan pl;
    if (pencil_plan(s, w, bx, cx, cy, pass, ncu, pl) && !f(pl)) return;
  }
}
// what a pass of an assembly costs: pencil_segments' figure summed over the very plans launch_pencils makes, so that the model's
// workgroup size, resident-workgroup count and LDS-limited segment lengths are those of the launches (without the small-mesh model
// and IGX_NSEG, which that figure never saw)
static long long pencil_box_cost(const Space &s, const PencilWalk &w, const Box &bx, const PencilPass &pass, int ncu) {
  long long total = 0;
  for_each_plan(s, w, bx, pass, ncu, [&](const PencilPlan &pl) { total += pl.seg_cost; return true; });
  return total;
}

// ------------------------------------------------------------------ the kernel switchboard
// the variant of gram_pencil<SYSTEM, W, P, GEO, RAT, FIXT> a plan asks for
template <bool SYSTEM, int W, int P, bool GEO, bool RAT, bool FIXT>
static GramKernel gram_pencil_kernel(const PencilPlan &pl) {
  constexpr bool SFOK = P == 3 && !GEO;      // the sum-factorised Gram walk (pencil_mfma_sf; IGX_GRAM_SUMFACT=0: pencil_mfma)
  const bool sf = pl.sf, alias0 = pl.pa.alias0 != 0;
  GramKernel kern = gram_pencil<SYSTEM, W, P, GEO, RAT, FIXT>;
  if constexpr (SFOK && W != 0) { if (sf) kern = gram_pencil<SYSTEM, W, P, GEO, RAT, FIXT, -1, true>; }
  if constexpr (W == 0 && !GEO) {
    if (sf) kern = alias0 ? gram_pencil<SYSTEM, W, P, GEO, RAT, FIXT, 1, SFOK> : gram_pencil<SYSTEM, W, P, GEO, RAT, FIXT, 0, SFOK>;
    else kern = alias0 ? gram_pencil<SYSTEM, W, P, GEO, RAT, FIXT, 1> : gram_pencil<SYSTEM, W, P, GEO, RAT, FIXT, 0>;
  }
  if constexpr (W == 0 && P == 2 && !GEO && !FIXT) {
    if (pl.pack) kern = alias0 ? gram_pencil_w6<SYSTEM, P, 1, true> : gram_pencil_w6<SYSTEM, P, 0, true>;
    else if (pl.w6) kern = alias0 ? gram_pencil_w6<SYSTEM, P, 1> : gram_pencil_w6<SYSTEM, P, 0>;
  }
  return kern;
}
// Run-time values to template arguments, in one place.  The library holds 22 instantiations and this admits exactly those: on the
// axis-0 walk every driver / degree / metric combination in which a fix table comes with the System driver and rational weights with
// a metric (geometry + fix table 4, geometry or module 8, fix table alone 2, plain 4); on axes 1 and 2 the plain p = 3 walk (4).
template <class F> static inline void on_bool(bool b, F f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <class F> static inline void on_axis(int a, F f) {
  if (a == 0) f(std::integral_constant<int, 0>{}); else if (a == 1) f(std::integral_constant<int, 1>{}); else f(std::integral_constant<int, 2>{});
}
static GramKernelPick gram_pencil_switchboard(bool sys, int walk_axis, int deg, bool geo, bool rat, bool fixt) {
  GramKernelPick pick = nullptr;
  on_bool(sys, [&](auto SYS) { on_axis(walk_axis, [&](auto W) { on_bool(deg == 3, [&](auto P3) { on_bool(geo, [&](auto GEO) { on_bool(rat, [&](auto RAT) { on_bool(fixt, [&](auto FIXT) {
    constexpr bool s_ = decltype(SYS)::value, g_ = decltype(GEO)::value, r_ = decltype(RAT)::value, f_ = decltype(FIXT)::value;
    constexpr int w_ = decltype(W)::value, p_ = decltype(P3)::value ? 3 : 2;
    if constexpr (w_ == 0 ? ((!f_ || s_) && (!r_ || g_)) : (p_ == 3 && !g_ && !r_ && !f_)) pick = gram_pencil_kernel<s_, w_, p_, g_, r_, f_>;
  }); }); }); }); }); });
  return pick;
}

// ------------------------------------------------------------------ launches
template <bool SYSTEM>
static void launch_elements(const Space &s, const SpaceDev &S, const OutDev &out, hipStream_t stream, const Box &bx, const GramArgs &g0, int &launches) {
  for (int d = 0; d < 3; ++d) if (bx.hi[d] <= bx.lo[d]) return;
  for (int c2 = 0; c2 < s.lay[2].ncolors; ++c2) for (int c1 = 0; c1 < s.lay[1].ncolors; ++c1) for (int c0 = 0; c0 < s.lay[0].ncolors; ++c0) {
    const int cc[3] = {c0, c1, c2};
    ColorRange cr; bool ok = true;
    for (int d = 0; d < 3 && ok; ++d) ok = color_range(s.lay[d], cc[d], bx.lo[d], bx.hi[d], cr.start[d], cr.step[d], cr.count[d]);
    if (!ok) continue;
    GramArgs ga = g0; ga.nwaves = cr.count[0] * cr.count[1] * cr.count[2];
    hipLaunchKernelGGL((gram_p3_element<SYSTEM>), dim3((unsigned)((ga.nwaves + 3) / 4)), dim3(256), 0, stream, S, out, cr, ga);
    launches++;
  }
}

// the colour launches of a box of elements: plan, pick the kernel, launch
static void launch_pencils(const Space &s, const SpaceDev &S, const OutDev &out, hipStream_t stream, const PencilWalk &w, const Box &bx, const PencilPass &pass, int &launches) {
  const PencilModule *mod = w.mod;
  for_each_plan(s, w, bx, pass, pencil_cus(), [&](PencilPlan &pl) {
    PencilArgs &pa = pl.pa;
    static StampGate gate;
    const bool dbg_t = gate.due(s);
    if (dbg_t) stamps_alloc(pa, pencil_stamp_count(pa));
    if (pl.lds > LDS_MAX) { pencil_launch_error() = "the pencil walk's tables do not fit the 160 KB of LDS for any segment length"; return false; }
    if (mod && mod->kfn) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mod->kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
      hipLaunchKernelGGL(mod->kfn, dim3(pl.grid), dim3(pl.block), pl.lds, stream, S, out, pa, mod->prm);
    } else if (mod) {      // form_pencil<SYSTEM, P, IDENT, RAT, UserForm> of a run-time form: a module function (rtc.hpp)
      struct { SpaceDev S; OutDev out; PencilArgs pa; ParamsDev prm; } args;
      memset(&args, 0, sizeof(args));
      args.S = S; args.out = out; args.pa = pa; args.prm = mod->prm;
      if (module_launch(mod->fn, pl.grid, pl.block, pl.lds, stream, args) != hipSuccess) { pencil_launch_error() = "launch of the run-time instantiation of the pencil walk failed"; return false; }
    } else {
      const GramKernel kern = w.pick(pl);
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
      hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(pl.block), pl.lds, stream, S, out, pa);
    }
    if (dbg_t) report_pencil_stamps(stamps_fetch(stream, pa, pencil_stamp_count(pa)), pa);      // (cycle stamps of the ping-pong phases: diagnostic only)
    launches++;
    return true;
  });
}

// ---- the patch walks: the arguments of the launch of colour (cx, cy) -- the colours are launched cy-major, patch_first_touch knows the
// order -- its segments and its LDS (lds_bytes(ne_max) of the kernel).  Returns whether the colour has patches to launch;
// pencil_launch_error is set (and nothing is to be launched) when no segment length fits the LDS.
// Segments: the count with the fewest rounds x (length + halo + set-up) over the slots for resident workgroups.
template <class G, class LdsBytes>
static bool patch_colour_args(const Space &s, int cx, int cy, double forcing, bool first_touch, LdsBytes lds_bytes, const char *no_fit, int ncu, PatchArgs &A, size_t &lds) {
  const int nx = s.elem_width[1], ny = s.elem_width[2], nw = s.elem_width[0];
  const int npx = (nx + G::MX - 1) / G::MX, npy = (ny + G::MY - 1) / G::MY;
  memset(&A, 0, sizeof(A));
  A.px_start = cx; A.px_step = G::SX; A.px_count = (npx - cx + G::SX - 1) / G::SX;
  A.py_start = cy; A.py_step = G::SY; A.py_count = (npy - cy + G::SY - 1) / G::SY;
  if (A.px_count <= 0 || A.py_count <= 0) return false;
  PencilArgs &pa = A.pa;
  pa.forcing = forcing; pa.first_touch = first_touch ? 1 : 0;
  pa.nelx = nx; pa.nely = ny; pa.w_lo = 0; pa.w_hi = nw; pa.w_halo_lo = 0; pa.open_hi = 0; pa.wpb = G::W;
  const long long patches = (long long)A.px_count * A.py_count;
  SegmentChoice c{1};
  segment_search(c, nw, patches, ncu, 1, false, 0.0, lds_bytes,
                 [&](int len, int ns, size_t lds_n, long long per_cu) {
                   const long long resident = G::SLOTS_FROM_LDS ? std::max<long long>(1, (long long)LDS_MAX / (long long)lds_n) : 1;
                   return (double)(((per_cu + resident - 1) / resident) * (len + (ns > 1 ? G::P : 0) + 1));
                 });
  if (s.env.nseg > 0) c.n = segments_forced(s.env.nseg, nw, 1);
  pa.seg_len = (nw + c.n - 1) / c.n; pa.nseg = (nw + pa.seg_len - 1) / pa.seg_len;
  pa.blocks_per_seg = (int)patches; pa.ne_max = pa.seg_len + 3;
  lds = lds_bytes(pa.ne_max);
  if (lds > LDS_MAX) { pencil_launch_error() = no_fit; return false; }
  return true;
}

// the launches of an assembly: SX x SY colours of patches, cy-major (the first-touch rule knows the order).  launch(cx, cy, A, lds)
// makes the colour's launch; pencil_launch_error is set when no segment length fits the LDS
template <class G, class LdsBytes, class Launch>
static void launch_patch_colours(const Space &s, double forcing, bool first_touch, LdsBytes lds_bytes, const char *no_fit, const void *kern, int &launches, Launch launch) {
  for (int cy = 0; cy < G::SY; ++cy) for (int cx = 0; cx < G::SX; ++cx) {
    PatchArgs A; size_t lds = 0;
    if (!patch_colour_args<G>(s, cx, cy, forcing, first_touch, lds_bytes, no_fit, pencil_cus(), A, lds)) { if (pencil_launch_error()) return; continue; }
    (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    launch(cx, cy, A, lds, dim3((unsigned)((long long)A.pa.blocks_per_seg * A.pa.nseg)), dim3(G::W * 64));
    launches++;
  }
}
// gram_patch.hpp (round 6): the p = 2 walk of 4 x 3 patches of pencils
static void launch_patches_p2(const Space &s, const SpaceDev &S, const OutDev &out, hipStream_t stream, int &launches, double forcing, bool first_touch) {
  using G = PatchP2;
  auto kern = out.op == OP_SYSTEM ? gram_patch_p2<true> : gram_patch_p2<false>;
  launch_patch_colours<G>(s, forcing, first_touch, patch_lds_bytes, "the patch walk's tables do not fit the LDS", reinterpret_cast<const void *>(kern), launches,
                          [&](int cx, int cy, PatchArgs &A, size_t lds, dim3 grid, dim3 block) {
    static StampGate gate;      // -DIGX_DEBUG, IGX_DEBUG_TIMING=n: the n-th patch launch of the process is stamped
    const bool dbg_t = gate.due(s);
    const size_t dbg_n = patch2_stamp_count(A.pa, G::W);
    if (dbg_t) stamps_alloc(A.pa, dbg_n);
    hipLaunchKernelGGL(kern, grid, block, lds, stream, S, out, A);
    if (dbg_t) report_patch2_stamps(stamps_fetch(stream, A.pa, dbg_n), A.pa, G::W, cx, cy);
  });
}
// ... of a Tangent (Jacobian / IJacobian): `kernel` = state_patch_p2<Form>
typedef void (*StatePatchKernel)(SpaceDev, OutDev, PatchArgs, ParamsDev);
static void launch_state_patches_p2(const Space &s, const SpaceDev &S, const OutDev &out, hipStream_t stream, int &launches, bool first_touch, const void *kernel, const ParamsDev &prm) {
  StatePatchKernel kern = reinterpret_cast<StatePatchKernel>(const_cast<void *>(kernel));
  launch_patch_colours<StatePatchP2>(s, 0.0, first_touch, spatch_lds_bytes, "the patch walk's tables do not fit the LDS", kernel, launches,
                                     [&](int, int, PatchArgs &A, size_t lds, dim3 grid, dim3 block) { hipLaunchKernelGGL(kern, grid, block, lds, stream, S, out, A, prm); });
}
// gram_patch3.hpp (round 8): the p = 3 walk of MX x MY patches of pencils
// ... its ticket counters (round 12): one per colour launch, each on a 128-byte line of its own, in memory the engine owns.  All of an
// assembly's counters are zeroed by one memset on the engine's stream ahead of its first launch that takes tickets: stream order puts
// it behind the previous assembly's last launch and before this one's, and a counter belongs to one engine -- a ticket of an earlier assembly,
// or of another engine, cannot be met.
constexpr int PATCH3_COUNTER_INTS = 32;
template <int MX, int MY> constexpr size_t patch3_counter_bytes() { return (size_t)Patch3<MX, MY>::SX * Patch3<MX, MY>::SY * PATCH3_COUNTER_INTS * sizeof(int); }
// workgroups of the kernel the device holds at once: the occupancy of its block and LDS size times the CUs
// (asked once per kernel and LDS size: the six launches of an assembly, and the assemblies of a run, share the answer)
static int patch3_resident(const void *kern, int block, size_t lds) {
  static thread_local std::map<std::pair<const void *, size_t>, int> known;
  int &per_cu = known[{kern, lds}];
  if (per_cu < 1 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, block, lds) != hipSuccess || per_cu < 1)) { (void)hipGetLastError(); per_cu = 1; }
  return per_cu * pencil_cus();
}
// The launch of a colour: IGX_PATCH3_PERSIST=1 (default) min(items, resident workgroups) workgroups that take their items by ticket --
// where the device holds every item at once a ticket has nothing to hand out, and the launch is the one below; IGX_PATCH3_GRID=n: n
// workgroups with tickets whatever the items (tests, experiments).  IGX_PATCH3_PERSIST=0: one workgroup per item.
template <int MX, int MY>
static void launch_patches_p3(const Space &s, const SpaceDev &S, const OutDev &out, hipStream_t stream, int &launches, double forcing, bool first_touch, int *counters) {
  using G = Patch3<MX, MY>;
  auto kern = out.op == OP_SYSTEM ? gram_pencil_patch3<true, MX, MY, false> : gram_pencil_patch3<false, MX, MY, false>;      // one workgroup per item
  auto kern_t = out.op == OP_SYSTEM ? gram_pencil_patch3<true, MX, MY, true> : gram_pencil_patch3<false, MX, MY, true>;      // tickets
  const bool persist = s.env.patch3_persist != 0;
  if (persist && !counters) { pencil_launch_error() = "the p = 3 patch walk's ticket counters are missing"; return; }
  bool zeroed = false;      // (the memset goes ahead of the first launch that takes tickets: an assembly without one makes none)
  launch_patch_colours<G>(s, forcing, first_touch, patch3_lds_bytes<MX, MY>, "the p = 3 patch walk's tables do not fit the LDS", reinterpret_cast<const void *>(kern), launches,
                          [&](int cx, int cy, PatchArgs &A, size_t lds, dim3 grid, dim3 block) {
    static StampGate gate;      // -DIGX_DEBUG, IGX_DEBUG_TIMING=n: the n-th launch of the process is stamped (as launch_patches_p2)
    const bool dbg_t = gate.due(s);
    const size_t dbg_n = patch3_stamp_count(A.pa, G::W);
    if (dbg_t) stamps_alloc(A.pa, dbg_n);
    Patch3Tickets K{nullptr, s.env.patch3_order};
    if (persist) {
      const long long items = grid.x, resident = patch3_resident(reinterpret_cast<const void *>(kern_t), (int)block.x, lds);
      if (s.env.patch3_grid > 0 || items > resident) {
        if (!zeroed) { (void)hipMemsetAsync(counters, 0, patch3_counter_bytes<MX, MY>(), stream); zeroed = true; }
        K.counter = counters + (cy * G::SX + cx) * PATCH3_COUNTER_INTS;
        grid.x = (unsigned)(s.env.patch3_grid > 0 ? s.env.patch3_grid : std::min(items, resident));
      }
    }
    if (K.counter) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern_t), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kern_t, grid, block, lds, stream, S, out, A, K);
    } else hipLaunchKernelGGL(kern, grid, block, lds, stream, S, out, A, K);
    if (dbg_t) report_patch3_stamps(stamps_fetch(stream, A.pa, dbg_n), A.pa, G::W, cx, cy);
  });
}

// one rank, no axis wrapped inside it, one new node per element on axes 1 and 2 (a patch's nodes are consecutive)
static bool patch_walk_covers(const Space &s) {
  if (s.proc_sizes[0] * s.proc_sizes[1] * s.proc_sizes[2] != 1) return false;
  for (int d = 0; d < 3; ++d) if (s.lay[d].alias) return false;
  for (int d = 1; d < 3; ++d)
    for (int e = 0; e + 1 < s.elem_width[d]; ++e) if (s.basis[d].offset[s.elem_start[d] + e + 1] != s.basis[d].offset[s.elem_start[d] + e] + 1) return false;
  return true;
}

// the p = 3 patch walk's shape (pencils on axes 1, 2) and where it is the automatic choice (IGX_PATCH3=1).  Measured against the pencil
// walk on cubes of 16^3 to 256^3 elements (System driver, profiles/r08_gram_patch_p3.txt) it was faster at every size, 1.57x at 16^3 and
// 1.6-1.9x from 24^3 to 256^3; below 16^3 nothing was measured and the pencil walk stays.
constexpr int PATCH3_MX = 4, PATCH3_MY = 2;
constexpr long long PATCH3_MIN_ELEMENTS = 16 * 16 * 16;
static bool patch3_pays(const Space &s) {
  return (long long)s.elem_width[0] * s.elem_width[1] * s.elem_width[2] >= PATCH3_MIN_ELEMENTS;
}

// gram_rows3.hpp (round 13): the p = 3 matrix gathered by rows.  It covers what the patch walk covers, on axes that are not periodic and
// bring one new node per element, axis 0 included (a node's elements are then the four below it on every axis).
static bool rows3_covers(const Space &s) {
  if (!patch_walk_covers(s)) return false;
  for (int d = 0; d < 3; ++d) {
    if (s.axis[d].periodic || s.lay[d].gwidth != s.elem_width[d] + 3 || s.lay[d].nrow != s.lay[d].gwidth) return false;
    for (int e = 0; e + 1 < s.elem_width[d]; ++e) if (s.basis[d].offset[s.elem_start[d] + e + 1] != s.basis[d].offset[s.elem_start[d] + e] + 1) return false;
  }
  return true;
}
// ... where it is the automatic choice (IGX_ROWS3=1): the smallest measured cube at which both alternated pairs were faster than the
// patch walk (profiles/r13_rows3.txt)
constexpr long long ROWS3_MIN_ELEMENTS = 48LL * 48 * 48;
static bool rows3_pays(const Space &s) {
  return (long long)s.elem_width[0] * s.elem_width[1] * s.elem_width[2] >= ROWS3_MIN_ELEMENTS;
}
// ... and where its full layers of regular tiles are staged in LDS and stored as contiguous spans (IGX_ROWS3_STAGE=1; 2: wherever the
// walk runs, 0: nowhere).  Never where the mesh has nothing to stage: a regular tile needs six elements on axes 1 and 2, a full layer four
// on axis 0.  The default: from the smallest measured cube at which staging was faster in both alternated pairs
// (profiles/r14_rows3_stores.txt: slower at 48^3 and 64^3, one pair each way at 96^3, 4-5 % faster at 128^3, 13 % at 256^3).  Only cubes
// were measured; the count of elements stands in for them, and a slab or a bar of as many elements was not.
constexpr long long ROWS3_STAGE_MIN_ELEMENTS = 128LL * 128 * 128;
static bool rows3_stages(const Space &s) {
  if (s.env.rows3_stage == 0 || s.elem_width[0] < 4 || s.elem_width[1] < 6 || s.elem_width[2] < 6) return false;
  return s.env.rows3_stage == 2 || (long long)s.elem_width[0] * s.elem_width[1] * s.elem_width[2] >= ROWS3_STAGE_MIN_ELEMENTS;
}
// Segments of node layers: as long as possible (an item stages its tables and forms its planes once: about two layers' worth of
// time), at most ROWS3_SEG_MAX layers, and shorter down to eight layers while the items are fewer than two per resident workgroup.
// IGX_NSEG forces the count (down to one layer per segment).
constexpr int ROWS3_SEG_MAX = 64;
static void rows3_segments(const Space &s, int nl0, long long tiles, long long resident, int &seg_len, int &nseg) {
  int n = (nl0 + ROWS3_SEG_MAX - 1) / ROWS3_SEG_MAX;
  while (tiles * n < 2 * resident && (nl0 + n) / (n + 1) >= 8) ++n;
  if (s.env.nseg > 0) n = std::max((nl0 + ROWS3_SEG_MAX - 1) / ROWS3_SEG_MAX, std::min(s.env.nseg, nl0));
  seg_len = (nl0 + n - 1) / n; nseg = (nl0 + seg_len - 1) / seg_len;
}
// One launch per assembly.  Where the items outnumber the resident workgroups (or IGX_ROWS3_GRID=n asks for n workgroups) they are
// taken by ticket from the first of the engine's counters, zeroed on the stream ahead of the launch; else one workgroup per item.
static void launch_rows3(const Space &s, const SpaceDev &S, const OutDev &out, hipStream_t stream, int &launches, double forcing, int *counters) {
  using R = Rows3;
  const bool sys = out.op == OP_SYSTEM;
  auto kern = sys ? gram_pencil_rows3<true, false> : gram_pencil_rows3<false, false>;
  auto kern_t = sys ? gram_pencil_rows3<true, true> : gram_pencil_rows3<false, true>;
  Rows3Args A; memset(&A, 0, sizeof(A));
  A.forcing = forcing;
  A.nel0 = s.elem_width[0]; A.nelx = s.elem_width[1]; A.nely = s.elem_width[2];
  A.nl0 = A.nel0 + 3; A.nnx = A.nelx + 3; A.nny = A.nely + 3;
  A.ntx = (A.nnx + R::TX - 1) / R::TX; A.nty = (A.nny + R::TY - 1) / R::TY;
  const long long tiles = (long long)A.ntx * A.nty;
  A.stage = rows3_stages(s) ? 1 : 0;
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern_t), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rows3_lds_bytes(ROWS3_SEG_MAX, A.stage != 0));
  const long long resident = patch3_resident(reinterpret_cast<const void *>(kern_t), R::NTHR, rows3_lds_bytes(ROWS3_SEG_MAX, A.stage != 0));
  rows3_segments(s, A.nl0, tiles, resident, A.seg_len, A.nseg);
  const size_t lds = rows3_lds_bytes(A.seg_len, A.stage != 0);
  const long long items = tiles * A.nseg;
  if (lds > LDS_MAX || items > INT_MAX) { pencil_launch_error() = "the p = 3 rows walk's items or tables are beyond the launch's limits"; return; }
  unsigned grid = (unsigned)items;
  if (s.env.rows3_grid > 0 || items > resident) {
    if (!counters) { pencil_launch_error() = "the p = 3 rows walk's ticket counter is missing"; return; }
    (void)hipMemsetAsync(counters, 0, patch3_counter_bytes<PATCH3_MX, PATCH3_MY>(), stream);
    A.counter = counters;
    grid = (unsigned)(s.env.rows3_grid > 0 ? s.env.rows3_grid : resident);
  }
  const auto k = A.counter ? kern_t : kern;
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, dim3(grid), dim3(R::NTHR), lds, stream, S, out, A);
  launches++;
}

// ------------------------------------------------------------------ the Tangent's module
// the walk's instantiation for the Tangent of a built-in state form: no geometry (state_pencil; p = 2 with packed tiles state_pencil_k,
// with the Residual on the same MFMAs state_pencil_kr, and state_patch_p2 for the patch walk), a mapped geometry at p = 2
// (state_pencil_geo: the map's second derivatives and the state's in one sum factorisation; packed state_pencil_geo_k).
// pack: 4 MFMAs per feature and k-step instead of 9 (IGX_P2_PACK=0: the layer-pair tiles).  flop_per_element: executed, k-steps x
// tiles x features.
template <class Form>
static void state_module_of(PencilModule &st, const char *name, int deg, bool geo, bool rat, bool pack, bool fused) {
  st.name = name; st.state = true; st.state_geo = geo;
  st.flop_per_element = 2048.0 * Form::PENCIL_NFEAT * (pack ? 7 * 4 : (deg == 2 ? 7 * 9 : 16 * 16));
  if (geo) {
    if (pack) st.kfn = rat ? state_pencil_geo_k<true, Form> : state_pencil_geo_k<false, Form>;
    else st.kfn = rat ? state_pencil_geo<2, true, Form> : state_pencil_geo<2, false, Form>;
    st.pack = pack ? 2 : 0;
    st.extra_lds = pencil_state_bytes() + pencil_sgeo_bytes() - pencil_geo_bytes();
    return;
  }
  if (pack) st.kfn = fused ? state_pencil_kr<Form> : state_pencil_k<Form>;
  else st.kfn = deg == 2 ? state_pencil<2, Form> : state_pencil<3, Form>;
  st.pack = pack ? 1 : 0;
  if (pack && fused) st.name += "+Residual";
  if (pack && !fused) st.patch_kfn = reinterpret_cast<const void *>(state_patch_p2<Form>);
  st.extra_lds = pencil_state_bytes() + (fused ? (size_t)8 * (RWIN_DOUBLES + 128) * 8 : 0);      // fused: the Residual's ring and the scratch of its u_t sums, per wavefront
}
// ... of the space's form for a Jacobian / IJacobian driver, where the walk is the choice (IGX_STATE_PENCIL, IGXSetKernel 0 or 2);
// false: the form has none (fused: the call forms IFunction + IJacobian in one pass)
static bool state_pencil_module(const Space &s, int op, int kernel_choice, bool fused, PencilModule &st) {
  memset(&st.prm, 0, sizeof(st.prm));
  const int deg = s.axis[0].p;
  const bool geo = s.nsd == 3;
  if (!((op == OP_JACOBIAN || op == OP_IJACOBIAN) && s.dim == 3 && (geo || s.nsd == 0) && s.env.state_pencil && (kernel_choice == 0 || kernel_choice == 2))) return false;
  if (geo ? deg != 2 : (deg != 2 && deg != 3)) return false;
  const bool pack = deg == 2 && s.env.p2_pack != 0;
  if (s.form == IGX_FORM_CAHNHILLIARD) state_module_of<FormCahnHilliard<3>>(st, "CahnHilliard", deg, geo, s.rational != 0, pack, fused);
  else if (s.form == IGX_FORM_BRATU) state_module_of<FormBratu<3>>(st, "Bratu", deg, geo, s.rational != 0, pack, fused);
  else return false;
  st.prm = params_of(s);
  return true;
}

// ------------------------------------------------------------------ the passes of an assembly
// Upper faces first (multi-rank, axis-0 walk): the upper half of axis 2 in every colour, a mark for the exchange (slab_done); of
// what is left, the upper half of axis 1, a mark (face_done(1)); then the upper half of every remaining pencil -- the upper face
// of axis 0: segments of their own, the first of which re-computes p halo elements and owns the rows from its first layer on --
// and a mark (face_done(0)); then the rest, whose last segment owns no row past its elements.  The ghost rows of a face get nothing from the passes after its mark: its messages travel under them (comm.hpp).
// First touch makes the launch order part of the result: per pass the rule applies to the elements of that pass alone, and an
// entry an earlier pass reaches as well is only added to (PencilPass::fty / ftx).
struct WalkPass { Box box; PencilPass pp; int mark = -1; };      // mark: the axis whose upper face is complete after the pass (-1: none)
struct WalkPasses { WalkPass p[4]; int n = 0; };
// can[d]: the upper face of axis d gets a pass of its own, the elements [cut[d], n_d) of what the earlier passes left of the box P
static WalkPasses walk_passes(const Box &P, const bool can[3], const int cut[3]) {
  WalkPasses L;
  Box R = P;
  auto add = [&](const Box &b, int mark, bool face0, bool rest0) {
    WalkPass &w = L.p[L.n++];
    w.box = b; w.mark = mark;
    w.pp.fty[0] = b.lo[2]; w.pp.fty[1] = b.hi[2]; w.pp.fty[2] = (can[2] && b.hi[2] <= cut[2]) ? cut[2] : 0x7fffffff;
    w.pp.ftx[0] = b.lo[1]; w.pp.ftx[1] = b.hi[1]; w.pp.ftx[2] = (can[1] && b.hi[1] <= cut[1]) ? cut[1] : 0x7fffffff;
    w.pp.halo_lo = face0 ? 0 : -1; w.pp.open_hi = rest0;
  };
  for (int d = 2; d >= 0; --d) if (can[d]) { Box F = R; F.lo[d] = cut[d]; R.hi[d] = cut[d]; add(F, d, d == 0, false); }
  add(R, -1, false, can[0]);
  return L;
}

// The passes of the pencil walk over the box P of a rank's elements: faces first where the rank has upper neighbours, the caller marks
// for their exchange (marks2: of axis 2, slab_done; marks01: of axes 0 and 1, face_done) and the walk is the axis-0 walk over the
// whole rank; else the one pass.
static WalkPasses assembly_passes(const Space &s, const PencilWalk &pw, const Box &P, bool marks2, bool marks01, int ncu) {
  const int deg = pw.P, n0 = s.elem_width[0], n1 = s.elem_width[1], n2 = s.elem_width[2];
  WalkPasses one; one.n = 1; one.p[0].box = P;
  auto upper = [&](int d) { return s.proc_sizes[d] > 1 && (s.proc_ranks[d] < s.proc_sizes[d] - 1 || s.axis[d].periodic); };
  const bool whole = pw.W == 0 && P.lo[0] == 0 && P.hi[0] == n0 && P.lo[1] == 0 && P.hi[1] == n1 && P.lo[2] == 0 && P.hi[2] == n2;
  const bool can[3] = {marks01 && whole && upper(0) && n0 >= 16 && !s.lay[0].alias,
                       marks01 && whole && upper(1) && n1 >= 2 * (deg + 1) && !s.lay[1].alias,
                       marks2 && whole && upper(2) && n2 >= 2 * (deg + 1)};
  const int cut[3] = {std::max(8, face_cut(n0, deg)), face_cut(n1, deg), face_cut(n2, deg)};      // (thick passes: pencil_common.hpp)
  if (!(can[2] || can[1] || can[0])) return one;
  const WalkPasses passes = walk_passes(P, can, cut);
  if (s.env.overlap < 0) {
    // IGX_OVERLAP unset: make the passes only when they cost less than what they hide.  Cost: the launcher's own measure (rounds x
    // segment length, summed over the launches) of the passes against one pass, times the time of an element-step.  Gain: the
    // largest face message at the link's rate -- the faces travel on different links, at once (IGX_LINK_GBS, default 60 GB/s per
    // direction).  At 8 ranks of the metric configuration (128^3 per rank) three passes cost 6 ms of a 33 ms assembly and a face
    // is 141 MB = 2.4 ms: one pass; at 2 ranks (256 x 256 x 128) the pass costs 2.3 ms and the face is 552 MB = 9 ms: faces first
    // (scripts/time_rank_box.py, profiles/r04_face_passes.txt).
    long long multi = 0;
    for (int k = 0; k < passes.n; ++k) multi += pencil_box_cost(s, pw, passes.p[k].box, passes.p[k].pp, ncu);
    const long long single = pencil_box_cost(s, pw, P, PencilPass(), ncu);
    const double t_step = (deg == 3 ? 30e-6 : 9e-6) * (pw.geo ? 1.4 : 1.0);      // s per element-step of a launch (256^3: 16 ms / (4 rounds x 131))
    const double cost_s = (double)(multi - single) * t_step;
    // (the communicator's figure: $IGX_LINK_GBS, else what IGXCommInitRCCL measured on this rank's own links, else 60)
    const char *lr = getenv("IGX_LINK_GBS"); const double rate = (lr && atof(lr) > 0 ? atof(lr) : (s.link_gbs > 0 ? s.link_gbs : 60.0)) * 1e9;
    double face = 0; const double rowb = 8.0 * (2 * deg + 1) * (2 * deg + 1) * (2 * deg + 1);
    const double nr[3] = {(double)s.lay[0].nrow, (double)s.lay[1].nrow, (double)s.lay[2].nrow};
    if (can[2]) face = std::max(face, deg * nr[0] * nr[1] * rowb);
    if (can[1]) face = std::max(face, deg * nr[0] * nr[2] * rowb);
    if (can[0]) face = std::max(face, deg * nr[1] * nr[2] * rowb);
    if (!(face / rate > cost_s)) return one;
  }
  return passes;
}

// ------------------------------------------------------------------ reporting
struct WalkInfo {
  enum Kind { PATCH_P2, PATCH_P3, ROWS_P3, STATE_PATCH_P2, ELEMENTS, PENCILS } kind;
  int deg = 3, walk_axis = 0; bool geo = false, fixt = false; const PencilModule *mod = nullptr;
  bool staged = false;      // ROWS_P3: full layers of regular tiles leave through LDS (rows3_stages)
  bool state() const { return mod && mod->state; }
};
static std::string walk_dom_name(const WalkInfo &w) {
  switch (w.kind) {
  case WalkInfo::PATCH_P2: return "gram_patch<p=2>";
  case WalkInfo::PATCH_P3: return "gram_pencil<walk=0,p=3,patch>";
  case WalkInfo::ROWS_P3: return "gram_pencil<walk=0,p=3,rows>";
  case WalkInfo::STATE_PATCH_P2: return "state_patch<p=2>";
  case WalkInfo::ELEMENTS: return "gram_p3_element";
  default: return std::string(w.state() ? "state_pencil<walk=" : w.mod ? "form_pencil<hiprtc,walk=" : "gram_pencil<walk=") + char('0' + w.walk_axis) + ",p=" + char('0' + w.deg) + (w.geo ? ",geometry" : "") + ">";
  }
}
// executed MFMA flops per element: 2*16*16*4 per v_mfma_f64_16x16x4
static double walk_flop_per_element(const Space &s, const WalkInfo &w) {
  switch (w.kind) {
  case WalkInfo::PATCH_P2: return 2048.0 * 21 * 3;
  case WalkInfo::PATCH_P3: return 2.0 * 2 * 4 * 64 * 10;      // (the element phase of the sum-factorised walk: pencil_mfma_sf on 10 tiles)
  // the rows walk: per layer of a tile of nine rows, wavefront dy runs (4 - |dy|) x 4 pencils x 16 (ta, tb) x 2 v_fma_f64 on 64 lanes (16 pencil
  // rows over the seven wavefronts), on the vector pipe; a mesh has one row per element up to its faces
  case WalkInfo::ROWS_P3: return 2.0 * 2 * 16 * 4 * 16 * 64 / Rows3::COLS;
  case WalkInfo::STATE_PATCH_P2: return w.mod->flop_per_element;
  case WalkInfo::ELEMENTS: return 2048.0 * 48 * 16;
  default: break;
  }
  if (w.state()) return w.mod->flop_per_element;
  // the sum-factorised p = 3 Gram walk (pencil_mfma_sf): 2 fp64 FMAs on each of the 4 accumulator doubles of a tile, 64 lanes (its 12
  // MFMAs are once per pencil)
  if (w.deg == 3 && !w.geo && !w.mod && s.env.gram_sumfact != 0) return 2.0 * 2 * 4 * 64 * (w.walk_axis == 0 ? 10 : 16);
  // 48 k-steps, 10 (symmetric, walk 0) or 16 tiles (p = 2: 21 k-steps x 6 layer-pair tiles, or x 3 packed tiles)
  return 2048.0 * (w.deg == 3 ? 48 * (w.walk_axis == 0 ? 10 : 16) : 21 * ((w.walk_axis == 0 && pencil_p2_pack(s, w.deg, w.geo, w.fixt, w.mod != nullptr)) ? 3 : 6));
}
static std::string walk_kname(const Space &s, const WalkInfo &w) {
  switch (w.kind) {
  case WalkInfo::PATCH_P2: return "gram_patch(mfma_f64_16x16x4,p=2,walk=0,packed tiles,4x3 pencils per workgroup,one window)";
  case WalkInfo::PATCH_P3: return "gram_pencil(mfma_f64_16x16x4,p=3,walk=0," + std::to_string(PATCH3_MX) + "x" + std::to_string(PATCH3_MY) + " pencils per workgroup,one window)";
  case WalkInfo::ROWS_P3: return "gram_pencil(fp64 fma,p=3,walk=0,rows gathered by their owner,each entry stored once" + std::string(w.staged ? ",full rows staged in LDS" : "") + ")";
  case WalkInfo::STATE_PATCH_P2: return "state_patch<" + w.mod->name + ">(mfma_f64_16x16x4,p=2,walk=0,packed tiles,4x2 pencils per workgroup,one window)";
  case WalkInfo::ELEMENTS: return "gram_p3_element(mfma_f64_16x16x4)";
  default: break;
  }
  const bool packed = w.deg == 2 && w.walk_axis == 0 && (pencil_p2_pack(s, w.deg, w.geo, w.fixt, w.mod != nullptr) || (w.mod && w.mod->pack));
  return (w.state() ? std::string("state_pencil<") + w.mod->name + ">(mfma_f64_16x16x4,p=" : w.mod ? std::string("form_pencil<") + w.mod->name + ">(hiprtc,mfma_f64_16x16x4,p=" : std::string("gram_pencil(mfma_f64_16x16x4,p=")) +
         char('0' + w.deg) + ",walk=" + char('0' + w.walk_axis) + (w.geo ? ",mapped geometry" : "") + (packed ? ",packed tiles" : "") + (w.walk_axis == 0 ? ")" : ")+gram_p3_element(faces)");
}
static void walk_report(const Space &s, const WalkInfo &w, int launches, long long elements, DomInfo &dom, std::string &kname) {
  dom.name = walk_dom_name(w); dom.launches = launches; dom.elements = elements; dom.flop_per_element = walk_flop_per_element(s, w);
  kname = walk_kname(s, w);
}

// the end of a walk's launches: what a launcher could not do (pencil_launch_error), else what the runtime refused
static int walk_launch_status(const char *launch_failed, std::string &err) {
  if (pencil_launch_error()) { err = pencil_launch_error(); pencil_launch_error() = nullptr; (void)hipGetLastError(); return IGX_ERR_LIB; }
  if (hipGetLastError() != hipSuccess) { err = launch_failed; return IGX_ERR_LIB; }
  return 0;
}
// a patch walk takes the whole assembly: its launches between the events of the roofline line, their status, the report
template <class Launch>
static int run_patch_walk(const Space &s, hipStream_t stream, const WalkInfo &w, const char *launch_failed, Launch launch, std::string &kname, int &launches, std::string &err, bool &done, DomInfo &dom) {
  if (dom.ev0) (void)hipEventRecord(dom.ev0, stream);
  launch();
  if (dom.ev1) (void)hipEventRecord(dom.ev1, stream);
  if (int rc = walk_launch_status(launch_failed, err)) return rc;
  walk_report(s, w, launches, (long long)s.elem_width[0] * s.elem_width[1] * s.elem_width[2], dom, kname);
  done = true;
  return 0;
}

// ------------------------------------------------------------------ dispatch
// zero_matrix: MatZeroEntries of the caller; called before the first launch unless the axis-0 walk stores first touches
// patch3_counters: the engine's ticket counters of the p = 3 patch walk (patch3_counter_bytes of device memory; launch_patches_p3)
// slab_done (may be empty): called between the two passes of an assembly that forms the elements next to the upper face of axis
// 2 first -- the ghost rows of that face are complete then and their exchange can run under the rest of the launches
static int try_gram_mfma(const Space &s, const SpaceDev &S, const OutDev &out, hipStream_t stream, bool forced,
                         std::string &kname, int &launches, std::string &err, bool &done, DomInfo &dom, const std::function<void()> &zero_matrix,
                         const std::function<void()> &slab_done = std::function<void()>(), const PencilModule *mod = nullptr,
                         const std::function<void(int)> &face_done = std::function<void(int)>(), int *patch3_counters = nullptr) {
  done = false;
  auto no = [&](const char *why) { if (forced) { err = std::string("MFMA kernel does not cover this configuration: ") + why; return (int)IGX_ERR_SUP; } return 0; };
  if (!mod && s.form != IGX_FORM_POISSON && s.form != IGX_FORM_POISSON_F) return no("form is not a scalar gradient-Gram form");
  const bool state = mod && mod->state;       // a Tangent (state_pencil): Jacobian / IJacobian drivers, no geometry
  if (state ? (out.op != OP_JACOBIAN && out.op != OP_IJACOBIAN) : (out.op != OP_SYSTEM && out.op != OP_MATRIX)) return no("only System / Matrix drivers (a Tangent: Jacobian / IJacobian)");
  if (s.dim != 3 || s.dof != 1) return no("needs dim=3, dof=1");
  const bool geo = s.nsd != 0;
  if (geo && s.nsd != 3) return no("mapped geometry of another dimension");
  if (state && geo != mod->state_geo) return no("a Tangent on a mapped geometry takes the walk at p = 2 only");
  for (int a = 0; a < 3; ++a) for (int sd = 0; sd < 2; ++sd) if (s.visit[a][sd]) return no("boundary-form passes");
  const int deg = s.axis[0].p;
  if (deg != 2 && deg != 3) return no("needs p=2 or p=3");
  for (int d = 0; d < 3; ++d) {
    if (s.axis[d].p != deg || s.basis[d].nqp != deg + 1) return no("needs the same degree p and p+1 Gauss points on every axis");
    for (int sd = 0; sd < 2; ++sd) if (s.load[d][sd].count && out.op == OP_SYSTEM && !boundary_loads_supported(s)) return no("boundary loads next to an axis wrapped inside the rank");
  }
  GramArgs ga; ga.forcing = (s.form == IGX_FORM_POISSON) ? 1.0 : -6.0; ga.nwaves = 0;
  launches = 0;
  const bool sys = out.op == OP_SYSTEM;
  // walk axis: the slowest-varying mesh axis that qualifies keeps axis 0 (contiguous CSR columns) on the lanes
  int walk_axis = -1;
  { const int pref[3] = {s.env.walk_axis, 2, 1};
    for (int k = 0; k < 3 && walk_axis < 0; ++k) if (pref[k] >= 0 && pref[k] < 3 && axis_walkable(s, pref[k], pref[k] == 0)) walk_axis = pref[k]; }
  const bool walk = walk_axis >= 0;
  if (deg == 2 && walk_axis != 0) return no("p=2 needs a walkable axis 0");
  if ((geo || mod) && walk_axis != 0) return no("a mapped geometry / a run-time form needs a walkable axis 0");
  const bool fixt = S.fixtable != nullptr && sys;       // IGASetFixTable: Dirichlet values per node (the Matrix driver applies none)
  if (fixt && walk_axis != 0) return no("fix table without a walkable axis 0");
  if (fixt && mod) return no("fix table with a run-time form");
  Box all; for (int d = 0; d < 3; ++d) { all.lo[d] = 0; all.hi[d] = s.elem_width[d]; }
  if (!walk && deg != 3) return no("p=2 needs a walkable axis 0");
  const bool first_touch = walk_axis == 0 && !s.env.no_first_touch && out.val && axis_first_touch_ok(s, 1) && axis_first_touch_ok(s, 2);
  // (round 13: IGX_ROWS3) p = 3 where the patch walk applies, one new node per element on axis 0 too: the rows walk (gram_rows3.hpp) stores
  // every entry once and reads none -- no MatZeroEntries, no first touch, one launch.  Chosen under IGX_PATCH3=1 only.
  const bool patch_ok = walk_axis == 0 && !geo && !mod && !fixt && (out.op == OP_MATRIX || out.op == OP_SYSTEM) && patch_walk_covers(s);
  const bool rows3 = deg == 3 && s.env.gram_sumfact != 0 && patch_ok && out.val && s.env.patch3 == 1 && rows3_covers(s) &&
                     (s.env.rows3 == 2 || (s.env.rows3 == 1 && rows3_pays(s)));
  if (rows3) { /* nothing to zero */ }
  else if (!first_touch) zero_matrix();
  else if (s.proc_sizes[0] * s.proc_sizes[1] * s.proc_sizes[2] > 1) zero_neighbour_rows(s, out, stream);   // the only entries no local element reaches
  // boundary loads first: F is zeroed and only added to, so the order is free -- and the ghost rows of the upper face of axis 2
  // must be complete when the first pass of a multi-rank assembly ends (slab_done below)
  if (sys) { if (int rc = launch_boundary_loads(s, S, out, stream, err)) return rc; }
  WalkInfo info; info.deg = deg; info.walk_axis = walk_axis; info.geo = geo; info.fixt = fixt; info.mod = mod;
  auto gram_patch_ok = [&] { return patch_ok; };
  if (rows3) {
    info.kind = WalkInfo::ROWS_P3; info.staged = rows3_stages(s);
    return run_patch_walk(s, stream, info, "gram_pencil_rows3 kernel launch failed", [&] { launch_rows3(s, S, out, stream, launches, ga.forcing, patch3_counters); }, kname, launches, err, done, dom);
  }
  // (round 6: IGX_PATCH=1) p = 2 on the identity geometry, one rank: the walk of 4 x 3 patches of pencils whose band rows leave through the whole
  // workgroup (gram_patch.hpp): 4 colours, 190 instead of 405 entries per element read-add-written
  if (deg == 2 && s.env.patch && gram_patch_ok()) {
    info.kind = WalkInfo::PATCH_P2;
    return run_patch_walk(s, stream, info, "gram_patch kernel launch failed", [&] { launch_patches_p2(s, S, out, stream, launches, ga.forcing, first_touch); }, kname, launches, err, done, dom);
  }
  // (round 8: IGX_PATCH3) p = 3 on the identity geometry, one rank, the sum-factorised Gram phase: the walk of 4 x 2 patches of pencils whose
  // band rows leave through the whole workgroup (gram_patch3.hpp): 6 colours, 745 instead of 1792 entries per element read-add-written.
  // It reports itself as a Gram pencil walk: the same element phase, bit-repeatable like it.
  if (deg == 3 && s.env.gram_sumfact != 0 && gram_patch_ok() && (s.env.patch3 == 2 || (s.env.patch3 == 1 && patch3_pays(s)))) {
    info.kind = WalkInfo::PATCH_P3;
    return run_patch_walk(s, stream, info, "gram_pencil_patch3 kernel launch failed", [&] { launch_patches_p3<PATCH3_MX, PATCH3_MY>(s, S, out, stream, launches, ga.forcing, first_touch, patch3_counters); }, kname, launches, err, done, dom);
  }
  // p = 2, a Tangent (IGX_PATCH_STATE=1): 4 x 2 pencils per workgroup, state_patch_p2
  if (deg == 2 && walk_axis == 0 && s.env.patch_state && state && !geo && mod->patch_kfn && patch_walk_covers(s)) {
    info.kind = WalkInfo::STATE_PATCH_P2;
    return run_patch_walk(s, stream, info, "state_patch kernel launch failed", [&] { launch_state_patches_p2(s, S, out, stream, launches, first_touch, mod->patch_kfn, mod->prm); }, kname, launches, err, done, dom);
  }
  auto elements = [&](const Box &b) { if (sys) launch_elements<true>(s, S, out, stream, b, ga, launches); else launch_elements<false>(s, S, out, stream, b, ga, launches); };
  if (!walk) {
    if (dom.ev0) (void)hipEventRecord(dom.ev0, stream);
    elements(all);
    if (dom.ev1) (void)hipEventRecord(dom.ev1, stream);
    info.kind = WalkInfo::ELEMENTS;
    walk_report(s, info, launches, (long long)s.elem_width[0] * s.elem_width[1] * s.elem_width[2], dom, kname);
  } else {
    // P = elements without a Dirichlet face (pencil kernel), E = the rest (element kernel, which owns the BC logic)
    Box P = all;
    // (the axis-0 walk applies the Dirichlet fix-up itself; the other walks leave face elements to gram_p3_element)
    if (sys && walk_axis != 0) for (int d = 0; d < 3; ++d) {
      if (s.axis[d].periodic) continue;
      if (s.value[d][0].count && s.elem_start[d] == 0) P.lo[d] = 1;
      if (s.value[d][1].count && s.elem_start[d] + s.elem_width[d] == s.elem_sizes[d]) P.hi[d] = s.elem_width[d] - 1;
    }
    const int l0 = launches;
    if (dom.ev0) (void)hipEventRecord(dom.ev0, stream);
    // (geo of the walk: the metric tensor per Gauss point from the wavefront's own geometry evaluation; a run-time form: its own coefficients)
    PencilWalk pw; pw.W = walk_axis; pw.P = deg; pw.geo = geo || mod; pw.fixt = fixt; pw.mod = mod; pw.forcing = ga.forcing; pw.first_touch = first_touch;
    pw.pick = gram_pencil_switchboard(sys, walk_axis, deg, pw.geo, pw.geo && s.rational, fixt);
    if (!pw.pick) { err = "the library holds no instantiation of the pencil walk for this configuration"; return IGX_ERR_LIB; }
    const WalkPasses passes = assembly_passes(s, pw, P, (bool)slab_done, (bool)face_done, pencil_cus());
    dom.passes = passes.n;
    for (int k = 0; k < passes.n; ++k) {
      const WalkPass &wp = passes.p[k];
      launch_pencils(s, S, out, stream, pw, wp.box, wp.pp, launches);
      if (wp.mark == 2) slab_done(); else if (wp.mark >= 0) face_done(wp.mark);
    }
    if (dom.ev1) (void)hipEventRecord(dom.ev1, stream);
    info.kind = WalkInfo::PENCILS;
    walk_report(s, info, launches - l0, (long long)std::max(0, P.hi[0] - P.lo[0]) * std::max(0, P.hi[1] - P.lo[1]) * std::max(0, P.hi[2] - P.lo[2]), dom, kname);
    // E as disjoint slabs: axis 0 faces (full), axis 1 faces (inside P along 0), axis 2 faces (inside P along 0,1)
    for (int d = 0; d < 3; ++d) for (int side = 0; side < 2; ++side) {
      Box b = all;
      for (int k = 0; k < d; ++k) { b.lo[k] = P.lo[k]; b.hi[k] = P.hi[k]; }
      if (side == 0) { b.lo[d] = all.lo[d]; b.hi[d] = std::min(P.lo[d], P.hi[d]); }
      else { b.lo[d] = std::max(P.hi[d], P.lo[d]); b.hi[d] = all.hi[d]; }
      elements(b);
    }
  }
  if (int rc = walk_launch_status("gram MFMA kernel launch failed", err)) return rc;
  done = true;
  return 0;
}

}  // namespace igx
