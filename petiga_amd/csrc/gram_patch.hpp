// gram_patch.hpp -- the p = 2 Gram walk with the band rows combined across ALL THREE axes before they reach memory (round 6).
//
// gram_pencil_w6 (gram_mfma.hpp) gives each of a workgroup's twelve wavefronts a pencil of its own and a window of its own: a band
// row is combined along the walk and then read-add-written once per pencil -- 405 entries per element, nine colours of pencils.
// Here the twelve wavefronts walk a PATCH of 4 x 3 adjacent pencils in step and add into ONE window in LDS,
//   win[4 node layers (ring)][y pair][x pair][5 walk-axis offsets],
// a "pair" being two nodes of the patch on an axis that share one of its elements (24 on axis 1, 19 on axis 2).  A layer of the
// patch is complete when every wavefront has added its element: 2280 entries for 12 elements -- 190 per element instead of 405 --
// in runs that lie 25 to a 200-byte stretch of a CSR row, and patches conflict only with their neighbours: 4 colours instead of 9.
// Every thread of the workgroup owns ONE run (y pair, x pair) for the whole walk: its matrix address is a per-thread constant plus
// the layer's part, its old values are requested a step ahead -- before the element's MFMAs -- and consumed behind them.  One barrier
// per element.
//
// The price: up to nine wavefronts add to one window entry with ds_add_f64 and the ORDER of those adds is not fixed -- the assembly is
// correct to rounding (1e-12 against the oracle like every other path) but not bit-repeatable, which every other kernel of this library
// is.  A deterministic variant (each wavefront its own window, the runs gathered from the windows in a fixed order) was built, passed
// the bit-repeat tests and was slower than the pencil walk (profiles/r06_patch_walk.txt).  The shared window is + 23 % on config 2 (System
// driver, 128^3: 326 against 265 M el/s; Matrix driver 383 against 324) and the default where it applies; IGX_PATCH=0 keeps the
// bit-repeatable pencil walk.
//
// Degree 2, identity geometry, one rank, axis-0 walk; System and Matrix drivers, Dirichlet values on any face, first touch.
#pragma once
#include "gram_mfma.hpp"
#include "patch_walk.hpp"

namespace igx {

using PatchP2 = PatchShape<2, 4, 3>;                                            // gram_patch_p2: 4 x 3 pencils
static_assert(PatchP2::W == 12 && PatchP2::NX == 6 && PatchP2::NY == 5 && PatchP2::NXP == 24 && PatchP2::NYP == 19 && PatchP2::SX == 2 && PatchP2::SY == 2, "the 4 x 3 patch at p = 2");
constexpr int PATCH_SLOTS = 4;                                                  // ring: three layers being added to, one leaving
template <class G> constexpr int PATCH_LAYER = G::NYP * G::NXP * G::BW;         // doubles per node layer of the window (p = 2 walks)

// LDS behind the walk's tables: the window, the pair tables (ints), the System driver's F and lifting stages (three deep: a layer's F leaves a
// step behind its band rows)
__host__ __device__ static inline size_t patch_lds_bytes(int ne_max) {
  using G = PatchP2;
  return pencil_lds_bytes(ne_max, false, G::W) + (size_t)PATCH_SLOTS * PATCH_LAYER<G> * 8 + (size_t)G::PAIR_INTS * 4 + (size_t)3 * (G::W * 9 + G::NODES) * 8 + 64;
}

template <bool SYSTEM>
__global__ void __launch_bounds__(768, 3)
gram_patch_p2(SpaceDev S, OutDev out, PatchArgs A) {
  using G = PatchP2;
  constexpr int P = G::P, NB = 3, BW = G::BW, LAYER = PATCH_LAYER<G>;
  extern __shared__ __attribute__((aligned(16))) double pencil_sm[];
  const PencilArgs &pa = A.pa;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const PatchWalk D = patch_decode<G>(S, A, wave, (int)blockIdx.x);
  const int seg = D.seg, ex0 = D.ex0, ey0 = D.ey0, mxv = D.mxv, myv = D.myv, wi = D.wi, wj = D.wj, elx = D.elx, ely = D.ely, wh = D.wh, ne = D.ne, nl = D.nl;
  const bool valid = D.valid;
  const AxisDev &AW = S.ax[0], &AX = S.ax[1], &AY = S.ax[2];

  PencilLds T = pencil_lds_carve(pencil_sm, pa.ne_max, false);
  T.lay0 = AW.off[wh];
  double *win = reinterpret_cast<double *>(reinterpret_cast<char *>(pencil_sm) + pencil_lds_bytes(pa.ne_max, false, G::W));
  int *XP = reinterpret_cast<int *>(win + PATCH_SLOTS * LAYER), *YP = XP + G::NX * BW, *XI = YP + G::NY * BW, *YI = XI + G::NXP, *cntp = YI + G::NYP;
  double *Fp = reinterpret_cast<double *>(cntp + 8);            // [layer % 3][wave][9]: the leaving layer's F sums of each pencil
  double *corrp = Fp + 3 * G::W * 9;                         // [layer % 3][node]: the lifting sum_k K_ik v_k of the row, summed over its runs
  {   // the walk-axis tables of the segment (as gram_pencil_body stages them), the windows, the pair tables
    const int nthr = G::W * 64;
    for (int i = tid; i < ne * 32; i += nthr) {
      const int e = i >> 5, j = i & 31, q = j >> 3, aa = (j >> 1) & 3, k = j & 1, eg = wh + e;
      T.zt[i] = (q < NB && aa < NB) ? AW.tab[((size_t)eg * NB * NB + q * NB + aa) * NDER + k] * sqrt(AW.w[eg * NB + q] * AW.J[eg]) : 0.0;
    }
    for (int i = tid; i < ne * 4; i += nthr) { const int e = i >> 2, q = i & 3, eg = wh + e; T.wq[i] = (q < NB) ? sqrt(AW.w[eg * NB + q] * AW.J[eg]) : 0.0; }
    for (int i = tid; i < ne; i += nthr) T.Jz[i] = AW.J[wh + i];
    patch_stage_layers<BW>(T, AW, nl, tid, nthr);
    for (int i = tid; i < PATCH_SLOTS * LAYER; i += nthr) win[i] = 0.0;
    for (int i = tid; i < 3 * G::NODES; i += nthr) corrp[i] = 0.0;
    patch_pair_tables<G>(XP, YP, XI, YI, cntp, mxv, myv, tid);
  }
  __syncthreads();
  const int nxp = cntp[0], nyp = cntp[1];

  // ---- this wavefront's pencil: the 1-D rows of axes 1, 2 in LDS (scaled by sqrt(w J)), its window, the F factor of its F lanes
  double *rows = reinterpret_cast<double *>(reinterpret_cast<char *>(pencil_sm) + (pencil_lds_bytes(pa.ne_max, false, G::W) - (size_t)2 * G::W * 32 * 8));
  double *vys = rows + wave * 32, *uxs = rows + G::W * 32 + wave * 32;
  double sxy = 0;
  {
    const double *__restrict__ TX = AX.tab + (size_t)elx * (NB * NB * NDER);
    const double *__restrict__ TY = AY.tab + (size_t)ely * (NB * NB * NDER);
    const double *__restrict__ WX = AX.w + elx * NB, *__restrict__ WYq = AY.w + ely * NB;
    if (lane < 32) { const int aa = lane >> 3, qq = (lane >> 1) & 3, kk = lane & 1; vys[lane] = (aa < NB && qq < NB) ? TY[(qq * NB + aa) * NDER + kk] * sqrt(WYq[qq] * AY.J[ely]) : 0.0; }
    else { const int l2 = lane - 32, qq = l2 >> 3, aa = (l2 >> 1) & 3, kk = l2 & 1; uxs[l2] = (aa < NB && qq < NB) ? TX[(qq * NB + aa) * NDER + kk] * sqrt(WX[qq] * AX.J[elx]) : 0.0; }
    if constexpr (SYSTEM) {      // F lane (fx = lane & 3, fy = (lane >> 2) & 3, slot = lane >> 4): forcing * sum_q w N on axes 1, 2 (as PencilLane::sxy)
      const int fx = lane & 3, fy = (lane >> 2) & 3;
      double sx = 0, sy = 0;
      if (fx < NB && fy < NB) {
#pragma unroll
        for (int q = 0; q < NB; ++q) { sx += WX[q] * TX[(q * NB + fx) * NDER]; sy += WYq[q] * TY[(q * NB + fy) * NDER]; }
      }
      sxy = valid ? pa.forcing * (sx * sy) * (AX.J[elx] * AY.J[ely]) : 0.0;
    }
  }
  const P2kLaneT<false> K = pencil_p2k_lane<false>(lane);      // (its operand offsets; the window offsets below replace the rest)
  // where the lane's results go in the window: (y pair, x pair, walk offset) of (row a, column b); code = offset * 4 + the row's a_w (the
  // ring slot's layer part), -1 for the padding.  Tiles (0,0), (0,1), (1,1) and the mirror entries of (0,1).
  int code[3][4], codem[4];
  {
    auto split = [](int f, int &aw, int &ay, int &ax) { aw = f / 9; const int r = f - 9 * aw; ay = r / 3; ax = r - 3 * ay; };
    auto entry = [&](int a, int b) -> int {
      if (a >= 27 || b >= 27 || !valid) return -1;
      int aw, ay, ax, bw, by, bx; split(a, aw, ay, ax); split(b, bw, by, bx);
      const int yp = YP[(wj + ay) * 5 + (by - ay + 2)], xp = XP[(wi + ax) * 5 + (bx - ax + 2)];
      return (((yp * nxp + xp) * 5 + (bw - aw + 2)) << 2) | aw;
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a0 = 4 * i + (lane >> 4), a1 = 16 + a0, b0 = lane & 15, b1 = 16 + b0;
      code[0][i] = entry(a0, b0); code[1][i] = entry(a0, b1); code[2][i] = entry(a1, b1);
      codem[i] = entry(b1, a0);
    }
  }
  const int fslot = lane >> 4;
  double Facc = 0;

  PatchFix<P> fx;      // the Dirichlet data of the patch
  if constexpr (SYSTEM) fx.fill(S, D);

  // ---- this thread's run of the band rows: (y pair, x pair) for the whole walk; pos = RA + RB prefix0(layer) + RC count0(layer) + P0(layer, d)
  const bool unit = tid < nxp * nyp;
  long long RA = 0; int RB = 0, RC = 0;
  int uyr = 0, udy = 0, uxr = 0, udx = 0;
  bool ufirst = false;
  if (unit) {
    const int yp = tid / nxp, xp = tid - yp * nxp;
    patch_pair<P>(YI[yp], uyr, udy); patch_pair<P>(XI[xp], uxr, udx);
    patch_run_address<P>(S, ex0, ey0, uxr, udx, uyr, udy, RA, RB, RC);
    if (pa.first_touch) ufirst = patch_first_touch<G>(A, D, uxr, udx, uyr, udy);
  }
  int own_lo, own_hi;
  patch_owned_layers(S, A, D, own_lo, own_hi);
  // rows of the F stage: thread t < 30 is patch node (yr, xr) = (t / 6, t % 6); its F row without the walk-axis part (read ONCE: two dependent
  // global loads per element in the F leave made wavefront 0 late at every barrier -- 1.2 of 7.9 ms at 128^3)
  long long frowxy = 0;
  constexpr int FT0 = (G::W - 1) * 64;
  static_assert(G::NYP * G::NXP <= FT0 && G::NODES <= 64, "the runs leave the last wavefront free for the F rows");
  if (SYSTEM && tid >= FT0 && tid < FT0 + G::NODES) {
    const int yr = (tid - FT0) / G::NX, xr = (tid - FT0) - yr * G::NX;
    if (xr <= mxv + 1 && yr <= myv + 1) frowxy = (long long)S.ax[0].nrow * AX.rowmap[AX.off[ex0] + xr] + (long long)S.ax[0].nrow * S.ax[1].nrow * AY.rowmap[AY.off[ey0] + yr];
  }

  // the run of layer li: its five old values are requested a step ahead (fetch) and consumed when the layer is complete (leave)
  struct Run { long long base; double o[5]; int p0[5]; bool on, full; };
  auto fetch = [&](int li, Run &r) {
    const int lay = T.lay0 + li;
    r.on = unit && li >= 0 && li < nl && T.cnt[li] > 0 && lay >= own_lo && lay < own_hi;
    if (!r.on) return;
    r.base = RA + (long long)RB * T.pre[li] + (long long)RC * T.cnt[li];
#pragma unroll
    for (int d = 0; d < 5; ++d) r.p0[d] = T.P[li * 8 + d];
    r.full = patch_layer_full<BW>(r.p0);      // (an interior layer: the run is 40 contiguous bytes)
    patch_run_load<BW>(out.val, r.base, r.p0, r.full, ufirst, r.o);
  };
  auto leave = [&](int li, const Run &r) {
    if (!unit) return;
    double *w = win + (li & (PATCH_SLOTS - 1)) * LAYER + tid * 5;
    double v[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) { v[d] = w[d]; w[d] = 0.0; }
    if (!r.on) return;
    const int lay = T.lay0 + li;
    if constexpr (SYSTEM) {      // IGAElementFixSystem (src/petigaelem.c:1377-1387) on the combined run; the lifting of its row goes to the F stage
      double corr = 0;
      if (fx.reaches(lay)) {
        double rv = 0; const bool rf = fx.fixed(uxr, uyr, lay, rv);
#pragma unroll
        for (int d = 0; d < 5; ++d) {
          double cv = 0; const bool cf = fx.fixed(uxr + udx, uyr + udy, lay + d - P, cv);
          if (cf) corr += v[d] * cv;
          if (rf || cf) v[d] = (d == P && udx == 0 && udy == 0 && rf) ? (double)fx.held(li, uxr, uyr, ne) : 0.0;
        }
      }
      // (this path is the one that is not bit-repeatable anyway: the row's lifting is summed with LDS atomics too, by the runs that have any)
      if (corr != 0.0) (void)__hip_atomic_fetch_add(corrp + (li % 3) * G::NODES + uyr * G::NX + uxr, corr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    patch_run_add_store<BW>(out.val, r.base, r.p0, r.full, r.o, v);
  };
  // F of layer li: thread t < 30 = patch node (yr, xr): the pencils' sums (Fp) and its runs' liftings (corrp), each in a fixed order
  auto leave_f = [&](int li) {
    if constexpr (SYSTEM) {
      const int lay = T.lay0 + li;
      const bool on = li >= 0 && li < nl && T.cnt[li] > 0 && lay >= own_lo && lay < own_hi;
      const int ft = tid - FT0;      // (the F rows belong to threads of the last wavefront, which own no run)
      if (!on || ft < 0 || ft >= G::NODES) return;
      const int yr = ft / G::NX, xr = ft - yr * G::NX;
      if (xr > mxv + 1 || yr > myv + 1) return;
      double f = 0;
      const double *Fl = Fp + (li % 3) * (G::W * 9); double *cl = corrp + (li % 3) * G::NODES;
      for (int j = max(0, yr - 2); j <= min(yr, myv - 1); ++j)
        for (int i = max(0, xr - 2); i <= min(xr, mxv - 1); ++i) f += Fl[(j * G::MX + i) * 9 + 3 * (yr - j) + (xr - i)];
      double fv = 0;
      if (fx.reaches(lay)) {
        if (fx.fixed(xr, yr, lay, fv)) f = fv * (double)fx.held(li, xr, yr, ne);
        else f -= cl[ft];
      }
      cl[ft] = 0.0;
      const long long row = (long long)T.rho[li] + frowxy;
      // one memory-side add per row and launch (patches of a colour share no node): order-free, and nothing waits for it -- a load / add /
      // store chain here makes its wavefront late at every barrier
      (void)__hip_atomic_fetch_add(out.vec + row, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };

  auto f_stage = [&](int li) {      // the leaving layer's F sums of this pencil (slot 0 of the F lanes), then the slots slide
    if constexpr (SYSTEM) {
      if (fslot == 0 && (lane & 3) < NB && ((lane >> 2) & 3) < NB) Fp[(li % 3) * (G::W * 9) + wave * 9 + 3 * ((lane >> 2) & 3) + (lane & 3)] = Facc;
      const double up = __shfl_down(Facc, 16);
      Facc = (fslot >= NB - 1) ? 0.0 : up;
    }
  };
  Run run; run.on = false;
  fetch(0, run);
  long long st_mfma = 0, st_wait = 0, st_leave = 0, st_t0 = 0; const long long st_wall0 = (kDebug && pa.debug_buf) ? wall_clock64() : 0;
  for (int ei = 0; ei < ne; ++ei) {
    if (kDebug && pa.debug_buf) st_t0 = __builtin_readcyclecounter();
    if (valid) {
      d4_t pk[3];
      pencil_mfma_p2k(pk, uxs, vys, T.zt + ei * 32, K, lane);
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = code[t][i];
          if (c >= 0) (void)__hip_atomic_fetch_add(win + ((ei + (c & 3)) & (PATCH_SLOTS - 1)) * LAYER + (c >> 2), pk[t][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (t == 1) { const int m = codem[i]; if (m >= 0) (void)__hip_atomic_fetch_add(win + ((ei + (m & 3)) & (PATCH_SLOTS - 1)) * LAYER + (m >> 2), pk[t][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
        }
    }
    if constexpr (SYSTEM) {      // F_a += f J prod_d sum_q w N: the walk-axis factor is sum_q sqrt(wJ) (sqrt(wJ) N)
      double sw = 0;
      const int fs = fslot < NB ? fslot : 0;
#pragma unroll
      for (int q = 0; q < NB; ++q) sw += T.wq[ei * 4 + q] * T.zt[ei * 32 + (q * 4 + fs) * 2];
      if (fslot < NB) Facc += sxy * sw;
      f_stage(ei);
    }
    long long st_t1 = 0, st_t2 = 0;
    if (kDebug && pa.debug_buf) st_t1 = __builtin_readcyclecounter();
    __syncthreads();      // every wavefront's element ei is in the window: layer ei is complete (and its F sums are staged)
    if (kDebug && pa.debug_buf) st_t2 = __builtin_readcyclecounter();
    leave(ei, run);
    if (ei >= 1) leave_f(ei - 1);      // (a step behind: the liftings of its runs were staged before this barrier)
    fetch(ei + 1, run);
    if (kDebug && pa.debug_buf) { const long long t3 = __builtin_readcyclecounter(); st_mfma += st_t1 - st_t0; st_wait += st_t2 - st_t1; st_leave += t3 - st_t2; }
  }
  if (kDebug && pa.debug_buf && lane == 0) {      // -DIGX_DEBUG: per wavefront [MFMAs + window adds | wait at the barrier | leave + next fetch] summed over the walk, elements; workgroup record
    long long *d = pa.debug_buf + ((size_t)blockIdx.x * G::W + wave) * 4;
    d[0] = st_mfma; d[1] = st_wait; d[2] = st_leave; d[3] = ne;
    if (wave == 0) { long long *w = pa.debug_buf + (size_t)gridDim.x * G::W * 4 + (size_t)blockIdx.x * 4; w[0] = st_wall0; w[1] = wall_clock64(); w[2] = __builtin_amdgcn_s_getreg((16 - 1) << 11 | 4); w[3] = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 20); }
  }
  if constexpr (SYSTEM) { __syncthreads(); leave_f(ne - 1); }
  if (seg == pa.nseg - 1 && !pa.open_hi)
    for (int k = 0; k < P; ++k) {
      f_stage(ne + k);
      leave(ne + k, run);
      if constexpr (SYSTEM) { __syncthreads(); leave_f(ne + k); }
      fetch(ne + k + 1, run);
    }
}

// ---- the same walk for the Tangent of a nonlinear scalar form on the identity geometry (config 4: demo/CahnHilliard3D.c:111-179 through
// IGAComputeIJacobian).  state_pencil_k (gram_mfma.hpp) gives each of eight wavefronts a pencil, a window and a flush of its own; here the
// eight walk a patch of 4 x 2 pencils in step: the state's point values and the 140 MFMAs of an element are the pencil walk's
// (pencil_state_eval, pencil_mfma_state_p2k), the four tiles -- a Tangent is not symmetric -- go to ONE window, and every thread owns
// one run of the patch's band rows (14 x 24 pairs of nodes: 210 entries per element instead of 405, 4 colours instead of 9).
// IGAElementFixJacobian on the combined run (src/petigaelem.c:1483-1500).  Not bit-repeatable, like gram_patch_p2.
using StatePatchP2 = PatchShape<2, 4, 2>;
static_assert(StatePatchP2::W == 8 && StatePatchP2::NX == 6 && StatePatchP2::NY == 4 && StatePatchP2::NXP == 24 && StatePatchP2::NYP == 14 && StatePatchP2::SX == 2 && StatePatchP2::SY == 2, "the 4 x 2 patch at p = 2");
__host__ __device__ static inline size_t spatch_lds_bytes(int ne_max) {
  using G = StatePatchP2;
  return pencil_lds_bytes(ne_max, true, G::W) + (size_t)PATCH_SLOTS * PATCH_LAYER<G> * 8 + (size_t)G::W * GEO_DOUBLES * 8 + (size_t)G::W * STATE_D2 * 8 + (size_t)G::PAIR_INTS * 4 + 64;
}

template <class Form>
__global__ void __launch_bounds__(512, 2)
state_patch_p2(SpaceDev S, OutDev out, PatchArgs A, ParamsDev prm) {
  static_assert(pencil_state_of<Form>::v, "state_patch_p2: the form declares PENCIL_NFEAT, PENCIL_NC, pencil_coef and pencil_trial");
  using G = StatePatchP2;
  constexpr int P = G::P, NB = 3, BW = G::BW, LAYER = PATCH_LAYER<G>, GZ = GEO_Z, GD = GEO_DOUBLES;
  extern __shared__ __attribute__((aligned(16))) double pencil_sm[];
  const PencilArgs &pa = A.pa;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const PatchWalk D = patch_decode<G>(S, A, wave, (int)blockIdx.x);
  const int seg = D.seg, ex0 = D.ex0, ey0 = D.ey0, mxv = D.mxv, myv = D.myv, wi = D.wi, wj = D.wj, elx = D.elx, ely = D.ely, wh = D.wh, ne = D.ne, nl = D.nl;
  const bool valid = D.valid;
  const AxisDev &AW = S.ax[0], &AX = S.ax[1], &AY = S.ax[2];

  PencilLds T = pencil_lds_carve(pencil_sm, pa.ne_max, true);      // (no scaled walk-axis rows: an element's raw rows travel with its point numbers)
  T.lay0 = AW.off[wh];
  char *base = reinterpret_cast<char *>(pencil_sm) + pencil_lds_bytes(pa.ne_max, true, G::W);
  double *win = reinterpret_cast<double *>(base);
  double *geo = win + PATCH_SLOTS * LAYER + wave * GD;
  double *d2w = win + PATCH_SLOTS * LAYER + G::W * GD + wave * STATE_D2;
  int *XP = reinterpret_cast<int *>(win + PATCH_SLOTS * LAYER + G::W * GD + G::W * STATE_D2), *YP = XP + G::NX * BW, *XI = YP + G::NY * BW, *YI = XI + G::NXP, *cntp = YI + G::NYP;
  {
    const int nthr = G::W * 64;
    for (int i = tid; i < ne * 4; i += nthr) { const int e = i >> 2, q = i & 3, eg = wh + e; T.wq[i] = (q < NB) ? AW.w[eg * NB + q] * AW.J[eg] : 0.0; }      // (the weight itself: pencil_coef takes the whole JW)
    for (int i = tid; i < ne; i += nthr) T.Jz[i] = AW.J[wh + i];
    patch_stage_layers<BW>(T, AW, nl, tid, nthr);
    for (int i = tid; i < PATCH_SLOTS * LAYER; i += nthr) win[i] = 0.0;
    patch_pair_tables<G>(XP, YP, XI, YI, cntp, mxv, myv, tid);
  }
  __syncthreads();
  const int nxp = cntp[0], nyp = cntp[1];

  // ---- this wavefront's pencil: raw 1-D rows of axes 1, 2 and their second derivatives (LDS), the Gauss weights of the lane's point
  double *rows = reinterpret_cast<double *>(reinterpret_cast<char *>(pencil_sm) + (pencil_lds_bytes(pa.ne_max, true, G::W) - (size_t)2 * G::W * 32 * 8));
  double *vyr = rows + wave * 32, *uxr = rows + G::W * 32 + wave * 32;
  double wjxy = 0;
  {
    const double *__restrict__ TX = AX.tab + (size_t)elx * (NB * NB * NDER);
    const double *__restrict__ TY = AY.tab + (size_t)ely * (NB * NB * NDER);
    if (lane < 32) { const int aa = lane >> 3, qq = (lane >> 1) & 3, kk = lane & 1; vyr[lane] = (aa < NB && qq < NB) ? TY[(qq * NB + aa) * NDER + kk] : 0.0; }
    else { const int l2 = lane - 32, qq = l2 >> 3, aa = (l2 >> 1) & 3, kk = l2 & 1; uxr[l2] = (aa < NB && qq < NB) ? TX[(qq * NB + aa) * NDER + kk] : 0.0; }
    if (lane < 16) { const int qq = lane >> 2, aa = lane & 3; d2w[lane] = (qq < NB && aa < NB) ? TX[(qq * NB + aa) * NDER + 2] : 0.0; }
    else if (lane < 32) { const int aa = (lane - 16) >> 2, qq = lane & 3; d2w[lane] = (qq < NB && aa < NB) ? TY[(qq * NB + aa) * NDER + 2] : 0.0; }
    const int gqx = lane & 3, gqy = (lane >> 2) & 3;
    if (gqx < NB && gqy < NB) wjxy = (AX.w[elx * NB + gqx] * AX.J[elx]) * (AY.w[ely * NB + gqy] * AY.J[ely]);
  }
  const P2kLaneT<false> K = pencil_p2k_lane<false>(lane);      // (its operand offsets)
  int code[4][2];      // tile (Ta, Tb) = code[2 Ta + Tb], rows i = 0..3 in 16-bit halves: offset * 4 + the row's a_w, 0xffff for the padding
  {
    auto split = [](int f, int &aw, int &ay, int &ax) { aw = f / 9; const int r = f - 9 * aw; ay = r / 3; ax = r - 3 * ay; };
    auto entry = [&](int a, int b) -> int {
      if (a >= 27 || b >= 27 || !valid) return 0xffff;
      int aw, ay, ax, bw, by, bx; split(a, aw, ay, ax); split(b, bw, by, bx);
      const int yp = YP[(wj + ay) * 5 + (by - ay + 2)], xp = XP[(wi + ax) * 5 + (bx - ax + 2)];
      return (((yp * nxp + xp) * 5 + (bw - aw + 2)) << 2) | aw;
    };
    static_assert(LAYER * 4 < 0xffff, "a window offset and its slot fit 16 bits");
#pragma unroll
    for (int Ta = 0; Ta < 2; ++Ta)
#pragma unroll
      for (int Tb = 0; Tb < 2; ++Tb)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          code[Ta * 2 + Tb][h] = entry(16 * Ta + 4 * (2 * h) + (lane >> 4), 16 * Tb + (lane & 15)) | (entry(16 * Ta + 4 * (2 * h + 1) + (lane >> 4), 16 * Tb + (lane & 15)) << 16);
  }
  PatchFix<P> fx;      // the Dirichlet data of the patch (a Tangent's rows and the state's fixed values: every driver)
  fx.fill(S, D);
  // ---- this thread's run
  // Wavefronts w and w + 4 share a SIMD; group 0 (wavefronts 0-3) and group 1 (4-7) run half a period apart as in the pencil walk -- one
  // issues its MFMAs while the other leaves its runs and evaluates its next state -- and each group owns half of the patch's runs.
  const int grp = wave >> 2;
  const int nruns = nxp * nyp, half = (nruns + 1) >> 1;
  const int rid = (tid & 255) + grp * half;
  const bool unit = (tid & 255) < half && rid < nruns;
  long long RA = 0; int RB = 0, RC = 0, uyr = 0, udy = 0, uxr_ = 0, udx = 0;
  bool ufirst = false;
  if (unit) {
    const int yp = rid / nxp, xp = rid - yp * nxp;
    patch_pair<P>(YI[yp], uyr, udy); patch_pair<P>(XI[xp], uxr_, udx);
    patch_run_address<P>(S, ex0, ey0, uxr_, udx, uyr, udy, RA, RB, RC);
    if (pa.first_touch) ufirst = patch_first_touch<G>(A, D, uxr_, udx, uyr, udy);
  }
  int own_lo, own_hi;
  patch_owned_layers(S, A, D, own_lo, own_hi);
  const long long rsx = S.ax[0].nrow, rsy = (long long)S.ax[0].nrow * S.ax[1].nrow;
  // U rows of this lane's node (aw, ay, ax) without the walk-axis part
  const int naw = lane >> 4, nay = (lane >> 2) & 3, nax = lane & 3;
  const bool isnode = valid && naw < NB && nay < NB && nax < NB;
  const long long urowxy = isnode ? rsx * AX.rowmap[AX.off[elx] + nax] + rsy * AY.rowmap[AY.off[ely] + nay] : 0;

  struct Run { long long base; double o[5]; bool on, full; };
  auto fetch = [&](int li, Run &r) {
    const int lay = T.lay0 + li;
    r.on = unit && li >= 0 && li < nl && T.cnt[li] > 0 && lay >= own_lo && lay < own_hi;
    if (!r.on) return;
    r.base = RA + (long long)RB * T.pre[li] + (long long)RC * T.cnt[li];
    r.full = patch_layer_full<BW>(T.P + li * 8);
    patch_run_load<BW>(out.val, r.base, T.P + li * 8, r.full, ufirst, r.o);
  };
  auto leave = [&](int li, const Run &r) {
    if (!unit || li < 0) return;
    double *w = win + (li & (PATCH_SLOTS - 1)) * LAYER + rid * 5;
    double v[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) { v[d] = w[d]; w[d] = 0.0; }
    if (!r.on) return;
    const int lay = T.lay0 + li;
    // IGAElementFixJacobian (src/petigaelem.c:1483-1500) on the combined run: rows and columns of fixed nodes emptied, the diagonal counting the elements
    if (fx.reaches(lay)) {
      double rv = 0; const bool rf = fx.fixed(uxr_, uyr, lay, rv);
#pragma unroll
      for (int d = 0; d < 5; ++d) {
        double cv = 0; const bool cf = fx.fixed(uxr_ + udx, uyr + udy, lay + d - P, cv);
        if (rf || cf) v[d] = (d == P && udx == 0 && udy == 0 && rf) ? (double)fx.held(li, uxr_, uyr, ne) : 0.0;
      }
    }
    patch_run_add_store<BW>(out.val, r.base, T.P + li * 8, r.full, r.o, v);
  };
  // the state of element wh + ei at its Gauss points -> the form's point numbers in this wavefront's geo area (as gram_pencil_body's geometry())
  auto state = [&](int ei) {
    if (lane < 32) { const int q = lane >> 3, a = (lane >> 1) & 3, k = lane & 1; geo[GZ + lane] = (q < NB && a < NB) ? AW.tab[((size_t)(wh + ei) * NB * NB + q * NB + a) * NDER + k] : 0.0; }
    if (lane >= 32 && lane < 48) { const int l2 = lane - 32, q = l2 >> 2, a = l2 & 3; d2w[lane] = (q < NB && a < NB) ? AW.tab[((size_t)(wh + ei) * NB * NB + q * NB + a) * NDER + 2] : 0.0; }
    __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    double uc = 0.0;
    if (isnode) {
      const int li = ei + naw;
      const long long urow = (long long)T.rho[li] + urowxy;
      uc = out.U[urow];
      double fv = 0;
      if (fx.any && fx.fixed(wi + nax, wj + nay, T.lay0 + li, fv)) uc = S.fixtable ? S.fixtable[urow] : fv;
    }
    double xpar[3] = {0, 0, 0};
    const int gqx = lane & 3, gqy = (lane >> 2) & 3, gqw = lane >> 4;
    if (gqx < NB && gqy < NB && gqw < NB && valid) { xpar[0] = AW.pt[(wh + ei) * NB + gqw]; xpar[1] = AX.pt[elx * NB + gqx]; xpar[2] = AY.pt[ely * NB + gqy]; }
    pencil_state_eval<P, Form>(geo, d2w, lane, uxr, vyr, geo + GZ, wjxy * (gqw < NB ? T.wq[ei * 4 + gqw] : 0.0), uc, prm.v, out.shift, out.t, xpar);
  };

  // Schedule (a column = the span between two barriers):
  //   group 0:  mfma(0) | flush(0) | mfma(1) | flush(1) | ...          flush(e) of group 0: layer e - 1 leaves, state of element e + 1
  //   group 1:          | mfma(0)  | flush(0)| mfma(1)  | ...          flush(e) of group 1: layer e leaves,     state of element e + 1
  // Layer e is complete when both groups' mfma(e) are: group 1 leaves its runs of it right away, group 0 a column later, both while the
  // other group adds to the layers above only; with four slots, slot (e & 3) is empty again before mfma(e + 2) of group 0 reaches layer e + 4.
  const int lag = grp == 0 ? 1 : 0;
  Run run; run.on = false;
  fetch(-lag, run);
  if (valid) state(0);
  if (grp == 1) __syncthreads();
  for (int ei = 0; ei < ne; ++ei) {
    if (valid) {
      d4_t pk[4];
      pencil_mfma_state_p2k<Form, false, P2kLaneT<false>>(pk, uxr, vyr, geo + GZ, d2w, geo, K, lane);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = (code[t][i >> 1] >> (16 * (i & 1))) & 0xffff;
          if (c != 0xffff) (void)__hip_atomic_fetch_add(win + ((ei + (c & 3)) & (PATCH_SLOTS - 1)) * LAYER + (c >> 2), pk[t][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    __builtin_amdgcn_s_setprio(3);      // (the partner wavefront streams MFMAs now: without priority this one gets the left-over issue slots)
    leave(ei - lag, run); fetch(ei - lag + 1, run);
    if (valid && ei + 1 < ne) state(ei + 1);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }
  if (grp == 0) __syncthreads();
  // every element is in the window: what is left of it (group 0's runs of the last layer; the last segment's two layers beyond)
  const int last = (seg == pa.nseg - 1 && !pa.open_hi) ? ne + P - 1 : ne - 1;
  for (int li = ne - lag; li <= last; ++li) { leave(li, run); fetch(li + 1, run); }
}


}  // namespace igx
