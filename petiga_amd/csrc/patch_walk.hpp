// patch_walk.hpp -- what the walks of a PATCH of adjacent pencils share: gram_patch_p2 and state_patch_p2 (gram_patch.hpp, p = 2) and
// gram_pencil_patch3 (gram_patch3.hpp, p = 3).
//
// One workgroup of MX x MY wavefronts walks MX x MY adjacent pencils in step and combines their band rows in one window in LDS; a
// "pair" of an axis is two nodes of the patch that share one of its elements, a RUN the 2p + 1 walk-axis entries of one (y pair, x pair)
// and node layer.  Here, once, templated on the degree P (and the patch shape where it enters): the shape's constants, the decode of a
// workgroup, the walk-axis layer table, the pair tables, the Dirichlet fix-up of a combined run, a run's matrix address and first-touch
// rule, the load / add / store of a run (the host's arguments and segments of one colour: pencil_launch.hpp).  What differs for measured reasons stays
// with each kernel: the LDS carve-up, the window and its zeroing, the element phase, the F and lifting stages, which thread owns which
// run, the barriers.
//
// Every helper is __forceinline__ and its state scalars: nothing here goes through memory or is indexed dynamically.
#pragma once
#include "gram_mfma.hpp"

namespace igx {

template <int P_, int MX_, int MY_> struct PatchShape {
  static constexpr int P = P_, MX = MX_, MY = MY_, BW = 2 * P + 1;
  static constexpr int W = MX * MY;                                               // pencils (= wavefronts) of a workgroup
  static constexpr int NX = MX + P, NY = MY + P, NODES = NX * NY;                 // nodes of a patch on axes 1, 2
  static constexpr int NXP = BW * MX + P * P, NYP = BW * MY + P * P;              // node pairs that share an element of the patch
  static constexpr int PAIR_INTS = NX * BW + NY * BW + NXP + NYP + 8;             // the pair tables XP, YP, XI, YI and their counts
  static constexpr int SX = MX >= P ? 2 : 3, SY = MY >= P ? 2 : 3;                // colours per axis: patches SX apart share no node
  // the segment cost model counts the resident workgroups per CU from the LDS size at p = 3 (launch bounds (., 1): the LDS decides);
  // the p = 2 walks were tuned counting one workgroup per CU
  static constexpr bool SLOTS_FROM_LDS = P >= 3;
  static_assert(MX >= 2 && MY >= 2 && 2 * MX >= P && 2 * MY >= P, "a patch of at least 2 x 2 pencils; three colours separate the patches of an axis");
};

struct PatchArgs {
  PencilArgs pa;                         // walk-axis range and segments, forcing, first touch (as for the pencil walk)
  int px_start, px_step, px_count;       // patches of this colour: patch indices on axis 1 ...
  int py_start, py_step, py_count;       // ... and on axis 2
};

// ---- a workgroup's patch, segment and this wavefront's pencil, from the index of its item (segment, patch) of the colour: blockIdx.x
// where a workgroup walks one item, the ticket's item where resident workgroups take theirs from a counter (gram_patch3.hpp)
struct PatchWalk {
  int seg, ppx, ppy;       // segment of the walk axis, patch indices on axes 1, 2
  int ex0, ey0, mxv, myv;  // first element of the patch, elements of the patch inside the mesh
  int wi, wj, elx, ely;    // this wavefront's pencil in the patch, its elements (those of pencil (0, 0) when it has none: valid)
  int ws, we, wh, ne, nl;  // the segment's elements [ws, we), its first walked element (halo), elements and node layers walked
  bool valid;
};
template <class G>
__device__ __forceinline__ PatchWalk patch_decode(const SpaceDev &S, const PatchArgs &A, int wave, int item) {
  const PencilArgs &pa = A.pa;
  PatchWalk D;
  D.seg = item / pa.blocks_per_seg;
  const int patch = item - D.seg * pa.blocks_per_seg;
  const int tx = patch % A.px_count, ty = patch / A.px_count;
  D.ppx = A.px_start + tx * A.px_step; D.ppy = A.py_start + ty * A.py_step;
  D.ex0 = D.ppx * G::MX; D.ey0 = D.ppy * G::MY;
  D.mxv = min(G::MX, pa.nelx - D.ex0); D.myv = min(G::MY, pa.nely - D.ey0);
  D.wi = wave % G::MX; D.wj = wave / G::MX;
  D.valid = D.wi < D.mxv && D.wj < D.myv;
  D.elx = D.ex0 + (D.valid ? D.wi : 0); D.ely = D.ey0 + (D.valid ? D.wj : 0);
  D.ws = pa.w_lo + D.seg * pa.seg_len; D.we = min(D.ws + pa.seg_len, pa.w_hi);
  D.wh = max(D.ws - G::P, pa.w_halo_lo);
  D.ne = D.we - D.wh; D.nl = D.ne + G::P;
  return D;
}
// the node layers [own_lo, own_hi) that leave through this segment (the first takes what lies below, the last what lies above)
__device__ __forceinline__ void patch_owned_layers(const SpaceDev &S, const PatchArgs &A, const PatchWalk &D, int &own_lo, int &own_hi) {
  const PencilArgs &pa = A.pa;
  const AxisDev &AW = S.ax[0];
  own_lo = (D.seg == 0 && pa.w_halo_lo == pa.w_lo) ? -1 : AW.off[D.ws];
  own_hi = (D.seg == pa.nseg - 1 && !pa.open_hi) ? (1 << 30) : AW.off[D.we];
}

// ---- the walk-axis layer table of the segment: CSR row, count, prefix and band positions of node layer T.lay0 + i (count -1 beyond the mesh)
template <int BW>
__device__ __forceinline__ void patch_stage_layers(const PencilLds &T, const AxisDev &AW, int nl, int tid, int nthr) {
  for (int i = tid; i < nl; i += nthr) {
    const int lay = T.lay0 + i;
    if (lay < AW.gwidth) {
      const int rho = AW.rowmap[lay];
      T.rho[i] = rho; T.cnt[i] = AW.rcnt[rho]; T.pre[i] = AW.prefix[rho];
      for (int d = 0; d < BW; ++d) T.P[i * 8 + d] = AW.P[lay * BW + d];
    } else { T.rho[i] = 0; T.cnt[i] = -1; T.pre[i] = 0; }
  }
}

// ---- the pair tables (threads 0 and 1: axes 1 and 2).  Pairs (r, r + d) of an axis that share one of the patch's mv elements k:
// max(r, c) - P <= k <= min(r, c), 0 <= k < mv.  PT[r][d + P] = the pair's index or -1, PI[index] = r | (d + P) << 8, cntp[axis] = their count
template <class G>
__device__ __forceinline__ void patch_pair_tables(int *XP, int *YP, int *XI, int *YI, int *cntp, int mxv, int myv, int tid) {
  constexpr int P = G::P, BW = G::BW;
  if (tid >= 2) return;
  const int nn = tid == 0 ? G::NX : G::NY, mv = tid == 0 ? mxv : myv;
  int *PT = tid == 0 ? XP : YP, *PI = tid == 0 ? XI : YI;
  int n = 0;
  for (int r = 0; r < nn; ++r) for (int d = -P; d <= P; ++d) {
    const int c = r + d, hi = r > c ? r : c, lo = r < c ? r : c;
    const bool ok = c >= 0 && c < nn && max(hi - P, 0) <= min(lo, mv - 1);
    PT[r * BW + d + P] = ok ? n : -1;
    if (ok) PI[n++] = r | ((d + P) << 8);
  }
  cntp[tid] = n;
}
template <int P>
__device__ __forceinline__ void patch_pair(int entry, int &r, int &d) { r = entry & 255; d = (entry >> 8) - P; }

// ---- Dirichlet data of the patch (IGAElementBuildFix, src/petigaelem.c:1214-1283: a node is fixed by position, later faces override
// earlier ones: axis 0, 1, 2; side 0, 1).  The fix-up of a combined run restates IGAElementFixSystem / IGAElementFixJacobian
// (src/petigaelem.c:1377-1387, 1483-1500) for rows combined across elements: the kernels apply it with fixed(), reaches() and held().
template <int P> struct PatchFix {
  bool any = false, xlo = false, xhi = false, ylo = false, yhi = false;
  int wlo = -1000, whi = -1000;      // the fixed node layers of the walk axis
  int mxv = 0, myv = 0;
  double vwlo = 0, vwhi = 0, vxlo = 0, vxhi = 0, vylo = 0, vyhi = 0;
  __device__ __forceinline__ void fill(const SpaceDev &S, const PatchWalk &D) {
    constexpr int X = 1, Y = 2;
    const AxisDev &AW = S.ax[0], &AX = S.ax[1], &AY = S.ax[2];
    mxv = D.mxv; myv = D.myv;
    xlo = !AX.periodic && S.bcv[X][0].count > 0 && D.ex0 + AX.estart == 0;                       vxlo = S.bcv[X][0].value[0];
    xhi = !AX.periodic && S.bcv[X][1].count > 0 && D.ex0 + D.mxv + AX.estart == AX.esizes;       vxhi = S.bcv[X][1].value[0];
    ylo = !AY.periodic && S.bcv[Y][0].count > 0 && D.ey0 + AY.estart == 0;                       vylo = S.bcv[Y][0].value[0];
    yhi = !AY.periodic && S.bcv[Y][1].count > 0 && D.ey0 + D.myv + AY.estart == AY.esizes;       vyhi = S.bcv[Y][1].value[0];
    if (!AW.periodic && S.bcv[0][0].count > 0 && AW.estart == 0) { wlo = AW.off[0]; vwlo = S.bcv[0][0].value[0]; }
    if (!AW.periodic && S.bcv[0][1].count > 0 && AW.estart + AW.nel == AW.esizes) { whi = AW.off[AW.nel - 1] + P; vwhi = S.bcv[0][1].value[0]; }
    any = xlo || xhi || ylo || yhi || wlo > -1000 || whi > -1000;
  }
  __device__ __forceinline__ bool fixed(int xr, int yr, int lay, double &val) const {      // node (layer lay, patch nodes yr, xr)
    bool f = false;
    if (lay == wlo) { f = true; val = vwlo; }
    if (lay == whi) { f = true; val = vwhi; }
    if (xlo && xr == 0) { f = true; val = vxlo; }
    if (xhi && xr == mxv + P - 1) { f = true; val = vxhi; }
    if (ylo && yr == 0) { f = true; val = vylo; }
    if (yhi && yr == myv + P - 1) { f = true; val = vyhi; }
    return f;
  }
  // the rows the fix-up can reach: a patch on a face of axis 1 or 2, or within p layers of a fixed layer of the walk axis -- patch-uniform
  __device__ __forceinline__ bool reaches(int lay) const {
    return any && (xlo || xhi || ylo || yhi || (lay >= wlo - P && lay <= wlo + P) || (lay >= whi - P && lay <= whi + P));
  }
  // elements of the patch's walk (ne of them) that hold node (layer li of the segment, yr, xr): the diagonal of a fixed row counts
  // them, each sets K_kk = 1
  __device__ __forceinline__ int held(int li, int xr, int yr, int ne) const {
    return (min(li, ne - 1) - max(li - P, 0) + 1) * (min(xr, mxv - 1) - max(xr - P, 0) + 1) * (min(yr, myv - 1) - max(yr - P, 0) + 1);
  }
};

// ---- a run's matrix address: for the run (x pair (xr, xr + dx), y pair (yr, yr + dy)) of the patch at elements (ex0, ey0),
// pos = RA + RB prefix0(layer) + RC count0(layer) + P0(layer, d)
template <int P>
__device__ __forceinline__ void patch_run_address(const SpaceDev &S, int ex0, int ey0, int xr, int dx, int yr, int dy, long long &RA, int &RB, int &RC) {
  constexpr int BW = 2 * P + 1;
  const AxisDev &AX = S.ax[1], &AY = S.ax[2];
  const int ixg = AX.off[ex0] + xr, iyg = AY.off[ey0] + yr;
  const int rhox = AX.rowmap[ixg], rhoy = AY.rowmap[iyg];
  const long long ps1 = AX.prefix[rhox], ps2 = AY.prefix[rhoy];
  const int c1 = AX.rcnt[rhox], c2 = AY.rcnt[rhoy], P1 = AX.P[ixg * BW + dx + P], P2 = AY.P[iyg * BW + dy + P];
  const long long T0 = S.ax[0].tot, T10 = S.ax[1].tot * S.ax[0].tot;
  RA = ps2 * T10 + (long long)c2 * (ps1 * T0); RB = c2 * c1; RC = P2 * c1 + P1;
}

// ---- First touch: the colours are launched (cx, cy) = (0,0), (1,0), ..., cy-major, and a pair (r, c) of an axis is also held by the
// patches of the other elements that share it.  A patch stores -- no read -- when, on both axes, no patch of an earlier colour holds
// the pair: when its colour is the lowest among the pair's patches (the first colour of the holders is their lowest cy, then their
// lowest cx).  With two colours this is the even / odd rule the p = 2 walks were written with (an even patch always; an odd one unless
// both nodes are among the p it shares with a neighbour): compared by brute force at P = 2, patches 2, 3 and 4 wide, 1 to 40 elements,
// every patch and valid pair -- 16008 pairs, no disagreement.
template <int P>
__device__ __forceinline__ bool patch_axis_first(int pp, int s, int m, int e0, int nel, int r, int c) {
  const int lo = max(e0 + max(r, c) - P, 0), hi = min(e0 + min(r, c), nel - 1);
  int mn = s;
  for (int q = lo / m; q <= hi / m; ++q) mn = min(mn, q % s);
  return pp % s == mn;
}
template <class G>
__device__ __forceinline__ bool patch_first_touch(const PatchArgs &A, const PatchWalk &D, int xr, int dx, int yr, int dy) {
  return patch_axis_first<G::P>(D.ppx, G::SX, G::MX, D.ex0, A.pa.nelx, xr, xr + dx) &&
         patch_axis_first<G::P>(D.ppy, G::SY, G::MY, D.ey0, A.pa.nely, yr, yr + dy);
}

// ---- a run's old values and its add and store.  p0 = the layer's band positions P0(layer, .) (registers or LDS); full = they are
// 0 .. BW - 1 (an interior layer: the run is BW contiguous doubles, 8-byte aligned); first = a first touch, stored without a read
template <int BW>
__device__ __forceinline__ bool patch_layer_full(const int *p0) {
  bool full = true;
#pragma unroll
  for (int d = 0; d < BW; ++d) full = full && p0[d] == d;
  return full;
}
template <int BW>
__device__ __forceinline__ void patch_run_load(const double *val, long long base, const int *p0, bool full, bool first, double (&o)[BW]) {
  const double *p = val + base;
  if (first) {
#pragma unroll
    for (int d = 0; d < BW; ++d) o[d] = 0.0;
  } else if (full) {
#pragma unroll
    for (int k = 0; k < (BW - 1) / 2; ++k) { const d2u_t a = *reinterpret_cast<const d2u_t *>(p + 2 * k); o[2 * k] = a[0]; o[2 * k + 1] = a[1]; }
    o[BW - 1] = p[BW - 1];
  } else {
#pragma unroll
    for (int d = 0; d < BW; ++d) o[d] = p0[d] >= 0 ? p[p0[d]] : 0.0;
  }
}
template <int BW>
__device__ __forceinline__ void patch_run_add_store(double *val, long long base, const int *p0, bool full, const double (&o)[BW], const double (&v)[BW]) {
  double *p = val + base;
  if (full) {
#pragma unroll
    for (int k = 0; k < (BW - 1) / 2; ++k) { d2u_t a; a[0] = o[2 * k] + v[2 * k]; a[1] = o[2 * k + 1] + v[2 * k + 1]; *reinterpret_cast<d2u_t *>(p + 2 * k) = a; }
    p[BW - 1] = o[BW - 1] + v[BW - 1];
  } else {
#pragma unroll
    for (int d = 0; d < BW; ++d) if (p0[d] >= 0) p[p0[d]] = o[d] + v[d];
  }
}


}  // namespace igx
