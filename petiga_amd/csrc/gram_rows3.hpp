// gram_rows3.hpp -- the p = 3 Gram matrix gathered by rows: a row's owner adds the contributions of the at most 64 elements that hold
// its node and stores the finished row, once, without reading memory (round 13).
//
// The patch walk (gram_patch3.hpp) scatters an element's tiles into a window and read-add-writes 745 entries per element in six
// colours where 343 are compulsory.  Here nobody scatters.  An ITEM is a tile of 3 x 3 node columns (axes 1, 2) times a segment of node
// layers of axis 0; its workgroup computes every entry of every row in it.  With the 1-D Gram sums of each element on its own,
//   G_e[k][ta][tb] (walk axis, staged per segment in LDS, zero for an element outside the mesh), X_e[k][ia][ib], Y_e[k][ja][jb]
// (k = 0 values, 1 first derivatives; each from its element's points and weights, scaled by sqrt(w J) as the patch walk's), entry
//   A[(L, ax, ay), (L + d, ax + dx, ay + dy)] = sum_ja sum_ia sum_ta  G_{L-ta}[0][ta][ta+d] mxy + G_{L-ta}[1][ta][ta+d] mw,
//   mw = X_{ax-ia}[0][ia][ia+dx] Y_{ay-ja}[0][ja][ja+dy],   mxy = X[1] Y[0] + X[0] Y[1]  (same indices):
// each term is one element's product g0_e mxy_pencil + g1_e mw_pencil as the patch walk's `products` forms it, added by ONE thread in
// the order (ja, ia, ta).  No Gram factor is summed across elements or pencils before the product, no entry takes part in an LDS add or
// an atomic, no colours, no first touch: bit-repeatable whatever the grid and the ticket order.
//
// Mapping: a thread owns one RUN -- (node column, dy, dx), the seven walk-axis entries d = -3 .. 3 -- for the whole segment, as in the
// patch walk; its planes mw, mxy (at most 16 pairs) stay in registers, only G changes with the layer (a workgroup-uniform LDS read).
// Threads are ordered (dy, node column, dx): wavefront w < 7 has dy = w - 3 and loops over exactly its 4 - |dy| pencils in y; its 63
// lanes are 9 columns x 7 dx, so the seven lanes of a column store 49 consecutive doubles of the row (columns are ordered y, x, layer)
// and the seven wavefronts the row's 343.  Placed round-robin, the wavefronts load every SIMD with four pencil-rows.  Wavefront 7 owns
// the F rows of the nine columns and gathers the liftings of the Dirichlet rows.
//
// Staged stores (round 14, Rows3Args::stage): on a FULL layer (seven band positions on the walk axis) of a REGULAR tile (every node column
// at least three nodes from both ends of axes 1 and 2) a column's row is 343 consecutive doubles in the order (dy, dx, d) and the next
// layer's row follows it directly.  There the run lanes write their finished runs to one of two LDS buffers in memory order, and after one
// barrier all eight wavefronts copy the nine rows out, consecutive lanes storing consecutive doubles: a store instruction covers 512
// contiguous bytes of a row where a run lane's covers 63 pieces at a 56-byte stride.  Same values from the same adder; every other layer
// and tile keeps the per-run stores.
//
// Degree 3, identity geometry, one rank, no wrapped axis, one new node per element on every axis; System and Matrix drivers,
// Dirichlet values on any face.  Boundary loads: the per-face launch that runs first (F is added to).
#pragma once
#include "patch_walk.hpp"

namespace igx {

struct Rows3 {
  static constexpr int P = 3, BW = 7, TX = 3, TY = 3, COLS = TX * TY, RUNW = BW, W = RUNW + 1, NTHR = W * 64;
  static constexpr int ES = TX + P;            // elements of an axis that hold a node of the tile (TX = TY)
  static constexpr int RUNS = BW * BW;         // runs of a row
  static constexpr int ROW = RUNS * BW;        // entries of a full row of a regular tile
  static constexpr int STG = COLS * ROW;       // doubles of a staged tile-layer
  static constexpr int NCOPY = (STG + NTHR - 1) / NTHR;      // doubles a thread copies per staged layer
  static_assert(COLS * BW <= 64 && TX == TY, "a wavefront holds the runs (column, dx) of one dy");
  static_assert((NCOPY - 1) * NTHR <= STG, "only a thread's last copy can lie beyond the buffer");
};
// where the entry (node column col of the tile, dy, dx, d) of a full layer of a regular tile lies in the staged tile-layer: the column's
// row, in memory order -- RC 7 + P0[d] of patch_run_address and the layer table
__host__ __device__ static inline int rows3_stage_offset(int col, int dy, int dx, int d) {
  using R = Rows3;
  return col * R::ROW + ((dy + R::P) * R::BW + dx + R::P) * R::BW + d + R::P;
}

struct Rows3Args {
  double forcing;
  int nel0, nelx, nely;      // elements of the mesh
  int nl0, nnx, nny;         // node layers of axis 0, nodes of axes 1, 2
  int ntx, nty;              // tiles of node columns
  int seg_len, nseg;         // node layers per segment, segments: item = tile * nseg + segment (a column's rows follow each other in memory)
  int *counter;              // the assembly's ticket counter (null: one workgroup per item)
  int stage;                 // full layers of regular tiles leave through LDS as contiguous spans (the launch's LDS holds the buffers)
};

// LDS: G [seg_len + 3 elements][4 ta][4 tb][2], wq [seg_len + 3][4], X and Y [ES][2][16], the F factors of axes 1, 2, the liftings of a layer's
// runs, the two buffers of a staged tile-layer (stage only), the nine column bases, a layer's prefix where it is full, the layer table,
// the ticket
__host__ __device__ static inline size_t rows3_lds_bytes(int seg_len, bool stage) {
  using R = Rows3;
  const size_t doubles = (size_t)(seg_len + 3) * 36 + 2 * R::ES * 32 + 2 * R::ES * 4 + 2 * 8 + ((R::COLS * R::RUNS + 7) & ~7) + (stage ? 2 * ((R::STG + 1) & ~1) : 0);
  return doubles * 8 + (size_t)(R::COLS + 1) * 8 + (size_t)seg_len * 8 + (size_t)seg_len * 8 + (size_t)seg_len * 4 * 10 + 64;
}

// elements that hold node n of an axis of nel elements
__host__ __device__ static inline int rows3_held(int n, int nel) { return (n < nel - 1 ? n : nel - 1) - (n > 3 ? n - 3 : 0) + 1; }

template <bool SYSTEM, bool TICKETS>
__global__ void __launch_bounds__(Rows3::NTHR, 1)
gram_pencil_rows3(SpaceDev S, OutDev out, Rows3Args A) {
  using R = Rows3;
  constexpr int P = R::P, NB = 4, BW = R::BW, NTHR = R::NTHR, ES = R::ES;
  extern __shared__ __attribute__((aligned(16))) double pencil_sm[];
  const AxisDev &AW = S.ax[0], &AX = S.ax[1], &AY = S.ax[2];
  const int sl = A.seg_len, net = sl + 3, nitems = A.ntx * A.nty * A.nseg;
  double *G = pencil_sm, *wq = G + net * 32, *Xt = wq + net * 4, *Yt = Xt + ES * 32, *sxl = Yt + ES * 32, *syl = sxl + ES * 4, *Jxl = syl + ES * 4, *Jyl = Jxl + 8;
  double *corr = Jyl + 8;      // [column][dy][dx]: the lifting sum_k K_ik v_k of the run's row over its fixed columns
  double *stg = corr + ((R::COLS * R::RUNS + 7) & ~7);      // [2][column][dy][dx][d]: the finished rows of a staged tile-layer, in memory order
  long long *colbase = reinterpret_cast<long long *>(stg + (A.stage ? 2 * ((R::STG + 1) & ~1) : 0));      // a regular tile's columns: where the row of prefix 0 begins
  long long *lrow = colbase + R::COLS + 1;      // the layer's prefix where it is full (T.cnt = 7, band positions 0 .. 6), else -1: all a layer's stores ask
  PencilLds T;
  T.zt = G; T.wq = wq; T.Jz = nullptr;
  T.pre = lrow + sl;
  T.cnt = reinterpret_cast<int *>(T.pre + sl); T.rho = T.cnt + sl; T.P = T.rho + sl;
  int *tick = T.P + sl * 8;

  int ticket = blockIdx.x;
  if (ticket >= nitems) return;      // (a workgroup beyond the items: IGX_ROWS3_GRID)
  do {
  // (the thread's index is made opaque once per item, as in gram_pencil_patch3: what depends on it alone is computed again in every item
  //  instead of being carried in registers across the walk)
  int tid = threadIdx.x;
  if constexpr (TICKETS) asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the next ticket, asked for at the head of this item: its latency passes under the walk
  int next_ticket = 0;
  if (TICKETS && tid == 0) next_ticket = (int)gridDim.x + __hip_atomic_fetch_add(A.counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int item = ticket;
  const int tile = item / A.nseg, seg = item - tile * A.nseg;
  const int ty = tile / A.ntx, tx = tile - ty * A.ntx;
  const int ax0 = tx * R::TX, ay0 = ty * R::TY;
  const int l_lo = seg * sl, nlay = min(l_lo + sl, A.nl0) - l_lo;      // the segment's node layers [l_lo, l_lo + nlay), counted from the axis' first
  // (workgroup-uniform) a regular tile: each of its rows has 7 x 7 column pairs on axes 1, 2
  const bool regular = A.stage && ax0 >= P && ax0 + R::TX - 1 <= A.nnx - 1 - P && ay0 >= P && ay0 + R::TY - 1 <= A.nny - 1 - P;

  {   // ---- the tables of the item.  Element slot i of G and wq is element l_lo - 3 + i of the walk axis, slot i of the others element
      // ax0 - 3 + i (ay0 - 3 + i); an element outside the mesh leaves zeroes: the loops below have no branches
    for (int i = tid; i < net * 32; i += NTHR) {
      const int j = i & 31, ta = j >> 3, tb = (j >> 1) & 3, k = j & 1, eg = l_lo - P + (i >> 5);
      double g = 0;
      if (eg >= 0 && eg < A.nel0) {
        const double *tw = AW.tab + (size_t)eg * NB * NB * NDER;
#pragma unroll
        for (int q = 0; q < NB; ++q) { const double sq = sqrt(AW.w[eg * NB + q] * AW.J[eg]); g += (tw[(q * NB + ta) * NDER + k] * sq) * (tw[(q * NB + tb) * NDER + k] * sq); }
      }
      G[i] = g;
    }
    for (int i = tid; i < net * 4; i += NTHR) {
      const int a = i & 3, eg = l_lo - P + (i >> 2);
      double sw = 0;
      if (eg >= 0 && eg < A.nel0) {
#pragma unroll
        for (int q = 0; q < NB; ++q) { const double sq = sqrt(AW.w[eg * NB + q] * AW.J[eg]); sw += sq * (AW.tab[((size_t)eg * NB * NB + q * NB + a) * NDER] * sq); }
      }
      wq[i] = sw;
    }
    T.lay0 = AW.off[0] + l_lo;
    patch_stage_layers<BW>(T, AW, nlay, tid, NTHR);
    for (int i = tid; i < nlay; i += NTHR) lrow[i] = (T.cnt[i] == BW && patch_layer_full<BW>(T.P + i * 8)) ? T.pre[i] : -1;      // (the thread that staged the layer)
    if (regular && tid < R::COLS) {
      long long ca = 0; int cb = 0, cc = 0;
      patch_run_address<P>(S, 0, 0, ax0 + tid % R::TX, -P, ay0 + tid / R::TX, -P, ca, cb, cc);
      colbase[tid] = ca + (long long)cc * BW;
    }
    for (int i = tid; i < 2 * ES * 32; i += NTHR) {      // X, then Y: [slot][k][ia][ib]
      const bool isy = i >= ES * 32;
      const int j = isy ? i - ES * 32 : i, slot = j >> 5, k = (j >> 4) & 1, ia = (j >> 2) & 3, ib = j & 3;
      const AxisDev &AA = isy ? AY : AX;
      const int eg = (isy ? ay0 : ax0) - P + slot, nel = isy ? A.nely : A.nelx;
      double g = 0;
      if (eg >= 0 && eg < nel) {
        const double *tw = AA.tab + (size_t)eg * NB * NB * NDER;
#pragma unroll
        for (int q = 0; q < NB; ++q) { const double sq = sqrt(AA.w[eg * NB + q] * AA.J[eg]); g += (tw[(q * NB + ia) * NDER + k] * sq) * (tw[(q * NB + ib) * NDER + k] * sq); }
      }
      (isy ? Yt : Xt)[j] = g;
    }
    for (int i = tid; i < 2 * ES * 4; i += NTHR) {      // the F factors sum_q w N of axes 1, 2: [slot][a]
      const bool isy = i >= ES * 4;
      const int j = isy ? i - ES * 4 : i, slot = j >> 2, a = j & 3;
      const AxisDev &AA = isy ? AY : AX;
      const int eg = (isy ? ay0 : ax0) - P + slot, nel = isy ? A.nely : A.nelx;
      double sv = 0;
      if (eg >= 0 && eg < nel) {
#pragma unroll
        for (int q = 0; q < NB; ++q) sv += AA.w[eg * NB + q] * AA.tab[((size_t)eg * NB * NB + q * NB + a) * NDER];
      }
      (isy ? syl : sxl)[j] = sv;
    }
    for (int i = tid; i < 2 * ES; i += NTHR) {
      const bool isy = i >= ES;
      const int slot = isy ? i - ES : i, eg = (isy ? ay0 : ax0) - P + slot, nel = isy ? A.nely : A.nelx;
      (isy ? Jyl : Jxl)[slot] = (eg >= 0 && eg < nel) ? (isy ? AY : AX).J[eg] : 0.0;
    }
  }
  __syncthreads();

  // ---- this thread's run: wavefront w < 7 has dy = w - 3, lane (column, dx); lane 63 and wavefront 7 own none
  const bool runw = wave < R::RUNW;
  const int dy = wave - P;
  const int col = min(lane / BW, R::COLS - 1), dxi = lane - (lane / BW) * BW, dx = dxi - P;
  const int cx = col % R::TX, cy = col / R::TX, ax = ax0 + cx, ay = ay0 + cy;
  const bool node = lane < R::COLS * BW && ax < A.nnx && ay < A.nny;
  bool active = runw && node;
  if (active) active = AX.P[(AX.off[0] + ax) * BW + dxi] >= 0 && AY.P[(AY.off[0] + ay) * BW + dy + P] >= 0;      // (the column node lies inside the mesh)
  long long RA = 0; int RB = 0, RC = 0;
  if (active) patch_run_address<P>(S, 0, 0, ax, dx, ay, dy, RA, RB, RC);
  const long long RA7 = RA + (long long)RC * BW;      // ... on a full layer: pos = RA7 + RB prefix0(layer) + d
  // what this thread copies of a staged tile-layer: doubles tid + k NTHR of the buffer, to their places in the rows of prefix 0
  double *cdst[R::NCOPY];
#pragma unroll
  for (int k = 0; k < R::NCOPY; ++k) {
    const int i = min(tid + k * NTHR, R::STG - 1), c = i / R::ROW;
    cdst[k] = regular ? out.val + colbase[c] + (i - c * R::ROW) : nullptr;
  }
  const int sgo = rows3_stage_offset(col, dy, dx, -P);
  int sb = 0;      // the buffer of the next staged layer: two, so one barrier per layer is enough
  // its planes: pencil (ja, ia) is the element (ay - ja, ax - ia); jj counts the wavefront's 4 - |dy| pencils in y from ja_lo
  const int ja_lo = max(0, -dy), nj = runw ? NB - abs(dy) : 0;
  double mw[NB][NB], mxy[NB][NB];
#pragma unroll
  for (int jj = 0; jj < NB; ++jj)
#pragma unroll
    for (int ia = 0; ia < NB; ++ia) {
      const int ja = ja_lo + jj, jb = ja + dy, ib = ia + dx;
      const bool ok = active && jj < nj && ib >= 0 && ib < NB;
      const int jas = ok ? ja : 0, jbs = ok ? jb : 0, ibs = ok ? ib : 0;
      const double *xt = Xt + (cx + P - ia) * 32 + ia * 4 + ibs, *yt = Yt + (cy + P - jas) * 32 + jas * 4 + jbs;
      const double x0 = ok ? xt[0] : 0.0, x1 = ok ? xt[16] : 0.0, y0 = ok ? yt[0] : 0.0, y1 = ok ? yt[16] : 0.0;
      mw[jj][ia] = x0 * y0;
      mxy[jj][ia] = __builtin_fma(x1, y0, x0 * y1);
    }

  // ---- the F row of wavefront 7's lane c < 9: node column c of the tile.  sxy of pencil (ja, ia) as the patch walk forms it
  const bool frow = SYSTEM && !runw && lane < R::COLS && (ax0 + lane % R::TX) < A.nnx && (ay0 + lane / R::TX) < A.nny;
  const int fcx = frow ? lane % R::TX : 0, fcy = frow ? lane / R::TX : 0, fax = ax0 + fcx, fay = ay0 + fcy;
  double sxy[NB][NB];
  long long frowxy = 0;
  if constexpr (SYSTEM) {
#pragma unroll
    for (int ja = 0; ja < NB; ++ja)
#pragma unroll
      for (int ia = 0; ia < NB; ++ia)
        sxy[ja][ia] = frow ? A.forcing * (sxl[(fcx + P - ia) * 4 + ia] * syl[(fcy + P - ja) * 4 + ja]) * (Jxl[fcx + P - ia] * Jyl[fcy + P - ja]) : 0.0;
    if (frow) frowxy = (long long)AW.nrow * AX.rowmap[AX.off[0] + fax] + (long long)AW.nrow * AX.nrow * AY.rowmap[AY.off[0] + fay];
  }

  // ---- the Dirichlet data of the mesh (PatchFix with the mesh in place of the patch: node indices are the mesh's), and whether the
  // tile lies within p nodes of a fixed face of axis 1 or 2
  PatchFix<P> fx;
  bool tile_reach = false;
  if constexpr (SYSTEM) {
    PatchWalk D;
    D.ex0 = 0; D.ey0 = 0; D.mxv = A.nelx; D.myv = A.nely;
    fx.fill(S, D);
    tile_reach = (fx.xlo && ax0 <= P) || (fx.xhi && ax0 + R::TX - 1 >= A.nnx - 1 - P) || (fx.ylo && ay0 <= P) || (fx.yhi && ay0 + R::TY - 1 >= A.nny - 1 - P);
  }
  const int hxy = rows3_held(ax, A.nelx) * rows3_held(ay, A.nely), fhxy = rows3_held(fax, A.nelx) * rows3_held(fay, A.nely);

  long long tk0 = 0, tw0 = 0;
  if (out.clk) { tk0 = __builtin_readcyclecounter(); tw0 = wall_clock64(); }
  for (int li = 0; li < nlay; ++li) {
    const int lay = T.lay0 + li;
    // (workgroup-uniform: the rows of this layer of the tile that the fix-up can reach)
    const bool bcl = SYSTEM && fx.any && (tile_reach || (lay >= fx.wlo - P && lay <= fx.wlo + P) || (lay >= fx.whi - P && lay <= fx.whi + P));
    const long long lr = lrow[li];
    const bool staged = regular && lr >= 0;      // (workgroup-uniform)
    if (runw) {
      // the Gram sums of the four elements L - ta that hold the layer: slot li + 3 - ta
      double g0[NB][NB], g1[NB][NB];
#pragma unroll
      for (int ta = 0; ta < NB; ++ta)
#pragma unroll
        for (int tb = 0; tb < NB; ++tb) { const double *g = G + (li + P - ta) * 32 + (ta * 4 + tb) * 2; g0[ta][tb] = g[0]; g1[ta][tb] = g[1]; }
      double v[BW];
#pragma unroll
      for (int d = 0; d < BW; ++d) v[d] = 0.0;
#pragma unroll
      for (int jj = 0; jj < NB; ++jj) {
        if (jj < nj) {      // (wavefront-uniform)
#pragma unroll
          for (int ia = 0; ia < NB; ++ia)
#pragma unroll
            for (int ta = 0; ta < NB; ++ta)
#pragma unroll
              for (int tb = 0; tb < NB; ++tb)
                v[tb - ta + P] = __builtin_fma(g0[ta][tb], mxy[jj][ia], __builtin_fma(g1[ta][tb], mw[jj][ia], v[tb - ta + P]));
        }
      }
      if constexpr (SYSTEM) {      // IGAElementFixSystem on the finished run; its row's lifting to wavefront 7
        if (bcl) {
          double c = 0, rv = 0;
          if (active) {
            const bool rf = fx.fixed(ax, ay, lay, rv);
#pragma unroll
            for (int d = 0; d < BW; ++d) {
              double cv = 0; const bool cf = fx.fixed(ax + dx, ay + dy, lay + d - P, cv);
              if (cf) c += v[d] * cv;
              if (rf || cf) v[d] = (d == P && dx == 0 && dy == 0 && rf) ? (double)(rows3_held(l_lo + li, A.nel0) * hxy) : 0.0;
            }
          }
          if (lane < R::COLS * BW) corr[col * R::RUNS + (dy + P) * BW + dxi] = c;
        }
      }
      const double zero[BW] = {0, 0, 0, 0, 0, 0, 0};
      if (staged) {
        if (lane < R::COLS * BW) {      // (a regular tile: every run is active)
          double *sg = stg + sb * ((R::STG + 1) & ~1) + sgo;
#pragma unroll
          for (int d = 0; d < BW; ++d) sg[d] = zero[d] + v[d];
        }
      } else if (active && lr >= 0) {
        patch_run_add_store<BW>(out.val, RA7 + (long long)RB * lr, T.P + li * 8, true, zero, v);
      } else if (active && T.cnt[li] > 0) {
        const int *p0 = T.P + li * 8;
        patch_run_add_store<BW>(out.val, RA + (long long)RB * T.pre[li] + (long long)RC * T.cnt[li], p0, patch_layer_full<BW>(p0), zero, v);
      }
    }
    if (staged) {
      __syncthreads();      // the tile-layer is staged; the other buffer's readers passed the barrier of the layer before
      const double *src = stg + sb * ((R::STG + 1) & ~1);
      const long long adv = (long long)R::RUNS * lr;
#pragma unroll
      for (int k = 0; k < R::NCOPY; ++k)
        if (k + 1 < R::NCOPY || tid + k * NTHR < R::STG) cdst[k][adv] = src[tid + k * NTHR];
      sb ^= 1;
    }
    if constexpr (SYSTEM) {
      if (bcl) __syncthreads();      // the liftings of the layer's runs are staged
      if (frow && T.cnt[li] > 0) {
        // F of the row: the sum over the elements that hold the node, in the order (ja, ia, ta); one add per row and assembly on top of
        // the boundary loads
        double f = 0;
#pragma unroll
        for (int ja = 0; ja < NB; ++ja)
#pragma unroll
          for (int ia = 0; ia < NB; ++ia)
#pragma unroll
            for (int ta = 0; ta < NB; ++ta) f += sxy[ja][ia] * wq[(li + P - ta) * 4 + ta];
        if (bcl) {
          double fv = 0;
          if (fx.fixed(fax, fay, lay, fv)) f = fv * (double)(rows3_held(l_lo + li, A.nel0) * fhxy);
          else {
            const double *cl = corr + lane * R::RUNS;
            double c = 0;
            for (int k = 0; k < R::RUNS; ++k) c += cl[k];
            f -= c;
          }
        }
        (void)__hip_atomic_fetch_add(out.vec + (long long)T.rho[li] + frowxy, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (bcl) __syncthreads();      // ... and read: the next layer may stage its own
    }
  }
  if (out.clk && (item == 0 || item == nitems - 1) && tid == 0) {
    // IGX_CLOCK_PROBE: s_memtime against the 100 MHz s_memrealtime over the walk, first and last item, by whoever walks them
    atomicAdd(reinterpret_cast<unsigned long long *>(out.clk), (unsigned long long)(__builtin_readcyclecounter() - tk0));
    atomicAdd(reinterpret_cast<unsigned long long *>(out.clk) + 1, (unsigned long long)(wall_clock64() - tw0));
    atomicAdd(reinterpret_cast<unsigned long long *>(out.clk) + 2, (unsigned long long)nlay);
  }
  if constexpr (!TICKETS) break;
  // the workgroup learns its next ticket through LDS; the barrier also closes the item: nothing of it is read after this
  if (tid == 0) tick[0] = next_ticket;
  __syncthreads();
  ticket = __builtin_amdgcn_readfirstlane(tick[0]);
  } while (ticket < nitems);
}

}  // namespace igx
