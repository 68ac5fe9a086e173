// gram_patch3.hpp -- the p = 3 Gram walk with the band rows combined across all three axes before they reach memory (round 8).
//
// The sum-factorised pencil walk (gram_pencil<..., SF = true>, gram_mfma.hpp) is bound by its band-row flush alone: a pencil combines
// its rows along the walk axis only and read-add-writes 1792 entries per element, 224 bytes at a time, in 16 colours.  Here a
// workgroup of MX x MY wavefronts walks a PATCH of MX x MY adjacent pencils in step and adds into ONE window in LDS.  A "pair" of an
// axis is two nodes of the patch that share one of its elements (7 m + 9 of them for m elements); a window BLOCK (r, c) holds the
// entries (node layer r, pair y, pair x ; node layer c) for all pairs.  Only the upper walk-axis blocks c = r .. r + 3 are kept:
//   win[16 slots = (c & 3, c - r)][y pair][x pair],
// the lower half of a band row being read transposed from the blocks of its column layer.  Layer L is complete when every wavefront
// has added its element L; its runs (row node, 7 column layers) then leave through the whole workgroup -- (7MX+9)(7MY+9) runs of 7
// entries for MX MY elements: 745 entries per element at 4 x 2 instead of 1792, and 6 colours instead of 16.
//
// The element phase is the pencil walk's: pencil_sf_planes once per pencil, then 2 x 4 v_fma_f64 per tile on the staged walk-axis Gram
// sums.  A tile (ta, tb) of element e belongs to block (e + ta, e + tb), and every tile of a pencil uses the same planes and the same
// window offsets, so a pencil's part of a block is summed over its 4 - d elements in REGISTERS (round 11): a wavefront keeps the ten
// blocks of its four open rows, adds element e's tiles to them (rows e .. e + 3), and row e is then complete: its four blocks go to the
// window once, in eight TICKS between barriers -- in tick k wavefront w adds block d = (k + w) mod 8, if d <= 3 -- and the rows slide.
// 32 LDS instructions and 8 barriers per wavefront and step, where adding every tile to the window took 80 and 10 (round 10 had
// stamped nearly half of a step there).  Every element is still formed from its own Gauss-point data, and the walk-axis Gram sums are
// not summed across elements before the product: only where the partial sums wait has changed.  Bit-repeatable like every walk but
// gram_patch_p2: between two barriers a block belongs to one wavefront and an entry to one lane (a plain LDS read, add and write, no
// atomic), and an entry takes its adds in the order of the ticks (Patch3Ticks and its static_asserts).  Behind the last element of the
// last segment three rows are complete in registers only: one more round of the ticks adds all three to the window before the
// trailing layers leave.  Other segments drop theirs: the next segment's halo forms them again.
// The F stage and the lifting of the Dirichlet rows are summed in a fixed order too (per-run liftings in LDS, gathered
// per node).  Every thread owns RUNS runs for the whole walk; their old values are requested a step ahead and consumed behind the
// barrier that completes the layer.
//
// Degree 3, identity geometry, one rank, axis-0 walk, sum-factorised Gram phase; System and Matrix drivers, Dirichlet values on any
// face, first touch.  Boundary loads: the per-face launch that runs first.
#pragma once
#include "gram_patch.hpp"

namespace igx {

template <int MX, int MY> struct Patch3 : PatchShape<3, MX, MY> {
  using G = PatchShape<3, MX, MY>;
  static constexpr int BLK = G::NXP * G::NYP;                           // doubles per window block (= runs of a layer)
  static constexpr int SLOTS = 16;                                      // blocks (r, r + d), d = 0..3, keyed by (r + d) & 3 and d
  static constexpr int RUNS = (BLK + G::W * 64 - 1) / (G::W * 64);      // runs per thread
  static_assert(G::NXP == 7 * MX + 9 && G::NYP == 7 * MY + 9 && G::SX == (MX >= 3 ? 2 : 3) && G::SY == (MY >= 3 ? 2 : 3), "the patch at p = 3");
  static_assert(G::W <= 10, "at most one wavefront per tile of the element");
  static_assert(G::NODES <= 64 * G::W, "one thread per F row of the patch");
  // the ticks of a step: in tick k wavefront w adds block d = (k + w) mod TICKS of its completed row to the window, if d <= 3
  static constexpr int TICKS = G::W < 4 ? 4 : G::W;
  static constexpr int tick_block(int k, int w) { return (k + w) % TICKS < 4 ? (k + w) % TICKS : -1; }
};
// the table (tick, wavefront) -> block of the row, and what makes the walk bit-repeatable: every wavefront adds each of its four blocks
// once in a step, and no two wavefronts add to one block between two barriers (a window entry takes its adds in the order of the ticks)
template <class G> struct Patch3Ticks { int d[G::TICKS][G::W]; };
template <class G> constexpr Patch3Ticks<G> patch3_ticks() {
  Patch3Ticks<G> t{};
  for (int k = 0; k < G::TICKS; ++k) for (int w = 0; w < G::W; ++w) t.d[k][w] = G::tick_block(k, w);
  return t;
}
template <class G> constexpr bool patch3_ticks_once_each(const Patch3Ticks<G> t) {
  for (int w = 0; w < G::W; ++w) for (int d = 0; d < 4; ++d) {
    int n = 0;
    for (int k = 0; k < G::TICKS; ++k) n += t.d[k][w] == d;
    if (n != 1) return false;
  }
  return true;
}
template <class G> constexpr bool patch3_ticks_one_owner(const Patch3Ticks<G> t) {
  for (int k = 0; k < G::TICKS; ++k) for (int w = 0; w < G::W; ++w) for (int v = w + 1; v < G::W; ++v)
    if (t.d[k][w] >= 0 && t.d[k][w] == t.d[k][v]) return false;
  return true;
}

// LDS behind the walk's tables: the window, the per-run liftings of two layers, the F stage of two layers, the pair tables (ints)
template <int MX, int MY>
__host__ __device__ static inline size_t patch3_lds_bytes(int ne_max) {
  using G = Patch3<MX, MY>;
  return pencil_lds_bytes(ne_max, false, G::W) + (size_t)(G::SLOTS + 2) * G::BLK * 8 + (size_t)2 * G::W * 16 * 8 +
         (size_t)G::PAIR_INTS * 4 + 64;
}

// ---- tickets (round 12).  A colour's ITEMS are its (segment, patch) pairs, item = segment x patches + patch as blockIdx.x used to
// count them.  With a counter, the launch is as many workgroups as the device holds at once; each walks item after item: its first
// TICKET is its index in the grid, every later one gridDim.x + what a relaxed atomicAdd on the colour's counter returns (the counter
// starts at zero: the launcher zeroes all of an assembly's counters ahead of its first launch), until a ticket is at or past the item
// count.  Nobody waits for anybody: no flag, no grid barrier, no spin; the one shared object is the counter, and the loop ends after at
// most items + grid increments.  Without tickets (TICKETS = false: IGX_PATCH3_PERSIST=0, or a colour whose items the device holds at
// once) a workgroup walks item blockIdx.x and leaves.
struct Patch3Tickets {
  int *counter;      // this launch's counter in device memory (null without tickets)
  int order;         // patch3_ticket_item's order
};
// Ticket -> item, a permutation of the colour's items.  order 0: the identity.  order 1, heavy first: the patches on a face of axis 1 or
// 2 (where a Dirichlet fix-up runs in every layer) before the interior ones, as list scheduling would have it; within either class
// segment-major and then in the patches' own order, so that neighbours in memory are still walked at about the same time.
// *face: whether the ticket's patch lies on such a face.
template <class G>
__host__ __device__ inline int patch3_ticket_item(const PatchArgs &A, int order, int t, bool *face = nullptr) {
  const int px = A.px_count, py = A.py_count, npx = (A.pa.nelx + G::MX - 1) / G::MX, npy = (A.pa.nely + G::MY - 1) / G::MY;
  const bool x0 = A.px_start == 0, x1 = A.px_start + (px - 1) * A.px_step == npx - 1;
  const bool y0 = A.py_start == 0, y1 = A.py_start + (py - 1) * A.py_step == npy - 1;
  if (!order) {
    if (face) { const int patch = t % (px * py), tx = patch % px, ty = patch / px; *face = (x0 && tx == 0) || (x1 && tx == px - 1) || (y0 && ty == 0) || (y1 && ty == py - 1); }
    return t;
  }
  // columns and rows with the face ones in front: nfx, nfy of them (the low face first), the others behind in their own order
  const int nfx = (x0 ? 1 : 0) + ((x1 && !(x0 && px == 1)) ? 1 : 0), nfy = (y0 ? 1 : 0) + ((y1 && !(y0 && py == 1)) ? 1 : 0);
  const int nface = nfy * px + (py - nfy) * nfx, nfi = nface * A.pa.nseg;
  int seg, tx, ty;
  if (t < nfi) {
    seg = t / nface;
    const int k = t - seg * nface;
    if (k < nfy * px) { const int r = k / px; ty = (y0 && r == 0) ? 0 : py - 1; tx = k - r * px; }      // a face row, whole
    else { const int k2 = k - nfy * px, r = k2 / nfx, c = k2 - r * nfx; ty = r + (y0 ? 1 : 0); tx = (x0 && c == 0) ? 0 : px - 1; }      // the face columns of another row
  } else {
    const int wd = px - nfx, nin = (py - nfy) * wd, u = t - nfi;
    seg = u / nin;
    const int k = u - seg * nin, r = k / wd;
    ty = r + (y0 ? 1 : 0); tx = k - r * wd + (x0 ? 1 : 0);
  }
  if (face) *face = t < nfi;
  return seg * (px * py) + ty * px + tx;
}

// TICKETS = false is the launch of one workgroup per item with nothing of the loop compiled in (K is not read): the kernel of the rounds
// before, which small meshes keep -- the loop's instantiation carries more across an item and took 5 us longer per launch there.
template <bool SYSTEM, int MX, int MY, bool TICKETS>
__global__ void __launch_bounds__(MX * MY * 64, 1)
gram_pencil_patch3(SpaceDev S, OutDev out, PatchArgs A, Patch3Tickets K) {
  using G = Patch3<MX, MY>;
  constexpr int P = G::P, NB = 4, BW = G::BW, W = G::W, NX = G::NX, NY = G::NY, BLK = G::BLK, NTHR = W * 64;
  static_assert(patch3_ticks_once_each<G>(patch3_ticks<G>()), "a wavefront adds each block of its completed row once in a step");
  static_assert(patch3_ticks_one_owner<G>(patch3_ticks<G>()), "one wavefront per window block between two barriers");
  extern __shared__ __attribute__((aligned(16))) double pencil_sm[];
  const PencilArgs &pa = A.pa;
  const bool stamped = kDebug && pa.debug_buf;
  const int nitems = pa.blocks_per_seg * pa.nseg;
  // Everything an item leaves behind is built again inside the loop: every table in LDS, the window's zeroes, each register the walk
  // keeps (the ten open blocks, the F sums, the old values requested ahead, the Dirichlet data) is declared in the loop's body.  The
  // barrier at its end follows the last read of the trailing layers (leave_f: Fp, corr, the pair tables, the layer table).
  int ticket = blockIdx.x;
  if (TICKETS && ticket >= nitems) return;      // (a workgroup beyond the items: IGX_PATCH3_GRID)
  do {
  // (the thread's index is made opaque once per item: what depends on it alone is then computed again in every item instead of being
  //  carried in registers across the whole walk, which took the System instantiation past its 256 VGPRs)
  int tid = threadIdx.x;
  if constexpr (TICKETS) asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long st_wall0 = stamped ? wall_clock64() : 0;
  // the next ticket, asked for at the head of this item: its latency passes under the walk
  int next_ticket = 0;
  if (TICKETS && tid == 0) next_ticket = (int)gridDim.x + __hip_atomic_fetch_add(K.counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int item = TICKETS ? patch3_ticket_item<G>(A, K.order, ticket) : ticket;
  const PatchWalk D = patch_decode<G>(S, A, wave, item);
  const int seg = D.seg, ex0 = D.ex0, ey0 = D.ey0, mxv = D.mxv, myv = D.myv, wi = D.wi, wj = D.wj, elx = D.elx, ely = D.ely, wh = D.wh, ne = D.ne, nl = D.nl;
  const bool valid = D.valid;
  const AxisDev &AW = S.ax[0], &AX = S.ax[1], &AY = S.ax[2];

  PencilLds T = pencil_lds_carve(pencil_sm, pa.ne_max, false);
  T.lay0 = AW.off[wh];
  double *win = reinterpret_cast<double *>(reinterpret_cast<char *>(pencil_sm) + pencil_lds_bytes(pa.ne_max, false, W));
  double *corr = win + G::SLOTS * BLK;          // [layer & 1][run]: the lifting sum_k K_ik v_k of the run's row over its fixed columns
  double *Fp = corr + 2 * BLK;                  // [layer & 1][wave][16]: the leaving layer's F sums of each pencil
  int *XP = reinterpret_cast<int *>(Fp + 2 * W * 16), *YP = XP + NX * 7, *XI = YP + NY * 7, *YI = XI + G::NXP, *cntp = YI + G::NYP;
  // this wavefront's pencil: its Y-axis rows [a][q][2] (scaled by sqrt(w J)) in LDS, as gram_pencil_body stages them
  double *vyw = reinterpret_cast<double *>(reinterpret_cast<char *>(pencil_sm) + (pencil_lds_bytes(pa.ne_max, false, W) - (size_t)2 * W * 32 * 8)) + wave * 32;
  PencilLane L;
  double sxy = 0;
  {   // the walk-axis tables of the segment (the Gram sums G_k and F factors of the sum-factorised walk), the window, the pair tables
    for (int i = tid; i < ne * 32; i += NTHR) {
      const int e = i >> 5, j = i & 31, ta = j >> 3, tb = (j >> 1) & 3, k = j & 1, eg = wh + e;
      const double *tw = AW.tab + (size_t)eg * NB * NB * NDER;
      double g = 0;
#pragma unroll
      for (int q = 0; q < NB; ++q) { const double sq = sqrt(AW.w[eg * NB + q] * AW.J[eg]); g += (tw[(q * NB + ta) * NDER + k] * sq) * (tw[(q * NB + tb) * NDER + k] * sq); }
      T.zt[i] = g;
    }
    for (int i = tid; i < ne * 4; i += NTHR) {
      const int e = i >> 2, a = i & 3, eg = wh + e;
      double sw = 0;
#pragma unroll
      for (int q = 0; q < NB; ++q) { const double sq = sqrt(AW.w[eg * NB + q] * AW.J[eg]); sw += sq * (AW.tab[((size_t)eg * NB * NB + q * NB + a) * NDER] * sq); }
      T.wq[i] = sw;
    }
    patch_stage_layers<BW>(T, AW, nl, tid, NTHR);
    for (int i = tid; i < G::SLOTS * BLK; i += NTHR) win[i] = 0.0;
    patch_pair_tables<G>(XP, YP, XI, YI, cntp, mxv, myv, tid);
    const double *__restrict__ TX = AX.tab + (size_t)elx * (NB * NB * NDER);
    const double *__restrict__ TY = AY.tab + (size_t)ely * (NB * NB * NDER);
    const double *__restrict__ WX = AX.w + elx * NB, *__restrict__ WYq = AY.w + ely * NB;
    const int qx = lane >> 4, ix = lane & 3, iy = (lane >> 2) & 3;
    const double sx0 = sqrt(WX[qx] * AX.J[elx]);
    L.u0 = TX[(qx * NB + ix) * NDER + 0] * sx0; L.u1 = TX[(qx * NB + ix) * NDER + 1] * sx0;
    if (lane < 32) { const int aa = lane >> 3, qq = (lane >> 1) & 3, kk = lane & 1; vyw[lane] = TY[(qq * NB + aa) * NDER + kk] * sqrt(WYq[qq] * AY.J[ely]); }
    L.vy = vyw + iy * 8;
    if constexpr (SYSTEM) {      // F lane (fx = lane & 3, fy = (lane >> 2) & 3, walk-axis slot = lane >> 4): forcing * sum_q w N on axes 1, 2
      const int fx = lane & 3, fy = (lane >> 2) & 3;
      double sx = 0, sy = 0;
#pragma unroll
      for (int q = 0; q < NB; ++q) { sx += WX[q] * TX[(q * NB + fx) * NDER]; sy += WYq[q] * TY[(q * NB + fy) * NDER]; }
      sxy = valid ? pa.forcing * (sx * sy) * (AX.J[elx] * AY.J[ely]) : 0.0;
    }
  }
  __syncthreads();
  const int nxp = cntp[0], nyp = cntp[1], nruns = nxp * nyp;

  // ---- the pencil's x-y planes of the Gram block (12 MFMAs), and where this lane's entries go in a window block: tile entry (row a, r ;
  // column b1, b2) is (y pair (wj + r, wj + b2), x pair (wi + a, wi + b1)) -- the same for all ten tiles
  d4_t mw, mxy;
  pencil_sf_planes<NB>(L, mw, mxy);
  int woff[4];
  {
    const int a = lane >> 4, b1 = lane & 3, b2 = (lane >> 2) & 3;
    const int xp = XP[(wi + a) * 7 + (b1 - a + 3)];
#pragma unroll
    for (int r = 0; r < 4; ++r) woff[r] = valid ? YP[(wj + r) * 7 + (b2 - r + 3)] * nxp + xp : 0;
  }

  PatchFix<P> fx;      // the Dirichlet data of the patch
  if constexpr (SYSTEM) fx.fill(S, D);

  // ---- this thread's runs u = tid + j NTHR of the band rows, (y pair, x pair) for the whole walk:
  // pos = RA + RB prefix0(layer) + RC count0(layer) + P0(layer, d); ut = the transposed pair (where the row's lower half is read)
  long long RA[G::RUNS]; int RB[G::RUNS], RC[G::RUNS], ut[G::RUNS], ucode[G::RUNS];      // ucode: xr | dx + 3 << 5 | yr << 8 | dy + 3 << 13 | first << 16
#pragma unroll
  for (int j = 0; j < G::RUNS; ++j) {
    const int u = tid + j * NTHR;
    RA[j] = 0; RB[j] = 0; RC[j] = 0; ut[j] = 0; ucode[j] = 0;
    if (u >= nruns) continue;
    const int yp = u / nxp, xp = u - yp * nxp;
    int yr, dy, xr, dx;
    patch_pair<P>(YI[yp], yr, dy); patch_pair<P>(XI[xp], xr, dx);
    patch_run_address<P>(S, ex0, ey0, xr, dx, yr, dy, RA[j], RB[j], RC[j]);
    ut[j] = YP[(yr + dy) * 7 + (3 - dy)] * nxp + XP[(xr + dx) * 7 + (3 - dx)];
    bool first = false;
    if (pa.first_touch) first = patch_first_touch<G>(A, D, xr, dx, yr, dy);
    ucode[j] = xr | ((dx + 3) << 5) | (yr << 8) | ((dy + 3) << 13) | (first ? 1 << 16 : 0);
  }
  int own_lo, own_hi;
  patch_owned_layers(S, A, D, own_lo, own_hi);
  // the F rows: thread t < NODES is patch node (yr, xr) = (t / NX, t % NX); its F row without the walk-axis part
  long long frowxy = 0;
  if (SYSTEM && tid < G::NODES) {
    const int yr = tid / NX, xr = tid - yr * NX;
    if (xr <= mxv + P - 1 && yr <= myv + P - 1) frowxy = (long long)S.ax[0].nrow * AX.rowmap[AX.off[ex0] + xr] + (long long)S.ax[0].nrow * S.ax[1].nrow * AY.rowmap[AY.off[ey0] + yr];
  }

  // the runs of layer li: their seven old values are requested a step ahead (fetch) and consumed when the layer is complete (leave)
  auto layer_on = [&](int li) { const int lay = T.lay0 + li; return li >= 0 && li < nl && T.cnt[li] > 0 && lay >= own_lo && lay < own_hi; };
  struct Run { long long base; double o[7]; bool full; };
  bool ron = false;
  auto fetch = [&](int li, Run (&rr)[G::RUNS]) {
    ron = layer_on(li);
    if (!ron) return;
    const long long pre = T.pre[li]; const int cnt = T.cnt[li];
    const int *p0 = T.P + li * 8;
    const bool full = patch_layer_full<BW>(p0);      // (an interior layer: a run is 56 contiguous bytes)
#pragma unroll
    for (int j = 0; j < G::RUNS; ++j) {
      Run &r = rr[j];
      r.full = full;
      if (tid + j * NTHR >= nruns) continue;
      r.base = RA[j] + (long long)RB[j] * pre + (long long)RC[j] * cnt;
      patch_run_load<BW>(out.val, r.base, p0, full, (ucode[j] >> 16) & 1, r.o);
    }
  };
  long long st[5] = {0, 0, 0, 0, 0}, st_t = 0;      // -DIGX_DEBUG: cycles of [products | ticks | wait for the old values | leave's window and stores, the next loads | closing barrier + F]
  auto stamp = [&](int k) { if (stamped) { const long long t = __builtin_readcyclecounter(); st[k] += t - st_t; st_t = t; } };
  auto leave = [&](int li, const Run (&rr)[G::RUNS]) {
    if (stamped) { __builtin_amdgcn_s_waitcnt(0x0F70); stamp(2); }      // (stamped launch only: the wait for the old values, at the top of leave)
    const int c0 = li & 3;
    const bool bcl = SYSTEM && ron && fx.reaches(T.lay0 + li);
#pragma unroll
    for (int j = 0; j < G::RUNS; ++j) {
      const int u = tid + j * NTHR;
      if (u >= nruns) continue;
      // upper half: blocks (li, li + d) at the run's pair; lower half: blocks (li - d, li) at the transposed pair.  The blocks of column
      // layer li are read for the last time here: zeroed for the layer that takes their slots next.
      double v[7];
#pragma unroll
      for (int d = 0; d <= 3; ++d) v[3 + d] = win[(((li + d) & 3) * 4 + d) * BLK + u];
      win[(c0 * 4) * BLK + u] = 0.0;
#pragma unroll
      for (int d = 1; d <= 3; ++d) { double *w = win + (c0 * 4 + d) * BLK + ut[j]; v[3 - d] = *w; *w = 0.0; }
      if (!ron) continue;
      const Run &r = rr[j];
      const int lay = T.lay0 + li;
      if constexpr (SYSTEM) {      // IGAElementFixSystem (src/petigaelem.c:1377-1387) on the combined run; its row's lifting to the F stage
        if (bcl) {
          const int xr = ucode[j] & 31, dx = ((ucode[j] >> 5) & 7) - 3, yr = (ucode[j] >> 8) & 31, dy = ((ucode[j] >> 13) & 7) - 3;
          double c = 0, rv = 0;
          const bool rf = fx.fixed(xr, yr, lay, rv);
#pragma unroll
          for (int d = 0; d < 7; ++d) {
            double cv = 0; const bool cf = fx.fixed(xr + dx, yr + dy, lay + d - P, cv);
            if (cf) c += v[d] * cv;
            if (rf || cf) v[d] = (d == P && dx == 0 && dy == 0 && rf) ? (double)fx.held(li, xr, yr, ne) : 0.0;
          }
          corr[(li & 1) * BLK + u] = c;
        }
      }
      patch_run_add_store<BW>(out.val, r.base, T.P + li * 8, r.full, r.o, v);
    }
  };
  // F of layer li: thread t < NODES = patch node (yr, xr): the pencils' sums (Fp) and its runs' liftings (corr), each in a fixed order
  auto leave_f = [&](int li) {
    if constexpr (SYSTEM) {
      if (tid >= G::NODES || !layer_on(li)) return;
      const int yr = tid / NX, xr = tid - yr * NX;
      if (xr > mxv + P - 1 || yr > myv + P - 1) return;
      const int lay = T.lay0 + li;
      const double *Fl = Fp + (li & 1) * (W * 16);
      double f = 0;
      for (int j = max(0, yr - P); j <= min(yr, myv - 1); ++j)
        for (int i = max(0, xr - P); i <= min(xr, mxv - 1); ++i) f += Fl[(j * MX + i) * 16 + 4 * (yr - j) + (xr - i)];
      if (fx.reaches(lay)) {
        double fv = 0;
        if (fx.fixed(xr, yr, lay, fv)) f = fv * (double)fx.held(li, xr, yr, ne);
        else {
          const double *cl = corr + (li & 1) * BLK;
          double c = 0;
          for (int dy = 0; dy < 7; ++dy) {
            const int yp = YP[yr * 7 + dy];
            if (yp < 0) continue;
            for (int dx = 0; dx < 7; ++dx) { const int xp = XP[xr * 7 + dx]; if (xp >= 0) c += cl[yp * nxp + xp]; }
          }
          f -= c;
        }
      }
      // one memory-side add per row and launch (patches of a colour share no node): order-free, and nothing waits for it
      (void)__hip_atomic_fetch_add(out.vec + (long long)T.rho[li] + frowxy, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  const int fslot = lane >> 4;
  double Facc = 0;
  auto f_stage = [&](int li) {      // the leaving layer's F sums of this pencil (slot 0 of the F lanes), then the slots slide
    if constexpr (SYSTEM) {
      if (fslot == 0) Fp[(li & 1) * (W * 16) + wave * 16 + lane] = Facc;
      const double up = __shfl_down(Facc, 16);
      Facc = (fslot >= NB - 1) ? 0.0 : up;
    }
  };

  // ---- the pencil's open band rows: acc[i][d][r] = this lane's four entries of block (ei + i, ei + i + d), d = 0 .. 3 - i, summed over
  // the elements walked so far.  Row ei is complete once element ei is in: its four blocks go to the window in the ticks, the rows slide.
  double acc[4][4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][d][r] = 0.0;
  auto products = [&](int ei) {      // element ei's ten tiles (ta, tb), ta <= tb, into rows ei + ta: 2 x 4 v_fma_f64 each
    if (!valid) return;
    const double *g = T.zt + ei * 32;
#pragma unroll
    for (int ta = 0; ta < 4; ++ta)
#pragma unroll
      for (int tb = ta; tb < 4; ++tb) {
        const double g0 = g[(ta * 4 + tb) * 2 + 0], g1 = g[(ta * 4 + tb) * 2 + 1];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[ta][tb - ta][r] = __builtin_fma(g0, mxy[r], __builtin_fma(g1, mw[r], acc[ta][tb - ta][r]));
      }
  };
  // the ticks of row li: in tick k wavefront w adds its block d = tick_block(k, w) of the row to window block (li, li + d).  One
  // wavefront per block between two barriers, an entry of it one lane's: a plain read, add and write.  Then the rows slide.
  auto tick_add = [&](double *blk, const double (&a)[4]) {
    double w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) w[r] = blk[woff[r]];
#pragma unroll
    for (int r = 0; r < 4; ++r) blk[woff[r]] = w[r] + a[r];
  };
  auto window_block = [&](int r, int d) { return win + (((r + d) & 3) * 4 + d) * BLK; };      // block (r, r + d)
  auto ticks = [&](int li) {
#pragma unroll
    for (int k = 0; k < G::TICKS; ++k) {
      const int d = G::tick_block(k, wave);      // (wave-uniform: branches, not a register index)
      if (valid && d >= 0) {
        double *blk = window_block(li, d);
        if (d == 0) tick_add(blk, acc[0][0]);
        else if (d == 1) tick_add(blk, acc[0][1]);
        else if (d == 2) tick_add(blk, acc[0][2]);
        else tick_add(blk, acc[0][3]);
      }
      if (SYSTEM && k == 0) {      // F_a += f J prod_d sum_q w N: the walk-axis factor was staged with the Gram sums
        Facc += sxy * T.wq[li * 4 + fslot];
        f_stage(li);
      }
      __syncthreads();      // (the last one: every wavefront's row li is in the window, layer li is complete, its F sums are staged)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {      // row li + 1 + i takes the place of row li + i; its last block and the new last row start at zero
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int d = 0; d < 3 - i; ++d) acc[i][d][r] = acc[i + 1][d][r];
        acc[i][3 - i][r] = 0.0;
      }
      acc[3][0][r] = 0.0;
    }
  };

  Run run[G::RUNS];
  long long tk0 = 0, tw0 = 0;
  if (out.clk) { tk0 = __builtin_readcyclecounter(); tw0 = wall_clock64(); }
  const long long st_wall1 = stamped ? wall_clock64() : 0;
  fetch(0, run);
  for (int ei = 0; ei < ne; ++ei) {
    if (stamped) st_t = __builtin_readcyclecounter();
    products(ei);
    stamp(0);
    ticks(ei);
    stamp(1);
    leave(ei, run);
    fetch(ei + 1, run);
    stamp(3);
    __syncthreads();      // the slots of column layer ei are zero again; the liftings of layer ei are staged
    leave_f(ei);
    stamp(4);
  }
  const long long st_wall2 = stamped ? wall_clock64() : 0;
  if (seg == pa.nseg - 1 && !pa.open_hi) {
    // the last segment owns the layers beyond its last element too (other segments drop theirs: the next one's halo forms them again).
    // Their rows ne .. ne + 2 are complete in registers: acc[i][d], d <= 2 - i (there is no column layer ne + 3).  One round of the
    // ticks adds all three to the window -- blocks (ne + i, ne + i + d), whose slots the layers up to ne - 1 have left -- in tick k
    // wavefront w the blocks d of every row; then the layers leave as they always did.
#pragma unroll
    for (int k = 0; k < G::TICKS; ++k) {
      const int d = G::tick_block(k, wave);
      if (valid && d >= 0) {
        if (d == 0) { tick_add(window_block(ne, 0), acc[0][0]); tick_add(window_block(ne + 1, 0), acc[1][0]); tick_add(window_block(ne + 2, 0), acc[2][0]); }
        else if (d == 1) { tick_add(window_block(ne, 1), acc[0][1]); tick_add(window_block(ne + 1, 1), acc[1][1]); }
        else if (d == 2) tick_add(window_block(ne, 2), acc[0][2]);
      }
      __syncthreads();
    }
    for (int li = ne; li < nl; ++li) {
      f_stage(li);
      leave(li, run);
      fetch(li + 1, run);
      __syncthreads();
      leave_f(li);
      __syncthreads();
    }
  }
  if (stamped && lane == 0) {
    // -DIGX_DEBUG: per wavefront, the five parts of a step summed over the walk, its elements, and on the 100 MHz clock the set-up before
    // the walk and the trailing layers behind it; behind them the item's record {entry, exit, HW_ID, XCC_ID} (one per item: a workgroup
    // that walks several leaves several, and the report's gaps are those between two items on a CU)
    long long *d = pa.debug_buf + ((size_t)item * W + wave) * 8;
    const long long st_wall3 = wall_clock64();
    d[0] = st[0]; d[1] = st[1]; d[2] = st[2]; d[3] = st[3]; d[4] = st[4]; d[5] = ne; d[6] = st_wall1 - st_wall0; d[7] = st_wall3 - st_wall2;
    if (wave == 0) { long long *w = pa.debug_buf + (size_t)nitems * W * 8 + (size_t)item * 4; w[0] = st_wall0; w[1] = st_wall3; w[2] = __builtin_amdgcn_s_getreg((16 - 1) << 11 | 4); w[3] = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 20); }
  }
  if (out.clk && (item == 0 || item == nitems - 1) && tid == 0) {
    // IGX_CLOCK_PROBE: s_memtime against the 100 MHz s_memrealtime over the walk, first and last item of every launch (as gram_pencil_body's
    // first and last workgroup), by whoever walks them
    atomicAdd(reinterpret_cast<unsigned long long *>(out.clk), (unsigned long long)(__builtin_readcyclecounter() - tk0));
    atomicAdd(reinterpret_cast<unsigned long long *>(out.clk) + 1, (unsigned long long)(wall_clock64() - tw0));
    atomicAdd(reinterpret_cast<unsigned long long *>(out.clk) + 2, (unsigned long long)ne);
  }
  if constexpr (!TICKETS) break;
  // the workgroup learns its next ticket through LDS; the barrier also closes the item: nothing of it is read after this
  if (tid == 0) cntp[4] = next_ticket;
  __syncthreads();
  ticket = __builtin_amdgcn_readfirstlane(cntp[4]);
  } while (ticket < nitems);
}


}  // namespace igx
