// vec_sumfact.hpp -- the vector-only drivers (IGAComputeVector / Function / IFunction, src/petigaksp.c:33, src/petigasnes.c:23,
// src/petigats.c:23) by sum factorisation in both directions.
//
// The reference's point callback fills F[a] for every basis function a of the element at every quadrature point
// (IGAPointAddVec, src/petigapoint.c:427-450): nen * nqp evaluations per element, and the feature kernel's vector-only mode keeps
// that shape (Phi for all (a,q) pairs, vec() per pair).  But every IGAFormVector / Function / IFunction is LINEAR in the test
// function, F_a^i = sum_q JW sum_f Phi_f(a,q) r^i_f(q) with r_f = vec(p, e_f), and on a tensor-product basis both halves factor over
// the axes:
//   forward   u, grad u, hess u (and x, dx/du, d2x/du2 of a mapped geometry) at the points from the nodal values: three short
//             contractions, one axis at a time (src/petigaval.F90:182-232 summed the long way);
//   point     the geometry chain K3-K6 (Rationalize, GeometryMap, InverseMap, src/petigarat/mapgeo/mapinv.f90.in), the form's
//             vec() on the unit test features -- nqp evaluations instead of nen * nqp;
//   backward  F_a = w_a sum_q sum_k C_k(q) D_k N_a(q) over the 10 parametric derivatives D_k up to order 2: the transpose of the
//             forward contractions.
// One wavefront per element (4 x 4 x 4 lanes = nodes = points), two elements per wavefront when no axis has more than three basis
// functions or points (p <= 2: 2 x 27 of the 64 lanes), no matrix cores (there is no
// dense contraction left: the work per element drops from ~nen * nqp * features to ~(nen + nqp) * (p+1) * components), coloured
// scatter (conflict-free, fixed order: bitwise repeatable).  dim 3, nen <= 4 and nqp <= 4 per axis (the matrix-free ACTION and DIAGONAL
// instantiations: up to 8, one workgroup per element above 4 -- vs_layout below); first-order test features on
// any geometry, second-order test features (Cahn-Hilliard's Laplacian) likewise (round 4); no boundary loads, no boundary
// passes -- everything else stays on the feature kernel.
#pragma once
#include "feature_mfma.hpp"
#include "element_sweep.hpp"

namespace igx {

// derivative k of the 10 (value, d0, d1, d2, d00, d01, d02, d11, d12, d22): orders on the axes, and the two-axis stage m it comes from
__device__ __forceinline__ constexpr int vs_v0(int k) { return (k == 1 || k == 5 || k == 6) ? 1 : (k == 4 ? 2 : 0); }
__device__ __forceinline__ constexpr int vs_v1(int k) { return (k == 2 || k == 5 || k == 8) ? 1 : (k == 7 ? 2 : 0); }
__device__ __forceinline__ constexpr int vs_v2(int k) { return (k == 3 || k == 6 || k == 8) ? 1 : (k == 9 ? 2 : 0); }
// m -> (v0, v1): 0 (0,0) 1 (1,0) 2 (0,1) 3 (2,0) 4 (1,1) 5 (0,2)
__device__ __forceinline__ constexpr int vs_m(int v0, int v1) { return v0 == 0 ? (v1 == 0 ? 0 : (v1 == 1 ? 2 : 5)) : (v0 == 1 ? (v1 == 0 ? 1 : 4) : 3); }
__device__ __forceinline__ constexpr int vs_mv0(int m) { return (m == 1 || m == 4) ? 1 : (m == 3 ? 2 : 0); }
__device__ __forceinline__ constexpr int vs_mv1(int m) { return (m == 2 || m == 4) ? 1 : (m == 5 ? 2 : 0); }

// the barrier between the stages of a contraction: of the wavefront where a wavefront holds the element (NS <= 4), of the workgroup
// (WG) where a workgroup does (NS = 6, 8).  Every thread of the workgroup reaches every one of them.
template <bool WG> __device__ __forceinline__ void vs_sync() {
  if constexpr (WG) __syncthreads();
  else { __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
}
#define VS_SYNC() vs_sync<WG>()
// the loops over the contracted index: unrolled in full up to NS = 4, by half above (8 steps in full keep up to 80 LDS loads of the way
// back in flight: Elasticity's and NS-VMS' actions spilled 16-146 registers at NS = 6, 8 under the 256 two wavefronts per SIMD leave)
#define VS_UNROLL(NS) ((NS) <= 4 ? (NS) : (NS) / 2)      // (UNR in the helpers)

// forward: D[k] = sum_a coef_a D_k N_a(q) at this lane's point; ORD = highest derivative order wanted.  buf: 10 x BS doubles of this
// wave (WG: of this workgroup; BS >= NS^3 is the stride between the buffers); tab[d]: [q][a][3] (value, first, second derivative),
// zero padded to NS x NS.
// NS: lanes per axis -- 4: one element per wavefront; 3 (nen, nqp <= 3 on every axis): two elements per wavefront, lanes 0..26 and
// 27..53.  L: this lane's (i0, i1, i2) and the first lane of its element.
struct VsLane { int i0, i1, i2, base; };
template <int ORD, int NS, int BS = 64, bool WG = false>
__device__ __forceinline__ void vs_forward(double coef, double *buf, const double *tab0, const double *tab1, const double *tab2, int lane, const VsLane &L, double (&D)[10]) {
  const int i0 = L.i0, i1 = L.i1, i2 = L.i2;
  constexpr int S1 = NS, S2 = NS * NS, UNR = VS_UNROLL(NS);
  double *in = buf + L.base, *T1 = buf + BS + L.base, *T2 = buf + 4 * BS + L.base;
  lane -= L.base;
  VS_SYNC();
  in[lane] = coef;
  VS_SYNC();
  {   // axis 0: lane (q0, a1, a2)
    double t[3] = {0, 0, 0};
#pragma unroll UNR
    for (int a0 = 0; a0 < NS; ++a0) {
      const double c = in[a0 + S1 * i1 + S2 * i2];
#pragma unroll
      for (int v = 0; v <= ORD; ++v) t[v] += c * tab0[(i0 * NS + a0) * 3 + v];
    }
#pragma unroll
    for (int v = 0; v <= ORD; ++v) T1[v * BS + lane] = t[v];
  }
  VS_SYNC();
  {   // axis 1: lane (q0, q1, a2)
    double t[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll UNR
    for (int a1 = 0; a1 < NS; ++a1) {
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        if (vs_mv0(m) + vs_mv1(m) > ORD) continue;
        t[m] += T1[vs_mv0(m) * BS + i0 + S1 * a1 + S2 * i2] * tab1[(i1 * NS + a1) * 3 + vs_mv1(m)];
      }
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) if (vs_mv0(m) + vs_mv1(m) <= ORD) T2[m * BS + lane] = t[m];
  }
  VS_SYNC();
#pragma unroll
  for (int k = 0; k < 10; ++k) D[k] = 0.0;
#pragma unroll UNR
  for (int a2 = 0; a2 < NS; ++a2) {
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      if (vs_v0(k) + vs_v1(k) + vs_v2(k) > ORD) continue;
      D[k] += T2[vs_m(vs_v0(k), vs_v1(k)) * BS + i0 + S1 * i1 + S2 * a2] * tab2[(i2 * NS + a2) * 3 + vs_v2(k)];
    }
  }
}

// backward: F_a = sum_q sum_k C_k(q) D_k N_a(q) at this lane's node; buf: max(popc(KMASK), 9) x BS doubles of this wave (workgroup)
// KMASK: the derivatives k whose coefficient can be non-zero (the others are neither stored nor summed); Cb holds them back to back
__device__ __forceinline__ constexpr int vs_popc(unsigned m) { int n = 0; for (; m; m &= m - 1) ++n; return n; }
__device__ __forceinline__ constexpr int vs_kc(unsigned kmask, int k) { return vs_popc(kmask & ((1u << k) - 1u)); }
template <int ORD, unsigned KMASK, int NS, int BS = 64, bool WG = false>
__device__ __forceinline__ double vs_backward(const double (&C)[10], double *buf, const double *tab0, const double *tab1, const double *tab2, int lane, const VsLane &L) {
  const int i0 = L.i0, i1 = L.i1, i2 = L.i2;
  constexpr int T1s = NS, T2s = NS * NS, UNR = VS_UNROLL(NS);
  // (round 6: S2 takes the place of Cb -- every lane holds its sums in registers until all have read Cb -- and S1 sits behind S2:
  //  max(popc, 9) buffers instead of popc + 6; with the forward stage's 10 that is 30 KB per workgroup, five workgroups per CU instead of four)
  constexpr int NS2 = ORD >= 2 ? 6 : 3;
  double *Cb = buf + L.base, *S2 = buf + L.base, *S1 = buf + NS2 * BS + L.base;
  lane -= L.base;
  VS_SYNC();
#pragma unroll
  for (int k = 0; k < 10; ++k) if (((KMASK >> k) & 1u) && vs_v0(k) + vs_v1(k) + vs_v2(k) <= ORD) Cb[vs_kc(KMASK, k) * BS + lane] = C[k];
  VS_SYNC();
  {   // axis 2: lane (q0, q1, a2)
    double t[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll UNR
    for (int q2 = 0; q2 < NS; ++q2) {
#pragma unroll
      for (int k = 0; k < 10; ++k) {
        if (!((KMASK >> k) & 1u) || vs_v0(k) + vs_v1(k) + vs_v2(k) > ORD) continue;
        t[vs_m(vs_v0(k), vs_v1(k))] += Cb[vs_kc(KMASK, k) * BS + i0 + T1s * i1 + T2s * q2] * tab2[(q2 * NS + i2) * 3 + vs_v2(k)];
      }
    }
    VS_SYNC();      // (every lane has read Cb)
#pragma unroll
    for (int m = 0; m < 6; ++m) if (vs_mv0(m) + vs_mv1(m) <= ORD) S2[m * BS + lane] = t[m];
  }
  VS_SYNC();
  {   // axis 1: lane (q0, a1, a2)
    double t[3] = {0, 0, 0};
#pragma unroll UNR
    for (int q1 = 0; q1 < NS; ++q1) {
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        if (vs_mv0(m) + vs_mv1(m) > ORD) continue;
        t[vs_mv0(m)] += S2[m * BS + i0 + T1s * q1 + T2s * i2] * tab1[(q1 * NS + i1) * 3 + vs_mv1(m)];
      }
    }
#pragma unroll
    for (int v = 0; v <= ORD; ++v) S1[v * BS + lane] = t[v];
  }
  VS_SYNC();
  double f = 0;
#pragma unroll UNR
  for (int q0 = 0; q0 < NS; ++q0) {
#pragma unroll
    for (int v = 0; v <= ORD; ++v) f += S1[v * BS + q0 + T1s * i1 + T2s * i2] * tab0[(q0 * NS + i0) * 3 + v];
  }
  return f;
}

// identity geometry: test feature tf (0 value, 1..3 gradient, 4 + 3a + b second derivative) -> derivative k of the 10
__device__ __forceinline__ constexpr unsigned vs_kmask_ident(unsigned vmask) {
  unsigned m = 0;
  for (int tf = 0; tf < 13; ++tf) {
    if (!((vmask >> tf) & 1u)) continue;
    if (tf < 4) m |= 1u << tf;
    else { const int a = (tf - 4) / 3, b = (tf - 4) % 3, lo = a < b ? a : b, hi = a < b ? b : a; m |= 1u << (4 + (lo == 0 ? hi : (lo == 1 ? 2 + hi : 5))); }
  }
  return m | 0x7u;      // (at least three slots: S1 is laid over them)
}

// GEO: a mapped geometry and / or NURBS weights; without them the geometry chain is the identity at compile time (no E1 / E2
// products, no quotient rule) and the kernel needs half the registers
// the pipelined walk of round 6 (see the kernel): scalar forms without a geometry, where its registers fit four wavefronts per SIMD
template <class Form, bool GEO> __host__ __device__ constexpr bool vs_pipe() { return !GEO && Form::DOF == 1; }
template <int N> struct vs_int { static constexpr int value = N; };      // (a derivative order handed to a generic lambda)
// ACTION: the matrix-free product Y = A X of the matrix the Matrix / Jacobian / IJacobian driver would assemble (OP_*_ACTION): every
// mat(p, Na, Nb, T) is linear in Nb, so sum_b K_ab X_b = sum_q JW sum_f Phi_f(a, q) sum_j mat(p, e_f, Xf^j)[.][j] with Xf^j = (x^j, grad x^j,
// hess x^j) the direction's point features -- one more forward pass per field, DOF calls of mat() per test feature, and the way back,
// the colours and the scatter of the vector drivers.  No matrix is allocated and no index is read.
// DIAGONAL: the diagonal D_a^i = K_aa^ii of the same matrix (OP_*_DIAGONAL), first-order shape features only.  mat() is linear in Na
// as well, and R_a's features are w_a M(q) (N_a, d0 N_a, d1 N_a, d2 N_a) with M the point's 4 x 4 geometry chain (1 / W, E1 / W and the
// rational correction; the identity without a geometry), so mat() on the columns of M gives B_kl = JW (M^T C M)_kl directly: at most
// 4 x 4 calls per point.  D_k N_a D_l N_a factorises per axis into N^2, N N' or N'^2 and the per-axis product commutes: B folds
// into ten slots indexed like the ten derivatives, and the way back is vs_backward<2> on the product rows {N^2, N N', N'^2} in
// place of {N, N', N''}, once per field, times w_a^2.  No direction, no pass for one.
// NS = 6, 8 (ACTION and DIAGONAL; nen or nqp above 4 on some axis): one workgroup per element -- 256 threads (216 of them lanes of the
// 6 x 6 x 6 nodes = points, the 40 others idle: they load zeros, store nothing and reach every barrier) or 512 threads (8 x 8 x 8), thread t
// = (i0, i1, i2) with i0 fastest; the same helpers with the workgroup's barrier and a stride of 256 / 512 doubles between the buffers; no
// pairing of elements and no early loads (PIPE, EF).  Not covered: the vector-only drivers above four (they stay on the feature
// kernel), nen or nqp above 8, the diagonal of second-order shape features (refused by name).
template <int NS> struct vs_layout {
  static constexpr bool WG = NS > 4;                                     // one workgroup, not one wavefront, per element
  static constexpr int BS = NS <= 4 ? 64 : (NS <= 6 ? 256 : 512);        // doubles between two buffers = threads of an element's unit
  static constexpr int THREADS = WG ? BS : 256, NWAVE = WG ? 1 : 4;      // threads per workgroup, units per workgroup
};
// BLOCK (with DIAGONAL): the dof x dof point-block diagonal B_a^ij = K_aa^ij of the same matrix (OP_*_BLOCK_DIAGONAL), column j into
// out.bcol[j].  D_k N_a D_l N_a is symmetric in (k, l) for every field pair, so every (i, j) folds into the same ten slots; the tile
// mat() returns holds them all.  Block row by block row: for a test field i the point stage keeps row i of every tile (DOF x 10
// coefficients, as many as DIAGONAL holds -- all DOF^2 x 10 would be 320 registers for NS-VMS) and DOF ways back follow; the compiler
// drops the rows of a call that are not kept.  An entry beside a fixed dof is 0, a fixed (i, i) the unit diagonal (IGAElementFixJacobian).
// BATCH (with ACTION): the action on a block of nc <= IGX_ACTION_MAXCOLS vectors in one launch, Y_c = A X_c (the launcher below;
// DESIGN.md 3.22).  What an element needs that does not depend on the direction -- rows, offsets, row map, control points, the geometry
// chain, the state's point values, the Dirichlet flags, JW and G -- is done once; the direction's forward pass, the DOF calls of mat() per
// test feature, the rational correction, the way back and the scatter run per column in ONE loop body that is not unrolled, so a column's
// arithmetic does not depend on its place in the block.  nc is uniform over the launch: every thread of a workgroup reaches the barriers
// of the helpers the same number of times.  The columns share buf; each helper opens with VS_SYNC() ahead of its first store, which is
// the barrier between one column's way back and the next column's way forward.  No early load of the old result (PIPE, EF: it belongs
// to one column): Y_c is read where it is added to, which the colour makes as safe as the early read.  Scalar forms fetch the next
// column's nodal value while the current one computes (one register); the others load it at the top of the loop (no register to spare).
// The block's table is a kernel argument of its own, behind the five every instantiation takes: the pack COLS is empty (the kernel's
// signature is the one it always had, also for the run-time compiled instantiations that name it) or, with BATCH, ActionCols.
__device__ __forceinline__ const ActionCols *vs_cols() { return nullptr; }
__device__ __forceinline__ const ActionCols *vs_cols(const ActionCols &c) { return &c; }
template <class Form, bool GEO, int NS = 4, bool ACTION = false, bool DIAGONAL = false, bool BLOCK = false, bool BATCH = false, class... COLS>
__global__ void __launch_bounds__(vs_layout<NS>::THREADS, ((!vs_layout<NS>::WG && vs_pipe<Form, GEO>()) ? 4 : 2))      // (two waves per SIMD: the geometry variants of NS-VMS and Cahn-Hilliard need 290-350 VGPRs uncapped, one wave per SIMD)
vec_sumfact(SpaceDev S, ParamsDev prm, OutDev out, ColorRange cr, long long nelem, COLS... colsarg) {
  static_assert(sizeof...(COLS) == (BATCH ? 1 : 0), "BATCH takes the table of columns as its one further argument, the others none");
  const ActionCols *cols = vs_cols(colsarg...);
  static_assert(!BATCH || ACTION, "a block of columns is a variant of ACTION");
  constexpr int EPW = NS == 3 ? 2 : 1, NL = NS * NS * NS;               // elements per wavefront, lanes per element
  constexpr int DOF = Form::DOF;
  constexpr bool WG = vs_layout<NS>::WG;
  constexpr int BS = vs_layout<NS>::BS, NWAVE = vs_layout<NS>::NWAVE;
  static_assert(NS == 3 || NS == 4 || ((NS == 6 || NS == 8) && (ACTION || DIAGONAL)), "lanes per axis: 3 or 4 per wavefront, 6 or 8 per workgroup (ACTION, DIAGONAL)");
  static_assert(!(ACTION && DIAGONAL), "one of the two");
  static_assert(!BLOCK || DIAGONAL, "the point-block diagonal is a variant of DIAGONAL");
  static_assert(!DIAGONAL || shape_order_of<Form>::v < 2, "the matrix diagonal does not cover forms with second-order shape features: its ten product slots hold N and grad N only");
  constexpr bool MATOP = ACTION || DIAGONAL;                             // mat() at the points, not vec()
  constexpr unsigned VMASK = MATOP ? mat_test_mask_of<Form>::v : vec_test_mask_of<Form>::v;      // test features vec() (MATOP: mat()) reads (bit f)
  constexpr bool SECOND_T = shape_order_of<Form>::v >= 2;                // second-order test features
  constexpr unsigned SNEED = MATOP ? mat_need_of<Form>::v : Form::NEED;  // what the point callback reads of the state (MATOP: mat() alone)
  constexpr bool NEEDHU = (SNEED & NEED_HU) != 0, NEEDGU = (SNEED & (NEED_GU | NEED_HU)) != 0;
  constexpr int UORD = NEEDHU ? 2 : (NEEDGU ? 1 : 0);                    // derivative order of the state
  constexpr int XORD = ACTION ? (SECOND_T ? 2 : 1) : 0;                  // ... of the direction: the trial features mat() reads (Na's layout)
  constexpr int GORD = UORD > XORD ? UORD : XORD;                        // ... of the geometry map (UORD without ACTION)
  constexpr int NFS = SECOND_T ? 13 : 4;
  // derivatives of the test functions that can carry a coefficient: without a geometry feature tf maps to one of them; with one, the
  // inverse Jacobian mixes the three first derivatives and the rational correction reaches the value
  constexpr unsigned KMASK = DIAGONAL ? 0x3FFu : (GEO ? (SECOND_T ? 0x3FFu : 0xFu) : vs_kmask_ident(VMASK & ((1u << NFS) - 1u)));      // (DIAGONAL: the ten product slots)
  constexpr bool BACK2 = SECOND_T || DIAGONAL;                           // the way back runs to order 2
  constexpr int NBACK = vs_popc(KMASK) > (BACK2 ? 9 : 5) ? vs_popc(KMASK) : (BACK2 ? 9 : 5), NFWD = (GORD == 2 || GEO) ? 10 : 7, NBUF = NBACK > NFWD ? NBACK : NFWD;
  constexpr int TB = NS * NS * 3;                                        // doubles of one axis' rows [q][a][3], zero padded to NS x NS
  constexpr int NTAB = DIAGONAL ? 2 : 1;                                 // DIAGONAL: the product rows [q][a][3] = (N^2, N N', N'^2) behind the rows
  __shared__ double sm_all[NWAVE][NBUF * BS + NTAB * EPW * 3 * TB];      // Cahn-Hilliard without a geometry: 25 KB per workgroup, two elements per wavefront (a sixth workgroup per CU measured no gain over five: 12.8 ms either way)
  const int lane = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63), wave = WG ? 0 : (int)(threadIdx.x >> 6);
  const int esub = (EPW == 2 && lane >= NL) ? 1 : 0;                    // which of the wavefront's elements this lane works on
  // Round 6 (PIPE: scalar forms without a geometry): every global load of the unit -- the 1-D rows, the node's state and old F, the
  // point's weights -- leaves at its start, behind closed forms for the element's offset and the row map.  A wavefront's life was a
  // chain of dependent round trips (offset -> row map -> state; the rows; the point's weights; F read-add-write at the end, each
  // behind a wavefront fence the compiler does not move loads across) around 2-3 us of arithmetic: 9.3 us with four wavefronts per
  // SIMD to hide it, 7.7 us now.  (The colour makes the early read of F safe: no other element of the launch touches these rows.)
  // Off for the geometry variants: they are at their 256 registers already.
  constexpr bool PIPE = !WG && vs_pipe<Form, GEO>();
  constexpr bool EF = !WG && GEO && Form::DOF == 1;      // ... scalar forms on a geometry: old F and the product of the point's weights (three registers) leave early too
  constexpr int TPL = EPW * 3;                                           // table entries per lane: lane j < TB holds entry j of each (element, axis) block
  const long long nunits = (nelem + EPW - 1) / EPW, ustride = (long long)gridDim.x * NWAVE;
  long long unit = (long long)blockIdx.x * NWAVE + wave;
  if (unit >= nunits) return;      // (WG: the whole workgroup leaves, ahead of every barrier)
  double *buf = sm_all[wave], *tab0 = buf + NBUF * BS + esub * 3 * TB, *tab1 = tab0 + TB, *tab2 = tab1 + TB;
  auto element_at = [&](long long ww, long long wfirst, int (&e3)[3]) {
    long long b = ww < nelem ? ww : wfirst;
    const int t0 = (int)(b % cr.count[0]); b /= cr.count[0];
    const int t1 = (int)(b % cr.count[1]); b /= cr.count[1];
    e3[0] = cr.start[0] + t0 * cr.step[0]; e3[1] = cr.start[1] + t1 * cr.step[1]; e3[2] = cr.start[2] + (int)b * cr.step[2];
  };
  const int ll = lane < EPW * NL ? lane - esub * NL : 0;                 // (the lanes beyond the last element idle on lane 0's indices)
  const int i0 = NS == 4 ? (ll & 3) : ll % NS, i1 = NS == 4 ? ((ll >> 2) & 3) : (ll / NS) % NS, i2 = NS == 4 ? (ll >> 4) : ll / (NS * NS);
  const VsLane VL = {i0, i1, i2, esub * NL};
  const int il[3] = {i0, i1, i2};
  const int op = out.op;
  const bool geo = GEO && S.nsd > 0, rat = GEO && S.rational != 0;
  const bool sysvec = out.vec_mode == 1, sysbody = out.vec_mode == 2;      // parts of a System assembly (igx.hpp: OutDev::vec_mode)
  const bool readU = out.U != nullptr && !sysvec && !sysbody, useU = readU || sysvec, useV = out.V != nullptr && !sysvec && !sysbody;
  int nb[3], nq[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) { nb[d] = S.ax[d].nen; nq[d] = S.ax[d].nqp; }
  const bool lanenode = i0 < nb[0] && i1 < nb[1] && i2 < nb[2], lanepoint = i0 < nq[0] && i1 < nq[1] && i2 < nq[2];
  // what an element needs from memory, in two steps: its offsets (A), then everything addressed through them (B)
  struct Pre { int el[3], off[3]; bool live; size_t row; double tab[TPL], U[DOF], V[DOF], Fo[DOF], fx[DOF], wgt, X[3], pt[3], wq[3], Jd[3], Xd[ACTION ? DOF : 1]; };
  auto stageA = [&](long long un, Pre &P) {
    const long long w0n = un * EPW, wn = w0n + esub;
    P.live = lane < EPW * NL && wn < nelem;                             // (an odd count leaves the second half of the last wavefront idle)
    element_at(wn, w0n, P.el);
#pragma unroll
    for (int d = 0; d < 3; ++d) P.off[d] = S.ax[d].off_lin ? S.ax[d].off0 + P.el[d] : S.ax[d].off[P.el[d]];      // (closed form: the loads behind it leave with the first round trip)
  };
  auto stageB = [&](long long un, Pre &P) {
    const long long w0n = un * EPW;
    {      // 1-D rows of the element(s), [q][a][3], zero padded to 4 x 4 (the axis is a compile-time index: an index known only at run time sent nq / nb / the element to scratch and LDS)
      const int j = lane < TB ? lane : 0, q = j / (3 * NS), a = (j / 3) % NS, v = j % 3;
#pragma unroll
      for (int es = 0; es < EPW; ++es) {
        int e3[3]; element_at(w0n + es, w0n, e3);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          P.tab[es * 3 + d] = 0.0;
          if (lane < TB && q < nq[d] && a < nb[d]) P.tab[es * 3 + d] = S.ax[d].tab[((size_t)e3[d] * nq[d] * nb[d] + q * nb[d] + a) * NDER + v];
        }
      }
    }
    P.row = 0; P.wgt = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) P.X[c] = 0.0;
#pragma unroll
    for (int f = 0; f < DOF; ++f) { P.U[f] = 0; P.V[f] = 0; P.Fo[f] = 0; P.fx[f] = 0; if constexpr (ACTION) P.Xd[f] = 0; }
    if (P.live && lanenode) {      // this lane's node: control point, state, old F (rowmap in closed form: AxisDev::rwrap)
      const int n0 = P.off[0] + i0, n1 = P.off[1] + i1, n2 = P.off[2] + i2;
      const size_t g = (size_t)n0 + (size_t)S.ax[0].gwidth * ((size_t)n1 + (size_t)S.ax[1].gwidth * (size_t)n2);
      const int r0 = n0 < S.ax[0].rwrap ? n0 : n0 - S.ax[0].rwrap, r1 = n1 < S.ax[1].rwrap ? n1 : n1 - S.ax[1].rwrap, r2 = n2 < S.ax[2].rwrap ? n2 : n2 - S.ax[2].rwrap;
      P.row = (size_t)r0 + (size_t)S.ax[0].nrow * ((size_t)r1 + (size_t)S.ax[1].nrow * (size_t)r2);
      P.wgt = rat ? S.W[g] : 1.0;
      if (geo) for (int c = 0; c < 3; ++c) P.X[c] = S.X[g * 3 + c];
#pragma unroll
      for (int f = 0; f < DOF; ++f) {
        if (readU) P.U[f] = out.U[P.row * DOF + f];
        if (useV) P.V[f] = out.V[P.row * DOF + f];
        if (S.fixtable) P.fx[f] = S.fixtable[P.row * DOF + f];
        if constexpr ((PIPE || EF) && !BATCH) P.Fo[f] = out.vec[P.row * DOF + f];
        if constexpr (ACTION && !BATCH) P.Xd[f] = out.X[P.row * DOF + f];
      }
    }
    if constexpr (PIPE) {      // (the geometry variants read these where they use them: no register to spare)
      const bool on = P.live && lanepoint;
      P.pt[0] = on ? S.ax[0].pt[P.el[0] * nq[0] + i0] : 0.0; P.pt[1] = on ? S.ax[1].pt[P.el[1] * nq[1] + i1] : 0.0; P.pt[2] = on ? S.ax[2].pt[P.el[2] * nq[2] + i2] : 0.0;
      P.wq[0] = on ? S.ax[0].w[P.el[0] * nq[0] + i0] : 0.0; P.wq[1] = on ? S.ax[1].w[P.el[1] * nq[1] + i1] : 0.0; P.wq[2] = on ? S.ax[2].w[P.el[2] * nq[2] + i2] : 0.0;
#pragma unroll
      for (int d = 0; d < 3; ++d) P.Jd[d] = S.ax[d].J[P.el[d]];
    } else if constexpr (EF) {
      const bool on = P.live && lanepoint;
      P.wq[0] = on ? (S.ax[0].w[P.el[0] * nq[0] + i0] * S.ax[0].J[P.el[0]]) * (S.ax[1].w[P.el[1] * nq[1] + i1] * S.ax[1].J[P.el[1]]) * (S.ax[2].w[P.el[2] * nq[2] + i2] * S.ax[2].J[P.el[2]]) : 0.0;
    }
  };
  Pre cur, nxt;
  if (PIPE) { stageA(unit, cur); stageB(unit, cur); }
  // One unit per wavefront.  Measured in round 6 (config 4's Residual, 256^3, 18.9 ms before): a wavefront walking a SEQUENCE of units with
  // the next one's loads in flight held 228 registers -- two wavefronts per SIMD -- and took 24.6 ms; TWO units as straight-line code
  // spilled 71 registers under the cap of 128 and took 32.6 ms; this, every load of the unit issued at its start, takes 15.6 ms.
  constexpr int UNITS = 1;
#pragma unroll
  for (int it = 0; it < UNITS; ++it) {
  const long long unext = unit + ustride; const bool more = PIPE && it + 1 < UNITS && unext < nunits;
  if (!PIPE) { stageA(unit, cur); stageB(unit, cur); }
  const bool live = cur.live;
  int el[3] = {cur.el[0], cur.el[1], cur.el[2]};
  VS_SYNC();      // (the previous element's readers of the rows are done)
#pragma unroll
  for (int k = 0; k < TPL; ++k) if (lane < TB) buf[NBUF * BS + k * TB + lane] = cur.tab[k];
  if constexpr (DIAGONAL) {      // the product rows, once per element and axis: entry (q, a, v) from (N, N') of (q, a)
    VS_SYNC();
    const int j0 = lane < TB ? lane - lane % 3 : 0, v = lane % 3;
#pragma unroll
    for (int k = 0; k < TPL; ++k) {
      const double n0 = buf[NBUF * BS + k * TB + j0], n1 = buf[NBUF * BS + k * TB + j0 + 1];
      if (lane < TB) buf[NBUF * BS + (TPL + k) * TB + lane] = (v == 0 ? n0 : n1) * (v == 2 ? n1 : n0);
    }
  }
  if (PIPE && more) stageA(unext, nxt);
  // Dirichlet flags (IGAElementBuildFix / FixValues, src/petigaelem.c:1214-1358)
  const bool isnode = live && lanenode;
  const bool ispoint = live && lanepoint;
  const size_t row = cur.row; double Xw[3] = {cur.X[0] * cur.wgt, cur.X[1] * cur.wgt, cur.X[2] * cur.wgt}; const double wgt = cur.wgt; double Uv[DOF], Vv[DOF], ufix[DOF], Fold[DOF]; bool fixed[DOF];
#pragma unroll
  for (int f = 0; f < DOF; ++f) { Uv[f] = cur.U[f]; Vv[f] = cur.V[f]; Fold[f] = cur.Fo[f]; ufix[f] = 0; fixed[f] = false; }
  double Xv[ACTION ? DOF : 1];      // ACTION: the node's values of the direction
  if constexpr (ACTION) {
#pragma unroll
    for (int f = 0; f < DOF; ++f) Xv[f] = cur.Xd[f];
  }
  if (isnode) {
    if (op != OP_VECTOR || sysvec || sysbody) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {      // (unrolled: el[d] / il[d] stay registers -- indexed at run time the arrays went to scratch and LDS)
        const AxisDev &A = S.ax[d];
        if (A.periodic) continue;
#pragma unroll
        for (int sd = 0; sd < 2; ++sd) {
          if (el[d] + A.estart != (sd ? A.esizes - 1 : 0) || il[d] != (sd ? nb[d] - 1 : 0)) continue;
          const BCDev &bv = S.bcv[d][sd];
          for (int k = 0; k < bv.count; ++k) {
            const int f = bv.field[k];
#pragma unroll
            for (int ff = 0; ff < DOF; ++ff) if (ff == f) { fixed[ff] = true; ufix[ff] = S.fixtable ? cur.fx[ff] : bv.value[k]; }
          }
        }
      }
    }
  }
  VS_SYNC();
  // ---- forward: geometry (homogeneous coordinates), state
  double x[3], E1[9], E2[27], iw = 1.0, o1[3] = {0, 0, 0}, o2[9], detX = 1.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) { E1[i] = (i % 4 == 0) ? 1.0 : 0.0; o2[i] = 0.0; }
#pragma unroll
  for (int i = 0; i < 27; ++i) E2[i] = 0.0;
  if constexpr (PIPE) { x[0] = cur.pt[0]; x[1] = cur.pt[1]; x[2] = cur.pt[2]; }
  else { x[0] = ispoint ? S.ax[0].pt[el[0] * nq[0] + i0] : 0.0; x[1] = ispoint ? S.ax[1].pt[el[1] * nq[1] + i1] : 0.0; x[2] = ispoint ? S.ax[2].pt[el[2] * nq[2] + i2] : 0.0; }
  // index of the second derivative (a, b) among the 10
  auto k2 = [](int a, int b) { const int lo = a < b ? a : b, hi = a < b ? b : a; return 4 + (lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)); };
  if constexpr (GEO) if (geo || rat) {
    double Dw[10], Dx[3][10];
    if (GORD == 2) vs_forward<2, NS, BS, WG>(wgt, buf, tab0, tab1, tab2, lane, VL, Dw); else vs_forward<1, NS, BS, WG>(wgt, buf, tab0, tab1, tab2, lane, VL, Dw);
    const double W0 = ispoint ? Dw[0] : 1.0;
    iw = 1.0 / W0;
#pragma unroll
    for (int a = 0; a < 3; ++a) o1[a] = Dw[1 + a] * iw;
    if (GORD == 2)
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) o2[a * 3 + b] = Dw[k2(a, b)] * iw;
    if (geo) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { if (GORD == 2) vs_forward<2, NS, BS, WG>(Xw[c], buf, tab0, tab1, tab2, lane, VL, Dx[c]); else vs_forward<1, NS, BS, WG>(Xw[c], buf, tab0, tab1, tab2, lane, VL, Dx[c]); }
      double X1[9], X2[27];
#pragma unroll
      for (int c = 0; c < 3; ++c) {      // quotient rule on A = sum w X N, W = sum w N (src/petigarat.f90.in + petigamapgeo.f90.in)
        x[c] = Dx[c][0] * iw;
#pragma unroll
        for (int a = 0; a < 3; ++a) X1[c * 3 + a] = (Dx[c][1 + a] - x[c] * Dw[1 + a]) * iw;
        if (GORD == 2)
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) X2[c * 9 + a * 3 + b] = (Dx[c][k2(a, b)] - x[c] * Dw[k2(a, b)] - X1[c * 3 + a] * Dw[1 + b] - X1[c * 3 + b] * Dw[1 + a]) * iw;
      }
      if (!ispoint) { for (int i = 0; i < 9; ++i) X1[i] = (i % 4 == 0) ? 1.0 : 0.0; }
      detX = det3(X1, 3);
      inv3(X1, 3, detX, E1);
      if (ispoint && !(detX > 0.0)) atomicExch(out.errflag, IGX_ERR_USER);   // src/petigaelem.c:989-993
      if (GORD == 2) {   // InverseMap order 2 (src/petigamapinv.f90.in:32-45): E2[c][i][j] = -X2[k][a][b] E1[a][i] E1[b][j] E1[c][k]
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double U9[9], T9[9];
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int j = 0; j < 3; ++j) { double sm = 0; for (int b = 0; b < 3; ++b) sm += X2[k * 9 + a * 3 + b] * E1[b * 3 + j]; U9[a * 3 + j] = sm; }
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) { double sm = 0; for (int a = 0; a < 3; ++a) sm += U9[a * 3 + j] * E1[a * 3 + i]; T9[i * 3 + j] = sm; }
#pragma unroll
          for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 9; ++i) E2[c * 9 + i] -= T9[i] * E1[c * 3 + k];
        }
      }
    }
  }
  // a nodal coefficient -> (value, gradient, Hessian up to order ORD) at this lane's point: the forward contraction, the quotient rule of
  // rational weights and the inverse map (E1, E2).  The state's fields and, with ACTION, the direction's go through it.
  auto field_at_point = [&](auto ordc, double coef, double &val, double *g3, double *h9) {
    constexpr int ORD = decltype(ordc)::value;
    double D[10];
    vs_forward<ORD, NS, BS, WG>(coef * wgt, buf, tab0, tab1, tab2, lane, VL, D);
    val = D[0] * iw;
    if constexpr (!GEO) {
      if (ORD >= 1) for (int a = 0; a < 3; ++a) g3[a] = D[1 + a];
      if (ORD == 2) for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) h9[a * 3 + b] = D[k2(a, b)];
    } else
    if (ORD >= 1) {
      double u1[3], u2[9];
#pragma unroll
      for (int a = 0; a < 3; ++a) u1[a] = D[1 + a] * iw - val * o1[a];      // u = A / W, du = (dA - u dW) / W (o1 = dW / W; 0 without weights)
#pragma unroll
      for (int i = 0; i < 3; ++i) g3[i] = u1[0] * E1[0 * 3 + i] + u1[1] * E1[1 * 3 + i] + u1[2] * E1[2 * 3 + i];
      if (ORD == 2) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) {
            double t = D[k2(a, b)] * iw;
            if (rat) t -= val * o2[a * 3 + b] + u1[a] * o1[b] + u1[b] * o1[a];
            u2[a * 3 + b] = t;
          }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) {     // ShapeFunctions summed over a (src/petigamapshf.f90.in:30-58)
            double sm = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
              for (int b = 0; b < 3; ++b) sm += u2[a * 3 + b] * E1[a * 3 + i] * E1[b * 3 + j];
              sm += u1[a] * E2[a * 9 + i * 3 + j];
            }
            h9[i * 3 + j] = sm;
          }
      }
    }
  };
  double u[DOF], ut[DOF], gu[DOF * 3], hu[DOF * 9];
#pragma unroll
  for (int f = 0; f < DOF; ++f) {
    u[f] = 0; ut[f] = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) gu[f * 3 + i] = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) hu[f * 9 + i] = 0;
    if ((SNEED & (NEED_U | NEED_GU | NEED_HU)) && useU) field_at_point(vs_int<UORD>(), fixed[f] ? ufix[f] : Uv[f], u[f], gu + f * 3, hu + f * 9);
    if ((SNEED & NEED_UT) && useV) {
      double D[10];
      vs_forward<0, NS, BS, WG>((fixed[f] ? 0.0 : Vv[f]) * wgt, buf, tab0, tab1, tab2, lane, VL, D);
      ut[f] = D[0] * iw;
    }
  }
  // BATCH: the columns of the block go through the body below one after the other; everything above is done once for them all, and so
  // are JW and G, at the first column (they stand where they always stood, behind the direction's forward pass).  Else the body runs
  // once: no loop.  Xn: the next column's nodal value, on its way while this column computes.
  constexpr bool XPRE = BATCH && DOF == 1;
  double JW = 0.0, G[9], Xn = 0.0;
  int col = 0;
  if constexpr (XPRE) { if (isnode) Xn = cols->X[0][row]; }
#pragma unroll 1
  do {
  if constexpr (BATCH) {
    if constexpr (XPRE) { Xv[0] = Xn; if (isnode && col + 1 < cols->nc) Xn = cols->X[col + 1][row]; }
    else {
      const double *Xc = cols->X[col];
#pragma unroll
      for (int f = 0; f < DOF; ++f) Xv[f] = isnode ? Xc[row * DOF + f] : 0.0;
    }
  }
  // ACTION: the direction's point features, field by field, behind the state's (a fixed column takes no contribution: gathered as 0)
  double xv[ACTION ? DOF : 1], gx[ACTION ? DOF * 3 : 1], hx[ACTION && XORD == 2 ? DOF * 9 : 1];
  if constexpr (ACTION) {
#pragma unroll
    for (int f = 0; f < DOF; ++f) {
      double h9[9];
      field_at_point(vs_int<XORD>(), fixed[f] ? 0.0 : Xv[f], xv[f], gx + f * 3, h9);
      if constexpr (XORD == 2) for (int i = 0; i < 9; ++i) hx[f * 9 + i] = h9[i];
    }
  }
  // the next element's loads go out here: its offsets have arrived, and the point stage and the way back lie ahead
  if (PIPE && more) stageB(unext, nxt);
  // ---- point: JW and the form's vec() on the unit test features
  if (!BATCH || col == 0) {
  if (ispoint) {
    JW = detX;
    if constexpr (EF && !PIPE) JW *= cur.wq[0];
    else {
#pragma unroll
    for (int d = 0; d < 3; ++d) JW *= PIPE ? cur.wq[d] * cur.Jd[d] : S.ax[d].w[el[d] * nq[d] + il[d]] * S.ax[d].J[el[d]];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int i = 0; i < 3; ++i) G[a * 3 + i] = E1[a * 3 + i] / (PIPE ? cur.Jd[a] : S.ax[a].J[el[a]]);      // IGAPointFormInvGradGeomMap, src/petigapoint.c:269-294
  }
  PtView p; p.x = x; p.u = u; p.ut = ut; p.gu = gu; p.hu = hu; p.G = G; p.prm = prm.v; p.shift = out.shift; p.t = out.t;
  p.normal = nullptr; p.atboundary = 0; p.boundary_id = -1;
  double Cq[DOF][10];
#pragma unroll
  for (int f = 0; f < DOF; ++f)
#pragma unroll
    for (int k = 0; k < 10; ++k) Cq[f][k] = 0.0;
  if constexpr (!DIAGONAL)      // (its point stage follows the loop)
#pragma unroll
  for (int tf = 0; tf < NFS; ++tf) {
    if (!((VMASK >> tf) & 1u)) continue;
    double e[NFS], R[DOF];
#pragma unroll
    for (int g = 0; g < NFS; ++g) e[g] = (g == tf) ? 1.0 : 0.0;
    if constexpr (!ACTION) Form::vec(p, e, R);
    else {      // column j of the blocks against the direction's field j: DOF calls per test feature, not nen x nen
#pragma unroll
      for (int i = 0; i < DOF; ++i) R[i] = 0.0;
#pragma unroll
      for (int j = 0; j < DOF; ++j) {
        double Nb[NFS], T[DOF * DOF];
        Nb[0] = xv[j];
#pragma unroll
        for (int a = 0; a < 3; ++a) Nb[1 + a] = gx[j * 3 + a];
        if constexpr (SECOND_T)
#pragma unroll
          for (int a = 0; a < 9; ++a) Nb[4 + a] = hx[j * 9 + a];
#pragma unroll
        for (int i = 0; i < DOF * DOF; ++i) T[i] = 0.0;
        Form::mat(p, e, Nb, T);
#pragma unroll
        for (int i = 0; i < DOF; ++i) R[i] += T[i * DOF + j];
      }
    }
#pragma unroll
    for (int f = 0; f < DOF; ++f) {
      const double r = ispoint ? R[f] * JW : 0.0;      // (a padded lane evaluates vec() on zeros: its value may not even be finite)
      if (tf == 0) Cq[f][0] += r;
      else if (tf < 4) {      // physical gradient component tf-1 -> parametric: d_i R_a = sum_b E1[b][i] d_b R_a
        if constexpr (!GEO) Cq[f][tf] += r;
        else {
#pragma unroll
          for (int b = 0; b < 3; ++b) Cq[f][1 + b] += E1[b * 3 + (tf - 1)] * r;
        }
      } else {                // second-order test feature (i, j)
        const int i = (tf - 4) / 3, j = (tf - 4) % 3;
        if constexpr (!GEO) Cq[f][k2(i, j)] += r;      // (physical = parametric)
        else {
          // d_i d_j R_a = sum_ab E1[a][i] E1[b][j] d_a d_b R_a + sum_a E2[a][i][j] d_a R_a (ShapeFunctions order 2, src/petigamapshf.f90.in:30-58,
          // transposed: the slot of (a, b) takes both orders)
#pragma unroll
          for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) Cq[f][k2(a, b)] += E1[a * 3 + i] * E1[b * 3 + j] * r;
            Cq[f][1 + a] += E2[a * 9 + i * 3 + j] * r;
          }
        }
      }
    }
  }
  if constexpr (DIAGONAL) {
    // column k of M (the header's comment): the physical features (value, gradient) of a function whose parametric ones are e_k
    auto mcol = [&](int k, double (&c)[4]) {
      if constexpr (!GEO) { for (int f = 0; f < 4; ++f) c[f] = (f == k) ? 1.0 : 0.0; }
      else {
        c[0] = k == 0 ? iw : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) c[1 + i] = k == 0 ? -(E1[0 * 3 + i] * o1[0] + E1[1 * 3 + i] * o1[1] + E1[2 * 3 + i] * o1[2]) * iw : E1[(k - 1) * 3 + i] * iw;
      }
    };
    // columns of M with an entry mat() reads on the test side: without a geometry e_k itself; with one the gradient rows fill every column
    constexpr unsigned TK = GEO ? ((VMASK & 0xEu) ? 0xFu : 0x1u) : (VMASK & 0xFu);
    if constexpr (!BLOCK) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!((TK >> k) & 1u)) continue;
      double Na[4]; mcol(k, Na);
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        double Nb[4], T[DOF * DOF]; mcol(l, Nb);
#pragma unroll
        for (int i = 0; i < DOF * DOF; ++i) T[i] = 0.0;
        Form::mat(p, Na, Nb, T);
        const int slot = (k == 0 || l == 0) ? k + l : k2(k - 1, l - 1);      // B_kl and B_lk share a slot
#pragma unroll
        for (int f = 0; f < DOF; ++f) Cq[f][slot] += ispoint ? T[f * DOF + f] * JW : 0.0;
      }
    }
    } else {
      // ---- BLOCK, block row by block row: the point stage for the test field f keeps row f of every tile (Cq[g]: the trial field g),
      // then one way back per trial field
#pragma unroll
      for (int f = 0; f < DOF; ++f) {
#pragma unroll
        for (int g = 0; g < DOF; ++g)
#pragma unroll
          for (int k = 0; k < 10; ++k) Cq[g][k] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((TK >> k) & 1u)) continue;
          double Na[4]; mcol(k, Na);
#pragma unroll
          for (int l = 0; l < 4; ++l) {
            double Nb[4], T[DOF * DOF]; mcol(l, Nb);
#pragma unroll
            for (int i = 0; i < DOF * DOF; ++i) T[i] = 0.0;
            Form::mat(p, Na, Nb, T);
            const int slot = (k == 0 || l == 0) ? k + l : k2(k - 1, l - 1);      // B^{fg}_kl and B^{fg}_lk share a slot, for every field pair
#pragma unroll
            for (int g = 0; g < DOF; ++g) Cq[g][slot] += ispoint ? T[f * DOF + g] * JW : 0.0;
          }
        }
#pragma unroll
        for (int g = 0; g < DOF; ++g) {
          double F = vs_backward<2, KMASK, NS, BS, WG>(Cq[g], buf, tab0 + EPW * 3 * TB, tab1 + EPW * 3 * TB, tab2 + EPW * 3 * TB, lane, VL) * wgt;      // (the product rows; w_a^2 with the line below)
          F *= wgt;
          if (isnode) {
            if (fixed[f] || fixed[g]) F = (f == g) ? 1.0 : 0.0;      // IGAElementFixJacobian: the unit diagonal, a zero row and column beside it
            if (F != 0.0) { double *col = out.bcol[g]; if constexpr (PIPE || EF) col[row * DOF + f] = Fold[f] + F; else col[row * DOF + f] += F; }      // (PIPE, EF: DOF = 1, bcol[0] is vec)
          }
        }
      }
    }
  }
  // rational test functions: R_a = w_a N_a / W, d_b R_a = (w_a / W) (d_b N_a - N_a W_b / W), d_b d_c R_a = (w_a / W) (d_b d_c N_a -
  // d_b N_a o_c - d_c N_a o_b - N_a (W_bc / W - 2 o_b o_c)) (src/petigarat.f90.in, order 2): the coefficients of the polynomial basis
  if (!DIAGONAL && rat) {      // (DIAGONAL: M holds the correction)
#pragma unroll
    for (int f = 0; f < DOF; ++f) {
      double c0 = Cq[f][0] - (Cq[f][1] * o1[0] + Cq[f][2] * o1[1] + Cq[f][3] * o1[2]);
      if constexpr (GEO && SECOND_T) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = a; b < 3; ++b) {
            const double sk = Cq[f][k2(a, b)];      // (the slot holds both orders of (a, b))
            c0 -= sk * (o2[a * 3 + b] - 2.0 * o1[a] * o1[b]);
            if (a == b) Cq[f][1 + a] -= 2.0 * sk * o1[a];
            else { Cq[f][1 + a] -= sk * o1[b]; Cq[f][1 + b] -= sk * o1[a]; }
            Cq[f][k2(a, b)] = sk * iw;
          }
      }
      Cq[f][0] = c0 * iw; Cq[f][1] *= iw; Cq[f][2] *= iw; Cq[f][3] *= iw;
    }
  }
  // ---- backward, IGAElementFixFunction (src/petigaelem.c:1449-1461), IGAElementAssembleVec
  if constexpr (!BLOCK)      // (its ways back follow its point stages above)
#pragma unroll
  for (int f = 0; f < DOF; ++f) {
    double F;
    if constexpr (DIAGONAL) F = vs_backward<2, KMASK, NS, BS, WG>(Cq[f], buf, tab0 + EPW * 3 * TB, tab1 + EPW * 3 * TB, tab2 + EPW * 3 * TB, lane, VL) * wgt;      // (the product rows; w_a^2 with the line below)
    else F = SECOND_T ? vs_backward<2, KMASK, NS, BS, WG>(Cq[f], buf, tab0, tab1, tab2, lane, VL) : vs_backward<1, KMASK, NS, BS, WG>(Cq[f], buf, tab0, tab1, tab2, lane, VL);
    F *= wgt;
    if (isnode) {
      if constexpr (ACTION) { if (fixed[f]) F = Xv[f]; }        // IGAElementFixJacobian: a unit diagonal per element, zero row and column beside it
      else if constexpr (DIAGONAL) { if (fixed[f]) F = 1.0; }   // ... and that unit diagonal itself: the element count once assembled
      else if (fixed[f] && sysvec) F = ufix[f];                  // IGAElementFixSystem: F_e[k] = v
      else if (fixed[f] && sysbody) F = 0.0;                     // (the band-row kernel that follows adds v per element itself)
      else if (fixed[f] && (op == OP_FUNCTION || op == OP_IFUNCTION)) F = Uv[f] - ufix[f];
      if constexpr (BATCH) { if (F != 0.0) cols->Y[col][row * DOF + f] += F; }
      else
      if (F != 0.0) { if constexpr (PIPE || EF) out.vec[row * DOF + f] = Fold[f] + F; else out.vec[row * DOF + f] += F; }
    }
  }
  } while (BATCH && ++col < cols->nc);      // the block's next column
  if (!more) break;
  if (PIPE) cur = nxt;
  unit = unext;
  }      // the wavefront's next element
}
#undef VS_SYNC
#undef VS_UNROLL

#ifndef IGX_RTC
// dim 3, at most 4 basis functions and 4 points per axis; vector-only drivers; no boundary loads (Function / IFunction subtract
// their lumped flux per element), no boundary-form passes
template <class Form>
static bool vec_sumfact_covers(const Space &s, const OutDev &out) {
  if constexpr (nscalar_of<Form>::v > 0 || has_boundary_of<Form>::v) return false;
  else {
    if (s.env.vec_sumfact == 0) return false;
    if (out.op != OP_VECTOR && out.op != OP_FUNCTION && out.op != OP_IFUNCTION && !out.vec_mode) return false;
    if (s.dim != 3 || s.dof != Form::DOF || (s.nsd != 0 && s.nsd != 3)) return false;
    for (int d = 0; d < 3; ++d) {
      if (s.basis[d].nen > 4 || s.basis[d].nqp > 4) return false;
      for (int sd = 0; sd < 2; ++sd) { if (s.visit[d][sd]) return false; if (out.op != OP_VECTOR && !out.vec_mode && s.load[d][sd].count) return false; }      // (vec_mode: the band-row launchers add the loads themselves)
    }
    return true;
  }
}

// One launch per colour of the mode's instantiation (igx.hpp: VsMode, vs_traits) in the layout of the space (vs_launch_of).
// ACTION_BATCH: on the columns of cols (at most IGX_ACTION_MAXCOLS: the caller cuts the block).  The matrix-free modes: the caller has asked matfree_refusal.
template <class Form, VsMode M = VsMode::VECTOR>
static int try_vec_sumfact(const Space &s, const SpaceDev &S, const ParamsDev &prm, const OutDev &out, hipStream_t stream, std::string &kname, int &launches, bool &done, const ActionCols *cols = nullptr) {
  done = false;
  constexpr VsTraits T = vs_traits(M);
  if constexpr (nscalar_of<Form>::v > 0 || has_boundary_of<Form>::v) return 0;
  else {
  if constexpr (M == VsMode::VECTOR) { if (!vec_sumfact_covers<Form>(s, out)) return 0; }
  if constexpr (T.batch) { if (!cols || cols->nc < 1 || cols->nc > IGX_ACTION_MAXCOLS) return IGX_ERR_PLIB; }
  const VsLaunch L = vs_launch_of(s, M);
  const bool g1 = s.nsd > 0 || s.rational;
  launches = 0;
  color_sweeps(s, SweepSpec(), [&](const ColorRange &cr) -> int {
    const long long nelem = (long long)cr.count[0] * cr.count[1] * cr.count[2];
    // the instantiation of a layout (lanes per axis) on a mapped / rational geometry or on none
    auto launch = [&](auto nsc) {
      constexpr int NS = decltype(nsc)::value;
      const dim3 grid(L.grid(nelem)), threads(vs_layout<NS>::THREADS);
      if constexpr (T.batch) {
        if (g1) hipLaunchKernelGGL((vec_sumfact<Form, true, NS, T.action, T.diagonal, T.block, true, ActionCols>), grid, threads, 0, stream, S, prm, out, cr, nelem, *cols);
        else hipLaunchKernelGGL((vec_sumfact<Form, false, NS, T.action, T.diagonal, T.block, true, ActionCols>), grid, threads, 0, stream, S, prm, out, cr, nelem, *cols);
      } else {
        if (g1) hipLaunchKernelGGL((vec_sumfact<Form, true, NS, T.action, T.diagonal, T.block>), grid, threads, 0, stream, S, prm, out, cr, nelem);
        else hipLaunchKernelGGL((vec_sumfact<Form, false, NS, T.action, T.diagonal, T.block>), grid, threads, 0, stream, S, prm, out, cr, nelem);
      }
    };
    switch (L.ns) {
    case 3: launch(vs_int<3>()); break;
    case 4: launch(vs_int<4>()); break;
    case 6: if constexpr (T.wide) launch(vs_int<6>()); break;      // more than four basis functions or points on an axis: one workgroup per element
    default: if constexpr (T.wide) launch(vs_int<8>()); break;
    }
    launches++;
    return 0;
  });
  if (hipGetLastError() != hipSuccess) return IGX_ERR_LIB;
  kname = std::string("vec_sumfact(") + T.words + L.tail;
  done = true;
  return 0;
  }
}

#endif   // !IGX_RTC

}  // namespace igx
