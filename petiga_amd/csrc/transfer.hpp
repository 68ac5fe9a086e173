// transfer.hpp -- prolongation and restriction between nested spline spaces (IGXTransfer; the tables: transfer_axis_setup in host.cpp).
// Included by the main unit only, after the probe.  With vectors in the natural numbering [n2][n1][n0][dof] the prolongation is
// P = T2 (x) T1 (x) T0 (x) I_dof, every T an nf x nc band of at most p + 1 consecutive columns per row; the restriction is P^T.
// transfer_prolong_fused: one workgroup owns a box of TR_FX x TR_FY x TR_FZ fine rows (clipped at the upper ends and to an axis' extent).
//   A block of F consecutive fine rows reads at most F + p consecutive coarse columns on an axis (the first column grows by at most one per
//   row and a row holds at most p + 1), so the box's coarse footprint is a box: its corner and extents per axis come from the host
//   (boxlo, boxlen: the host takes them from the tables, not from the bound).  The workgroup stages the footprint with all dof fields in
//   LDS, contracts axis 0 (A -> B), axis 1 (B -> A) and axis 2 (A -> global) and stores the fine box as lines of F0 * dof doubles along
//   axis 0.  Index arithmetic inside a box is by multiply-high with a reciprocal made once per workgroup (TrDiv: exact below 2^16).
// transfer_axis_pass: one axis at a time, for the prolongation where the footprint does not fit the LDS budget or the caller asks for the
//   passes, and for the restriction always: dst[o][r][i] = sum_e val[e] * src[o][idx[e]][i] over the CSR row r, i running over
//   inner = dof * (the extents below the axis), o over the extents above it.  A coarse row of the restriction GATHERS from its fine rows
//   (the transposed table as CSR by coarse row, fine rows ascending): rows of any length, no atomics.
// Every output entry is one chain per axis -- the first product, then fma in the table's order -- whichever kernel, box or lane computes
// it, so results are bit-repeatable and an entry does not depend on where it lies in a box.  A row with the single entry 1.0 multiplies by
// one and adds nothing: identity axes are exact copies (the sign of a zero included).
#pragma once
#include <hip/hip_runtime.h>
#include "igx.hpp"

namespace igx {

constexpr int TR_T = 256;                               // lanes per workgroup (both kernels)
constexpr int TR_FX = 16, TR_FY = 8, TR_FZ = 8;         // fine rows of a box along axis 0, 1, 2
constexpr int TR_LDS_MAX = 64 * 1024;                   // LDS of a workgroup at the most: the fused kernel runs where A + B fit
constexpr int TR_G = 16384;                             // workgroups of an axis pass at the most (grid-stride loop over blocks of TR_T outputs)

struct TrAxisDev {
  const int *ufirst, *count;     // [nf] first column before folding, band length
  const double *T;               // [nf][width]
  const int *boxlo, *boxlen;     // [nbox] first column (before folding) and number of columns of a box's footprint
  int nf, nc, width, F, nbox;
  int wrap;                      // nc on a periodic axis (a column c >= wrap is column c - wrap), else INT_MAX
};
struct TrFusedDev { TrAxisDev ax[3]; int dof, sizeA; };      // sizeA: doubles of the LDS buffer A (B follows it)
struct TrPassDev {
  const int *ptr, *idx; const double *val;      // CSR by output row
  unsigned nout, nin, inner, outer;             // nout * inner < 2^32, outer * ceil(nout * inner / TR_T) < 2^32 (checked by the host)
};

// n / d for n, d < 2^16 by one multiply-high: m = ceil(2^32 / d), exact while n * (m d - 2^32) < 2^32
struct TrDiv {
  unsigned m, d;
  __device__ explicit TrDiv(unsigned dd) : m(0xffffffffu / dd + 1u), d(dd) {}
  __device__ unsigned operator()(unsigned n) const { return d == 1u ? n : __umulhi(n, m); }
};
__device__ inline double tr_row(const double *__restrict__ t, const double *__restrict__ s, int cnt, unsigned stride) {
  double acc = t[0] * s[0];
  for (int k = 1; k < cnt; ++k) acc = fma(t[k], s[(size_t)k * stride], acc);
  return acc;
}

__global__ void __launch_bounds__(TR_T) transfer_prolong_fused(TrFusedDev P, const double *__restrict__ xc, double *xf, int add) {
  extern __shared__ double tr_lds[];
  double *A = tr_lds, *B = tr_lds + P.sizeA;
  const TrAxisDev &X = P.ax[0], &Y = P.ax[1], &Z = P.ax[2];
  unsigned bid = blockIdx.x;
  const unsigned b0 = bid % (unsigned)X.nbox; bid /= (unsigned)X.nbox;
  const unsigned b1 = bid % (unsigned)Y.nbox, b2 = bid / (unsigned)Y.nbox;
  const unsigned dof = (unsigned)P.dof, tid = threadIdx.x;
  const int lo0 = X.boxlo[b0], lo1 = Y.boxlo[b1], lo2 = Z.boxlo[b2];
  const unsigned C0 = (unsigned)X.boxlen[b0], C1 = (unsigned)Y.boxlen[b1], C2 = (unsigned)Z.boxlen[b2];
  const int g0 = (int)b0 * X.F, g1 = (int)b1 * Y.F, g2 = (int)b2 * Z.F;
  const unsigned f0 = (unsigned)min(X.F, X.nf - g0), f1 = (unsigned)min(Y.F, Y.nf - g1), f2 = (unsigned)min(Z.F, Z.nf - g2);
  const unsigned C0d = C0 * dof, f0d = f0 * dof;
  const TrDiv by_C0d(C0d), by_C1(C1), by_dof(dof), by_f0d(f0d), by_f1(f1);
  // the coarse footprint, all fields: A[z][y][x][c]
  for (unsigned i = tid, n = C2 * C1 * C0d; i < n; i += TR_T) {
    const unsigned yz = by_C0d(i), x = i - yz * C0d, z = by_C1(yz), y = yz - z * C1, cx = by_dof(x), c = x - cx * dof;
    int j0 = lo0 + (int)cx, j1 = lo1 + (int)y, j2 = lo2 + (int)z;
    while (j0 >= X.wrap) j0 -= X.wrap;
    while (j1 >= Y.wrap) j1 -= Y.wrap;
    while (j2 >= Z.wrap) j2 -= Z.wrap;
    A[i] = xc[(((size_t)j2 * Y.nc + j1) * X.nc + j0) * dof + c];
  }
  __syncthreads();
  // axis 0: B[z][y][ix][c]
  for (unsigned i = tid, n = C2 * C1 * f0d; i < n; i += TR_T) {
    const unsigned yz = by_f0d(i), xo = i - yz * f0d, ix = by_dof(xo), c = xo - ix * dof;
    const int gi = g0 + (int)ix, rel = X.ufirst[gi] - lo0;
    B[i] = tr_row(X.T + (size_t)gi * X.width, A + yz * C0d + (unsigned)rel * dof + c, X.count[gi], dof);
  }
  __syncthreads();
  // axis 1: A[z][iy][ix][c]
  for (unsigned i = tid, n = C2 * f1 * f0d; i < n; i += TR_T) {
    const unsigned t = by_f0d(i), xo = i - t * f0d, z = by_f1(t), iy = t - z * f1;
    const int gi = g1 + (int)iy, rel = Y.ufirst[gi] - lo1;
    A[i] = tr_row(Y.T + (size_t)gi * Y.width, B + (z * C1 + (unsigned)rel) * f0d + xo, Y.count[gi], f0d);
  }
  __syncthreads();
  // axis 2, to the fine vector: lines of f0 * dof doubles along axis 0
  for (unsigned i = tid, n = f2 * f1 * f0d; i < n; i += TR_T) {
    const unsigned t = by_f0d(i), xo = i - t * f0d, iz = by_f1(t), iy = t - iz * f1;
    const int gi = g2 + (int)iz, rel = Z.ufirst[gi] - lo2;
    const double acc = tr_row(Z.T + (size_t)gi * Z.width, A + ((unsigned)rel * f1 + iy) * f0d + xo, Z.count[gi], f1 * f0d);
    double *dst = xf + (((size_t)gi * Y.nf + (g1 + iy)) * X.nf + g0) * dof + xo;
    *dst = add ? *dst + acc : acc;
  }
}

__global__ void __launch_bounds__(TR_T) transfer_axis_pass(TrPassDev P, const double *__restrict__ src, double *dst, int add) {
  const unsigned line = P.nout * P.inner, nchunk = (line + TR_T - 1) / TR_T, nblk = P.outer * nchunk;
  for (unsigned b = blockIdx.x; b < nblk; b += gridDim.x) {
    const unsigned o = b / nchunk, e = (b - o * nchunk) * TR_T + threadIdx.x;
    if (e >= line) continue;
    const unsigned r = e / P.inner, in = e - r * P.inner;
    const double *s = src + (size_t)o * P.nin * P.inner + in;
    const int k0 = P.ptr[r], k1 = P.ptr[r + 1];
    double acc = 0.0;
    if (k1 > k0) {
      acc = P.val[k0] * s[(size_t)P.idx[k0] * P.inner];
      for (int k = k0 + 1; k < k1; ++k) acc = fma(P.val[k], s[(size_t)P.idx[k] * P.inner], acc);
    }
    double *d = dst + (size_t)o * line + e;
    *d = add ? *d + acc : acc;
  }
}

}  // namespace igx
