// block_vec.hpp -- block-vector algebra on IGXVec: IGXVecMDot (G = X^T Y) and IGXVecMAXPY (Y = beta Y + X C) for two blocks of up to BV_MAX
// vectors, and the fused residual sweep of IGXEigenSolve (the host side: solve_loops.hpp).  Included by the main unit only, after krylov.hpp,
// whose reduction discipline it keeps: capped grids, one partial per workgroup in its own slab slot, slots added in index order by a
// finishing kernel, no atomics: bit-repeatable.  The columns of a block are separate allocations, handed over as a table of pointers in the
// kernel arguments (BvCols: 384 bytes).
//   bv_mdot<TX, TY>  a tall-skinny contraction over the rows on v_mfma_f64_16x16x4_f64 with the ROW as the MFMA's k: the summation index may
//       be dealt out to the lanes in any way, so a lane owns a RUN of BV_RUN = 8 consecutive rows of "its" column of every 16-wide tile
//       (lane l: column l & 15, k slot l >> 4) and reads it in four 16-byte loads per column; the four k slots of a column read 256
//       consecutive bytes.  No LDS staging, no barrier in the loop: (TX + TY) * 4 loads of 16 bytes in flight per lane.  Eight MFMAs per
//       tile pair and step consume the run (first the .x halves, then the .y halves, of the four loads in order).  A wavefront walks the
//       steps w, w + W, ... of BV_STEP = 32 rows (w its index in the grid, W the grid's wavefronts); the eight wavefronts of a workgroup
//       are added in wave order through LDS, tile by tile, and the workgroup stores its nx x ny partial into slot blockIdx.x.
//       A: lane l holds X_{16 tx + (l & 15)}[row], k = l >> 4;  B: lane l holds Y_{16 ty + (l & 15)}[row];  D: lane l, register r holds
//       G[16 tx + (l >> 4) + 4 r][16 ty + (l & 15)].  Columns past nx / ny and rows past n feed zeros and are never read.
//   bv_mdot_finish   G[e] = the sum over the slots of entry e, in slot order (one thread per entry).
//   bv_maxpy<NXB>    one row per thread (adjacent lanes: 512 consecutive bytes per column and wavefront), the row's nx inputs held in
//       registers (NXB blocks of 8, zeros past nx), then for every output j: s = beta y, s = fma(C[i][j], x_i, s) in ascending i, on the
//       vector units: the stream moves (nx + 2 ny) 8 bytes per row against nx ny multiply-adds (48 x 48: 4 flop per byte, a third of the
//       balance of the FP64 vector units against HBM), so the matrix cores have nothing to win, their D layout would scatter the stores in 32-byte pieces, and here
//       the order of the sum is written down.  C comes from a small device buffer [ny][8 NXB] (zero past nx) through uniform loads.
//   bv_resid         R_j = AX_j - theta_j BX_j for all columns in one sweep of 16-byte accesses, with the partials of |R_j|^2 and |AX_j|^2
//       in slabs 2 j and 2 j + 1;  bv_record adds the 2 m slabs in index order into the record the host reads.
#pragma once
#include "krylov.hpp"

namespace igx {

constexpr int BV_MAX = 48;                 // columns of a block at the most (three tiles of 16)
constexpr int BV_RUN = 8;                  // consecutive rows a lane reads of each of its columns per step
constexpr int BV_STEP = 4 * BV_RUN;        // rows a wavefront contracts per step: four k slots
constexpr int BV_EIG_MAX = 16;             // columns of IGXEigenSolve's block at the most
struct BvCols { double *p[BV_MAX]; };
struct BvEigCols { double *p[BV_EIG_MAX]; };
struct BvTheta { double v[BV_EIG_MAX]; };
typedef double bv_d4 __attribute__((ext_vector_type(4)));

// rows (row, row + 1) of a column, row even; zeros past n and for a column that is not there
__device__ inline kr_d2 bv_load2(const double *p, long long row, long long n) {
  if (!p || row >= n) return kr_d2{0.0, 0.0};
  if (row + 1 < n) return *reinterpret_cast<const kr_d2 *>(p + row);
  return kr_d2{p[row], 0.0};
}

template <int TX, int TY>
__global__ void __launch_bounds__(KR_T) bv_mdot(const BvCols X, int nx, const BvCols Y, int ny, long long n, double *slab) {
  __shared__ double red[KR_T / 64][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, ks = lane >> 4;
  const double *xp[TX], *yp[TY];
#pragma unroll
  for (int t = 0; t < TX; ++t) xp[t] = 16 * t + col < nx ? X.p[16 * t + col] : nullptr;
#pragma unroll
  for (int t = 0; t < TY; ++t) yp[t] = 16 * t + col < ny ? Y.p[16 * t + col] : nullptr;
  bv_d4 acc[TX][TY];
#pragma unroll
  for (int a = 0; a < TX; ++a)
#pragma unroll
    for (int b = 0; b < TY; ++b) acc[a][b] = bv_d4{0.0, 0.0, 0.0, 0.0};
  const long long nwaves = (long long)gridDim.x * (KR_T / 64), w = (long long)blockIdx.x * (KR_T / 64) + wave;
  for (long long r0 = w * BV_STEP; r0 < n; r0 += nwaves * BV_STEP) {
    const long long r = r0 + (long long)ks * BV_RUN;
    kr_d2 xv[TX][BV_RUN / 2], yv[TY][BV_RUN / 2];
#pragma unroll
    for (int t = 0; t < TX; ++t)
#pragma unroll
      for (int q = 0; q < BV_RUN / 2; ++q) xv[t][q] = bv_load2(xp[t], r + 2 * q, n);
#pragma unroll
    for (int t = 0; t < TY; ++t)
#pragma unroll
      for (int q = 0; q < BV_RUN / 2; ++q) yv[t][q] = bv_load2(yp[t], r + 2 * q, n);
#pragma unroll
    for (int q = 0; q < BV_RUN / 2; ++q)
#pragma unroll
      for (int a = 0; a < TX; ++a)
#pragma unroll
        for (int b = 0; b < TY; ++b) {
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[a][q].x, yv[b][q].x, acc[a][b], 0, 0, 0);
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[a][q].y, yv[b][q].y, acc[a][b], 0, 0, 0);
        }
  }
  // the workgroup's partial: the eight wavefronts in wave order, tile by tile; thread t < 256 owns register t >> 6 of lane t & 63
  const int reg = threadIdx.x >> 6, ln = threadIdx.x & 63;
  double *mine = slab + (size_t)blockIdx.x * nx * ny;
#pragma unroll
  for (int a = 0; a < TX; ++a)
#pragma unroll
    for (int b = 0; b < TY; ++b) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[wave][k * 64 + lane] = acc[a][b][k];
      __syncthreads();
      if (threadIdx.x < 256) {
        double s = red[0][threadIdx.x];
        for (int v = 1; v < KR_T / 64; ++v) s += red[v][threadIdx.x];
        const int i = 16 * a + (ln >> 4) + 4 * reg, j = 16 * b + (ln & 15);
        if (i < nx && j < ny) mine[i * ny + j] = s;
      }
      __syncthreads();
    }
}

__global__ void __launch_bounds__(256) bv_mdot_finish(const double *slab, int nslots, int count, double *G) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  double s = 0.0;
  for (int b = 0; b < nslots; ++b) s += slab[(size_t)b * count + e];
  G[e] = s;
}

template <int NXB>
__global__ void __launch_bounds__(KR_T) bv_maxpy(const BvCols Y, int ny, const BvCols X, int nx, const double *__restrict__ C, double beta, long long n) {
  constexpr int NXP = 8 * NXB;
  for (long long r = (long long)blockIdx.x * KR_T + threadIdx.x; r < n; r += (long long)gridDim.x * KR_T) {
    double x[NXP];
#pragma unroll
    for (int i = 0; i < NXP; ++i) x[i] = i < nx ? X.p[i][r] : 0.0;
    for (int j = 0; j < ny; ++j) {
      const double *c = C + j * NXP;
      double *y = Y.p[j];
      double s = beta == 0.0 ? 0.0 : beta * y[r];
#pragma unroll
      for (int i = 0; i < NXP; ++i) s = __builtin_fma(c[i], x[i], s);
      y[r] = s;
    }
  }
}

#include "kr_sweep_begin.hpp"
__device__ inline double bv_resid_of(double ax, double theta, double bx) {
#pragma clang fp contract(off)
  const double t = theta * bx;
  return ax - t;
}
// slabs: [2 m][KR_G]; always KR_G workgroups
__global__ void __launch_bounds__(KR_T) bv_resid(const BvEigCols R, const BvEigCols AX, const BvEigCols BX, const BvTheta th, int m, long long n, double *slabs) {
  __shared__ double red[KR_T / 64];
  for (int j = 0; j < m; ++j) {
    double *r = R.p[j]; const double *ax = AX.p[j], *bx = BX.p[j]; const double theta = th.v[j];
    double rr = 0.0, aa = 0.0;
    KR_PAIRS(i) {
      const kr_d2 u = KR_C2(ax)[i], v = KR_C2(bx)[i];
      const kr_d2 q = kr_d2{bv_resid_of(u.x, theta, v.x), bv_resid_of(u.y, theta, v.y)};
      KR_V2(r)[i] = q; rr += q.x * q.x; rr += q.y * q.y; aa += u.x * u.x; aa += u.y * u.y;
    }
    if (KR_TAIL) { const double u = ax[n - 1], q = bv_resid_of(u, theta, bx[n - 1]); r[n - 1] = q; rr += q * q; aa += u * u; }
    rr = kr_block_sum(rr, red); aa = kr_block_sum(aa, red);
    if (threadIdx.x == 0) { slabs[(size_t)(2 * j) * KR_G + blockIdx.x] = rr; slabs[(size_t)(2 * j + 1) * KR_G + blockIdx.x] = aa; }
  }
}
#include "kr_sweep_end.hpp"
__global__ void __launch_bounds__(64) bv_record(const double *slabs, int count, double *rec) {
  if ((int)threadIdx.x < count) rec[threadIdx.x] = kr_slab_sum(slabs + (size_t)threadIdx.x * KR_G);
}

// workgroups of bv_mdot: one step per wavefront at the least, KR_G at the most (the slots of the slab)
inline unsigned bv_mdot_grid(long long n) { const long long per = (long long)(KR_T / 64) * BV_STEP, w = (n + per - 1) / per; return (unsigned)(w < 1 ? 1 : (w > KR_G ? KR_G : w)); }
// ... of bv_maxpy: one row per thread
inline unsigned bv_maxpy_grid(long long n) { const long long w = (n + KR_T - 1) / KR_T; return (unsigned)(w < 1 ? 1 : (w > KR_G ? KR_G : w)); }

typedef void (*bv_mdot_fn)(const BvCols, int, const BvCols, int, long long, double *);
inline bv_mdot_fn bv_mdot_kernel(int tx, int ty) {
  static const bv_mdot_fn table[3][3] = {{bv_mdot<1, 1>, bv_mdot<1, 2>, bv_mdot<1, 3>}, {bv_mdot<2, 1>, bv_mdot<2, 2>, bv_mdot<2, 3>}, {bv_mdot<3, 1>, bv_mdot<3, 2>, bv_mdot<3, 3>}};
  return table[tx - 1][ty - 1];
}
typedef void (*bv_maxpy_fn)(const BvCols, int, const BvCols, int, const double *, double, long long);
inline bv_maxpy_fn bv_maxpy_kernel(int nxb) {
  static const bv_maxpy_fn table[6] = {bv_maxpy<1>, bv_maxpy<2>, bv_maxpy<3>, bv_maxpy<4>, bv_maxpy<5>, bv_maxpy<6>};
  return table[nxb - 1];
}

}  // namespace igx
