// block_diag.hpp -- the two per-node kernels that make the point-block diagonal (IGXCompute*BlockDiagonal, vec_sumfact.hpp: BLOCK) a
// preconditioner on the device: PCPBJACOBI's set-up (MatInvertBlockDiagonal) and its apply.
// The blocks live in dof ordinary vectors, one per block column: col[j][node * dof + i] = A_(node,i),(node,j).  One thread per node, the
// block in registers, dof a template parameter (1..MAXBC).  A thread reads dof consecutive doubles of a column and a wavefront 64 * dof
// consecutive ones: every column is read and written as one contiguous stream.
#pragma once
#include <hip/hip_runtime.h>
#include "igx.hpp"

namespace igx {

struct BlockCols { double *col[MAXBC]; };

// In-place Gauss-Jordan with partial pivoting (row swaps on the way down, the matching column swaps undone at the end): dof^2 registers, no
// second copy.  Every index is a compile-time one -- the pivot row is swapped in by selects over the unrolled candidates -- so the block
// stays in registers.  A zero or non-finite pivot: the block becomes the zero block and is counted (nsing may be null).
template <int DOF>
__global__ void __launch_bounds__(256) block_diag_invert(BlockCols B, long long nnode, unsigned long long *nsing) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= nnode) return;
  double A[DOF][DOF];
#pragma unroll
  for (int j = 0; j < DOF; ++j)
#pragma unroll
    for (int i = 0; i < DOF; ++i) A[i][j] = B.col[j][n * DOF + i];
  int perm[DOF];
  bool bad = false;
#pragma unroll
  for (int c = 0; c < DOF; ++c) {
    int pr = c; double pm = fabs(A[c][c]);
#pragma unroll
    for (int r = c + 1; r < DOF; ++r) { const double v = fabs(A[r][c]); if (v > pm) { pm = v; pr = r; } }
    perm[c] = pr;
#pragma unroll
    for (int r = c + 1; r < DOF; ++r) {      // rows c and pr change places
      const bool sw = pr == r;
#pragma unroll
      for (int k = 0; k < DOF; ++k) { const double a = A[c][k], b = A[r][k]; A[c][k] = sw ? b : a; A[r][k] = sw ? a : b; }
    }
    const double pv = A[c][c];
    const bool ok = fabs(pv) > 0.0 && fabs(pv) < __builtin_huge_val();      // (false for 0, infinities and NaN)
    bad = bad || !ok;
    const double ip = ok ? 1.0 / pv : 0.0;
    A[c][c] = 1.0;
#pragma unroll
    for (int k = 0; k < DOF; ++k) A[c][k] *= ip;
#pragma unroll
    for (int r = 0; r < DOF; ++r) {
      if (r == c) continue;
      const double f = A[r][c];
      A[r][c] = 0.0;
#pragma unroll
      for (int k = 0; k < DOF; ++k) A[r][k] -= f * A[c][k];
    }
  }
#pragma unroll
  for (int c = DOF - 1; c >= 0; --c) {      // the inverse of the row-permuted block: its columns go back in reverse order
#pragma unroll
    for (int k = c + 1; k < DOF; ++k) {
      const bool sw = perm[c] == k;
#pragma unroll
      for (int r = 0; r < DOF; ++r) { const double a = A[r][c], b = A[r][k]; A[r][c] = sw ? b : a; A[r][k] = sw ? a : b; }
    }
  }
#pragma unroll
  for (int j = 0; j < DOF; ++j)
#pragma unroll
    for (int i = 0; i < DOF; ++i) B.col[j][n * DOF + i] = bad ? 0.0 : A[i][j];
  if (bad && nsing) atomicAdd(nsing, 1ull);
}

// Y_node = B_node X_node: dof^2 + dof doubles read, dof written per node
template <int DOF>
__global__ void __launch_bounds__(256) block_diag_apply(BlockCols B, const double *__restrict__ X, double *__restrict__ Y, long long nnode) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= nnode) return;
  double x[DOF], y[DOF];
#pragma unroll
  for (int j = 0; j < DOF; ++j) x[j] = X[n * DOF + j];
#pragma unroll
  for (int i = 0; i < DOF; ++i) y[i] = 0.0;
#pragma unroll
  for (int j = 0; j < DOF; ++j)
#pragma unroll
    for (int i = 0; i < DOF; ++i) y[i] += B.col[j][n * DOF + i] * x[j];
#pragma unroll
  for (int i = 0; i < DOF; ++i) Y[n * DOF + i] = y[i];
}

#ifndef IGX_RTC
template <int DOF = 1>
static void block_diag_launch(int dof, bool invert, const BlockCols &B, const double *X, double *Y, long long nnode, unsigned long long *nsing, hipStream_t stream) {
  if constexpr (DOF <= MAXBC) {
    if (dof != DOF) return block_diag_launch<DOF + 1>(dof, invert, B, X, Y, nnode, nsing, stream);
    const unsigned grid = (unsigned)((nnode + 255) / 256);
    if (!grid) return;
    if (invert) hipLaunchKernelGGL((block_diag_invert<DOF>), dim3(grid), dim3(256), 0, stream, B, nnode, nsing);
    else hipLaunchKernelGGL((block_diag_apply<DOF>), dim3(grid), dim3(256), 0, stream, B, X, Y, nnode);
  }
}
#endif

}  // namespace igx
