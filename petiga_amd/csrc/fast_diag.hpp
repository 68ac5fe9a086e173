// fast_diag.hpp -- the contraction of the fast-diagonalisation preconditioner (IGXFastDiagApply; the host half: host.cpp).
//   out[o][i][c] = sum_j T_f[j][i] * in[o][j][c],   i, j < n,  c < inner,  f = c % dof
// along one axis of the vector seen as [outer][n][inner]: axis 0 has inner = dof, axis 1 inner = n0 dof, axis 2 inner = n0 n1 dof.  No
// transposed copy of the vector exists: the strides do it.  T_f is the n x n table of field f's eigen-system on the axis, zero outside its
// free range (rows of fixed functions, modes past m), so every field runs the same full-size contraction and a fixed node carries zeros.
// One workgroup of four wavefronts owns 64 columns (o, c) of one field and NT * 16 output rows; a wavefront owns 16 of the columns and
// all the rows, NT accumulator tiles of v_mfma_f64_16x16x4_f64:
//   A[row i][k j] = T[j][i]: lane l holds row l & 15, k = l >> 4;  B[k j][col] = in[j][col]: lane l holds col l & 15, k = l >> 4;
//   D: lane l, register r holds row (l >> 4) + 4 r, col l & 15.
// The contraction runs in chunks of 16 j: the chunk of T (16 x NT*16) and of the input (16 x 64) are staged in LDS, zero-filled past n and
// past the last column, so neither the k loop of 4 nor the tiles of 16 have a remainder of their own.  Sums run in a fixed order, no
// atomics: bit-repeatable.  The epilogue of the third forward contraction scales by the reciprocal denominators; the one of the last
// backward contraction writes the quotient R / count into the fixed rows.
#pragma once
#include <hip/hip_runtime.h>
#include "igx.hpp"

namespace igx {

constexpr int FD_COLS = 64;        // columns per workgroup (16 per wavefront)
constexpr int FD_KJ = 16;          // contraction chunk
constexpr int FD_BSTRIDE = 80;     // LDS row strides in doubles, = 16 mod 32: the four k rows an operand read touches fall into distinct banks
constexpr int fd_tstride(int nt) { return (nt * 16) | 16; }

enum FdMode { FD_PLAIN = 0, FD_SCALE = 1, FD_FINAL = 2 };

struct FdArgs {
  const double *in; double *out;
  const double *T[MAXBC];          // per field: [n][n] row-major, T[j][i]
  int n;                           // length of the contracted axis (in and out)
  long long inner, outer;          // the vector as [outer][n][inner]
  int dof, nsel;                   // nsel = dof: a workgroup's columns belong to one field; nsel = 1: every field has the tables of field 0
  int mode;
  // epilogues
  int n0, n1, n2;
  const double *s[3][MAXBC];       // FD_SCALE: beta_d lambda_d per field, [n_d], zero past m
  double alpha, thresh;
  const double *R;                 // FD_FINAL: the vector the preconditioner is applied to
  const double *count[3];          // FD_FINAL: elements per function, [n_d]
  unsigned char lo[3][MAXBC], hi[3][MAXBC];   // FD_FINAL: the first / last function of the axis is fixed for the field
};

typedef double fd_d4 __attribute__((ext_vector_type(4)));

template <int NT>
__global__ void __launch_bounds__(256) fast_diag_contract(const FdArgs a) {
  constexpr int TS = fd_tstride(NT);
  __shared__ double Tl[FD_KJ * TS];
  __shared__ double Bl[FD_KJ * FD_BSTRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n;
  const long long cpf = a.inner / a.nsel;                    // columns of one field per outer index
  const long long ncols = a.outer * cpf;                     // columns per field
  const long long ntile = (ncols + FD_COLS - 1) / FD_COLS;   // column tiles per field
  const int fsel = (int)(blockIdx.x / ntile);
  const long long col0 = (long long)(blockIdx.x % ntile) * FD_COLS;
  const int i0 = blockIdx.y * (NT * 16);
  const double *__restrict__ T = a.T[fsel];
  // element j of column q of this field sits at colbase(q) + j * inner
  auto colbase = [&](long long q) { const long long o = q / cpf, c = q % cpf; return o * n * a.inner + c * a.nsel + fsel; };
  const bool jfast = a.inner < 8;      // axis 0: consecutive j are (nearly) consecutive in memory, consecutive columns are not
  fd_d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = fd_d4{0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < n; j0 += FD_KJ) {
    for (int e = tid; e < FD_KJ * NT * 16; e += 256) {      // T chunk: rows j0.., columns i0..
      const int jj = e / (NT * 16), ii = e % (NT * 16);
      const int j = j0 + jj, i = i0 + ii;
      Tl[jj * TS + ii] = (j < n && i < n) ? T[(size_t)j * n + i] : 0.0;
    }
    for (int e = tid; e < FD_KJ * FD_COLS; e += 256) {      // input chunk
      const int jj = jfast ? e % FD_KJ : e / FD_COLS, cc = jfast ? e / FD_KJ : e % FD_COLS;
      const int j = j0 + jj; const long long q = col0 + cc;
      Bl[jj * FD_BSTRIDE + cc] = (j < n && q < ncols) ? a.in[colbase(q) + (long long)j * a.inner] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k0 = 0; k0 < FD_KJ; k0 += 4) {
      const int kk = k0 + (lane >> 4);
      const double b = Bl[kk * FD_BSTRIDE + wave * 16 + (lane & 15)];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Tl[kk * TS + t * 16 + (lane & 15)], b, acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  const long long q = col0 + wave * 16 + (lane & 15);
  if (q >= ncols) return;
  const long long base = colbase(q);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + t * 16 + (lane >> 4) + 4 * r;
      if (i >= n) continue;
      const long long idx = base + (long long)i * a.inner;
      double v = acc[t][r];
      if (a.mode != FD_PLAIN) {
        const long long node = idx / a.dof; const int f = fsel;      // (nsel = 1: the tables of field 0 are every field's)
        const int c0 = (int)(node % a.n0), c1 = (int)((node / a.n0) % a.n1), c2 = (int)(node / ((long long)a.n0 * a.n1));
        if (a.mode == FD_SCALE) {
          const double den = ((a.alpha + a.s[0][f][c0]) + a.s[1][f][c1]) + a.s[2][f][c2];
          v = fabs(den) <= a.thresh ? 0.0 : v * (1.0 / den);
        } else {
          const bool fixed = (a.lo[0][f] && c0 == 0) || (a.hi[0][f] && c0 == a.n0 - 1) || (a.lo[1][f] && c1 == 0) || (a.hi[1][f] && c1 == a.n1 - 1) ||
                             (a.lo[2][f] && c2 == 0) || (a.hi[2][f] && c2 == a.n2 - 1);
          if (fixed) v = a.R[idx] / (a.count[0][c0] * a.count[1][c1] * a.count[2][c2]);
        }
      }
      a.out[idx] = v;
    }
}

#ifndef IGX_RTC
// row tiles per workgroup for an axis of n functions: the tiles split evenly over the fewest workgroups of at most 16
inline int fd_row_tiles(int n) {
  const int tiles = (n + 15) / 16, blocks = (tiles + 15) / 16, want = (tiles + blocks - 1) / blocks;
  for (int nt : {1, 2, 3, 4, 6, 9, 12, 16}) if (nt >= want) return nt;
  return 16;
}
inline int fast_diag_launch(const FdArgs &a, hipStream_t stream) {
  const int nt = fd_row_tiles(a.n);
  const long long ncols = a.outer * (a.inner / a.nsel), ntile = (ncols + FD_COLS - 1) / FD_COLS, gx = ntile * a.nsel;
  const int gy = (a.n + nt * 16 - 1) / (nt * 16);
  if (gx <= 0 || gx > 0x7fffffffLL || gy > 65535) return 1;
  const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
  switch (nt) {
    case 1:  hipLaunchKernelGGL((fast_diag_contract<1>), grid, block, 0, stream, a); break;
    case 2:  hipLaunchKernelGGL((fast_diag_contract<2>), grid, block, 0, stream, a); break;
    case 3:  hipLaunchKernelGGL((fast_diag_contract<3>), grid, block, 0, stream, a); break;
    case 4:  hipLaunchKernelGGL((fast_diag_contract<4>), grid, block, 0, stream, a); break;
    case 6:  hipLaunchKernelGGL((fast_diag_contract<6>), grid, block, 0, stream, a); break;
    case 9:  hipLaunchKernelGGL((fast_diag_contract<9>), grid, block, 0, stream, a); break;
    case 12: hipLaunchKernelGGL((fast_diag_contract<12>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((fast_diag_contract<16>), grid, block, 0, stream, a); break;
  }
  return 0;
}
#endif

}  // namespace igx
