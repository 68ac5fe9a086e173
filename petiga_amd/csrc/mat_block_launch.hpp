// mat_block_launch.hpp -- the host launcher of mat_mult_block (mat_ops.hpp).  A header of its own, included by
// mat_ops_host.hpp: a unit that includes mat_ops.hpp for its kernels alone does not instantiate the block kernel's 112 cases with it.
#pragma once
#include "mat_ops.hpp"

namespace igx {

// the launch of mat_mult_block for nc = 2, 4 or 8 columns starting at x[0], y[0]; the widths a block size takes are those mat_block_plan
// gives it (2 .. mat_block_nc(bs)) and no wider one is instantiated.  false: a block size or a width the device path does not hold.
template <int BS, int G, int NC>
inline void mat_mult_block_launch_nc(bool tables, const MatPat &P, long long nbrows, const int64_t *browptr, const int32_t *bcolidx, const double *val, const double *const *x, double *const *y, hipStream_t st) {
  MatBlockCols<NC> V;
  for (int c = 0; c < NC; ++c) { V.x[c] = x[c]; V.y[c] = y[c]; }
  const unsigned grid = (unsigned)((nbrows + MM_T / G - 1) / (MM_T / G));
  if (tables) hipLaunchKernelGGL((mat_mult_block<BS, G, true, NC>), dim3(grid), dim3(MM_T), 0, st, P, nbrows, browptr, bcolidx, val, V);
  else hipLaunchKernelGGL((mat_mult_block<BS, G, false, NC>), dim3(grid), dim3(MM_T), 0, st, P, nbrows, browptr, bcolidx, val, V);
}
template <int BS, int NC>
inline bool mat_mult_block_launch_g(int lanes, bool tables, const MatPat &P, long long nbrows, const int64_t *browptr, const int32_t *bcolidx, const double *val, const double *const *x, double *const *y, hipStream_t st) {
  if constexpr (NC <= mat_block_nc(BS)) {
    switch (lanes) {
      case 8:  mat_mult_block_launch_nc<BS, 8, NC>(tables, P, nbrows, browptr, bcolidx, val, x, y, st); break;
      case 16: mat_mult_block_launch_nc<BS, 16, NC>(tables, P, nbrows, browptr, bcolidx, val, x, y, st); break;
      case 32: mat_mult_block_launch_nc<BS, 32, NC>(tables, P, nbrows, browptr, bcolidx, val, x, y, st); break;
      default: mat_mult_block_launch_nc<BS, 64, NC>(tables, P, nbrows, browptr, bcolidx, val, x, y, st); break;
    }
    return true;
  }
  return false;
}
template <int BS>
inline bool mat_mult_block_launch_bs(int nc, int lanes, bool tables, const MatPat &P, long long nbrows, const int64_t *browptr, const int32_t *bcolidx, const double *val, const double *const *x, double *const *y, hipStream_t st) {
  switch (nc) {
    case 2: return mat_mult_block_launch_g<BS, 2>(lanes, tables, P, nbrows, browptr, bcolidx, val, x, y, st);
    case 4: return mat_mult_block_launch_g<BS, 4>(lanes, tables, P, nbrows, browptr, bcolidx, val, x, y, st);
    case 8: return mat_mult_block_launch_g<BS, 8>(lanes, tables, P, nbrows, browptr, bcolidx, val, x, y, st);
  }
  return false;
}
inline bool mat_mult_block_launch(int bs, int nc, int lanes, bool tables, const MatPat &P, long long nbrows, const int64_t *browptr, const int32_t *bcolidx, const double *val, const double *const *x, double *const *y, hipStream_t st) {
  switch (bs) {
#define IGX_MM_CASE(B) case B: return mat_mult_block_launch_bs<B>(nc, lanes, tables, P, nbrows, browptr, bcolidx, val, x, y, st);
    IGX_MM_CASE(1) IGX_MM_CASE(2) IGX_MM_CASE(3) IGX_MM_CASE(4) IGX_MM_CASE(5) IGX_MM_CASE(6) IGX_MM_CASE(7) IGX_MM_CASE(8)
#undef IGX_MM_CASE
  }
  return false;
}

}  // namespace igx
