// mat_ops.hpp -- the stored block-CSR matrix of IGXCreateMat as an operator: y = A x (IGXMatMult, and through it IGXMatSolve) and the copies
// of its diagonal and of its bs x bs diagonal blocks (IGXMatGetDiagonal / IGXMatGetBlockDiagonal).  Included by the main unit only, behind
// everything else; the host entries follow it in mat_ops_host.hpp.  One rank on every axis: the column node index is then the row index of x.
// Layout (k_browptr, k_bcolidx): row r = (r0, r1, r2) owns c0 c1 c2 blocks, c_d = rcnt[d][r_d]; block k = k0 + c0 (k1 + c1 k2) lies at
// val[(browptr[r] + k) bs^2], row-major inside, and its column node is rcol[0][r0 W0 + k0] + ncol0 (rcol[1][r1 W1 + k1] + ncol1 rcol[2][r2 W2 + k2]).
// mat_mult: G lanes per row (G = 8, 16, 32: sub-groups of a wavefront, 64 / G rows per wavefront; G = 64: one wavefront per row), MM_T / G rows
// per workgroup.  The row's len = nblk bs^2 doubles are contiguous; its lanes stride over them in pairs of 16 bytes.  A row starts at an odd
// double wherever browptr[r] bs^2 is odd: the pairs then begin one double later, and the double before the first pair (head) and the one
// behind the last (tail) are taken alone, by lane 0 and by lane G - 1, as the run sweeps of krylov.hpp take their ends.  Pair q belongs to
// lane q mod G.  For bs > 1 the doubles of a lane belong to different block rows i = (e mod bs^2) / bs: a lane keeps bs sums and adds each
// product to the one its entry names, so the loads stay contiguous whatever bs is.  The bs sums then go through the same xor butterfly over
// the G lanes (every lane ends with the same bits) and lanes 0 .. bs - 1 store y[r bs + lane]: no atomics, and a row's result depends on its
// own values, its own start's parity and the x it reads -- not on the grid, nor on the wavefront that took it.
// The column of an entry: TABLES = true from the per-axis tables (a few KB, cache resident; the divisions by c0 and c0 c1 <= 15^2 of k < 15^3
// are a float multiplication by the reciprocal, exact at these sizes; a row whose columns are consecutive on every axis -- all but the rows a
// periodic axis wraps -- reads six table entries once and none per entry), TABLES = false from bcolidx (4 bytes per block more to read).
#pragma once
#include <hip/hip_runtime.h>
#include "igx.hpp"

namespace igx {

constexpr int MM_T = 256;      // threads per workgroup
struct MatPat { int nrow[3], ncol[3], W[3]; const int *rcnt[3]; const int *rcol[3]; };
struct MatCols { double *col[MAXBC]; };

// lanes per row from the longest row's doubles: the smallest sub-group in which a lane takes two pairs at the most, else the wavefront
inline int mat_mult_lanes(long long longest) { return longest <= 32 ? 8 : longest <= 64 ? 16 : longest <= 128 ? 32 : 64; }

// k / c for 0 <= k < W^3 and 1 <= c <= W^2 with rc = 1 / c in float, W = 2p + 1 the widest stencil of an axis.  (k + 1/2) / c is at least
// 1 / (2 W^2) away from an integer; the float product differs from it by at most 4 ulp of a number below W (the reciprocal, the product and
// the conversion of k + 1/2, which is exact below 2^23), i.e. by 2.4e-7 W.  Exact while 2.4e-7 W < 1 / (2 W^2), W < 127; the host takes the
// tables up to MM_MAXW = 63 (a margin of 8) and bcolidx beyond.  The library assembles p <= 7 today (W <= 15: margin 600).
constexpr int MM_MAXW = 63;
__device__ inline int mm_div(int k, float rc) { return (int)(((float)k + 0.5f) * rc); }

template <int BS, int G, bool TABLES>
__global__ void __launch_bounds__(MM_T) mat_mult(const MatPat P, long long nbrows, const int64_t *__restrict__ browptr, const int32_t *__restrict__ bcolidx,
                                                 const double *__restrict__ val, const double *__restrict__ x, double *__restrict__ y) {
  constexpr int BB = BS * BS;
  const int lane = threadIdx.x % G;
  const long long r = (long long)blockIdx.x * (MM_T / G) + threadIdx.x / G;
  if (r >= nbrows) return;      // (a whole sub-group leaves: its shuffles stay inside it)
  const long long b0 = browptr[r];
  const int nblk = (int)(browptr[r + 1] - b0), len = nblk * BB;
  int c0 = 1, c01 = 1;
  float rc0 = 1.0f, rc01 = 1.0f;
  const int *t0 = nullptr, *t1 = nullptr, *t2 = nullptr;
  const int ncol0 = P.ncol[0], ncol1 = P.ncol[1];
  // a row whose columns are consecutive on every axis (every row but those a periodic axis wraps: sorted and distinct, so last - first =
  // count - 1 says it) needs its first column alone: col(k) = first + k0 + ncol0 (k1 + ncol1 k2), and no table is read per entry
  bool run = false;
  int first = 0;
  if (TABLES) {
    const unsigned ru = (unsigned)r, q = ru / (unsigned)P.nrow[0];
    const int r0 = (int)(ru - q * (unsigned)P.nrow[0]), r2 = (int)(q / (unsigned)P.nrow[1]), r1 = (int)(q - (unsigned)r2 * (unsigned)P.nrow[1]);
    const int c1 = P.rcnt[1][r1], c2 = P.rcnt[2][r2];
    c0 = P.rcnt[0][r0]; c01 = c0 * c1;
    rc0 = 1.0f / (float)c0; rc01 = 1.0f / (float)c01;
    t0 = P.rcol[0] + r0 * P.W[0]; t1 = P.rcol[1] + r1 * P.W[1]; t2 = P.rcol[2] + r2 * P.W[2];
    const int f0 = t0[0], f1 = t1[0], f2 = t2[0];
    run = t0[c0 - 1] - f0 == c0 - 1 && t1[c1 - 1] - f1 == c1 - 1 && t2[c2 - 1] - f2 == c2 - 1;
    first = f0 + ncol0 * (f1 + ncol1 * f2);
  }
  auto column = [&](int k) -> long long {
    if (!TABLES) return (long long)bcolidx[b0 + k];
    const int k2 = mm_div(k, rc01), w = k - k2 * c01, k1 = mm_div(w, rc0), k0 = w - k1 * c0;
    if (run) return (long long)(first + k0 + ncol0 * (k1 + ncol1 * k2));
    return (long long)(t0[k0] + ncol0 * (t1[k1] + ncol1 * t2[k2]));
  };
  double acc[BS];
#pragma unroll
  for (int i = 0; i < BS; ++i) acc[i] = 0.0;
  auto add = [&](int e, double v) {      // entry e of the row: block e / bs^2, block row i, block column j
    const int k = e / BB, w = e - k * BB, i = w / BS, j = w - i * BS;
    const double xv = x[column(k) * BS + j];
#pragma unroll
    for (int ii = 0; ii < BS; ++ii) if (ii == i) acc[ii] = fma(v, xv, acc[ii]);
  };
  const double *row = val + b0 * BB;
  const int head = (int)((b0 * BB) & 1) & (len > 0 ? 1 : 0), npairs = (len - head) >> 1, tail = (len - head) & 1;
  typedef double mm_d2 __attribute__((ext_vector_type(2)));
  const mm_d2 *pairs = reinterpret_cast<const mm_d2 *>(row + head);
#pragma unroll 2
  for (int q = lane; q < npairs; q += G) {
    const mm_d2 v = pairs[q];
    add(head + 2 * q, v.x); add(head + 2 * q + 1, v.y);
  }
  if (head && lane == 0) add(0, row[0]);
  if (tail && lane == G - 1) add(len - 1, row[len - 1]);
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) acc[i] += __shfl_xor(acc[i], o, G);
  if (lane < BS) {
    double out = acc[0];
#pragma unroll
    for (int i = 1; i < BS; ++i) if (lane == i) out = acc[i];
    y[r * BS + lane] = out;
  }
}

// mat_mult_block: Y_c = A X_c for the NC columns of a chunk in one pass over val (IGXMatMultBlock).  mat_mult's lane mapping,
// pairs, head and tail, entry rule and column rule, restated and not shared: mat_mult stays the code it is.  A lane keeps BS x NC sums; for
// every value it loads once it gathers x_c[col bs + j] for the NC columns and does NC fmas.  Column c's products enter column c's sums in
// mat_mult's order (the strided pairs in ascending q, x before y of a pair, then the head on lane 0 and the tail on lane G - 1), with the same
// fma and the same xor butterfly: column c of the result is bit for bit what mat_mult stores for X_c, whatever NC is, wherever the column
// stands in the chunk and whatever the other columns hold.  Nothing is read from Y; no atomics.  val, browptr, bcolidx and the tables are read
// once per chunk.  The column pointers arrive by value.
template <int NC> struct MatBlockCols { const double *x[NC]; double *y[NC]; };
// columns of a full chunk by block size: BS NC sums in double are 2 BS NC VGPRs, 32 at the most here, so that nothing goes to scratch and four
// waves per SIMD stay resident (the gathered x of an unrolled pair of pairs takes up to 8 NC more).  What is left of a block after its
// full chunks goes to the next narrower widths (NC / 2, NC / 4, ... >= 2) and the last single column to mat_mult itself.
constexpr int mat_block_nc(int bs) { return bs <= 2 ? 8 : bs <= 4 ? 4 : 2; }
// the chunk plan of nx columns: widths[k] columns in launch k, in order; returns the number of launches (widths may be null).  Pure host code.
inline int mat_block_plan(int bs, int nx, int *widths) {
  int n = 0;
  for (int w = mat_block_nc(bs), left = nx; left > 0;) {
    while (w > left) w >>= 1;
    if (widths) widths[n] = w;
    ++n; left -= w;
  }
  return n;
}

template <int BS, int G, bool TABLES, int NC>
__global__ void __launch_bounds__(MM_T) mat_mult_block(const MatPat P, long long nbrows, const int64_t *__restrict__ browptr, const int32_t *__restrict__ bcolidx,
                                                       const double *__restrict__ val, const MatBlockCols<NC> V) {
  constexpr int BB = BS * BS;
  const int lane = threadIdx.x % G;
  const long long r = (long long)blockIdx.x * (MM_T / G) + threadIdx.x / G;
  if (r >= nbrows) return;
  const long long b0 = browptr[r];
  const int nblk = (int)(browptr[r + 1] - b0), len = nblk * BB;
  int c0 = 1, c01 = 1;
  float rc0 = 1.0f, rc01 = 1.0f;
  const int *t0 = nullptr, *t1 = nullptr, *t2 = nullptr;
  const int ncol0 = P.ncol[0], ncol1 = P.ncol[1];
  bool run = false;
  int first = 0;
  if (TABLES) {
    const unsigned ru = (unsigned)r, q = ru / (unsigned)P.nrow[0];
    const int r0 = (int)(ru - q * (unsigned)P.nrow[0]), r2 = (int)(q / (unsigned)P.nrow[1]), r1 = (int)(q - (unsigned)r2 * (unsigned)P.nrow[1]);
    const int c1 = P.rcnt[1][r1], c2 = P.rcnt[2][r2];
    c0 = P.rcnt[0][r0]; c01 = c0 * c1;
    rc0 = 1.0f / (float)c0; rc01 = 1.0f / (float)c01;
    t0 = P.rcol[0] + r0 * P.W[0]; t1 = P.rcol[1] + r1 * P.W[1]; t2 = P.rcol[2] + r2 * P.W[2];
    const int f0 = t0[0], f1 = t1[0], f2 = t2[0];
    run = t0[c0 - 1] - f0 == c0 - 1 && t1[c1 - 1] - f1 == c1 - 1 && t2[c2 - 1] - f2 == c2 - 1;
    first = f0 + ncol0 * (f1 + ncol1 * f2);
  }
  auto column = [&](int k) -> long long {
    if (!TABLES) return (long long)bcolidx[b0 + k];
    const int k2 = mm_div(k, rc01), w = k - k2 * c01, k1 = mm_div(w, rc0), k0 = w - k1 * c0;
    if (run) return (long long)(first + k0 + ncol0 * (k1 + ncol1 * k2));
    return (long long)(t0[k0] + ncol0 * (t1[k1] + ncol1 * t2[k2]));
  };
  double acc[BS][NC];
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[i][c] = 0.0;
  auto add = [&](int e, double v) {
    const int k = e / BB, w = e - k * BB, i = w / BS, j = w - i * BS;
    const long long at = column(k) * BS + j;
    double xv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) xv[c] = V.x[c][at];
#pragma unroll
    for (int ii = 0; ii < BS; ++ii) if (ii == i) {
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[ii][c] = fma(v, xv[c], acc[ii][c]);
    }
  };
  const double *row = val + b0 * BB;
  const int head = (int)((b0 * BB) & 1) & (len > 0 ? 1 : 0), npairs = (len - head) >> 1, tail = (len - head) & 1;
  typedef double mm_d2 __attribute__((ext_vector_type(2)));
  const mm_d2 *pairs = reinterpret_cast<const mm_d2 *>(row + head);
#pragma unroll 2
  for (int q = lane; q < npairs; q += G) {
    const mm_d2 v = pairs[q];
    add(head + 2 * q, v.x); add(head + 2 * q + 1, v.y);
  }
  if (head && lane == 0) add(0, row[0]);
  if (tail && lane == G - 1) add(len - 1, row[len - 1]);
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) acc[i][c] += __shfl_xor(acc[i][c], o, G);
  if (lane < BS) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      double out = acc[0][c];
#pragma unroll
      for (int i = 1; i < BS; ++i) if (lane == i) out = acc[i][c];
      V.y[c][r * BS + lane] = out;
    }
  }
}

// The diagonal block of every row, copied: one thread per scalar.  BLOCK = false: out.col[0][r bs + i] = A[r][r][i][i]; BLOCK = true: column j of
// the block goes to out.col[j][r bs + i] (the layout of IGXCompute*BlockDiagonal).  The block's position in the row comes from the per-axis
// tables: on each axis the place of the row's own node among the row's sorted columns.
template <bool BLOCK>
__global__ void __launch_bounds__(MM_T) mat_get_diag(const MatPat P, long long nbrows, int bs, const int64_t *__restrict__ browptr, const double *__restrict__ val, const MatCols out) {
  const int per = BLOCK ? bs * bs : bs;
  const long long t = (long long)blockIdx.x * MM_T + threadIdx.x;
  if (t >= nbrows * per) return;
  const long long r = t / per;
  const int w = (int)(t - r * per), i = BLOCK ? w / bs : w, j = BLOCK ? w - i * bs : w;
  const unsigned ru = (unsigned)r, q = ru / (unsigned)P.nrow[0];
  const int rd[3] = {(int)(ru - q * (unsigned)P.nrow[0]), (int)(q % (unsigned)P.nrow[1]), (int)(q / (unsigned)P.nrow[1])};
  int pos[3], cnt[3];
  bool found = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    cnt[d] = P.rcnt[d][rd[d]]; pos[d] = -1;
    const int *rc = P.rcol[d] + rd[d] * P.W[d];
    for (int k = 0; k < cnt[d]; ++k) if (rc[k] == rd[d]) pos[d] = k;
    found = found && pos[d] >= 0;
  }
  double v = 0.0;
  if (found) v = val[(browptr[r] + pos[0] + cnt[0] * (pos[1] + cnt[1] * pos[2])) * (long long)(bs * bs) + i * bs + j];
  double *dst = out.col[0];
  if (BLOCK) {
#pragma unroll
    for (int c = 1; c < MAXBC; ++c) if (c == j) dst = out.col[c];
  }
  dst[r * bs + i] = v;
}

// the launch of mat_mult for a block size, a sub-group and an index variant
template <int BS, int G>
inline void mat_mult_launch_g(bool tables, const MatPat &P, long long nbrows, const int64_t *browptr, const int32_t *bcolidx, const double *val, const double *x, double *y, hipStream_t st) {
  const unsigned grid = (unsigned)((nbrows + MM_T / G - 1) / (MM_T / G));
  if (tables) hipLaunchKernelGGL((mat_mult<BS, G, true>), dim3(grid), dim3(MM_T), 0, st, P, nbrows, browptr, bcolidx, val, x, y);
  else hipLaunchKernelGGL((mat_mult<BS, G, false>), dim3(grid), dim3(MM_T), 0, st, P, nbrows, browptr, bcolidx, val, x, y);
}
template <int BS>
inline void mat_mult_launch_bs(int lanes, bool tables, const MatPat &P, long long nbrows, const int64_t *browptr, const int32_t *bcolidx, const double *val, const double *x, double *y, hipStream_t st) {
  switch (lanes) {
    case 8:  mat_mult_launch_g<BS, 8>(tables, P, nbrows, browptr, bcolidx, val, x, y, st); break;
    case 16: mat_mult_launch_g<BS, 16>(tables, P, nbrows, browptr, bcolidx, val, x, y, st); break;
    case 32: mat_mult_launch_g<BS, 32>(tables, P, nbrows, browptr, bcolidx, val, x, y, st); break;
    default: mat_mult_launch_g<BS, 64>(tables, P, nbrows, browptr, bcolidx, val, x, y, st); break;
  }
}
// false: a block size the device path does not hold (bs > MAXBC)
inline bool mat_mult_launch(int bs, int lanes, bool tables, const MatPat &P, long long nbrows, const int64_t *browptr, const int32_t *bcolidx, const double *val, const double *x, double *y, hipStream_t st) {
  switch (bs) {
#define IGX_MM_CASE(B) case B: mat_mult_launch_bs<B>(lanes, tables, P, nbrows, browptr, bcolidx, val, x, y, st); return true;
    IGX_MM_CASE(1) IGX_MM_CASE(2) IGX_MM_CASE(3) IGX_MM_CASE(4) IGX_MM_CASE(5) IGX_MM_CASE(6) IGX_MM_CASE(7) IGX_MM_CASE(8)
#undef IGX_MM_CASE
  }
  return false;
}
inline void mat_get_diag_launch(bool block, const MatPat &P, long long nbrows, int bs, const int64_t *browptr, const double *val, const MatCols &out, hipStream_t st) {
  const long long n = nbrows * (block ? bs * bs : bs);
  const unsigned grid = (unsigned)((n + MM_T - 1) / MM_T);
  if (block) hipLaunchKernelGGL(mat_get_diag<true>, dim3(grid), dim3(MM_T), 0, st, P, nbrows, bs, browptr, val, out);
  else hipLaunchKernelGGL(mat_get_diag<false>, dim3(grid), dim3(MM_T), 0, st, P, nbrows, bs, browptr, val, out);
}

}  // namespace igx
