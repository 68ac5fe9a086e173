// krylov.hpp -- vector algebra on IGXVec (IGXVecSet ... IGXVecNorm2) and the device-resident Krylov loop (IGXSolve: CG and right-preconditioned
// BiCGStab over IGXCompute*Action and the diagonal / point-block / fast-diagonalisation preconditioners).  Included by the main unit only,
// after the drivers it calls.  The sweep macros (KR_PAIRS ... KR_C2) live between kr_sweep_begin.hpp and kr_sweep_end.hpp, here and in newton.hpp.
// Sweeps: KR_T threads per workgroup, a grid-stride loop over a grid capped at KR_G workgroups, 16-byte accesses (every IGXVec starts at its
// allocation, so the pairs are aligned) and a scalar tail of n & 1 entries in thread 0 of workgroup 0.  On a partition the sweeps of the two
// loops run over the rows the rank owns instead: runs of contiguous doubles at a constant stride (KrRuns, KR_RUN_SWEEP; the end of this file).
// Reductions: a kernel that emits a sum always runs KR_G workgroups; each adds its lanes in a fixed tree (wavefront shuffles, then LDS in wave
// order) and stores ONE partial into a slab of KR_G doubles (an idle workgroup stores 0).  The slab is added in index order at the launch
// boundary: by the prologue of the kernel that consumes the scalar (every thread adds the KR_G partials itself: uniform addresses, one chain
// of KR_G additions) or by the one-workgroup record kernel when the host wants the number.  No atomics, no in-launch hand-off: bit-repeatable.
// alpha, beta and omega never leave the device; the host reads one record per iteration (kr_record / kr_bicg_record) for the stop test.
// A kernel that would divide by a zero or non-finite denominator leaves x and r as they are: the host sees the denominator in the record and
// reports the breakdown, and x stays the iterate whose norm was tested.
#pragma once
#include <hip/hip_runtime.h>
#include "igx.hpp"

namespace igx {

constexpr int KR_G = 256;          // workgroups of a sweep at the most, and partials per slab
constexpr int KR_T = 512;          // threads per workgroup (8 wavefronts)
// slabs of the scalar buffer (KR_G doubles each), then KR_NREC doubles of record and 4 of BiCGStab's scalars (rho, alpha, omega of the last iteration)
enum { KS_RR = 0, KS_BB, KS_A, KS_B, KS_C, KS_D, KS_E, KS_USER, KR_NSLAB };
constexpr int KR_NREC = 8;
constexpr size_t KR_SCAL_DOUBLES = (size_t)KR_NSLAB * KR_G + KR_NREC + 4;

typedef double kr_d2 __attribute__((ext_vector_type(2)));

__device__ inline bool kr_bad(double d) { return !(fabs(d) > 0.0) || !(fabs(d) <= 1.79769313486231570e308); }      // zero, NaN or infinite
__device__ inline double kr_slab_sum(const double *s) { double a = 0.0; for (int i = 0; i < KR_G; ++i) a += s[i]; return a; }
// this workgroup's sum of v in thread 0: __shfl_down over the 64 lanes, then the 8 wavefronts' sums in wave order
__device__ inline double kr_block_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) { s = red[0]; for (int w = 1; w < KR_T / 64; ++w) s += red[w]; }
  __syncthreads();
  return s;
}
#include "kr_sweep_begin.hpp"

// ------------------------------------------------------------------ vector algebra
__global__ void __launch_bounds__(KR_T) kr_set(double *y, double v, long long n) {
  KR_PAIRS(i) KR_V2(y)[i] = kr_d2{v, v};
  if (KR_TAIL) y[n - 1] = v;
}
__global__ void __launch_bounds__(KR_T) kr_scale(double *y, double a, long long n) {
  KR_PAIRS(i) { const kr_d2 v = KR_C2(y)[i]; KR_V2(y)[i] = kr_d2{a * v.x, a * v.y}; }
  if (KR_TAIL) y[n - 1] = a * y[n - 1];
}
// y = a x + b y; b == 0: y = a x whatever y held
__global__ void __launch_bounds__(KR_T) kr_axpby(double *y, double a, const double *x, double b, long long n) {
  if (b == 0.0) {
    KR_PAIRS(i) { const kr_d2 u = KR_C2(x)[i]; KR_V2(y)[i] = kr_d2{a * u.x, a * u.y}; }
    if (KR_TAIL) y[n - 1] = a * x[n - 1];
  } else {
    KR_PAIRS(i) { const kr_d2 u = KR_C2(x)[i], v = KR_C2(y)[i]; KR_V2(y)[i] = kr_d2{a * u.x + b * v.x, a * u.y + b * v.y}; }
    if (KR_TAIL) y[n - 1] = a * x[n - 1] + b * y[n - 1];
  }
}
__global__ void __launch_bounds__(KR_T) kr_pdiv(double *z, const double *x, const double *d, long long n) {
  KR_PAIRS(i) { const kr_d2 u = KR_C2(x)[i], v = KR_C2(d)[i]; KR_V2(z)[i] = kr_d2{u.x / v.x, u.y / v.y}; }
  if (KR_TAIL) z[n - 1] = x[n - 1] / d[n - 1];
}
// slab[workgroup] = this workgroup's part of x . y
__global__ void __launch_bounds__(KR_T) kr_dot(const double *x, const double *y, long long n, double *slab) {
  __shared__ double red[KR_T / 64];
  double s = 0.0;
  KR_PAIRS(i) { const kr_d2 u = KR_C2(x)[i], v = KR_C2(y)[i]; s += u.x * v.x; s += u.y * v.y; }
  if (KR_TAIL) s += x[n - 1] * y[n - 1];
  s = kr_block_sum(s, red);
  if (threadIdx.x == 0) slab[blockIdx.x] = s;
}
// ... over the owned rows of a rank that holds ghosts: a prefix (nown0, nown1, nown2) of the row box (nrow0, nrow1, .), bs entries per row
__global__ void __launch_bounds__(KR_T) kr_dot_owned(const double *x, const double *y, int nown0, int nown1, int nown2, int nrow0, int nrow1, int bs, double *slab) {
  __shared__ double red[KR_T / 64];
  const long long nown = (long long)nown0 * nown1 * nown2 * bs;
  double s = 0.0;
  for (long long k = (long long)blockIdx.x * KR_T + threadIdx.x; k < nown; k += (long long)gridDim.x * KR_T) {
    const long long node = k / bs; const int f = (int)(k % bs);
    const int r0 = (int)(node % nown0), r1 = (int)((node / nown0) % nown1), r2 = (int)(node / ((long long)nown0 * nown1));
    const long long e = ((long long)r0 + (long long)nrow0 * ((long long)r1 + (long long)nrow1 * r2)) * bs + f;
    s += x[e] * y[e];
  }
  s = kr_block_sum(s, red);
  if (threadIdx.x == 0) slab[blockIdx.x] = s;
}
// slab_a = t . s, slab_b = t . t
__global__ void __launch_bounds__(KR_T) kr_dot2(const double *t, const double *s, long long n, double *slab_a, double *slab_b) {
  __shared__ double red[KR_T / 64];
  double a = 0.0, b = 0.0;
  KR_PAIRS(i) { const kr_d2 u = KR_C2(t)[i], v = KR_C2(s)[i]; a += u.x * v.x; a += u.y * v.y; b += u.x * u.x; b += u.y * u.y; }
  if (KR_TAIL) { a += t[n - 1] * s[n - 1]; b += t[n - 1] * t[n - 1]; }
  a = kr_block_sum(a, red); b = kr_block_sum(b, red);
  if (threadIdx.x == 0) { slab_a[blockIdx.x] = a; slab_b[blockIdx.x] = b; }
}
// the finishing kernel: rec[j] = the sum of slab j in index order, j < m (one workgroup, thread j)
struct KrSlabs { const double *s[KR_NREC]; int m; };
__global__ void __launch_bounds__(64) kr_record(const KrSlabs a, double *rec) {
  if ((int)threadIdx.x < a.m) rec[threadIdx.x] = kr_slab_sum(a.s[threadIdx.x]);
}

// ------------------------------------------------------------------ both methods: r = b - w, with r . r and b . b
__global__ void __launch_bounds__(KR_T) kr_resid0(double *r, const double *b, const double *w, long long n, double *slab_rr, double *slab_bb) {
  __shared__ double red[KR_T / 64];
  double rr = 0.0, bb = 0.0;
  KR_PAIRS(i) {
    const kr_d2 u = KR_C2(b)[i], v = KR_C2(w)[i]; const kr_d2 q = kr_d2{u.x - v.x, u.y - v.y};
    KR_V2(r)[i] = q; rr += q.x * q.x; rr += q.y * q.y; bb += u.x * u.x; bb += u.y * u.y;
  }
  if (KR_TAIL) { const double u = b[n - 1], q = u - w[n - 1]; r[n - 1] = q; rr += q * q; bb += u * u; }
  rr = kr_block_sum(rr, red); bb = kr_block_sum(bb, red);
  if (threadIdx.x == 0) { slab_rr[blockIdx.x] = rr; slab_bb[blockIdx.x] = bb; }
}

// ------------------------------------------------------------------ CG
// alpha = r.z / p.Ap from the two slabs; x += alpha p; r -= alpha Ap; r . r
__global__ void __launch_bounds__(KR_T) kr_cg_update(double *x, double *r, const double *p, const double *Ap, long long n, const double *slab_pAp, const double *slab_rz, double *slab_rr) {
  __shared__ double red[KR_T / 64];
  const double pAp = kr_slab_sum(slab_pAp), rz = kr_slab_sum(slab_rz);
  const bool skip = !(pAp > 0.0) || kr_bad(pAp) || kr_bad(rz);
  const double alpha = skip ? 0.0 : rz / pAp;
  double rr = 0.0;
  if (skip) {
    KR_PAIRS(i) { const kr_d2 q = KR_C2(r)[i]; rr += q.x * q.x; rr += q.y * q.y; }
    if (KR_TAIL) rr += r[n - 1] * r[n - 1];
  } else {
    KR_PAIRS(i) {
      const kr_d2 u = KR_C2(p)[i], v = KR_C2(Ap)[i]; kr_d2 xx = KR_C2(x)[i], q = KR_C2(r)[i];
      xx.x += alpha * u.x; xx.y += alpha * u.y; q.x -= alpha * v.x; q.y -= alpha * v.y;
      KR_V2(x)[i] = xx; KR_V2(r)[i] = q; rr += q.x * q.x; rr += q.y * q.y;
    }
    if (KR_TAIL) { x[n - 1] += alpha * p[n - 1]; const double q = r[n - 1] - alpha * Ap[n - 1]; r[n - 1] = q; rr += q * q; }
  }
  rr = kr_block_sum(rr, red);
  if (threadIdx.x == 0) slab_rr[blockIdx.x] = rr;
}
// z = r ./ D; r . z
__global__ void __launch_bounds__(KR_T) kr_jacobi_rz(double *z, const double *r, const double *D, long long n, double *slab_rz) {
  __shared__ double red[KR_T / 64];
  double s = 0.0;
  KR_PAIRS(i) { const kr_d2 u = KR_C2(r)[i], d = KR_C2(D)[i]; const kr_d2 q = kr_d2{u.x / d.x, u.y / d.y}; KR_V2(z)[i] = q; s += u.x * q.x; s += u.y * q.y; }
  if (KR_TAIL) { const double q = r[n - 1] / D[n - 1]; z[n - 1] = q; s += r[n - 1] * q; }
  s = kr_block_sum(s, red);
  if (threadIdx.x == 0) slab_rz[blockIdx.x] = s;
}
// beta = r.z / (r.z of the iteration before); p = z + beta p
__global__ void __launch_bounds__(KR_T) kr_cg_p(double *p, const double *z, long long n, const double *slab_new, const double *slab_old) {
  const double beta = kr_slab_sum(slab_new) / kr_slab_sum(slab_old);
  KR_PAIRS(i) { const kr_d2 u = KR_C2(z)[i], v = KR_C2(p)[i]; KR_V2(p)[i] = kr_d2{u.x + beta * v.x, u.y + beta * v.y}; }
  if (KR_TAIL) p[n - 1] = z[n - 1] + beta * p[n - 1];
}

// ------------------------------------------------------------------ BiCGStab; sc = (rho, alpha, omega) of the iteration before
// beta = (rho' / rho) (alpha / omega); p = r + beta (p - omega v)
__global__ void __launch_bounds__(KR_T) kr_bicg_p(double *p, const double *r, const double *v, long long n, const double *slab_rho, const double *sc) {
  const double rho1 = kr_slab_sum(slab_rho), omega = sc[2];
  const double beta = (rho1 / sc[0]) * (sc[1] / omega);
  KR_PAIRS(i) { const kr_d2 a = KR_C2(r)[i], b = KR_C2(p)[i], c = KR_C2(v)[i]; KR_V2(p)[i] = kr_d2{a.x + beta * (b.x - omega * c.x), a.y + beta * (b.y - omega * c.y)}; }
  if (KR_TAIL) p[n - 1] = r[n - 1] + beta * (p[n - 1] - omega * v[n - 1]);
}
// alpha = rho' / rhat.v; s = r - alpha v
__global__ void __launch_bounds__(KR_T) kr_bicg_s(double *s, const double *r, const double *v, long long n, const double *slab_rho, const double *slab_rhatv) {
  const double alpha = kr_slab_sum(slab_rho) / kr_slab_sum(slab_rhatv);
  KR_PAIRS(i) { const kr_d2 a = KR_C2(r)[i], c = KR_C2(v)[i]; KR_V2(s)[i] = kr_d2{a.x - alpha * c.x, a.y - alpha * c.y}; }
  if (KR_TAIL) s[n - 1] = r[n - 1] - alpha * v[n - 1];
}
// omega = t.s / t.t; x += alpha y + omega z; r = s - omega t; r . r and rhat . r (the next rho')
__global__ void __launch_bounds__(KR_T) kr_bicg_xr(double *x, double *r, const double *y, const double *z, const double *s, const double *t, const double *rhat, long long n,
                                                   const double *slab_rho, const double *slab_rhatv, const double *slab_ts, const double *slab_tt, double *slab_rr, double *slab_rho_next) {
  __shared__ double red[KR_T / 64];
  const double rhatv = kr_slab_sum(slab_rhatv), tt = kr_slab_sum(slab_tt);
  const bool skip = kr_bad(rhatv) || kr_bad(tt);
  const double alpha = skip ? 0.0 : kr_slab_sum(slab_rho) / rhatv, omega = skip ? 0.0 : kr_slab_sum(slab_ts) / tt;
  double rr = 0.0, rh = 0.0;
  if (skip) {
    KR_PAIRS(i) { const kr_d2 q = KR_C2(r)[i], h = KR_C2(rhat)[i]; rr += q.x * q.x; rr += q.y * q.y; rh += h.x * q.x; rh += h.y * q.y; }
    if (KR_TAIL) { rr += r[n - 1] * r[n - 1]; rh += rhat[n - 1] * r[n - 1]; }
  } else {
    KR_PAIRS(i) {
      const kr_d2 a = KR_C2(y)[i], b = KR_C2(z)[i], c = KR_C2(s)[i], d = KR_C2(t)[i], h = KR_C2(rhat)[i]; kr_d2 xx = KR_C2(x)[i];
      xx.x += alpha * a.x + omega * b.x; xx.y += alpha * a.y + omega * b.y;
      const kr_d2 q = kr_d2{c.x - omega * d.x, c.y - omega * d.y};
      KR_V2(x)[i] = xx; KR_V2(r)[i] = q; rr += q.x * q.x; rr += q.y * q.y; rh += h.x * q.x; rh += h.y * q.y;
    }
    if (KR_TAIL) { x[n - 1] += alpha * y[n - 1] + omega * z[n - 1]; const double q = s[n - 1] - omega * t[n - 1]; r[n - 1] = q; rr += q * q; rh += rhat[n - 1] * q; }
  }
  rr = kr_block_sum(rr, red); rh = kr_block_sum(rh, red);
  if (threadIdx.x == 0) { slab_rr[blockIdx.x] = rr; slab_rho_next[blockIdx.x] = rh; }
}
// the iteration's record (r.r, rhat.v, t.t, t.s, the next rho', alpha, omega) and the scalars the next iteration's kernels read
__global__ void __launch_bounds__(64) kr_bicg_record(const double *slab_rr, const double *slab_rho, const double *slab_rhatv, const double *slab_ts, const double *slab_tt, const double *slab_rho_next, double *rec, double *sc) {
  if (threadIdx.x != 0) return;
  const double rho1 = kr_slab_sum(slab_rho), rhatv = kr_slab_sum(slab_rhatv), ts = kr_slab_sum(slab_ts), tt = kr_slab_sum(slab_tt);
  const bool skip = kr_bad(rhatv) || kr_bad(tt);
  const double alpha = skip ? 0.0 : rho1 / rhatv, omega = skip ? 0.0 : ts / tt;
  rec[0] = kr_slab_sum(slab_rr); rec[1] = rhatv; rec[2] = tt; rec[3] = ts; rec[4] = kr_slab_sum(slab_rho_next); rec[5] = alpha; rec[6] = omega;
  sc[0] = rho1; sc[1] = alpha; sc[2] = omega;
}

// ------------------------------------------------------------------ the sweeps of the two loops over the owned rows of a rank with ghosts
// The rows a rank owns are a prefix box (nown0, nown1, nown2) of its row box (nrow0, nrow1, .): with the leading axes the rank holds whole
// collapsed, the owned entries are runs of len contiguous doubles -- one run when only axis 2 is cut, runs of bs nrow0 nown1 when axis 1
// is cut too, runs of bs nown0 when axis 0 is.  KR_RUN_SWEEP (kr_sweep_begin.hpp) walks them; a kernel below states its arithmetic once, as
// a lambda over the width of the access (an aligned pair inside a run, one entry at its ends), and has the name and the prologue of its
// contiguous sibling above.  A one-rank solve launches the siblings; a partitioned one these, on every rank, the top one with its one run.
struct KrRuns { long long len, s1, s2; int n1, n2; };
inline KrRuns kr_runs(const int nown[3], int nrow0, int nrow1, int bs) {
  KrRuns r;
  if (nown[0] == nrow0 && nown[1] == nrow1) r = KrRuns{(long long)bs * nrow0 * nrow1 * nown[2], 0, 0, 1, 1};
  else if (nown[0] == nrow0) r = KrRuns{(long long)bs * nrow0 * nown[1], (long long)bs * nrow0 * nrow1, 0, nown[2], 1};
  else r = KrRuns{(long long)bs * nown[0], (long long)bs * nrow0, (long long)bs * nrow0 * nrow1, nown[1], nown[2]};
  if (r.len <= 0 || r.n1 <= 0) { r.len = 0; r.n1 = 1; r.n2 = 0; }      // a rank that owns nothing: no run
  return r;
}
// workgroups of a run sweep that emits no sum: one pass of its (run, chunk) items, KR_G at the most
inline unsigned kr_run_grid(const KrRuns &r) {
  const long long half = r.len >> 1, items = (half > 0 ? (half + 63) >> 6 : 1) * r.n1 * r.n2, w = (items + KR_T / 64 - 1) / (KR_T / 64);
  return (unsigned)(w < 1 ? 1 : (w > KR_G ? KR_G : w));
}
template <class T> __device__ inline T kr_ld(const double *p, long long e) { return *reinterpret_cast<const T *>(p + e); }
template <class T> __device__ inline void kr_st(double *p, long long e, T v) { *reinterpret_cast<T *>(p + e) = v; }
__device__ inline void kr_acc(double &s, double u, double v) { s += u * v; }
__device__ inline void kr_acc(double &s, kr_d2 u, kr_d2 v) { s += u.x * v.x; s += u.y * v.y; }
__device__ inline double kr_fill(double, double v) { return v; }      // v in the width of the first argument, bit for bit (-0.0 stays -0.0)
__device__ inline kr_d2 kr_fill(kr_d2, double v) { return kr_d2{v, v}; }
// Every kernel below restates the prologue (the skip conditions, alpha, beta, omega) and the arithmetic of the contiguous kernel of the same
// name above, which keeps its own text so that a one-rank solve stays bit for bit what it was: a change to one of a pair is a change to both.

__global__ void __launch_bounds__(KR_T) kr_set_runs(const KrRuns rn, double *y, double v) {
  auto body = [&](auto w, long long e) { typedef decltype(w) T; kr_st<T>(y, e, kr_fill(w, v)); };
  KR_RUN_SWEEP(rn, body);
}
__global__ void __launch_bounds__(KR_T) kr_pdiv_runs(const KrRuns rn, double *z, const double *x, const double *d) {
  auto body = [&](auto w, long long e) { typedef decltype(w) T; kr_st<T>(z, e, kr_ld<T>(x, e) / kr_ld<T>(d, e)); };
  KR_RUN_SWEEP(rn, body);
}
__global__ void __launch_bounds__(KR_T) kr_dot_runs(const KrRuns rn, const double *x, const double *y, double *slab) {
  __shared__ double red[KR_T / 64];
  double s = 0.0;
  auto body = [&](auto w, long long e) { typedef decltype(w) T; kr_acc(s, kr_ld<T>(x, e), kr_ld<T>(y, e)); };
  KR_RUN_SWEEP(rn, body);
  s = kr_block_sum(s, red);
  if (threadIdx.x == 0) slab[blockIdx.x] = s;
}
__global__ void __launch_bounds__(KR_T) kr_dot2_runs(const KrRuns rn, const double *t, const double *s, double *slab_a, double *slab_b) {
  __shared__ double red[KR_T / 64];
  double a = 0.0, b = 0.0;
  auto body = [&](auto w, long long e) { typedef decltype(w) T; const T u = kr_ld<T>(t, e); kr_acc(a, u, kr_ld<T>(s, e)); kr_acc(b, u, u); };
  KR_RUN_SWEEP(rn, body);
  a = kr_block_sum(a, red); b = kr_block_sum(b, red);
  if (threadIdx.x == 0) { slab_a[blockIdx.x] = a; slab_b[blockIdx.x] = b; }
}
__global__ void __launch_bounds__(KR_T) kr_resid0_runs(const KrRuns rn, double *r, const double *b, const double *w_, double *slab_rr, double *slab_bb) {
  __shared__ double red[KR_T / 64];
  double rr = 0.0, bb = 0.0;
  auto body = [&](auto w, long long e) { typedef decltype(w) T; const T u = kr_ld<T>(b, e), q = u - kr_ld<T>(w_, e); kr_st<T>(r, e, q); kr_acc(rr, q, q); kr_acc(bb, u, u); };
  KR_RUN_SWEEP(rn, body);
  rr = kr_block_sum(rr, red); bb = kr_block_sum(bb, red);
  if (threadIdx.x == 0) { slab_rr[blockIdx.x] = rr; slab_bb[blockIdx.x] = bb; }
}
__global__ void __launch_bounds__(KR_T) kr_cg_update_runs(const KrRuns rn, double *x, double *r, const double *p, const double *Ap, const double *slab_pAp, const double *slab_rz, double *slab_rr) {
  __shared__ double red[KR_T / 64];
  const double pAp = kr_slab_sum(slab_pAp), rz = kr_slab_sum(slab_rz);
  const bool skip = !(pAp > 0.0) || kr_bad(pAp) || kr_bad(rz);
  const double alpha = skip ? 0.0 : rz / pAp;
  double rr = 0.0;
  auto body = [&](auto w, long long e) {
    typedef decltype(w) T;
    T q = kr_ld<T>(r, e);
    if (!skip) { kr_st<T>(x, e, kr_ld<T>(x, e) + alpha * kr_ld<T>(p, e)); q -= alpha * kr_ld<T>(Ap, e); kr_st<T>(r, e, q); }
    kr_acc(rr, q, q);
  };
  KR_RUN_SWEEP(rn, body);
  rr = kr_block_sum(rr, red);
  if (threadIdx.x == 0) slab_rr[blockIdx.x] = rr;
}
__global__ void __launch_bounds__(KR_T) kr_jacobi_rz_runs(const KrRuns rn, double *z, const double *r, const double *D, double *slab_rz) {
  __shared__ double red[KR_T / 64];
  double s = 0.0;
  auto body = [&](auto w, long long e) { typedef decltype(w) T; const T u = kr_ld<T>(r, e), q = u / kr_ld<T>(D, e); kr_st<T>(z, e, q); kr_acc(s, u, q); };
  KR_RUN_SWEEP(rn, body);
  s = kr_block_sum(s, red);
  if (threadIdx.x == 0) slab_rz[blockIdx.x] = s;
}
__global__ void __launch_bounds__(KR_T) kr_cg_p_runs(const KrRuns rn, double *p, const double *z, const double *slab_new, const double *slab_old) {
  const double beta = kr_slab_sum(slab_new) / kr_slab_sum(slab_old);
  auto body = [&](auto w, long long e) { typedef decltype(w) T; kr_st<T>(p, e, kr_ld<T>(z, e) + beta * kr_ld<T>(p, e)); };
  KR_RUN_SWEEP(rn, body);
}
__global__ void __launch_bounds__(KR_T) kr_bicg_p_runs(const KrRuns rn, double *p, const double *r, const double *v, const double *slab_rho, const double *sc) {
  const double rho1 = kr_slab_sum(slab_rho), omega = sc[2];
  const double beta = (rho1 / sc[0]) * (sc[1] / omega);
  auto body = [&](auto w, long long e) { typedef decltype(w) T; kr_st<T>(p, e, kr_ld<T>(r, e) + beta * (kr_ld<T>(p, e) - omega * kr_ld<T>(v, e))); };
  KR_RUN_SWEEP(rn, body);
}
__global__ void __launch_bounds__(KR_T) kr_bicg_s_runs(const KrRuns rn, double *s, const double *r, const double *v, const double *slab_rho, const double *slab_rhatv) {
  const double alpha = kr_slab_sum(slab_rho) / kr_slab_sum(slab_rhatv);
  auto body = [&](auto w, long long e) { typedef decltype(w) T; kr_st<T>(s, e, kr_ld<T>(r, e) - alpha * kr_ld<T>(v, e)); };
  KR_RUN_SWEEP(rn, body);
}
__global__ void __launch_bounds__(KR_T) kr_bicg_xr_runs(const KrRuns rn, double *x, double *r, const double *y, const double *z, const double *s, const double *t, const double *rhat,
                                                        const double *slab_rho, const double *slab_rhatv, const double *slab_ts, const double *slab_tt, double *slab_rr, double *slab_rho_next) {
  __shared__ double red[KR_T / 64];
  const double rhatv = kr_slab_sum(slab_rhatv), tt = kr_slab_sum(slab_tt);
  const bool skip = kr_bad(rhatv) || kr_bad(tt);
  const double alpha = skip ? 0.0 : kr_slab_sum(slab_rho) / rhatv, omega = skip ? 0.0 : kr_slab_sum(slab_ts) / tt;
  double rr = 0.0, rh = 0.0;
  auto body = [&](auto w, long long e) {
    typedef decltype(w) T;
    T q;
    if (skip) q = kr_ld<T>(r, e);
    else {
      kr_st<T>(x, e, kr_ld<T>(x, e) + (alpha * kr_ld<T>(y, e) + omega * kr_ld<T>(z, e)));
      q = kr_ld<T>(s, e) - omega * kr_ld<T>(t, e);
      kr_st<T>(r, e, q);
    }
    kr_acc(rr, q, q); kr_acc(rh, kr_ld<T>(rhat, e), q);
  };
  KR_RUN_SWEEP(rn, body);
  rr = kr_block_sum(rr, red); rh = kr_block_sum(rh, red);
  if (threadIdx.x == 0) { slab_rr[blockIdx.x] = rr; slab_rho_next[blockIdx.x] = rh; }
}

#include "kr_sweep_end.hpp"

// workgroups of a sweep that emits no sum: one pass of pairs, KR_G at the most
inline unsigned kr_grid(long long n) { const long long w = ((n >> 1) + KR_T - 1) / KR_T; return (unsigned)(w < 1 ? 1 : (w > KR_G ? KR_G : w)); }

}  // namespace igx
