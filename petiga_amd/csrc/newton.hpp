// newton.hpp -- the sweeps of the device-resident Newton loop (IGXSolveNonlinear: engine.hip, beside IGXSolve).  Included by the main unit
// only, after krylov.hpp, whose sweep discipline it keeps: KR_T threads per workgroup, a grid-stride loop of 16-byte accesses over KR_G
// workgroups, the n & 1 tail in thread 0 of workgroup 0, one partial per workgroup and slab in a fixed tree, the slabs added in index order by
// kr_record.  No atomics: the trial iterate and both sums are bit-repeatable.
// Between two operator calls a trial is ONE sweep: the saved copy, the step, the state V of an IFunction and the partials of d.d and x.x.
//   x - lambda d   lambda is a power of two, so lambda d is exact and the difference rounds once with or without contraction
//   a x + W        the rounded product plus W, formed with contraction switched off, so a host restatement gives the same bits
#pragma once
#include "krylov.hpp"

namespace igx {

#include "kr_sweep_begin.hpp"

// (hipcc's __dmul_rn / __dadd_rn are plain operators and contract into an FMA like any others: the pragma is what keeps the two roundings)
__device__ inline double nw_state_of(double a, double x, double w) {
#pragma clang fp contract(off)
  const double p = a * x;
  return p + w;
}

// V = a x + W: the state of the first residual
__global__ void __launch_bounds__(KR_T) nw_state(double *V, const double *x, const double *W, double a, long long n) {
  KR_PAIRS(i) { const kr_d2 u = KR_C2(x)[i], w = KR_C2(W)[i]; KR_V2(V)[i] = kr_d2{nw_state_of(a, u.x, w.x), nw_state_of(a, u.y, w.y)}; }
  if (KR_TAIL) V[n - 1] = nw_state_of(a, x[n - 1], W[n - 1]);
}

// FIRST: xs = x (the accepted iterate), x = xs - d.  Otherwise: x = xs - lambda d from the saved copy, which is left alone.
// Both: V = a x + W where V is given, slab_dd = d . d, slab_xx = x . x of the trial.
template <bool FIRST>
__device__ inline void nw_trial(double *x, double *xs, const double *d, double *V, const double *W, double a, double lambda, long long n, double *slab_dd, double *slab_xx, double *red) {
  double dd = 0.0, xx = 0.0;
  KR_PAIRS(i) {
    const kr_d2 s = FIRST ? KR_C2(x)[i] : KR_C2(xs)[i], e = KR_C2(d)[i];
    const kr_d2 q = FIRST ? kr_d2{s.x - e.x, s.y - e.y} : kr_d2{s.x - lambda * e.x, s.y - lambda * e.y};
    if (FIRST) KR_V2(xs)[i] = s;
    KR_V2(x)[i] = q;
    if (V) { const kr_d2 w = KR_C2(W)[i]; KR_V2(V)[i] = kr_d2{nw_state_of(a, q.x, w.x), nw_state_of(a, q.y, w.y)}; }
    dd += e.x * e.x; dd += e.y * e.y; xx += q.x * q.x; xx += q.y * q.y;
  }
  if (KR_TAIL) {
    const double s = FIRST ? x[n - 1] : xs[n - 1], e = d[n - 1], q = FIRST ? s - e : s - lambda * e;
    if (FIRST) xs[n - 1] = s;
    x[n - 1] = q;
    if (V) V[n - 1] = nw_state_of(a, q, W[n - 1]);
    dd += e * e; xx += q * q;
  }
  dd = kr_block_sum(dd, red); xx = kr_block_sum(xx, red);
  if (threadIdx.x == 0) { slab_dd[blockIdx.x] = dd; slab_xx[blockIdx.x] = xx; }
}
__global__ void __launch_bounds__(KR_T) nw_first_trial(double *x, double *xs, const double *d, double *V, const double *W, double a, long long n, double *slab_dd, double *slab_xx) {
  __shared__ double red[KR_T / 64];
  nw_trial<true>(x, xs, d, V, W, a, 1.0, n, slab_dd, slab_xx, red);
}
__global__ void __launch_bounds__(KR_T) nw_back_trial(double *x, const double *xs, const double *d, double *V, const double *W, double a, double lambda, long long n, double *slab_dd, double *slab_xx) {
  __shared__ double red[KR_T / 64];
  nw_trial<false>(x, const_cast<double *>(xs), d, V, W, a, lambda, n, slab_dd, slab_xx, red);
}

#include "kr_sweep_end.hpp"

}  // namespace igx
