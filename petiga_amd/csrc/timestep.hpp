// timestep.hpp -- the sweeps of the device-resident generalized-alpha time loop (IGXTimeStep: engine.hip, beside IGXSolveNonlinear).  Included by
// the main unit only, after newton.hpp, whose sweep discipline it keeps: KR_T threads per workgroup, a grid-stride loop of 16-byte accesses over
// KR_G workgroups, the n & 1 tail in thread 0 of workgroup 0, one partial per workgroup and slab in a fixed tree, the slabs added in index order
// by kr_record.  No atomics: the trial state and both sums are bit-repeatable.
// Around one Newton solve an attempt is TWO sweeps:
//   ts_stage    W = c0 V0 - a U0 and the stage guess x = U0
//   ts_update   U1 = U0 + c1 (x - U0), V1 = c2 (U1 - U0) + c3 V0, the partials of U1 . U1 and, with an estimate, of the weighted error
// Every product and every sum rounds on its own (contraction switched off, as in nw_state_of), so a host restatement gives the same bits.
#pragma once
#include "newton.hpp"

namespace igx {

#include "kr_sweep_begin.hpp"

// the constants of one attempt, formed on the host in double
struct TsUpdate {
  double c1, c2, c3;          // 1 / alpha_f, 1 / (gamma h), 1 - 1 / gamma
  double d1, d2, d3;          // r, r - 1, r (r - 1) with r = 1 + h_{n-1} / h: the divisors of the backward-difference estimate
  double atol, rtol;
};

__device__ inline double ts_w_of(double c0, double v, double a, double u) {
#pragma clang fp contract(off)
  const double p = c0 * v, q = a * u;
  return p - q;
}
__device__ inline double ts_u1_of(double c1, double x, double u) {
#pragma clang fp contract(off)
  const double d = x - u, p = c1 * d;
  return u + p;
}
__device__ inline double ts_v1_of(double c2, double c3, double u1, double u, double v) {
#pragma clang fp contract(off)
  const double d = u1 - u, p = c2 * d, q = c3 * v;
  return p + q;
}
// e / (atol + rtol max(|U1|, |U1 + e|)) with e = U1 / r - U0 / (r - 1) + Uprev / (r (r - 1)): three rounded quotients added left to right
__device__ inline double ts_err_of(const TsUpdate &k, double u1, double u, double up) {
#pragma clang fp contract(off)
  const double q1 = u1 / k.d1, q2 = u / k.d2, q3 = up / k.d3;
  const double s = q1 - q2, e = s + q3;
  const double y = u1 + e, m = fmax(fabs(u1), fabs(y));
  const double p = k.rtol * m, tol = k.atol + p;
  return e / tol;
}

// W = c0 V0 - a U0, x = U0
__global__ void __launch_bounds__(KR_T) ts_stage(double *W, double *x, const double *U0, const double *V0, double c0, double a, long long n) {
  KR_PAIRS(i) {
    const kr_d2 u = KR_C2(U0)[i], v = KR_C2(V0)[i];
    KR_V2(W)[i] = kr_d2{ts_w_of(c0, v.x, a, u.x), ts_w_of(c0, v.y, a, u.y)};
    KR_V2(x)[i] = u;
  }
  if (KR_TAIL) { const double u = U0[n - 1]; W[n - 1] = ts_w_of(c0, V0[n - 1], a, u); x[n - 1] = u; }
}

// the trial state from the stage solution x, slab_uu = U1 . U1 and, with ESTIMATE, slab_ee = sum (e / tol)^2 (otherwise slab_ee = 0)
template <bool ESTIMATE>
__global__ void __launch_bounds__(KR_T) ts_update(double *U1, double *V1, const double *x, const double *U0, const double *V0, const double *Uprev, const TsUpdate k, long long n,
                                                  double *slab_uu, double *slab_ee) {
  __shared__ double red[KR_T / 64];
  double uu = 0.0, ee = 0.0;
  KR_PAIRS(i) {
    const kr_d2 s = KR_C2(x)[i], u = KR_C2(U0)[i], v = KR_C2(V0)[i];
    const kr_d2 u1 = kr_d2{ts_u1_of(k.c1, s.x, u.x), ts_u1_of(k.c1, s.y, u.y)};
    KR_V2(U1)[i] = u1;
    KR_V2(V1)[i] = kr_d2{ts_v1_of(k.c2, k.c3, u1.x, u.x, v.x), ts_v1_of(k.c2, k.c3, u1.y, u.y, v.y)};
    uu += u1.x * u1.x; uu += u1.y * u1.y;
    if (ESTIMATE) {
      const kr_d2 up = KR_C2(Uprev)[i];
      const double qx = ts_err_of(k, u1.x, u.x, up.x), qy = ts_err_of(k, u1.y, u.y, up.y);
      ee += qx * qx; ee += qy * qy;
    }
  }
  if (KR_TAIL) {
    const double u = U0[n - 1], u1 = ts_u1_of(k.c1, x[n - 1], u);
    U1[n - 1] = u1;
    V1[n - 1] = ts_v1_of(k.c2, k.c3, u1, u, V0[n - 1]);
    uu += u1 * u1;
    if (ESTIMATE) { const double q = ts_err_of(k, u1, u, Uprev[n - 1]); ee += q * q; }
  }
  uu = kr_block_sum(uu, red); ee = kr_block_sum(ee, red);
  if (threadIdx.x == 0) { slab_uu[blockIdx.x] = uu; slab_ee[blockIdx.x] = ee; }
}

#include "kr_sweep_end.hpp"

}  // namespace igx
