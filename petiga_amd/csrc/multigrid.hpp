// multigrid.hpp -- the sweeps of the V-cycle (IGXMultigrid: multigrid_host.hpp, behind the transfer it calls).  Included by the main unit only, after
// timestep.hpp, whose sweep discipline it keeps: KR_T threads per workgroup, a grid-stride loop of 16-byte accesses over a grid capped at KR_G
// workgroups, the n & 1 tail in thread 0 of workgroup 0.  None of them emits a sum; no atomics: a cycle is bit-repeatable.
// A Chebyshev step of the smoother between two operator calls is ONE sweep:
//   mg_cheb_first<ZERO>   ZERO: r = b, z = r / D, d = c z, x = d;  otherwise r holds b - A x already: z = r / D, d = c z, x = x + d    (c = 1 / theta)
//   mg_cheb_step          r = r - w, z = r / D, d = c1 d + c2 z, x = x + d      (w = A d; c1 = rho_j rho_{j-1}, c2 = 2 rho_j / delta)
//                         reads r w d D x, writes r d x: 8 doubles per entry where AXPBY, PointwiseDivide, AXPBY, AXPBY move 12
//   mg_resid              r = r - w, or with FROM_B r = b - w: the residual after pre-smoothing and the one before post-smoothing
// With point blocks (PB) the quotient is a product B_node r_node that block_diag.hpp's apply kernel forms between two sweeps: mg_resid, the
// apply (z = B r), then the same kernels with PB set, which read z where the others divide and leave r alone.
// Every product, quotient and sum rounds on its own (contraction switched off, as in ts_w_of), so a host restatement gives the same bits.
// mg_zero_fixed zeroes the rows of the Dirichlet faces, field by field: the grid runs over the nodes of the faces alone.
#pragma once
#include "timestep.hpp"

namespace igx {

#include "kr_sweep_begin.hpp"

__device__ inline double mg_first_of(double q, double D, double c, bool pb) {
#pragma clang fp contract(off)
  const double z = pb ? D : q / D;
  return c * z;
}
__device__ inline double mg_sum_of(double x, double d) {
#pragma clang fp contract(off)
  return x + d;
}
__device__ inline double mg_diff_of(double r, double w) {
#pragma clang fp contract(off)
  return r - w;
}
__device__ inline double mg_d_of(double c1, double d, double c2, double z) {
#pragma clang fp contract(off)
  const double p = c1 * d, q = c2 * z;
  return p + q;
}
__device__ inline double mg_quot_of(double r, double D) {
#pragma clang fp contract(off)
  return r / D;
}

// Dz: the diagonal D, or with PB the vector z = B r
template <bool ZERO, bool PB>
__global__ void __launch_bounds__(KR_T) mg_cheb_first(double *x, double *d, double *r, const double *b, const double *Dz, double c, long long n) {
  KR_PAIRS(i) {
    const kr_d2 q = ZERO ? KR_C2(b)[i] : KR_C2(r)[i], D = KR_C2(Dz)[i];
    const kr_d2 dd = kr_d2{mg_first_of(q.x, D.x, c, PB), mg_first_of(q.y, D.y, c, PB)};
    if (ZERO) { KR_V2(r)[i] = q; KR_V2(x)[i] = dd; }
    else { const kr_d2 xx = KR_C2(x)[i]; KR_V2(x)[i] = kr_d2{mg_sum_of(xx.x, dd.x), mg_sum_of(xx.y, dd.y)}; }
    KR_V2(d)[i] = dd;
  }
  if (KR_TAIL) {
    const long long e = n - 1;
    const double q = ZERO ? b[e] : r[e], dd = mg_first_of(q, Dz[e], c, PB);
    if (ZERO) { r[e] = q; x[e] = dd; } else x[e] = mg_sum_of(x[e], dd);
    d[e] = dd;
  }
}

template <bool PB>
__global__ void __launch_bounds__(KR_T) mg_cheb_step(double *x, double *d, double *r, const double *w, const double *Dz, double c1, double c2, long long n) {
  KR_PAIRS(i) {
    const kr_d2 D = KR_C2(Dz)[i], dd = KR_C2(d)[i], xx = KR_C2(x)[i];
    kr_d2 z;
    if (PB) z = D;
    else {
      const kr_d2 rr = KR_C2(r)[i], ww = KR_C2(w)[i];
      const kr_d2 q = kr_d2{mg_diff_of(rr.x, ww.x), mg_diff_of(rr.y, ww.y)};
      KR_V2(r)[i] = q;
      z = kr_d2{mg_quot_of(q.x, D.x), mg_quot_of(q.y, D.y)};
    }
    const kr_d2 dn = kr_d2{mg_d_of(c1, dd.x, c2, z.x), mg_d_of(c1, dd.y, c2, z.y)};
    KR_V2(d)[i] = dn;
    KR_V2(x)[i] = kr_d2{mg_sum_of(xx.x, dn.x), mg_sum_of(xx.y, dn.y)};
  }
  if (KR_TAIL) {
    const long long e = n - 1;
    double z;
    if (PB) z = Dz[e];
    else { const double q = mg_diff_of(r[e], w[e]); r[e] = q; z = mg_quot_of(q, Dz[e]); }
    const double dn = mg_d_of(c1, d[e], c2, z);
    d[e] = dn; x[e] = mg_sum_of(x[e], dn);
  }
}

template <bool FROM_B>
__global__ void __launch_bounds__(KR_T) mg_resid(double *r, const double *b, const double *w, long long n) {
  KR_PAIRS(i) {
    const kr_d2 q = FROM_B ? KR_C2(b)[i] : KR_C2(r)[i], ww = KR_C2(w)[i];
    KR_V2(r)[i] = kr_d2{mg_diff_of(q.x, ww.x), mg_diff_of(q.y, ww.y)};
  }
  if (KR_TAIL) r[n - 1] = mg_diff_of(FROM_B ? b[n - 1] : r[n - 1], w[n - 1]);
}

#include "kr_sweep_end.hpp"

// The Dirichlet faces of a vector [n2][n1][n0][dof]: face k lies at index at[k] of axis axis[k] and fixes the fields of mask[k].  A node on
// an edge of two fixed faces is zeroed by both: the same store twice.
constexpr int MG_FACE_T = 256;
struct MgFaces { int nface, dof, n[3]; int axis[6], at[6]; unsigned mask[6]; };
__global__ void __launch_bounds__(MG_FACE_T) mg_zero_fixed(double *v, const MgFaces F) {
  const int k = blockIdx.y, ax = F.axis[k];
  const int a = ax == 0 ? 1 : 0, b = ax == 2 ? 1 : 2;      // the two axes of the face, a the faster one
  const long long na = F.n[a], count = na * F.n[b];
  for (long long i = (long long)blockIdx.x * MG_FACE_T + threadIdx.x; i < count; i += (long long)gridDim.x * MG_FACE_T) {
    long long idx[3];
    idx[a] = i % na; idx[b] = i / na; idx[ax] = F.at[k];
    double *row = v + ((idx[2] * F.n[1] + idx[1]) * F.n[0] + idx[0]) * F.dof;
    for (int f = 0; f < F.dof; ++f) if (F.mask[k] >> f & 1u) row[f] = 0.0;
  }
}

}  // namespace igx
