// probe.hpp -- evaluation of a discrete field at arbitrary parametric points (IGXProbe: IGAProbe, src/petigaprobe.c).  Included by the main
// unit only, after the drivers.
// probe_locate: one lane per point, a binary search per axis in the knot vector (IGA_FindSpan's rule: U[k] <= u < U[k+1], the upper end of
//   the axis in the last non-empty span); stores the span triple and whether the rank's element box holds the element.
// probe_eval / probe_geom: one point per lane, one wavefront per workgroup, a grid-stride loop over a grid capped at PROBE_G workgroups.
//   A lane computes the 1-D rows N, N', N'', N''' of its point on the device (probe_rows: Cox-de Boor with derivatives, the device twin of
//   bspline_ders in host.cpp) into LDS, row entry by row entry across the lanes (no bank conflict), then walks the (p+1)^dim basis functions
//   of its span in the fixed order a2, a1, a0 (a0 fastest) and adds coefficient * product of rows into the DISTINCT parametric partial sums
//   (probe_np: 1, 4, 10, 20 in 3-D at order 0..3) of the weight W, of every X component and of one field at a time.  The quotient rule
//   (probe_quot) and the chain through the geometry map (probe_chain) act once per point on those sums, not once per basis function as the
//   reference's Rationalize / InverseMap / ShapeFunctions do (src/petigaprobe.c:346-423): the same numbers mathematically.
//   The order of every sum depends on the point alone: no atomics, no cross-lane operation, so a point's result is bit-identical wherever
//   it stands in the list.  A point of another rank's element box writes zeros.
#pragma once
#include <hip/hip_runtime.h>
#include "igx.hpp"

namespace igx {

constexpr int PROBE_T = 64;        // lanes per workgroup: one wavefront, one point per lane
constexpr int PROBE_G = 2048;      // workgroups of a launch at the most (PROBE_G * PROBE_T points per turn of the grid-stride loop)

struct ProbeAxisDev {
  const double *U;     // [m+1] the knot vector
  const int *elof;     // [m+1] global element of knot span k (-1: an empty span)
  int p, n;            // degree; index of the last basis function (m - p - 1): the axis is [U[p], U[n+1]]
  int estart, ewidth;  // the rank's element box
};
struct ProbeDev { int dim, namax; ProbeAxisDev ax[3]; };      // namax: the largest p + 1 (row stride in LDS)

__global__ void __launch_bounds__(256) probe_locate(ProbeDev L, const double *pts, long long npts, int *span, unsigned char *local) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npts; i += (long long)gridDim.x * blockDim.x) {
    bool loc = true;
    for (int d = 0; d < 3; ++d) {
      int k = 0;
      if (d < L.dim) {
        const ProbeAxisDev &A = L.ax[d];
        const double u = pts[i * L.dim + d];
        int lo = A.p, hi = A.n + 1;                       // U[lo] <= u; u < U[hi] or hi is the upper end
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (A.U[mid] <= u) lo = mid; else hi = mid; }
        while (lo > A.p && A.U[lo] == A.U[lo + 1]) --lo;  // the upper end (or a repeated last knot): the last non-empty span
        k = lo;
        const int el = A.elof[k] - A.estart;
        loc = loc && el >= 0 && el < A.ewidth;
      }
      span[i * 3 + d] = k;
    }
    local[i] = loc ? 1 : 0;
  }
}

// number of distinct partial derivatives of order <= der, and the position of the partial (k0, k1, k2) among them (graded: by total
// order, then by k2, then by k1)
template <int DIM> __host__ __device__ constexpr int probe_np(int der) { return DIM == 1 ? der + 1 : (DIM == 2 ? (der + 1) * (der + 2) / 2 : (der + 1) * (der + 2) * (der + 3) / 6); }
template <int DIM> __host__ __device__ constexpr int probe_pi(int k0, int k1, int k2) {
  const int r = k0 + k1 + k2;
  return DIM == 1 ? r : (DIM == 2 ? r * (r + 1) / 2 + k1 : r * (r + 1) * (r + 2) / 6 + k2 * (r + 1) - k2 * (k2 - 1) / 2 + k1);
}
template <int DIM> __host__ __device__ constexpr int probe_p1(int a) { return probe_pi<DIM>(a == 0, a == 1, a == 2); }
template <int DIM> __host__ __device__ constexpr int probe_p2(int a, int b) { return probe_pi<DIM>((a == 0) + (b == 0), (a == 1) + (b == 1), (a == 2) + (b == 2)); }
template <int DIM> __host__ __device__ constexpr int probe_p3(int a, int b, int c) { return probe_pi<DIM>((a == 0) + (b == 0) + (c == 0), (a == 1) + (b == 1) + (c == 1), (a == 2) + (b == 2) + (c == 2)); }

// The 1-D rows of span `span` at u: out[(a * (DER + 1) + k) * PROBE_T] = k-th derivative of function span - p + a (bspline_ders, host.cpp:
// the same operations in the same order; derivatives above the degree are 0).
template <int DER>
__device__ inline void probe_rows(int span, double u, int p, const double *U, double *out) {
  double ndu[8][8], left[8], right[8], a[2][8];
  ndu[0][0] = 1.0;
  for (int j = 1; j <= p; ++j) {
    left[j] = u - U[span + 1 - j];
    right[j] = U[span + j] - u;
    double saved = 0.0;
    for (int r = 0; r < j; ++r) {
      ndu[j][r] = right[r + 1] + left[j - r];
      const double tmp = ndu[r][j - 1] / ndu[j][r];
      ndu[r][j] = saved + right[r + 1] * tmp;
      saved = left[j - r] * tmp;
    }
    ndu[j][j] = saved;
  }
  for (int j = 0; j <= p; ++j) out[(j * (DER + 1)) * PROBE_T] = ndu[j][p];
  if constexpr (DER > 0) {
    const int nders = DER < p ? DER : p;
    for (int r = 0; r <= p; ++r) {
      int s1 = 0, s2 = 1;
      a[0][0] = 1.0;
      double fac = 1.0;
      for (int k = 1; k <= DER; ++k) {
        double d = 0.0;
        if (k <= nders) {
          const int rk = r - k, pk = p - k;
          if (r >= k) { a[s2][0] = a[s1][0] / ndu[pk + 1][rk]; d = a[s2][0] * ndu[rk][pk]; }
          const int j1 = (rk >= -1) ? 1 : -rk;
          const int j2 = (r - 1 <= pk) ? k - 1 : p - r;
          for (int j = j1; j <= j2; ++j) {
            a[s2][j] = (a[s1][j] - a[s1][j - 1]) / ndu[pk + 1][rk + j];
            d += a[s2][j] * ndu[rk + j][pk];
          }
          if (r <= pk) { a[s2][k] = -a[s1][k - 1] / ndu[pk + 1][r]; d += a[s2][k] * ndu[r][pk]; }
          fac *= (double)(p - k + 1);
          const int t = s1; s1 = s2; s2 = t;
        }
        out[(r * (DER + 1) + k) * PROBE_T] = d * fac;
      }
    }
  }
}

// The partial sums: acc[q * NP + s] += v[q] * d^s N_a over the basis functions a of the span, a0 fastest.  coef(a0, a1, a2, v) hands
// the NQ coefficients of function a.
template <int DIM, int DER, int NQ, class Coef>
__device__ __forceinline__ void probe_sums(const double *rows, int namax, const int na[3], Coef coef, double *acc) {
  constexpr int NP = probe_np<DIM>(DER), K = DER + 1;
#pragma unroll
  for (int i = 0; i < NQ * NP; ++i) acc[i] = 0.0;
  const int n1 = DIM > 1 ? na[1] : 1, n2 = DIM > 2 ? na[2] : 1;
  for (int a2 = 0; a2 < n2; ++a2) {
    double r2[K];
#pragma unroll
    for (int k = 0; k < K; ++k) r2[k] = DIM > 2 ? rows[((2 * namax + a2) * K + k) * PROBE_T] : (k == 0 ? 1.0 : 0.0);
    for (int a1 = 0; a1 < n1; ++a1) {
      double r1[K], t12[K][K];
#pragma unroll
      for (int k = 0; k < K; ++k) r1[k] = DIM > 1 ? rows[((1 * namax + a1) * K + k) * PROBE_T] : (k == 0 ? 1.0 : 0.0);
#pragma unroll
      for (int k2 = 0; k2 < K; ++k2)
#pragma unroll
        for (int k1 = 0; k1 + k2 < K; ++k1) t12[k1][k2] = r1[k1] * r2[k2];
      for (int a0 = 0; a0 < na[0]; ++a0) {
        double r0[K], v[NQ];
#pragma unroll
        for (int k = 0; k < K; ++k) r0[k] = rows[((0 * namax + a0) * K + k) * PROBE_T];
        coef(a0, a1, a2, v);
#pragma unroll
        for (int k2 = 0; k2 < (DIM > 2 ? K : 1); ++k2)
#pragma unroll
          for (int k1 = 0; k1 < (DIM > 1 ? K - k2 : 1); ++k1)
#pragma unroll
            for (int k0 = 0; k0 < K - k1 - k2; ++k0) {
              const double b = r0[k0] * t12[k1][k2];
#pragma unroll
              for (int q = 0; q < NQ; ++q) acc[q * NP + probe_pi<DIM>(k0, k1, k2)] += v[q] * b;
            }
      }
    }
  }
}

// The quotient rule on the sums, in place: Y holds the partials of sum w_a Y_a N_a on entry and those of the quotient by W on return
// (Rationalize, src/petigarat.f90.in:3-57, applied to the sum instead of to every basis function).
template <int DIM, int DER>
__device__ __forceinline__ void probe_quot(const double *W, double *Y) {
  const double w0 = W[0];
  Y[0] = Y[0] / w0;
  if constexpr (DER >= 1) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) Y[probe_p1<DIM>(a)] = (Y[probe_p1<DIM>(a)] - Y[0] * W[probe_p1<DIM>(a)]) / w0;
  }
  if constexpr (DER >= 2) {
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int b = a; b < DIM; ++b)
        Y[probe_p2<DIM>(a, b)] = (Y[probe_p2<DIM>(a, b)] - Y[0] * W[probe_p2<DIM>(a, b)] - Y[probe_p1<DIM>(a)] * W[probe_p1<DIM>(b)] - Y[probe_p1<DIM>(b)] * W[probe_p1<DIM>(a)]) / w0;
  }
  if constexpr (DER >= 3) {
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int b = a; b < DIM; ++b)
#pragma unroll
        for (int c = b; c < DIM; ++c)
          Y[probe_p3<DIM>(a, b, c)] = (Y[probe_p3<DIM>(a, b, c)] - Y[0] * W[probe_p3<DIM>(a, b, c)]
                                       - Y[probe_p1<DIM>(a)] * W[probe_p2<DIM>(b, c)] - Y[probe_p1<DIM>(b)] * W[probe_p2<DIM>(a, c)] - Y[probe_p1<DIM>(c)] * W[probe_p2<DIM>(a, b)]
                                       - Y[probe_p2<DIM>(b, c)] * W[probe_p1<DIM>(a)] - Y[probe_p2<DIM>(a, c)] * W[probe_p1<DIM>(b)] - Y[probe_p2<DIM>(a, b)] * W[probe_p1<DIM>(c)]) / w0;
  }
}

// The chain through the geometry map on the sums: F holds the parametric partials of a field f(x(u)), X those of the DIM components of
// x (X + l * NP), e1[a * DIM + i] = du_a / dx_i.  out receives the DIM^DER physical derivatives of order DER.  With g = grad_x f,
// h = hess_x f, t = the third derivatives:
//   f_a = g_l x^l_a;  f_ab = h_lm x^l_a x^m_b + g_l x^l_ab;  f_abc = t_lmn x^l_a x^m_b x^n_c + h_lm (x^l_ab x^m_c + x^l_ac x^m_b + x^l_bc x^m_a) + g_l x^l_abc,
// solved for g, h, t in turn (InverseMap + ShapeFunctions, src/petigamapinv.f90.in, src/petigamapshf.f90.in, without forming the
// derivatives of the inverse map).
template <int DIM, int DER>
__device__ __forceinline__ void probe_chain(const double *F, const double *X, const double *e1, double *out) {
  constexpr int NP = probe_np<DIM>(DER), D2 = DIM * DIM;
  double g[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) { double s = 0; for (int a = 0; a < DIM; ++a) s += F[probe_p1<DIM>(a)] * e1[a * DIM + i]; g[i] = s; }
  if constexpr (DER == 1) { for (int i = 0; i < DIM; ++i) out[i] = g[i]; return; }
  else {
    double r2[D2], h[D2], t1[D2];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int b = 0; b < DIM; ++b) { double s = F[probe_p2<DIM>(a, b)]; for (int l = 0; l < DIM; ++l) s -= g[l] * X[l * NP + probe_p2<DIM>(a, b)]; r2[a * DIM + b] = s; }
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
      for (int b = 0; b < DIM; ++b) { double s = 0; for (int a = 0; a < DIM; ++a) s += r2[a * DIM + b] * e1[a * DIM + i]; t1[i * DIM + b] = s; }
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
      for (int j = 0; j < DIM; ++j) { double s = 0; for (int b = 0; b < DIM; ++b) s += t1[i * DIM + b] * e1[b * DIM + j]; h[i * DIM + j] = s; }
    if constexpr (DER == 2) { for (int i = 0; i < D2; ++i) out[i] = h[i]; return; }
    else {
      constexpr int D3 = D2 * DIM;
      double r3[D3], u3[D3];
#pragma unroll
      for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b)
#pragma unroll
          for (int c = 0; c < DIM; ++c) {
            double s = F[probe_p3<DIM>(a, b, c)];
            for (int l = 0; l < DIM; ++l) {
              s -= g[l] * X[l * NP + probe_p3<DIM>(a, b, c)];
              for (int m = 0; m < DIM; ++m)
                s -= h[l * DIM + m] * (X[l * NP + probe_p2<DIM>(a, b)] * X[m * NP + probe_p1<DIM>(c)] + X[l * NP + probe_p2<DIM>(a, c)] * X[m * NP + probe_p1<DIM>(b)]
                                       + X[l * NP + probe_p2<DIM>(b, c)] * X[m * NP + probe_p1<DIM>(a)]);
            }
            r3[(a * DIM + b) * DIM + c] = s;
          }
      // one index at a time: a -> i, b -> j, c -> k
#pragma unroll
      for (int i = 0; i < DIM; ++i)
#pragma unroll
        for (int bc = 0; bc < D2; ++bc) { double s = 0; for (int a = 0; a < DIM; ++a) s += r3[a * D2 + bc] * e1[a * DIM + i]; u3[i * D2 + bc] = s; }
#pragma unroll
      for (int i = 0; i < DIM; ++i)
#pragma unroll
        for (int j = 0; j < DIM; ++j)
#pragma unroll
          for (int c = 0; c < DIM; ++c) { double s = 0; for (int b = 0; b < DIM; ++b) s += u3[(i * DIM + b) * DIM + c] * e1[b * DIM + j]; r3[(i * DIM + j) * DIM + c] = s; }
#pragma unroll
      for (int ij = 0; ij < D2; ++ij)
#pragma unroll
        for (int k = 0; k < DIM; ++k) { double s = 0; for (int c = 0; c < DIM; ++c) s += r3[ij * DIM + c] * e1[c * DIM + k]; out[ij * DIM + k] = s; }
    }
  }
}

// the rows of a point's three axes into LDS, its element's first functions and sizes; false: the point is another rank's
template <int DIM, int DER>
__device__ __forceinline__ void probe_point_rows(const SpaceDev &S, const ProbeDev &L, const double *pts, const int *span, long long i, double *rows, int off[3], int na[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    off[d] = 0; na[d] = 1;
    if (d < DIM) {
      const int k = span[i * 3 + d];
      na[d] = L.ax[d].p + 1;
      off[d] = S.ax[d].off[L.ax[d].elof[k] - L.ax[d].estart];
      probe_rows<DER>(k, pts[i * DIM + d], L.ax[d].p, L.ax[d].U, rows + (size_t)d * L.namax * (DER + 1) * PROBE_T);
    }
  }
}

// Derivative DER of every field at every point: out[pt][c][DIM^DER] (IGA_GetValue / Grad / Hess / Der3, src/petigaprobe.c:456-462).
// RAT: rational weights enter (S.W); MAP: a geometry with nsd = dim, derivatives with respect to x (else parametric).
template <int DIM, int DER, bool RAT, bool MAP>
__global__ void __launch_bounds__(PROBE_T) probe_eval(SpaceDev S, ProbeDev L, const double *pts, const int *span, const unsigned char *local,
                                                      const double *U, double *out, long long npts) {
  constexpr int NP = probe_np<DIM>(DER), K = DER + 1;
  constexpr int NO = DER == 0 ? 1 : (DER == 1 ? DIM : (DER == 2 ? DIM * DIM : DIM * DIM * DIM));
  constexpr bool CHAIN = MAP && DER > 0;
  constexpr int NG = (RAT ? 1 : 0) + (CHAIN ? DIM : 0);      // geometry sums: W, then the components of w X
  extern __shared__ __attribute__((aligned(16))) double probe_lds[];
  double *rows = probe_lds + threadIdx.x;
  const int dof = S.dof;
  const int gw0 = S.ax[0].gwidth, gw1 = S.ax[1].gwidth, nr0 = S.ax[0].nrow, nr1 = S.ax[1].nrow;
  const int rw0 = S.ax[0].rwrap, rw1 = S.ax[1].rwrap, rw2 = S.ax[2].rwrap;
  for (long long i = (long long)blockIdx.x * PROBE_T + threadIdx.x; i < npts; i += (long long)gridDim.x * PROBE_T) {
    double *o = out + (size_t)i * dof * NO;
    if (!local[i]) { for (int k = 0; k < dof * NO; ++k) o[k] = 0.0; continue; }
    int off[3], na[3];
    probe_point_rows<DIM, DER>(S, L, pts, span, i, rows, off, na);
    double geo[(NG > 0 ? NG : 1) * NP], e1[DIM * DIM];
    if constexpr (NG > 0) {
      probe_sums<DIM, DER, NG>(rows, L.namax, na, [&](int a0, int a1, int a2, double *v) {
        const size_t g = (size_t)(off[0] + a0) + (size_t)gw0 * ((size_t)(off[1] + a1) + (size_t)gw1 * (size_t)(off[2] + a2));
        const double w = RAT ? S.W[g] : 1.0;
        if (RAT) v[0] = w;
        if constexpr (CHAIN) for (int c = 0; c < DIM; ++c) v[(RAT ? 1 : 0) + c] = RAT ? w * S.X[g * DIM + c] : S.X[g * DIM + c];
      }, geo);
    }
    const double *Wp = geo, *Xp = geo + (RAT ? NP : 0);
    if constexpr (CHAIN) {
      if (RAT) for (int c = 0; c < DIM; ++c) probe_quot<DIM, DER>(Wp, geo + (1 + c) * NP);
      double X1[DIM * DIM];
#pragma unroll
      for (int l = 0; l < DIM; ++l)
#pragma unroll
        for (int a = 0; a < DIM; ++a) X1[l * DIM + a] = Xp[l * NP + probe_p1<DIM>(a)];
      inv3(X1, DIM, det3(X1, DIM), e1);
    }
    for (int c = 0; c < dof; ++c) {
      double F[NP];
      probe_sums<DIM, DER, 1>(rows, L.namax, na, [&](int a0, int a1, int a2, double *v) {
        const int i0 = off[0] + a0, i1 = off[1] + a1, i2 = off[2] + a2;
        const size_t row = (size_t)(i0 < rw0 ? i0 : i0 - rw0) + (size_t)nr0 * ((size_t)(i1 < rw1 ? i1 : i1 - rw1) + (size_t)nr1 * (size_t)(i2 < rw2 ? i2 : i2 - rw2));
        double u = U[row * dof + c];
        if (RAT) u *= S.W[(size_t)i0 + (size_t)gw0 * ((size_t)i1 + (size_t)gw1 * (size_t)i2)];
        v[0] = u;
      }, F);
      if (RAT) probe_quot<DIM, DER>(Wp, F);
      double *oc = o + c * NO;
      if constexpr (DER == 0) oc[0] = F[0];
      else if constexpr (CHAIN) probe_chain<DIM, DER>(F, Xp, e1, oc);
      else if constexpr (DER == 1) { for (int a = 0; a < DIM; ++a) oc[a] = F[probe_p1<DIM>(a)]; }
      else if constexpr (DER == 2) { for (int a = 0; a < DIM; ++a) for (int b = 0; b < DIM; ++b) oc[a * DIM + b] = F[probe_p2<DIM>(a, b)]; }
      else { for (int a = 0; a < DIM; ++a) for (int b = 0; b < DIM; ++b) for (int cc = 0; cc < DIM; ++cc) oc[(a * DIM + b) * DIM + cc] = F[probe_p3<DIM>(a, b, cc)]; }
    }
  }
  (void)K;
}

// The geometry map at every point: out[pt][nsd] (IGAProbeGeomMap); nsd may exceed dim (a curve or a surface in space).
template <int DIM, bool RAT>
__global__ void __launch_bounds__(PROBE_T) probe_geom(SpaceDev S, ProbeDev L, const double *pts, const int *span, const unsigned char *local, double *out, long long npts) {
  extern __shared__ __attribute__((aligned(16))) double probe_lds[];
  double *rows = probe_lds + threadIdx.x;
  const int nsd = S.nsd, gw0 = S.ax[0].gwidth, gw1 = S.ax[1].gwidth;
  for (long long i = (long long)blockIdx.x * PROBE_T + threadIdx.x; i < npts; i += (long long)gridDim.x * PROBE_T) {
    double *o = out + (size_t)i * nsd;
    if (!local[i]) { for (int k = 0; k < nsd; ++k) o[k] = 0.0; continue; }
    int off[3], na[3];
    probe_point_rows<DIM, 0>(S, L, pts, span, i, rows, off, na);
    double acc[4];
    probe_sums<DIM, 0, 4>(rows, L.namax, na, [&](int a0, int a1, int a2, double *v) {
      const size_t g = (size_t)(off[0] + a0) + (size_t)gw0 * ((size_t)(off[1] + a1) + (size_t)gw1 * (size_t)(off[2] + a2));
      const double w = RAT ? S.W[g] : 1.0;
      v[0] = w;
      for (int c = 0; c < 3; ++c) v[1 + c] = c < nsd ? w * S.X[g * nsd + c] : 0.0;
    }, acc);
    for (int c = 0; c < nsd; ++c) o[c] = RAT ? acc[1 + c] / acc[0] : acc[1 + c];
  }
}

}  // namespace igx
