// host.cpp -- O(N) discretisation set-up that stays on the host: knot vectors, Gauss rules, 1-D basis
// tables, processor grid, element/node ranges and the per-axis index layout of the device matrix.
// Restates L0 of the reference (petigaaxis.c, petigarule.c, petigabasis.c, petigapart.c,
// petiga.c:1111-1310, petigamat.c:197-267); results are bit-exact for every integer quantity.
#include "igx.hpp"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <string>
#include <cstdlib>

namespace igx {

EnvSwitches read_env_switches() {
  EnvSwitches e;
  auto num = [](const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; };
  e.kernel = num("IGX_KERNEL", 0); if (e.kernel < 0 || e.kernel > 4) e.kernel = 0;
  e.walk_axis = num("IGX_WALK_AXIS", 0);
  e.nseg = num("IGX_NSEG", 0);
  e.no_first_touch = num("IGX_NO_FIRST_TOUCH", 0) != 0;
  e.block_pencil = num("IGX_BLOCK_PENCIL", 1);
  e.vec_sumfact = num("IGX_VEC_SUMFACT", 1);
  e.state_pencil = num("IGX_STATE_PENCIL", 1);
  e.no_vec_pairs = num("IGX_NO_VEC_PAIRS", 0);
  e.fuse_groups = num("IGX_FUSE_GROUPS", 1);
  e.overlap = num("IGX_OVERLAP", -1);
  e.clock_probe = num("IGX_CLOCK_PROBE", 0) != 0;
  e.feature_lds_kb = num("IGX_FEATURE_LDS_KB", 0);
  e.combine = num("IGX_COMBINE", -1);
  e.free_run = num("IGX_FREE_RUN", -1);
  e.p2_pack = num("IGX_P2_PACK", 1);
  e.fuse_resid = num("IGX_FUSE_RESID", 0);
  e.patch = num("IGX_PATCH", 1);
  e.gram_sumfact = num("IGX_GRAM_SUMFACT", 1);
  e.patch_state = num("IGX_PATCH_STATE", 0);
  e.patch3 = num("IGX_PATCH3", 1);
  e.patch3_persist = num("IGX_PATCH3_PERSIST", 1) != 0;
  e.patch3_grid = std::max(0, std::min(num("IGX_PATCH3_GRID", 0), 1 << 16));
  e.patch3_order = num("IGX_PATCH3_ORDER", 1) != 0;
  e.rows3 = num("IGX_ROWS3", 1); if (e.rows3 < 0 || e.rows3 > 2) e.rows3 = 1;
  e.rows3_grid = std::max(0, std::min(num("IGX_ROWS3_GRID", 0), 1 << 16));
  e.rows3_stage = num("IGX_ROWS3_STAGE", 1); if (e.rows3_stage < 0 || e.rows3_stage > 2) e.rows3_stage = 1;
  e.small_wpb = num("IGX_SMALL_WPB", 1);
  e.matmult_index = num("IGX_MATMULT_INDEX", -1); if (e.matmult_index < 0 || e.matmult_index > 1) e.matmult_index = -1;
  e.band_prio = num("IGX_BAND_PRIO", 0); e.band_rmw_prio = num("IGX_BAND_RMW_PRIO", 0);
  if (kDebug) { e.debug_feature = num("IGX_DEBUG_FEATURE", 0); e.debug_noflush = num("IGX_DEBUG_NOFLUSH", 0); e.debug_timing = getenv("IGX_DEBUG_TIMING") != nullptr; e.debug_noprio = num("IGX_DEBUG_NOPRIO", 0); }
  return e;
}

// ------------------------------------------------------------------ quadrature rules
// The reference tabulates Gauss-Legendre q = 1..10 (src/petigarule.c:182-319) and Gauss-Lobatto q = 2..10 (:321-459) as
// 36-digit constants.  Here the nodes are computed: Newton's method on P_q (Legendre) or P'_{q-1} (Lobatto) in long double
// from a cosine guess, polished in quadruple precision so that the value cast to double is the correctly rounded one -- the
// double the reference's literal denotes (tests/test_golden.py holds both rules to tests/golden/gauss_rules.json, bit for bit).
namespace {
using quad = __float128;
struct Leg { quad P, dP, ddP; };        // P_n(x), P_n'(x), P_n''(x)
Leg legendre(int n, quad x) {
  quad a = 1, b = x;
  if (n == 0) return {1, 0, 0};
  for (int k = 2; k <= n; ++k) { quad c = ((2 * k - 1) * x * b - (k - 1) * a) / k; a = b; b = c; }
  const quad dP = n * (x * b - a) / (x * x - 1);
  return {b, dP, (2 * x * dP - n * (n + 1) * b) / (1 - x * x)};      // Legendre's equation gives the second derivative
}
template <bool LOBATTO> quad rule_root(int n, long double guess) {
  long double x = guess;
  for (int it = 0; it < 64; ++it) {
    const Leg l = legendre(n, (quad)x);
    const long double dx = LOBATTO ? (long double)(l.dP / l.ddP) : (long double)(l.P / l.dP);
    x -= dx;
    if (fabsl(dx) < 1e-19L) break;
  }
  quad xq = x;
  for (int it = 0; it < 3; ++it) { const Leg l = legendre(n, xq); xq -= LOBATTO ? l.dP / l.ddP : l.P / l.dP; }
  return xq;
}
const long double kPi = 3.14159265358979323846264338327950288L;
}  // namespace

int gauss_legendre(int q, double *X, double *W) {
  if (q < 1 || q > 10) return IGX_ERR_ARG_OUTOFRANGE;
  for (int i = 0; i < (q + 1) / 2; ++i) {
    const quad x = rule_root<false>(q, cosl(kPi * (i + 0.75L) / (q + 0.5L)));
    const Leg l = legendre(q, x);
    const quad w = 2 / ((1 - x * x) * l.dP * l.dP);
    X[i] = -(double)x; X[q - 1 - i] = (double)x;
    W[i] = (double)w;  W[q - 1 - i] = (double)w;
  }
  if (q & 1) X[q / 2] = 0.0;
  return 0;
}

// Gauss-Lobatto: the end points and the roots of P'_{q-1}; weights 2 / (q (q-1) P_{q-1}(x)^2).
int gauss_lobatto(int q, double *X, double *W) {
  if (q < 2 || q > 10) return IGX_ERR_ARG_OUTOFRANGE;
  const int n = q - 1;
  for (int i = 0; i < (q + 1) / 2; ++i) {
    const quad x = i == 0 ? (quad)1 : rule_root<true>(n, cosl(kPi * i / n));
    const Leg l = legendre(n, x);
    const quad w = 2 / ((quad)(q * n) * l.P * l.P);
    X[i] = -(double)x; X[q - 1 - i] = (double)x;
    W[i] = (double)w;  W[q - 1 - i] = (double)w;
  }
  if (q & 1) X[q / 2] = 0.0;
  return 0;
}

// IGARuleSetUp (src/petigarule.c:116-143): the rule of an axis by type.
int rule_setup(const Rule1D &r, int nqp, double *X, double *W, std::string &err) {
  int rc = 0;
  switch (r.type) {
    case IGX_RULE_LEGENDRE: rc = gauss_legendre(nqp, X, W); break;
    case IGX_RULE_LOBATTO:  rc = gauss_lobatto(nqp, X, W); break;
    case IGX_RULE_USER:
      if ((int)r.x.size() != nqp) { err = "user-defined rule has a different number of points"; return IGX_ERR_ARG_WRONGSTATE; }
      for (int q = 0; q < nqp; ++q) { X[q] = r.x[q]; W[q] = r.w[q]; }
      break;
    default:   // IGA_RULE_REDUCED: Gauss-Legendre; basis_init gives the interior elements one point less (src/petigabasis.c:144-171)
      rc = gauss_legendre(nqp, X, W); break;
  }
  if (rc) { err = "Number of quadrature points not implemented"; return IGX_ERR_ARG_OUTOFRANGE; }
  return 0;
}

// ------------------------------------------------------------------ B-spline basis and derivatives
// Piegl & Tiller A2.3 (the algorithm of src/petigabsb.f90.in:3-63); output [a][0..4] like
// src/petigabsp.F90:3-16 with unused derivative slots zero.
void bspline_ders(int span, double u, int p, int nders, const double *U, double *out) {
  constexpr int MP = 8;
  double ndu[MP][MP], left[MP], right[MP], a[2][MP];
  ndu[0][0] = 1.0;
  for (int j = 1; j <= p; ++j) {
    left[j] = u - U[span + 1 - j];
    right[j] = U[span + j] - u;
    double saved = 0.0;
    for (int r = 0; r < j; ++r) {
      ndu[j][r] = right[r + 1] + left[j - r];
      double tmp = ndu[r][j - 1] / ndu[j][r];
      ndu[r][j] = saved + right[r + 1] * tmp;
      saved = left[j - r] * tmp;
    }
    ndu[j][j] = saved;
  }
  for (int j = 0; j <= p; ++j) {
    for (int k = 0; k < 5; ++k) out[j * 5 + k] = 0.0;
    out[j * 5] = ndu[j][p];
  }
  for (int r = 0; r <= p; ++r) {
    int s1 = 0, s2 = 1;
    a[0][0] = 1.0;
    for (int k = 1; k <= nders; ++k) {
      double d = 0.0;
      const int rk = r - k, pk = p - k;
      if (r >= k) { a[s2][0] = a[s1][0] / ndu[pk + 1][rk]; d = a[s2][0] * ndu[rk][pk]; }
      const int j1 = (rk >= -1) ? 1 : -rk;
      const int j2 = (r - 1 <= pk) ? k - 1 : p - r;
      for (int j = j1; j <= j2; ++j) {
        a[s2][j] = (a[s1][j] - a[s1][j - 1]) / ndu[pk + 1][rk + j];
        d += a[s2][j] * ndu[rk + j][pk];
      }
      if (r <= pk) { a[s2][k] = -a[s1][k - 1] / ndu[pk + 1][r]; d += a[s2][k] * ndu[r][pk]; }
      out[r * 5 + k] = d;
      std::swap(s1, s2);
    }
  }
  int fac = p;
  for (int k = 1; k <= nders; ++k) {
    for (int j = 0; j <= p; ++j) out[j * 5 + k] *= (double)fac;
    fac *= (p - k);
  }
}

// ------------------------------------------------------------------ knot vectors
static int next_knot(int m, const double *U, int k, int dir) {   // src/petigaaxis.c:482-494
  if (dir >= 0) {
    if (k < 0) return 0;
    for (int j = k + 1; j < m; ++j) if (U[j] > U[k]) return j;
    return m;
  }
  if (k > m) return m;
  for (int j = k - 1; j > 0; --j) if (U[j] < U[k]) return j;
  return 0;
}

void axis_finish(Axis &ax) {   // src/petigaaxis.c:286-312, :513-523
  const int p = ax.p, m = ax.m, n = m - p - 1;
  ax.span.clear();
  for (int k = next_knot(m, ax.U.data(), p, 1); k <= n + 1; k = next_knot(m, ax.U.data(), k, 1)) ax.span.push_back(k - 1);
  ax.nel = (int)ax.span.size();
  if (ax.periodic) {
    const int k = n + 1, j = next_knot(m, ax.U.data(), k, 1), s = j - k, C = p - s;
    ax.nnp = n - C;
  } else ax.nnp = n + 1;
}

int axis_init_uniform(Axis &ax, int N, double Ui, double Uf, int C, std::string &err) {   // src/petigaaxis.c:401-456
  const int p = ax.p;
  if (p < 1) { err = "Must call IGAAxisSetDegree() first"; return IGX_ERR_ORDER; }
  if (C == IGX_DECIDE) C = p - 1;
  if (N < 1) { err = "Number of elements must be greater than zero"; return IGX_ERR_ARG_WRONG; }
  if (Ui >= Uf) { err = "Initial value must be less than final value"; return IGX_ERR_ARG_WRONG; }
  if (C < 0 || C >= p) { err = "Continuity must be in range [0,p-1]"; return IGX_ERR_ARG_WRONG; }
  const int s = p - C, m = 2 * (p + 1) + (N - 1) * s - 1, n = m - p - 1;
  ax.m = m;
  ax.U.assign((size_t)m + 1, 0.0);
  int k = 0;
  for (; k <= p; ++k) { ax.U[k] = Ui; ax.U[m - k] = Uf; }
  for (int b = 1; b < N; ++b)
    for (int j = 0; j < s; ++j) ax.U[k++] = Ui + (double)b / (double)N * (Uf - Ui);
  if (ax.periodic)
    for (k = 0; k <= C; ++k) {
      ax.U[C - k] = ax.U[p] - ax.U[m - p] + ax.U[n - k];
      ax.U[m - C + k] = ax.U[m - p] - ax.U[p] + ax.U[p + 1 + k];
    }
  ax.nel = N;
  ax.span.resize(N);
  for (int e = 0; e < N; ++e) ax.span[e] = p + e * s;
  ax.nnp = ax.periodic ? n - C : n + 1;
  return 0;
}

int axis_set_knots(Axis &ax, int m, const double *U, std::string &err) {   // src/petigaaxis.c:202-253
  const int p = ax.p;
  if (p < 1) { err = "Must call IGAAxisSetDegree() first"; return IGX_ERR_ORDER; }
  if (m < 2 * p + 1) { err = "Number of knots must be at least 2*(p+1)"; return IGX_ERR_ARG_OUTOFRANGE; }
  for (int k = 1; k <= m; ++k) if (U[k - 1] > U[k]) { err = "Knot sequence must be increasing"; return IGX_ERR_ARG_OUTOFRANGE; }
  for (int k = 1, j = m; k < m; k = j) {
    j = next_knot(m, U, k, 1);
    if (j - k > p) { err = "Knot multiplicity greater than degree"; return IGX_ERR_ARG_OUTOFRANGE; }
  }
  ax.m = m;
  ax.U.assign(U, U + m + 1);
  axis_finish(ax);
  return 0;
}

// ------------------------------------------------------------------ 1-D tables (src/petigabasis.c:83-219)
int basis_init(Basis1D &b, const Axis &ax, const Rule1D &rule, int nqp, std::string &err) {
  std::vector<double> Xv(std::max(nqp, 10)), Wv(std::max(nqp, 10));
  double *X = Xv.data(), *W = Wv.data();
  if (int rc = rule_setup(rule, nqp, X, W, err)) return rc;
  if (ax.p > 7) { err = "degree > 7 not supported"; return IGX_ERR_SUP; }
  const int p = ax.p, nel = ax.nel, nen = p + 1, d = std::min(p, 4);
  // IGA_RULE_REDUCED (src/petigabasis.c:144-171): the first and the last element keep the nqp points, the others take the rule with
  // nqp - 1.  The reference pads the last slot with weight 0 and trims it per element (IGA_Quadrature_SIZE, src/petigaelem.c:764-776);
  // the kernels here keep one point count per axis, so the padded slot stays in the tables with weight 0 -- it adds an exact zero --
  // and sits at the element's midpoint, where every form is finite (the reference leaves PETSC_MAX_REAL and no basis values there).
  std::vector<double> Xr, Wr;
  if (rule.type == IGX_RULE_REDUCED && nel > 2 && nqp > 1) {
    Xr.assign(std::max(nqp, 10), 0.0); Wr.assign(std::max(nqp, 10), 0.0);
    if (gauss_legendre(nqp - 1, Xr.data(), Wr.data())) { err = "Number of quadrature points not implemented"; return IGX_ERR_ARG_OUTOFRANGE; }
  }
  b.nel = nel; b.nqp = nqp; b.nen = nen;
  b.offset.assign(nel, 0); b.detJac.assign(nel, 0.0);
  b.weight.assign((size_t)nel * nqp, 0.0); b.point.assign((size_t)nel * nqp, 0.0);
  b.value.assign((size_t)nel * nqp * nen * 5, 0.0);
  for (int e = 0; e < nel; ++e) {
    const int k = ax.span[e];
    const double u0 = ax.U[k], u1 = ax.U[k + 1], J = (u1 - u0) / 2;
    b.detJac[e] = J;
    b.offset[e] = k - p;
    const bool reduced = !Xr.empty() && e > 0 && e < nel - 1;
    for (int q = 0; q < nqp; ++q) {
      const bool pad = reduced && q == nqp - 1;
      b.weight[(size_t)e * nqp + q] = reduced ? (pad ? 0.0 : Wr[q]) : W[q];
      const double u = ((reduced ? (pad ? 0.0 : Xr[q]) : X[q]) + 1) * J + u0;
      b.point[(size_t)e * nqp + q] = u;
      bspline_ders(k, u, p, d, ax.U.data(), &b.value[((size_t)e * nqp + q) * nen * 5]);
    }
  }
  {   // basis at the two ends of the axis for boundary-form passes (src/petigabasis.c:196-216)
    const int k0 = ax.span[0], k1 = ax.span[nel - 1];
    b.bnd_point[0] = ax.U[k0]; b.bnd_point[1] = ax.U[k1 + 1];
    for (int sd = 0; sd < 2; ++sd) b.bnd_value[sd].assign((size_t)nen * 5, 0.0);
    bspline_ders(k0, b.bnd_point[0], p, d, ax.U.data(), b.bnd_value[0].data());
    bspline_ders(k1, b.bnd_point[1], p, d, ax.U.data(), b.bnd_value[1].data());
  }
  return 0;
}

// ------------------------------------------------------------------ fast diagonalisation: the host half (IGXFastDiagSetUp)
// On a tensor-product space the parametric operator alpha M2 x M1 x M0 + beta0 M2 x M1 x K0 + beta1 M2 x K1 x M0 + beta2 K2 x M1 x M0 is
// diagonal in the basis U2 x U1 x U0 of the 1-D generalised eigenvectors K_d U_d = M_d U_d Lambda_d, U_d^T M_d U_d = I (Sangalli & Tani,
// SIAM J. Sci. Comput. 38 (2016)).  M_d and K_d come from the tables the element kernels read (offset, detJac, weight, value[..][0 and 1]),
// so the inverse is exact for the rule the user set.  The eigen-solver is this file's: Cholesky of M and the reduction L^-1 K L^-T in
// long double, cyclic Jacobi on the reduced matrix in double, a refinement of its eigenpairs in long double (refine_eigen), U = L^-T Q in
// long double.  Sizes are one axis' function count.
void fast_diag_fixed_faces(const Space &s, bool fixed[3][2][MAXFD]) {
  for (int d = 0; d < 3; ++d) for (int sd = 0; sd < 2; ++sd) for (int f = 0; f < MAXFD; ++f) {
    fixed[d][sd][f] = false;
    if (d >= s.dim || s.axis[d].periodic) continue;      // (IGAElementBuildFix skips periodic axes, src/petigaelem.c:1214)
    const BC &bc = s.value[d][sd];
    for (int k = 0; k < bc.count; ++k) if (bc.field[k] == f && f < s.dof) fixed[d][sd][f] = true;
  }
}

namespace {
// eigenpairs of the symmetric C [m][m] (destroyed): cyclic Jacobi, eigenvalues ascending in lam, eigenvector k in row k of Qt
void jacobi_eigen(int m, std::vector<double> &C, std::vector<double> &lam, std::vector<double> &Qt) {
  Qt.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) Qt[(size_t)i * m + i] = 1.0;
  double norm2 = 0;
  for (size_t i = 0; i < (size_t)m * m; ++i) norm2 += C[i] * C[i];
  const double small2 = norm2 * 1e-40, skip = std::sqrt(norm2) * 1e-24;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off2 = 0;
    for (int p = 0; p < m; ++p) for (int q = p + 1; q < m; ++q) off2 += C[(size_t)p * m + q] * C[(size_t)p * m + q];
    if (off2 <= small2) break;
    for (int p = 0; p < m - 1; ++p) {
      double *rp = &C[(size_t)p * m], *vp = &Qt[(size_t)p * m];
      for (int q = p + 1; q < m; ++q) {
        double *rq = &C[(size_t)q * m], *vq = &Qt[(size_t)q * m];
        const double apq = rp[q];
        if (std::fabs(apq) <= skip) { rp[q] = 0.0; rq[p] = 0.0; continue; }
        const double app = rp[p], aqq = rq[q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < m; ++k) { const double a = rp[k], b = rq[k]; rp[k] = c * a - sn * b; rq[k] = sn * a + c * b; }
        rp[p] = app - t * apq; rq[q] = aqq + t * apq; rp[q] = 0.0; rq[p] = 0.0;
        for (int k = 0; k < m; ++k) { if (k == p || k == q) continue; C[(size_t)k * m + p] = rp[k]; C[(size_t)k * m + q] = rq[k]; }
        for (int k = 0; k < m; ++k) { const double a = vp[k], b = vq[k]; vp[k] = c * a - sn * b; vq[k] = sn * a + c * b; }
      }
    }
  }
  std::vector<int> order(m);
  for (int i = 0; i < m; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return C[(size_t)a * m + a] < C[(size_t)b * m + b]; });
  lam.resize(m);
  std::vector<double> Q2((size_t)m * m);
  for (int k = 0; k < m; ++k) { lam[k] = C[(size_t)order[k] * m + order[k]]; std::copy(&Qt[(size_t)order[k] * m], &Qt[(size_t)order[k] * m] + m, &Q2[(size_t)k * m]); }
  Qt.swap(Q2);
}

// Refinement of the eigenpairs of the symmetric C [m][m] in long double (Ogita & Aishima, Japan J. Indust. Appl. Math. 35 (2018)):
// Q holds the approximate eigenvector k in its row k, lam the eigenvalues, ascending.  The double-precision rotations above leave
// Q Q^T - I and the off-diagonal of Q C Q^T at some 4e-16 m; one step Q <- (I + E^T) Q with
//   R = I - Q Q^T,  S = Q C Q^T,  lam_k = S_kk / (1 - R_kk),  E_kl = (S_kl + lam_l R_kl) / (lam_l - lam_k),  E_kk = R_kk / 2
// squares both errors.  Inside a cluster of eigenvalues (a periodic axis has exact pairs; |lam_l - lam_k| <= delta = 2 (|S - diag S| +
// |lam|max |R|), what the present pairs cannot resolve) the quotient is meaningless and any orthonormal basis of the invariant subspace
// serves: there E_kl = R_kl / 2, which restores orthonormality alone.  Steps repeat until max|E| <= 1e-9
// (the next step's correction would be below the long-double rounding of the products), three at the most.
void refine_eigen(int m, const std::vector<long double> &C, std::vector<double> &lam, std::vector<long double> &Q) {
  typedef long double ld;
  const size_t mm = (size_t)m * m;
  std::vector<ld> W(mm), S(mm), R(mm), E(mm), l(m);
  std::vector<double> Ed(mm), Qd(mm), D(mm);
  for (int step = 0; step < 3; ++step) {
    std::fill(W.begin(), W.end(), 0.0L);
    for (int k = 0; k < m; ++k)      // W = Q C
      for (int i = 0; i < m; ++i) { const ld q = Q[(size_t)k * m + i]; const ld *c = &C[(size_t)i * m]; ld *w = &W[(size_t)k * m]; for (int j = 0; j < m; ++j) w[j] += q * c[j]; }
    for (int k = 0; k < m; ++k) for (int h = k; h < m; ++h) {
      const ld *qk = &Q[(size_t)k * m], *qh = &Q[(size_t)h * m], *wk = &W[(size_t)k * m];
      ld s = 0, g = 0;
      for (int j = 0; j < m; ++j) { s += wk[j] * qh[j]; g += qk[j] * qh[j]; }
      S[(size_t)k * m + h] = S[(size_t)h * m + k] = s;
      R[(size_t)k * m + h] = R[(size_t)h * m + k] = (k == h ? 1.0L : 0.0L) - g;
    }
    for (int k = 0; k < m; ++k) l[k] = S[(size_t)k * m + k] / (1.0L - R[(size_t)k * m + k]);
    ld s2 = 0, r2 = 0, lmax = 0, emax = 0;
    for (int k = 0; k < m; ++k) {
      lmax = std::max(lmax, fabsl(l[k]));
      for (int h = 0; h < m; ++h) { r2 += R[(size_t)k * m + h] * R[(size_t)k * m + h]; if (h != k) s2 += S[(size_t)k * m + h] * S[(size_t)k * m + h]; }
    }
    // a cluster: a gap the present eigenvalues cannot tell from 0 (the paper's delta, Frobenius for spectral norms), or below double's reach
    const ld delta = std::max(2 * (sqrtl(s2) + lmax * sqrtl(r2)), 1e-14L * lmax);
    for (int k = 0; k < m; ++k) for (int h = 0; h < m; ++h) {
      const ld r = R[(size_t)k * m + h];
      ld e = r / 2;
      if (k != h) {
        const ld num = S[(size_t)k * m + h] + l[h] * r, gap = l[h] - l[k];
        if (fabsl(gap) > delta && fabsl(num) <= 1e-3L * fabsl(gap)) e = num / gap;
      }
      E[(size_t)k * m + h] = e;
      emax = std::max(emax, fabsl(e));
    }
    // row h of Q += sum_k E_kh (row k of Q): the correction is at most 1e-3 of Q, so double products leave it exact to 1e-19 of Q
    for (size_t i = 0; i < mm; ++i) { Ed[i] = (double)E[i]; Qd[i] = (double)Q[i]; }
    std::fill(D.begin(), D.end(), 0.0);
    for (int h = 0; h < m; ++h) {
      double *dh = &D[(size_t)h * m];
      for (int k = 0; k < m; ++k) { const double e = Ed[(size_t)k * m + h]; const double *qk = &Qd[(size_t)k * m]; for (int i = 0; i < m; ++i) dh[i] += e * qk[i]; }
    }
    for (size_t i = 0; i < mm; ++i) Q[i] += D[i];
    if (emax <= 1e-9L) break;
  }
  // the Rayleigh quotients of the step before the last correction are exact to second order in it; a cluster may have changed its order
  std::vector<int> order(m);
  for (int i = 0; i < m; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return l[a] < l[b]; });
  W = Q;
  for (int k = 0; k < m; ++k) { lam[k] = (double)l[order[k]]; std::copy(&W[(size_t)order[k] * m], &W[(size_t)order[k] * m] + m, &Q[(size_t)k * m]); }
}

}  // namespace

// K U = M U Lambda, U^T M U = I for the symmetric positive definite M and symmetric K, both [m][m] (IGX_ERR_PLIB: M is not positive definite)
int generalised_eigen(int m, const std::vector<double> &M, const std::vector<double> &K, FastDiagEig &out, std::string &err) {
  typedef long double ld;
  out.lambda.clear(); out.U.clear();
  if (m <= 0) return 0;
  std::vector<ld> L((size_t)m * m, 0.0L), X((size_t)m * m);
  for (int j = 0; j < m; ++j) {      // M = L L^T
    ld dg = M[(size_t)j * m + j];
    for (int k = 0; k < j; ++k) dg -= L[(size_t)j * m + k] * L[(size_t)j * m + k];
    if (!(dg > 0)) { err = "fast diagonalisation: the 1-D mass matrix of an axis is not positive definite"; return IGX_ERR_PLIB; }
    const ld ljj = sqrtl(dg);
    L[(size_t)j * m + j] = ljj;
    for (int i = j + 1; i < m; ++i) {
      ld v = M[(size_t)i * m + j];
      for (int k = 0; k < j; ++k) v -= L[(size_t)i * m + k] * L[(size_t)j * m + k];
      L[(size_t)i * m + j] = v / ljj;
    }
  }
  // X = L^-1 K (rows by forward substitution), then C = X L^-T, i.e. C^T = L^-1 X^T: the same substitution on X^T
  auto forward = [&](std::vector<ld> &B) {      // B <- L^-1 B, B [m][m] row-major
    for (int i = 0; i < m; ++i) {
      ld *bi = &B[(size_t)i * m];
      for (int k = 0; k < i; ++k) { const ld l = L[(size_t)i * m + k]; if (l == 0) continue; const ld *bk = &B[(size_t)k * m]; for (int c = 0; c < m; ++c) bi[c] -= l * bk[c]; }
      const ld inv = 1.0L / L[(size_t)i * m + i];
      for (int c = 0; c < m; ++c) bi[c] *= inv;
    }
  };
  for (size_t i = 0; i < (size_t)m * m; ++i) X[i] = K[i];
  forward(X);
  for (int i = 0; i < m; ++i) for (int j = i + 1; j < m; ++j) std::swap(X[(size_t)i * m + j], X[(size_t)j * m + i]);
  forward(X);
  std::vector<double> C((size_t)m * m), Qt;
  for (int i = 0; i < m; ++i) for (int j = i; j < m; ++j) X[(size_t)i * m + j] = X[(size_t)j * m + i] = (X[(size_t)i * m + j] + X[(size_t)j * m + i]) / 2;
  for (size_t i = 0; i < (size_t)m * m; ++i) C[i] = (double)X[i];
  jacobi_eigen(m, C, out.lambda, Qt);
  std::vector<ld> Q(Qt.begin(), Qt.end());
  refine_eigen(m, X, out.lambda, Q);
  out.U.assign((size_t)m * m, 0.0);
  std::vector<ld> y(m);
  for (int k = 0; k < m; ++k) {      // L^T u = q_k by back substitution
    for (int i = m - 1; i >= 0; --i) {
      ld v = Q[(size_t)k * m + i];
      for (int j = i + 1; j < m; ++j) v -= L[(size_t)j * m + i] * y[j];
      y[i] = v / L[(size_t)i * m + i];
    }
    for (int i = 0; i < m; ++i) out.U[(size_t)i + (size_t)m * k] = (double)y[i];
  }
  return 0;
}

int fast_diag_setup(const Space &s, double alpha, const double beta[3], FastDiag &fd, std::string &err) {
  fd = FastDiag();
  fd.alpha = alpha; fd.dof = s.dof;
  for (int d = 0; d < 3; ++d) fd.beta[d] = beta[d];
  fast_diag_fixed_faces(s, fd.fixed);
  std::vector<double> Mfull[3], Kfull[3];
  for (int d = 0; d < 3; ++d) {
    const Basis1D &b = s.basis[d];
    const int n = s.axis[d].nnp, per = s.axis[d].periodic;
    if (s.lay[d].nrow != n) { err = "fast diagonalisation: the row box of an axis is not its function range"; return IGX_ERR_PLIB; }
    fd.n[d] = n;
    std::vector<double> &M = Mfull[d], &K = Kfull[d];
    M.assign((size_t)n * n, 0.0); K.assign((size_t)n * n, 0.0); fd.count[d].assign(n, 0.0);
    for (int e = 0; e < b.nel; ++e) {
      auto fn = [&](int a) { const int i = b.offset[e] + a; return per ? ((i % n) + n) % n : i; };
      for (int a = 0; a < b.nen; ++a) fd.count[d][fn(a)] += 1.0;
      for (int q = 0; q < b.nqp; ++q) {
        const double wj = b.weight[(size_t)e * b.nqp + q] * b.detJac[e];
        const double *v = &b.value[((size_t)e * b.nqp + q) * b.nen * 5];
        for (int a = 0; a < b.nen; ++a) for (int c = 0; c < b.nen; ++c) {
          M[(size_t)fn(a) * n + fn(c)] += wj * v[a * 5] * v[c * 5];
          K[(size_t)fn(a) * n + fn(c)] += wj * v[a * 5 + 1] * v[c * 5 + 1];
        }
      }
    }
    for (int f = 0; f < s.dof; ++f) {
      FastDiagEig &E = fd.eig[d][fd.combo(d, f)];
      if (E.used) continue;
      E.used = true;
      E.first = fd.fixed[d][0][f] ? 1 : 0;
      E.m = std::max(0, n - E.first - (fd.fixed[d][1][f] ? 1 : 0));
      // an axis with the tables and the combination of an earlier one (a cube): its eigenpairs
      bool reused = false;
      for (int d2 = 0; d2 < d && !reused; ++d2) {
        const FastDiagEig &E2 = fd.eig[d2][fd.combo(d, f)];
        if (E2.used && fd.n[d2] == n && Mfull[d2] == M && Kfull[d2] == K) { E.lambda = E2.lambda; E.U = E2.U; reused = true; }
      }
      if (reused) continue;
      const int m = E.m;
      std::vector<double> Ms((size_t)m * m), Ks((size_t)m * m);
      for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) { Ms[(size_t)i * m + j] = M[(size_t)(E.first + i) * n + E.first + j]; Ks[(size_t)i * m + j] = K[(size_t)(E.first + i) * n + E.first + j]; }
      if (int rc = generalised_eigen(m, Ms, Ks, E, err)) return rc;
    }
  }
  // the denominators ((alpha + s0) + s1) + s2 with the rounded products s_d = beta_d lambda_d: sums alone, in this order here and on the
  // device, so the modes zeroed there are the modes counted here
  double dmax = 0;
  for (int d = 0; d < 3; ++d) for (int c = 0; c < 4; ++c) {
    FastDiagEig &E = fd.eig[d][c];
    E.s.resize(E.lambda.size());
    for (size_t i = 0; i < E.lambda.size(); ++i) E.s[i] = beta[d] * E.lambda[i];
  }
  for (int f = 0; f < s.dof; ++f) {
    double v = alpha;
    for (int d = 0; d < 3; ++d) { double mx = 0; for (double x : fd.eig[d][fd.combo(d, f)].s) mx = std::max(mx, std::fabs(x)); v += mx; }
    dmax = std::max(dmax, v);
  }
  fd.thresh = 1e-12 * dmax;
  fd.nzeroed = 0;
  for (int f = 0; f < s.dof; ++f) {
    const FastDiagEig &E0 = fd.eig[0][fd.combo(0, f)], &E1 = fd.eig[1][fd.combo(1, f)], &E2 = fd.eig[2][fd.combo(2, f)];
    for (int k = 0; k < E2.m; ++k) for (int j = 0; j < E1.m; ++j) {
      const double sjk[2] = {E1.s[j], E2.s[k]};
      for (int i = 0; i < E0.m; ++i) {
        const double den = ((alpha + E0.s[i]) + sjk[0]) + sjk[1];
        if (std::fabs(den) <= fd.thresh) fd.nzeroed++;
      }
    }
  }
  return 0;
}

// ------------------------------------------------------------------ processor grid (src/petigapart.c:11-168)
// The search below follows the reference step for step (initial guesses from the real-valued optimum,
// three descending sweeps, cube tie-breaks) because the resulting grid is part of the bit-exact contract.
namespace {
struct Grid2 { int m, n, cut; };
struct Grid3 { int m, n, p, cut; };
inline int cut2(int M, int N, int m, int n) { return M * (n - 1) + N * (m - 1); }
inline int cut3(int M, int N, int P, int m, int n, int p) { return N * P * (m - 1) + M * P * (n - 1) + M * N * (p - 1); }
inline int snap(int size, int m) { if (m == 0) m = 1; while (m > 0 && size % m) --m; return m; }

Grid2 guess2(int size, int M, int N) {
  Grid2 g;
  g.m = snap(size, (int)(0.5 + std::sqrt(((double)M) / ((double)N) * ((double)size))));
  g.n = size / g.m;
  g.cut = cut2(M, N, g.m, g.n);
  return g;
}
Grid2 best2(int size, int M, int N) {
  Grid2 a = guess2(size, M, N), bt = guess2(size, N, M), r;
  if (a.cut < bt.cut) { r.m = a.m; r.n = a.n; } else { r.m = bt.n; r.n = bt.m; }
  if (M == N && r.n < r.m) std::swap(r.m, r.n);
  r.cut = cut2(M, N, r.m, r.n);
  return r;
}
Grid3 sweep3(int size, int M, int N, int P) {
  Grid3 g;
  g.m = snap(size, (int)(0.5 + std::pow(((double)M * (double)M) / ((double)N * (double)P) * (double)size, 1. / 3.)));
  { Grid2 h = best2(size / g.m, N, P); g.n = h.m; g.p = h.n; }
  int C = cut3(M, N, P, g.m, g.n, g.p);
  for (int mm = g.m; mm >= 1; --mm) {
    if (size % mm) continue;
    Grid2 h = best2(size / mm, N, P);
    int CC = cut3(M, N, P, mm, h.m, h.n);
    if (CC < C) { g.m = mm; g.n = h.m; g.p = h.n; C = CC; }
  }
  for (int nn = g.n; nn >= 1; --nn) {
    if (size % nn) continue;
    Grid2 h = best2(size / nn, M, P);
    int CC = cut3(M, N, P, h.m, nn, h.n);
    if (CC < C) { g.m = h.m; g.n = nn; g.p = h.n; C = CC; }
  }
  for (int pp = g.p; pp >= 1; --pp) {
    if (size % pp) continue;
    Grid2 h = best2(size / pp, M, N);
    int CC = cut3(M, N, P, h.m, h.n, pp);
    if (CC < C) { g.m = h.m; g.n = h.n; g.p = pp; C = CC; }
  }
  g.cut = cut3(M, N, P, g.m, g.n, g.p);
  return g;
}
void best3(int size, int M, int N, int P, int &m, int &n, int &p) {
  Grid3 a = sweep3(size, M, N, P), b = sweep3(size, N, M, P), c = sweep3(size, P, M, N);
  int mm[3] = {a.m, b.n, c.n}, nn[3] = {a.n, b.m, c.p}, pp[3] = {a.p, b.p, c.m}, C[3] = {a.cut, b.cut, c.cut};
  int best = 0, Cmin = INT_MAX;
  for (int k = 0; k < 3; ++k) if (C[k] < Cmin) { Cmin = C[k]; best = k; }
  m = mm[best]; n = nn[best]; p = pp[best];
  if (M == N && n < m) std::swap(m, n);
  if (M == P && p < m) std::swap(m, p);
  if (N == P && p < n) std::swap(n, p);
}
}  // namespace

int partition(int size, int rank, int dim, const int N[3], int n[3], int coords[3]) {
  if (size < 1 || rank < 0 || rank >= size) return IGX_ERR_ARG_OUTOFRANGE;
  if (dim == 3) {
    int &m = n[0], &q = n[1], &p = n[2];
    if (m < 1 && q < 1 && p < 1) best3(size, N[0], N[1], N[2], m, q, p);
    else if (m < 1 && q < 1) { Grid2 g = best2(size / p, N[0], N[1]); m = g.m; q = g.n; }
    else if (m < 1 && p < 1) { Grid2 g = best2(size / q, N[0], N[2]); m = g.m; p = g.n; }
    else if (q < 1 && p < 1) { Grid2 g = best2(size / m, N[1], N[2]); q = g.m; p = g.n; }
    else if (m < 1) m = size / (q * p);
    else if (q < 1) q = size / (m * p);
    else if (p < 1) p = size / (m * q);
  } else if (dim == 2) {
    if (n[0] < 1 && n[1] < 1) { Grid2 g = best2(size, N[0], N[1]); n[0] = g.m; n[1] = g.n; }
    else if (n[0] < 1) n[0] = size / n[1];
    else if (n[1] < 1) n[1] = size / n[0];
  } else if (dim == 1) {
    if (n[0] < 1) n[0] = size;
  } else return IGX_ERR_ARG_OUTOFRANGE;
  int prod = 1;
  for (int k = 0; k < dim; ++k) prod *= n[k];
  if (prod != size) return IGX_ERR_ARG_OUTOFRANGE;
  for (int k = 0; k < dim; ++k) if (N[k] < n[k]) return IGX_ERR_ARG_OUTOFRANGE;
  for (int k = 0; k < dim; ++k) { coords[k] = rank % n[k]; rank = (rank - coords[k]) / n[k]; }
  return 0;
}

void distribute(int dim, const int size[3], const int rank[3], const int N[3], int n[3], int s[3]) {   // src/petigapart.c:170-202
  for (int k = 0; k < dim; ++k) {
    const int q = N[k] / size[k], r = N[k] % size[k];
    n[k] = q + (r > rank[k] ? 1 : 0);
    s[k] = rank[k] * q + std::min(rank[k], r);
  }
}

// ------------------------------------------------------------------ stencil of a basis function (src/petigamat.c:197-233)
void stencil(const Axis &ax, int i, int *first, int *last) {
  const int p = ax.p, m = ax.m, n = m - p - 1;
  const double *U = ax.U.data();
  *first = next_knot(m, U, i, +1) - p - 1;
  *last = next_knot(m, U, i + p + 1, -1);
  if (!ax.periodic) {
    if (i <= p) *first = 0;
    if (i >= n - p) *last = n;
  } else if (i == 0) {
    const int k = n + 1, j = next_knot(m, U, k, +1), s = j - k, C = p - s, nnp = n - C;
    *first = next_knot(m, U, nnp, +1) - nnp - p - 1;
  }
}

// ------------------------------------------------------------------ IGASetUp
// The ghost-row exchange (exchange.hpp) moves a rank's ghost rows to its +1 neighbour on each axis.  That is every owner
// only while no rank's ghost layer reaches past its neighbour's owned nodes, i.e. while every rank of a split axis owns at
// least as many nodes as its lower neighbour has ghosts (fewer than p elements per rank breaks it: the reference's PETSc
// stash would route such rows two ranks up).  Refused by the exchange entry points rather than summed into the wrong rows.
int exchange_supported(const Space &s, std::string &err) {
  // Ghost rows go to their true owners however thin the ranks are (exchange.hpp: one message per rank the ghost layer reaches).
  // What cannot be served: a periodic axis whose ghost layer reaches around to the sender itself (fewer nodes on the other
  // ranks together than one ghost layer).
  for (int i = 0; i < s.dim; ++i) {
    const Axis &ax = s.axis[i];
    const int np = s.proc_sizes[i], nel = s.elem_sizes[i], p = ax.p;
    if (np == 1 || !ax.periodic) continue;
    auto ranges = [&](int c, int &lw, int &gw) {   // node ranges of the rank with coordinate c on this axis (space_setup)
      const int q = nel / np, r = nel % np, ew = q + (r > c ? 1 : 0), es = c * q + std::min(c, r), el = es + ew - 1;
      const int lstart = ax.span[es] - p, gend = ax.span[el] + 1;
      const int lend = (el < nel - 1) ? ax.span[el + 1] - p : ax.span[el] + 1;
      lw = (c == np - 1) ? ax.nnp - lstart : lend - lstart; gw = gend - lstart;
    };
    for (int c = 0; c < np; ++c) {
      int lw, gw; ranges(c, lw, gw);
      int others = 0;
      for (int k = 1; k < np; ++k) { int lwn, gwn; ranges((c + k) % np, lwn, gwn); others += lwn; }
      if (gw - lw > others) {
        err = "axis " + std::to_string(i) + ": the ghost layer of a rank reaches around the periodic axis to the rank itself; use fewer processors on this axis";
        return IGX_ERR_SUP;
      }
    }
  }
  return 0;
}

int space_setup(Space &s, std::string &err) {
  const int dim = s.dim;
  if (dim < 1 || dim > 3) { err = "Must call IGASetDim() first"; return IGX_ERR_ARG_WRONGSTATE; }
  if (s.dof < 1) { err = "Must call IGASetDof() first"; return IGX_ERR_ARG_WRONGSTATE; }
  for (int i = 0; i < dim; ++i) {
    if (s.axis[i].p < 1) { err = "Must call IGAAxisSetDegree() first"; return IGX_ERR_ORDER; }
    if (s.axis[i].m < 2 * s.axis[i].p + 1) { err = "Must call IGAAxisSetKnots() first"; return IGX_ERR_ORDER; }
    if (s.axis[i].span.empty()) axis_finish(s.axis[i]);
  }
  int N[3] = {1, 1, 1};
  for (int i = 0; i < dim; ++i) N[i] = s.axis[i].nel;
  int n[3] = {s.proc_req[0], s.proc_req[1], s.proc_req[2]}, c[3] = {0, 0, 0};
  if (partition(s.comm_size, s.comm_rank, dim, N, n, c)) { err = "Bad partition"; return IGX_ERR_ARG_OUTOFRANGE; }
  for (int i = 0; i < 3; ++i) { s.proc_sizes[i] = i < dim ? n[i] : 1; s.proc_ranks[i] = i < dim ? c[i] : 0; }
  for (int i = 0; i < dim; ++i) s.elem_sizes[i] = N[i];
  distribute(dim, s.proc_sizes, s.proc_ranks, s.elem_sizes, s.elem_width, s.elem_start);
  for (int i = 0; i < dim; ++i) {   // src/petiga.c:1160-1209
    const Axis &ax = s.axis[i];
    const int nel = N[i], ef = s.elem_start[i], el = ef + s.elem_width[i] - 1, p = ax.p;
    const int lstart = ax.span[ef] - p, gstart = lstart, gend = ax.span[el] + 1;
    const int lend = (el < nel - 1) ? ax.span[el + 1] - p : ax.span[el] + 1;
    s.node_sizes[i] = ax.nnp;
    s.node_lstart[i] = lstart; s.node_lwidth[i] = lend - lstart;
    s.node_gstart[i] = gstart; s.node_gwidth[i] = gend - gstart;
    if (s.proc_ranks[i] == s.proc_sizes[i] - 1) s.node_lwidth[i] = s.node_sizes[i] - s.node_lstart[i];
  }
  for (int i = dim; i < 3; ++i) {
    s.elem_sizes[i] = 1; s.elem_start[i] = 0; s.elem_width[i] = 1;
    s.node_sizes[i] = 1; s.node_lstart[i] = 0; s.node_lwidth[i] = 1; s.node_gstart[i] = 0; s.node_gwidth[i] = 1;
  }
  s.nsd = 0; s.rational = 0; s.geomX.clear(); s.geomW.clear(); s.propA.clear();   // src/petiga.c:1290-1299
  if (s.order < 0) { int o = 0; for (int i = 0; i < dim; ++i) o = std::max(o, s.axis[i].p); s.order = std::min(std::max(o, 1), 4); }
  for (int i = 0; i < dim; ++i) {
    const int q = s.rule_nqp[i] > 0 ? s.rule_nqp[i] : s.axis[i].p + 1;   // src/petigabasis.c:103
    if (int rc = basis_init(s.basis[i], s.axis[i], s.rule[i], q, err)) return rc;
  }
  for (int i = dim; i < 3; ++i) {   // a collapsed axis: one element, one point, the constant 1
    Basis1D &b = s.basis[i];
    b.nel = 1; b.nqp = 1; b.nen = 1;
    b.offset.assign(1, 0); b.detJac.assign(1, 1.0); b.weight.assign(1, 1.0); b.point.assign(1, 0.0);
    b.value.assign(5, 0.0); b.value[0] = 1.0;
    s.axis[i] = Axis();
  }
  if (int rc = space_layout(s, err)) return rc;
  s.setup = true;
  return 0;
}

// ------------------------------------------------------------------ per-axis index layout of the local matrix
// Rows: the ghosted node box [gstart, gstart+gwidth) (src/petiga.c:1172-1208); a periodic axis held by a
// single rank wraps onto [0,nnp) (src/petigagrid.c:158-163).  Columns: the union of the rows' stencils
// (src/petigamat.c:243-267), sorted as PETSc stores an AIJ/BAIJ row (ascending column index).
int space_layout(Space &s, std::string &err) {
  for (int d = 0; d < 3; ++d) {
    AxisLayout &L = s.lay[d];
    L = AxisLayout();
    if (d >= s.dim) {
      L.p = 0; L.gstart = 0; L.gwidth = 1; L.nrow = 1; L.ncol = 1;
      L.rowmap = {0}; L.rownode = {0}; L.colnode = {0}; L.rcnt = {1}; L.rcol = {0}; L.P = {0}; L.owned = {1};
      L.ncolors = 1; L.color = {0};
      continue;
    }
    const Axis &ax = s.axis[d];
    const int p = ax.p, nnp = ax.nnp, W = 2 * p + 1;
    L.p = p; L.gstart = s.node_gstart[d]; L.gwidth = s.node_gwidth[d];
    L.alias = (ax.periodic && s.proc_sizes[d] == 1) ? 1 : 0;
    // A periodic axis with fewer than 2p+1 basis functions: the stencil of a row wraps onto itself and the reference's Mat adds
    // the duplicate columns (ghost indices through the LGMap, src/petigamat.c:243-267).  Held by one rank the row keeps its
    // distinct columns and P sends every duplicate to the same position; the elements of such an axis get one colour each
    // (below).  Still refused: fewer than p+1 functions (an element's own basis functions would alias each other) and the
    // axis split over ranks (a rank could not even hold its ghost layer, exchange_supported()).
    if (ax.periodic && nnp < (L.alias ? p + 1 : W)) { err = L.alias ? "periodic axis needs at least p+1 basis functions" : "periodic axis split over ranks needs at least 2p+1 basis functions"; return IGX_ERR_SUP; }
    auto wrapn = [&](int i) { int r = i % nnp; return r < 0 ? r + nnp : r; };
    auto st = [&](int I, int &f, int &l) {   // stencil of the (possibly unwrapped) node I, unwrapped
      if (!ax.periodic) { stencil(ax, I, &f, &l); return; }
      const int w = wrapn(I), shift = I - w;
      stencil(ax, w, &f, &l); f += shift; l += shift;
    };
    L.rowmap.resize(L.gwidth);
    if (L.alias) {
      L.nrow = nnp; L.ncol = nnp; L.cstart = 0;
      for (int i = 0; i < L.gwidth; ++i) L.rowmap[i] = wrapn(L.gstart + i);
      L.rownode.resize(nnp); L.colnode.resize(nnp);
      for (int i = 0; i < nnp; ++i) { L.rownode[i] = i; L.colnode[i] = i; }
    } else {
      L.nrow = L.gwidth;
      int f0, l0, f1, l1;
      st(L.gstart, f0, l0); st(L.gstart + L.gwidth - 1, f1, l1);
      L.cstart = f0; L.ncol = l1 - f0 + 1;
      L.rownode.resize(L.nrow); L.colnode.resize(L.ncol);
      for (int i = 0; i < L.gwidth; ++i) { L.rowmap[i] = i; L.rownode[i] = ax.periodic ? wrapn(L.gstart + i) : L.gstart + i; }
      for (int j = 0; j < L.ncol; ++j) L.colnode[j] = ax.periodic ? wrapn(L.cstart + j) : L.cstart + j;
    }
    L.rcnt.assign(L.nrow, 0); L.rcol.assign((size_t)L.nrow * W, -1); L.owned.assign(L.nrow, 0);
    L.P.assign((size_t)L.gwidth * W, -1);
    for (int i = 0; i < L.gwidth; ++i) {
      const int I = L.gstart + i, r = L.rowmap[i];
      int f, l; st(I, f, l);
      if (l - f + 1 > W) { err = "stencil wider than 2p+1"; return IGX_ERR_PLIB; }
      std::vector<int> cols;
      for (int Jn = f; Jn <= l; ++Jn) cols.push_back(L.alias ? wrapn(Jn) : Jn - L.cstart);
      std::vector<int> sorted = cols;
      std::sort(sorted.begin(), sorted.end());
      sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
      L.rcnt[r] = (int)sorted.size();
      for (size_t k = 0; k < sorted.size(); ++k) L.rcol[(size_t)r * W + k] = sorted[k];
      for (int dlt = 0; dlt < W; ++dlt) {
        const int Jn = I + dlt - p;
        if (Jn < f || Jn > l) continue;
        const int c = L.alias ? wrapn(Jn) : Jn - L.cstart;
        L.P[(size_t)i * W + dlt] = (int)(std::lower_bound(sorted.begin(), sorted.end(), c) - sorted.begin());
      }
      // ownership: [lstart, lstart+lwidth) on this axis (src/petiga.c:1172-1208); aliased rows are all owned
      const int ls = s.node_lstart[d], lw = s.node_lwidth[d];
      L.owned[r] = L.alias ? 1 : ((I >= ls && I < ls + lw) ? 1 : 0);
    }
    // element colours: e mod (p+1); elements e, e' with e'-e >= p+1 never share a basis function because
    // offset[e] strictly increases.  On an aliased periodic axis the trailing N mod (p+1) elements would
    // meet element 0's colour through the wrap, so each gets a colour of its own.
    const int nel = s.elem_width[d], stride = p + 1;
    L.color.resize(nel);
    int tail = L.alias ? nel % stride : 0;
    if (L.alias && nel < 2 * stride) tail = nel;   // tiny periodic axes: one colour per element
    const int regular = nel - tail;
    for (int e = 0; e < nel; ++e) L.color[e] = e < regular ? e % stride : std::min(regular, stride) + (e - regular);
    L.ncolors = std::min(regular, stride) + tail;
    if (L.ncolors < 1) L.ncolors = 1;
  }
  return 0;
}

// ------------------------------------------------------------------ transfer between nested spline spaces (IGXTransferCreate)
// Row i of T holds the coefficients of the coarse functions in the fine function i's dual functional: the blossom of the coarse spline's
// polynomial piece on the coarse span [u_mu, u_mu+1) that holds the fine knot t_i, at the fine knots t_i+1 .. t_i+p.  It is evaluated by de
// Boor's triangle on the unit vectors, with the arguments taken from t_i+p down to t_i+1: at level k every weight
// (x - u_j) / (u_j+p+1-k - u_j) then lies in [0, 1] (u_mu <= t_i <= x = t_i+p+1-k <= u_mu+p+1-k, the coarse knots being fine knots too), so a
// row is p levels of convex combinations whatever the number of inserted knots, weights of exactly 0 and 1 leave exact zeros and ones (an
// unrefined axis gives the identity, a clamped end the unit row), and no chain of single insertions is applied.
// A periodic axis is built on the unwrapped knot sequence: the knots of one period, U[p+1 .. p+nnp], continued to any index by the same
// formula on both axes (so that equal knots stay equal); the row of the fine function i < nnp over unwrapped coarse columns is folded
// column by column with j mod nc, the closed form of the row map (AxisLayout::rowmap).  Set-up grants nnp >= p + 1, so a row's columns
// stay distinct.  The caller has checked: same degree and periodicity, a non-periodic axis clamped.
int transfer_axis_setup(const Axis &c, const Axis &f, int axis, TransferAxis &t, std::string &err) {
  const int p = f.p, mc = c.m, mf = f.m, per = f.periodic ? 1 : 0;
  const std::string where = "axis " + std::to_string(axis) + ": ";
  const double a = f.U[p], b = f.U[mf - p], L = b - a;
  bool ends = c.U[p] == a && c.U[mc - p] == b;
  if (!per) for (int k = 0; k <= p; ++k) ends = ends && c.U[k] == f.U[k] && c.U[mc - k] == f.U[mf - k];
  if (!ends) { err = where + "the spaces are not nested: the end knots differ"; return IGX_ERR_ARG_OUTOFRANGE; }
  {   // every coarse knot (periodic: of one period) with at least its multiplicity
    const double *Kc = per ? c.U.data() + p + 1 : c.U.data(), *Kf = per ? f.U.data() + p + 1 : f.U.data();
    const int nkc = per ? c.nnp : mc + 1, nkf = per ? f.nnp : mf + 1;
    for (int ic = 0, jf = 0; ic < nkc;) {
      const double v = Kc[ic]; int mcv = 0, mfv = 0;
      while (ic < nkc && Kc[ic] == v) { ++mcv; ++ic; }
      while (jf < nkf && Kf[jf] < v) ++jf;
      while (jf < nkf && Kf[jf] == v) { ++mfv; ++jf; }
      if (mfv < mcv) {
        char buf[256];
        if (!mfv) snprintf(buf, sizeof(buf), "the spaces are not nested: the coarse knot %.17g is missing in the fine axis", v);
        else snprintf(buf, sizeof(buf), "the spaces are not nested: the coarse knot %.17g has multiplicity %d, in the fine axis %d", v, mcv, mfv);
        err = where + buf; return IGX_ERR_ARG_OUTOFRANGE;
      }
    }
  }
  auto ext = [&](const Axis &A, int j) -> double {      // the periodic knot sequence at any index
    const int nn = A.nnp, q = j - (p + 1), k = q >= 0 ? q / nn : -((-q + nn - 1) / nn), r = q - k * nn;
    const double v = A.U[p + 1 + r];
    if (!k) return v;
    return k < 0 ? a - ((double)(-k - 1) * L + (b - v)) : b + ((double)(k - 1) * L + (v - a));
  };
  auto cu = [&](int j) -> double { return per ? ext(c, j) : c.U[j]; };
  auto tf = [&](int i) -> double { return per ? ext(f, i) : f.U[i]; };
  const int nf = f.nnp, nc = c.nnp, W = p + 1, ncl = mc - p - 1;      // ncl: the last coarse function of a clamped axis
  t.p = p; t.nf = nf; t.nc = nc; t.width = W; t.periodic = per;
  t.first.assign(nf, 0); t.count.assign(nf, 0); t.ufirst.assign(nf, 0); t.T.assign((size_t)nf * W, 0.0);
  int mu = per ? -(nc + p + 1) : p;
  double D[8][8];
  for (int i = 0; i < nf; ++i) {
    const double t0 = tf(i);
    while ((per || mu + 1 <= ncl) && cu(mu + 1) <= t0) ++mu;
    for (int r = 0; r <= p; ++r) for (int q = 0; q <= p; ++q) D[r][q] = r == q ? 1.0 : 0.0;
    for (int k = 1; k <= p; ++k) {
      const double x = tf(i + p + 1 - k);
      for (int jj = p; jj >= k; --jj) {
        const int j = mu - p + jj;
        const double uj = cu(j), w = (x - uj) / (cu(j + p + 1 - k) - uj), w1 = 1.0 - w;
        for (int q = 0; q <= p; ++q) D[jj][q] = w1 * D[jj - 1][q] + w * D[jj][q];
      }
    }
    int lo = 0, hi = p;
    while (lo < p && D[p][lo] == 0.0) ++lo;
    while (hi > lo && D[p][hi] == 0.0) --hi;
    t.ufirst[i] = mu - p + lo; t.count[i] = hi - lo + 1;
    for (int k = 0; k <= hi - lo; ++k) t.T[(size_t)i * W + k] = D[p][lo + k];
  }
  if (per) {
    const int u0 = t.ufirst[0], shift = (u0 >= 0 ? u0 / nc : -((-u0 + nc - 1) / nc)) * nc;
    for (int i = 0; i < nf; ++i) t.ufirst[i] -= shift;
  }
  for (int i = 0; i < nf; ++i) {
    if (t.ufirst[i] < 0 || (!per && t.ufirst[i] + t.count[i] > nc)) { err = where + "a row of the transfer table leaves the coarse axis"; return IGX_ERR_PLIB; }
    t.first[i] = t.ufirst[i] % nc;
  }
  t.identity = nf == nc;
  for (int i = 0; i < nf && t.identity; ++i) t.identity = t.count[i] == 1 && t.first[i] == i && t.T[(size_t)i * W] == 1.0;
  // the rows as CSR with folded columns, and the transpose by counting: fine rows ascending in every coarse row
  t.pptr.assign(nf + 1, 0); t.rptr.assign(nc + 1, 0);
  for (int i = 0; i < nf; ++i) t.pptr[i + 1] = t.pptr[i] + t.count[i];
  t.pidx.resize(t.pptr[nf]); t.pval.resize(t.pptr[nf]);
  for (int i = 0; i < nf; ++i) for (int k = 0; k < t.count[i]; ++k) {
    const int col = (t.first[i] + k) % nc;
    t.pidx[t.pptr[i] + k] = col; t.pval[t.pptr[i] + k] = t.T[(size_t)i * W + k];
    ++t.rptr[col + 1];
  }
  for (int j = 0; j < nc; ++j) t.rptr[j + 1] += t.rptr[j];
  t.ridx.resize(t.rptr[nc]); t.rval.resize(t.rptr[nc]);
  std::vector<int> fill(t.rptr.begin(), t.rptr.end() - 1);
  for (int i = 0; i < nf; ++i) for (int e = t.pptr[i]; e < t.pptr[i + 1]; ++e) { const int at = fill[t.pidx[e]]++; t.ridx[at] = i; t.rval[at] = t.pval[e]; }
  return 0;
}

}  // namespace igx
