// engine.hip -- the main unit of libpetiga_amd's device side: the C ABI, table upload, sparsity pattern, the drivers, the Gram walks and,
// from solve_loops.hpp on, the loops.  One translation unit on purpose ("The units"): a kernel's machine code here depends on
// what else is in its unit.  The element kernels are instantiated in the dispatch units (dispatch_unit.hip).
// Reference citations are file:line of dalcinl/PetIGA @ 2025-04-04.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>
#include "igx.hpp"
#include "generic_kernel.hpp"
#include "feature_mfma.hpp"
#include "first_touch.hpp"
#include "element_sweep.hpp"
#include "block_diag.hpp"
#include "fast_diag.hpp"
#include "pencil_launch.hpp"      // (the Gram walks: gram_mfma.hpp, gram_patch.hpp, gram_patch3.hpp, boundary_loads.hpp, pencil_stamps.hpp and their host side)
#include "block_pencil.hpp"      // (the host launcher, for run-time forms: rtc.hpp; no kernel of it is instantiated in this unit)
#include "band_pt.hpp"           // (likewise: band_pt_run)
#include "engine_objects.hpp"

extern "C" const char *IGXGetLastError(void) { return g_err.c_str(); }

// ------------------------------------------------------------------ set-up mirror
extern "C" int IGXCreate(IGX *iga) { if (!iga) return fail(IGX_ERR_ARG_WRONG, "null pointer"); *iga = new _p_IGX(); igx_pool_acquire(); return 0; }
extern "C" int IGXDestroy(IGX *iga) {
  if (!iga || !*iga) return 0;
  (*iga)->comm.reset();       // (synchronises its exchange stream first)
  for (auto &e : (*iga)->ev) if (e) (void)hipEventDestroy(e);
  if ((*iga)->slab_ev) (void)hipEventDestroy((*iga)->slab_ev);
  for (int k = 0; k < 2; ++k) if ((*iga)->face_ev[k]) (void)hipEventDestroy((*iga)->face_ev[k]);
  delete *iga; *iga = nullptr;
  igx_pool_release();          // the last one out hands the launch-scoped pool back to the driver
  return 0;
}
static void touch(IGX g) { g->s.setup = false; g->on_device = false; }
static void drop_net(IGX g) { g->s.netX.clear(); g->s.netW.clear(); g->s.net_nsd = 0; g->s.netA.clear(); g->s.npd = 0; }

extern "C" int IGXSetDim(IGX g, int dim) { NEEDIGA(g); if (dim < 1 || dim > 3) return fail(IGX_ERR_ARG_OUTOFRANGE, "Number of parametric dimensions must be in range [1,3]"); g->s.dim = dim; touch(g); return 0; }
extern "C" int IGXSetDof(IGX g, int dof) { NEEDIGA(g); if (dof < 1) return fail(IGX_ERR_ARG_OUTOFRANGE, "Number of DOFs per node must be greater than one"); if (dof > MAXBC) return fail(IGX_ERR_SUP, "device path supports dof <= 8"); g->s.dof = dof; touch(g); return 0; }
extern "C" int IGXSetOrder(IGX g, int order) { NEEDIGA(g); if (order < 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "Order must be nonnegative"); g->s.order = order < 1 ? 1 : (order > 4 ? 4 : order); return 0; }
extern "C" int IGXSetQuadrature(IGX g, int i, int q) { AXISCK(g, i); if (q == IGX_DECIDE && g->s.axis[i].p > 0) q = g->s.axis[i].p + 1; if (q <= 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "Number of quadrature points must be positive"); g->s.rule_nqp[i] = q; touch(g); return 0; }
extern "C" int IGXSetRuleType(IGX g, int i, IGXRuleType type) {
  AXISCK(g, i);
  if ((int)type < 0 || (int)type > 3) return fail(IGX_ERR_ARG_OUTOFRANGE, "unknown rule type");
  if (g->s.rule[i].type == (int)type) return 0;
  if (type == IGX_RULE_USER) return fail(IGX_ERR_ARG_WRONGSTATE, "a user-defined rule is set with IGXSetRule");
  g->s.rule[i].type = (int)type; g->s.rule[i].x.clear(); g->s.rule[i].w.clear(); touch(g); return 0;
}
extern "C" int IGXSetRuleSize(IGX g, int i, int nqp) {
  AXISCK(g, i);
  if (nqp < 1) return fail(IGX_ERR_ARG_OUTOFRANGE, "Number of quadrature points must be greater than zero");
  if (g->s.rule[i].type == IGX_RULE_USER && (int)g->s.rule[i].x.size() != nqp) return fail(IGX_ERR_ARG_WRONGSTATE, "the size of a user-defined rule is set with IGXSetRule");
  g->s.rule_nqp[i] = nqp; touch(g); return 0;
}
extern "C" int IGXSetRule(IGX g, int i, int q, const double x[], const double w[]) {
  AXISCK(g, i);
  if (q < 1) return fail(IGX_ERR_ARG_OUTOFRANGE, "Number of quadrature points must be greater than zero");
  if (!x || !w) return fail(IGX_ERR_ARG_WRONG, "null rule");
  g->s.rule[i].type = IGX_RULE_USER; g->s.rule[i].x.assign(x, x + q); g->s.rule[i].w.assign(w, w + q); g->s.rule_nqp[i] = q; touch(g); return 0;
}
extern "C" int IGXGetRule(IGX g, int i, int *q, double x[], double w[]) {
  AXISCK(g, i);
  const int n = g->s.rule_nqp[i] > 0 ? g->s.rule_nqp[i] : g->s.axis[i].p + 1;      // src/petigabasis.c:103
  if (q) *q = n;
  if (!x && !w) return 0;
  std::vector<double> X(std::max(n, 10)), W(std::max(n, 10));
  std::string e;
  if (int rc = rule_setup(g->s.rule[i], n, X.data(), W.data(), e)) return fail(rc, e);
  for (int k = 0; k < n; ++k) { if (x) x[k] = X[k]; if (w) w[k] = W[k]; }
  return 0;
}
extern "C" int IGXSetProcessors(IGX g, int i, int n) { AXISCK(g, i); g->s.proc_req[i] = n; touch(g); return 0; }
extern "C" int IGXSetComm(IGX g, int size, int rank) { NEEDIGA(g); if (size < 1 || rank < 0 || rank >= size) return fail(IGX_ERR_ARG_OUTOFRANGE, "bad communicator size/rank"); g->s.comm_size = size; g->s.comm_rank = rank; touch(g); return 0; }
extern "C" int IGXAxisSetDegree(IGX g, int i, int p) { AXISCK(g, i); if (p < 1) return fail(IGX_ERR_ARG_OUTOFRANGE, "Polynomial degree must be greater than zero"); if (p > 7) return fail(IGX_ERR_SUP, "degree > 7 not supported"); g->s.axis[i].p = p; touch(g); drop_net(g); return 0; }
extern "C" int IGXAxisSetPeriodic(IGX g, int i, int flag) { AXISCK(g, i); g->s.axis[i].periodic = flag ? 1 : 0; touch(g); return 0; }
extern "C" int IGXAxisInitUniform(IGX g, int i, int N, double Ui, double Uf, int C) { AXISCK(g, i); std::string e; int rc = axis_init_uniform(g->s.axis[i], N, Ui, Uf, C, e); touch(g); drop_net(g); return rc ? fail(rc, e) : 0; }
extern "C" int IGXAxisSetKnots(IGX g, int i, int m, const double U[]) { AXISCK(g, i); if (!U) return fail(IGX_ERR_ARG_WRONG, "null knots"); std::string e; int rc = axis_set_knots(g->s.axis[i], m, U, e); touch(g); drop_net(g); return rc ? fail(rc, e) : 0; }
static int apply_geometry(IGX g);
static int apply_property(IGX g);
extern "C" int IGXSetUp(IGX g) {
  NEEDIGA(g); std::string e; int rc = space_setup(g->s, e); g->on_device = false; ++g->setup_gen; g->fd.reset(); g->krylov.reset(); g->newton.reset(); g->timestep.reset(); g->eigen.reset(); g->self_timed.clear();
  if (rc) return fail(rc, e);
  if (int rp = apply_property(g)) return rp;
  return apply_geometry(g);   // a control net given by IGXRead / an earlier IGXSetGeometry survives re-partitioning
}

// copy the ghosted-local box of the global control net (what IGALoadGeometry's scatters produce, src/petigaio.c:240-275)
static int apply_geometry(IGX g) {
  Space &s = g->s;
  const int nsd = s.net_nsd;
  if (!nsd) return 0;
  if (nsd < s.dim || nsd > 3) return fail(IGX_ERR_ARG_OUTOFRANGE, "Number of space dimensions must be in range [dim,3]");
  int gs[3] = {1, 1, 1};
  for (int i = 0; i < s.dim; ++i) gs[i] = s.axis[i].span[s.axis[i].nel - 1] + 1;
  const size_t nnet = (size_t)gs[0] * gs[1] * gs[2];
  if (s.netX.size() != nnet * nsd) return fail(IGX_ERR_ARG_WRONG, "control net does not match the knot vectors");
  const bool hasW = !s.netW.empty();
  const int *g0 = s.node_gstart, *gw = s.node_gwidth;
  s.geomX.assign((size_t)gw[0] * gw[1] * gw[2] * nsd, 0.0);
  s.geomW.clear(); if (hasW) s.geomW.assign((size_t)gw[0] * gw[1] * gw[2], 0.0);
  size_t pos = 0;
  for (int k = g0[2]; k < g0[2] + gw[2]; ++k) for (int j = g0[1]; j < g0[1] + gw[1]; ++j) for (int i = g0[0]; i < g0[0] + gw[0]; ++i, ++pos) {
    const size_t gi = (size_t)i + (size_t)gs[0] * ((size_t)j + (size_t)gs[1] * (size_t)k);
    for (int c = 0; c < nsd; ++c) s.geomX[pos * nsd + c] = s.netX[gi * nsd + c];
    if (hasW) s.geomW[pos] = s.netW[gi];
  }
  s.nsd = nsd; s.rational = hasW ? 1 : 0;
  g->on_device = false;
  return 0;
}

// ... and of the property array (IGALoadProperty's scatters, src/petigaio.c:393-458)
static int apply_property(IGX g) {
  Space &s = g->s;
  s.propA.clear();
  if (!s.npd) return 0;
  int gs[3] = {1, 1, 1};
  for (int i = 0; i < s.dim; ++i) gs[i] = s.axis[i].span[s.axis[i].nel - 1] + 1;
  const size_t nnet = (size_t)gs[0] * gs[1] * gs[2], npd = (size_t)s.npd;
  if (s.netA.size() != nnet * npd) return fail(IGX_ERR_ARG_WRONG, "property array does not match the knot vectors");
  const int *g0 = s.node_gstart, *gw = s.node_gwidth;
  s.propA.assign((size_t)gw[0] * gw[1] * gw[2] * npd, 0.0);
  size_t pos = 0;
  for (int k = g0[2]; k < g0[2] + gw[2]; ++k) for (int j = g0[1]; j < g0[1] + gw[1]; ++j) for (int i = g0[0]; i < g0[0] + gw[0]; ++i, ++pos) {
    const size_t gi = (size_t)i + (size_t)gs[0] * ((size_t)j + (size_t)gs[1] * (size_t)k);
    for (size_t c = 0; c < npd; ++c) s.propA[pos * npd + c] = s.netA[gi * npd + c];
  }
  g->on_device = false;
  return 0;
}
// IGASetPropertyDim + the array IGALoadProperty fills (src/petigaio.c:359-458): npd numbers per node of the geometry grid, natural order; npd = 0 drops it
extern "C" int IGXSetProperty(IGX g, int npd, const double A[]) {
  NEEDIGA(g); Space &s = g->s;
  if (!s.setup) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetUp() first");
  if (npd < 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "Number of properties must be nonnegative");
  if (npd > 64) return fail(IGX_ERR_SUP, "device path supports at most 64 properties per node");
  if (npd == 0) { s.npd = 0; s.netA.clear(); return apply_property(g); }
  if (!A) return fail(IGX_ERR_ARG_WRONG, "null property array");
  size_t nnet = 1;
  for (int i = 0; i < s.dim; ++i) nnet *= (size_t)(s.axis[i].span[s.axis[i].nel - 1] + 1);
  s.netA.assign(A, A + nnet * (size_t)npd); s.npd = npd;
  return apply_property(g);
}
extern "C" int IGXGetPropertyDim(IGX g, int *npd) { NEEDIGA(g); if (!npd) return fail(IGX_ERR_ARG_WRONG, "null pointer"); *npd = g->s.npd; return 0; }

extern "C" int IGXSetGeometry(IGX g, int nsd, const double X[], const double W[]) {
  NEEDIGA(g); Space &s = g->s;
  if (!s.setup) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetUp() first");
  if (nsd < s.dim || nsd > 3) return fail(IGX_ERR_ARG_OUTOFRANGE, "Number of space dimensions must be in range [dim,3]");      // (IGASetGeometryDim, src/petigaio.c:187: [1,3]; below dim there is no map)
  if (!X) return fail(IGX_ERR_ARG_WRONG, "null control points");
  size_t nnet = 1;
  for (int i = 0; i < s.dim; ++i) nnet *= (size_t)(s.axis[i].span[s.axis[i].nel - 1] + 1);
  s.netX.assign(X, X + nnet * nsd);
  s.netW.clear(); if (W) s.netW.assign(W, W + nnet);
  s.net_nsd = nsd;
  return apply_geometry(g);
}

static int bc_set(BC &bc, int field, double value) {   // src/petigaform.c:100-110
  int k; for (k = 0; k < bc.count; ++k) if (bc.field[k] == field) break;
  if (k == bc.count) bc.count++;
  bc.field[k] = field; bc.value[k] = value; return 0;
}
static int bc_args(IGX g, int axis, int side, int field) {
  if (axis < 0 || axis >= (g->s.dim > 0 ? g->s.dim : 3)) return fail(IGX_ERR_ARG_OUTOFRANGE, "Expecting 0<=axis<dim");
  if (side < 0 || side >= 2) return fail(IGX_ERR_ARG_OUTOFRANGE, "Expecting 0<=side<2");
  if (field < 0 || field >= (g->s.dof > 0 ? g->s.dof : 64)) return fail(IGX_ERR_ARG_OUTOFRANGE, "Expecting 0<=field<dof");
  return 0;
}
extern "C" int IGXSetBoundaryValue(IGX g, int axis, int side, int field, double v) { NEEDIGA(g); if (int rc = bc_args(g, axis, side, field)) return rc; return bc_set(g->s.value[axis][side], field, v); }
extern "C" int IGXSetBoundaryLoad(IGX g, int axis, int side, int field, double v) { NEEDIGA(g); if (int rc = bc_args(g, axis, side, field)) return rc; return bc_set(g->s.load[axis][side], field, v); }
extern "C" int IGXClearBoundary(IGX g) { NEEDIGA(g); for (int a = 0; a < 3; ++a) for (int s = 0; s < 2; ++s) { g->s.value[a][s].count = 0; g->s.load[a][s].count = 0; g->s.visit[a][s] = false; } return 0; }
extern "C" int IGXSetBoundaryForm(IGX g, int axis, int side, int flag) {   // IGASetBoundaryForm -> IGAFormSetBoundaryForm, src/petigaform.c:134
  NEEDIGA(g);
  if (axis < 0 || axis >= 3) return fail(IGX_ERR_ARG_OUTOFRANGE, "Index must be in range [0,2]");
  if (side < 0 || side >= 2) return fail(IGX_ERR_ARG_OUTOFRANGE, "Index must be in range [0,1]");
  g->s.visit[axis][side] = flag != 0; return 0;
}
extern "C" int IGXSetForm(IGX g, IGXFormKind kind, const double params[], int nparams) {
  NEEDIGA(g);
  if (nparams < 0 || nparams > MAXPARAM) return fail(IGX_ERR_ARG_OUTOFRANGE, "too many form parameters");
  g->s.form = kind; g->s.params.assign(params ? params : nullptr, params ? params + nparams : nullptr);
  return 0;
}
extern "C" int IGXGetSizes(IGX g, int es[3], int est[3], int ew[3], int ns[3], int nls[3], int nlw[3], int ngs[3], int ngw[3]) {
  NEEDIGA(g); const Space &s = g->s;
  if (!s.setup) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetUp() first");
  for (int i = 0; i < 3; ++i) {
    if (es) es[i] = s.elem_sizes[i]; if (est) est[i] = s.elem_start[i]; if (ew) ew[i] = s.elem_width[i];
    if (ns) ns[i] = s.node_sizes[i]; if (nls) nls[i] = s.node_lstart[i]; if (nlw) nlw[i] = s.node_lwidth[i];
    if (ngs) ngs[i] = s.node_gstart[i]; if (ngw) ngw[i] = s.node_gwidth[i];
  }
  return 0;
}
extern "C" int IGXGetBasis(IGX g, int i, int *nel, int *nqp, int *nen, int offset[], double detJac[], double weight[], double point[], double value[]) {
  AXISCK(g, i); const Space &s = g->s;
  if (!s.setup) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetUp() first");
  const Basis1D &b = s.basis[i];
  if (nel) *nel = b.nel; if (nqp) *nqp = b.nqp; if (nen) *nen = b.nen;
  if (offset) std::copy(b.offset.begin(), b.offset.end(), offset);
  if (detJac) std::copy(b.detJac.begin(), b.detJac.end(), detJac);
  if (weight) std::copy(b.weight.begin(), b.weight.end(), weight);
  if (point) std::copy(b.point.begin(), b.point.end(), point);
  if (value) std::copy(b.value.begin(), b.value.end(), value);
  return 0;
}
extern "C" int IGXGetProcessors(IGX g, int ps[3], int pr[3]) { NEEDIGA(g); for (int i = 0; i < 3; ++i) { if (ps) ps[i] = g->s.proc_sizes[i]; if (pr) pr[i] = g->s.proc_ranks[i]; } return 0; }
extern "C" int64_t IGXGetElementCount(IGX g) { if (!g || !g->s.setup) return 0; return (int64_t)g->s.elem_width[0] * g->s.elem_width[1] * g->s.elem_width[2]; }
extern "C" int IGXGetColoring(IGX g, int nc[3]) { NEEDIGA(g); if (!g->s.setup) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetUp() first"); for (int i = 0; i < 3; ++i) nc[i] = g->s.lay[i].ncolors; return 0; }
extern "C" int IGXGetElementColor(IGX g, int axis, int e) { if (!g || !g->s.setup || axis < 0 || axis > 2 || e < 0 || e >= (int)g->s.lay[axis].color.size()) return -1; return g->s.lay[axis].color[e]; }

extern "C" int IGXCreateFromTables(const IGXTables *t, IGX *out) {
  if (!t || !out) return fail(IGX_ERR_ARG_WRONG, "null pointer");
  std::unique_ptr<_p_IGX> g(new _p_IGX());
  Space &s = g->s;
  if (t->dim < 1 || t->dim > 3 || t->dof < 1 || t->dof > MAXBC) return fail(IGX_ERR_ARG_OUTOFRANGE, "bad dim/dof");
  s.dim = t->dim; s.dof = t->dof; s.order = t->order < 1 ? 1 : (t->order > 4 ? 4 : t->order);
  s.comm_size = 1; s.comm_rank = 0;
  for (int i = 0; i < 3; ++i) {
    s.proc_sizes[i] = i < s.dim ? t->proc_sizes[i] : 1; s.proc_ranks[i] = i < s.dim ? t->proc_ranks[i] : 0;
    s.comm_size *= s.proc_sizes[i];
  }
  for (int i = s.dim - 1; i >= 0; --i) s.comm_rank = s.comm_rank * s.proc_sizes[i] + s.proc_ranks[i];
  for (int i = 0; i < s.dim; ++i) {
    const IGXAxisTables &a = t->axis[i];
    if (!a.U || !a.span || !a.offset || !a.detJac || !a.weight || !a.point || !a.value) return fail(IGX_ERR_ARG_WRONG, "null axis table");
    Axis &ax = s.axis[i]; ax.p = a.p; ax.m = a.m; ax.periodic = a.periodic; ax.nel = a.nel; ax.nnp = a.nnp;
    if (a.p > 7) return fail(IGX_ERR_SUP, "degree > 7 not supported");
    ax.U.assign(a.U, a.U + a.m + 1); ax.span.assign(a.span, a.span + a.nel);
    Basis1D &b = s.basis[i]; b.nel = a.nel; b.nqp = a.nqp; b.nen = a.nen;
    b.offset.assign(a.offset, a.offset + a.nel); b.detJac.assign(a.detJac, a.detJac + a.nel);
    b.weight.assign(a.weight, a.weight + (size_t)a.nel * a.nqp); b.point.assign(a.point, a.point + (size_t)a.nel * a.nqp);
    b.value.assign(a.value, a.value + (size_t)a.nel * a.nqp * a.nen * 5);
    s.rule_nqp[i] = a.nqp;
  }
  for (int i = s.dim; i < 3; ++i) {
    Basis1D &b = s.basis[i]; b.nel = 1; b.nqp = 1; b.nen = 1;
    b.offset.assign(1, 0); b.detJac.assign(1, 1.0); b.weight.assign(1, 1.0); b.point.assign(1, 0.0); b.value.assign(5, 0.0); b.value[0] = 1.0;
  }
  for (int i = 0; i < 3; ++i) {
    const bool in = i < s.dim;
    s.elem_sizes[i] = in ? t->elem_sizes[i] : 1; s.elem_start[i] = in ? t->elem_start[i] : 0; s.elem_width[i] = in ? t->elem_width[i] : 1;
    s.node_sizes[i] = in ? t->node_sizes[i] : 1; s.node_lstart[i] = in ? t->node_lstart[i] : 0; s.node_lwidth[i] = in ? t->node_lwidth[i] : 1;
    s.node_gstart[i] = in ? t->node_gstart[i] : 0; s.node_gwidth[i] = in ? t->node_gwidth[i] : 1;
  }
  std::string e;
  if (int rc = space_layout(s, e)) return fail(rc, e);
  s.setup = true;
  if (t->nsd) {
    if (t->nsd < s.dim || t->nsd > 3) return fail(IGX_ERR_ARG_OUTOFRANGE, "Number of space dimensions must be in range [dim,3]");
    if (!t->geometryX) return fail(IGX_ERR_ARG_WRONGSTATE, "No geometry set");
    const size_t n = (size_t)s.node_gwidth[0] * s.node_gwidth[1] * s.node_gwidth[2];
    s.geomX.assign(t->geometryX, t->geometryX + n * t->nsd); s.nsd = t->nsd;
    if (t->rational) { if (!t->rationalW) return fail(IGX_ERR_ARG_WRONGSTATE, "No geometry set"); s.geomW.assign(t->rationalW, t->rationalW + n); s.rational = 1; }
  }
  if (t->property) {      // iga->property / iga->propertyA
    if (!t->propertyA) return fail(IGX_ERR_ARG_WRONGSTATE, "No property set");
    if (t->property < 0 || t->property > 64) return fail(IGX_ERR_SUP, "device path supports at most 64 properties per node");
    const size_t n = (size_t)s.node_gwidth[0] * s.node_gwidth[1] * s.node_gwidth[2];
    s.npd = t->property; s.propA.assign(t->propertyA, t->propertyA + n * (size_t)t->property);
  }
  *out = g.release(); igx_pool_acquire();
  return 0;
}

// ------------------------------------------------------------------ device upload
static int ensure_device(IGX g) {
  Space &s = g->s;
  if (!s.setup) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetUp() first");
  if (g->on_device) return 0;
  for (int d = 0; d < 3; ++d) {
    const Basis1D &b = s.basis[d]; const AxisLayout &L = s.lay[d];
    const int e0 = s.elem_start[d], ne = s.elem_width[d], nq = b.nqp, na = b.nen;
    std::vector<double> tab((size_t)ne * nq * na * NDER), w((size_t)ne * nq), pt((size_t)ne * nq), J(ne);
    std::vector<int> off(ne);
    for (int e = 0; e < ne; ++e) {
      J[e] = b.detJac[e0 + e]; off[e] = b.offset[e0 + e] - L.gstart;
      for (int q = 0; q < nq; ++q) {
        w[(size_t)e * nq + q] = b.weight[(size_t)(e0 + e) * nq + q]; pt[(size_t)e * nq + q] = b.point[(size_t)(e0 + e) * nq + q];
        for (int a = 0; a < na; ++a) for (int k = 0; k < NDER; ++k)
          tab[(((size_t)e * nq + q) * na + a) * NDER + k] = b.value[(((size_t)(e0 + e) * nq + q) * na + a) * 5 + k];
      }
    }
    std::vector<int64_t> prefix(L.nrow + 1, 0);
    for (int r = 0; r < L.nrow; ++r) prefix[r + 1] = prefix[r] + L.rcnt[r];
    AxisBufs &B = g->ab[d];
    std::vector<double> bnd((size_t)2 * na * NDER, 0.0);
    for (int sd = 0; sd < 2; ++sd) {
      std::vector<double> bv = b.bnd_value[sd];
      if (bv.size() < (size_t)na * 5) {   // axis beyond dim, or tables handed over without the end-of-axis rows: evaluate here
        bv.assign((size_t)na * 5, 0.0);
        const Axis &ax = s.axis[d];
        if (d < s.dim && !ax.U.empty() && !ax.span.empty()) {
          const int k = sd ? ax.span[ax.nel - 1] : ax.span[0];
          bspline_ders(k, sd ? ax.U[k + 1] : ax.U[k], ax.p, std::min(ax.p, 4), ax.U.data(), bv.data());
        } else bv[0] = 1.0;
      }
      for (int a = 0; a < na; ++a) for (int k = 0; k < NDER; ++k) bnd[((size_t)sd * na + a) * NDER + k] = bv[(size_t)a * 5 + k];
    }
    {   // the element kernels take rowmap in closed form (AxisDev::rwrap): i, or i - nnp past the wrap of a rank-local periodic axis
      const int rw = L.alias ? s.axis[d].nnp : 0x7fffffff;
      for (int i = 0; i < L.gwidth; ++i) if (L.rowmap[i] != (i < rw ? i : i - rw)) return fail(IGX_ERR_PLIB, "row map of an axis is not of the closed form the kernels assume");
    }
    std::vector<double> knots; std::vector<int> elof;      // the probe's span search (probe.hpp): the knot vector itself and the element of every span
    if (d < s.dim) {
      const Axis &ax = s.axis[d];
      knots = ax.U; elof.assign(ax.U.size(), -1);
      for (int e = 0; e < ax.nel && e < (int)ax.span.size(); ++e) if (ax.span[e] >= 0 && ax.span[e] < (int)elof.size()) elof[ax.span[e]] = e;
    }
    if (B.knots.upload(knots) || B.elof.upload(elof)) return fail(IGX_ERR_MEM, "device allocation of the knot vectors failed");
    if (B.bnd.upload(bnd) || B.tab.upload(tab) || B.w.upload(w) || B.J.upload(J) || B.pt.upload(pt) || B.off.upload(off) || B.rowmap.upload(L.rowmap) ||
        B.rcnt.upload(L.rcnt) || B.P.upload(L.P) || B.rcol.upload(L.rcol) || B.prefix.upload(prefix))
      return fail(IGX_ERR_MEM, "device allocation of axis tables failed");
  }
  if (g->X.upload(s.geomX) || g->W.upload(s.geomW) || g->A.upload(s.propA)) return fail(IGX_ERR_MEM, "device allocation of geometry failed");
  if (!g->errflag.p) { if (g->errflag.alloc(sizeof(int))) return fail(IGX_ERR_MEM, "device allocation failed"); HIPCK(hipMemset(g->errflag.p, 0, sizeof(int))); }
  g->nbrows = (int64_t)s.lay[0].nrow * s.lay[1].nrow * s.lay[2].nrow;
  {
    int64_t t[3];
    for (int d = 0; d < 3; ++d) { t[d] = 0; for (int r = 0; r < s.lay[d].nrow; ++r) t[d] += s.lay[d].rcnt[r]; }
    g->nblocks = t[0] * t[1] * t[2];
  }
  g->on_device = true;
  return 0;
}

static SpaceDev make_spacedev(IGX g) {
  const Space &s = g->s; SpaceDev S;
  memset(&S, 0, sizeof(S));
  S.dim = s.dim; S.dof = s.dof; S.order = s.order; S.nsd = s.nsd; S.rational = s.rational;
  for (int d = 0; d < 3; ++d) {
    AxisDev &A = S.ax[d]; const AxisBufs &B = g->ab[d]; const AxisLayout &L = s.lay[d];
    A.nel = s.elem_width[d]; A.nqp = s.basis[d].nqp; A.nen = s.basis[d].nen; A.p = L.p;
    A.estart = s.elem_start[d]; A.esizes = s.elem_sizes[d]; A.periodic = d < s.dim ? s.axis[d].periodic : 0;
    A.gwidth = L.gwidth; A.nrow = L.nrow; A.ncol = L.ncol;
    A.tab = B.tab.as<double>(); A.w = B.w.as<double>(); A.J = B.J.as<double>(); A.pt = B.pt.as<double>();
    A.bnd = B.bnd.as<double>();
    if (d < s.dim && !s.axis[d].U.empty() && !s.axis[d].span.empty()) { const Axis &ax = s.axis[d]; A.bndpt[0] = ax.U[ax.span[0]]; A.bndpt[1] = ax.U[ax.span[ax.nel - 1] + 1]; }
    {
      const Basis1D &bd = s.basis[d]; const int e0 = s.elem_start[d], ne = s.elem_width[d];
      A.off_lin = 1; A.off0 = ne > 0 ? bd.offset[e0] - L.gstart : 0;
      for (int e = 0; e < ne; ++e) if (bd.offset[e0 + e] - L.gstart != A.off0 + e) { A.off_lin = 0; break; }
    }
    A.off = B.off.as<int>(); A.rowmap = B.rowmap.as<int>(); A.rwrap = L.alias ? s.axis[d].nnp : 0x7fffffff; A.rcnt = B.rcnt.as<int>(); A.P = B.P.as<int>();
    A.prefix = B.prefix.as<int64_t>(); A.tot = 0; for (int r = 0; r < L.nrow; ++r) A.tot += L.rcnt[r];
  }
  S.X = s.nsd ? g->X.as<double>() : nullptr; S.W = s.rational ? g->W.as<double>() : nullptr;
  S.npd = s.propA.empty() ? 0 : s.npd; S.A = S.npd ? g->A.as<double>() : nullptr;
  for (int a = 0; a < 3; ++a) for (int sd = 0; sd < 2; ++sd) {
    auto cp = [&](const BC &h, BCDev &dv) { dv.count = 0; for (int k = 0; k < h.count && dv.count < MAXBC; ++k) if (h.field[k] < s.dof) { dv.field[dv.count] = h.field[k]; dv.value[dv.count] = h.value[k]; dv.count++; } };
    cp(s.value[a][sd], S.bcv[a][sd]); cp(s.load[a][sd], S.bcl[a][sd]);
  }
  S.fixtable = g->fixtable.as<double>();
  return S;
}

// ------------------------------------------------------------------ sparsity pattern kernels (IGACreateMat, src/petigamat.c:345-549)
struct PatDev { int nrow[3], ncol[3], W[3]; const int *rcnt[3]; const int *rcol[3]; const int64_t *prefix[3]; int64_t tot[3]; };

__global__ void k_browptr(PatDev P, int64_t nbrows, int64_t *browptr) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > nbrows) return;
  if (r == nbrows) { browptr[r] = P.tot[0] * P.tot[1] * P.tot[2]; return; }
  const int r0 = (int)(r % P.nrow[0]), r1 = (int)((r / P.nrow[0]) % P.nrow[1]), r2 = (int)(r / ((int64_t)P.nrow[0] * P.nrow[1]));
  const int64_t c1 = P.rcnt[1][r1], c2 = P.rcnt[2][r2];
  browptr[r] = P.prefix[2][r2] * P.tot[1] * P.tot[0] + c2 * (P.prefix[1][r1] * P.tot[0] + c1 * P.prefix[0][r0]);
}
// one wavefront per row, lanes stride over the row's entries: coalesced 256-byte stores
__global__ void k_bcolidx(PatDev P, int64_t nbrows, const int64_t *browptr, int32_t *bcolidx) {
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= nbrows) return;
  const int lane = threadIdx.x & 63;
  const int r0 = (int)(r % P.nrow[0]), r1 = (int)((r / P.nrow[0]) % P.nrow[1]), r2 = (int)(r / ((int64_t)P.nrow[0] * P.nrow[1]));
  const int c0 = P.rcnt[0][r0], c1 = P.rcnt[1][r1], c2 = P.rcnt[2][r2];
  int32_t *dst = bcolidx + browptr[r];
  const int n = c0 * c1 * c2;
  for (int k = lane; k < n; k += 64) {
    const int k0 = k % c0, k1 = (k / c0) % c1, k2 = k / (c0 * c1);
    dst[k] = P.rcol[0][r0 * P.W[0] + k0] + P.ncol[0] * (P.rcol[1][r1 * P.W[1] + k1] + P.ncol[1] * P.rcol[2][r2 * P.W[2] + k2]);
  }
}

extern "C" int IGXCreateMat(IGX g, IGXMat *mat) {
  NEEDIGA(g); if (!mat) return fail(IGX_ERR_ARG_WRONG, "null pointer");
  if (int rc = ensure_device(g)) return rc;
  const Space &s = g->s;
  if ((int64_t)s.lay[0].ncol * s.lay[1].ncol * s.lay[2].ncol > INT32_MAX) return fail(IGX_ERR_SUP, "more than 2^31 column nodes per rank");
  std::unique_ptr<_p_IGXMat> A(new _p_IGXMat());
  A->iga = g; A->bs = s.dof; A->nbrows = g->nbrows; A->nblocks = g->nblocks; A->gen = g->setup_gen;
  if (A->browptr.alloc((size_t)(A->nbrows + 1) * sizeof(int64_t)) || A->bcolidx.alloc((size_t)A->nblocks * sizeof(int32_t)) ||
      A->val.alloc((size_t)A->nblocks * s.dof * s.dof * sizeof(double)))
    return fail(IGX_ERR_MEM, "device allocation of the matrix failed");
  PatDev P;
  for (int d = 0; d < 3; ++d) {
    P.nrow[d] = s.lay[d].nrow; P.ncol[d] = s.lay[d].ncol; P.W[d] = 2 * s.lay[d].p + 1;
    P.rcnt[d] = g->ab[d].rcnt.as<int>(); P.rcol[d] = g->ab[d].rcol.as<int>(); P.prefix[d] = g->ab[d].prefix.as<int64_t>();
    P.tot[d] = 0; for (int r = 0; r < s.lay[d].nrow; ++r) P.tot[d] += s.lay[d].rcnt[r];
  }
  const int64_t n1 = A->nbrows + 1;
  hipLaunchKernelGGL(k_browptr, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, g->stream, P, A->nbrows, A->browptr.as<int64_t>());
  hipLaunchKernelGGL(k_bcolidx, dim3((unsigned)((A->nbrows + 3) / 4)), dim3(256), 0, g->stream, P, A->nbrows, A->browptr.as<int64_t>(), A->bcolidx.as<int32_t>());
  HIPCK(hipMemsetAsync(A->val.p, 0, A->val.bytes, g->stream));
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(g->stream));
  *mat = A.release();
  return 0;
}
extern "C" int IGXMatDestroy(IGXMat *m) { if (m && *m) { delete *m; *m = nullptr; } return 0; }
extern "C" int IGXMatGetInfo(IGXMat m, int64_t *nbrows, int64_t *nblocks, int *bs) { if (!m) return fail(IGX_ERR_ARG_WRONG, "null matrix"); if (nbrows) *nbrows = m->nbrows; if (nblocks) *nblocks = m->nblocks; if (bs) *bs = m->bs; return 0; }
extern "C" int IGXMatGetDeviceArrays(IGXMat m, const int64_t **rp, const int32_t **ci, double **v) { if (!m) return fail(IGX_ERR_ARG_WRONG, "null matrix"); if (rp) *rp = m->browptr.as<int64_t>(); if (ci) *ci = m->bcolidx.as<int32_t>(); if (v) *v = m->val.as<double>(); return 0; }
extern "C" int IGXMatCopyToHost(IGXMat m, int64_t *rp, int32_t *ci, double *v) {
  if (!m) return fail(IGX_ERR_ARG_WRONG, "null matrix");
  HIPCK(hipStreamSynchronize(m->iga->stream));
  if (rp) HIPCK(hipMemcpy(rp, m->browptr.p, m->browptr.bytes, hipMemcpyDeviceToHost));
  if (ci) HIPCK(hipMemcpy(ci, m->bcolidx.p, m->bcolidx.bytes, hipMemcpyDeviceToHost));
  if (v) HIPCK(hipMemcpy(v, m->val.p, m->val.bytes, hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int IGXMatGetLayout(IGXMat m, int nrow[3], int ncol[3]) { if (!m) return fail(IGX_ERR_ARG_WRONG, "null matrix"); for (int d = 0; d < 3; ++d) { nrow[d] = m->iga->s.lay[d].nrow; ncol[d] = m->iga->s.lay[d].ncol; } return 0; }
extern "C" int IGXMatGetAxisMaps(IGXMat m, int axis, int *rownode, int *colnode) {
  if (!m || axis < 0 || axis > 2) return fail(IGX_ERR_ARG_WRONG, "bad argument");
  const AxisLayout &L = m->iga->s.lay[axis];
  if (rownode) memcpy(rownode, L.rownode.data(), L.rownode.size() * sizeof(int));
  if (colnode) memcpy(colnode, L.colnode.data(), L.colnode.size() * sizeof(int));
  return 0;
}

extern "C" int IGXCreateVec(IGX g, IGXVec *vec) {
  NEEDIGA(g); if (!vec) return fail(IGX_ERR_ARG_WRONG, "null pointer");
  if (int rc = ensure_device(g)) return rc;
  std::unique_ptr<_p_IGXVec> v(new _p_IGXVec());
  v->iga = g; v->n = g->nbrows * g->s.dof;
  if (v->a.alloc((size_t)v->n * sizeof(double))) return fail(IGX_ERR_MEM, "device allocation of the vector failed");
  HIPCK(hipMemset(v->a.p, 0, v->a.bytes));
  *vec = v.release();
  return 0;
}
extern "C" int IGXVecDestroy(IGXVec *v) { if (v && *v) { delete *v; *v = nullptr; } return 0; }
extern "C" int IGXVecGetSize(IGXVec v, int64_t *n) { if (!v) return fail(IGX_ERR_ARG_WRONG, "null vector"); *n = v->n; return 0; }
extern "C" int IGXVecGetDeviceArray(IGXVec v, double **a) { if (!v) return fail(IGX_ERR_ARG_WRONG, "null vector"); *a = v->a.as<double>(); return 0; }
extern "C" int IGXVecCopyToHost(IGXVec v, double *h) { if (!v || !h) return fail(IGX_ERR_ARG_WRONG, "null argument"); HIPCK(hipStreamSynchronize(v->iga->stream)); HIPCK(hipMemcpy(h, v->a.p, v->a.bytes, hipMemcpyDeviceToHost)); return 0; }
extern "C" int IGXVecCopyFromHost(IGXVec v, const double *h) { if (!v || !h) return fail(IGX_ERR_ARG_WRONG, "null argument"); v->iga->slab_valid = false; /* a write after the assembly's face mark (comm.hpp) */ HIPCK(hipStreamSynchronize(v->iga->stream)); HIPCK(hipMemcpy(v->a.p, h, v->a.bytes, hipMemcpyHostToDevice)); return 0; }

extern "C" int IGXSetFixTable(IGX g, IGXVec U) {   // src/petigaform.c:273-298
  NEEDIGA(g);
  if (!U) { g->fixtable.alloc(0); return 0; }
  if (U->iga != g) return fail(IGX_ERR_ARG_WRONG, "vector belongs to another IGX");
  if (g->fixtable.alloc(U->a.bytes)) return fail(IGX_ERR_MEM, "device allocation failed");
  HIPCK(hipStreamSynchronize(g->stream));
  HIPCK(hipMemcpy(g->fixtable.p, U->a.p, U->a.bytes, hipMemcpyDeviceToDevice));
  return 0;
}

// ------------------------------------------------------------------ engine controls
extern "C" int IGXSetStream(IGX g, void *stream) { NEEDIGA(g); g->stream = (hipStream_t)stream; return 0; }
extern "C" int IGXSynchronize(IGX g) {
  NEEDIGA(g);
  HIPCK(hipStreamSynchronize(g->stream));
  if (g->errflag.p) {
    int flag = 0; HIPCK(hipMemcpy(&flag, g->errflag.p, sizeof(int), hipMemcpyDeviceToHost));
    if (flag) { HIPCK(hipMemset(g->errflag.p, 0, sizeof(int))); return fail(flag, "Non-positive det(Jacobian)"); }
  }
  return 0;
}
extern "C" int IGXSetKernel(IGX g, int which) { NEEDIGA(g); if (which < 0 || which > 4) return fail(IGX_ERR_ARG_OUTOFRANGE, "kernel choice must be 0, 1, 2, 3 or 4"); g->kernel_choice = which; return 0; }
extern "C" int IGXGetKernelName(IGX g, char *buf, int len) { NEEDIGA(g); if (!buf || len < 1) return fail(IGX_ERR_ARG_WRONG, "bad buffer"); snprintf(buf, (size_t)len, "%s%s%s%s", g->last_kernel.c_str(), g->rtc_note.empty() ? "" : " [", g->rtc_note.c_str(), g->rtc_note.empty() ? "" : "]"); return 0; }
extern "C" int IGXGetFacePasses(IGX g, int *passes) { NEEDIGA(g); if (passes) *passes = g->dom.passes; return 0; }
extern "C" int IGXSetTiming(IGX g, int flag) {
  NEEDIGA(g); g->timing = flag != 0;
  if (g->timing) for (auto &e : g->ev) if (!e) HIPCK(hipEventCreate(&e));
  return 0;
}
extern "C" int IGXGetLastTiming(IGX g, double *total_ms, double *kernel_ms, int *launches) {
  NEEDIGA(g);
  if (g->timing && g->ev[0] && g->self_timed != g->last_kernel) {      // (after IGXSolve / IGXSolveNonlinear / IGXTimeStep: the figures the call stored)
    HIPCK(hipEventSynchronize(g->ev[3]));
    float a = 0, b = 0;
    HIPCK(hipEventElapsedTime(&a, g->ev[0], g->ev[3]));
    HIPCK(hipEventElapsedTime(&b, g->ev[1], g->ev[2]));
    g->last_total_ms = a; g->last_kernel_ms = b;
  }
  if (total_ms) *total_ms = g->last_total_ms; if (kernel_ms) *kernel_ms = g->last_kernel_ms; if (launches) *launches = g->last_launches;
  return 0;
}
extern "C" int IGXGetDominantKernelTiming(IGX g, char *name, int len, double *ms, int *launches, int64_t *elements, double *flop_per_element) {
  NEEDIGA(g);
  double t = 0;
  if (g->timing && g->ev[4] && g->dom.launches > 0) {
    HIPCK(hipEventSynchronize(g->ev[5]));
    float a = 0; HIPCK(hipEventElapsedTime(&a, g->ev[4], g->ev[5])); t = a;
  }
  if (name && len > 0) snprintf(name, (size_t)len, "%s", g->dom.name.c_str());
  if (ms) *ms = t; if (launches) *launches = g->dom.launches; if (elements) *elements = g->dom.elements;
  if (flop_per_element) *flop_per_element = g->dom.flop_per_element;
  return 0;
}
extern "C" int IGXGetDeviceInfo(char *buf, int len) {
  int dev = 0; hipDeviceProp_t pr;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) { snprintf(buf, (size_t)len, "no HIP device"); return IGX_ERR_LIB; }
  snprintf(buf, (size_t)len, "%s arch=%s CUs=%d clock=%dMHz mem=%.1fGB", pr.name, pr.gcnArchName, pr.multiProcessorCount, pr.clockRate / 1000, pr.totalGlobalMem / 1e9);
  return 0;
}

static int launch_generic_rtc(IGX g, const SpaceDev &S, const OutDev &out, VsMode mode = VsMode::VECTOR);
// entry(dimension, form group) of the unit that holds the space's dimension (dim 3: the three form groups in turn)
template <class Entry>
static int unit_by_dim(IGX g, Entry &&entry) {
  using std::integral_constant;
  switch (g->s.dim) {
  case 1: return entry(integral_constant<int, 1>(), integral_constant<int, -1>());
  case 2: return entry(integral_constant<int, 2>(), integral_constant<int, -1>());
  default: {
    int rc = entry(integral_constant<int, 3>(), integral_constant<int, 0>());
    if (rc == IGX_NOT_MINE) rc = entry(integral_constant<int, 3>(), integral_constant<int, 1>());
    if (rc == IGX_NOT_MINE) rc = entry(integral_constant<int, 3>(), integral_constant<int, 2>());
    return rc;
  }
  }
}
static int dispatch_by_dim(IGX g, const SpaceDev &S, const OutDev &out) { return unit_by_dim(g, [&](auto d, auto gr) { return igx_tu_dispatch(d, gr, g, S, out); }); }
static int matfree_by_dim(IGX g, const SpaceDev &S, const OutDev &out, VsMode mode, const ActionCols *cols) { return unit_by_dim(g, [&](auto d, auto gr) { return igx_tu_matfree(d, gr, g, S, out, mode, cols); }); }

// ------------------------------------------------------------------ the drivers
// The overlap marks of an assembly with a communicator (IGX_OVERLAP): slab_done records "upper face of axis 2 assembled" on the engine
// stream, face_done(axis) the same for axes 1 and 0 (IGX_OVERLAP=2: the mark of axis 2 alone, as in round 3).  Both stay empty without a
// communicator or with the overlap off; slab_valid starts from 0 either way.
static void overlap_marks(IGX g, IGXMat A, IGXVec b, std::function<void()> &slab_done, std::function<void(int)> &face_done) {
  g->slab_valid = 0;
  if (!g->comm || !g->s.env.overlap) return;
  slab_done = [g, A, b]() {
    if (!g->slab_ev && hipEventCreateWithFlags(&g->slab_ev, hipEventDisableTiming) != hipSuccess) return;
    if (hipEventRecord(g->slab_ev, g->stream) == hipSuccess) { g->slab_valid |= 1; g->slab_A = A; g->slab_b = b; }
  };
  if (g->s.env.overlap != 2) face_done = [g, A, b](int axis) {
    if (axis < 0 || axis > 1) return;
    if (!g->face_ev[axis] && hipEventCreateWithFlags(&g->face_ev[axis], hipEventDisableTiming) != hipSuccess) return;
    if (hipEventRecord(g->face_ev[axis], g->stream) == hipSuccess) { g->slab_valid |= (axis == 1 ? 2 : 4); g->slab_A = A; g->slab_b = b; }
  };
}
// fused (IGXComputeFunctionJacobian / IGXComputeIFunctionIJacobian): op is the Jacobian's, b the Function's vector; one pass of the
// walk forms both (state_pencil_kr).  *fused_done = false and nothing written when no fused kernel covers the case: the caller
// then runs the two drivers one after the other.
static int compute(IGX g, int op, IGXMat A, IGXVec b, IGXVec U, IGXVec V, double shift, double t, bool *fused_done = nullptr) {
  NEEDIGA(g);
  if (int rc = ensure_device(g)) return rc;
  const Space &s = g->s;
  if (s.form == IGX_FORM_NONE) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetForm...() first");
  const bool fused = fused_done != nullptr;
  if (fused) {
    *fused_done = false;
    bool ok = s.dim == 3 && s.nsd == 0 && s.axis[0].p == 2 && s.env.state_pencil && s.env.p2_pack != 0 && s.env.fuse_resid != 0 && (g->kernel_choice == 0 || g->kernel_choice == 2) &&
              (s.form == IGX_FORM_CAHNHILLIARD || s.form == IGX_FORM_BRATU);
    for (int d = 0; d < 3 && ok; ++d) for (int sd = 0; sd < 2; ++sd) if (s.load[d][sd].count || s.visit[d][sd]) ok = false;      // (loads: F_e[k] -= flux, src/petigaelem.c:1449-1454 -- the element kernels' business)
    if (!ok) return 0;
  }
  const bool hasM = op_has_matrix(op);
  const bool hasV = fused || op_has_vector(op);
  if (hasM && (!A || A->iga != g)) return fail(IGX_ERR_ARG_WRONG, "matrix missing or created by another IGX");
  if (hasV && (!b || b->iga != g)) return fail(IGX_ERR_ARG_WRONG, "vector missing or created by another IGX");
  if (U && U->iga != g) return fail(IGX_ERR_ARG_WRONG, "state vector created by another IGX");
  if (V && V->iga != g) return fail(IGX_ERR_ARG_WRONG, "state vector created by another IGX");
  OutDev out; memset(&out, 0, sizeof(out));
  out.op = op; out.shift = shift; out.t = t; out.errflag = g->errflag.as<int>(); out.bid = -1;
  out.debug = s.env.debug_feature;
  if (kDebug && (out.debug & 8)) { if (!g->dbgbuf.p) g->dbgbuf.alloc(32 * sizeof(long long)); HIPCK(hipMemsetAsync(g->dbgbuf.p, 0, 32 * sizeof(long long), g->stream)); out.dbg = g->dbgbuf.as<long long>(); }
  if (s.env.clock_probe) { if (!g->clkbuf.p) { if (g->clkbuf.alloc(4 * sizeof(long long))) return fail(IGX_ERR_MEM, "clock probe buffer"); HIPCK(hipMemsetAsync(g->clkbuf.p, 0, 4 * sizeof(long long), g->stream)); } out.clk = g->clkbuf.as<long long>(); }
  if ((s.env.patch3_persist || s.env.rows3) && s.dim == 3 && s.axis[0].p == 3 && !g->patch3_counters.p && g->patch3_counters.alloc(patch3_counter_bytes<PATCH3_MX, PATCH3_MY>())) return fail(IGX_ERR_MEM, "ticket counters of the patch walk");
  if (hasM) { out.browptr = A->browptr.as<int64_t>(); out.val = A->val.as<double>(); }
  if (hasV) out.vec = b->a.as<double>();
  out.U = U ? U->a.as<double>() : nullptr; out.V = V ? V->a.as<double>() : nullptr;
  if (g->timing) HIPCK(hipEventRecord(g->ev[0], g->stream));
  // MatZeroEntries / VecZeroEntries (src/petigaksp.c:166-167)
  // (the matrix is zeroed lazily: the axis-0 pencil walk stores first touches and needs no MatZeroEntries at all)
  bool zeroed = !hasM;
  auto zero_matrix = [&]() { if (!zeroed) { (void)hipMemsetAsync(A->val.p, 0, A->val.bytes, g->stream); zeroed = true; } };
  if (hasV) HIPCK(hipMemsetAsync(b->a.p, 0, b->a.bytes, g->stream));
  if (g->timing) HIPCK(hipEventRecord(g->ev[1], g->stream));
  const SpaceDev S = make_spacedev(g);
  int rc;
  bool done = false;
  g->dom = DomInfo(); g->dom.ev0 = g->timing ? g->ev[4] : nullptr; g->dom.ev1 = g->timing ? g->ev[5] : nullptr;
  if (g->kernel_choice != 1 && g->kernel_choice != 3 && s.form != IGX_FORM_SOURCE) {   // (a run-time form reaches the pencil walk through rtc.hpp)
    std::function<void()> slab_done;
    std::function<void(int)> face_done;
    overlap_marks(g, A, b, slab_done, face_done);
    g->face_done = face_done;
    // the Tangent of a nonlinear scalar form walks the same pencils (pencil_launch.hpp: state_pencil_module)
    PencilModule st;
    const bool tangent = state_pencil_module(s, op, g->kernel_choice, fused, st);
    // (asked for by name, a Tangent on a mapped geometry at another degree is refused with the reason; the automatic choice goes on to the feature kernel)
    if ((op == OP_JACOBIAN || op == OP_IJACOBIAN) && s.dim == 3 && s.nsd == 3 && s.axis[0].p != 2 && g->kernel_choice == 2 && (s.form == IGX_FORM_CAHNHILLIARD || s.form == IGX_FORM_BRATU))
      return fail(IGX_ERR_SUP, "a Tangent on a mapped geometry takes the walk at p = 2 only (state_pencil_geo); the feature kernel covers the other degrees");
    rc = try_gram_mfma(g->s, S, out, g->stream, g->kernel_choice == 2, g->last_kernel, g->last_launches, g_err, done, g->dom, zero_matrix, slab_done, tangent ? &st : nullptr, face_done, g->patch3_counters.as<int>());
    g->face_done = nullptr;
    if (rc) return rc;
  }
  if (fused) {      // (no walk took it -- a non-walkable axis 0, a reduced continuity: the caller falls back to the two drivers)
    *fused_done = done;
    if (g->timing) { HIPCK(hipEventRecord(g->ev[2], g->stream)); HIPCK(hipEventRecord(g->ev[3], g->stream)); }
    return 0;
  }
  if (!done) {
    g->zero_matrix = zero_matrix;      // the feature kernel stores first touches and skips it; everything else zeroes first
    overlap_marks(g, A, b, g->slab_done, g->face_done);      // (the face marks: run-time forms on the pencil walk, rtc.hpp)
    rc = (s.form == IGX_FORM_SOURCE) ? launch_generic_rtc(g, S, out) : dispatch_by_dim(g, S, out);
    g->zero_matrix = nullptr; g->slab_done = nullptr; g->face_done = nullptr;
    if (rc) return rc;
  }
  if (g->timing) { HIPCK(hipEventRecord(g->ev[2], g->stream)); HIPCK(hipEventRecord(g->ev[3], g->stream)); }
  if (kDebug && out.dbg) {
    long long h[32]; HIPCK(hipStreamSynchronize(g->stream)); HIPCK(hipMemcpy(h, g->dbgbuf.p, sizeof(h), hipMemcpyDeviceToHost));
    fprintf(stderr, "[feature stamps]"); for (int i = 1; i < (int)h[31] && i < 31; ++i) fprintf(stderr, " %lld", h[i] - h[i - 1]); fprintf(stderr, "\n");
  }
  return 0;
}

extern "C" int IGXComputeSystem(IGX g, IGXMat A, IGXVec b) { return compute(g, OP_SYSTEM, A, b, nullptr, nullptr, 0, 0); }
extern "C" int IGXComputeMatrix(IGX g, IGXMat A) { return compute(g, OP_MATRIX, A, nullptr, nullptr, nullptr, 0, 0); }
extern "C" int IGXComputeVector(IGX g, IGXVec b) { return compute(g, OP_VECTOR, nullptr, b, nullptr, nullptr, 0, 0); }
extern "C" int IGXComputeFunction(IGX g, IGXVec U, IGXVec F) { if (!U) return fail(IGX_ERR_ARG_WRONG, "null state vector"); return compute(g, OP_FUNCTION, nullptr, F, U, nullptr, 0, 0); }
extern "C" int IGXComputeJacobian(IGX g, IGXVec U, IGXMat J) { if (!U) return fail(IGX_ERR_ARG_WRONG, "null state vector"); return compute(g, OP_JACOBIAN, J, nullptr, U, nullptr, 0, 0); }
extern "C" int IGXComputeIFunction(IGX g, double a, IGXVec V, double t, IGXVec U, IGXVec F) { if (!U || !V) return fail(IGX_ERR_ARG_WRONG, "null state vector"); return compute(g, OP_IFUNCTION, nullptr, F, U, V, a, t); }
extern "C" int IGXComputeIJacobian(IGX g, double a, IGXVec V, double t, IGXVec U, IGXMat J) { if (!U || !V) return fail(IGX_ERR_ARG_WRONG, "null state vector"); return compute(g, OP_IJACOBIAN, J, nullptr, U, V, a, t); }
// The matrix-free drivers: passes of vec_sumfact (vec_sumfact.hpp) over the elements in the mode's instantiation of the operator igx_op
// (IGX_OP_MATRIX / _JACOBIAN / _IJACOBIAN), or a refusal with IGX_ERR_SUP: there is no other kernel.  The nres result
// columns R are zeroed and assembled like vectors; on several ranks X, U and V hold their ghosts and one IGXReduceGhostRows(iga, NULL, R[j])
// per column completes the ghost rows.  ACTION: nx = nres = 1, one pass.  ACTION_BATCH: Y_j = A X_j for nx = nres columns,
// IGX_ACTION_MAXCOLS of them per pass (what does not depend on the direction is done once per element and chunk), so
// last_launches = colours x ceil(nx / IGX_ACTION_MAXCOLS); a run-time struct (IGX_FORM_SOURCE) has no batched instantiation yet: its columns
// go through the single-column kernel one by one (colours x nx launches), and the kernel name says so.  The diagonals: nx = 0.
// The entries below and the solve loops check their own arguments; what they share is here, once.
static int compute_matfree(IGX g, VsMode mode, int igx_op, IGXVec U, IGXVec V, int nx, IGXVec *X, int nres, IGXVec *R, double shift, double t) {
  const VsTraits tr = vs_traits(mode);
  const Space &s = g->s;
  if ((U && U->iga != g) || (V && V->iga != g)) return fail(IGX_ERR_ARG_WRONG, "state vector created by another IGX");
  for (int j = 0; j < nres; ++j) if ((U && U == R[j]) || (V && V == R[j])) return fail(IGX_ERR_ARG_WRONG, tr.block ? "a block column must not be a state vector" : "the result must not be a state vector");
  if (tr.batch) {      // (the block calls' pinned order, include/petiga_amd.h: the form and the space ahead of the first HIP call)
    if (s.form == IGX_FORM_NONE) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetForm...() first");
    if (const MfRefusal r = matfree_refusal(s, g->kernel_choice, mode, nullptr, MfCaller::FORM)) return fail(r.code, r.msg);
  }
  if (int rc = ensure_device(g)) return rc;
  if (s.form == IGX_FORM_NONE) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetForm...() first");
  OutDev out; memset(&out, 0, sizeof(out));
  out.op = matfree_op(mode, igx_op); out.shift = shift; out.t = t; out.errflag = g->errflag.as<int>(); out.bid = -1;
  if (tr.block) for (int j = 0; j < nres; ++j) out.bcol[j] = R[j]->a.as<double>();
  if (!tr.batch) { out.vec = R[0]->a.as<double>(); out.X = nx ? X[0]->a.as<double>() : nullptr; }
  out.U = U ? U->a.as<double>() : nullptr; out.V = V ? V->a.as<double>() : nullptr;
  if (g->timing) HIPCK(hipEventRecord(g->ev[0], g->stream));
  for (int j = 0; j < nres; ++j) HIPCK(hipMemsetAsync(R[j]->a.p, 0, R[j]->a.bytes, g->stream));
  if (g->timing) HIPCK(hipEventRecord(g->ev[1], g->stream));
  const SpaceDev S = make_spacedev(g);
  g->dom = DomInfo(); g->slab_valid = 0;
  g->zero_matrix = nullptr; g->slab_done = nullptr; g->face_done = nullptr;
  const bool rtc = s.form == IGX_FORM_SOURCE;
  int launches = 0;
  for (int j0 = 0; j0 < (tr.batch ? nx : 1); j0 += rtc ? 1 : IGX_ACTION_MAXCOLS) {      // (one pass unless ACTION_BATCH: a chunk of columns, a struct's next column)
    ActionCols cols; memset(&cols, 0, sizeof(cols));
    if (tr.batch && rtc) { out.X = X[j0]->a.as<double>(); out.vec = R[j0]->a.as<double>(); }
    else if (tr.batch) {
      cols.nc = std::min(nx - j0, (int)IGX_ACTION_MAXCOLS);
      for (int c = 0; c < cols.nc; ++c) { cols.X[c] = X[j0 + c]->a.as<double>(); cols.Y[c] = R[j0 + c]->a.as<double>(); }
    }
    if (int rc = rtc ? launch_generic_rtc(g, S, out, mode) : matfree_by_dim(g, S, out, mode, tr.batch ? &cols : nullptr)) return rc;
    launches += g->last_launches;
  }
  g->last_launches = launches;
  if (tr.batch && rtc) {
    const size_t at = g->last_kernel.find("matrix action:");
    if (at != std::string::npos) g->last_kernel.replace(at, 14, "matrix action on a block, column by column:");
  }
  if (g->timing) { HIPCK(hipEventRecord(g->ev[2], g->stream)); HIPCK(hipEventRecord(g->ev[3], g->stream)); }
  return 0;
}
// Matrix-free actions: Y = A X with A the matrix IGXComputeSystem (IGXComputeMatrix's K with the fix-up of IGAElementFixSystem) / Jacobian /
// IJacobian would assemble on this rank, IGAElementFixJacobian included (a fixed column takes nothing, a fixed row receives X_row once per
// local element that holds the node).  No matrix is formed.
static int action_args(IGX g, IGXVec X, IGXVec Y) {
  NEEDIGA(g);
  if (!X || !Y) return fail(IGX_ERR_ARG_WRONG, "null direction or result vector");
  if (X == Y) return fail(IGX_ERR_ARG_WRONG, "the direction and the result must be different vectors");
  if (X->iga != g || Y->iga != g) return fail(IGX_ERR_ARG_WRONG, "vector created by another IGX");
  return 0;
}
extern "C" int IGXComputeMatrixAction(IGX g, IGXVec X, IGXVec Y) { if (int rc = action_args(g, X, Y)) return rc; return compute_matfree(g, VsMode::ACTION, IGX_OP_MATRIX, nullptr, nullptr, 1, &X, 1, &Y, 0, 0); }
extern "C" int IGXComputeJacobianAction(IGX g, IGXVec U, IGXVec X, IGXVec Y) { if (!U) return fail(IGX_ERR_ARG_WRONG, "null state vector"); if (int rc = action_args(g, X, Y)) return rc; return compute_matfree(g, VsMode::ACTION, IGX_OP_JACOBIAN, U, nullptr, 1, &X, 1, &Y, 0, 0); }
extern "C" int IGXComputeIJacobianAction(IGX g, double a, IGXVec V, double t, IGXVec U, IGXVec X, IGXVec Y) { if (!U || !V) return fail(IGX_ERR_ARG_WRONG, "null state vector"); if (int rc = action_args(g, X, Y)) return rc; return compute_matfree(g, VsMode::ACTION, IGX_OP_IJACOBIAN, U, V, 1, &X, 1, &Y, a, t); }

// The actions on a block of vectors (compute_matfree, ACTION_BATCH).  Refusals: the single action's, under the block call's name.
constexpr int ACTION_BLOCK_MAX = 48;      // columns of a block call at the most (= BV_MAX: the block-vector limit, block_vec.hpp)
// the pinned order of the block calls' refusals (include/petiga_amd.h), all ahead of the first HIP call
static int action_block_args(IGX g, bool needU, IGXVec U, bool needV, IGXVec V, int nx, IGXVec *X, IGXVec *Y) {
  NEEDIGA(g);
  if (!X || !Y) return fail(IGX_ERR_ARG_WRONG, "null array of directions or results");
  if ((needU && !U) || (needV && !V)) return fail(IGX_ERR_ARG_WRONG, "null state vector");
  if (nx < 1 || nx > ACTION_BLOCK_MAX) return fail(IGX_ERR_ARG_OUTOFRANGE, "the matrix action on a block takes 1 to " + std::to_string(ACTION_BLOCK_MAX) + " columns, got " + std::to_string(nx));
  for (int j = 0; j < nx; ++j) {
    if (!X[j] || !Y[j]) return fail(IGX_ERR_ARG_WRONG, "null direction or result vector in the block");
    if (X[j]->iga != g || Y[j]->iga != g) return fail(IGX_ERR_ARG_WRONG, "vector created by another IGX");
  }
  if ((U && U->iga != g) || (V && V->iga != g)) return fail(IGX_ERR_ARG_WRONG, "state vector created by another IGX");
  for (int j = 0; j < nx; ++j) {
    for (int k = 0; k < j; ++k) if (Y[k] == Y[j]) return fail(IGX_ERR_ARG_WRONG, "the same vector given for two results of the block");
    for (int i = 0; i < nx; ++i) if (X[i] == Y[j]) return fail(IGX_ERR_ARG_WRONG, "a direction and a result of the block must be different vectors");
    if ((U && U == Y[j]) || (V && V == Y[j])) return fail(IGX_ERR_ARG_WRONG, "a result must not be a state vector");
  }
  return 0;
}
extern "C" int IGXComputeMatrixActionBlock(IGX g, int nx, IGXVec *X, IGXVec *Y) { if (int rc = action_block_args(g, false, nullptr, false, nullptr, nx, X, Y)) return rc; return compute_matfree(g, VsMode::ACTION_BATCH, IGX_OP_MATRIX, nullptr, nullptr, nx, X, nx, Y, 0, 0); }
extern "C" int IGXComputeJacobianActionBlock(IGX g, IGXVec U, int nx, IGXVec *X, IGXVec *Y) { if (int rc = action_block_args(g, true, U, false, nullptr, nx, X, Y)) return rc; return compute_matfree(g, VsMode::ACTION_BATCH, IGX_OP_JACOBIAN, U, nullptr, nx, X, nx, Y, 0, 0); }
extern "C" int IGXComputeIJacobianActionBlock(IGX g, double a, IGXVec V, double t, IGXVec U, int nx, IGXVec *X, IGXVec *Y) { if (int rc = action_block_args(g, true, U, true, V, nx, X, Y)) return rc; return compute_matfree(g, VsMode::ACTION_BATCH, IGX_OP_IJACOBIAN, U, V, nx, X, nx, Y, a, t); }
extern "C" int IGXSetBatchedActions(IGX g, int flag) { NEEDIGA(g); g->batched_actions = flag ? 1 : 0; return 0; }

// Matrix-free diagonals: D = diag A of the matrix the matching action applies (IGAElementFixJacobian included: a fixed dof holds the
// number of local elements at its node): what a Jacobi or Chebyshev preconditioner of the shell matrix needs.
static int diagonal_args(IGX g, IGXVec D) {
  NEEDIGA(g);
  if (!D) return fail(IGX_ERR_ARG_WRONG, "null result vector");
  if (D->iga != g) return fail(IGX_ERR_ARG_WRONG, "vector created by another IGX");
  return 0;
}
extern "C" int IGXComputeMatrixDiagonal(IGX g, IGXVec D) { if (int rc = diagonal_args(g, D)) return rc; return compute_matfree(g, VsMode::DIAGONAL, IGX_OP_MATRIX, nullptr, nullptr, 0, nullptr, 1, &D, 0, 0); }
extern "C" int IGXComputeJacobianDiagonal(IGX g, IGXVec U, IGXVec D) { if (!U) return fail(IGX_ERR_ARG_WRONG, "null state vector"); if (int rc = diagonal_args(g, D)) return rc; return compute_matfree(g, VsMode::DIAGONAL, IGX_OP_JACOBIAN, U, nullptr, 0, nullptr, 1, &D, 0, 0); }
extern "C" int IGXComputeIJacobianDiagonal(IGX g, double a, IGXVec V, double t, IGXVec U, IGXVec D) { if (!U || !V) return fail(IGX_ERR_ARG_WRONG, "null state vector"); if (int rc = diagonal_args(g, D)) return rc; return compute_matfree(g, VsMode::DIAGONAL, IGX_OP_IJACOBIAN, U, V, 0, nullptr, 1, &D, a, t); }

// Matrix-free point-block diagonals: the dof x dof blocks A_(a,i),(a,j) of every node a of the same operator (what PCPBJACOBI /
// MatInvertBlockDiagonal ask of a shell matrix), in dof ordinary vectors, one per block column: B[j][node * dof + i] = A_(node,i),(node,j).
static int check_block_columns(IGX g, int nb, IGXVec *B) {
  if (nb != g->s.dof) return fail(IGX_ERR_ARG_WRONG, "the block diagonal has dof columns: nb must equal dof");
  if (nb < 1 || nb > MAXBC) return fail(IGX_ERR_ARG_WRONG, "the block diagonal needs dof <= 8");
  if (!B) return fail(IGX_ERR_ARG_WRONG, "null array of block columns");
  for (int j = 0; j < nb; ++j) {
    if (!B[j]) return fail(IGX_ERR_ARG_WRONG, "null block column");
    if (B[j]->iga != g) return fail(IGX_ERR_ARG_WRONG, "block column created by another IGX");
    for (int k = 0; k < j; ++k) if (B[k] == B[j]) return fail(IGX_ERR_ARG_WRONG, "the same vector given for two block columns");
  }
  return 0;
}
extern "C" int IGXComputeMatrixBlockDiagonal(IGX g, int nb, IGXVec *B) { NEEDIGA(g); if (int rc = check_block_columns(g, nb, B)) return rc; return compute_matfree(g, VsMode::BLOCK_DIAGONAL, IGX_OP_MATRIX, nullptr, nullptr, 0, nullptr, nb, B, 0, 0); }
extern "C" int IGXComputeJacobianBlockDiagonal(IGX g, IGXVec U, int nb, IGXVec *B) { if (!U) return fail(IGX_ERR_ARG_WRONG, "null state vector"); NEEDIGA(g); if (int rc = check_block_columns(g, nb, B)) return rc; return compute_matfree(g, VsMode::BLOCK_DIAGONAL, IGX_OP_JACOBIAN, U, nullptr, 0, nullptr, nb, B, 0, 0); }
extern "C" int IGXComputeIJacobianBlockDiagonal(IGX g, double a, IGXVec V, double t, IGXVec U, int nb, IGXVec *B) { if (!U || !V) return fail(IGX_ERR_ARG_WRONG, "null state vector"); NEEDIGA(g); if (int rc = check_block_columns(g, nb, B)) return rc; return compute_matfree(g, VsMode::BLOCK_DIAGONAL, IGX_OP_IJACOBIAN, U, V, 0, nullptr, nb, B, a, t); }

// The blocks as a preconditioner (block_diag.hpp): B <- B^-1 block by block in place (every local row; on several ranks after the
// reduction and a refresh of each column), and Y_node = B_node X_node.  nsingular: the number of blocks with a zero or non-finite pivot,
// which become zero blocks; reading it synchronises the stream, NULL skips both.
static int block_diagonal_run(IGX g, int nb, IGXVec *B, IGXVec X, IGXVec Y, int64_t *nsingular, bool invert) {
  NEEDIGA(g);
  if (int rc = check_block_columns(g, nb, B)) return rc;
  if (!invert) {
    if (!X || !Y) return fail(IGX_ERR_ARG_WRONG, "null vector");
    if (X->iga != g || Y->iga != g) return fail(IGX_ERR_ARG_WRONG, "vector created by another IGX");
    if (X == Y) return fail(IGX_ERR_ARG_WRONG, "X and Y must differ");
    for (int j = 0; j < nb; ++j) if (X == B[j] || Y == B[j]) return fail(IGX_ERR_ARG_WRONG, "X and Y must not be block columns");
  }
  if (int rc = ensure_device(g)) return rc;
  BlockCols cols; memset(&cols, 0, sizeof(cols));
  for (int j = 0; j < nb; ++j) cols.col[j] = B[j]->a.as<double>();
  unsigned long long *cnt = nullptr;
  if (invert && nsingular) {
    if (!g->nsingular.p && g->nsingular.alloc(sizeof(unsigned long long))) return fail(IGX_ERR_MEM, "device allocation failed");
    cnt = g->nsingular.as<unsigned long long>();
    HIPCK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), g->stream));
  }
  if (g->timing) { HIPCK(hipEventRecord(g->ev[0], g->stream)); HIPCK(hipEventRecord(g->ev[1], g->stream)); }
  g->slab_valid = 0;
  block_diag_launch(nb, invert, cols, invert ? nullptr : X->a.as<double>(), invert ? nullptr : Y->a.as<double>(), (long long)g->nbrows, cnt, g->stream);
  if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "block diagonal kernel launch failed");
  if (g->timing) { HIPCK(hipEventRecord(g->ev[2], g->stream)); HIPCK(hipEventRecord(g->ev[3], g->stream)); }
  g->last_launches = 1;
  g->last_kernel = invert ? "block_diag_invert(Gauss-Jordan with partial pivoting, one thread per node)" : "block_diag_apply(one thread per node)";
  if (cnt) {
    unsigned long long h = 0;
    HIPCK(hipMemcpyAsync(&h, cnt, sizeof(h), hipMemcpyDeviceToHost, g->stream));
    HIPCK(hipStreamSynchronize(g->stream));
    *nsingular = (int64_t)h;
  }
  return 0;
}
extern "C" int IGXBlockDiagonalInvert(IGX g, int nb, IGXVec *B, int64_t *nsingular) { return block_diagonal_run(g, nb, B, nullptr, nullptr, nsingular, true); }
extern "C" int IGXBlockDiagonalApply(IGX g, int nb, IGXVec *B, IGXVec X, IGXVec Y) { return block_diagonal_run(g, nb, B, X, Y, nullptr, false); }

// Fast diagonalisation (Sangalli & Tani 2016): Z = P R with P the exact inverse of alpha M + sum_d beta_d K_d on the parametric tensor-product
// space, field by field over each field's free dofs, and R / count in the fixed rows.  IGXFastDiagSetUp is host work (host.cpp: the 1-D
// matrices from the space's tables and their generalised eigenpairs); IGXFastDiagApply uploads the tables at its first call and runs six
// contractions of fast_diag.hpp over two work vectors: axes 0, 1, 2 forward (the last one scales by the reciprocal denominators), then 2, 1, 0
// backward (the last one writes the fixed rows).
static const char *fast_diag_refusal(IGX g) {
  const Space &s = g->s;
  if (s.dim != 3) return "fast diagonalisation needs dim = 3 (three 1-D eigen-systems and six contractions)";
  for (int d = 0; d < 3; ++d) if (s.proc_sizes[d] != 1) return "fast diagonalisation needs one rank on every axis: its transforms are global along an axis";
  if (g->fixtable.p) return "fast diagonalisation does not cover a fix table (IGXSetFixTable): its fixed dofs are not a union of faces";
  if (s.dof > MAXBC) return "fast diagonalisation needs dof <= 8";
  return nullptr;
}
extern "C" int IGXFastDiagSetUp(IGX g, double alpha, const double beta[3], int *nzeroed) {
  NEEDIGA(g);
  if (!g->s.setup) return fail(IGX_ERR_ORDER, "Must call IGXSetUp() before IGXFastDiagSetUp()");
  if (const char *why = fast_diag_refusal(g)) return fail(IGX_ERR_SUP, why);
  if (!beta) return fail(IGX_ERR_ARG_WRONG, "null beta");
  if (!(alpha >= 0) || !(beta[0] >= 0) || !(beta[1] >= 0) || !(beta[2] >= 0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "fast diagonalisation needs alpha >= 0 and beta >= 0");
  if (alpha == 0 && beta[0] == 0 && beta[1] == 0 && beta[2] == 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "fast diagonalisation needs alpha or some beta positive");
  std::shared_ptr<FastDiagState> st(new FastDiagState());
  std::string e;
  if (int rc = fast_diag_setup(g->s, alpha, beta, st->h, e)) return fail(rc, e);
  g->fd = st;
  if (nzeroed) *nzeroed = st->h.nzeroed;
  return 0;
}
extern "C" int IGXFastDiagGetAxis(IGX g, int axis, int field, int *first, int *m, double lambda[], double U[]) {
  AXISCK(g, axis);
  if (!g->fd) return fail(IGX_ERR_ORDER, "Must call IGXFastDiagSetUp() first");
  if (field < 0 || field >= g->fd->h.dof) return fail(IGX_ERR_ARG_OUTOFRANGE, "Expecting 0<=field<dof");
  const FastDiagEig &E = g->fd->h.eig[axis][g->fd->h.combo(axis, field)];
  if (first) *first = E.first; if (m) *m = E.m;
  if (lambda) std::copy(E.lambda.begin(), E.lambda.end(), lambda);
  if (U) std::copy(E.U.begin(), E.U.end(), U);
  return 0;
}
static int fast_diag_upload(IGX g) {
  FastDiagState &st = *g->fd; const FastDiag &h = st.h;
  for (int d = 0; d < 3; ++d) {
    const int n = h.n[d];
    for (int c = 0; c < 4; ++c) {
      const FastDiagEig &E = h.eig[d][c];
      if (!E.used) continue;
      std::vector<double> tf((size_t)n * n, 0.0), tb((size_t)n * n, 0.0), sv(n, 0.0);
      for (int i = 0; i < E.m; ++i) for (int k = 0; k < E.m; ++k) {      // node first + i, mode k
        const double u = E.U[(size_t)i + (size_t)E.m * k];
        tf[(size_t)(E.first + i) * n + k] = u; tb[(size_t)k * n + E.first + i] = u;
      }
      for (int k = 0; k < E.m; ++k) sv[k] = E.s[k];
      if (st.tf[d][c].upload(tf) || st.tb[d][c].upload(tb) || st.s[d][c].upload(sv)) return fail(IGX_ERR_MEM, "device allocation of the fast-diagonalisation tables failed");
    }
    if (st.count[d].upload(h.count[d])) return fail(IGX_ERR_MEM, "device allocation of the fast-diagonalisation tables failed");
  }
  const size_t bytes = (size_t)g->nbrows * g->s.dof * sizeof(double);
  for (int k = 0; k < 2; ++k) if (st.work[k].alloc(bytes)) return fail(IGX_ERR_MEM, "device allocation of the fast-diagonalisation work vectors failed");
  st.on_device = true;
  return 0;
}
extern "C" int IGXFastDiagApply(IGX g, IGXVec R, IGXVec Z) {
  NEEDIGA(g);
  if (!g->fd) return fail(IGX_ERR_ORDER, "Must call IGXFastDiagSetUp() before IGXFastDiagApply()");
  if (const char *why = fast_diag_refusal(g)) return fail(IGX_ERR_SUP, why);
  FastDiagState &st = *g->fd; const FastDiag &h = st.h;
  {
    bool now[3][2][MAXFD];
    fast_diag_fixed_faces(g->s, now);
    if (memcmp(now, h.fixed, sizeof(now)) != 0) return fail(IGX_ERR_ARG_WRONGSTATE, "the set of Dirichlet faces changed since IGXFastDiagSetUp(): call IGXFastDiagSetUp() again");
  }
  if (!R || !Z) return fail(IGX_ERR_ARG_WRONG, "null vector");
  if (R->iga != g || Z->iga != g) return fail(IGX_ERR_ARG_WRONG, "vector created by another IGX");
  if (int rc = ensure_device(g)) return rc;
  const long long n0 = h.n[0], n1 = h.n[1], n2 = h.n[2], dof = h.dof;
  if (R->n != n0 * n1 * n2 * dof || Z->n != R->n || g->nbrows != n0 * n1 * n2) return fail(IGX_ERR_ARG_WRONG, "vector of another size than the space's");
  if (!st.on_device) if (int rc = fast_diag_upload(g)) return rc;
  bool uniform = true;      // every field has the tables of field 0: the fields are columns like any others
  for (int d = 0; d < 3; ++d) for (int f = 1; f < dof; ++f) if (h.combo(d, f) != h.combo(d, 0)) uniform = false;
  FdArgs a; memset(&a, 0, sizeof(a));
  a.dof = (int)dof; a.nsel = uniform ? 1 : (int)dof;
  a.n0 = (int)n0; a.n1 = (int)n1; a.n2 = (int)n2; a.alpha = h.alpha; a.thresh = h.thresh; a.R = R->a.as<double>();
  for (int d = 0; d < 3; ++d) {
    a.count[d] = st.count[d].as<double>();
    for (int f = 0; f < dof; ++f) { a.s[d][f] = st.s[d][h.combo(d, f)].as<double>(); a.lo[d][f] = h.fixed[d][0][f]; a.hi[d][f] = h.fixed[d][1][f]; }
  }
  const long long inner[3] = {dof, n0 * dof, n0 * n1 * dof}, outer[3] = {n1 * n2, n2, 1};
  double *w0 = st.work[0].as<double>(), *w1 = st.work[1].as<double>();
  struct Step { int axis; bool back; int mode; const double *in; double *out; };
  const Step steps[6] = {{0, false, FD_PLAIN, R->a.as<double>(), w0}, {1, false, FD_PLAIN, w0, w1}, {2, false, FD_SCALE, w1, w0},
                         {2, true, FD_PLAIN, w0, w1}, {1, true, FD_PLAIN, w1, w0}, {0, true, FD_FINAL, w0, Z->a.as<double>()}};
  if (g->timing) { HIPCK(hipEventRecord(g->ev[0], g->stream)); HIPCK(hipEventRecord(g->ev[1], g->stream)); }
  g->slab_valid = 0;
  for (const Step &sp : steps) {
    const int d = sp.axis;
    a.in = sp.in; a.out = sp.out; a.mode = sp.mode; a.n = h.n[d]; a.inner = inner[d]; a.outer = outer[d];
    for (int f = 0; f < dof; ++f) a.T[f] = (sp.back ? st.tb : st.tf)[d][h.combo(d, f)].as<double>();
    if (fast_diag_launch(a, g->stream)) return fail(IGX_ERR_SUP, "fast diagonalisation: the vector is too large for one launch grid");
    if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "fast diagonalisation kernel launch failed");
  }
  if (g->timing) { HIPCK(hipEventRecord(g->ev[2], g->stream)); HIPCK(hipEventRecord(g->ev[3], g->stream)); }
  g->last_launches = 6;
  char name[160];
  snprintf(name, sizeof(name), "fast_diag(mfma_f64_16x16x4, 6 contractions, row tiles %d/%d/%d, %s)", fd_row_tiles(h.n[0]), fd_row_tiles(h.n[1]), fd_row_tiles(h.n[2]),
           uniform ? "fields share their tables" : "tables per field");
  g->last_kernel = name;
  return 0;
}

// One pass for the pair a Newton step asks for at the same state (SNESComputeFunction + SNESComputeJacobian; src/petigats.c:23-159,
// src/petigasnes.c:23-139): the results are those of the two drivers, in one walk where a fused kernel exists, else in two calls.
extern "C" int IGXComputeIFunctionIJacobian(IGX g, double a, IGXVec V, double t, IGXVec U, IGXVec F, IGXMat J) {
  if (!U || !V) return fail(IGX_ERR_ARG_WRONG, "null state vector");
  bool done = false;
  if (int rc = compute(g, OP_IJACOBIAN, J, F, U, V, a, t, &done)) return rc;
  if (done) return 0;
  if (int rc = compute(g, OP_IFUNCTION, nullptr, F, U, V, a, t)) return rc;
  const std::string kf = g->last_kernel;
  if (int rc = compute(g, OP_IJACOBIAN, J, nullptr, U, V, a, t)) return rc;
  g->last_kernel = kf + " | " + g->last_kernel;
  return 0;
}
extern "C" int IGXComputeFunctionJacobian(IGX g, IGXVec U, IGXVec F, IGXMat J) {
  if (!U) return fail(IGX_ERR_ARG_WRONG, "null state vector");
  bool done = false;
  if (int rc = compute(g, OP_JACOBIAN, J, F, U, nullptr, 0, 0, &done)) return rc;
  if (done) return 0;
  if (int rc = compute(g, OP_FUNCTION, nullptr, F, U, nullptr, 0, 0)) return rc;
  const std::string kf = g->last_kernel;
  if (int rc = compute(g, OP_JACOBIAN, J, nullptr, U, nullptr, 0, 0)) return rc;
  g->last_kernel = kf + " | " + g->last_kernel;
  return 0;
}

// ------------------------------------------------------------------ IGAComputeScalar (src/petigacomp.c:35-98)
// What the built-in functionals and a user's (IGXComputeScalarSource, rtc.hpp) share: a row of ns partial sums per element, and one more per
// element of a visited face; launch(Sd, out) fills them with the functional's parameters travelling like a form's; two stages of sums,
// the read-back of S[ns], and the geometry's error flag.
template <class Launch>
static int reduce_scalars(IGX g, int ns, IGXVec U, const double params[], int nparams, Launch &&launch, double S[]) {
  Space &s = g->s;
  int64_t nel = (int64_t)s.elem_width[0] * s.elem_width[1] * s.elem_width[2];
  for (int a = 0; a < s.dim; ++a) for (int sd = 0; sd < 2; ++sd) {   // one more partial row per element of a visited face
    const int eface = sd ? s.elem_sizes[a] - 1 : 0;
    if (s.visit[a][sd] && eface >= s.elem_start[a] && eface < s.elem_start[a] + s.elem_width[a]) nel += (int64_t)s.elem_width[0] * s.elem_width[1] * s.elem_width[2] / s.elem_width[a];
  }
  const int nblk = (int)std::min<int64_t>(1024, (nel + 255) / 256);
  const int64_t chunk = (nel + nblk - 1) / nblk;
  const size_t need = ((size_t)nel + nblk + 1) * ns * sizeof(double);
  if (g->partials.bytes < need) { HIPCK(hipStreamSynchronize(g->stream)); if (g->partials.alloc(need)) return fail(IGX_ERR_MEM, "partial-sum buffer allocation failed"); }
  double *part = g->partials.as<double>(), *stage = part + (size_t)nel * ns, *res = stage + (size_t)nblk * ns;
  HIPCK(hipMemsetAsync(part, 0, (size_t)nel * ns * sizeof(double), g->stream));
  OutDev out; memset(&out, 0, sizeof(out));
  out.op = OP_SCALAR; out.bid = -1; out.errflag = g->errflag.as<int>(); out.vec = part; out.U = U ? U->a.as<double>() : nullptr;
  const SpaceDev Sd = make_spacedev(g);
  const std::vector<double> keep = s.params;
  s.params.assign(params, params + (params ? nparams : 0));
  const int rc = launch(Sd, out);
  s.params = keep;
  if (rc) return rc;
  hipLaunchKernelGGL(k_sum_partials, dim3(nblk), dim3(256), 0, g->stream, part, nel, ns, stage, chunk);
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, g->stream, stage, (int64_t)nblk, ns, res, (int64_t)nblk);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(S, res, ns * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIPCK(hipStreamSynchronize(g->stream));
  int flag = 0; HIPCK(hipMemcpy(&flag, g->errflag.p, sizeof(int), hipMemcpyDeviceToHost));
  if (flag) { HIPCK(hipMemset(g->errflag.p, 0, sizeof(int))); return fail(flag, "Non-positive det(Jacobian) of the geometry mapping"); }
  return 0;
}
extern "C" int IGXComputeScalar(IGX g, IGXVec U, int kind, const double params[], int nparams, int n, double S[]) {
  NEEDIGA(g);
  if (int rc = ensure_device(g)) return rc;
  if (U && U->iga != g) return fail(IGX_ERR_ARG_WRONG, "state vector created by another IGX");
  if (!S || n < 1) return fail(IGX_ERR_ARG_WRONG, "null result array");
  const int ns = (kind == IGX_SCALAR_ERRNORM) ? 4 : (kind == IGX_SCALAR_VOLUME ? 2 : 1);
  if (n != ns) return fail(IGX_ERR_ARG_WRONG, "this functional returns " + std::to_string(ns) + " scalars");
  if (nparams < 0 || nparams > MAXPARAM || (nparams && !params)) return fail(IGX_ERR_ARG_OUTOFRANGE, "bad parameter list");
  const int order = (kind == IGX_SCALAR_ERRNORM && nparams > 0) ? (int)params[0] : 0;
  if (order < 0 || order > 2) return fail(IGX_ERR_ARG_OUTOFRANGE, "derivative order must be in range [0,2]");
  return reduce_scalars(g, ns, U, params, nparams, [&](const SpaceDev &Sd, const OutDev &out) {
    switch (g->s.dim) {
    case 1: return igx_tu_scalar(std::integral_constant<int, 1>(), g, kind, Sd, out, order);
    case 2: return igx_tu_scalar(std::integral_constant<int, 2>(), g, kind, Sd, out, order);
    default: return igx_tu_scalar(std::integral_constant<int, 3>(), g, kind, Sd, out, order);
    }
  }, S);
}

// ------------------------------------------------------------------ checksums over the owned rows
// one workgroup per stride of rows; fixed grid and a fixed in-block tree: bitwise repeatable
__global__ void __launch_bounds__(256) k_checksum(int nown0, int nown1, int nown2, int nrow0, int nrow1, int bs, const int64_t *browptr, const double *val, const double *vec, double *part) {
  __shared__ double red[256];
  const int64_t nown = (int64_t)nown0 * nown1 * nown2;
  double s[4] = {0, 0, 0, 0};
  for (int64_t k = blockIdx.x; k < nown; k += gridDim.x) {
    const int r0 = (int)(k % nown0), r1 = (int)((k / nown0) % nown1), r2 = (int)(k / ((int64_t)nown0 * nown1));
    const int64_t row = (int64_t)r0 + (int64_t)nrow0 * ((int64_t)r1 + (int64_t)nrow1 * r2);
    if (val) {
      const int64_t lo = browptr[row] * bs * bs, hi = browptr[row + 1] * bs * bs;
      for (int64_t i = lo + threadIdx.x; i < hi; i += 256) { const double v = val[i]; s[0] += v; s[1] += fabs(v); }
    }
    if (vec && (int)threadIdx.x < bs) { const double v = vec[row * bs + threadIdx.x]; s[2] += v; s[3] += v * v; }
  }
  for (int c = 0; c < 4; ++c) {
    red[threadIdx.x] = s[c]; __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * 4 + c] = red[0];
    __syncthreads();
  }
}

extern "C" int IGXChecksum(IGX g, IGXMat A, IGXVec b, double S[4]) {
  NEEDIGA(g);
  if (int rc = ensure_device(g)) return rc;
  if (!S) return fail(IGX_ERR_ARG_WRONG, "null result array");
  if ((A && A->iga != g) || (b && b->iga != g)) return fail(IGX_ERR_ARG_WRONG, "matrix / vector created by another IGX");
  const Space &s = g->s;
  int nown[3];
  for (int d = 0; d < 3; ++d) {   // owned rows are a prefix of the row box on every axis (ghosts sit on the high side, src/petiga.c:1172-1208)
    const AxisLayout &L = s.lay[d]; nown[d] = 0;
    for (int r = 0; r < L.nrow; ++r) { if (L.owned[r]) { if (nown[d] != r) return fail(IGX_ERR_PLIB, "owned rows are not a prefix of the row box"); nown[d]++; } }
  }
  const int nblk = 2048;
  const size_t need = ((size_t)nblk + 1) * 4 * sizeof(double);
  if (g->partials.bytes < need) { HIPCK(hipStreamSynchronize(g->stream)); if (g->partials.alloc(need)) return fail(IGX_ERR_MEM, "partial-sum buffer allocation failed"); }
  double *part = g->partials.as<double>(), *res = part + (size_t)nblk * 4;
  hipLaunchKernelGGL(k_checksum, dim3(nblk), dim3(256), 0, g->stream, nown[0], nown[1], nown[2], s.lay[0].nrow, s.lay[1].nrow, s.dof,
                     A ? A->browptr.as<int64_t>() : nullptr, A ? A->val.as<double>() : nullptr, b ? b->a.as<double>() : nullptr, part);
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, g->stream, part, (int64_t)nblk, 4, res, (int64_t)nblk);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(S, res, 4 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIPCK(hipStreamSynchronize(g->stream));
  return 0;
}

extern "C" int IGXGetClockProbe(IGX g, double *shader_mhz, int64_t *elements) {
  NEEDIGA(g);
  if (!shader_mhz) return fail(IGX_ERR_ARG_WRONG, "null result");
  if (!g->s.env.clock_probe || !g->clkbuf.p) return fail(IGX_ERR_ARG_WRONGSTATE, "set IGX_CLOCK_PROBE=1 before IGXCreate and run an assembly on the pencil kernel first");
  long long h[4];
  HIPCK(hipStreamSynchronize(g->stream));
  HIPCK(hipMemcpy(h, g->clkbuf.p, sizeof(h), hipMemcpyDeviceToHost));
  if (h[1] <= 0) return fail(IGX_ERR_ARG_WRONGSTATE, "no pencil-kernel launch since the last call");
  *shader_mhz = 100.0 * (double)h[0] / (double)h[1];
  if (elements) *elements = h[2];
  HIPCK(hipMemsetAsync(g->clkbuf.p, 0, 4 * sizeof(long long), g->stream));   // the sums start again
  return 0;
}

// the host side of patch3_ticket_item (gram_patch3.hpp), on the colour's arguments as patch_colour_args fills them
extern "C" int IGXPatch3TicketOrder(int n1, int n2, int nseg, int cx, int cy, int order, int cap, int *nitems, int *items, int *faces) {
  using G = Patch3<PATCH3_MX, PATCH3_MY>;
  if (!nitems || n1 < 1 || n2 < 1 || nseg < 1 || cx < 0 || cx >= G::SX || cy < 0 || cy >= G::SY || (cap > 0 && (!items || !faces))) return fail(IGX_ERR_ARG_WRONG, "IGXPatch3TicketOrder: sizes, colour or result arrays");
  const int npx = (n1 + G::MX - 1) / G::MX, npy = (n2 + G::MY - 1) / G::MY;
  PatchArgs A; memset(&A, 0, sizeof(A));
  A.px_start = cx; A.px_step = G::SX; A.px_count = (npx - cx + G::SX - 1) / G::SX;
  A.py_start = cy; A.py_step = G::SY; A.py_count = (npy - cy + G::SY - 1) / G::SY;
  A.pa.nelx = n1; A.pa.nely = n2; A.pa.nseg = nseg;
  *nitems = (A.px_count <= 0 || A.py_count <= 0) ? 0 : A.px_count * A.py_count * nseg;
  for (int t = 0; t < std::min(*nitems, cap); ++t) { bool f = false; items[t] = patch3_ticket_item<G>(A, order, t, &f); faces[t] = f ? 1 : 0; }
  return 0;
}

// the rows walk's staged tile-layer (gram_rows3.hpp): where the entry (node column col of the tile, dy, dx, d) lies in the buffer --
// rows3_stage_offset, the function the kernel calls -- and the buffer's doubles
extern "C" int IGXRows3StageOffset(int col, int dy, int dx, int d, int *offset, int *doubles) {
  using R = Rows3;
  if (!offset || col < 0 || col >= R::COLS || std::abs(dy) > R::P || std::abs(dx) > R::P || std::abs(d) > R::P) return fail(IGX_ERR_ARG_WRONG, "IGXRows3StageOffset: column, offsets or result");
  *offset = rows3_stage_offset(col, dy, dx, d);
  if (doubles) *doubles = R::STG;
  return 0;
}

// ------------------------------------------------------------------ multi-GPU ghost rows (filled in by exchange.hpp)
#include "exchange.hpp"
#include "comm.hpp"
#include "coo.hpp"
#include "fileio.hpp"
#include "rtc.hpp"

// ------------------------------------------------------------------ vector algebra on IGXVec, IGXSolve, IGXSolveNonlinear, IGXTimeStep
// (host code and, through it, krylov.hpp, block_vec.hpp, newton.hpp, timestep.hpp and multigrid.hpp).  From here on every subsystem is a host
// header that includes its kernels; each came last when it was added, so every kernel above it is compiled as it was before it existed.
// Keep the order (scripts/kernel_digest.py shows what a change of it does).
#include "solve_loops.hpp"
#include "probe_host.hpp"        // point evaluation of a discrete field (probe.hpp)
#include "transfer_host.hpp"     // transfer between nested spline spaces (transfer.hpp)
#include "multigrid_host.hpp"    // the multigrid cycle (its sweeps: multigrid.hpp, above)
#include "mat_ops_host.hpp"      // the stored matrix as an operator (mat_ops.hpp)
