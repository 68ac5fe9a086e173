// multigrid_host.hpp -- the host side of IGXMultigrid (sweeps: multigrid.hpp, which solve_loops.hpp includes ahead of IGXEigenSolve).  Host
// code only.  Included by the main unit (engine.hip) behind transfer_host.hpp, whose transfers it calls.
#pragma once
// IGXMultigrid: one V-cycle over a hierarchy of set-up IGX as a preconditioner application, and IGXSolve's loop preconditioned by it.  The
// cycle is the one the header states line by line; between two operator calls a Chebyshev step is one sweep of multigrid.hpp, everything
// else is the drivers above: compute_matfree, block_diagonal_run, IGXFastDiagApply, the transfer and IGXSolve.  IGXMultigridCreate touches
// no device; IGXMultigridSetUp allocates the work vectors of every level, forms the diagonals and estimates lambda.  The clock is the
// loops': the figures of a call are stored on the FINEST IGX.
enum { MG_X = 0, MG_B, MG_R, MG_D, MG_W, MG_Z, MG_NWORK };
struct MgLevel {
  IGX g = nullptr; unsigned long long gen = 0;
  IGXVec U = nullptr, V = nullptr;                       // the state of the level's operator (IGXMultigridSetState)
  int64_t n = 0; int kind = IGX_PC_JACOBI;               // kind: what D is, the diagonal or the inverted point blocks
  double lambda = 0, theta = 0, delta = 0;
  std::vector<double> c1, c2;                            // the constants of Chebyshev step j: rho_j rho_{j-1} and 2 rho_j / delta
  std::vector<std::unique_ptr<_p_IGXVec>> work, dv;      // x b r d w z; the diagonal or the dof block columns
  std::vector<IGXVec> cols;
  MgFaces faces; int face_nodes = 0;
  int launches = 0;                                      // of the last cycle, on this level
};
struct _p_IGXMultigrid : LoopState {
  IGXMultigridSpec spec; int L = 0;
  std::vector<MgLevel> lv; std::vector<IGXTransfer> tr;
  bool ready = false;
  std::shared_ptr<KrylovState> krylov;                   // IGXMultigridSolve's work vectors, on the finest IGX
  std::string action;                                    // the finest action's kernel name
  ~_p_IGXMultigrid() { for (auto &t : tr) IGXTransferDestroy(&t); }
};
static const SolverWords kMultigridWords = {"IGXMultigridSetUp", "the multigrid needs one rank on every axis of every level",
                                            "the multigrid runs where its actions, its diagonals and its coarse solve run, and ", nullptr};
static const char *const kMgPcNames[4] = {"none", "jacobi", "pbjacobi", "fastdiag"};
static int mg_stale(_p_IGXMultigrid *q, const char *fn) {
  if (!q) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": null multigrid");
  for (const MgLevel &l : q->lv) if (!l.g->current(l.gen))
    return fail(IGX_ERR_ORDER, std::string(fn) + ": the multigrid is stale: IGXSetUp() ran on one of its levels after IGXMultigridCreate(); make a new multigrid");
  return 0;
}
static std::string mg_name(const _p_IGXMultigrid *q) {
  const IGXMultigridSpec &sp = q->spec;
  std::string coarse = sp.coarse_maxit == 0 ? std::string(kMgPcNames[sp.coarse_pc]) + " x1" : std::string(sp.coarse_method == IGX_SOLVE_CG ? "cg" : "bicgstab") + "+" + kMgPcNames[sp.coarse_pc];
  return "multigrid(" + std::to_string(q->L) + " levels, chebyshev-" + kMgPcNames[sp.smoother_pc] + " " + std::to_string(sp.degree) + ", coarse " + coarse + ", " + q->action + ")";
}
// the figures of a driver call, and of a call that stored its own (the transfer, IGXSolve), on a level's IGX
static int mg_driver(LoopClock &clk, IGX gl) {
  clk.launches += gl->last_launches;
  if (clk.timing && gl->timing) { float ms = 0; HIPCK(hipEventSynchronize(gl->ev[2])); HIPCK(hipEventElapsedTime(&ms, gl->ev[1], gl->ev[2])); clk.op_ms += ms; }
  return 0;
}
static void mg_stored(LoopClock &clk, IGX gl) { clk.launches += gl->last_launches; if (clk.timing && gl->timing) clk.op_ms += gl->last_kernel_ms; }
static int mg_refused(int rc) { return solver_refused(kMultigridWords, rc); }

extern "C" int IGXMultigridCreate(int nlevels, IGX levels[], const IGXMultigridSpec *sp, IGXMultigrid *mg) {
  if (!levels || !sp || !mg) return fail(IGX_ERR_ARG_WRONG, "IGXMultigridCreate: null pointer: the multigrid takes its levels, a specification and a place for the handle");
  for (int k = 0; k < nlevels; ++k) if (!levels[k]) return fail(IGX_ERR_ARG_WRONG, "IGXMultigridCreate: the multigrid's level " + std::to_string(k) + " is a null IGX");
  if (nlevels < 2) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMultigridCreate: the multigrid needs two levels at the least, got " + std::to_string(nlevels));
  auto range = [](const char *what) { return fail(IGX_ERR_ARG_OUTOFRANGE, std::string("IGXMultigridCreate: the multigrid's specification: ") + what); };
  if (sp->op < IGX_OP_MATRIX || sp->op > IGX_OP_IJACOBIAN) return range("unknown operator");
  if (sp->smoother_pc != IGX_PC_JACOBI && sp->smoother_pc != IGX_PC_PBJACOBI) return range("smoother_pc must be IGX_PC_JACOBI or IGX_PC_PBJACOBI");
  if (sp->degree < 1) return range("degree must be 1 at the least");
  if (!(sp->lo > 0) || !(sp->hi > sp->lo) || !std::isfinite(sp->lo) || !std::isfinite(sp->hi)) return range("lo and hi must be finite with 0 < lo < hi");
  if (sp->power_its < 1) return range("power_its must be 1 at the least");
  if (sp->coarse_method != IGX_SOLVE_CG && sp->coarse_method != IGX_SOLVE_BICGSTAB) return range("unknown coarse method");
  if (sp->coarse_pc < IGX_PC_NONE || sp->coarse_pc > IGX_PC_FASTDIAG) return range("unknown coarse preconditioner");
  if (sp->coarse_maxit < 0) return range("coarse_maxit must not be negative");
  if (!(sp->coarse_rtol >= 0)) return range("coarse_rtol must not be negative");
  if (sp->coarse_maxit == 0 && sp->coarse_pc == IGX_PC_NONE) return range("coarse_maxit == 0 is one application of coarse_pc, which must not be IGX_PC_NONE");
  for (int k = 0; k < nlevels; ++k) if (!levels[k]->s.setup) return fail(IGX_ERR_ORDER, "Must call IGXSetUp() on every level before IGXMultigridCreate(): the multigrid's level " + std::to_string(k) + " is not set up");
  for (int k = 0; k < nlevels; ++k) if (levels[k]->s.form == IGX_FORM_NONE) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetForm...() on every level first: the multigrid's level " + std::to_string(k) + " has no form");
  bool faces0[3][2][MAXFD];
  fast_diag_fixed_faces(levels[0]->s, faces0);
  for (int k = 1; k < nlevels; ++k) {
    const Space &a = levels[0]->s, &b = levels[k]->s;
    if (a.form != b.form || a.params != b.params || levels[0]->rtc_source != levels[k]->rtc_source || levels[0]->rtc_name != levels[k]->rtc_name)
      return fail(IGX_ERR_ARG_WRONG, "IGXMultigridCreate: the multigrid needs the same form with the same parameters on every level, level " + std::to_string(k) + " differs from level 0");
    bool faces[3][2][MAXFD];
    fast_diag_fixed_faces(b, faces);
    if (a.dof != b.dof || memcmp(faces, faces0, sizeof(faces)) != 0)
      return fail(IGX_ERR_ARG_WRONG, "IGXMultigridCreate: the multigrid needs the same Dirichlet faces per field on every level, level " + std::to_string(k) + " differs from level 0");
  }
  for (int k = 0; k < nlevels; ++k) if (levels[k]->fixtable.p) return fail(IGX_ERR_SUP, "IGXMultigridCreate: the multigrid does not cover a fix table (IGXSetFixTable, level " + std::to_string(k) + "): its fixed rows are not a union of faces");
  for (int k = 1; k < nlevels; ++k) if (levels[k]->stream != levels[0]->stream) return fail(IGX_ERR_ARG_WRONG, "IGXMultigridCreate: the multigrid needs the same stream on every level (IGXSetStream), level " + std::to_string(k) + " differs from level 0");
  std::unique_ptr<_p_IGXMultigrid> q(new _p_IGXMultigrid());
  q->spec = *sp; q->L = nlevels; q->lv.resize(nlevels);
  for (int k = 0; k < nlevels; ++k) {
    MgLevel &l = q->lv[k]; IGX g = levels[k]; const Space &s = g->s;
    l.g = g; l.gen = g->setup_gen;
    l.kind = (k == 0 && sp->coarse_maxit == 0 && (sp->coarse_pc == IGX_PC_JACOBI || sp->coarse_pc == IGX_PC_PBJACOBI)) ? sp->coarse_pc : sp->smoother_pc;
    int64_t nodes = 1;
    MgFaces &F = l.faces; memset(&F, 0, sizeof(F));
    F.dof = s.dof;
    for (int d = 0; d < 3; ++d) { F.n[d] = d < s.dim ? s.lay[d].nrow : 1; nodes *= F.n[d]; }
    l.n = nodes * s.dof;
    for (int d = 0; d < s.dim; ++d) for (int sd = 0; sd < 2; ++sd) {
      unsigned mask = 0;
      for (int f = 0; f < s.dof; ++f) if (faces0[d][sd][f]) mask |= 1u << f;
      if (!mask) continue;
      F.axis[F.nface] = d; F.at[F.nface] = sd ? F.n[d] - 1 : 0; F.mask[F.nface] = mask; ++F.nface;
      l.face_nodes = std::max<int64_t>(l.face_nodes, nodes / F.n[d]);
    }
  }
  for (int k = 1; k < nlevels; ++k) {
    IGXTransfer t = nullptr;
    if (int rc = IGXTransferCreate(levels[k - 1], levels[k], &t)) return fail(rc, "IGXMultigridCreate: the multigrid's levels " + std::to_string(k - 1) + " and " + std::to_string(k) + ": " + std::string(g_err));
    q->tr.push_back(t);
  }
  *mg = reinterpret_cast<IGXMultigrid>(q.release());
  return 0;
}
extern "C" int IGXMultigridDestroy(IGXMultigrid *mg) { if (mg && *mg) { delete reinterpret_cast<_p_IGXMultigrid *>(*mg); *mg = nullptr; } return 0; }
extern "C" int IGXMultigridSetState(IGXMultigrid mg, int level, IGXVec V, IGXVec U) {
  _p_IGXMultigrid *q = reinterpret_cast<_p_IGXMultigrid *>(mg);
  if (int rc = mg_stale(q, "IGXMultigridSetState")) return rc;
  if (level < 0 || level >= q->L) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMultigridSetState: the multigrid's level must be in range [0," + std::to_string(q->L - 1) + "]");
  MgLevel &l = q->lv[level];
  if ((U && U->iga != l.g) || (V && V->iga != l.g)) return fail(IGX_ERR_ARG_WRONG, "IGXMultigridSetState: the multigrid's state vector was created by another IGX than level " + std::to_string(level));
  if ((U && U->n != l.n) || (V && V->n != l.n)) return fail(IGX_ERR_ARG_WRONG, "IGXMultigridSetState: the multigrid's state vector is of another size than the level's space");
  l.U = U; l.V = V; q->ready = false;
  return 0;
}
extern "C" int IGXMultigridGetInfo(IGXMultigrid mg, int level, double *lambda, int64_t *n, int *launches_per_cycle) {
  _p_IGXMultigrid *q = reinterpret_cast<_p_IGXMultigrid *>(mg);
  if (int rc = mg_stale(q, "IGXMultigridGetInfo")) return rc;
  if (level < 0 || level >= q->L) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMultigridGetInfo: the multigrid's level must be in range [0," + std::to_string(q->L - 1) + "]");
  if (lambda) *lambda = q->lv[level].lambda;
  if (n) *n = q->lv[level].n;
  if (launches_per_cycle) *launches_per_cycle = q->lv[level].launches;
  return 0;
}
// the level's action at its state, and z = D^-1 in
static int mg_action(_p_IGXMultigrid *q, int k, IGXVec in, IGXVec out, LoopClock *clk) {
  MgLevel &l = q->lv[k]; const IGXMultigridSpec &sp = q->spec;
  const bool ij = sp.op == IGX_OP_IJACOBIAN;
  if (int rc = compute_matfree(l.g, VsMode::ACTION, sp.op, sp.op == IGX_OP_MATRIX ? nullptr : l.U, ij ? l.V : nullptr, 1, &in, 1, &out, ij ? sp.a : 0.0, ij ? sp.t : 0.0)) return mg_refused(rc);
  if (k == q->L - 1) q->action = l.g->last_kernel;
  return clk ? mg_driver(*clk, l.g) : 0;
}
static int mg_blocks(MgLevel &l, IGXVec in, IGXVec out, LoopClock *clk) {
  if (int rc = block_diagonal_run(l.g, (int)l.cols.size(), l.cols.data(), in, out, nullptr, false)) return mg_refused(rc);
  return clk ? mg_driver(*clk, l.g) : 0;
}
extern "C" int IGXMultigridSetUp(IGXMultigrid mg) {
  _p_IGXMultigrid *q = reinterpret_cast<_p_IGXMultigrid *>(mg);
  if (int rc = mg_stale(q, "IGXMultigridSetUp")) return rc;
  const IGXMultigridSpec &sp = q->spec;
  q->ready = false;
  if (sp.coarse_pc == IGX_PC_FASTDIAG && !q->lv[0].g->fd) return fail(IGX_ERR_ORDER, "Must call IGXFastDiagSetUp() on level 0 before IGXMultigridSetUp(): the multigrid's coarse preconditioner is IGX_PC_FASTDIAG");
  for (int k = 0; k < q->L; ++k) {
    const MgLevel &l = q->lv[k];
    if (sp.op != IGX_OP_MATRIX && !l.U) return fail(IGX_ERR_ARG_WRONG, "IGXMultigridSetUp: the multigrid's level " + std::to_string(k) + " has no state vector U (IGXMultigridSetState)");
    if (sp.op == IGX_OP_IJACOBIAN && !l.V) return fail(IGX_ERR_ARG_WRONG, "IGXMultigridSetUp: the multigrid's level " + std::to_string(k) + " has no state vector V (IGXMultigridSetState)");
  }
  for (const MgLevel &l : q->lv) if (int rc = solver_runs_here(l.g, kMultigridWords)) return rc;
  const bool ij = sp.op == IGX_OP_IJACOBIAN;
  for (int k = 0; k < q->L; ++k) {
    MgLevel &l = q->lv[k]; IGX g = l.g;
    if (int rc = ensure_device(g)) return rc;
    if ((int64_t)g->nbrows * g->s.dof != l.n) return fail(IGX_ERR_PLIB, "IGXMultigridSetUp: the multigrid's vectors and the level's row box differ");
    if (int rc = kr_scalars(g)) return rc;
    const bool pb = l.kind == IGX_PC_PBJACOBI;
    if (l.work.empty()) if (int rc = add_vecs(g, l.n, pb ? MG_NWORK : MG_NWORK - 1, l.work, "device allocation of the multigrid's work vectors failed")) return rc;
    if (l.dv.empty()) {
      if (int rc = add_vecs(g, l.n, pb ? g->s.dof : 1, l.dv, "device allocation of the multigrid's diagonals failed")) return rc;
      for (auto &v : l.dv) l.cols.push_back(v.get());
    }
    IGXVec U = sp.op == IGX_OP_MATRIX ? nullptr : l.U, V = ij ? l.V : nullptr;
    if (int rc = compute_matfree(g, pb ? VsMode::BLOCK_DIAGONAL : VsMode::DIAGONAL, sp.op, U, V, 0, nullptr, (int)l.cols.size(), l.cols.data(), ij ? sp.a : 0.0, ij ? sp.t : 0.0)) return mg_refused(rc);
    if (pb) if (int rc = block_diagonal_run(g, g->s.dof, l.cols.data(), nullptr, nullptr, nullptr, true)) return mg_refused(rc);
    // lambda: power_its steps on D^-1 A from v_i = sin(1 + i); after each step lambda = |D^-1 A v| / |v|, and v <- D^-1 A v / |D^-1 A v|
    IGXVec v = l.work[MG_X].get(), w = l.work[MG_W].get(), z = l.work[MG_D].get();
    {
      std::vector<double> h((size_t)l.n);
      for (int64_t i = 0; i < l.n; ++i) h[(size_t)i] = std::sin(1.0 + (double)i);
      HIPCK(hipMemcpy(v->a.p, h.data(), v->a.bytes, hipMemcpyHostToDevice));
    }
    double nv = 0, nz = 0;
    for (int it = 0; it < sp.power_its; ++it) {
      if (int rc = IGXVecNorm2(v, &nv)) return rc;
      if (int rc = mg_action(q, k, v, w, nullptr)) return rc;
      if (pb) { if (int rc = mg_blocks(l, w, z, nullptr)) return rc; }
      else KR_LAUNCH(kr_pdiv, kr_grid(l.n), KR_T, g, z->a.as<double>(), w->a.as<double>(), l.cols[0]->a.as<double>(), (long long)l.n);
      if (int rc = IGXVecNorm2(z, &nz)) return rc;
      l.lambda = nz / nv;
      if (!(l.lambda > 0) || !std::isfinite(l.lambda)) return fail(IGX_ERR_ARG_WRONGSTATE, "IGXMultigridSetUp: the multigrid's estimate of lambda on level " + std::to_string(k) + " is not positive and finite: the operator or its diagonal is singular at this state");
      KR_LAUNCH(kr_axpby, kr_grid(l.n), KR_T, g, v->a.as<double>(), 1.0 / nz, z->a.as<double>(), 0.0, (long long)l.n);
    }
    // theta = (hi + lo) lambda / 2, delta = (hi - lo) lambda / 2, sigma = theta / delta, rho_1 = 1 / sigma, rho_j = 1 / (2 sigma - rho_{j-1})
    l.theta = (sp.hi + sp.lo) * l.lambda / 2; l.delta = (sp.hi - sp.lo) * l.lambda / 2;
    const double sigma = l.theta / l.delta;
    double rho = 1.0 / sigma;
    l.c1.assign(sp.degree + 1, 0.0); l.c2.assign(sp.degree + 1, 0.0);
    for (int j = 2; j <= sp.degree; ++j) { const double rn = 1.0 / (2 * sigma - rho); l.c1[j] = rn * rho; l.c2[j] = 2 * rn / l.delta; rho = rn; }
    l.launches = 0;
  }
  for (IGXTransfer t : q->tr) if (int rc = transfer_upload(reinterpret_cast<_p_IGXTransfer *>(t))) return rc;
  HIPCK(hipStreamSynchronize(q->lv[q->L - 1].g->stream));
  q->ready = true;
  return 0;
}
// Smooth(l, b, x, zero guess): degree Chebyshev steps; on return r holds the residual BEFORE the last step's correction d
static int mg_smooth(_p_IGXMultigrid *q, int k, IGXVec b, IGXVec x, bool zero, LoopClock &clk) {
  MgLevel &l = q->lv[k]; IGX g = l.g; const long long n = (long long)l.n;
  const bool pb = l.kind == IGX_PC_PBJACOBI;
  IGXVec r = l.work[MG_R].get(), d = l.work[MG_D].get(), w = l.work[MG_W].get(), z = pb ? l.work[MG_Z].get() : nullptr;
  double *xd = x->a.as<double>(), *dd = d->a.as<double>(), *rd = r->a.as<double>(), *wd = w->a.as<double>();
  const double *bd = b->a.as<double>(), *Dz = pb ? z->a.as<double>() : l.cols[0]->a.as<double>();
  const double c = 1.0 / l.theta;
  const unsigned grid = kr_grid(n);
  if (!zero) {
    if (int rc = mg_action(q, k, x, w, &clk)) return rc;
    KR_LAUNCH(mg_resid<true>, grid, KR_T, g, rd, bd, wd, n); clk.own(1);
  }
  if (pb) if (int rc = mg_blocks(l, zero ? b : r, z, &clk)) return rc;
  void (*mg_cheb_first_k)(double *, double *, double *, const double *, const double *, double, long long) =
      zero ? (pb ? mg_cheb_first<true, true> : mg_cheb_first<true, false>) : (pb ? mg_cheb_first<false, true> : mg_cheb_first<false, false>);
  KR_LAUNCH(mg_cheb_first_k, grid, KR_T, g, xd, dd, rd, bd, Dz, c, n);
  clk.own(1);
  for (int j = 2; j <= q->spec.degree; ++j) {
    if (int rc = mg_action(q, k, d, w, &clk)) return rc;
    if (pb) {
      KR_LAUNCH(mg_resid<false>, grid, KR_T, g, rd, bd, wd, n); clk.own(1);
      if (int rc = mg_blocks(l, r, z, &clk)) return rc;
      KR_LAUNCH(mg_cheb_step<true>, grid, KR_T, g, xd, dd, rd, wd, Dz, l.c1[j], l.c2[j], n);
    } else KR_LAUNCH(mg_cheb_step<false>, grid, KR_T, g, xd, dd, rd, wd, Dz, l.c1[j], l.c2[j], n);
    clk.own(1);
  }
  return 0;
}
// x = V(k, b) from a zero guess
static int mg_cycle(_p_IGXMultigrid *q, int k, IGXVec b, IGXVec x, LoopClock &clk) {
  MgLevel &l = q->lv[k]; IGX g = l.g; const long long n = (long long)l.n;
  const IGXMultigridSpec &sp = q->spec;
  const int at_entry = clk.launches;
  g->slab_valid = 0;
  if (k == 0) {
    if (sp.coarse_maxit == 0) {
      if (sp.coarse_pc == IGX_PC_JACOBI) { KR_LAUNCH(kr_pdiv, kr_grid(n), KR_T, g, x->a.as<double>(), b->a.as<double>(), l.cols[0]->a.as<double>(), n); clk.own(1); }
      else if (sp.coarse_pc == IGX_PC_PBJACOBI) { if (int rc = mg_blocks(l, b, x, &clk)) return rc; }
      else { if (int rc = IGXFastDiagApply(g, b, x)) return mg_refused(rc); if (int rc = mg_driver(clk, g)) return rc; }
    } else {
      KR_LAUNCH(kr_set, kr_grid(n), KR_T, g, x->a.as<double>(), 0.0, n); clk.own(1);
      IGXSolveSpec cs; memset(&cs, 0, sizeof(cs));
      cs.method = sp.coarse_method; cs.op = sp.op; cs.pc = sp.coarse_pc; cs.a = sp.a; cs.t = sp.t; cs.V = l.V; cs.U = l.U; cs.rtol = sp.coarse_rtol; cs.atol = 0.0; cs.maxit = sp.coarse_maxit;
      IGXSolveInfo ci; memset(&ci, 0, sizeof(ci));
      if (int rc = IGXSolve(g, &cs, b, x, &ci, nullptr)) return mg_refused(rc);
      mg_stored(clk, g);
    }
    l.launches = clk.launches - at_entry;
    return 0;
  }
  MgLevel &c = q->lv[k - 1];
  IGXVec r = l.work[MG_R].get(), d = l.work[MG_D].get(), w = l.work[MG_W].get(), bc = c.work[MG_B].get(), xc = c.work[MG_X].get();
  if (int rc = mg_smooth(q, k, b, x, true, clk)) return rc;
  if (int rc = mg_action(q, k, d, w, &clk)) return rc;
  KR_LAUNCH(mg_resid<false>, kr_grid(n), KR_T, g, r->a.as<double>(), b->a.as<double>(), w->a.as<double>(), n); clk.own(1);
  if (int rc = IGXTransferRestrict(q->tr[k - 1], r, bc)) return rc;
  mg_stored(clk, g);
  if (c.faces.nface) {
    hipLaunchKernelGGL(mg_zero_fixed, dim3((unsigned)std::min(256, (c.face_nodes + MG_FACE_T - 1) / MG_FACE_T), (unsigned)c.faces.nface), dim3(MG_FACE_T), 0, g->stream, bc->a.as<double>(), c.faces);
    if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "mg_zero_fixed: kernel launch failed");
    clk.own(1);
  }
  const int before = clk.launches;
  if (int rc = mg_cycle(q, k - 1, bc, xc, clk)) return rc;
  const int below = clk.launches - before;
  if (int rc = IGXTransferProlong(q->tr[k - 1], xc, x, 1)) return rc;
  mg_stored(clk, g);
  if (int rc = mg_smooth(q, k, b, x, false, clk)) return rc;
  l.launches = clk.launches - at_entry - below;
  return 0;
}
static int mg_vec_args(_p_IGXMultigrid *q, const char *fn, IGXVec a, IGXVec b) {
  const MgLevel &l = q->lv[q->L - 1];
  if (!a || !b) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": null vector: the multigrid takes two vectors of its finest IGX");
  if (a->iga != l.g || b->iga != l.g) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": vector created by another IGX than the multigrid's finest level");
  if (a->n != l.n || b->n != l.n) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": vector of another size than the multigrid's finest space");
  if (a == b) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": the multigrid needs two different vectors, got the same one twice");
  return 0;
}
extern "C" int IGXMultigridApply(IGXMultigrid mg, IGXVec r, IGXVec z) {
  _p_IGXMultigrid *q = reinterpret_cast<_p_IGXMultigrid *>(mg);
  if (int rc = mg_stale(q, "IGXMultigridApply")) return rc;
  if (!q->ready) return fail(IGX_ERR_ORDER, "Must call IGXMultigridSetUp() before IGXMultigridApply(): the multigrid has no diagonals and no lambda yet (or a state changed since)");
  if (int rc = mg_vec_args(q, "IGXMultigridApply", r, z)) return rc;
  IGX g = q->lv[q->L - 1].g;
  LoopClock clk(g, *q);
  if (int rc = clk.begin(g)) return rc;
  if (int rc = mg_cycle(q, q->L - 1, r, z, clk)) return rc;
  return clk.finish(g, mg_name(q));
}
extern "C" int IGXMultigridSolve(IGXMultigrid mg, int method, double rtol, double atol, int maxit, IGXVec b, IGXVec x, IGXSolveInfo *info, double *history) {
  _p_IGXMultigrid *q = reinterpret_cast<_p_IGXMultigrid *>(mg);
  if (int rc = mg_stale(q, "IGXMultigridSolve")) return rc;
  if (method != IGX_SOLVE_CG && method != IGX_SOLVE_BICGSTAB) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMultigridSolve: unknown method");
  if (maxit < 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMultigridSolve: maxit must not be negative");
  if (!(rtol >= 0) || !(atol >= 0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMultigridSolve: the tolerances must not be negative");
  if (!q->ready) return fail(IGX_ERR_ORDER, "Must call IGXMultigridSetUp() before IGXMultigridSolve(): the multigrid has no diagonals and no lambda yet (or a state changed since)");
  if (int rc = mg_vec_args(q, "IGXMultigridSolve", b, x)) return rc;
  const int fine = q->L - 1;
  MgLevel &l = q->lv[fine]; IGX g = l.g;
  if ((l.U && l.U == x) || (l.V && l.V == x)) return fail(IGX_ERR_ARG_WRONG, "IGXMultigridSolve: the solution must not be a state vector of the multigrid");
  const bool cg = method == IGX_SOLVE_CG;
  if (!q->krylov || q->krylov->method != method) {
    q->krylov.reset();
    std::shared_ptr<KrylovState> ks(new KrylovState());
    if (int rc = ks->ensure(g, l.n, cg ? 4 : 8, "device allocation of the multigrid solve's work vectors failed")) return rc;
    ks->method = method; ks->pc = -1; ks->dof = g->s.dof;
    q->krylov = ks;
  }
  KrylovState &st = *q->krylov;
  LoopClock clk(g, st);
  if (int rc = clk.begin(g)) return rc;
  auto A = [&](IGXVec in, IGXVec out) -> int { return mg_action(q, fine, in, out, &clk); };
  auto M = [&](IGXVec in, IGXVec out) -> int { return mg_cycle(q, fine, in, out, clk); };
  const KrylovPlan kp = {method, rtol, atol, maxit, false, nullptr};
  int its = 0;
  if (int rc = krylov_loop(g, st, clk, kp, A, M, b, x, info, &its, history)) return rc;
  return clk.finish(g, std::string("krylov(") + (cg ? "cg" : "bicgstab") + ", pc=" + mg_name(q) + ", " + q->action + ", " + std::to_string(its) + " iterations)");
}
// One fused Chebyshev step against the four IGXVec kernels it replaces (r = r - w by kr_axpby, z = r / D by kr_pdiv, d = c1 d + c2 z and
// x = x + d by kr_axpby), on the work vectors of a level, for scripts/multigrid_rate.py: per round `reps` launches of each version between
// two events, the versions alternating; fused_ms / split_ms receive the time of ONE step per round.  w is zeroed first, so r keeps its
// values; x and d are overwritten (every cycle starts from a zero guess: nothing depends on them).
extern "C" int IGXMultigridMeasureStep(IGXMultigrid mg, int level, int reps, int rounds, double *fused_ms, double *split_ms) {
  _p_IGXMultigrid *q = reinterpret_cast<_p_IGXMultigrid *>(mg);
  if (int rc = mg_stale(q, "IGXMultigridMeasureStep")) return rc;
  if (level < 0 || level >= q->L) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMultigridMeasureStep: the multigrid's level must be in range [0," + std::to_string(q->L - 1) + "]");
  if (reps < 1 || rounds < 1 || !fused_ms || !split_ms) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMultigridMeasureStep: the multigrid's measurement needs reps >= 1, rounds >= 1 and two arrays of rounds doubles");
  if (!q->ready) return fail(IGX_ERR_ORDER, "Must call IGXMultigridSetUp() before IGXMultigridMeasureStep()");
  MgLevel &l = q->lv[level]; IGX g = l.g; const long long n = (long long)l.n;
  if (l.kind != IGX_PC_JACOBI) return fail(IGX_ERR_SUP, "IGXMultigridMeasureStep: the multigrid's fused step exists for the diagonal alone; with point blocks a step is three launches");
  double *x = l.work[MG_X]->a.as<double>(), *d = l.work[MG_D]->a.as<double>(), *r = l.work[MG_R]->a.as<double>(), *w = l.work[MG_W]->a.as<double>(), *z = l.work[MG_B]->a.as<double>();
  const double *D = l.cols[0]->a.as<double>();
  const double c1 = 0.25, c2 = 0.5;
  const unsigned grid = kr_grid(n);
  for (auto &e : q->ev) if (!e) HIPCK(hipEventCreate(&e));
  HIPCK(hipMemsetAsync(w, 0, (size_t)n * sizeof(double), g->stream));
  auto fused = [&]() -> int { KR_LAUNCH(mg_cheb_step<false>, grid, KR_T, g, x, d, r, w, D, c1, c2, n); return 0; };
  auto split = [&]() -> int {
    KR_LAUNCH(kr_axpby, grid, KR_T, g, r, -1.0, w, 1.0, n);
    KR_LAUNCH(kr_pdiv, grid, KR_T, g, z, r, D, n);
    KR_LAUNCH(kr_axpby, grid, KR_T, g, d, c2, z, c1, n);
    KR_LAUNCH(kr_axpby, grid, KR_T, g, x, 1.0, d, 1.0, n);
    return 0;
  };
  for (int k = 0; k < 3; ++k) { if (int rc = fused()) return rc; if (int rc = split()) return rc; }      // warm-up: both code objects, both access patterns
  for (int round = 0; round < rounds; ++round) for (int version = 0; version < 2; ++version) {
    float ms = 0;
    HIPCK(hipEventRecord(q->ev[0], g->stream));
    for (int k = 0; k < reps; ++k) if (int rc = version ? split() : fused()) return rc;
    HIPCK(hipEventRecord(q->ev[1], g->stream)); HIPCK(hipEventSynchronize(q->ev[1])); HIPCK(hipEventElapsedTime(&ms, q->ev[0], q->ev[1]));
    (version ? split_ms : fused_ms)[round] = (double)ms / reps;
  }
  return 0;
}
