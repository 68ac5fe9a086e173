// solve_loops.hpp -- the host side of the vector algebra on IGXVec and of the device-resident loops: IGXSolve (kernels: krylov.hpp),
// IGXSolveNonlinear (newton.hpp), IGXTimeStep (timestep.hpp) and IGXEigenSolve (block_vec.hpp).  Host code only: it launches kernels and defines none.  Included by the
// main unit (engine.hip) as the last thing before the probe (probe_host.hpp), so every kernel above is compiled as it was before these existed; the three
// kernel headers are included here, where their loops begin, in that order, block_vec.hpp (IGXVecMDot / IGXVecMAXPY) behind the vector algebra,
// and multigrid.hpp (the sweeps of IGXMultigrid's cycle) at the end, before IGXEigenSolve, which zeroes its start block's fixed rows with them.
// What the loops share is written once, up front: the state kept between calls (LoopState), the accounting of launches and kernel time
// (LoopClock), the blocking read of partial sums (read_sums), the entry checks in each solver's own words (SolverWords) and the map from
// the public operator to the matrix-free driver's op (matfree_op).  A new loop costs its own loop.  IGXSolve's two loops are written on
// callables (krylov_loop), so that a second caller with another operator and preconditioner -- IGXMultigridSolve -- runs the same code.
#pragma once

// ------------------------------------------------------------------ what the loops share
// count more zeroed vectors of length n at the end of a list
static int add_vecs(IGX g, int64_t n, int count, std::vector<std::unique_ptr<_p_IGXVec>> &to, const char *failure) {
  for (int k = 0; k < count; ++k) {
    std::unique_ptr<_p_IGXVec> v(new _p_IGXVec()); v->iga = g; v->n = n;
    if (v->a.alloc((size_t)n * sizeof(double)) || hipMemset(v->a.p, 0, v->a.bytes) != hipSuccess) return fail(IGX_ERR_MEM, failure);
    to.push_back(std::move(v));
  }
  return 0;
}
// Work vectors and the two events of a loop's own clock, kept with the IGX between calls (IGXSetUp drops them, IGXDestroy frees them).
struct LoopState {
  int64_t n = 0;
  std::vector<std::unique_ptr<_p_IGXVec>> work;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~LoopState() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
  int ensure(IGX g, int64_t len, int count, const char *failure) { n = len; return add_vecs(g, len, count, work, failure); }      // a new state's work vectors
};
struct KrylovState : LoopState {
  int method = -1, pc = -1, dof = 0;
  std::vector<std::unique_ptr<_p_IGXVec>> pcv;           // work: r z p Ap (CG), r rhat p v s t y z (BiCGStab); pcv: the diagonal or the dof block columns
};
struct NewtonState : LoopState {
  bool has_v = false;                                    // work: F F_t d xs, and V for an IFunction
};
struct TimeStepState : LoopState {                       // work: W x, three rotating U (U0 U1 Uprev), two rotating V (V0 V1)
  int u0 = 2, u1 = 3, uprev = 4, v0 = 5, v1 = 6;         // where the rotation stands
  bool have_prev = false; double hprev = 0;              // U_{n-1} = work[uprev] and h_{n-1} of the last accepted step: what resume = 1 continues from
};

// A loop's figures for IGXGetLastTiming: every launch of the call, the whole call by the loop's own two events and, as kernel time, the
// sum of the operators' own.  With timing on, driver() and finish() block on an event; with timing off nothing here touches the device.
struct LoopClock {
  LoopState &st; const bool timing; int launches = 0; double op_ms = 0;
  LoopClock(IGX g, LoopState &s) : st(s), timing(g->timing) {}
  int begin(IGX g) {
    if (timing) { for (auto &e : st.ev) if (!e) HIPCK(hipEventCreate(&e)); HIPCK(hipEventRecord(st.ev[0], g->stream)); }
    return 0;
  }
  void own(int k) { launches += k; }      // k launches of the loop's own
  int driver(IGX g) {                     // after a driver's entry: its launches and, timed, its kernel time
    launches += g->last_launches;
    if (timing) { float ms = 0; HIPCK(hipEventSynchronize(g->ev[2])); HIPCK(hipEventElapsedTime(&ms, g->ev[1], g->ev[2])); op_ms += ms; }
    return 0;
  }
  void solver(IGX g) { launches += g->last_launches; if (timing) op_ms += g->last_kernel_ms; }      // after an inner loop: the figures it stored
  int finish(IGX g, const std::string &name) {
    g->last_kernel = g->self_timed = name; g->last_launches = launches;
    if (timing) {
      float ms = 0;
      HIPCK(hipEventRecord(st.ev[1], g->stream)); HIPCK(hipEventSynchronize(st.ev[1])); HIPCK(hipEventElapsedTime(&ms, st.ev[0], st.ev[1]));
      g->last_total_ms = ms; g->last_kernel_ms = op_ms;
    }
    return 0;
  }
};

// Each solver's words for the checks they share; the codes and the order are the same for all.  where: the prefix of "this solver runs where
// ..., and <reason>", put before the reason of matfree_refusal's space rules and before an inner IGX_ERR_SUP.  inner: the stepper alone puts every inner
// refusal, of any code, under a prefix of its own.
struct SolverWords { const char *call, *one_rank, *where, *inner; };
static const SolverWords kKrylovWords = {"IGXSolve", "the Krylov solve needs one rank on every axis: the library has no sum across ranks (IGXVecDot gives each rank's part)",
                                         "the Krylov solve runs where its operator and its preconditioner run, and ", nullptr};
static const SolverWords kNewtonWords = {"IGXSolveNonlinear", "the Newton solve needs one rank on every axis: its norms and its linear solve have no sum across ranks",
                                         "the Newton solve runs where its residual and its linear solve run, and ", nullptr};
static const SolverWords kTimeStepWords = {"IGXTimeStep", "the time stepper needs one rank on every axis: its norms and its Newton solve have no sum across ranks",
                                           "the time stepper runs where its Newton solve runs, and ", "IGXTimeStep: the time stepper takes its stages with IGXSolveNonlinear, and "};
// on_ranks: the solver runs on a partition once a communicator is there (IGXSolve); without one, and for every other solver, today's refusal
static int solver_ready(IGX g, const SolverWords &w, bool on_ranks = false) {
  if (!g->s.setup) return fail(IGX_ERR_ORDER, std::string("Must call IGXSetUp() before ") + w.call + "()");
  for (int d = 0; d < g->s.dim; ++d) if (g->s.proc_sizes[d] != 1 && !(on_ranks && g->comm)) return fail(IGX_ERR_SUP, w.one_rank);
  if (g->s.form == IGX_FORM_NONE) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetForm...() first");
  return 0;
}
static int solver_pc_ready(IGX g, const SolverWords &w, int pc) {
  if (pc == IGX_PC_FASTDIAG && !g->fd) return fail(IGX_ERR_ORDER, std::string("Must call IGXFastDiagSetUp() before ") + w.call + "() with IGX_PC_FASTDIAG");
  return 0;
}
static int solver_runs_here(IGX g, const SolverWords &w) {
  if (const MfRefusal r = matfree_refusal(g->s, g->kernel_choice, VsMode::ACTION, nullptr, MfCaller::FORM)) return fail(r.code, w.where + r.msg);
  return 0;
}
// what an operator or an inner loop refused, with its reason under the solver's own name
static int solver_refused(const SolverWords &w, int rc) {
  if (w.inner) return fail(rc, w.inner + std::string(g_err));
  return rc == IGX_ERR_SUP ? fail(rc, w.where + std::string(g_err)) : rc;
}

// ------------------------------------------------------------------ vector algebra on IGXVec and the Krylov loop (krylov.hpp)
#include "krylov.hpp"
// Everything is enqueued on the engine's stream; IGXVecDot / IGXVecNorm2 read their result back and so synchronise.  The sums run over the
// rows this rank owns (a prefix of the row box on every axis, as in IGXChecksum): on several ranks the caller adds the parts (IGXCommAllSum).
static int kr_scalars(IGX g) {
  if (g->krscal.p) return 0;
  if (g->krscal.alloc(KR_SCAL_DOUBLES * sizeof(double))) return fail(IGX_ERR_MEM, "device allocation of the partial-sum slabs failed");
  HIPCK(hipMemset(g->krscal.p, 0, g->krscal.bytes));
  return 0;
}
static double *kr_slab(IGX g, int k) { return g->krscal.as<double>() + (size_t)k * KR_G; }
static double *kr_rec(IGX g) { return g->krscal.as<double>() + (size_t)KR_NSLAB * KR_G; }
static int kr_vec_args(IGXVec a, IGXVec b = nullptr, IGXVec c = nullptr, bool three = false, bool two = false) {
  if (!a || ((two || three) && !b) || (three && !c)) return fail(IGX_ERR_ARG_WRONG, "null vector");
  if ((b && b->iga != a->iga) || (c && c->iga != a->iga)) return fail(IGX_ERR_ARG_WRONG, "vectors created by different IGX");
  if ((b && b->n != a->n) || (c && c->n != a->n)) return fail(IGX_ERR_ARG_WRONG, "vectors of different sizes");
  return 0;
}
#define KR_LAUNCH(kernel, grid, block, g, ...) do { hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (g)->stream, __VA_ARGS__); if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, #kernel ": kernel launch failed"); } while (0)
// the host's blocking read: the first m doubles of the record
static int read_record(IGX g, double *rec, int m) {
  HIPCK(hipMemcpyAsync(rec, kr_rec(g), (size_t)m * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIPCK(hipStreamSynchronize(g->stream));
  return 0;
}
// the sums of the slabs given, added in index order by kr_record (one launch) and read back
static int read_sums(IGX g, std::initializer_list<int> slabs, double *rec) {
  KrSlabs sl; memset(&sl, 0, sizeof(sl));
  for (int k : slabs) sl.s[sl.m++] = kr_slab(g, k);
  KR_LAUNCH(kr_record, 1, 64, g, sl, kr_rec(g));
  return read_record(g, rec, sl.m);
}
extern "C" int IGXVecSet(IGXVec y, double value) {
  if (int rc = kr_vec_args(y)) return rc;
  y->iga->slab_valid = 0;
  KR_LAUNCH(kr_set, kr_grid(y->n), KR_T, y->iga, y->a.as<double>(), value, (long long)y->n);
  return 0;
}
extern "C" int IGXVecCopy(IGXVec x, IGXVec y) {
  if (int rc = kr_vec_args(x, y, nullptr, false, true)) return rc;
  y->iga->slab_valid = 0;
  if (x != y) HIPCK(hipMemcpyAsync(y->a.p, x->a.p, x->a.bytes, hipMemcpyDeviceToDevice, y->iga->stream));
  return 0;
}
extern "C" int IGXVecScale(IGXVec y, double a) {
  if (int rc = kr_vec_args(y)) return rc;
  y->iga->slab_valid = 0;
  KR_LAUNCH(kr_scale, kr_grid(y->n), KR_T, y->iga, y->a.as<double>(), a, (long long)y->n);
  return 0;
}
extern "C" int IGXVecAXPBY(IGXVec y, double a, IGXVec x, double b) {
  if (int rc = kr_vec_args(y, x, nullptr, false, true)) return rc;
  y->iga->slab_valid = 0;
  KR_LAUNCH(kr_axpby, kr_grid(y->n), KR_T, y->iga, y->a.as<double>(), a, x->a.as<double>(), b, (long long)y->n);
  return 0;
}
extern "C" int IGXVecPointwiseDivide(IGXVec z, IGXVec x, IGXVec d) {
  if (int rc = kr_vec_args(z, x, d, true)) return rc;
  z->iga->slab_valid = 0;
  KR_LAUNCH(kr_pdiv, kr_grid(z->n), KR_T, z->iga, z->a.as<double>(), x->a.as<double>(), d->a.as<double>(), (long long)z->n);
  return 0;
}
extern "C" int IGXVecDot(IGXVec x, IGXVec y, double *s) {
  if (int rc = kr_vec_args(x, y, nullptr, false, true)) return rc;
  if (!s) return fail(IGX_ERR_ARG_WRONG, "null result");
  IGX g = x->iga;
  if (int rc = kr_scalars(g)) return rc;
  const Space &sp = g->s;
  int nown[3]; bool all = true;
  for (int d = 0; d < 3; ++d) {
    const AxisLayout &L = sp.lay[d]; nown[d] = 0;
    for (int r = 0; r < L.nrow; ++r) if (L.owned[r]) { if (nown[d] != r) return fail(IGX_ERR_PLIB, "owned rows are not a prefix of the row box"); nown[d]++; }
    if (nown[d] != L.nrow) all = false;
  }
  double *slab = kr_slab(g, KS_USER);
  if (all) KR_LAUNCH(kr_dot, KR_G, KR_T, g, x->a.as<double>(), y->a.as<double>(), (long long)x->n, slab);
  else KR_LAUNCH(kr_dot_owned, KR_G, KR_T, g, x->a.as<double>(), y->a.as<double>(), nown[0], nown[1], nown[2], sp.lay[0].nrow, sp.lay[1].nrow, sp.dof, slab);
  return read_sums(g, {KS_USER}, s);
}
extern "C" int IGXVecNorm2(IGXVec x, double *s) {
  if (int rc = IGXVecDot(x, x, s)) return rc;
  *s = std::sqrt(*s);
  return 0;
}

// ------------------------------------------------------------------ block-vector algebra (block_vec.hpp)
#include "block_vec.hpp"
// IGXVecMDot / IGXVecMAXPY and what IGXEigenSolve launches between its actions.  The state is kept with the IGX: the slab of partial tiles
// (KR_G slots of BV_MAX x BV_MAX), the Gram matrix on the device, the residual sweep's slabs and record, and a ring of BV_RING coefficient
// buffers -- pinned on the host, plain on the device -- so that IGXVecMAXPY can copy C and return without a synchronisation: a slot is
// written again only after the event behind its last copy.
constexpr int BV_RING = 16;
struct BlockVecState : LoopState {
  DevBuf slab, gram, rslab, rrec, cdev;
  double *chost = nullptr; hipEvent_t cev[BV_RING]; bool used[BV_RING]; int next = 0;
  BlockVecState() { for (int k = 0; k < BV_RING; ++k) { cev[k] = nullptr; used[k] = false; } }
  ~BlockVecState() { for (auto &e : cev) if (e) (void)hipEventDestroy(e); if (chost) (void)hipHostFree(chost); }
};
static int bv_state(IGX g) {
  if (g->blockvec) return 0;
  std::shared_ptr<BlockVecState> st(new BlockVecState());
  const size_t tile = (size_t)BV_MAX * BV_MAX;
  if (st->slab.alloc((size_t)KR_G * tile * sizeof(double)) || st->gram.alloc(tile * sizeof(double)) || st->rslab.alloc((size_t)2 * BV_EIG_MAX * KR_G * sizeof(double)) ||
      st->rrec.alloc((size_t)2 * BV_EIG_MAX * sizeof(double)) || st->cdev.alloc((size_t)BV_RING * tile * sizeof(double)))
    return fail(IGX_ERR_MEM, "device allocation of the block-vector buffers failed");
  HIPCK(hipHostMalloc((void **)&st->chost, (size_t)BV_RING * tile * sizeof(double), hipHostMallocDefault));
  for (auto &e : st->cev) HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  g->blockvec = st;
  return 0;
}
// the checks of a pair of blocks, in each call's words: null arrays, the ranges, null entries, one IGX and one length, one rank per axis
static int bv_block_args(const char *fn, int nx, IGXVec X[], int ny, IGXVec Y[], IGX *owner) {
  if (!X || !Y) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": null array of vectors");
  if (nx < 1 || nx > BV_MAX || ny < 1 || ny > BV_MAX) return fail(IGX_ERR_ARG_OUTOFRANGE, std::string(fn) + ": a block holds 1 to " + std::to_string(BV_MAX) + " vectors, got " + std::to_string(nx) + " and " + std::to_string(ny));
  for (int i = 0; i < nx; ++i) if (!X[i]) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": null vector in a block");
  for (int j = 0; j < ny; ++j) if (!Y[j]) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": null vector in a block");
  IGX g = X[0]->iga;
  for (int i = 0; i < nx; ++i) if (X[i]->iga != g || X[i]->n != X[0]->n) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": vectors created by different IGX");
  for (int j = 0; j < ny; ++j) if (Y[j]->iga != g || Y[j]->n != X[0]->n) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": vectors created by different IGX");
  for (int d = 0; d < g->s.dim; ++d) if (g->s.proc_sizes[d] != 1) return fail(IGX_ERR_SUP, std::string(fn) + ": the block-vector algebra needs one rank on every axis: the library has no sum across ranks");
  *owner = g;
  return 0;
}
static void bv_cols(BvCols &c, int n, IGXVec V[]) { memset(&c, 0, sizeof(c)); for (int k = 0; k < n; ++k) c.p[k] = V[k]->a.as<double>(); }
// G = X^T Y on the host: two launches and the blocking read
static int bv_mdot_run(IGX g, int nx, IGXVec X[], int ny, IGXVec Y[], double G[]) {
  BlockVecState &st = *g->blockvec;
  BvCols xc, yc; bv_cols(xc, nx, X); bv_cols(yc, ny, Y);
  const long long n = (long long)X[0]->n;
  const unsigned grid = bv_mdot_grid(n);
  const int count = nx * ny;
  KR_LAUNCH(bv_mdot_kernel((nx + 15) / 16, (ny + 15) / 16), grid, KR_T, g, xc, nx, yc, ny, n, st.slab.as<double>());
  KR_LAUNCH(bv_mdot_finish, (count + 255) / 256, 256, g, st.slab.as<double>(), (int)grid, count, st.gram.as<double>());
  HIPCK(hipMemcpyAsync(G, st.gram.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIPCK(hipStreamSynchronize(g->stream));
  return 0;
}
// Y = beta Y + X C, enqueued: one launch behind the copy of C through the ring
static int bv_maxpy_run(IGX g, int ny, IGXVec Y[], int nx, IGXVec X[], const double C[], double beta) {
  BlockVecState &st = *g->blockvec;
  const int nxb = (nx + 7) / 8, nxp = 8 * nxb, slot = st.next;
  st.next = (st.next + 1) % BV_RING;
  if (st.used[slot]) HIPCK(hipEventSynchronize(st.cev[slot]));
  double *hc = st.chost + (size_t)slot * BV_MAX * BV_MAX, *dc = st.cdev.as<double>() + (size_t)slot * BV_MAX * BV_MAX;
  for (int j = 0; j < ny; ++j) for (int i = 0; i < nxp; ++i) hc[j * nxp + i] = i < nx ? C[i * ny + j] : 0.0;
  HIPCK(hipMemcpyAsync(dc, hc, (size_t)ny * nxp * sizeof(double), hipMemcpyHostToDevice, g->stream));
  HIPCK(hipEventRecord(st.cev[slot], g->stream));
  st.used[slot] = true;
  BvCols xc, yc; bv_cols(xc, nx, X); bv_cols(yc, ny, Y);
  const long long n = (long long)X[0]->n;
  g->slab_valid = 0;
  KR_LAUNCH(bv_maxpy_kernel(nxb), bv_maxpy_grid(n), KR_T, g, yc, ny, xc, nx, dc, beta, n);
  return 0;
}
static int bv_finish(IGX g, LoopClock &clk, const std::string &name) {
  if (int rc = clk.finish(g, name)) return rc;
  if (clk.timing) g->last_kernel_ms = g->last_total_ms;      // nothing but kernels between the two events
  return 0;
}
extern "C" int IGXVecMDot(int nx, IGXVec X[], int ny, IGXVec Y[], double G[]) {
  IGX g = nullptr;
  if (!G) return fail(IGX_ERR_ARG_WRONG, "IGXVecMDot: null result");
  if (int rc = bv_block_args("IGXVecMDot", nx, X, ny, Y, &g)) return rc;
  if (int rc = bv_state(g)) return rc;
  LoopClock clk(g, *g->blockvec);
  if (int rc = clk.begin(g)) return rc;
  if (int rc = bv_mdot_run(g, nx, X, ny, Y, G)) return rc;
  clk.own(2);
  return bv_finish(g, clk, "vec_mdot(" + std::to_string(nx) + " x " + std::to_string(ny) + ", mfma_f64_16x16x4, " + std::to_string((nx + 15) / 16) + " x " + std::to_string((ny + 15) / 16) + " tiles, " + std::to_string(bv_mdot_grid((long long)X[0]->n)) + " slots)");
}
extern "C" int IGXVecMAXPY(int ny, IGXVec Y[], int nx, IGXVec X[], const double C[], double beta) {
  IGX g = nullptr;
  if (!C) return fail(IGX_ERR_ARG_WRONG, "IGXVecMAXPY: null coefficients");
  if (int rc = bv_block_args("IGXVecMAXPY", nx, X, ny, Y, &g)) return rc;
  for (int j = 0; j < ny; ++j) {
    for (int i = 0; i < nx; ++i) if (Y[j] == X[i]) return fail(IGX_ERR_ARG_WRONG, "IGXVecMAXPY: a vector of Y is also a vector of X: every Y_j must differ from every X_i");
    for (int k = 0; k < j; ++k) if (Y[j] == Y[k]) return fail(IGX_ERR_ARG_WRONG, "IGXVecMAXPY: a vector appears twice in Y");
  }
  if (int rc = bv_state(g)) return rc;
  LoopClock clk(g, *g->blockvec);
  if (int rc = clk.begin(g)) return rc;
  if (int rc = bv_maxpy_run(g, ny, Y, nx, X, C, beta)) return rc;
  clk.own(1);
  return bv_finish(g, clk, "vec_maxpy(" + std::to_string(nx) + " -> " + std::to_string(ny) + ", one row per thread, fma in ascending order)");
}

// The two loops of IGXSolve on callables: A(in, out) is the operator, M(in, out) the preconditioner (not called where kp.pc_none says there is
// none: the loops alias the vectors instead), kp.jacobi the diagonal of a Jacobi preconditioner, whose quotient CG fuses with r . z.  Both
// account their own launches on clk.  IGXSolve passes the matrix-free action and its four preconditioners, IGXMultigridSolve the V-cycle.
// st.work: r z p Ap (CG), r rhat p v s t y z (BiCGStab), of length st.n on g.
static bool kr_bad_host(double d) { return !(std::fabs(d) > 0.0) || !std::isfinite(d); }
// On a partition the plan also carries the owned box as runs (krylov.hpp: every sweep then visits the owned entries only) and the number of
// ranks: each group of sums is then added across the ranks in rank order (comm_rank_sum) before anything reads it.  runs == nullptr is one
// rank: every launch, argument and bit as it was before the loop knew of ranks.
struct KrylovPlan { int method; double rtol, atol; int maxit; bool pc_none; const double *jacobi; const KrRuns *runs = nullptr; int ranks = 1; };
template <class FA, class FM>
static int krylov_loop(IGX g, KrylovState &st, LoopClock &clk, const KrylovPlan &kp, FA &&A, FM &&M, IGXVec b, IGXVec x, IGXSolveInfo *info, int *iterations, double *history) {
  const long long n = (long long)st.n;
  double rec[KR_NREC];
  double *drec = kr_rec(g), *dsc = drec + KR_NREC;
  auto record = [&](std::initializer_list<int> slabs) -> int { clk.own(1); return read_sums(g, slabs, rec); };
  auto D = [&](int k) { return st.work[k]->a.as<double>(); };
  auto S = [&](int k) { return kr_slab(g, k); };
  const KrRuns *const rn = kp.runs;
  // the slabs given hold the sum over all ranks afterwards (one rank: nothing to do)
  auto rank_sum = [&](std::initializer_list<int> slabs) -> int {
    if (kp.ranks <= 1) return 0;
    double *sl[KR_NREC]; int m = 0;
    for (int k : slabs) sl[m++] = S(k);
    clk.own(2);
    return comm_rank_sum(g, sl, m);
  };
  // the sweeps: the contiguous kernel over all n entries, or its sibling over the runs of the owned box
  auto k_dot = [&](const double *a, const double *c, int slab) -> int {
    if (rn) KR_LAUNCH(kr_dot_runs, KR_G, KR_T, g, *rn, a, c, S(slab)); else KR_LAUNCH(kr_dot, KR_G, KR_T, g, a, c, n, S(slab));
    return 0;
  };
  double *xd = x->a.as<double>(); const double *bd = b->a.as<double>();
  g->slab_valid = 0;
  int its = 0, reason = 0;
  double bnorm = 0, rnorm = 0, rnorm0 = 0, thr = 0;
  // r = b - A x with |r| and |b|, shared by both methods: the product goes to work vector 3 (Ap / v), r is work vector 0
  if (int rc = A(x, st.work[3].get())) return rc;
  if (rn) KR_LAUNCH(kr_resid0_runs, KR_G, KR_T, g, *rn, D(0), bd, D(3), S(KS_RR), S(KS_BB)); else KR_LAUNCH(kr_resid0, KR_G, KR_T, g, D(0), bd, D(3), n, kr_slab(g, KS_RR), kr_slab(g, KS_BB));
  clk.own(1);
  auto stop = [&]() {      // the test of the recurrence residual, 0 to go on
    if (std::isnan(rnorm)) return (int)IGX_DIVERGED_NAN;
    if (rnorm <= thr) return (int)(rnorm <= kp.rtol * bnorm ? IGX_CONVERGED_RTOL : IGX_CONVERGED_ATOL);
    if (its >= kp.maxit) return (int)IGX_DIVERGED_ITS;
    return 0;
  };
  auto start = [&]() -> bool {      // after the first record (rec[0] = r.r, rec[1] = b.b): true when the loop has something to do
    bnorm = std::sqrt(rec[1]); rnorm0 = rnorm = std::sqrt(rec[0]); thr = std::max(kp.rtol * bnorm, kp.atol);
    if (history) history[0] = rnorm;
    if (std::isnan(bnorm)) { reason = IGX_DIVERGED_NAN; return false; }
    if (bnorm == 0.0) { reason = IGX_CONVERGED_ATOL; return false; }
    return true;
  };
  const bool cg = kp.method == IGX_SOLVE_CG;
  if (cg) {
    IGXVec r = st.work[0].get(), z = kp.pc_none ? r : st.work[1].get(), p = st.work[2].get(), Ap = st.work[3].get();
    int cur = 0;      // KS_A + cur holds the newest r.z, KS_A + 1 - cur the one before; KS_C holds p.Ap
    auto precondition = [&](int slab) -> int {
      if (kp.jacobi) {
        if (rn) KR_LAUNCH(kr_jacobi_rz_runs, KR_G, KR_T, g, *rn, z->a.as<double>(), r->a.as<double>(), kp.jacobi, S(slab)); else KR_LAUNCH(kr_jacobi_rz, KR_G, KR_T, g, z->a.as<double>(), r->a.as<double>(), kp.jacobi, n, kr_slab(g, slab));
        clk.own(1); return 0;
      }
      if (int rc = M(r, z)) return rc;
      if (int rc = k_dot(r->a.as<double>(), z->a.as<double>(), slab)) return rc;
      clk.own(1);
      return 0;
    };
    if (int rc = precondition(KS_A)) return rc;
    if (int rc = rank_sum({KS_RR, KS_BB, KS_A})) return rc;
    if (int rc = record({KS_RR, KS_BB, KS_A})) return rc;
    double rz = rec[2];
    if (start()) {
      HIPCK(hipMemcpyAsync(p->a.p, z->a.p, z->a.bytes, hipMemcpyDeviceToDevice, g->stream));
      while (!(reason = stop())) {
        if (kr_bad_host(rz)) { reason = IGX_DIVERGED_BREAKDOWN; break; }
        if (its > 0) {
          if (rn) KR_LAUNCH(kr_cg_p_runs, kr_run_grid(*rn), KR_T, g, *rn, p->a.as<double>(), z->a.as<double>(), S(KS_A + cur), S(KS_A + 1 - cur));
          else KR_LAUNCH(kr_cg_p, kr_grid(n), KR_T, g, p->a.as<double>(), z->a.as<double>(), n, kr_slab(g, KS_A + cur), kr_slab(g, KS_A + 1 - cur));
          clk.own(1);
        }
        if (int rc = A(p, Ap)) return rc;
        if (int rc = k_dot(p->a.as<double>(), Ap->a.as<double>(), KS_C)) return rc;
        if (int rc = rank_sum({KS_C})) return rc;
        if (rn) KR_LAUNCH(kr_cg_update_runs, KR_G, KR_T, g, *rn, xd, r->a.as<double>(), p->a.as<double>(), Ap->a.as<double>(), S(KS_C), S(KS_A + cur), S(KS_RR));
        else KR_LAUNCH(kr_cg_update, KR_G, KR_T, g, xd, r->a.as<double>(), p->a.as<double>(), Ap->a.as<double>(), n, kr_slab(g, KS_C), kr_slab(g, KS_A + cur), kr_slab(g, KS_RR));
        clk.own(2);
        cur ^= 1;
        if (int rc = precondition(KS_A + cur)) return rc;
        if (int rc = rank_sum({KS_RR, KS_A + cur})) return rc;
        if (int rc = record({KS_RR, KS_C, KS_A + cur})) return rc;
        if (!(rec[1] > 0.0) || !std::isfinite(rec[1])) { reason = IGX_DIVERGED_BREAKDOWN; break; }      // p.Ap <= 0: the update kernel left x and r alone
        ++its; rnorm = std::sqrt(rec[0]); rz = rec[2];
        if (history) history[its] = rnorm;
      }
    }
  } else {
    IGXVec r = st.work[0].get(), rhat = st.work[1].get(), p = st.work[2].get(), v = st.work[3].get(), s = st.work[4].get(), tv = st.work[5].get();
    IGXVec y = kp.pc_none ? p : st.work[6].get(), z = kp.pc_none ? s : st.work[7].get();
    int cur = 0;      // KS_A + cur holds rho' = rhat.r of the iteration at hand; KS_C rhat.v, KS_D t.s, KS_E t.t
    static const double one3[3] = {1.0, 1.0, 1.0};
    HIPCK(hipMemcpyAsync(rhat->a.p, r->a.p, r->a.bytes, hipMemcpyDeviceToDevice, g->stream));
    if (int rc = k_dot(rhat->a.as<double>(), r->a.as<double>(), KS_A)) return rc;
    clk.own(1);
    if (int rc = rank_sum({KS_RR, KS_BB, KS_A})) return rc;
    if (int rc = record({KS_RR, KS_BB, KS_A})) return rc;
    double rho_next = rec[2], omega = 1.0;
    if (start()) {
      HIPCK(hipMemsetAsync(v->a.p, 0, v->a.bytes, g->stream));
      HIPCK(hipMemsetAsync(p->a.p, 0, p->a.bytes, g->stream));
      HIPCK(hipMemcpyAsync(dsc, one3, sizeof(one3), hipMemcpyHostToDevice, g->stream));
      while (!(reason = stop())) {
        if (kr_bad_host(rho_next) || kr_bad_host(omega)) { reason = IGX_DIVERGED_BREAKDOWN; break; }
        if (rn) KR_LAUNCH(kr_bicg_p_runs, kr_run_grid(*rn), KR_T, g, *rn, p->a.as<double>(), r->a.as<double>(), v->a.as<double>(), S(KS_A + cur), dsc);
        else KR_LAUNCH(kr_bicg_p, kr_grid(n), KR_T, g, p->a.as<double>(), r->a.as<double>(), v->a.as<double>(), n, kr_slab(g, KS_A + cur), dsc);
        clk.own(1);
        if (int rc = M(p, y)) return rc;
        if (int rc = A(y, v)) return rc;
        if (int rc = k_dot(rhat->a.as<double>(), v->a.as<double>(), KS_C)) return rc;
        if (int rc = rank_sum({KS_C})) return rc;
        if (rn) KR_LAUNCH(kr_bicg_s_runs, kr_run_grid(*rn), KR_T, g, *rn, s->a.as<double>(), r->a.as<double>(), v->a.as<double>(), S(KS_A + cur), S(KS_C));
        else KR_LAUNCH(kr_bicg_s, kr_grid(n), KR_T, g, s->a.as<double>(), r->a.as<double>(), v->a.as<double>(), n, kr_slab(g, KS_A + cur), kr_slab(g, KS_C));
        clk.own(2);
        if (int rc = M(s, z)) return rc;
        if (int rc = A(z, tv)) return rc;
        if (rn) KR_LAUNCH(kr_dot2_runs, KR_G, KR_T, g, *rn, tv->a.as<double>(), s->a.as<double>(), S(KS_D), S(KS_E)); else KR_LAUNCH(kr_dot2, KR_G, KR_T, g, tv->a.as<double>(), s->a.as<double>(), n, kr_slab(g, KS_D), kr_slab(g, KS_E));
        if (int rc = rank_sum({KS_D, KS_E})) return rc;
        if (rn) KR_LAUNCH(kr_bicg_xr_runs, KR_G, KR_T, g, *rn, xd, r->a.as<double>(), y->a.as<double>(), z->a.as<double>(), s->a.as<double>(), tv->a.as<double>(), rhat->a.as<double>(),
                          S(KS_A + cur), S(KS_C), S(KS_D), S(KS_E), S(KS_RR), S(KS_A + 1 - cur));
        else KR_LAUNCH(kr_bicg_xr, KR_G, KR_T, g, xd, r->a.as<double>(), y->a.as<double>(), z->a.as<double>(), s->a.as<double>(), tv->a.as<double>(), rhat->a.as<double>(), n,
                  kr_slab(g, KS_A + cur), kr_slab(g, KS_C), kr_slab(g, KS_D), kr_slab(g, KS_E), kr_slab(g, KS_RR), kr_slab(g, KS_A + 1 - cur));
        if (int rc = rank_sum({KS_RR, KS_A + 1 - cur})) return rc;
        KR_LAUNCH(kr_bicg_record, 1, 64, g, kr_slab(g, KS_RR), kr_slab(g, KS_A + cur), kr_slab(g, KS_C), kr_slab(g, KS_D), kr_slab(g, KS_E), kr_slab(g, KS_A + 1 - cur), drec, dsc);
        clk.own(3);
        if (int rc = read_record(g, rec, 7)) return rc;
        cur ^= 1;
        if (kr_bad_host(rec[1]) || kr_bad_host(rec[2])) { reason = IGX_DIVERGED_BREAKDOWN; break; }      // rhat.v or t.t: the update kernel left x and r alone
        ++its; rnorm = std::sqrt(rec[0]); rho_next = rec[4]; omega = rec[6];
        if (history) history[its] = rnorm;
      }
    }
  }
  if (reason == IGX_CONVERGED_ATOL && bnorm == 0.0) {      // b = 0: the solution is 0 (on a partition: on the owned rows; the caller's refresh carries it to the ghosts)
    if (rn) KR_LAUNCH(kr_set_runs, kr_run_grid(*rn), KR_T, g, *rn, xd, 0.0); else KR_LAUNCH(kr_set, kr_grid(n), KR_T, g, xd, 0.0, n);
    clk.own(1);
    rnorm0 = rnorm = 0.0; if (history) history[0] = 0.0;
    HIPCK(hipStreamSynchronize(g->stream));
  }
  if (info) { info->iterations = its; info->reason = reason; info->rnorm0 = rnorm0; info->rnorm = rnorm; info->bnorm = bnorm; }
  *iterations = its;
  return 0;
}

// IGXSolve.  The operator is the matrix-free driver's internal entry (compute_matfree) at the state of the specification, the preconditioners
// are the same driver's diagonals and point blocks with block_diagonal_run, and IGXFastDiagApply: whatever they refuse the solve refuses,
// with their reason under its own name.  The loops and their kernels: krylov.hpp.
extern "C" int IGXSolve(IGX g, const IGXSolveSpec *sp, IGXVec b, IGXVec x, IGXSolveInfo *info, double *history) {
  NEEDIGA(g);
  const SolverWords &words = kKrylovWords;
  if (!sp) return fail(IGX_ERR_ARG_WRONG, "null solve specification");
  if (sp->method != IGX_SOLVE_CG && sp->method != IGX_SOLVE_BICGSTAB) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolve: unknown method");
  if (sp->op < IGX_OP_MATRIX || sp->op > IGX_OP_IJACOBIAN) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolve: unknown operator");
  if (sp->pc < IGX_PC_NONE || sp->pc > IGX_PC_FASTDIAG) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolve: unknown preconditioner");
  if (sp->maxit < 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolve: maxit must not be negative");
  if (!(sp->rtol >= 0) || !(sp->atol >= 0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolve: the tolerances must not be negative");
  if (int rc = solver_ready(g, words, true)) return rc;
  // A partition: whatever is refused is refused from what every rank knows alike, before the first message
  const int ranks = g->s.comm_size;
  if (ranks > 1) {
    std::string e;
    if (int rc = exchange_supported(g->s, e)) return fail(rc, words.where + e);
    if (sp->pc == IGX_PC_FASTDIAG) return fail(IGX_ERR_SUP, std::string(words.where) + "fast diagonalisation solves along whole axes and needs one rank on every axis");
    if (ranks > KR_G) return fail(IGX_ERR_SUP, std::string(words.where) + "the sum across ranks holds " + std::to_string(KR_G) + " ranks at the most");
  }
  if (!b || !x) return fail(IGX_ERR_ARG_WRONG, "null right-hand side or solution vector");
  if (b->iga != g || x->iga != g) return fail(IGX_ERR_ARG_WRONG, "vector created by another IGX");
  if (x == b) return fail(IGX_ERR_ARG_WRONG, "the solution and the right-hand side must be different vectors");
  IGXVec U = sp->op == IGX_OP_MATRIX ? nullptr : sp->U, V = sp->op == IGX_OP_IJACOBIAN ? sp->V : nullptr;
  if (sp->op != IGX_OP_MATRIX && !U) return fail(IGX_ERR_ARG_WRONG, "null state vector");
  if (sp->op == IGX_OP_IJACOBIAN && !V) return fail(IGX_ERR_ARG_WRONG, "null state vector");
  if ((U && U->iga != g) || (V && V->iga != g)) return fail(IGX_ERR_ARG_WRONG, "state vector created by another IGX");
  if ((U && U == x) || (V && V == x)) return fail(IGX_ERR_ARG_WRONG, "the solution must not be a state vector");
  if (int rc = solver_pc_ready(g, words, sp->pc)) return rc;
  if (int rc = solver_runs_here(g, words)) return rc;
  if (int rc = ensure_device(g)) return rc;
  const long long n = (long long)g->nbrows * g->s.dof;
  if (b->n != n || x->n != n) return fail(IGX_ERR_ARG_WRONG, "vector of another size than the space's");
  if (int rc = kr_scalars(g)) return rc;
  // the owned box as runs, and the rank sum's buffers
  KrRuns runs = {0, 0, 0, 1, 0};
  if (ranks > 1) {
    int nown[3];
    for (int d = 0; d < 3; ++d) {
      const AxisLayout &L = g->s.lay[d]; nown[d] = 0;
      for (int r = 0; r < L.nrow; ++r) if (L.owned[r]) { if (nown[d] != r) return fail(IGX_ERR_PLIB, "owned rows are not a prefix of the row box"); nown[d]++; }
    }
    runs = kr_runs(nown, g->s.lay[0].nrow, g->s.lay[1].nrow, g->s.dof);
    if (int rc = comm_rank_sum_ready(g)) return rc;
  }
  const bool cg = sp->method == IGX_SOLVE_CG;
  const int dof = g->s.dof, pc = sp->pc;
  const double shift = sp->op == IGX_OP_IJACOBIAN ? sp->a : 0.0, t = sp->op == IGX_OP_IJACOBIAN ? sp->t : 0.0;
  // work vectors: kept while the method and the preconditioner need the same set
  if (!g->krylov || g->krylov->method != sp->method || g->krylov->pc != pc || g->krylov->dof != dof || g->krylov->n != n) {
    g->krylov.reset();
    std::shared_ptr<KrylovState> ks(new KrylovState());
    if (int rc = ks->ensure(g, n, cg ? 4 : 8, "device allocation of the Krylov work vectors failed")) return rc;
    if (int rc = add_vecs(g, n, pc == IGX_PC_JACOBI ? 1 : pc == IGX_PC_PBJACOBI ? dof : 0, ks->pcv, "device allocation of the preconditioner's vectors failed")) return rc;
    ks->method = sp->method; ks->pc = pc; ks->dof = dof;
    g->krylov = ks;
  }
  KrylovState &st = *g->krylov;
  LoopClock clk(g, st);
  if (int rc = clk.begin(g)) return rc;
  std::string opname;
  // on a partition: the ghosts of the input from their owners, the action, the ghost rows of the product to their owners
  auto A = [&](IGXVec in, IGXVec out) -> int {
    if (ranks > 1) if (int rc = IGXRefreshGhosts(g, in)) return solver_refused(words, rc);
    if (int rc = compute_matfree(g, VsMode::ACTION, sp->op, U, V, 1, &in, 1, &out, shift, t)) return solver_refused(words, rc);
    if (opname.empty()) opname = g->last_kernel;
    if (int rc = clk.driver(g)) return rc;
    if (ranks > 1) if (int rc = IGXReduceGhostRows(g, nullptr, out)) return solver_refused(words, rc);
    return 0;
  };
  std::vector<IGXVec> cols; for (auto &v : st.pcv) cols.push_back(v.get());
  if (pc == IGX_PC_JACOBI || pc == IGX_PC_PBJACOBI) {
    if (int rc = compute_matfree(g, pc == IGX_PC_JACOBI ? VsMode::DIAGONAL : VsMode::BLOCK_DIAGONAL, sp->op, U, V, 0, nullptr, (int)cols.size(), cols.data(), shift, t)) return solver_refused(words, rc);
    if (int rc = clk.driver(g)) return rc;
    // on a partition every column is completed on its owner and handed back, so that no local row holds a partial value
    if (ranks > 1) for (IGXVec c : cols) { if (int rc = IGXReduceGhostRows(g, nullptr, c)) return solver_refused(words, rc); if (int rc = IGXRefreshGhosts(g, c)) return solver_refused(words, rc); }
  }
  if (pc == IGX_PC_PBJACOBI) {
    if (int rc = block_diagonal_run(g, dof, cols.data(), nullptr, nullptr, nullptr, true)) return solver_refused(words, rc);
    if (int rc = clk.driver(g)) return rc;
  }
  // out = M^-1 in (IGX_PC_NONE: the caller aliases the two)
  auto M = [&](IGXVec in, IGXVec out) -> int {
    if (pc == IGX_PC_NONE) return 0;
    if (pc == IGX_PC_JACOBI) {
      if (ranks > 1) KR_LAUNCH(kr_pdiv_runs, kr_run_grid(runs), KR_T, g, runs, out->a.as<double>(), in->a.as<double>(), cols[0]->a.as<double>());
      else KR_LAUNCH(kr_pdiv, kr_grid(n), KR_T, g, out->a.as<double>(), in->a.as<double>(), cols[0]->a.as<double>(), n);
      clk.own(1); return 0;
    }
    if (int rc = pc == IGX_PC_PBJACOBI ? block_diagonal_run(g, dof, cols.data(), in, out, nullptr, false) : IGXFastDiagApply(g, in, out)) return solver_refused(words, rc);
    return clk.driver(g);
  };
  KrylovPlan kp = {sp->method, sp->rtol, sp->atol, sp->maxit, pc == IGX_PC_NONE, pc == IGX_PC_JACOBI ? cols[0]->a.as<double>() : nullptr};
  if (ranks > 1) { kp.runs = &runs; kp.ranks = ranks; }
  int its = 0;
  if (int rc = krylov_loop(g, st, clk, kp, A, M, b, x, info, &its, history)) return rc;
  if (ranks > 1) if (int rc = IGXRefreshGhosts(g, x)) return solver_refused(words, rc);      // x leaves with its ghosts, as the actions take it
  static const char *const methods[2] = {"cg", "bicgstab"}, *const pcs[4] = {"none", "jacobi", "pbjacobi", "fastdiag"};
  return clk.finish(g, std::string("krylov(") + methods[sp->method] + ", pc=" + pcs[pc] + ", " + opname + ", " + std::to_string(its) + " iterations" + (ranks > 1 ? ", " + std::to_string(ranks) + " ranks)" : ")"));
}

// The measurement hook of scripts/solve_ranks_rate.py: the mean time in ms of `reps` launches of one sweep of the two loops, after 3 untimed
// ones, by two events on the engine stream.  runs = 1: the run form over the owned box of this IGX's partition (no communicator needed);
// runs = 0: the contiguous sibling over the same NUMBER of entries.  The vectors are the call's own (ones), the slabs are set so that no
// kernel takes its skip path and every coefficient is 1; the slabs are zeroed again before the call returns.
extern "C" int IGXKrylovSweepTime(IGX g, int sweep, int runs, int reps, double *ms) {
  NEEDIGA(g);
  if (!ms) return fail(IGX_ERR_ARG_WRONG, "IGXKrylovSweepTime: null result");
  if (sweep < 0 || sweep >= IGX_SWEEP_COUNT || reps < 1 || (runs != 0 && runs != 1)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXKrylovSweepTime: unknown sweep or form, or reps < 1");
  if (!g->s.setup) return fail(IGX_ERR_ORDER, "Must call IGXSetUp() before IGXKrylovSweepTime()");
  if (int rc = ensure_device(g)) return rc;
  if (int rc = kr_scalars(g)) return rc;
  int nown[3];
  for (int d = 0; d < 3; ++d) { const AxisLayout &L = g->s.lay[d]; nown[d] = 0; for (int r = 0; r < L.nrow; ++r) if (L.owned[r]) nown[d]++; }
  const KrRuns rn = kr_runs(nown, g->s.lay[0].nrow, g->s.lay[1].nrow, g->s.dof);
  const long long n = rn.len * rn.n1 * rn.n2, nall = (long long)g->nbrows * g->s.dof;      // the owned entries; the local vector
  std::vector<std::unique_ptr<_p_IGXVec>> v;
  if (int rc = add_vecs(g, nall, 7, v, "device allocation of the sweep probe's vectors failed")) return rc;
  auto D = [&](int k) { return v[k]->a.as<double>(); };
  auto S = [&](int k) { return kr_slab(g, k); };
  for (int k = 0; k < 7; ++k) KR_LAUNCH(kr_set, kr_grid(nall), KR_T, g, D(k), 1.0, nall);
  double *sc = kr_rec(g) + KR_NREC;
  static const double scal[3] = {(double)KR_G, 1.0, 1.0};      // rho of the iteration before = the slab sum of rho': beta = 1
  auto launch = [&]() -> int {
    switch (sweep) {
      case IGX_SWEEP_RESID0: if (runs) KR_LAUNCH(kr_resid0_runs, KR_G, KR_T, g, rn, D(0), D(1), D(2), S(KS_RR), S(KS_BB)); else KR_LAUNCH(kr_resid0, KR_G, KR_T, g, D(0), D(1), D(2), n, S(KS_RR), S(KS_BB)); break;
      case IGX_SWEEP_DOT: if (runs) KR_LAUNCH(kr_dot_runs, KR_G, KR_T, g, rn, D(0), D(1), S(KS_USER)); else KR_LAUNCH(kr_dot, KR_G, KR_T, g, D(0), D(1), n, S(KS_USER)); break;
      case IGX_SWEEP_DOT2: if (runs) KR_LAUNCH(kr_dot2_runs, KR_G, KR_T, g, rn, D(0), D(1), S(KS_USER), S(KS_BB)); else KR_LAUNCH(kr_dot2, KR_G, KR_T, g, D(0), D(1), n, S(KS_USER), S(KS_BB)); break;
      case IGX_SWEEP_JACOBI_RZ: if (runs) KR_LAUNCH(kr_jacobi_rz_runs, KR_G, KR_T, g, rn, D(0), D(1), D(2), S(KS_USER)); else KR_LAUNCH(kr_jacobi_rz, KR_G, KR_T, g, D(0), D(1), D(2), n, S(KS_USER)); break;
      case IGX_SWEEP_CG_UPDATE: if (runs) KR_LAUNCH(kr_cg_update_runs, KR_G, KR_T, g, rn, D(0), D(1), D(2), D(3), S(KS_C), S(KS_A), S(KS_RR)); else KR_LAUNCH(kr_cg_update, KR_G, KR_T, g, D(0), D(1), D(2), D(3), n, S(KS_C), S(KS_A), S(KS_RR)); break;
      case IGX_SWEEP_BICG_XR:
        if (runs) KR_LAUNCH(kr_bicg_xr_runs, KR_G, KR_T, g, rn, D(0), D(1), D(2), D(3), D(4), D(5), D(6), S(KS_A), S(KS_C), S(KS_D), S(KS_E), S(KS_RR), S(KS_BB));
        else KR_LAUNCH(kr_bicg_xr, KR_G, KR_T, g, D(0), D(1), D(2), D(3), D(4), D(5), D(6), n, S(KS_A), S(KS_C), S(KS_D), S(KS_E), S(KS_RR), S(KS_BB));
        break;
      case IGX_SWEEP_CG_P: if (runs) KR_LAUNCH(kr_cg_p_runs, kr_run_grid(rn), KR_T, g, rn, D(0), D(1), S(KS_A), S(KS_C)); else KR_LAUNCH(kr_cg_p, kr_grid(n), KR_T, g, D(0), D(1), n, S(KS_A), S(KS_C)); break;
      case IGX_SWEEP_BICG_P: if (runs) KR_LAUNCH(kr_bicg_p_runs, kr_run_grid(rn), KR_T, g, rn, D(0), D(1), D(2), S(KS_A), sc); else KR_LAUNCH(kr_bicg_p, kr_grid(n), KR_T, g, D(0), D(1), D(2), n, S(KS_A), sc); break;
      case IGX_SWEEP_BICG_S: if (runs) KR_LAUNCH(kr_bicg_s_runs, kr_run_grid(rn), KR_T, g, rn, D(0), D(1), D(2), S(KS_A), S(KS_C)); else KR_LAUNCH(kr_bicg_s, kr_grid(n), KR_T, g, D(0), D(1), D(2), n, S(KS_A), S(KS_C)); break;
      case IGX_SWEEP_PDIV: if (runs) KR_LAUNCH(kr_pdiv_runs, kr_run_grid(rn), KR_T, g, rn, D(0), D(1), D(2)); else KR_LAUNCH(kr_pdiv, kr_grid(n), KR_T, g, D(0), D(1), D(2), n); break;
      default: if (runs) KR_LAUNCH(kr_set_runs, kr_run_grid(rn), KR_T, g, rn, D(0), 1.0); else KR_LAUNCH(kr_set, kr_grid(n), KR_T, g, D(0), 1.0, n); break;
    }
    return 0;
  };
  struct Events { hipEvent_t e[2] = {nullptr, nullptr}; ~Events() { for (auto &x : e) if (x) (void)hipEventDestroy(x); } } ev;      // (freed on every way out)
  for (auto &x : ev.e) HIPCK(hipEventCreate(&x));
  const hipEvent_t e0 = ev.e[0], e1 = ev.e[1];
  int rc = 0; float t = 0;
  for (int k = -3; k < reps && !rc; ++k) {
    // the slabs a sweep reads hold 1 in every entry again (a sweep before may have written some of them)
    if (k <= 0) {
      hipLaunchKernelGGL(kr_set, dim3(kr_grid((long long)KR_NSLAB * KR_G)), dim3(KR_T), 0, g->stream, g->krscal.as<double>(), 1.0, (long long)KR_NSLAB * KR_G);
      if (hipGetLastError() != hipSuccess) { rc = fail(IGX_ERR_LIB, "kr_set: kernel launch failed"); break; }
      if (hipMemcpyAsync(sc, scal, sizeof(scal), hipMemcpyHostToDevice, g->stream) != hipSuccess) { rc = fail(IGX_ERR_LIB, "IGXKrylovSweepTime: copy of the scalars failed"); break; }
      if (k == 0 && hipEventRecord(e0, g->stream) != hipSuccess) { rc = fail(IGX_ERR_LIB, "IGXKrylovSweepTime: hipEventRecord failed"); break; }
    }
    rc = launch();
  }
  if (!rc && (hipEventRecord(e1, g->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess)) rc = fail(IGX_ERR_LIB, "IGXKrylovSweepTime: the timed launches failed");
  (void)hipMemsetAsync(g->krscal.p, 0, g->krscal.bytes, g->stream);
  (void)hipStreamSynchronize(g->stream);
  if (rc) return rc;
  *ms = (double)t / reps;
  return 0;
}

// ------------------------------------------------------------------ the Newton loop (newton.hpp)
#include "newton.hpp"
// IGXSolveNonlinear.  The residual is the vector driver's internal entry (compute: what IGXComputeFunction / IGXComputeIFunction call), the
// linear solve is IGXSolve itself: whatever they refuse the Newton solve refuses, with their reason under its own name.  The loop is the
// one the header states; between two operator calls a trial is one sweep of newton.hpp.
// what the specification alone decides (IGXTimeStep asks the same of the spec it passes on)
static int nw_spec_refusal(const IGXNewtonSpec *sp) {
  if (sp->op == IGX_OP_MATRIX) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolveNonlinear: a linear operator has no Newton loop (IGX_OP_MATRIX: call IGXSolve)");
  if (sp->op != IGX_OP_JACOBIAN && sp->op != IGX_OP_IJACOBIAN) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolveNonlinear: unknown operator");
  if (sp->method != IGX_SOLVE_CG && sp->method != IGX_SOLVE_BICGSTAB) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolveNonlinear: unknown method");
  if (sp->pc < IGX_PC_NONE || sp->pc > IGX_PC_FASTDIAG) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolveNonlinear: unknown preconditioner");
  if (sp->linesearch != IGX_LINESEARCH_BASIC && sp->linesearch != IGX_LINESEARCH_BT) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolveNonlinear: unknown line search");
  if (sp->forcing != IGX_FORCING_CONSTANT && sp->forcing != IGX_FORCING_EW2) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolveNonlinear: unknown forcing");
  if (!(sp->lin_rtol >= 0) || !(sp->lin_atol >= 0) || !(sp->rtol >= 0) || !(sp->atol >= 0) || !(sp->stol >= 0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolveNonlinear: the tolerances must not be negative");
  if (sp->maxit < 0 || sp->lin_maxit < 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolveNonlinear: maxit and lin_maxit must not be negative");
  if (sp->max_backtracks < 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXSolveNonlinear: max_backtracks must not be negative");
  return 0;
}
extern "C" int IGXSolveNonlinear(IGX g, const IGXNewtonSpec *sp, IGXVec x, IGXNewtonInfo *info, double *history, int *linear_its) {
  NEEDIGA(g);
  const SolverWords &words = kNewtonWords;
  if (!sp) return fail(IGX_ERR_ARG_WRONG, "null Newton specification");
  if (int rc = nw_spec_refusal(sp)) return rc;
  if (int rc = solver_ready(g, words)) return rc;
  if (int rc = solver_pc_ready(g, words, sp->pc)) return rc;
  const bool ifun = sp->op == IGX_OP_IJACOBIAN;
  IGXVec W = ifun ? sp->W : nullptr;
  if (ifun && !W) return fail(IGX_ERR_ARG_WRONG, "IGXSolveNonlinear: IGX_OP_IJACOBIAN needs the vector W of V = a U + W");
  if (!x) return fail(IGX_ERR_ARG_WRONG, "null solution vector");
  if (x->iga != g || (W && W->iga != g)) return fail(IGX_ERR_ARG_WRONG, "vector created by another IGX");
  if (W == x) return fail(IGX_ERR_ARG_WRONG, "W and the solution must be different vectors");
  if (int rc = solver_runs_here(g, words)) return rc;
  if (int rc = ensure_device(g)) return rc;
  const long long n = (long long)g->nbrows * g->s.dof;
  if (x->n != n || (W && W->n != n)) return fail(IGX_ERR_ARG_WRONG, "vector of another size than the space's");
  if (int rc = kr_scalars(g)) return rc;
  if (!g->newton || g->newton->n != n || g->newton->has_v != ifun) {
    g->newton.reset();
    std::shared_ptr<NewtonState> ns(new NewtonState());
    if (int rc = ns->ensure(g, n, ifun ? 5 : 4, "device allocation of the Newton work vectors failed")) return rc;
    ns->has_v = ifun;
    g->newton = ns;
  }
  NewtonState &st = *g->newton;
  IGXVec F = st.work[0].get(), Ft = st.work[1].get(), d = st.work[2].get(), xs = st.work[3].get(), V = ifun ? st.work[4].get() : nullptr;
  const bool bt = sp->linesearch == IGX_LINESEARCH_BT;
  LoopClock clk(g, st);
  if (int rc = clk.begin(g)) return rc;
  std::string linname = "no linear solve";
  double *xd = x->a.as<double>(), *Vd = V ? V->a.as<double>() : nullptr; const double *Wd = W ? W->a.as<double>() : nullptr;
  const double shift = ifun ? sp->a : 0.0, t = ifun ? sp->t : 0.0;
  double rec[3] = {0, 0, 0};
  int evals = 0;
  // F_out = G(x) with the state V as the last sweep left it; rec = (F.F, d.d, x.x), the last two only after a trial sweep
  auto residual = [&](IGXVec out, bool trial) -> int {
    if (int rc = compute(g, ifun ? OP_IFUNCTION : OP_FUNCTION, nullptr, out, x, V, shift, t)) return solver_refused(words, rc);
    if (int rc = clk.driver(g)) return rc;
    KR_LAUNCH(kr_dot, KR_G, KR_T, g, out->a.as<double>(), out->a.as<double>(), n, kr_slab(g, KS_RR));
    clk.own(2); ++evals;
    return trial ? read_sums(g, {KS_RR, KS_A, KS_B}, rec) : read_sums(g, {KS_RR}, rec);
  };
  g->slab_valid = 0;
  int its = 0, reason = 0, lin_total = 0, backtracks = 0, last_lin = 0;
  double fnorm0 = 0, f = 0, snorm = 0, xnorm = 0, eta = sp->lin_rtol, fprev = 0;
  if (ifun) { KR_LAUNCH(nw_state, kr_grid(n), KR_T, g, Vd, xd, Wd, shift, n); clk.own(1); }
  if (int rc = residual(F, false)) return rc;
  fnorm0 = f = std::sqrt(rec[0]);
  if (history) history[0] = f;
  if (std::isnan(f)) reason = IGX_NEWTON_DIVERGED_FNORM_NAN;
  else if (f <= sp->atol) reason = IGX_NEWTON_CONVERGED_FNORM_ABS;
  else if (sp->maxit == 0) reason = IGX_NEWTON_DIVERGED_MAX_IT;
  while (!reason) {
    // the linear solve J(x) d = F from d = 0, to eta
    if (sp->forcing == IGX_FORCING_EW2 && its > 0) {
      const double q = f / fprev, floor_ = 0.9 * (eta * eta);
      double e = 0.9 * (q * q);
      if (floor_ > 0.1 && e < floor_) e = floor_;
      eta = e > 0.9 ? 0.9 : e;
    }
    KR_LAUNCH(kr_set, kr_grid(n), KR_T, g, d->a.as<double>(), 0.0, n); clk.own(1);
    IGXSolveSpec ls; memset(&ls, 0, sizeof(ls));
    ls.method = sp->method; ls.op = sp->op; ls.pc = sp->pc; ls.a = shift; ls.t = t; ls.V = V; ls.U = x; ls.rtol = eta; ls.atol = sp->lin_atol; ls.maxit = sp->lin_maxit;
    IGXSolveInfo li; memset(&li, 0, sizeof(li));
    if (int rc = IGXSolve(g, &ls, F, d, &li, nullptr)) return solver_refused(words, rc);
    clk.solver(g);
    linname = g->last_kernel;
    lin_total += li.iterations; last_lin = li.reason;
    if (linear_its) linear_its[its] = li.iterations;
    if (li.reason == IGX_DIVERGED_BREAKDOWN || li.reason == IGX_DIVERGED_NAN) { reason = IGX_NEWTON_DIVERGED_LINEAR_SOLVE; break; }
    // the line search: one sweep and one residual per trial
    double lambda = 1.0; int halvings = 0; bool accepted = false;
    KR_LAUNCH(nw_first_trial, KR_G, KR_T, g, xd, xs->a.as<double>(), d->a.as<double>(), Vd, Wd, shift, n, kr_slab(g, KS_A), kr_slab(g, KS_B)); clk.own(1);
    for (;;) {
      if (int rc = residual(Ft, true)) {      // x holds a trial that was never judged: hand back the last accepted iterate with the driver's error
        (void)hipMemcpyAsync(x->a.p, xs->a.p, x->a.bytes, hipMemcpyDeviceToDevice, g->stream); (void)hipStreamSynchronize(g->stream);
        return rc;
      }
      const double ft = std::sqrt(rec[0]);
      if (!bt) { if (std::isnan(ft)) reason = IGX_NEWTON_DIVERGED_FNORM_NAN; else accepted = true; }
      else if (std::isfinite(ft) && ft <= (1.0 - 1e-4 * lambda) * f) accepted = true;
      else if (halvings == sp->max_backtracks) reason = IGX_NEWTON_DIVERGED_LINE_SEARCH;
      if (accepted) { fprev = f; f = ft; break; }
      if (reason) break;
      lambda *= 0.5; ++halvings; ++backtracks;
      KR_LAUNCH(nw_back_trial, KR_G, KR_T, g, xd, xs->a.as<double>(), d->a.as<double>(), Vd, Wd, shift, lambda, n, kr_slab(g, KS_A), kr_slab(g, KS_B)); clk.own(1);
    }
    if (!accepted) {      // x is the last accepted iterate again, bit for bit
      HIPCK(hipMemcpyAsync(x->a.p, xs->a.p, x->a.bytes, hipMemcpyDeviceToDevice, g->stream)); HIPCK(hipStreamSynchronize(g->stream));
      break;
    }
    snorm = lambda * std::sqrt(rec[1]); xnorm = std::sqrt(rec[2]);
    std::swap(F, Ft);
    ++its;
    if (history) history[its] = f;
    if (std::isnan(f)) reason = IGX_NEWTON_DIVERGED_FNORM_NAN;
    else if (f <= sp->atol) reason = IGX_NEWTON_CONVERGED_FNORM_ABS;
    else if (f <= sp->rtol * fnorm0) reason = IGX_NEWTON_CONVERGED_FNORM_RELATIVE;
    else if (snorm <= sp->stol * xnorm) reason = IGX_NEWTON_CONVERGED_SNORM_RELATIVE;
    else if (its >= sp->maxit) reason = IGX_NEWTON_DIVERGED_MAX_IT;
  }
  if (int rc = clk.finish(g, std::string("newton(") + (bt ? "bt" : "basic") + ", " + linname + ", " + std::to_string(its) + " iterations)")) return rc;
  if (info) {
    info->iterations = its; info->reason = reason; info->linear_iterations = lin_total; info->function_evaluations = evals; info->backtracks = backtracks;
    info->last_linear_reason = last_lin; info->fnorm0 = fnorm0; info->fnorm = f; info->snorm = snorm; info->xnorm = xnorm;
  }
  return 0;
}

// ------------------------------------------------------------------ the generalized-alpha time loop (timestep.hpp)
#include "timestep.hpp"
// IGXTimeStep.  Every stage is IGXSolveNonlinear itself: whatever it refuses the stepper refuses, with its reason under the stepper's name.
// The loop is the one the header states; around a Newton solve an attempt is the two sweeps of timestep.hpp and one record of two sums.
extern "C" int IGXTimeStep(IGX g, const IGXTimeStepSpec *sp, IGXVec U, IGXVec V, IGXTimeStepInfo *info, IGXTimeStepLog *log, int nlog) {
  NEEDIGA(g);
  const SolverWords &words = kTimeStepWords;
  if (!sp) return fail(IGX_ERR_ARG_WRONG, "null time-step specification");
  if (sp->newton.op != IGX_OP_IJACOBIAN) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: newton.op must be IGX_OP_IJACOBIAN (the stepper is first order in time on an IFunction)");
  if (!(sp->alpha_m > 0) || !std::isfinite(sp->alpha_m)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: alpha_m must be positive and finite");
  if (!(sp->alpha_f > 0) || !std::isfinite(sp->alpha_f)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: alpha_f must be positive and finite");
  if (!(sp->gamma > 0) || !std::isfinite(sp->gamma)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: gamma must be positive and finite");
  if (!(sp->dt > 0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: dt must be positive");
  if (!(sp->max_time >= sp->t0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: max_time must not be below t0");
  if (sp->max_steps < 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: max_steps must not be negative");
  if (sp->max_rejections < 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: max_rejections must not be negative");
  if (!(sp->adapt_rtol >= 0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: adapt_rtol must not be negative");
  if (!(sp->adapt_atol >= 0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: adapt_atol must not be negative");
  if (!(sp->dt_min >= 0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: dt_min must not be negative");
  if (!(sp->dt_max >= 0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: dt_max must not be negative");
  if (sp->dt_max < sp->dt_min) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: dt_max must not be below dt_min");
  if (sp->adapt && sp->adapt_rtol == 0 && sp->adapt_atol == 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTimeStep: adapt needs a positive adapt_rtol or adapt_atol");
  if (int rc = nw_spec_refusal(&sp->newton)) return fail(rc, "IGXTimeStep: newton: " + std::string(g_err));
  if (int rc = solver_ready(g, words)) return rc;
  if (int rc = solver_pc_ready(g, words, sp->newton.pc)) return rc;
  if (!U || !V) return fail(IGX_ERR_ARG_WRONG, "IGXTimeStep: null U or V");
  if (U->iga != g || V->iga != g) return fail(IGX_ERR_ARG_WRONG, "vector created by another IGX");
  if (U == V) return fail(IGX_ERR_ARG_WRONG, "IGXTimeStep: U and V must be different vectors");
  if (U->n != V->n) return fail(IGX_ERR_ARG_WRONG, "vector of another size than the space's");
  if (sp->resume && !(g->timestep && g->timestep->have_prev && g->timestep->n == U->n)) return fail(IGX_ERR_ORDER, "IGXTimeStep: resume = 1 without a previous call on vectors of this length whose U_{n-1} the IGX still holds");
  if (int rc = solver_runs_here(g, words)) return rc;
  if (int rc = ensure_device(g)) return rc;
  const long long n = (long long)g->nbrows * g->s.dof;
  if (U->n != n) return fail(IGX_ERR_ARG_WRONG, "vector of another size than the space's");
  IGXTimeStepInfo out; memset(&out, 0, sizeof(out));
  out.t = sp->t0; out.dt_next = sp->dt;
  if (sp->max_steps == 0 || sp->t0 == sp->max_time) {      // nothing to do, nothing launched
    out.reason = sp->max_steps == 0 ? IGX_TS_CONVERGED_STEPS : IGX_TS_CONVERGED_TIME;
    if (info) *info = out;
    return 0;
  }
  if (int rc = kr_scalars(g)) return rc;
  if (!g->timestep || g->timestep->n != n) {
    g->timestep.reset();
    std::shared_ptr<TimeStepState> ts(new TimeStepState());
    if (int rc = ts->ensure(g, n, 7, "device allocation of the time stepper's work vectors failed")) return rc;
    g->timestep = ts;
  }
  TimeStepState &st = *g->timestep;
  if (!sp->resume) st.have_prev = false;
  IGXVec W = st.work[0].get(), x = st.work[1].get();
  auto D = [&](int k) { return st.work[k]->a.as<double>(); };
  LoopClock clk(g, st);
  if (int rc = clk.begin(g)) return rc;
  std::string nwname = "no newton solve";
  HIPCK(hipMemcpyAsync(D(st.u0), U->a.p, U->a.bytes, hipMemcpyDeviceToDevice, g->stream));
  HIPCK(hipMemcpyAsync(D(st.v0), V->a.p, V->a.bytes, hipMemcpyDeviceToDevice, g->stream));
  const double am = sp->alpha_m, af = sp->alpha_f, gm = sp->gamma;
  double t = sp->t0, h = sp->dt;
  double rec[2] = {0, 0};
  int reason = 0, rc_out = 0;
  while (!reason) {
    int rejections = 0;
    for (;;) {      // the attempts of one step
      const double p = h;
      const double left = sp->max_time - t;
      const bool shortened = left <= (1.0 + 1e-9) * h;      // ... or a remainder of rounding size would be left over
      if (shortened) h = left;
      const double a = am / (af * gm * h), c0 = 1.0 - am / gm;
      KR_LAUNCH(ts_stage, kr_grid(n), KR_T, g, D(0), D(1), D(st.u0), D(st.v0), c0, a, n); clk.own(1);
      IGXNewtonSpec ns = sp->newton; ns.op = IGX_OP_IJACOBIAN; ns.a = a; ns.t = t + af * h; ns.W = W;
      IGXNewtonInfo ni; memset(&ni, 0, sizeof(ni));
      if (int rc = IGXSolveNonlinear(g, &ns, x, &ni, nullptr, nullptr)) { rc_out = solver_refused(words, rc); break; }
      clk.solver(g);
      nwname = g->last_kernel;
      out.newton_iterations += ni.iterations; out.linear_iterations += ni.linear_iterations; out.function_evaluations += ni.function_evaluations;
      IGXTimeStepLog *lg = log && out.attempts < nlog ? log + out.attempts : nullptr;
      ++out.attempts;
      if (lg) { lg->t = t; lg->dt = h; lg->wlte = -1.0; lg->accepted = 0; lg->newton_iterations = ni.iterations; lg->newton_reason = ni.reason; lg->linear_iterations = ni.linear_iterations; }
      if (ni.reason < 0) {      // a failed attempt
        if (!sp->adapt) { reason = IGX_TS_DIVERGED_NONLINEAR_SOLVE; break; }
        ++rejections; ++out.rejections; h = h / 4;
        if (rejections > sp->max_rejections || h < sp->dt_min) { reason = IGX_TS_DIVERGED_NONLINEAR_SOLVE; break; }
        continue;
      }
      const bool estimate = sp->adapt && st.have_prev;
      TsUpdate k; memset(&k, 0, sizeof(k));
      k.c1 = 1.0 / af; k.c2 = 1.0 / (gm * h); k.c3 = 1.0 - 1.0 / gm; k.atol = sp->adapt_atol; k.rtol = sp->adapt_rtol;
      if (estimate) { const double r = 1.0 + st.hprev / h; k.d1 = r; k.d2 = r - 1.0; k.d3 = r * (r - 1.0); }
      if (estimate) KR_LAUNCH(ts_update<true>, KR_G, KR_T, g, D(st.u1), D(st.v1), D(1), D(st.u0), D(st.v0), D(st.uprev), k, n, kr_slab(g, KS_A), kr_slab(g, KS_B));
      else KR_LAUNCH(ts_update<false>, KR_G, KR_T, g, D(st.u1), D(st.v1), D(1), D(st.u0), D(st.v0), (const double *)nullptr, k, n, kr_slab(g, KS_A), kr_slab(g, KS_B));
      clk.own(2);
      if (int rc = read_sums(g, {KS_A, KS_B}, rec)) return rc;
      const double unorm = std::sqrt(rec[0]), wlte = estimate ? std::sqrt(rec[1] / (double)n) : -1.0;
      if (lg) lg->wlte = wlte;
      if (std::isnan(unorm) || std::isnan(wlte)) { reason = IGX_TS_DIVERGED_NAN; break; }
      double next = p;
      if (estimate) {
        const double fac = wlte == 0.0 ? 10.0 : std::min(10.0, std::max(0.1, 0.9 / std::sqrt(wlte)));
        if (!(wlte <= 1.0)) {      // rejected by the estimate
          ++rejections; ++out.rejections; h = fac * h;
          if (rejections > sp->max_rejections || h < sp->dt_min) { reason = IGX_TS_DIVERGED_STEP_REJECTED; break; }
          continue;
        }
        if (!shortened) next = std::min(sp->dt_max, std::max(sp->dt_min, fac * h));
      }
      // accepted: Uprev <- U0 <- U1, V0 <- V1 by pointer
      if (lg) lg->accepted = 1;
      { const int old = st.uprev; st.uprev = st.u0; st.u0 = st.u1; st.u1 = old; std::swap(st.v0, st.v1); }
      st.have_prev = true; st.hprev = h;
      t = shortened ? sp->max_time : t + h;
      ++out.steps; out.dt_last = h; out.unorm = unorm;
      h = next;
      if (t == sp->max_time) reason = IGX_TS_CONVERGED_TIME;
      else if (out.steps == sp->max_steps) reason = IGX_TS_CONVERGED_STEPS;
      break;
    }
    if (rc_out) break;
  }
  // the caller's U and V are written once, here: the last accepted state
  if (out.steps > 0) {
    (void)hipMemcpyAsync(U->a.p, D(st.u0), U->a.bytes, hipMemcpyDeviceToDevice, g->stream);
    (void)hipMemcpyAsync(V->a.p, D(st.v0), V->a.bytes, hipMemcpyDeviceToDevice, g->stream);
  }
  if (rc_out) { (void)hipStreamSynchronize(g->stream); return rc_out; }
  HIPCK(hipStreamSynchronize(g->stream));
  char scheme[96]; snprintf(scheme, sizeof(scheme), "timestep(am=%g, af=%g, g=%g, ", am, af, gm);
  if (int rc = clk.finish(g, std::string(scheme) + nwname + ", " + std::to_string(out.steps) + " steps, " + std::to_string(out.rejections) + " rejections)")) return rc;
  out.reason = reason; out.t = t; out.dt_next = h;
  if (info) *info = out;
  return 0;
}

// ------------------------------------------------------------------ the multigrid cycle's sweeps (multigrid.hpp)
#include "multigrid.hpp"
// IGXMultigrid's host side calls the transfer and so stands behind it (multigrid_host.hpp); its outer loop is krylov_loop above.

// ------------------------------------------------------------------ the eigen solve (LOBPCG; its sweeps: block_vec.hpp)
// IGXEigenSolve.  The two operators are the matrix-free driver's internal entry on stiff and on mass (both on stiff's vectors: the same
// space and layout), the preconditioners are IGXSolve's, the Gram matrices and the updates are the block-vector algebra above, the
// Rayleigh-Ritz step is host.cpp's dense symmetric-definite solver.  The loop is the one the header states, line by line.
struct EigenState : LoopState {
  int m = 0, pc = -1, dof = 0, nblocks = 0;
  std::vector<std::unique_ptr<_p_IGXVec>> pcv;           // the diagonal or the dof block columns
};
static const SolverWords kEigenWords = {"IGXEigenSolve", "IGXEigenSolve: the eigen solve needs one rank on every axis: its Gram matrices have no sum across ranks",
                                        "IGXEigenSolve: the eigen solve runs where its actions and its preconditioner run, and ",
                                        "IGXEigenSolve: the eigen solve takes its actions and its preconditioner from the matrix-free drivers, and "};
// 0: C [q][m] and theta [m] are the m lowest pairs of the leading q x q blocks of (GA, GB), both [.][ld]; 1: GB is not positive definite
// (or its diagonal not positive and finite); 2: an entry is not finite
static int eig_rayleigh_ritz(int q, int m, int ld, const std::vector<double> &GA, const std::vector<double> &GB, std::vector<double> &C, std::vector<double> &theta) {
  std::vector<double> A((size_t)q * q), B((size_t)q * q), d(q);
  for (int i = 0; i < q; ++i) for (int j = 0; j < q; ++j) if (!std::isfinite(GA[(size_t)i * ld + j]) || !std::isfinite(GB[(size_t)i * ld + j])) return 2;
  for (int i = 0; i < q; ++i) { const double b = GB[(size_t)i * ld + i]; if (!(b > 0.0)) return 1; d[i] = 1.0 / std::sqrt(b); }
  for (int i = 0; i < q; ++i) for (int j = 0; j < q; ++j) {
    A[(size_t)i * q + j] = 0.5 * (GA[(size_t)i * ld + j] + GA[(size_t)j * ld + i]) * d[i] * d[j];
    B[(size_t)i * q + j] = 0.5 * (GB[(size_t)i * ld + j] + GB[(size_t)j * ld + i]) * d[i] * d[j];
  }
  FastDiagEig E; std::string err;
  if (generalised_eigen(q, B, A, E, err)) return 1;
  C.assign((size_t)q * m, 0.0); theta.assign(m, 0.0);
  for (int j = 0; j < m; ++j) { theta[j] = E.lambda[j]; for (int i = 0; i < q; ++i) C[(size_t)i * m + j] = d[i] * E.U[(size_t)i + (size_t)q * j]; }
  return 0;
}
// the specification's ranges and nx == block, under the caller's name
static int eig_spec_refusal(const SolverWords &w, const IGXEigenSpec *sp, int nx) {
  auto range = [&](const char *what) { return fail(IGX_ERR_ARG_OUTOFRANGE, std::string(w.call) + ": the eigen solve's specification: " + what); };
  if (sp->nev < 1) return range("nev must be 1 at the least");
  if (sp->block < sp->nev || sp->block > BV_EIG_MAX) return range("block must be in range [nev,16]");
  if (sp->pc < IGX_PC_NONE || sp->pc > IGX_PC_FASTDIAG) return range("unknown preconditioner");
  if (!(sp->rtol >= 0) || !(sp->atol >= 0)) return range("the tolerances must not be negative");
  if (sp->maxit < 0) return range("maxit must not be negative");
  if (nx != sp->block) return fail(IGX_ERR_ARG_WRONG, std::string(w.call) + ": the eigen solve takes a start block of spec->block vectors, got " + std::to_string(nx));
  return 0;
}
// the IGX of B on the space of the IGX of A (fa: A's Dirichlet faces per field): dim, dof, then per axis degree, knots, periodicity, then the
// faces, then the stream; lead opens the refusal
static int eig_same_space(const char *lead, IGX ga, IGX gb, const bool fa[3][2][MAXFD]) {
  const Space &a = ga->s, &b = gb->s;
  auto differs = [&](const std::string &what) { return fail(IGX_ERR_ARG_WRONG, lead + what + " differs"); };
  if (a.dim != b.dim) return differs("dim");
  if (a.dof != b.dof) return differs("dof");
  for (int d = 0; d < a.dim; ++d) {
    if (a.axis[d].p != b.axis[d].p) return differs("the degree of axis " + std::to_string(d));
    if (a.axis[d].U != b.axis[d].U) return differs("the knot vector of axis " + std::to_string(d));
    if (a.axis[d].periodic != b.axis[d].periodic) return differs("the periodicity of axis " + std::to_string(d));
  }
  bool fb[3][2][MAXFD];
  fast_diag_fixed_faces(b, fb);
  if (memcmp(fa, fb, sizeof(fb)) != 0) return differs("the set of Dirichlet faces per field");
  if (ga->stream != gb->stream) return differs("the stream (IGXSetStream)");
  return 0;
}
// the eigen solve's work vectors on g for a block of m, in blocks of m: X' ; AX AX' ; W AW ; P P' AP AP' ; with a preconditioner R ; with a
// mass BX BX' BW BP BP'.  Kept between calls, replaced when a figure differs (IGXEigenSolve and IGXMatEigenSolve share the store).
typedef std::vector<IGXVec> EigBlock;
static int eig_state(IGX g, int m, int pc, int dof, long long n, bool has_mass) {
  const int nblocks = 9 + (pc != IGX_PC_NONE ? 1 : 0) + (has_mass ? 5 : 0);
  if (!g->eigen || g->eigen->m != m || g->eigen->pc != pc || g->eigen->dof != dof || g->eigen->n != n || g->eigen->nblocks != nblocks) {
    g->eigen.reset();
    std::shared_ptr<EigenState> es(new EigenState());
    if (int rc = es->ensure(g, n, nblocks * m, "device allocation of the eigen solve's work vectors failed")) return rc;
    if (int rc = add_vecs(g, n, pc == IGX_PC_JACOBI ? 1 : pc == IGX_PC_PBJACOBI ? dof : 0, es->pcv, "device allocation of the eigen solve's preconditioner failed")) return rc;
    es->m = m; es->pc = pc; es->dof = dof; es->nblocks = nblocks;
    g->eigen = es;
  }
  return 0;
}
// The loop the header states for IGXEigenSolve, line by line, on whatever applies the operators: IGXEigenSolve (the matrix-free actions) and
// IGXMatEigenSolve (the stored matrices) call it, as krylov_loop serves the Krylov solves.  The caller has checked its arguments, made the
// state (eig_state, bv_state) and begun the clock; it names the solve and finishes the clock afterwards.
//   act_block(in, aout, bout)   aout_j = A in_j and, with a mass, bout_j = B in_j for the block; it counts its launches on the clock
//   prepare()                   what T needs before its first use (the diagonal, the inverted point blocks): after the start block's fixed
//                               rows are zeroed and before the first action, the order the launches have always had
//   T(in, out)                  out = T in for one column; never called with pc none
//   faces                       the Dirichlet faces per field whose rows of the start block are zeroed (fast_diag_fixed_faces)
template <class FA, class FP, class FT>
static int eigen_loop(IGX g, EigenState &st, LoopClock &clk, const SolverWords &words, const IGXEigenSpec *sp, bool has_mass, const bool faces[3][2][MAXFD],
                      FA &&act_block, FP &&prepare, FT &&T, IGXVec X[], double lambda[], double resid[], IGXEigenInfo *info, double *history, const int &actions) {
  typedef EigBlock Block;
  const int m = sp->block, pc = sp->pc, dof = g->s.dof;
  const long long n = (long long)st.n;
  BlockVecState &bv = *g->blockvec;
  int next_block = 0;
  auto block = [&]() { Block b(m); for (int j = 0; j < m; ++j) b[j] = st.work[(size_t)next_block * m + j].get(); ++next_block; return b; };
  Block Xb[2] = {Block(X, X + m), block()}, AX[2] = {block(), block()}, W = block(), AW = block(), P[2] = {block(), block()}, AP[2] = {block(), block()};
  Block R = pc != IGX_PC_NONE ? block() : W;
  Block BX[2] = {Xb[0], Xb[1]}, BW = W, BP[2] = {P[0], P[1]};
  if (has_mass) { BX[0] = block(); BX[1] = block(); BW = block(); BP[0] = block(); BP[1] = block(); }
  g->slab_valid = 0;
  auto mdot = [&](Block &S, Block &T_, std::vector<double> &G) -> int { clk.own(2); return bv_mdot_run(g, (int)S.size(), S.data(), (int)T_.size(), T_.data(), G.data()); };
  auto maxpy = [&](Block &Y, Block &S, const double *C) -> int { clk.own(1); return bv_maxpy_run(g, (int)Y.size(), Y.data(), (int)S.size(), S.data(), C, 0.0); };
  auto join = [](std::initializer_list<const Block *> parts) { Block b; for (const Block *p : parts) b.insert(b.end(), p->begin(), p->end()); return b; };
  // the fixed rows of the start block
  {
    MgFaces F; memset(&F, 0, sizeof(F));
    long long nodes = 1, face_nodes = 0;
    F.dof = dof;
    for (int d = 0; d < 3; ++d) { F.n[d] = d < g->s.dim ? g->s.lay[d].nrow : 1; nodes *= F.n[d]; }
    for (int d = 0; d < g->s.dim; ++d) for (int sd = 0; sd < 2; ++sd) {
      unsigned mask = 0;
      for (int f = 0; f < dof; ++f) if (faces[d][sd][f]) mask |= 1u << f;
      if (!mask) continue;
      F.axis[F.nface] = d; F.at[F.nface] = sd ? F.n[d] - 1 : 0; F.mask[F.nface] = mask; ++F.nface;
      face_nodes = std::max(face_nodes, nodes / F.n[d]);
    }
    if (nodes * dof != n) return fail(IGX_ERR_PLIB, std::string(words.call) + ": the eigen solve's vectors and the row box differ");
    if (F.nface) for (int j = 0; j < m; ++j) {
      hipLaunchKernelGGL(mg_zero_fixed, dim3((unsigned)std::min<long long>(256, (face_nodes + MG_FACE_T - 1) / MG_FACE_T), (unsigned)F.nface), dim3(MG_FACE_T), 0, g->stream, X[j]->a.as<double>(), F);
      if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "mg_zero_fixed: kernel launch failed");
      clk.own(1);
    }
  }
  if (int rc = prepare()) return rc;
  int c = 0, its = 0, reason = 0, restarts = 0, nconv = 0;
  bool haveP = false;
  std::vector<double> GA((size_t)9 * m * m), GB((size_t)9 * m * m), C, theta(m, 0.0), rec((size_t)2 * m, 0.0), rn(m, 0.0);
  std::vector<double> CX((size_t)2 * m * m);
  // 0. Rayleigh-Ritz on the start block
  if (int rc = act_block(Xb[0], AX[0], BX[0])) return rc;
  if (int rc = mdot(Xb[0], AX[0], GA)) return rc;
  if (int rc = mdot(Xb[0], BX[0], GB)) return rc;
  if (const int bad = eig_rayleigh_ritz(m, m, m, GA, GB, C, theta)) reason = bad == 2 ? IGX_EIGEN_DIVERGED_NAN : IGX_EIGEN_DIVERGED_BREAKDOWN;
  else {
    if (int rc = maxpy(Xb[1], Xb[0], C.data())) return rc;
    if (int rc = maxpy(AX[1], AX[0], C.data())) return rc;
    if (has_mass) if (int rc = maxpy(BX[1], BX[0], C.data())) return rc;
    c = 1;
  }
  while (!reason) {
    // 1. the residuals of the block and the norms, one record
    BvEigCols rc_, ac_, bc_; BvTheta th;
    memset(&rc_, 0, sizeof(rc_)); memset(&ac_, 0, sizeof(ac_)); memset(&bc_, 0, sizeof(bc_)); memset(&th, 0, sizeof(th));
    for (int j = 0; j < m; ++j) { rc_.p[j] = R[j]->a.as<double>(); ac_.p[j] = AX[c][j]->a.as<double>(); bc_.p[j] = BX[c][j]->a.as<double>(); th.v[j] = theta[j]; }
    KR_LAUNCH(bv_resid, KR_G, KR_T, g, rc_, ac_, bc_, th, m, n, bv.rslab.as<double>());
    KR_LAUNCH(bv_record, 1, 64, g, bv.rslab.as<double>(), 2 * m, bv.rrec.as<double>());
    clk.own(2);
    HIPCK(hipMemcpyAsync(rec.data(), bv.rrec.p, (size_t)2 * m * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIPCK(hipStreamSynchronize(g->stream));
    // 2. the stop test
    bool nan = false;
    nconv = 0;
    for (int j = 0; j < m; ++j) {
      rn[j] = std::sqrt(rec[2 * j]);
      if (history) history[(size_t)its * m + j] = rn[j];
      if (std::isnan(rn[j])) nan = true;
      if (j < sp->nev && rn[j] <= std::max(sp->rtol * std::sqrt(rec[2 * j + 1]), sp->atol)) ++nconv;
    }
    if (nan) { reason = IGX_EIGEN_DIVERGED_NAN; break; }
    if (nconv == sp->nev) { reason = IGX_EIGEN_CONVERGED; break; }
    if (its >= sp->maxit) { reason = IGX_EIGEN_DIVERGED_ITS; break; }
    // 3. W = T R (no preconditioner: R is W)
    if (pc != IGX_PC_NONE) for (int j = 0; j < m; ++j) if (int rc = T(R[j], W[j])) return rc;
    // 4. the actions on W
    if (int rc = act_block(W, AW, BW)) return rc;
    // 5. the two Gram matrices of S = [X W P]
    Block S = haveP ? join({&Xb[c], &W, &P[c]}) : join({&Xb[c], &W});
    Block AS = haveP ? join({&AX[c], &AW, &AP[c]}) : join({&AX[c], &AW});
    Block BS = haveP ? join({&BX[c], &BW, &BP[c]}) : join({&BX[c], &BW});
    int q = (int)S.size();
    if (int rc = mdot(S, AS, GA)) return rc;
    if (int rc = mdot(S, BS, GB)) return rc;
    // 6. Rayleigh-Ritz; without a positive definite G_B: once more without P
    const int ld = q;
    int bad = eig_rayleigh_ritz(q, m, ld, GA, GB, C, theta);
    if (bad == 1 && haveP) { haveP = false; ++restarts; q = 2 * m; bad = eig_rayleigh_ritz(q, m, ld, GA, GB, C, theta); }
    if (bad) { reason = bad == 2 ? IGX_EIGEN_DIVERGED_NAN : IGX_EIGEN_DIVERGED_BREAKDOWN; break; }
    // 7. P' = [W P] C_WP, X' = X C_X + P', and the same for A. and B.
    for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) { CX[(size_t)i * m + j] = C[(size_t)i * m + j]; CX[(size_t)(m + i) * m + j] = i == j ? 1.0 : 0.0; }
    const double *CWP = C.data() + (size_t)m * m;
    Block WP = haveP ? join({&W, &P[c]}) : W, AWP = haveP ? join({&AW, &AP[c]}) : AW, BWP = haveP ? join({&BW, &BP[c]}) : BW;
    Block XP = join({&Xb[c], &P[1 - c]}), AXP = join({&AX[c], &AP[1 - c]}), BXP = join({&BX[c], &BP[1 - c]});
    if (int rc = maxpy(P[1 - c], WP, CWP)) return rc;
    if (int rc = maxpy(Xb[1 - c], XP, CX.data())) return rc;
    if (int rc = maxpy(AP[1 - c], AWP, CWP)) return rc;
    if (int rc = maxpy(AX[1 - c], AXP, CX.data())) return rc;
    if (has_mass) {
      if (int rc = maxpy(BP[1 - c], BWP, CWP)) return rc;
      if (int rc = maxpy(BX[1 - c], BXP, CX.data())) return rc;
    }
    c = 1 - c; haveP = true; ++its;
  }
  // the caller's block receives the last iterate
  if (c == 1) for (int j = 0; j < m; ++j) HIPCK(hipMemcpyAsync(X[j]->a.p, Xb[1][j]->a.p, X[j]->a.bytes, hipMemcpyDeviceToDevice, g->stream));
  HIPCK(hipStreamSynchronize(g->stream));
  for (int j = 0; j < m; ++j) { lambda[j] = theta[j]; if (resid) resid[j] = rn[j]; }
  info->iterations = its; info->reason = reason; info->nconverged = nconv; info->restarts = restarts; info->actions = actions;
  return 0;
}
extern "C" int IGXEigenSolve(IGX g, IGX mass, const IGXEigenSpec *sp, int nx, IGXVec X[], double lambda[], double resid[], IGXEigenInfo *info, double *history) {
  const SolverWords &words = kEigenWords;
  if (!g || !sp || !X || !lambda || !info) return fail(IGX_ERR_ARG_WRONG, "IGXEigenSolve: null pointer: the eigen solve takes the stiffness IGX, a specification, the block X, lambda and info");
  if (int rc = eig_spec_refusal(words, sp, nx)) return rc;
  if (!g->s.setup) return fail(IGX_ERR_ORDER, "Must call IGXSetUp() on the stiffness IGX before IGXEigenSolve(): the eigen solve needs a set-up space");
  if (mass && !mass->s.setup) return fail(IGX_ERR_ORDER, "Must call IGXSetUp() on the mass IGX before IGXEigenSolve(): the eigen solve needs a set-up space");
  if (g->s.form == IGX_FORM_NONE) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetForm...() on the stiffness IGX first: the eigen solve has no operator A");
  if (mass && mass->s.form == IGX_FORM_NONE) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetForm...() on the mass IGX first: the eigen solve has no operator B");
  bool faces[3][2][MAXFD];
  fast_diag_fixed_faces(g->s, faces);
  if (mass) if (int rc = eig_same_space("IGXEigenSolve: the eigen solve needs the mass IGX on the space of the stiffness IGX: ", g, mass, faces)) return rc;
  for (IGX h : {g, mass}) if (h) for (int d = 0; d < h->s.dim; ++d) if (h->s.proc_sizes[d] != 1) return fail(IGX_ERR_SUP, words.one_rank);
  for (IGX h : {g, mass}) if (h && h->fixtable.p) return fail(IGX_ERR_SUP, "IGXEigenSolve: the eigen solve does not cover a fix table (IGXSetFixTable): its fixed rows are not a union of faces");
  const int m = sp->block, pc = sp->pc;
  for (int j = 0; j < m; ++j) {
    if (!X[j]) return fail(IGX_ERR_ARG_WRONG, "IGXEigenSolve: the eigen solve's start block holds a null vector");
    if (X[j]->iga != g) return fail(IGX_ERR_ARG_WRONG, "IGXEigenSolve: the eigen solve's start block holds a vector created by another IGX than the stiffness IGX");
    for (int k = 0; k < j; ++k) if (X[k] == X[j]) return fail(IGX_ERR_ARG_WRONG, "IGXEigenSolve: the eigen solve's start block holds a vector twice");
  }
  if (pc == IGX_PC_FASTDIAG && !g->fd) return fail(IGX_ERR_ORDER, "Must call IGXFastDiagSetUp() on the stiffness IGX before IGXEigenSolve() with IGX_PC_FASTDIAG");
  for (IGX h : {g, mass}) if (h) if (int rc = solver_runs_here(h, words)) return rc;
  if (int rc = ensure_device(g)) return rc;
  if (mass) if (int rc = ensure_device(mass)) return rc;
  const long long n = (long long)g->nbrows * g->s.dof;
  for (int j = 0; j < m; ++j) if (X[j]->n != n) return fail(IGX_ERR_ARG_WRONG, "IGXEigenSolve: vector of another size than the space's");
  if (mass && (long long)mass->nbrows * mass->s.dof != n) return fail(IGX_ERR_PLIB, "IGXEigenSolve: the row boxes of the two IGX differ");
  if (int rc = bv_state(g)) return rc;
  const int dof = g->s.dof;
  if (int rc = eig_state(g, m, pc, dof, n, mass != nullptr)) return rc;
  EigenState &st = *g->eigen;
  typedef EigBlock Block;
  LoopClock clk(g, st);
  if (int rc = clk.begin(g)) return rc;
  std::string opname;
  int actions = 0;
  auto actA = [&](IGXVec in, IGXVec out) -> int {
    if (int rc = compute_matfree(g, VsMode::ACTION, IGX_OP_MATRIX, nullptr, nullptr, 1, &in, 1, &out, 0.0, 0.0)) return solver_refused(words, rc);
    if (opname.empty()) opname = g->last_kernel;
    ++actions;
    return clk.driver(g);
  };
  auto actB = [&](IGXVec in, IGXVec out) -> int {      // the mass IGX's figures: its own launches and, where it is timed too, its own events
    if (int rc = compute_matfree(mass, VsMode::ACTION, IGX_OP_MATRIX, nullptr, nullptr, 1, &in, 1, &out, 0.0, 0.0)) return solver_refused(words, rc);
    ++actions;
    clk.launches += mass->last_launches;
    if (clk.timing && mass->timing) { float ms = 0; HIPCK(hipEventSynchronize(mass->ev[2])); HIPCK(hipEventElapsedTime(&ms, mass->ev[1], mass->ev[2])); clk.op_ms += ms; }
    return 0;
  };
  // IGXSetBatchedActions(stiff, 1): one call of the action on a block per operator (compute_matfree, ACTION_BATCH) in place of m single actions;
  // the figures are taken as above, the block call's in place of the m calls'
  static_assert(BV_EIG_MAX <= IGX_ACTION_MAXCOLS && ACTION_BLOCK_MAX == BV_MAX, "the eigen solve's block is one chunk of the block action; a block call takes a block vector");
  auto act_block = [&](const Block &in, const Block &aout, const Block &bout) -> int {
    if (g->batched_actions) {
      if (int rc = compute_matfree(g, VsMode::ACTION_BATCH, IGX_OP_MATRIX, nullptr, nullptr, m, const_cast<IGXVec *>(in.data()), m, const_cast<IGXVec *>(aout.data()), 0.0, 0.0)) return solver_refused(words, rc);
      if (opname.empty()) opname = g->last_kernel;
      actions += m;
      if (int rc = clk.driver(g)) return rc;
      if (!mass) return 0;
      if (int rc = compute_matfree(mass, VsMode::ACTION_BATCH, IGX_OP_MATRIX, nullptr, nullptr, m, const_cast<IGXVec *>(in.data()), m, const_cast<IGXVec *>(bout.data()), 0.0, 0.0)) return solver_refused(words, rc);
      actions += m;
      clk.launches += mass->last_launches;
      if (clk.timing && mass->timing) { float ms = 0; HIPCK(hipEventSynchronize(mass->ev[2])); HIPCK(hipEventElapsedTime(&ms, mass->ev[1], mass->ev[2])); clk.op_ms += ms; }
      return 0;
    }
    for (int j = 0; j < m; ++j) if (int rc = actA(in[j], aout[j])) return rc;
    if (mass) for (int j = 0; j < m; ++j) if (int rc = actB(in[j], bout[j])) return rc;
    return 0;
  };
  // the preconditioner T of stiff: its diagonal, or its inverted point blocks
  std::vector<IGXVec> cols; for (auto &v : st.pcv) cols.push_back(v.get());
  auto prepare = [&]() -> int {
    if (pc == IGX_PC_JACOBI || pc == IGX_PC_PBJACOBI) {
      if (int rc = compute_matfree(g, pc == IGX_PC_JACOBI ? VsMode::DIAGONAL : VsMode::BLOCK_DIAGONAL, IGX_OP_MATRIX, nullptr, nullptr, 0, nullptr, (int)cols.size(), cols.data(), 0.0, 0.0)) return solver_refused(words, rc);
      if (int rc = clk.driver(g)) return rc;
    }
    if (pc == IGX_PC_PBJACOBI) {
      if (int rc = block_diagonal_run(g, dof, cols.data(), nullptr, nullptr, nullptr, true)) return solver_refused(words, rc);
      if (int rc = clk.driver(g)) return rc;
    }
    return 0;
  };
  auto T = [&](IGXVec in, IGXVec out) -> int {
    if (pc == IGX_PC_JACOBI) { KR_LAUNCH(kr_pdiv, kr_grid(n), KR_T, g, out->a.as<double>(), in->a.as<double>(), cols[0]->a.as<double>(), n); clk.own(1); return 0; }
    if (int rc = pc == IGX_PC_PBJACOBI ? block_diagonal_run(g, dof, cols.data(), in, out, nullptr, false) : IGXFastDiagApply(g, in, out)) return solver_refused(words, rc);
    return clk.driver(g);
  };
  if (int rc = eigen_loop(g, st, clk, words, sp, mass != nullptr, faces, act_block, prepare, T, X, lambda, resid, info, history, actions)) return rc;
  static const char *const pcs[4] = {"none", "jacobi", "pbjacobi", "fastdiag"};
  return clk.finish(g, "eigen(lobpcg, block " + std::to_string(m) + ", pc=" + pcs[pc] + ", " + opname + ", " + std::to_string(info->iterations) + " iterations)");
}
