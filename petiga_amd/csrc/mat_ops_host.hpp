// mat_ops_host.hpp -- the host side of the stored matrix as an operator (kernels: mat_ops.hpp, included here).  Host code only.
// IGXMatMult, IGXMatGetDiagonal, IGXMatGetBlockDiagonal and IGXMatSolve: what a caller without PETSc does with an assembled IGXMat; and the
// product on a block of vectors with the eigen solve on it, IGXMatMultBlock and IGXMatEigenSolve.  Included
// last by the main unit (engine.hip): its kernels are the last of the unit.  One rank on every axis; the refusals are decided in
// include/petiga_amd.h's order before the first HIP call.
#pragma once
#include "mat_ops.hpp"
#include "mat_block_launch.hpp"      // (the block product's launcher: apart, so that mat_ops.hpp alone instantiates none of its kernels)
// 2. the vectors are the matrix's IGX's, and the matrix and the vectors have the sizes of its present space
static int mat_current(const char *fn, IGXMat A, int nv, const IGXVec *v) {
  IGX g = A->iga; const Space &s = g->s;
  for (int k = 0; k < nv; ++k) if (v[k]->iga != g) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": vector created by another IGX than the matrix's");
  int64_t rows = 1, blocks = 1;
  if (s.setup) for (int d = 0; d < 3; ++d) { int64_t t = 0; for (int r = 0; r < s.lay[d].nrow; ++r) t += s.lay[d].rcnt[r]; rows *= s.lay[d].nrow; blocks *= t; }
  // (the set-up's count as well as the sizes: a set-up that keeps the three counts may still move the pattern, and the kernels walk the
  // matrix's browptr with the IGX's present axis tables)
  if (!g->current(A->gen) || A->bs != s.dof || A->nbrows != rows || A->nblocks != blocks)
    return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": the matrix was made before the last IGXSetUp() of its IGX (its pattern and size are that set-up's): create it again");
  for (int k = 0; k < nv; ++k) if (v[k]->n != rows * s.dof)
    return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": vector of another size than its IGX's space (made before the last IGXSetUp()): create it again");
  return 0;
}
// 4. one rank on every axis; with it, a column node index is a row index of x: checked here, not assumed
static int mat_one_rank(const char *fn, IGX g) {
  const Space &s = g->s;
  for (int d = 0; d < s.dim; ++d) if (s.proc_sizes[d] != 1)
    return fail(IGX_ERR_SUP, std::string(fn) + ": the stored matrix as an operator needs one rank on every axis: its columns are then the rows of x, and there is no ghost refresh in the product");
  for (int d = 0; d < 3; ++d) if (s.lay[d].nrow != s.lay[d].ncol || s.lay[d].rownode != s.lay[d].colnode)
    return fail(IGX_ERR_PLIB, std::string(fn) + ": the column box of an axis is not its row box");
  return 0;
}
static MatPat make_matpat(IGX g) {
  MatPat P;
  for (int d = 0; d < 3; ++d) {
    P.nrow[d] = g->s.lay[d].nrow; P.ncol[d] = g->s.lay[d].ncol; P.W[d] = 2 * g->s.lay[d].p + 1;
    P.rcnt[d] = g->ab[d].rcnt.as<int>(); P.rcol[d] = g->ab[d].rcol.as<int>();
  }
  return P;
}
// the lanes per row and the index variant of a product with A: the single product and the block product take the same
static void mat_mult_shape(IGXMat A, int *lanes_out, bool *tables_out) {
  IGX g = A->iga;
  long long longest = (long long)A->bs * A->bs;
  for (int d = 0; d < 3; ++d) longest *= *std::max_element(g->s.lay[d].rcnt.begin(), g->s.lay[d].rcnt.end());
  const int lanes = mat_mult_lanes(longest);
  // unset: the faster one as measured (profiles/matmult.txt) -- the tables where rows are short enough for sub-groups (dof 1 at p <= 2: by 1 to
  // 8 %), bcolidx where a wavefront takes a row (p = 3: by 1 to 5 %; bs = 3: level)
  bool tables = g->s.env.matmult_index < 0 ? lanes < 64 : g->s.env.matmult_index == 0;
  for (int d = 0; d < 3; ++d) if (2 * g->s.lay[d].p + 1 > MM_MAXW) tables = false;      // beyond the range mm_div is exact in (no degree the library takes today: p <= 7)
  *lanes_out = lanes; *tables_out = tables;
}
static std::string mat_mult_words(int lanes, bool tables) {
  return std::string(lanes == 64 ? "one wavefront per row" : (std::to_string(lanes) + " lanes per row").c_str()) + ", columns from " + (tables ? "the axis tables" : "bcolidx");
}
// y = A x, the arguments checked: one launch on the engine's stream
static int mat_mult_run(IGXMat A, IGXVec x, IGXVec y) {
  IGX g = A->iga;
  if (int rc = ensure_device(g)) return rc;
  int lanes; bool tables;
  mat_mult_shape(A, &lanes, &tables);
  if (g->timing) { HIPCK(hipEventRecord(g->ev[0], g->stream)); HIPCK(hipEventRecord(g->ev[1], g->stream)); }
  g->slab_valid = 0;
  if (!mat_mult_launch(A->bs, lanes, tables, make_matpat(g), (long long)A->nbrows, A->browptr.as<int64_t>(), A->bcolidx.as<int32_t>(), A->val.as<double>(), x->a.as<double>(), y->a.as<double>(), g->stream))
    return fail(IGX_ERR_SUP, "IGXMatMult: the block size must be 1 to 8");
  if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "mat_mult: kernel launch failed");
  if (g->timing) { HIPCK(hipEventRecord(g->ev[2], g->stream)); HIPCK(hipEventRecord(g->ev[3], g->stream)); }
  g->last_launches = 1;
  g->last_kernel = "mat_mult(bs=" + std::to_string(A->bs) + ", " + mat_mult_words(lanes, tables) + ")";
  return 0;
}
// Y[j] = A X[j] for j < nx, the arguments checked (the block size among them: 1 to MAXBC): mat_block_plan's launches on the engine's stream,
// mat_mult_block for a chunk of 2, 4 or 8 columns and mat_mult for a last single one
static int mat_mult_block_run(IGXMat A, int nx, IGXVec *X, IGXVec *Y) {
  IGX g = A->iga;
  if (int rc = ensure_device(g)) return rc;
  int lanes; bool tables;
  mat_mult_shape(A, &lanes, &tables);
  int widths[ACTION_BLOCK_MAX];
  const int nchunks = mat_block_plan(A->bs, nx, widths);
  const double *x[ACTION_BLOCK_MAX]; double *y[ACTION_BLOCK_MAX];
  for (int j = 0; j < nx; ++j) { x[j] = X[j]->a.as<double>(); y[j] = Y[j]->a.as<double>(); }
  if (g->timing) { HIPCK(hipEventRecord(g->ev[0], g->stream)); HIPCK(hipEventRecord(g->ev[1], g->stream)); }
  g->slab_valid = 0;
  const MatPat P = make_matpat(g);
  for (int k = 0, j = 0; k < nchunks; j += widths[k], ++k) {
    const bool ok = widths[k] == 1
      ? mat_mult_launch(A->bs, lanes, tables, P, (long long)A->nbrows, A->browptr.as<int64_t>(), A->bcolidx.as<int32_t>(), A->val.as<double>(), x[j], y[j], g->stream)
      : mat_mult_block_launch(A->bs, widths[k], lanes, tables, P, (long long)A->nbrows, A->browptr.as<int64_t>(), A->bcolidx.as<int32_t>(), A->val.as<double>(), x + j, y + j, g->stream);
    if (!ok) return fail(IGX_ERR_PLIB, "IGXMatMultBlock: the chunk plan names a launch the library does not hold");
    if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "mat_mult_block: kernel launch failed");
  }
  if (g->timing) { HIPCK(hipEventRecord(g->ev[2], g->stream)); HIPCK(hipEventRecord(g->ev[3], g->stream)); }
  g->last_launches = nchunks;
  g->last_kernel = "mat_mult_block(bs=" + std::to_string(A->bs) + ", " + mat_mult_words(lanes, tables) + ", NC=" + std::to_string(mat_block_nc(A->bs)) + ")";
  return 0;
}
// the diagonal (nb = 0: into B[0]) or the nb = bs block columns, the arguments checked: one launch
static int mat_diag_run(IGXMat A, int nb, IGXVec *B) {
  IGX g = A->iga;
  if (int rc = ensure_device(g)) return rc;
  MatCols cols; memset(&cols, 0, sizeof(cols));
  for (int j = 0; j < std::max(nb, 1); ++j) cols.col[j] = B[j]->a.as<double>();
  if (g->timing) { HIPCK(hipEventRecord(g->ev[0], g->stream)); HIPCK(hipEventRecord(g->ev[1], g->stream)); }
  g->slab_valid = 0;
  mat_get_diag_launch(nb > 0, make_matpat(g), (long long)A->nbrows, A->bs, A->browptr.as<int64_t>(), A->val.as<double>(), cols, g->stream);
  if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "mat_get_diag: kernel launch failed");
  if (g->timing) { HIPCK(hipEventRecord(g->ev[2], g->stream)); HIPCK(hipEventRecord(g->ev[3], g->stream)); }
  g->last_launches = 1;
  g->last_kernel = nb > 0 ? "mat_get_block_diagonal(one thread per scalar, the block's place from the axis tables)" : "mat_get_diagonal(one thread per scalar, the block's place from the axis tables)";
  return 0;
}
extern "C" int IGXMatMult(IGXMat A, IGXVec x, IGXVec y) {
  if (!A || !x || !y) return fail(IGX_ERR_ARG_WRONG, "IGXMatMult: null matrix or vector");
  const IGXVec v[2] = {x, y};
  if (int rc = mat_current("IGXMatMult", A, 2, v)) return rc;
  if (x == y) return fail(IGX_ERR_ARG_WRONG, "IGXMatMult: x and y must be different vectors");
  if (int rc = mat_one_rank("IGXMatMult", A->iga)) return rc;
  return mat_mult_run(A, x, y);
}
// the refusals of the block product in the header's order, under the caller's name
static int mat_block_args(const char *fn, IGXMat A, int nx, IGXVec X[], IGXVec Y[]) {
  const std::string f(fn);
  if (!A || !X || !Y) return fail(IGX_ERR_ARG_WRONG, f + ": null matrix or array of vectors");
  if (nx < 1 || nx > ACTION_BLOCK_MAX) return fail(IGX_ERR_ARG_OUTOFRANGE, f + ": the product on a block takes 1 to " + std::to_string(ACTION_BLOCK_MAX) + " columns, got " + std::to_string(nx));
  for (int j = 0; j < nx; ++j) if (!X[j] || !Y[j]) return fail(IGX_ERR_ARG_WRONG, f + ": null vector in the block");
  std::vector<IGXVec> v(X, X + nx); v.insert(v.end(), Y, Y + nx);
  if (int rc = mat_current(fn, A, 2 * nx, v.data())) return rc;
  for (int j = 0; j < nx; ++j) for (int k = 0; k < j; ++k) if (Y[k] == Y[j]) return fail(IGX_ERR_ARG_WRONG, f + ": the same vector given for two results of the block");
  for (int j = 0; j < nx; ++j) for (int i = 0; i < nx; ++i) if (X[i] == Y[j]) return fail(IGX_ERR_ARG_WRONG, f + ": a vector of X and a result of the block must be different vectors");
  if (int rc = mat_one_rank(fn, A->iga)) return rc;
  if (A->bs < 1 || A->bs > MAXBC) return fail(IGX_ERR_SUP, f + ": the block size must be 1 to 8");
  return 0;
}
extern "C" int IGXMatMultBlock(IGXMat A, int nx, IGXVec X[], IGXVec Y[]) {
  if (int rc = mat_block_args("IGXMatMultBlock", A, nx, X, Y)) return rc;
  return mat_mult_block_run(A, nx, X, Y);
}
extern "C" int IGXMatMultBlockPlan(int bs, int nx, int *nchunks, int widths[]) {
  if (!nchunks) return fail(IGX_ERR_ARG_WRONG, "IGXMatMultBlockPlan: null count");
  if (bs < 1 || bs > MAXBC || nx < 1 || nx > ACTION_BLOCK_MAX) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMatMultBlockPlan: the block size must be 1 to 8 and the block 1 to " + std::to_string(ACTION_BLOCK_MAX) + " columns");
  *nchunks = mat_block_plan(bs, nx, widths);
  return 0;
}
extern "C" int IGXMatGetDiagonal(IGXMat A, IGXVec d) {
  if (!A || !d) return fail(IGX_ERR_ARG_WRONG, "IGXMatGetDiagonal: null matrix or vector");
  if (int rc = mat_current("IGXMatGetDiagonal", A, 1, &d)) return rc;
  if (int rc = mat_one_rank("IGXMatGetDiagonal", A->iga)) return rc;
  return mat_diag_run(A, 0, &d);
}
extern "C" int IGXMatGetBlockDiagonal(IGXMat A, int nb, IGXVec B[]) {
  if (!A || !B) return fail(IGX_ERR_ARG_WRONG, "IGXMatGetBlockDiagonal: null matrix or array of block columns");
  if (nb != A->bs || nb < 1 || nb > MAXBC) return fail(IGX_ERR_ARG_WRONG, "IGXMatGetBlockDiagonal: the block diagonal has bs columns: nb must equal the matrix's block size");
  for (int j = 0; j < nb; ++j) if (!B[j]) return fail(IGX_ERR_ARG_WRONG, "IGXMatGetBlockDiagonal: null block column");
  if (int rc = mat_current("IGXMatGetBlockDiagonal", A, nb, B)) return rc;
  for (int j = 0; j < nb; ++j) for (int k = 0; k < j; ++k) if (B[k] == B[j]) return fail(IGX_ERR_ARG_WRONG, "IGXMatGetBlockDiagonal: the same vector given for two block columns");
  if (int rc = mat_one_rank("IGXMatGetBlockDiagonal", A->iga)) return rc;
  return mat_diag_run(A, nb, B);
}
// IGXSolve's loop (krylov_loop) with A(in, out) = the product above and the preconditioners read out of the matrix; the work vectors are
// IGXSolve's own store on the IGX, replaced under the same rule, so the two solves may follow each other in any order.
extern "C" int IGXMatSolve(IGXMat A, const IGXSolveSpec *sp, IGXVec b, IGXVec x, IGXSolveInfo *info, double *history) {
  if (!A || !sp || !b || !x) return fail(IGX_ERR_ARG_WRONG, "IGXMatSolve: null matrix, specification, right-hand side or solution vector");
  const IGXVec v[2] = {b, x};
  if (int rc = mat_current("IGXMatSolve", A, 2, v)) return rc;
  if (x == b) return fail(IGX_ERR_ARG_WRONG, "IGXMatSolve: the solution and the right-hand side must be different vectors");
  IGX g = A->iga;
  if (int rc = mat_one_rank("IGXMatSolve", g)) return rc;
  if (!(sp->rtol >= 0) || !(sp->atol >= 0)) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMatSolve: the tolerances must not be negative");
  if (sp->maxit < 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMatSolve: maxit must not be negative");
  if (sp->method != IGX_SOLVE_CG && sp->method != IGX_SOLVE_BICGSTAB) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMatSolve: unknown method");
  if (sp->pc < IGX_PC_NONE || sp->pc > IGX_PC_FASTDIAG) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXMatSolve: unknown preconditioner");
  static const SolverWords words = {"IGXMatSolve", "", "the Krylov solve on the stored matrix runs where its preconditioner runs, and ", nullptr};
  if (int rc = solver_pc_ready(g, words, sp->pc)) return rc;
  if (int rc = ensure_device(g)) return rc;
  if (int rc = kr_scalars(g)) return rc;
  const bool cg = sp->method == IGX_SOLVE_CG;
  const int dof = A->bs, pc = sp->pc;
  const long long n = (long long)b->n;
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
  auto Aop = [&](IGXVec in, IGXVec out) -> int {
    if (int rc = mat_mult_run(A, in, out)) return rc;
    if (opname.empty()) opname = g->last_kernel;
    return clk.driver(g);
  };
  std::vector<IGXVec> cols; for (auto &c : st.pcv) cols.push_back(c.get());
  if (pc == IGX_PC_JACOBI || pc == IGX_PC_PBJACOBI) {
    if (int rc = mat_diag_run(A, pc == IGX_PC_JACOBI ? 0 : dof, cols.data())) return rc;
    if (int rc = clk.driver(g)) return rc;
  }
  if (pc == IGX_PC_PBJACOBI) {
    if (int rc = block_diagonal_run(g, dof, cols.data(), nullptr, nullptr, nullptr, true)) return solver_refused(words, rc);
    if (int rc = clk.driver(g)) return rc;
  }
  auto M = [&](IGXVec in, IGXVec out) -> int {
    if (pc == IGX_PC_NONE) return 0;
    if (pc == IGX_PC_JACOBI) { KR_LAUNCH(kr_pdiv, kr_grid(n), KR_T, g, out->a.as<double>(), in->a.as<double>(), cols[0]->a.as<double>(), n); clk.own(1); return 0; }
    if (int rc = pc == IGX_PC_PBJACOBI ? block_diagonal_run(g, dof, cols.data(), in, out, nullptr, false) : IGXFastDiagApply(g, in, out)) return solver_refused(words, rc);
    return clk.driver(g);
  };
  const KrylovPlan kp = {sp->method, sp->rtol, sp->atol, sp->maxit, pc == IGX_PC_NONE, pc == IGX_PC_JACOBI ? cols[0]->a.as<double>() : nullptr};
  int its = 0;
  if (int rc = krylov_loop(g, st, clk, kp, Aop, M, b, x, info, &its, history)) return rc;
  static const char *const methods[2] = {"cg", "bicgstab"}, *const pcs[4] = {"none", "jacobi", "pbjacobi", "fastdiag"};
  return clk.finish(g, std::string("krylov(") + methods[sp->method] + ", pc=" + pcs[pc] + ", " + opname + ", " + std::to_string(its) + " iterations)");
}
// IGXEigenSolve's loop (eigen_loop) with A(block) and B(block) one block product each on the stored K and M, and the preconditioners read
// out of K as IGXMatSolve reads them.  The vectors and the work store are those of K's IGX; M may come from the same IGX or from another one
// on the same space (its product then runs on K's vectors with its own axis tables: the same layout).
static const SolverWords kMatEigenWords = {"IGXMatEigenSolve", "", "IGXMatEigenSolve: the eigen solve on the stored matrices runs where its preconditioner runs, and ",
                                           "IGXMatEigenSolve: the eigen solve on the stored matrices takes its preconditioner from the matrix and from fast diagonalisation, and "};
extern "C" int IGXMatEigenSolve(IGXMat K, IGXMat M, const IGXEigenSpec *sp, int nx, IGXVec X[], double lambda[], double resid[], IGXEigenInfo *info, double *history) {
  const SolverWords &words = kMatEigenWords;
  if (!K || !sp || !X || !lambda || !info) return fail(IGX_ERR_ARG_WRONG, "IGXMatEigenSolve: null pointer: the eigen solve takes the stiffness matrix, a specification, the block X, lambda and info");
  if (int rc = eig_spec_refusal(words, sp, nx)) return rc;
  const int m = sp->block, pc = sp->pc;
  for (int j = 0; j < m; ++j) if (!X[j]) return fail(IGX_ERR_ARG_WRONG, "IGXMatEigenSolve: the eigen solve's start block holds a null vector");
  if (int rc = mat_current("IGXMatEigenSolve", K, m, X)) return rc;
  for (int j = 0; j < m; ++j) for (int k = 0; k < j; ++k) if (X[k] == X[j]) return fail(IGX_ERR_ARG_WRONG, "IGXMatEigenSolve: the eigen solve's start block holds a vector twice");
  if (M) if (int rc = mat_current("IGXMatEigenSolve", M, 0, nullptr)) return rc;
  IGX g = K->iga, gm = M ? M->iga : nullptr;
  bool faces[3][2][MAXFD];
  fast_diag_fixed_faces(g->s, faces);
  if (M) {
    if (gm != g) if (int rc = eig_same_space("IGXMatEigenSolve: the eigen solve needs the mass matrix on the space of the stiffness matrix: ", g, gm, faces)) return rc;
    if (M->bs != K->bs || M->nbrows != K->nbrows || M->nblocks != K->nblocks) return fail(IGX_ERR_ARG_WRONG, "IGXMatEigenSolve: the eigen solve needs the mass matrix on the space of the stiffness matrix: the block size or the pattern differs");
  }
  if (int rc = mat_one_rank("IGXMatEigenSolve", g)) return rc;
  if (M && gm != g) if (int rc = mat_one_rank("IGXMatEigenSolve", gm)) return rc;
  for (IGX h : {g, gm}) if (h && h->fixtable.p) return fail(IGX_ERR_SUP, "IGXMatEigenSolve: the eigen solve does not cover a fix table (IGXSetFixTable): its fixed rows are not a union of faces");
  if (K->bs < 1 || K->bs > MAXBC) return fail(IGX_ERR_SUP, "IGXMatEigenSolve: the block size must be 1 to 8");
  if (pc == IGX_PC_FASTDIAG) {
    if (const char *why = fast_diag_refusal(g)) return fail(IGX_ERR_SUP, words.inner + std::string(why));
    if (!g->fd) return fail(IGX_ERR_ORDER, "Must call IGXFastDiagSetUp() on the stiffness matrix's IGX before IGXMatEigenSolve() with IGX_PC_FASTDIAG");
  }
  if (int rc = ensure_device(g)) return rc;
  if (gm && gm != g) if (int rc = ensure_device(gm)) return rc;
  const int dof = K->bs;
  const long long n = (long long)K->nbrows * dof;
  if (int rc = bv_state(g)) return rc;
  if (int rc = eig_state(g, m, pc, dof, n, M != nullptr)) return rc;
  EigenState &st = *g->eigen;
  LoopClock clk(g, st);
  if (int rc = clk.begin(g)) return rc;
  std::string opname;
  int actions = 0;
  auto act_block = [&](const EigBlock &in, const EigBlock &aout, const EigBlock &bout) -> int {
    if (int rc = mat_mult_block_run(K, m, const_cast<IGXVec *>(in.data()), const_cast<IGXVec *>(aout.data()))) return rc;
    if (opname.empty()) opname = g->last_kernel;
    actions += m;
    if (int rc = clk.driver(g)) return rc;
    if (!M) return 0;
    if (int rc = mat_mult_block_run(M, m, const_cast<IGXVec *>(in.data()), const_cast<IGXVec *>(bout.data()))) return rc;
    actions += m;
    if (gm == g) return clk.driver(g);
    clk.launches += gm->last_launches;      // the mass matrix's IGX's figures: its own launches and, where it is timed too, its own events
    if (clk.timing && gm->timing) { float ms = 0; HIPCK(hipEventSynchronize(gm->ev[2])); HIPCK(hipEventElapsedTime(&ms, gm->ev[1], gm->ev[2])); clk.op_ms += ms; }
    return 0;
  };
  // the preconditioner T out of K: its diagonal, or its inverted point blocks
  std::vector<IGXVec> cols; for (auto &v : st.pcv) cols.push_back(v.get());
  auto prepare = [&]() -> int {
    if (pc == IGX_PC_JACOBI || pc == IGX_PC_PBJACOBI) {
      if (int rc = mat_diag_run(K, pc == IGX_PC_JACOBI ? 0 : dof, cols.data())) return rc;
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
  if (int rc = eigen_loop(g, st, clk, words, sp, M != nullptr, faces, act_block, prepare, T, X, lambda, resid, info, history, actions)) return rc;
  static const char *const pcs[4] = {"none", "jacobi", "pbjacobi", "fastdiag"};
  return clk.finish(g, "eigen(lobpcg, block " + std::to_string(m) + ", pc=" + pcs[pc] + ", " + opname + ", " + std::to_string(info->iterations) + " iterations)");
}
