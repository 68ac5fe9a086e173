// mat_ops_host.hpp -- the host side of the stored matrix as an operator (kernels: mat_ops.hpp, included here).  Host code only.
// IGXMatMult, IGXMatGetDiagonal, IGXMatGetBlockDiagonal and IGXMatSolve: what a caller without PETSc does with an assembled IGXMat.  Included
// last by the main unit (engine.hip): its kernels are the last of the unit.  One rank on every axis; the refusals are decided in
// include/petiga_amd.h's order before the first HIP call.
#pragma once
#include "mat_ops.hpp"
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
// y = A x, the arguments checked: one launch on the engine's stream
static int mat_mult_run(IGXMat A, IGXVec x, IGXVec y) {
  IGX g = A->iga;
  if (int rc = ensure_device(g)) return rc;
  long long longest = (long long)A->bs * A->bs;
  for (int d = 0; d < 3; ++d) longest *= *std::max_element(g->s.lay[d].rcnt.begin(), g->s.lay[d].rcnt.end());
  const int lanes = mat_mult_lanes(longest);
  // unset: the faster one as measured (profiles/matmult.txt) -- the tables where rows are short enough for sub-groups (dof 1 at p <= 2: by 1 to
  // 8 %), bcolidx where a wavefront takes a row (p = 3: by 1 to 5 %; bs = 3: level)
  bool tables = g->s.env.matmult_index < 0 ? lanes < 64 : g->s.env.matmult_index == 0;
  for (int d = 0; d < 3; ++d) if (2 * g->s.lay[d].p + 1 > MM_MAXW) tables = false;      // beyond the range mm_div is exact in (no degree the library takes today: p <= 7)
  if (g->timing) { HIPCK(hipEventRecord(g->ev[0], g->stream)); HIPCK(hipEventRecord(g->ev[1], g->stream)); }
  g->slab_valid = 0;
  if (!mat_mult_launch(A->bs, lanes, tables, make_matpat(g), (long long)A->nbrows, A->browptr.as<int64_t>(), A->bcolidx.as<int32_t>(), A->val.as<double>(), x->a.as<double>(), y->a.as<double>(), g->stream))
    return fail(IGX_ERR_SUP, "IGXMatMult: the block size must be 1 to 8");
  if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "mat_mult: kernel launch failed");
  if (g->timing) { HIPCK(hipEventRecord(g->ev[2], g->stream)); HIPCK(hipEventRecord(g->ev[3], g->stream)); }
  g->last_launches = 1;
  char name[160];
  snprintf(name, sizeof(name), "mat_mult(bs=%d, %s, columns from %s)", A->bs, lanes == 64 ? "one wavefront per row" : (std::to_string(lanes) + " lanes per row").c_str(), tables ? "the axis tables" : "bcolidx");
  g->last_kernel = name;
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
