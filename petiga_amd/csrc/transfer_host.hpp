// transfer_host.hpp -- the host side of IGXTransfer (kernels: transfer.hpp, included here).  Host code only.  Included by the main unit
// (engine.hip) behind probe_host.hpp; uses engine_objects.hpp and, of solve_loops.hpp, LoopState, LoopClock and SolverWords.
#pragma once
#include "transfer.hpp"
// IGXTransfer: prolongation xf = P xc and restriction rc = P^T rf between two set-up IGX on nested knot vectors.  The tables are built on
// the host at IGXTransferCreate (transfer_axis_setup, host.cpp), which touches no device; the first Prolong / Restrict uploads them.  Every
// refusal is decided on the host before the first HIP call.  The clock is the loops' (LoopState's two events, LoopClock): the call stores
// its own figures on the FINE IGX under the self_timed rule.
struct TransferAxisBufs { DevBuf ufirst, count, T, boxlo, boxlen, pptr, pidx, pval, rptr, ridx, rval; };
struct _p_IGXTransfer : LoopState {
  IGX coarse = nullptr, fine = nullptr; unsigned long long cgen = 0, fgen = 0;
  int dim = 0, dof = 0, path = 0;                       // path: 0 automatic, 1 fused, 2 axis passes (IGXTransferSetPath)
  TransferAxis ax[3];
  int F[3] = {1, 1, 1}, nbox[3] = {1, 1, 1};            // the fused kernel's boxes: fine rows per box, boxes per axis
  std::vector<int> boxlo[3], boxlen[3];                 // a box's coarse footprint per axis (columns before folding)
  size_t sizeA = 0, sizeB = 0;                          // doubles of the fused kernel's two LDS buffers
  bool fits = false;                                    // the footprints fit TR_LDS_MAX: the fused kernel can run
  int64_t ntmp = 0;                                     // doubles of the largest intermediate of the axis passes
  bool on_device = false;
  TransferAxisBufs ab[3]; DevBuf tmp[2];
};
static const SolverWords kTransferWords = {"IGXTransferCreate", "the transfer needs one rank on every axis of both spaces: its boxes and gathers have no exchange across ranks", nullptr, nullptr};
static int transfer_stale(_p_IGXTransfer *q, const char *fn) {
  if (!q) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": null transfer");
  if (!q->coarse->current(q->cgen) || !q->fine->current(q->fgen))
    return fail(IGX_ERR_ORDER, std::string(fn) + ": the transfer is stale: IGXSetUp() ran on one of its IGX after IGXTransferCreate(); make a new transfer");
  return 0;
}
static void transfer_axis_unit(TransferAxis &t) {      // an axis beyond dim: one function on both sides
  t = TransferAxis(); t.first = {0}; t.count = {1}; t.ufirst = {0}; t.T = {1.0};
  t.pptr = {0, 1}; t.pidx = {0}; t.pval = {1.0}; t.rptr = {0, 1}; t.ridx = {0}; t.rval = {1.0};
}
static std::string transfer_name(const _p_IGXTransfer *q, bool down, bool fused) {      // down: the restriction, fine -> coarse
  std::string p, nc, nf;
  for (int d = 0; d < q->dim; ++d) {
    p += (d ? "," : "") + std::to_string(q->ax[d].p); nc += (d ? "x" : "") + std::to_string(q->ax[d].nc); nf += (d ? "x" : "") + std::to_string(q->ax[d].nf);
  }
  return std::string(down ? "transfer_restrict" : "transfer_prolong") + "(" + std::to_string(q->dim) + "d, p=" + p + ", " + (down ? nf : nc) + " -> " + (down ? nc : nf) + ", dof " + std::to_string(q->dof) + ", " + (fused ? "fused" : "axis passes") + ")";
}

extern "C" int IGXTransferCreate(IGX coarse, IGX fine, IGXTransfer *tr) {
  const SolverWords &words = kTransferWords;
  if (!coarse || !fine) return fail(IGX_ERR_ARG_WRONG, "IGXTransferCreate: null IGX: a transfer joins a coarse and a fine one");
  if (!tr) return fail(IGX_ERR_ARG_WRONG, "IGXTransferCreate: null pointer for the transfer");
  const Space &c = coarse->s, &f = fine->s;
  if (!c.setup || !f.setup) return fail(IGX_ERR_ORDER, std::string("Must call IGXSetUp() on both IGX before ") + words.call + "(): the transfer is built from the set-up knot vectors");
  if (c.dim != f.dim) return fail(IGX_ERR_ARG_WRONG, "IGXTransferCreate: the transfer needs the same dim on both sides, got " + std::to_string(c.dim) + " and " + std::to_string(f.dim));
  if (c.dof != f.dof) return fail(IGX_ERR_ARG_WRONG, "IGXTransferCreate: the transfer needs the same dof on both sides, got " + std::to_string(c.dof) + " and " + std::to_string(f.dof));
  for (int d = 0; d < f.dim; ++d) {
    if (c.axis[d].p != f.axis[d].p) return fail(IGX_ERR_ARG_WRONG, "IGXTransferCreate: the transfer needs the same degree on axis " + std::to_string(d) + " (degree elevation is not covered), got " + std::to_string(c.axis[d].p) + " and " + std::to_string(f.axis[d].p));
    if ((c.axis[d].periodic != 0) != (f.axis[d].periodic != 0)) return fail(IGX_ERR_ARG_WRONG, "IGXTransferCreate: the transfer needs the same periodicity on axis " + std::to_string(d));
  }
  if (coarse->stream != fine->stream) return fail(IGX_ERR_ARG_WRONG, "IGXTransferCreate: the transfer needs the same stream on both IGX (IGXSetStream): its work is enqueued on the fine one's");
  for (int d = 0; d < f.dim; ++d) if (c.proc_sizes[d] != 1 || f.proc_sizes[d] != 1) return fail(IGX_ERR_SUP, words.one_rank);
  for (int d = 0; d < f.dim; ++d) if (f.axis[d].p > 7) return fail(IGX_ERR_SUP, "IGXTransferCreate: the transfer covers degrees up to 7, axis " + std::to_string(d) + " has degree " + std::to_string(f.axis[d].p));
  for (int d = 0; d < f.dim; ++d) for (const Axis *ax : {&c.axis[d], &f.axis[d]}) {
    const int p = ax->p, m = ax->m;
    if ((int)ax->U.size() != m + 1 || m < 2 * p + 1) return fail(IGX_ERR_SUP, "IGXTransferCreate: the transfer needs the knot vectors, axis " + std::to_string(d) + " has none");
    if (!ax->periodic) for (int k = 0; k < p; ++k) if (ax->U[k] != ax->U[k + 1] || ax->U[m - k] != ax->U[m - k - 1])
      return fail(IGX_ERR_SUP, "IGXTransferCreate: the transfer covers clamped and periodic axes, axis " + std::to_string(d) + " is neither");
  }
  std::unique_ptr<_p_IGXTransfer> q(new _p_IGXTransfer());
  q->coarse = coarse; q->fine = fine; q->cgen = coarse->setup_gen; q->fgen = fine->setup_gen; q->dim = f.dim; q->dof = f.dof;
  for (int d = 0; d < 3; ++d) {
    if (d >= f.dim) { transfer_axis_unit(q->ax[d]); continue; }
    std::string e;
    if (int rc = transfer_axis_setup(c.axis[d], f.axis[d], d, q->ax[d], e)) return fail(rc, "IGXTransferCreate: the transfer refuses " + e);
    if (q->ax[d].nf != f.lay[d].nrow || q->ax[d].nc != c.lay[d].nrow) return fail(IGX_ERR_PLIB, "IGXTransferCreate: the transfer's tables and the vectors' row boxes differ on axis " + std::to_string(d));
  }
  // the fused kernel's boxes and their coarse footprints, from the tables themselves
  const int Fmax[3] = {TR_FX, TR_FY, TR_FZ};
  int cmax[3];
  for (int d = 0; d < 3; ++d) {
    const TransferAxis &t = q->ax[d];
    const int F = std::min(Fmax[d], t.nf), nb = (t.nf + F - 1) / F;
    q->F[d] = F; q->nbox[d] = nb; q->boxlo[d].resize(nb); q->boxlen[d].resize(nb); cmax[d] = 1;
    for (int b = 0; b < nb; ++b) {
      int lo = INT_MAX, hi = 0;
      for (int i = b * F; i < std::min(t.nf, (b + 1) * F); ++i) { lo = std::min(lo, t.ufirst[i]); hi = std::max(hi, t.ufirst[i] + t.count[i]); }
      q->boxlo[d][b] = lo; q->boxlen[d][b] = hi - lo; cmax[d] = std::max(cmax[d], hi - lo);
    }
  }
  q->sizeA = (size_t)q->dof * cmax[2] * std::max((size_t)cmax[1] * cmax[0], (size_t)q->F[1] * q->F[0]);
  q->sizeB = (size_t)q->dof * cmax[2] * cmax[1] * q->F[0];
  q->fits = (q->sizeA + q->sizeB) * sizeof(double) <= (size_t)TR_LDS_MAX && (int64_t)q->nbox[0] * q->nbox[1] * q->nbox[2] < (int64_t)INT_MAX;
  {   // the axis passes' intermediates: prolongation 0, 1, 2 and restriction 2, 1, 0
    const int64_t nf0 = q->ax[0].nf, nf1 = q->ax[1].nf, nc1 = q->ax[1].nc, nc2 = q->ax[2].nc;
    q->ntmp = q->dof * std::max(nc2 * std::max(nc1, nf1) * nf0, nc2 * nf1 * nf0);
    if ((int64_t)q->ax[2].nf * nf1 * nf0 * q->dof >= ((int64_t)1 << 32)) return fail(IGX_ERR_SUP, "IGXTransferCreate: the transfer covers fine vectors below 2^32 entries");
  }
  *tr = reinterpret_cast<IGXTransfer>(q.release());
  return 0;
}
extern "C" int IGXTransferDestroy(IGXTransfer *tr) { if (tr && *tr) { delete reinterpret_cast<_p_IGXTransfer *>(*tr); *tr = nullptr; } return 0; }
extern "C" int IGXTransferGetAxis(IGXTransfer tr, int axis, int *nf, int *nc, int *width, int first[], int count[], double T[]) {
  _p_IGXTransfer *q = reinterpret_cast<_p_IGXTransfer *>(tr);
  if (int rc = transfer_stale(q, "IGXTransferGetAxis")) return rc;
  if (axis < 0 || axis > 2) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTransferGetAxis: the transfer's axis must be in range [0,2]");
  const TransferAxis &t = q->ax[axis];
  if (nf) *nf = t.nf; if (nc) *nc = t.nc; if (width) *width = t.width;
  if (first) memcpy(first, t.first.data(), t.first.size() * sizeof(int));
  if (count) memcpy(count, t.count.data(), t.count.size() * sizeof(int));
  if (T) memcpy(T, t.T.data(), t.T.size() * sizeof(double));
  return 0;
}
extern "C" int IGXTransferSetPath(IGXTransfer tr, int path) {
  _p_IGXTransfer *q = reinterpret_cast<_p_IGXTransfer *>(tr);
  if (int rc = transfer_stale(q, "IGXTransferSetPath")) return rc;
  if (path < 0 || path > 2) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXTransferSetPath: the transfer's path must be 0 (automatic), 1 (fused) or 2 (axis passes)");
  if (path == 1 && !q->fits) return fail(IGX_ERR_SUP, "IGXTransferSetPath: the transfer's fused kernel needs " + std::to_string((q->sizeA + q->sizeB) * sizeof(double)) + " bytes of LDS for a box's coarse footprint, the budget is " + std::to_string(TR_LDS_MAX));
  q->path = path;
  return 0;
}
extern "C" int IGXTransferGetInfo(IGXTransfer tr, int box[3], int64_t *lds_bytes, int *fused) {
  _p_IGXTransfer *q = reinterpret_cast<_p_IGXTransfer *>(tr);
  if (int rc = transfer_stale(q, "IGXTransferGetInfo")) return rc;
  if (box) for (int d = 0; d < 3; ++d) box[d] = q->F[d];
  if (lds_bytes) *lds_bytes = (int64_t)((q->sizeA + q->sizeB) * sizeof(double));
  if (fused) *fused = q->fits && q->path != 2 ? 1 : 0;
  return 0;
}
static int transfer_upload(_p_IGXTransfer *q) {
  if (int rc = ensure_device(q->coarse)) return rc;
  if (int rc = ensure_device(q->fine)) return rc;
  if (q->on_device) return 0;
  for (int d = 0; d < 3; ++d) {
    const TransferAxis &t = q->ax[d]; TransferAxisBufs &B = q->ab[d];
    if (B.ufirst.upload(t.ufirst) || B.count.upload(t.count) || B.T.upload(t.T) || B.boxlo.upload(q->boxlo[d]) || B.boxlen.upload(q->boxlen[d]) || B.pptr.upload(t.pptr) ||
        B.pidx.upload(t.pidx) || B.pval.upload(t.pval) || B.rptr.upload(t.rptr) || B.ridx.upload(t.ridx) || B.rval.upload(t.rval))
      return fail(IGX_ERR_MEM, "device allocation of the transfer's tables failed");
  }
  for (auto &b : q->tmp) if (b.alloc((size_t)q->ntmp * sizeof(double))) return fail(IGX_ERR_MEM, "device allocation of the transfer's intermediates failed");
  q->on_device = true;
  return 0;
}
// the checks of Prolong and Restrict: vc lives on the coarse IGX, vf on the fine one
static int transfer_vec_args(_p_IGXTransfer *q, const char *fn, IGXVec vc, IGXVec vf) {
  if (int rc = transfer_stale(q, fn)) return rc;
  if (!vc || !vf) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": null vector: the transfer carries an IGXVec of the coarse IGX and one of the fine IGX");
  if (vc->iga != q->coarse) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": the coarse vector was created by another IGX than the transfer's coarse one");
  if (vf->iga != q->fine) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": the fine vector was created by another IGX than the transfer's fine one");
  if (vc->n != (int64_t)q->ax[0].nc * q->ax[1].nc * q->ax[2].nc * q->dof) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": the coarse vector is of another size than the transfer's coarse space");
  if (vf->n != (int64_t)q->ax[0].nf * q->ax[1].nf * q->ax[2].nf * q->dof) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": the fine vector is of another size than the transfer's fine space");
  if (vc == vf) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": the transfer needs two vectors, got the same one twice");
  if (q->coarse->stream != q->fine->stream) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": the transfer needs the same stream on both IGX (IGXSetStream)");
  return 0;
}
// the axis passes src -> dst in the order given, identity axes skipped (their rows multiply by 1.0: an exact copy); the last pass stores
// into dst, with add if asked; an all-identity transfer makes one pass, on the first axis of the order
static int transfer_passes(_p_IGXTransfer *q, bool down, const double *src, double *dst, int add, int *launches) {
  IGX g = q->fine;
  int order[3], n = 0;
  for (int k = 0; k < 3; ++k) { const int d = down ? 2 - k : k; if (!q->ax[d].identity) order[n++] = d; }
  if (!n) order[n++] = down ? 2 : 0;
  int64_t cur[3];
  for (int d = 0; d < 3; ++d) cur[d] = down ? q->ax[d].nf : q->ax[d].nc;
  const double *from = src;
  for (int k = 0; k < n; ++k) {
    const int d = order[k]; const TransferAxis &t = q->ax[d]; const TransferAxisBufs &B = q->ab[d];
    TrPassDev P;
    P.ptr = (down ? B.rptr : B.pptr).as<int>(); P.idx = (down ? B.ridx : B.pidx).as<int>(); P.val = (down ? B.rval : B.pval).as<double>();
    int64_t inner = q->dof, outer = 1;
    for (int e = 0; e < d; ++e) inner *= cur[e];
    for (int e = d + 1; e < 3; ++e) outer *= cur[e];
    const int64_t nout = down ? t.nc : t.nf, line = nout * inner, nblk = outer * ((line + TR_T - 1) / TR_T);
    if (line >= ((int64_t)1 << 32) || nblk >= ((int64_t)1 << 32)) return fail(IGX_ERR_SUP, "the transfer's axis pass covers lines and block counts below 2^32");
    P.nout = (unsigned)nout; P.nin = (unsigned)cur[d]; P.inner = (unsigned)inner; P.outer = (unsigned)outer;
    const bool last = k == n - 1;
    double *to = last ? dst : q->tmp[k & 1].as<double>();
    hipLaunchKernelGGL(transfer_axis_pass, dim3((unsigned)std::min<int64_t>(nblk, TR_G)), dim3(TR_T), 0, g->stream, P, from, to, last ? add : 0);
    if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "transfer_axis_pass: kernel launch failed");
    cur[d] = nout; from = to;
  }
  *launches = n;
  return 0;
}
extern "C" int IGXTransferProlong(IGXTransfer tr, IGXVec xc, IGXVec xf, int add) {
  _p_IGXTransfer *q = reinterpret_cast<_p_IGXTransfer *>(tr);
  if (int rc = transfer_vec_args(q, "IGXTransferProlong", xc, xf)) return rc;
  if (int rc = transfer_upload(q)) return rc;
  IGX g = q->fine; g->slab_valid = 0;
  const bool fused = q->fits && q->path != 2;
  LoopClock clock(g, *q);
  if (int rc = clock.begin(g)) return rc;
  if (fused) {
    TrFusedDev P; memset(&P, 0, sizeof(P));
    for (int d = 0; d < 3; ++d) {
      const TransferAxis &t = q->ax[d]; const TransferAxisBufs &B = q->ab[d]; TrAxisDev &A = P.ax[d];
      A.ufirst = B.ufirst.as<int>(); A.count = B.count.as<int>(); A.T = B.T.as<double>(); A.boxlo = B.boxlo.as<int>(); A.boxlen = B.boxlen.as<int>();
      A.nf = t.nf; A.nc = t.nc; A.width = t.width; A.F = q->F[d]; A.nbox = q->nbox[d]; A.wrap = t.periodic ? t.nc : INT_MAX;
    }
    P.dof = q->dof; P.sizeA = (int)q->sizeA;
    hipLaunchKernelGGL(transfer_prolong_fused, dim3((unsigned)(q->nbox[0] * q->nbox[1] * q->nbox[2])), dim3(TR_T), (q->sizeA + q->sizeB) * sizeof(double), g->stream, P, xc->a.as<double>(), xf->a.as<double>(), add ? 1 : 0);
    if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "transfer_prolong_fused: kernel launch failed");
    clock.own(1);
  } else {
    int n = 0;
    if (int rc = transfer_passes(q, false, xc->a.as<double>(), xf->a.as<double>(), add ? 1 : 0, &n)) return rc;
    clock.own(n);
  }
  if (int rc = clock.finish(g, transfer_name(q, false, fused))) return rc;
  if (clock.timing) g->last_kernel_ms = g->last_total_ms;      // the call is its kernels
  return 0;
}
extern "C" int IGXTransferRestrict(IGXTransfer tr, IGXVec rf, IGXVec rc_) {
  _p_IGXTransfer *q = reinterpret_cast<_p_IGXTransfer *>(tr);
  if (int rc = transfer_vec_args(q, "IGXTransferRestrict", rc_, rf)) return rc;
  if (int rc = transfer_upload(q)) return rc;
  IGX g = q->fine; g->slab_valid = 0; q->coarse->slab_valid = 0;
  LoopClock clock(g, *q);
  if (int rc = clock.begin(g)) return rc;
  int n = 0;
  if (int rc = transfer_passes(q, true, rf->a.as<double>(), rc_->a.as<double>(), 0, &n)) return rc;
  clock.own(n);
  if (int rc = clock.finish(g, transfer_name(q, true, false))) return rc;
  if (clock.timing) g->last_kernel_ms = g->last_total_ms;
  return 0;
}
