// probe_host.hpp -- the host side of IGXProbe (kernels: probe.hpp, included here).  Host code only: it launches kernels and defines none.
// Included by the main unit (engine.hip) behind solve_loops.hpp; uses engine_objects.hpp, ensure_device and the engine's timing marks.
#pragma once
#include "probe.hpp"
// IGXProbe: IGAProbe (src/petigaprobe.c) for many points at once.  The points are located on the device once, at IGXProbeCreate; every
// refusal is decided on the host before the first HIP call.  A probe of no points never touches the device.
struct _p_IGXProbe {
  IGX iga; unsigned long long gen; int order, dim; int64_t npts, nlocal;
  DevBuf pts, span, local, out;
  std::vector<double> hpts; std::vector<unsigned char> hlocal;
};
static int probe_stale(_p_IGXProbe *q, const char *fn) {
  if (!q) return fail(IGX_ERR_ARG_WRONG, std::string(fn) + ": null probe");
  if (!q->iga->current(q->gen)) return fail(IGX_ERR_ORDER, std::string(fn) + ": the probe is stale: IGXSetUp() ran on its IGX after IGXProbeCreate(); make a new probe");
  return 0;
}
static ProbeDev make_probedev(IGX g) {
  ProbeDev L; memset(&L, 0, sizeof(L));
  const Space &s = g->s; L.dim = s.dim; L.namax = 1;
  for (int d = 0; d < s.dim; ++d) {
    const Axis &ax = s.axis[d]; ProbeAxisDev &A = L.ax[d];
    A.U = g->ab[d].knots.as<double>(); A.elof = g->ab[d].elof.as<int>(); A.p = ax.p; A.n = (int)ax.U.size() - 1 - ax.p - 1;
    A.estart = s.elem_start[d]; A.ewidth = s.elem_width[d];
    if (ax.p + 1 > L.namax) L.namax = ax.p + 1;
  }
  return L;
}
static int probe_grid(int64_t n) { const int64_t b = (n + PROBE_T - 1) / PROBE_T; return (int)(b < 1 ? 1 : (b > PROBE_G ? PROBE_G : b)); }
static const char *probe_geometry_kind(const Space &s) {
  const bool map = s.nsd == s.dim;
  if (!s.nsd) return "identity";
  if (map) return s.rational ? "rational" : "polynomial";
  return s.rational ? "rational, parametric (nsd != dim)" : "polynomial, parametric (nsd != dim)";
}
static std::string probe_name(const Space &s, int order, int64_t npts) {
  std::string p = std::to_string(s.axis[0].p);
  bool same = true; for (int d = 1; d < s.dim; ++d) same = same && s.axis[d].p == s.axis[0].p;
  if (!same) for (int d = 1; d < s.dim; ++d) p += "x" + std::to_string(s.axis[d].p);
  return "probe(" + std::to_string(s.dim) + "d, p=" + p + ", order=" + std::to_string(order) + ", " + probe_geometry_kind(s) + ", " + std::to_string((long long)npts) + " points)";
}
#define PROBE_ARGS int grid, size_t lds, hipStream_t st, const SpaceDev &S, const ProbeDev &L, const double *pts, const int *span, const unsigned char *local, const double *U, double *out, long long n
#define PROBE_PASS grid, lds, st, S, L, pts, span, local, U, out, n
#define PROBE_GO(R, M) hipLaunchKernelGGL((probe_eval<DIM, DER, R, M>), dim3(grid), dim3(PROBE_T), lds, st, S, L, pts, span, local, U, out, n)
template <int DIM, int DER> static void probe_launch_kind(bool rat, bool map, PROBE_ARGS) {
  if constexpr (DER == 0) { if (rat) PROBE_GO(true, false); else PROBE_GO(false, false); }      // a value needs no map
  else { if (rat && map) PROBE_GO(true, true); else if (rat) PROBE_GO(true, false); else if (map) PROBE_GO(false, true); else PROBE_GO(false, false); }
}
template <int DIM> static void probe_launch_der(int der, bool rat, bool map, PROBE_ARGS) {
  switch (der) {
    case 0: probe_launch_kind<DIM, 0>(rat, map, PROBE_PASS); break;
    case 1: probe_launch_kind<DIM, 1>(rat, map, PROBE_PASS); break;
    case 2: probe_launch_kind<DIM, 2>(rat, map, PROBE_PASS); break;
    default: probe_launch_kind<DIM, 3>(rat, map, PROBE_PASS); break;
  }
}
template <int DIM> static void probe_launch_geom(bool rat, int grid, size_t lds, hipStream_t st, const SpaceDev &S, const ProbeDev &L, const double *pts, const int *span, const unsigned char *local, double *out, long long n) {
  if (rat) hipLaunchKernelGGL((probe_geom<DIM, true>), dim3(grid), dim3(PROBE_T), lds, st, S, L, pts, span, local, out, n);
  else hipLaunchKernelGGL((probe_geom<DIM, false>), dim3(grid), dim3(PROBE_T), lds, st, S, L, pts, span, local, out, n);
}

extern "C" int IGXProbeCreate(IGX g, int order, int64_t npts, const double *u, IGXProbe *prb) {
  if (!g) return fail(IGX_ERR_ARG_WRONG, "IGXProbeCreate: null IGX: a probe belongs to one");
  if (!prb) return fail(IGX_ERR_ARG_WRONG, "IGXProbeCreate: null pointer for the probe");
  if (order == 4) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXProbeCreate: the probe's order 4 is not covered: the device keeps derivative slots 0..3");
  if (order < 0 || order > 3) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXProbeCreate: the probe's order must be in range [0,3]");
  if (npts < 0) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXProbeCreate: the probe's number of points must not be negative");
  const Space &s = g->s;
  if (!s.setup) return fail(IGX_ERR_ORDER, "Must call IGXSetUp() before IGXProbeCreate(): the probe locates its points in the set-up knot vectors");
  for (int d = 0; d < s.dim; ++d) if (s.axis[d].p > 7) return fail(IGX_ERR_SUP, "IGXProbeCreate: the probe covers degrees up to 7, axis " + std::to_string(d) + " has degree " + std::to_string(s.axis[d].p));
  if (npts > 0 && !u) return fail(IGX_ERR_ARG_WRONG, "IGXProbeCreate: null points for a probe of " + std::to_string((long long)npts) + " points");
  for (int64_t i = 0; i < npts; ++i) for (int d = 0; d < s.dim; ++d) {
    const Axis &ax = s.axis[d]; const double v = u[i * s.dim + d];
    const double lo = ax.U[ax.p], hi = ax.U[ax.U.size() - 1 - ax.p];
    if (!(v >= lo && v <= hi)) {
      char buf[256]; snprintf(buf, sizeof(buf), "IGXProbeCreate: point %lld of the probe has u[%d] = %g outside the axis [%g, %g]", (long long)i, d, v, lo, hi);
      return fail(IGX_ERR_ARG_OUTOFRANGE, buf);
    }
  }
  std::unique_ptr<_p_IGXProbe> q(new _p_IGXProbe());
  q->iga = g; q->gen = g->setup_gen; q->order = order; q->dim = s.dim; q->npts = npts; q->nlocal = 0;
  if (npts > 0) {
    if (int rc = ensure_device(g)) return rc;
    q->hpts.assign(u, u + npts * s.dim); q->hlocal.assign((size_t)npts, 0);
    if (q->pts.upload(q->hpts) || q->span.alloc((size_t)npts * 3 * sizeof(int)) || q->local.alloc((size_t)npts))
      return fail(IGX_ERR_MEM, "device allocation of the probe's points failed");
    const ProbeDev L = make_probedev(g);
    const int64_t nb = (npts + 255) / 256;
    const bool timing = g->timing && g->ev[0];
    if (timing) { HIPCK(hipEventRecord(g->ev[0], g->stream)); HIPCK(hipEventRecord(g->ev[1], g->stream)); }
    hipLaunchKernelGGL(probe_locate, dim3((unsigned)(nb > PROBE_G ? PROBE_G : nb)), dim3(256), 0, g->stream, L, q->pts.as<double>(), (long long)npts, q->span.as<int>(), q->local.as<unsigned char>());
    if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "probe_locate: kernel launch failed");
    if (timing) HIPCK(hipEventRecord(g->ev[2], g->stream));
    HIPCK(hipMemcpyAsync(q->hlocal.data(), q->local.p, (size_t)npts, hipMemcpyDeviceToHost, g->stream));
    if (timing) HIPCK(hipEventRecord(g->ev[3], g->stream));
    HIPCK(hipStreamSynchronize(g->stream));
    for (unsigned char f : q->hlocal) q->nlocal += f ? 1 : 0;
    g->last_kernel = "probe_locate(" + std::to_string(s.dim) + "d, " + std::to_string((long long)npts) + " points)"; g->last_launches = 1;
  }
  *prb = reinterpret_cast<IGXProbe>(q.release());
  return 0;
}
extern "C" int IGXProbeDestroy(IGXProbe *prb) { if (prb && *prb) { delete reinterpret_cast<_p_IGXProbe *>(*prb); *prb = nullptr; } return 0; }
extern "C" int IGXProbeGetLocal(IGXProbe prb, int64_t *nlocal, unsigned char *local) {
  _p_IGXProbe *q = reinterpret_cast<_p_IGXProbe *>(prb);
  if (int rc = probe_stale(q, "IGXProbeGetLocal")) return rc;
  if (nlocal) *nlocal = q->nlocal;
  if (local && q->npts > 0) memcpy(local, q->hlocal.data(), (size_t)q->npts);
  return 0;
}
extern "C" int IGXProbeGetInfo(IGXProbe prb, int64_t *npts, int *order, int *nsd, int64_t *points_per_turn) {
  _p_IGXProbe *q = reinterpret_cast<_p_IGXProbe *>(prb);
  if (int rc = probe_stale(q, "IGXProbeGetInfo")) return rc;
  if (npts) *npts = q->npts;
  if (order) *order = q->order;
  if (nsd) *nsd = q->iga->s.nsd ? q->iga->s.nsd : q->iga->s.dim;
  if (points_per_turn) *points_per_turn = (int64_t)PROBE_G * PROBE_T;
  return 0;
}
extern "C" int IGXProbeGeomMap(IGXProbe prb, double *x) {
  _p_IGXProbe *q = reinterpret_cast<_p_IGXProbe *>(prb);
  if (int rc = probe_stale(q, "IGXProbeGeomMap")) return rc;
  if (q->npts == 0) return 0;
  if (!x) return fail(IGX_ERR_ARG_WRONG, "IGXProbeGeomMap: null array for the probe's points in space");
  IGX g = q->iga; const Space &s = g->s;
  if (!s.nsd) {      // no geometry: x = u (mapX[0] = point, src/petigaprobe.c:360-363); a point of another rank: zeros
    for (int64_t i = 0; i < q->npts; ++i) for (int d = 0; d < s.dim; ++d) x[i * s.dim + d] = q->hlocal[i] ? q->hpts[i * s.dim + d] : 0.0;
    return 0;
  }
  if (int rc = ensure_device(g)) return rc;
  const size_t bytes = (size_t)q->npts * s.nsd * sizeof(double);
  if (q->out.bytes < bytes && q->out.alloc(bytes)) return fail(IGX_ERR_MEM, "device allocation of the probe's result failed");
  const SpaceDev S = make_spacedev(g); const ProbeDev L = make_probedev(g);
  const size_t lds = (size_t)3 * L.namax * PROBE_T * sizeof(double);
  const int grid = probe_grid(q->npts);
  const bool timing = g->timing && g->ev[0];
  if (timing) { HIPCK(hipEventRecord(g->ev[0], g->stream)); HIPCK(hipEventRecord(g->ev[1], g->stream)); }
  switch (s.dim) {
    case 1: probe_launch_geom<1>(s.rational != 0, grid, lds, g->stream, S, L, q->pts.as<double>(), q->span.as<int>(), q->local.as<unsigned char>(), q->out.as<double>(), (long long)q->npts); break;
    case 2: probe_launch_geom<2>(s.rational != 0, grid, lds, g->stream, S, L, q->pts.as<double>(), q->span.as<int>(), q->local.as<unsigned char>(), q->out.as<double>(), (long long)q->npts); break;
    default: probe_launch_geom<3>(s.rational != 0, grid, lds, g->stream, S, L, q->pts.as<double>(), q->span.as<int>(), q->local.as<unsigned char>(), q->out.as<double>(), (long long)q->npts); break;
  }
  if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "probe_geom: kernel launch failed");
  if (timing) HIPCK(hipEventRecord(g->ev[2], g->stream));
  HIPCK(hipMemcpyAsync(x, q->out.p, bytes, hipMemcpyDeviceToHost, g->stream));
  if (timing) HIPCK(hipEventRecord(g->ev[3], g->stream));
  HIPCK(hipStreamSynchronize(g->stream));
  g->last_kernel = "probe_geom(" + std::to_string(s.dim) + "d, " + probe_geometry_kind(s) + ", " + std::to_string((long long)q->npts) + " points)"; g->last_launches = 1;
  return 0;
}
extern "C" int IGXProbeEvaluate(IGXProbe prb, IGXVec U, int der, double *out) {
  _p_IGXProbe *q = reinterpret_cast<_p_IGXProbe *>(prb);
  if (int rc = probe_stale(q, "IGXProbeEvaluate")) return rc;
  if (der < 0 || der > q->order) return fail(IGX_ERR_ARG_OUTOFRANGE, "IGXProbeEvaluate: expecting 0 <= der <= " + std::to_string(q->order) + " (the probe's order), got der = " + std::to_string(der));
  IGX g = q->iga; const Space &s = g->s;
  if (!U) return fail(IGX_ERR_ARG_WRONG, "IGXProbeEvaluate: null vector: the probe evaluates the field an IGXVec holds");
  if (U->iga != g) return fail(IGX_ERR_ARG_WRONG, "IGXProbeEvaluate: the vector was created by another IGX than the probe's");
  if (U->n != (int64_t)s.lay[0].nrow * s.lay[1].nrow * s.lay[2].nrow * s.dof) return fail(IGX_ERR_ARG_WRONG, "IGXProbeEvaluate: the vector is of another size than the probe's space");
  if (q->npts == 0) { g->last_kernel = g->self_timed = probe_name(s, der, 0); g->last_launches = 0; g->last_total_ms = g->last_kernel_ms = 0; return 0; }
  if (!out) return fail(IGX_ERR_ARG_WRONG, "IGXProbeEvaluate: null array for the probe's result");
  if (int rc = ensure_device(g)) return rc;
  int no = 1; for (int k = 0; k < der; ++k) no *= s.dim;
  const size_t bytes = (size_t)q->npts * s.dof * no * sizeof(double);
  if (q->out.bytes < bytes && q->out.alloc(bytes)) return fail(IGX_ERR_MEM, "device allocation of the probe's result failed");
  const SpaceDev S = make_spacedev(g); const ProbeDev L = make_probedev(g);
  const size_t lds = (size_t)3 * L.namax * (der + 1) * PROBE_T * sizeof(double);
  const int grid = probe_grid(q->npts);
  const bool rat = s.rational != 0, map = s.nsd != 0 && s.nsd == s.dim;
  const bool timing = g->timing && g->ev[0];
  if (timing) { HIPCK(hipEventRecord(g->ev[0], g->stream)); HIPCK(hipEventRecord(g->ev[1], g->stream)); }
  const double *pts = q->pts.as<double>(); const int *span = q->span.as<int>(); const unsigned char *local = q->local.as<unsigned char>();
  const double *Ud = U->a.as<double>(); double *od = q->out.as<double>(); const long long n = (long long)q->npts; hipStream_t st = g->stream;
  switch (s.dim) {
    case 1: probe_launch_der<1>(der, rat, map, grid, lds, st, S, L, pts, span, local, Ud, od, n); break;
    case 2: probe_launch_der<2>(der, rat, map, grid, lds, st, S, L, pts, span, local, Ud, od, n); break;
    default: probe_launch_der<3>(der, rat, map, grid, lds, st, S, L, pts, span, local, Ud, od, n); break;
  }
  if (hipGetLastError() != hipSuccess) return fail(IGX_ERR_LIB, "probe_eval: kernel launch failed");
  if (timing) HIPCK(hipEventRecord(g->ev[2], g->stream));
  HIPCK(hipMemcpyAsync(out, q->out.p, bytes, hipMemcpyDeviceToHost, g->stream));
  if (timing) HIPCK(hipEventRecord(g->ev[3], g->stream));
  HIPCK(hipStreamSynchronize(g->stream));
  g->last_kernel = probe_name(s, der, q->npts); g->last_launches = 1;
  return 0;
}
