// element_sweep.hpp -- host side shared by the launchers of the two element kernels, the point-form kernel (generic_assemble,
// generic_kernel.hpp) and the feature-GEMM kernel (feature_assemble, feature_mfma.hpp), for built-in forms (dispatch_unit.hip:
// launch_generic, launch_feature_plan) and run-time forms (rtc.hpp: rtc_generic_launch, launch_feature_rtc) alike:
//   FormFacts       what a launcher must know about a form, by name: from the traits of a built-in form, from igx_user_meta[16] of a module
//   matfree_refusal where the matrix-free operators run, and why not: the one rule table of vec_sumfact's callers
//   color_sweeps    the ColorRange of every non-empty colour combination of an interior sweep or a face pass (also vec_sumfact's sweeps)
//   carve_generic / carve_feature      the kernels' LDS layouts (Carve, FCarve): a new region is added here, once
//   sweep_generic / sweep_feature      the launch loops, templated on the callable that makes one launch (hipLaunchKernelGGL of an
//                                      instantiation, hipModuleLaunchKernel of a module function): a new kind of sweep is added here, once
// Host code only; no kernel is defined here and the header is not part of the run-time compiled program.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "igx.hpp"
#include "forms.hpp"
#include "generic_kernel.hpp"
#include "feature_mfma.hpp"
#include "first_touch.hpp"

namespace igx {

// ------------------------------------------------------------------ small helpers
inline ParamsDev params_of(const Space &s) {
  ParamsDev prm; memset(&prm, 0, sizeof(prm));
  for (size_t i = 0; i < s.params.size() && i < MAXPARAM; ++i) prm.v[i] = s.params[i];
  return prm;
}

// ------------------------------------------------------------------ form facts
// The sixteen slots of igx_user_meta[] (rtc.hpp, rtc_compile) in their order, named after the traits they come from; the last slot is unused.
struct FormFacts {
  int dof = 0, order = 0; unsigned need = 0; int nscalar = 0, shape_order = 0; unsigned mat_need = 0;
  int gram = 0;                 // MAT_PAIR_MASK != 0: all row fields from one set of Gram accumulators
  int has_boundary = 0;         // the struct has an atboundary branch
  unsigned mat_test_mask = 0; int mat_symmetric = 0; unsigned vec_test_mask = 0;
  int pencil_nfeat = 0;         // PENCIL_NFEAT or 0
  int npairs = 0;               // bits of MAT_PAIR_MASK
  int vec_zero = 0, point_coef = 0;      // VEC_ZERO; NCOEF / point_coef declared (band_pt.hpp)
  bool second() const { return order >= 2; }
  bool third() const { return order >= 3; }
  bool general_only() const { return order >= 3 || (need & (NEED_PROP | NEED_D3U | NEED_MAPX)) != 0; }      // general_only_of (forms.hpp)
};
template <class Form> constexpr FormFacts facts_of() {
  FormFacts f;
  f.dof = Form::DOF; f.order = Form::ORDER; f.need = Form::NEED; f.nscalar = nscalar_of<Form>::v; f.shape_order = shape_order_of<Form>::v; f.mat_need = mat_need_of<Form>::v;
  f.gram = mat_pair_mask_of<Form>::v != 0ull; f.has_boundary = has_boundary_of<Form>::v; f.mat_test_mask = mat_test_mask_of<Form>::v; f.mat_symmetric = mat_symmetric_of<Form>::v;
  f.vec_test_mask = vec_test_mask_of<Form>::v; f.pencil_nfeat = pencil_state_of<Form>::nfeat; f.npairs = fm_popcount(mat_pair_mask_of<Form>::v); f.vec_zero = vec_zero_of<Form>::v;
  f.point_coef = has_point_coef<Form>::v;
  return f;
}
// ... of a run-time form: the one place that knows the order of the device array
inline FormFacts facts_from_meta(const int meta[16]) {
  FormFacts f;
  f.dof = meta[0]; f.order = meta[1]; f.need = (unsigned)meta[2]; f.nscalar = meta[3]; f.shape_order = meta[4]; f.mat_need = (unsigned)meta[5];
  f.gram = meta[6]; f.has_boundary = meta[7]; f.mat_test_mask = (unsigned)meta[8]; f.mat_symmetric = meta[9];
  f.vec_test_mask = (unsigned)meta[10]; f.pencil_nfeat = meta[11]; f.npairs = meta[12]; f.vec_zero = meta[13];
  f.point_coef = meta[14];
  return f;
}
// igx_feature_meta[4] of one feature_assemble module (rtc.hpp, rtc_feature_module); igx_band_meta[4] shares the storage under its own names (launch_band_rtc)
struct FeatureFacts {
  int wgs_per_cu = 0;           // workgroups per CU the kernel is compiled for (fm_min_waves)
  int phi_in_lds = 0;           // features kept in LDS (bits of PHI_MASK below the feature count)
  int mfma_per_kstep = 0;       // executed MFMAs per k-step (fm_mfma_per_kstep)
};
inline FeatureFacts feature_facts_from_meta(const int meta[4]) { FeatureFacts f; f.wgs_per_cu = meta[0]; f.phi_in_lds = meta[1]; f.mfma_per_kstep = meta[2]; return f; }

// ------------------------------------------------------------------ where the matrix-free operators run
// The actions, the diagonals and the point-block diagonals run on vec_sumfact or not at all: the one table of why not.  The rules, and the
// orders in which the callers ask them (the first that applies answers; include/petiga_amd.h and tests/test_gpu_matfree_routing.py pin them):
//   the space   S1 a boundary-form face, S2 dim != 3, S3 a geometry with nsd != dim, S4 more than 8 functions or points on an axis,
//               S5 IGX_VEC_SUMFACT=0, S6 IGXSetKernel != 0 -- worded for the action
//   the form    F1 order 3 / the property array / the map's derivatives, F2 a boundary branch (a built-in form: "or functionals"),
//               F3 second-order shape features (the diagonals alone)
//   the fields  N a struct with NSCALAR; D dof != the form's DOF (IGX_ERR_ARG_WRONG, never under a prefix)
//   MfCaller::FORM    a built-in form's launcher.  Actions: S1 S2 F1 F2 S3..S6 D (a form the action does not cover is not asked for the
//                     kernel).  Diagonals: S1..S6 F1 F2 F3 D.
//   MfCaller::STRUCT  a run-time struct's launcher: N D S1..S6 F1 F2 F3.
//   MfCaller::CHECK   IGXCheckFormSource, no N and no D.  gram 7 (action): "needs dim 3", S1..S6.  gram 8 (diagonal): "needs dim 3", F1 F2 F3,
//                     S1..S6.  gram 9 (block diagonal): S1..S6, F1 F2 F3.
//   facts == nullptr  the struct's constants are not known (a module that is not loaded), or the caller asks before it has a form at hand
//                     (a solve loop, the block action ahead of its first HIP call): the space's rules alone.
// A diagonal gives a rule of the space under "the matrix diagonal runs where the matrix action runs, and "; the block diagonal and the
// action on a block give every reason under their own such prefix (N excepted for the block diagonal, as ever).
enum class MfCaller { FORM, STRUCT, CHECK };
struct MfRefusal { int code = 0; std::string msg; explicit operator bool() const { return code != 0; } };
inline const char *matfree_space_rule(const Space &s, int kernel_choice, int &rule) {
  rule = 1;
  for (int d = 0; d < s.dim; ++d) for (int sd = 0; sd < 2; ++sd) if (s.visit[d][sd]) return "the matrix action does not cover boundary-form passes (IGXSetBoundaryForm): it runs on vec_sumfact alone";
  rule = 2;
  if (s.dim != 3) return "the matrix action needs dim = 3 (vec_sumfact: sum factorisation in three dimensions)";
  rule = 3;
  if (s.nsd != 0 && s.nsd != 3) return "the matrix action needs a geometry with nsd = dim";
  if (vec_lanes_per_axis(s) > 8) return "the matrix action needs nen <= 8 and nqp <= 8 on every axis (degree <= 7)";
  if (s.env.vec_sumfact == 0) return "the matrix action runs on vec_sumfact alone, and IGX_VEC_SUMFACT=0 switches that kernel off";
  if (kernel_choice != 0) return "the matrix action runs on vec_sumfact alone: IGXSetKernel must leave the choice automatic (0)";
  return nullptr;
}
inline MfRefusal matfree_refusal(const Space &s, int kernel_choice, VsMode mode, const FormFacts *f, MfCaller who) {
  const VsTraits t = vs_traits(mode);
  const std::string subject = t.diagonal ? "the matrix diagonal" : "the matrix action";
  auto under = [&](std::string why) {      // ... the names of the calls that stand on another
    if (t.block) why = "the matrix block diagonal runs where the matrix diagonal runs, and " + why;
    if (t.batch) why = "the matrix action on a block runs where the matrix action runs, and " + why;
    return MfRefusal{IGX_ERR_SUP, why};
  };
  int rule = 0;
  const char *sp = matfree_space_rule(s, kernel_choice, rule);
  auto space = [&]() { return under((t.diagonal ? "the matrix diagonal runs where the matrix action runs, and " : "") + std::string(sp)); };
  auto form = [&]() -> MfRefusal {
    if (!f) return {};
    if (f->general_only()) return under(subject + " does not cover forms of order 3 or forms that read the property array or the geometry map's derivatives");
    if (f->has_boundary || (who == MfCaller::FORM && f->nscalar != 0)) return under(subject + " does not cover forms with a boundary branch" + (who == MfCaller::FORM ? " or functionals" : ""));
    if (t.diagonal && f->shape_order >= 2) return under("the matrix diagonal does not cover forms with second-order shape features (Cahn-Hilliard's Laplacian): six product rows per axis and 55 coefficient slots per point are another kernel");
    return {};
  };
  if (who == MfCaller::CHECK && !t.block && s.dim != 3) return {IGX_ERR_SUP, subject + " needs dim 3"};
  if (who == MfCaller::STRUCT && f) {
    if (f->nscalar > 0) return {IGX_ERR_SUP, std::string(t.batch ? "the matrix action on a block runs where the matrix action runs, and " : "") + "a struct with NSCALAR is a functional: IGXComputeScalarSource"};
    if (s.dof != f->dof) return {IGX_ERR_ARG_WRONG, "form does not match the number of fields (dof)"};
  }
  const bool form_first = (who == MfCaller::FORM && !t.diagonal && rule > 2) || (who == MfCaller::CHECK && mode == VsMode::DIAGONAL);
  if (sp && !form_first) return space();
  if (const MfRefusal r = form()) return r;
  if (sp) return space();
  if (who == MfCaller::FORM && f && s.dof != f->dof) return {IGX_ERR_ARG_WRONG, "form does not match the number of fields (dof)"};
  return {};
}

// ------------------------------------------------------------------ colour sweeps
// colour c of an axis restricted to [lo,hi): arithmetic sequence (regular colours) or a single element
static bool color_range(const AxisLayout &L, int c, int lo, int hi, int &start, int &step, int &count) {
  start = -1; count = 0; step = L.p + 1;
  for (int e = lo; e < hi; ++e) if (L.color[e] == c) { if (start < 0) start = e; count++; }
  return count > 0;
}

// which elements of the rank a sweep takes
struct SweepSpec {
  int face_axis = -1, face_layer = 0;     // a face pass: that axis is the one local element layer at the face
  bool single = false;                    // functionals scatter nothing: every element in one combination, step 1
  int lo2 = 0, hi2 = -1;                  // a window of elements on axis 2 (hi2 < 0: the whole axis)
  bool axis0_whole = false;               // pencil mode: a workgroup walks axis 0; colours of axes 1 and 2 only
};
// calls visit(const ColorRange &) -> int for every non-empty colour combination, colours of axis 2 outermost and of axis 0 innermost;
// a non-zero answer ends the sweep and is returned
template <class Visit>
static int color_sweeps(const Space &s, const SweepSpec &w, Visit &&visit) {
  struct One { int start, step, count; };
  std::vector<One> col[3];
  for (int d = 0; d < 3; ++d) {
    const int nel = s.elem_width[d];
    if (d == w.face_axis) col[d].push_back({w.face_layer, 1, 1});
    else if (d == 0 && w.axis0_whole) col[d].push_back({0, 1, nel});
    else if (w.single) col[d].push_back({0, 1, nel});
    else for (int c = 0; c < s.lay[d].ncolors; ++c) {
      One o;
      if (color_range(s.lay[d], c, d == 2 ? w.lo2 : 0, (d == 2 && w.hi2 >= 0) ? w.hi2 : nel, o.start, o.step, o.count)) col[d].push_back(o);
    }
  }
  for (const One &c2 : col[2]) for (const One &c1 : col[1]) for (const One &c0 : col[0]) {
    const ColorRange cr = {{c0.start, c1.start, c2.start}, {c0.step, c1.step, c2.step}, {c0.count, c1.count, c2.count}};
    if (int rc = visit(cr)) return rc;
  }
  return 0;
}

// the visited faces (IGXSetBoundaryForm) that lie on this rank: bid = 2 * axis + side and the local element layer at the face
struct RankFace { int bid, axis, layer; };
static int faces_on_rank(const Space &s, RankFace faces[6]) {
  int n = 0;
  for (int bid = 0; bid < 2 * s.dim; ++bid) {
    const int ax = bid / 2, sd = bid % 2;
    if (!s.visit[ax][sd]) continue;
    const int eface = sd ? s.elem_sizes[ax] - 1 : 0;
    if (eface < s.elem_start[ax] || eface >= s.elem_start[ax] + s.elem_width[ax]) continue;   // the face is on another rank
    faces[n++] = {bid, ax, eface - s.elem_start[ax]};
  }
  return n;
}

// ------------------------------------------------------------------ LDS layouts
struct CarveTaker {          // regions in the order they are taken, each rounded up to 16 bytes
  int pos = 0;
  int operator()(int n) { int o = pos; pos += (n + 1) & ~1; return o; }
};

// generic_assemble: every region of the element and its points, and Phi while the block stays within phi_limit bytes (else
// cv.phi = -1 and the launcher gives every workgroup a slice of HBM scratch of phi_doubles)
struct GenericCarve { Carve cv; size_t lds_bytes = 0, phi_doubles = 0; bool phi_in_lds = false; };
static GenericCarve carve_generic(const FormFacts &f, const Space &s, int npd, int op, size_t phi_limit) {
  const int DIM = s.dim, DOF = f.dof, NS = f.nscalar, D2 = DIM * DIM, D3 = D2 * DIM;
  const bool SECOND = f.second(), THIRD = f.third();
  const int NF = 1 + DIM + (SECOND ? D2 : 0) + (THIRD ? D3 : 0);      // nfeat<DIM>(order)
  const bool fields = (f.need & (NEED_U | NEED_UT | NEED_GU | NEED_HU | NEED_D3U)) != 0;
  int nq[3], na[3]; int NQ = 1, NE = 1;
  for (int d = 0; d < 3; ++d) { nq[d] = s.basis[d].nqp; na[d] = s.basis[d].nen; NQ *= nq[d]; NE *= na[d]; }
  GenericCarve r; Carve &cv = r.cv; CarveTaker take;
  for (int d = 0; d < 3; ++d) { cv.t1d[d] = take(nq[d] * na[d] * NDER); cv.w1d[d] = take(nq[d]); }
  const int nsd = s.nsd ? s.nsd : DIM; const bool emb = s.nsd && s.nsd != DIM;
  cv.gX = take(NE * nsd); cv.gW = take(NE); cv.Ue = take(NE * DOF); cv.Ve = take(NE * DOF);
  cv.ufix = take(NE * DOF); cv.fixval = take(NE * DOF); cv.fixflag = take(NE * DOF); cv.flux = take(NE * DOF);
  cv.JW = take(NQ); cv.xq = take(NQ * nsd); cv.E1 = take((s.nsd && !emb) ? NQ * D2 : 0); cv.E2 = take((s.nsd && !emb && SECOND) ? NQ * DIM * D2 : 0);
  cv.W0 = take(s.rational ? NQ : 0); cv.W1 = take(s.rational ? NQ * DIM : 0); cv.W2 = take((s.rational && SECOND) ? NQ * D2 : 0);
  cv.G = take((f.need & NEED_G) ? NQ * DIM * nsd : 0);
  cv.X1m = take((f.need & NEED_MAPX) ? NQ * nsd * DIM : 0); cv.X2m = take(((f.need & NEED_MAPX) && SECOND) ? NQ * nsd * D2 : 0);
  cv.E3 = take((s.nsd && !emb && THIRD) ? NQ * DIM * D3 : 0); cv.W3 = take((s.rational && THIRD) ? NQ * D3 : 0);
  cv.d3u = take((THIRD && (f.need & NEED_D3U)) ? NQ * DOF * D3 : 0); cv.gA = take(NE * npd);
  cv.u = take(fields ? NQ * DOF : 0); cv.ut = take(fields ? NQ * DOF : 0);
  cv.gu = take((f.need & NEED_GU) ? NQ * DOF * DIM : 0); cv.hu = take((f.need & NEED_HU) ? NQ * DOF * D2 : 0);
  cv.lift = take(NS > 0 ? NQ * NS : (op == OP_SYSTEM ? NQ * DOF * NF : 0));
  cv.nrm = take(NQ * nsd);
  r.phi_doubles = (size_t)NQ * NE * NF;
  r.phi_in_lds = ((size_t)take.pos + r.phi_doubles) * sizeof(double) <= phi_limit;
  if (r.phi_in_lds) cv.phi = take((int)r.phi_doubles); else cv.phi = -1;
  cv.total = take.pos;
  r.lds_bytes = (size_t)take.pos * sizeof(double);
  return r;
}

// feature_assemble<.., TA, NW, ..>: the fewest chunks of points whose block fits the LDS the kernel is sized for -- wgs_per_cu workgroups
// per CU for the 4-wave kernels, one per CU for the 8-wave ones unless the form is scalar (IGX_FEATURE_LDS_KB overrides) -- and failing
// that the fewest that fit the LDS at all.  nps: features kept in LDS; stage_need: doubles the pencil mode parks in the Phi region.
struct FeatureCarve { FCarve cv; size_t lds_bytes = 0; bool fits = false; };
static FeatureCarve carve_feature(const FormFacts &f, const Space &s, int op, int TA, int NW, bool HASM, int wgs_per_cu, int nps, int stage_need) {
  const int DIM = s.dim, DOF = f.dof, SCALN = f.nscalar, D2 = DIM * DIM;
  const bool SECOND = f.second(), SECOND_S = f.shape_order >= 2;
  const int NFS = SECOND_S ? 1 + DIM + D2 : 1 + DIM;
  int nq[3], na[3]; int NQ = 1, NE = 1;
  for (int d = 0; d < 3; ++d) { nq[d] = s.basis[d].nqp; na[d] = s.basis[d].nen; NQ *= nq[d]; NE *= na[d]; }
  const int NEP = 16 * TA, NQ4 = (NQ + 3) & ~3;
  const bool vec_op = op_has_vector(op);
  const unsigned need = (vec_op || SCALN > 0) ? f.need : f.mat_need;   // as in the kernel: matrix-only drivers skip residual-only point data
  const bool fields = (need & (NEED_U | NEED_UT | NEED_GU | NEED_HU)) != 0;
  // LDS budget per workgroup.  4-wave kernels (nen <= 32) are compiled for 2-4 waves per SIMD (fm_min_waves) and sized
  // so that as many workgroups fit a CU: their latency-bound tabulation phases then overlap (CahnHilliard p=2 tangent
  // 12.8 -> 21.6 M elements/s, residual 16.7 -> 28.9).  8-wave kernels (nen = 64) hold one workgroup per CU unless the
  // form is scalar (16 accumulator VGPRs: Poisson p=3 on a NURBS geometry 8.2 vs 6.4 M/s); for the others the fewest
  // chunks of points win (NS-VMS 0.92 vs 0.84, Elasticity 2.67 vs 2.24 M/s).
  // (a module kernel takes more than 64 KiB of dynamic LDS like any other: measured)
  const size_t lds_limit = 160 * 1024 - 512;
  const size_t lds_auto = (NW == 4) ? (size_t)(160 * 1024 / wgs_per_cu - 1024) : ((HASM && TA == 4 && DOF == 1) ? (size_t)78 * 1024 : lds_limit);
  const size_t lds_target = s.env.feature_lds_kb > 0 ? (size_t)s.env.feature_lds_kb * 1024 : lds_auto;   // experiment switch
  FeatureCarve r; FCarve &cv = r.cv;
  for (int pass = 0; pass < 2 && !r.fits; ++pass) {
    const size_t cap = pass == 0 ? lds_target : lds_limit;
    for (int nchunk = 1; nchunk <= NQ4 / 4 && !r.fits; ++nchunk) {
      const int QC = (((NQ4 + nchunk - 1) / nchunk) + 3) & ~3, NQP = QC * nchunk;
      CarveTaker take;
      memset(&cv, 0, sizeof(cv));
      for (int d = 0; d < 3; ++d) { cv.t1d[d] = take(nq[d] * na[d] * NDER); cv.w1d[d] = take(2 * nq[d]); }
      cv.gX = take(NE * DIM); cv.gW = take(NE); cv.Ue = take(NE * DOF); cv.Ve = take(NE * DOF);
      cv.ufix = take(NE * DOF); cv.fixval = take(NE * DOF); cv.fixflag = take(NE * DOF); cv.flux = take(NE * DOF);
      cv.JW = take(NQP); cv.xq = take(NQP * DIM); cv.E1 = take(s.nsd ? NQP * D2 : 0); cv.E2 = take((s.nsd && SECOND) ? NQP * DIM * D2 : 0);
      cv.W0 = take(s.rational ? NQP : 0); cv.W1 = take(s.rational ? NQP * DIM : 0); cv.W2 = take((s.rational && SECOND) ? NQP * D2 : 0);
      cv.G = take((f.need & NEED_G) ? NQP * D2 : 0);
      cv.u = take(fields ? QC * DOF : 0); cv.ut = take(fields ? QC * DOF : 0);
      cv.gu = take((need & NEED_GU) ? QC * DOF * DIM : 0);
      cv.hu = take((need & NEED_HU) ? ((SECOND && !SECOND_S) ? NQP : QC) * DOF * D2 : 0);
      cv.hpart = 0;
      cv.lift = take(SCALN > 0 ? QC * SCALN : (op == OP_SYSTEM ? QC * DOF * NFS : 0));
      cv.rowbase = take(HASM ? NE : 0); cv.rowid = take(NE); cv.cc = take(NE); cv.pax = take(96); cv.adec = take(NEP / 2); cv.qdec = take((NQP + 1) / 2); cv.nrm = take(NQP * DIM);
      // the sum-factorised geometry sums of phase 1 borrow the Phi region before Phi exists
      // (and so do the sums behind the field Hessians of a form that reads them without second derivatives of N: DOF components)
      const bool hu_fly = SECOND && !SECOND_S && (f.need & NEED_HU) != 0;
      cv.sfb = (NE > 64) ? 1 : DOF;      // large elements: one field at a time
      const int sf_nc = std::max((s.nsd || s.rational) ? DIM + 1 : 0, (hu_fly && (need & NEED_HU)) ? cv.sfb : 0);
      const int sf_need = sf_nc * ((SECOND ? 3 : 2) * nq[0] * na[1] * na[2] + (SECOND ? 6 : 3) * nq[0] * nq[1] * na[2] + (SECOND ? 10 : 4) * NQ);
      cv.boff = 0;
      cv.phi = take(std::max(std::max(nps * QC * NEP, sf_need), stage_need));
      cv.total = take.pos; cv.QC = QC; cv.nchunk = nchunk; cv.NEP = NEP;
      r.lds_bytes = (size_t)take.pos * sizeof(double);
      if (r.lds_bytes <= cap) r.fits = true;
    }
  }
  return r;
}

// ------------------------------------------------------------------ sweep drivers
// Engine is the IGX handle (engine_objects.hpp): its space, stream, scratch buffer, timing marks and the hooks of the running assembly.

// generic_assemble over the rank: the coloured interior sweep (functionals: one sweep), then one pass per visited face on this rank.
// Every colour or face layer is split along axis 2 so that no launch needs more than 2 GiB of HBM scratch for Phi (gc.phi_in_lds false);
// the scratch buffer grows to what the largest launch needs.  launch(sub, bid, elem_base, nblocks) -> int makes one launch of nblocks
// workgroups: bid = -1 for the interior, else the face; elem_base counts the elements of the launches before it (partial sums of functionals).
template <class Engine, class Launch>
static int sweep_generic(Engine g, std::string &err, const GenericCarve &gc, bool single, Launch &&launch) {
  const Space &s = g->s;
  const size_t scratch_cap = (size_t)2 << 30;   // HBM slice for Phi when it does not fit in LDS
  size_t max_blocks = gc.phi_in_lds ? ((size_t)1 << 30) : scratch_cap / (gc.phi_doubles * sizeof(double));
  if (max_blocks < 1) max_blocks = 1;
  int launches = 0; int64_t elem_base = 0;
  auto layer = [&](const ColorRange &cr, int bid) -> int {      // one colour (or face layer), split along axis 2 under the scratch cap
    const size_t per2 = (size_t)cr.count[0] * cr.count[1];
    const int chunk2 = (int)std::max<size_t>(1, std::min<size_t>((size_t)cr.count[2], max_blocks / std::max<size_t>(per2, 1)));
    if (!gc.phi_in_lds && per2 > max_blocks) { err = "scratch too small for one element layer"; return IGX_ERR_SUP; }
    for (int k0 = 0; k0 < cr.count[2]; k0 += chunk2) {
      ColorRange sub = cr; sub.start[2] = cr.start[2] + k0 * cr.step[2]; sub.count[2] = std::min(chunk2, cr.count[2] - k0);
      const size_t nblocks = per2 * sub.count[2];
      if (!gc.phi_in_lds) {
        const size_t need = nblocks * gc.phi_doubles * sizeof(double);
        if (g->scratch.bytes < need) {
          const hipError_t e = hipStreamSynchronize(g->stream);
          if (e != hipSuccess) { err = std::string("hipStreamSynchronize(g->stream): ") + hipGetErrorString(e); return IGX_ERR_LIB; }
          if (g->scratch.alloc(need)) { err = "scratch allocation failed"; return IGX_ERR_MEM; }
        }
      }
      if (int rc = launch(sub, bid, elem_base, nblocks)) return rc;
      elem_base += (int64_t)nblocks; launches++;
    }
    return 0;
  };
  SweepSpec w; w.single = single;
  if (int rc = color_sweeps(s, w, [&](const ColorRange &cr) { return layer(cr, -1); })) return rc;
  // boundary-form passes (IGAElementNextForm, src/petigaelem.c:427-447): the elements of this rank on a visited face, one point
  // layer at the face; their K_e / F_e add to what the interior pass left (stream order)
  RankFace faces[6];
  for (int k = 0, n = faces_on_rank(s, faces); k < n; ++k) {
    w.face_axis = faces[k].axis; w.face_layer = faces[k].layer;
    if (int rc = color_sweeps(s, w, [&](const ColorRange &cr) { return layer(cr, faces[k].bid); })) return rc;
  }
  g->last_launches = launches;
  return 0;
}

// feature_assemble over the rank.  Decides between first-touch stores and a zeroed matrix (regular e mod (p+1) colours on every axis; a
// rank with neighbours zeroes only the rows that keep neighbour-owned columns), makes the interior sweep -- element mode, or pencil mode
// with axis 0 whole -- in two passes over axis 2 with g->slab_done between them where two_pass allows it, then the face passes (element
// mode only), and fills g->dom around the launches.  launch(out, cr, nblocks, first, launches) -> int makes the launches of one colour.
struct FeatureSweep {
  bool HASM = false, pencil = false, single = false;
  bool two_pass = false;        // several ranks on axis 2 and a communicator: the elements within p layers of the upper face of axis 2 first
  const char *dom_name = "";
  long long dom_groups = 1;     // launches per element the roofline block counts
  double flop_per_element = 0;
};
template <class Engine, class Launch>
static int sweep_feature(Engine g, const OutDev &out, const FeatureSweep &fs, Launch &&launch) {
  const Space &s = g->s;
  const int DIM = s.dim;
  int launches = 0; bool first = true;
  // first-touch stores instead of MatZeroEntries + read (same rule as the pencil kernel)
  bool first_touch = fs.HASM && !s.env.no_first_touch;
  for (int d = 0; d < DIM && first_touch; ++d) first_touch = axis_first_touch_ok(s, d);
  OutDev out_ft = out; out_ft.first_touch = first_touch ? 1 : 0;
  if (fs.HASM) {
    if (!first_touch) { if (g->zero_matrix) g->zero_matrix(); }
    else if (s.proc_sizes[0] * s.proc_sizes[1] * s.proc_sizes[2] > 1) zero_neighbour_rows(s, out, g->stream);
  }
  int64_t elem_base = 0;
  if (g->timing && g->dom.ev0 && g->dom.launches == 0) (void)hipEventRecord(g->dom.ev0, g->stream);
  RankFace faces[6]; const int nfaces = faces_on_rank(s, faces);
  // the upper face of axis 2 first (every colour), a mark for the exchange (g->slab_done), then the rest -- as the pencil kernel does
  // (pencil_launch.hpp, try_gram_mfma)
  const int n2 = s.elem_width[2], p2 = s.axis[2].p;
  bool split = fs.two_pass && g->slab_done && !fs.single && DIM == 3 && s.proc_sizes[2] > 1 && (s.proc_ranks[2] < s.proc_sizes[2] - 1 || s.axis[2].periodic) && n2 >= 2 * (p2 + 1) && axis_first_touch_ok(s, 2);
  for (int a = 0; a < 3; ++a) for (int sd = 0; sd < 2; ++sd) if (s.visit[a][sd]) split = false;
  for (int pass = 0; pass < (split ? 2 : 1); ++pass) {
    SweepSpec w; w.single = fs.single; w.axis0_whole = fs.pencil;
    if (split) {
      w.lo2 = pass == 1 ? 0 : n2 - p2; w.hi2 = pass == 1 ? n2 - p2 : n2;
      out_ft.ft2_lo = w.lo2; out_ft.ft2_hi = w.hi2; out_ft.ft2_blocked = pass == 1 ? n2 - p2 : 0x7fffffff;
      if (pass == 1) g->slab_done();
    }
    const int rc = color_sweeps(s, w, [&](const ColorRange &cr) -> int {
      if (fs.pencil) {
        const int rc = launch(out_ft, cr, (size_t)cr.count[1] * cr.count[2], first, launches);
        first = false;
        return rc;
      }
      const size_t per2 = (size_t)cr.count[0] * cr.count[1];
      const int chunk2 = (int)std::max<size_t>(1, std::min<size_t>((size_t)cr.count[2], ((size_t)1 << 30) / std::max<size_t>(per2, 1)));
      for (int k0 = 0; k0 < cr.count[2]; k0 += chunk2) {
        ColorRange sub = cr; sub.start[2] = cr.start[2] + k0 * cr.step[2]; sub.count[2] = std::min(chunk2, cr.count[2] - k0);
        const size_t nblocks = per2 * sub.count[2];
        OutDev o2 = out_ft; o2.elem_base = elem_base; elem_base += (int64_t)nblocks;
        if (int rc = launch(o2, sub, nblocks, first, launches)) return rc;
        first = false;
      }
      return 0;
    });
    if (rc) return rc;
  }
  // boundary-form passes (IGAElementNextForm, src/petigaelem.c:427-447): the elements of this rank on a visited face,
  // one point layer at the face; their K_e / F_e add to what the interior pass left (stream order, no first touch)
  for (int k = 0; k < nfaces && !fs.pencil; ++k) {   // (the pencil plan is not chosen when a face is visited)
    OutDev ob = out; ob.bid = faces[k].bid;
    SweepSpec w; w.single = fs.single; w.face_axis = faces[k].axis; w.face_layer = faces[k].layer;
    const int rc = color_sweeps(s, w, [&](const ColorRange &cr) -> int {
      const size_t nblocks = (size_t)cr.count[0] * cr.count[1] * cr.count[2];
      ob.elem_base = elem_base; elem_base += (int64_t)nblocks;
      const int rc = launch(ob, cr, nblocks, first, launches);
      first = false;
      return rc;
    });
    if (rc) return rc;
  }
  g->last_launches = launches;
  if (g->dom.launches == 0) {   // dominant kernel of this assembly, for bench.py's roofline block
    if (g->timing && g->dom.ev1) (void)hipEventRecord(g->dom.ev1, g->stream);
    g->dom.name = fs.dom_name; g->dom.launches = launches;
    g->dom.elements = (long long)s.elem_width[0] * s.elem_width[1] * s.elem_width[2] * fs.dom_groups;
    g->dom.flop_per_element = fs.flop_per_element;
  }
  return 0;
}

}  // namespace igx
