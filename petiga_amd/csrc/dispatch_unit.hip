// dispatch_unit.hip -- the element-kernel instantiations of one dimension / form group: compiled once per (IGX_TU_DIM, IGX_TU_GROUP) of
// petiga_amd/build.py's UNITS.  The main unit (engine.hip) reaches them through igx_tu_dispatch / igx_tu_matfree / igx_tu_scalar
// (engine_objects.hpp); a form of another group answers IGX_NOT_MINE.
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
#if !defined(IGX_TU_DIM) || !defined(IGX_TU_GROUP)
#error "dispatch_unit.hip is compiled with -DIGX_TU_DIM=d -DIGX_TU_GROUP=g (g = -1: every form group)"
#endif
#if IGX_TU_DIM == 3
#include "vec_sumfact.hpp"
#define IGX_HAVE_VEC_SUMFACT 1
#endif
#if IGX_TU_DIM == 3 && (IGX_TU_GROUP < 0 || IGX_TU_GROUP == 1)
#include "band_pt.hpp"           // (includes block_pencil.hpp; the constant-coefficient multi-field forms take band_pt on a mapped geometry)
#define IGX_HAVE_BLOCK_PENCIL 1
#define IGX_HAVE_BAND_PT 1
#elif IGX_TU_DIM == 3 && IGX_TU_GROUP == 2
#include "band_pt.hpp"
#define IGX_HAVE_BAND_PT 1
#endif
#include "engine_objects.hpp"

// ------------------------------------------------------------------ feature-GEMM kernel dispatch (feature_mfma.hpp)
// one launch per group of DOFI row fields: I0 = 0, DOFI, 2*DOFI, ...
template <class Form, int DIM, int TA, int NW, int DOFI, int I0, bool HASM, bool PENCIL = false>
static void launch_feature_passes(IGX g, const SpaceDev &S, const ParamsDev &prm, const OutDev &out, const ColorRange &cr, const FCarve &cv, size_t nblocks, size_t lds_bytes, bool first, int &launches) {
  if constexpr (HASM && !PENCIL && I0 == 0 && DOFI < Form::DOF) {
    if (g->s.env.fuse_groups) {   // all groups of row fields in one launch: the element is tabulated once (feature_mfma.hpp, FUSE)
      auto fused = feature_assemble<Form, DIM, TA, NW, 0, DOFI, true, false, true>;
      if (first) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(fused), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
      hipLaunchKernelGGL(fused, dim3((unsigned)nblocks), dim3(64 * NW), lds_bytes, g->stream, S, prm, out, cr, cv);
      launches++;
      return;
    }
  }
  auto kern = feature_assemble<Form, DIM, TA, NW, I0, DOFI, HASM, PENCIL>;
  if (first) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(64 * NW), lds_bytes, g->stream, S, prm, out, cr, cv);
  launches++;
  if constexpr (HASM && I0 + DOFI < Form::DOF) launch_feature_passes<Form, DIM, TA, NW, DOFI, I0 + DOFI, HASM, PENCIL>(g, S, prm, out, cr, cv, nblocks, lds_bytes, first, launches);
}

// executed v_mfma_f64_16x16x4 flops per element of the feature kernel's matrix phase (roofline accounting)
template <class Form, int TA>
static double feature_mfma_flop(int nq_padded) {
  constexpr int NFS = (shape_order_of<Form>::v >= 2) ? 13 : 4;
  return 2048.0 * fm_mfma_per_kstep<Form>(NFS) * TA * TA * (nq_padded / 4);
}

// Pencil mode of the feature kernel (combine before write along axis 0): 4x4x4 basis functions, one new node layer per element
// on axis 0 (a periodic axis 0 wrapped inside the rank is walked too: the last elements add to the rows the first ones wrote,
// inside the same workgroup; such an axis never has first-touch stores), no boundary-form passes, and enough pencils per
// colour of axes 1, 2 to fill the CUs (a workgroup walks the whole local axis-0 range).  IGX_COMBINE=0 / 1 overrides the count.
static bool feature_pencil_wanted(IGX g, int wgs_per_cu, bool pays) {
  const Space &s = g->s;
  if (s.dim != 3 || s.env.combine == 0) return false;
  for (int d = 0; d < 3; ++d) if (s.basis[d].nen != 4) return false;
  if (s.elem_width[0] < 4) return false;
  for (int a = 0; a < 3; ++a) for (int sd = 0; sd < 2; ++sd) if (s.visit[a][sd]) return false;
  for (int e = 0; e + 1 < s.elem_width[0]; ++e) if (s.basis[0].offset[s.elem_start[0] + e + 1] != s.basis[0].offset[s.elem_start[0] + e] + 1) return false;
  if (s.env.combine > 0) return true;
  if (!pays) return false;
  static const int ncu = [] { int dev = 0; hipDeviceProp_t pr; return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256; }();
  const int nc1 = std::max(1, s.lay[1].ncolors), nc2 = std::max(1, s.lay[2].ncolors);
  const long long per_colour = (long long)((s.elem_width[1] + nc1 - 1) / nc1) * ((s.elem_width[2] + nc2 - 1) / nc2);
  return per_colour * 2 >= (long long)ncu * wgs_per_cu;   // too few pencils: one element per workgroup fills the chip better
}

// returns 0 and sets done when the feature kernel ran; done stays false when the case is not covered
template <class Form, int DIM, int TA, int NW, int DOFI, bool HASM, bool PEN = false>
static int launch_feature_plan(IGX g, const SpaceDev &S, const OutDev &out, bool &done) {
  const Space &s = g->s;
  constexpr int DOF = Form::DOF;
  constexpr FormFacts facts = facts_of<Form>();
  constexpr int NFS = (facts.shape_order >= 2) ? 1 + DIM + DIM * DIM : 1 + DIM;
  constexpr int WGS = fm_min_waves<Form, TA, NW, DOFI, HASM, PEN>();
  constexpr int NPS = fm_popcount((unsigned long long)(phi_mask_of<Form>::v & ((1u << NFS) - 1u)));   // features kept in LDS
  // pencil mode parks the 7 leaving tiles of every (i,j) block of a launch in the Phi region before they are written out
  constexpr unsigned long long PR = mat_pair_mask_of<Form>::v;
  constexpr int stage_need = PEN ? 7 * 16 * 17 * (PR ? fm_popcount(fm_pairs_upper(PR)) : DOFI * DOF) : 0;   // the leaving tiles (feature_mfma.hpp)
  const FeatureCarve fc = carve_feature(facts, s, out.op, TA, NW, HASM, WGS, NPS, stage_need);
  if (!fc.fits) return 0;   // not covered: the generic kernel takes it
  const FCarve &cv = fc.cv; const size_t lds_bytes = fc.lds_bytes;
  const ParamsDev prm = params_of(s);
  const bool fused = HASM && !PEN && DOFI < DOF && s.env.fuse_groups;   // one launch forms all groups of row fields of its elements
  FeatureSweep fs;
  fs.HASM = HASM; fs.pencil = PEN; fs.single = facts.nscalar > 0; fs.two_pass = true;
  fs.dom_name = PEN ? "feature_assemble<pencil>" : "feature_assemble<element>";
  fs.dom_groups = (HASM && !fused) ? (DOF / DOFI) : 1;
  fs.flop_per_element = HASM ? feature_mfma_flop<Form, TA>(cv.QC * cv.nchunk) * (fused ? DOF : DOFI) / DOF : 0.0;
  if (int rc = sweep_feature(g, out, fs, [&](const OutDev &o, const ColorRange &cr, size_t nblocks, bool first, int &launches) {
        launch_feature_passes<Form, DIM, TA, NW, DOFI, 0, HASM, PEN>(g, S, prm, o, cr, cv, nblocks, lds_bytes, first, launches);
        return 0;
      })) return rc;
  HIPCK(hipGetLastError());
  if (HASM) g->last_kernel = std::string("feature_assemble(mfma_f64_16x16x4,tiles=") + std::to_string(TA) + "x" + std::to_string(TA) + ",waves=" + char('0' + NW) +
                   ",rowfields/launch=" + char('0' + DOFI) + (fused ? std::string("x") + char('0' + DOF / DOFI) + " fused" : std::string()) +
                   ",chunks=" + std::to_string(cv.nchunk) + (PEN ? ",pencil walk axis 0" : "") + ")";
  else g->last_kernel = std::string("feature_assemble(vector only,waves=") + char('0' + NW) + ",chunks=" + std::to_string(cv.nchunk) + ")";
  done = true;
  return 0;
}

template <class Form, int DIM, int TA>
static int launch_feature_ta(IGX g, const SpaceDev &S, const OutDev &out, bool &done) {
  constexpr int DOF = Form::DOF;
  constexpr int NW = (TA >= 4) ? 8 : 4;
  // 4x4 tiles: 8 waves, <= 144 accumulator VGPRs per wave (dof 4: two launches of two row fields).  Measured on
  // Elasticity3D p=3: one launch of all row fields with 8 waves 2.67 M elements/s (3.2 with Gram accumulators); three
  // launches of one row field with 4-wave workgroups, two per CU, 1.63 M elements/s (tabulation repeated per launch).
  if constexpr (nscalar_of<Form>::v > 0) return launch_feature_plan<Form, DIM, TA, NW, DOF, false>(g, S, out, done);
  else {
    const bool hasM = op_has_matrix(out.op);
    if (!hasM) return launch_feature_plan<Form, DIM, TA, NW, DOF, false>(g, S, out, done);
    // field Hessians on the fly live in the vector-only kernels unless the matrix callback reads them too (feature_mfma.hpp,
    // HU_HERE): IGAComputeSystem of such a form (NS-VMS: nobody calls it) is left to the point-form kernel
    constexpr bool HU_SPLIT = Form::ORDER >= 2 && shape_order_of<Form>::v < 2 && (Form::NEED & NEED_HU) != 0 && (mat_need_of<Form>::v & NEED_HU) == 0;
    if (HU_SPLIT && out.op == OP_SYSTEM) return 0;
    constexpr bool GRAM = mat_pair_mask_of<Form>::v != 0ull;   // all row fields from one set of Gram accumulators
    // a scalar form at nen = 64 has 4 tiles per wave with 4-wave workgroups: small enough for 4 workgroups per CU
    // (Poisson p=3 on a NURBS geometry: 11.9 vs 10.4 M elements/s with the 8-wave layout)
    // 8x8 tiles (nen <= 128): a wave holds 8 tiles per accumulator set, so one row field per group (the groups are fused)
    constexpr int DOFI = (TA >= 8 && !GRAM) ? 1 : ((TA == 4 && DOF == 4 && !GRAM) ? 2 : DOF);
    if constexpr (TA == 4 && DIM == 3) {
      // pencil mode: the same wave layouts as the element mode (scalar forms: 4 waves with 4 tiles each, 4 workgroups per CU)
      constexpr int NWP = (DOF == 1) ? 4 : 8;
      constexpr int WG = fm_min_waves<Form, 4, NWP, (DOF == 1 ? 1 : DOFI), true, true>();
      // Measured (MI355X): Elasticity3D 128^3 3.35 -> 4.8 M elements/s; NavierStokesVMS 96^3 (two launches of 8 accumulator
      // sets, 128 registers live through a heavy tabulation) 1.41 -> 0.78: the automatic choice keeps the walk for the
      // constant-coefficient (Gram) multi-field forms.  Scalar forms lose as well (Poisson p=3 on a NURBS geometry, 128^3:
      // 8.5 vs 12.5 M elements/s: their scatter is small next to the tabulation, and the walk runs fewer workgroups per CU).
      constexpr bool PAYS = GRAM && DOF > 1;
      if (feature_pencil_wanted(g, WG, PAYS)) {   // (not covered when the staging buffers do not fit the LDS next to a mapped geometry's arrays)
        if (int rc = launch_feature_plan<Form, DIM, 4, NWP, (DOF == 1 ? 1 : DOFI), true, true>(g, S, out, done)) return rc;
        if (done) return 0;
      }
    }
    if constexpr (TA == 4 && DOF == 1) return launch_feature_plan<Form, DIM, 4, 4, 1, true>(g, S, out, done);
    else
    return launch_feature_plan<Form, DIM, TA, NW, DOFI, true>(g, S, out, done);
  }
}

template <class Form, int DIM>
static int launch_feature(IGX g, const SpaceDev &S, const OutDev &out, bool &done) {
  done = false;
  if constexpr (DIM < 2) return 0;
  else {
    const Space &s = g->s;
    constexpr bool fields = (Form::NEED & (NEED_U | NEED_UT | NEED_GU | NEED_HU)) != 0;
    if (s.dof != Form::DOF && (nscalar_of<Form>::v == 0 || fields)) return 0;
    int NE = 1; for (int d = 0; d < 3; ++d) NE *= s.basis[d].nen;
    if (NE > 256) return 0;
    if (NE > 128) {  // 16 tile rows x two panels of 8 tile columns (p = 5 in 3-D: nen = 216): one accumulator set of 16 tiles per wave
      constexpr unsigned long long PR = mat_pair_mask_of<Form>::v;
      constexpr int NACC16 = PR ? fm_popcount(PR) : Form::DOF;
      if constexpr (DIM == 3 && nscalar_of<Form>::v == 0 && !has_boundary_of<Form>::v) {
        for (int a = 0; a < 3; ++a) for (int sd = 0; sd < 2; ++sd) if (s.visit[a][sd]) return 0;
        if constexpr (NACC16 == 1) return launch_feature_ta<Form, DIM, 16>(g, S, out, done);
        else {
          const bool hasM = op_has_matrix(out.op);
          if (hasM) return 0;
          return launch_feature_plan<Form, DIM, 16, 8, Form::DOF, false>(g, S, out, done);
        }
      } else return 0;
    }
    if (NE > 64) {   // 8x8 tiles (p = 4 in 3-D: nen = 125) while the accumulators fit: <= 2 sets of 8 tiles per wave
      constexpr unsigned long long PR = mat_pair_mask_of<Form>::v;
      constexpr int NACC8 = PR ? fm_popcount(PR) : Form::DOF;      // Gram pairs, or the dof blocks of one row field
      if constexpr (DIM == 3 && nscalar_of<Form>::v == 0 && !has_boundary_of<Form>::v) {
        for (int a = 0; a < 3; ++a) for (int sd = 0; sd < 2; ++sd) if (s.visit[a][sd]) return 0;
        if constexpr (NACC8 <= 2) return launch_feature_ta<Form, DIM, 8>(g, S, out, done);
        else {   // more accumulator sets than a wave holds at 8 tiles each: the vector-only drivers still take the kernel
          const bool hasM = op_has_matrix(out.op);
          if (hasM) return 0;
          return launch_feature_plan<Form, DIM, 8, 8, Form::DOF, false>(g, S, out, done);
        }
      } else return 0;
    }
    if (NE <= 16) return launch_feature_ta<Form, DIM, 1>(g, S, out, done);
    if (NE <= 32) return launch_feature_ta<Form, DIM, 2>(g, S, out, done);
    return launch_feature_ta<Form, DIM, 4>(g, S, out, done);
  }
}

// ------------------------------------------------------------------ matrix-free dispatch
// The matrix-free operators of a built-in form (IGXCompute*Action, *ActionBlock, *Diagonal, *BlockDiagonal): vec_sumfact in the mode's
// instantiation, or the refusal matfree_refusal names (element_sweep.hpp) -- no other kernel forms them.  cols: ACTION_BATCH's columns.
template <class Form, int DIM>
static int launch_matfree(IGX g, const SpaceDev &S, const OutDev &out, VsMode mode, const ActionCols *cols) {
  const Space &s = g->s;
  constexpr FormFacts facts = facts_of<Form>();
  if (const MfRefusal r = matfree_refusal(s, g->kernel_choice, mode, &facts, MfCaller::FORM)) return fail(r.code, r.msg);
#ifdef IGX_HAVE_VEC_SUMFACT
  if constexpr (DIM == 3 && !general_only_of<Form>::v && nscalar_of<Form>::v == 0 && !has_boundary_of<Form>::v) {
    const ParamsDev prm = params_of(s);
    const VsTraits t = vs_traits(mode);
    bool done = false;
    auto run = [&](auto m) { return try_vec_sumfact<Form, decltype(m)::value>(s, S, prm, out, g->stream, g->last_kernel, g->last_launches, done, cols); };
    int rc = IGX_ERR_PLIB;
    if (mode == VsMode::ACTION) rc = run(std::integral_constant<VsMode, VsMode::ACTION>());
    else if (mode == VsMode::ACTION_BATCH) rc = run(std::integral_constant<VsMode, VsMode::ACTION_BATCH>());
    else if constexpr (shape_order_of<Form>::v < 2) rc = t.block ? run(std::integral_constant<VsMode, VsMode::BLOCK_DIAGONAL>()) : run(std::integral_constant<VsMode, VsMode::DIAGONAL>());
    if (rc) return fail(rc, "vec_sumfact kernel launch failed");
    return done ? 0 : fail(IGX_ERR_PLIB, std::string("vec_sumfact did not take a ") + (t.block ? "matrix block diagonal" : t.diagonal ? "matrix diagonal" : "matrix action") + " it covers");
  }
#endif
  return fail(IGX_ERR_PLIB, "matfree_refusal let a case pass that vec_sumfact does not hold");
}

// ------------------------------------------------------------------ generic kernel dispatch
template <class Form, int DIM>
static int launch_generic(IGX g, const SpaceDev &S, const OutDev &out) {
  const Space &s = g->s;
  constexpr int DOF = Form::DOF;
  constexpr bool THIRD = Form::ORDER >= 3;
  constexpr int NS = nscalar_of<Form>::v;
  // third-order tabulation, the property array and the point's shape table exist in the general kernel only
  constexpr bool GENERAL = general_only_of<Form>::v;
  const ParamsDev prm = params_of(s);
  if (GENERAL && g->kernel_choice != 0 && g->kernel_choice != 1) return fail(IGX_ERR_SUP, "a form of order 3 or one that reads the property array runs on the general kernel only");
  if ((Form::NEED & NEED_PROP) && !S.npd) return fail(IGX_ERR_ARG_WRONGSTATE, "No property set");      // src/petigaelem.c:300
  // a geometry of another dimension than the parametric one: tabulated by the general kernel only (no inverse map: src/petigaelem.c:966)
  const bool emb = s.nsd && s.nsd != DIM;
  if (emb && g->kernel_choice != 0 && g->kernel_choice != 1) return fail(IGX_ERR_SUP, "a geometry with nsd != dim runs on the general kernel only");
  if ((Form::NEED & NEED_MAPX) && !s.nsd) return fail(IGX_ERR_ARG_WRONGSTATE, "No geometry set");
  if (THIRD && s.order < 3) return fail(IGX_ERR_ARG_WRONGSTATE, "the form reads third derivatives (p->shape[3]): call IGASetOrder(iga,3) first");
#ifdef IGX_HAVE_VEC_SUMFACT
  if constexpr (DIM == 3 && !GENERAL) if (g->kernel_choice == 0 && !emb) {   // vector-only drivers: sum factorisation both ways (vec_sumfact.hpp)
    bool done = false;
    if (int rc = try_vec_sumfact<Form>(s, S, prm, out, g->stream, g->last_kernel, g->last_launches, done)) return fail(rc, "vec_sumfact kernel launch failed");
    if (done) return 0;
  }
#endif
#ifdef IGX_HAVE_BLOCK_PENCIL
  if constexpr (DIM == 3 && !GENERAL) if ((g->kernel_choice == 0 || g->kernel_choice == 4) && !emb) {   // band rows by node layer (block_pencil.hpp)
    bool done = false;
    if (int rc = try_block_pencil<Form>(s, S, prm, out, g->stream, g->last_kernel, g->last_launches, g_err, done, g->dom, g->zero_matrix, g->slab_done)) return rc;
    if (done) return 0;
  }
#endif
#ifdef IGX_HAVE_BAND_PT
  // (p = 2 only on request: the 27-function element in 4 x 4 x 4 tile slots wastes two thirds of the MFMAs there -- NS-VMS 48^3: 7.7 M el/s, the
  //  feature kernel's 2 x 2 tiles are as fast -- so the automatic choice keeps the feature kernel at p = 2)
  if constexpr (DIM == 3 && !GENERAL) if ((g->kernel_choice == 0 && s.axis[0].p == 3) || g->kernel_choice == 4) {   // band rows by node layer, point-dependent coefficients (band_pt.hpp)
    bool done = false;
    if (int rc = try_band_pt<Form>(s, S, prm, out, g->stream, g->last_kernel, g->last_launches, g_err, done, g->dom, g->zero_matrix, g->slab_done)) return rc;
    if (done) return 0;
  }
#endif
  if (g->kernel_choice == 4) return fail(IGX_ERR_SUP, "the band-row kernels do not cover this case (block_pencil: 3-D, p = 3, identity geometry, System / Matrix driver of a constant-coefficient form with 2 or 3 fields; band_pt: 3-D, p = 2 or 3, any geometry: matrix-only driver of a 4-field form with separated point coefficients, System / Matrix driver of a constant-coefficient form with 2 or 3 fields without boundary loads)");
  if constexpr (!GENERAL) if (g->kernel_choice != 1 && !emb) {   // matrix-producing ops: the dense contraction goes to the matrix cores when covered
    bool done = false;
    if (int rc = launch_feature<Form, DIM>(g, S, out, done)) return rc;
    if (done) return 0;
    if (g->kernel_choice == 3) return fail(IGX_ERR_SUP, "the feature-GEMM kernel does not cover this case (needs dim >= 2 and nen <= 64; in 3-D nen <= 128 / 256 for forms with at most two / one accumulator set)");
  }
  if (g->zero_matrix) g->zero_matrix();
  const bool fields = (Form::NEED & (NEED_U | NEED_UT | NEED_GU | NEED_HU | NEED_D3U)) != 0;
  if (s.dof != DOF && (NS == 0 || fields)) return fail(IGX_ERR_ARG_WRONG, "form does not match the number of fields (dof)");
  // Phi in LDS up to 64 KiB per workgroup, in an HBM slice beyond: a 131 KiB Phi (p = 3) in LDS leaves one workgroup per CU and
  // measured slower than the HBM slice with two (Poisson p=3 48^3: 0.91 vs 1.71 M elements/s, Elasticity 0.80 vs 1.28)
  const size_t lds_limit = 160 * 1024 - 512, phi_limit = 64 * 1024;
  const GenericCarve gc = carve_generic(facts_of<Form>(), s, S.npd, out.op, phi_limit);
  const size_t lds_bytes = gc.lds_bytes;
  if (lds_bytes > lds_limit) return fail(IGX_ERR_SUP, "element work set exceeds the 160 KiB LDS");
  auto kern = generic_assemble<Form, DIM>;
  HIPCK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  if (int rc = sweep_generic(g, g_err, gc, NS > 0, [&](const ColorRange &cr, int bid, int64_t elem_base, size_t nblocks) {
        OutDev o = out; o.bid = bid; o.elem_base = elem_base;
        hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(256), lds_bytes, g->stream, S, prm, o, cr, gc.cv, g->scratch.template as<double>(), gc.phi_doubles);
        return 0;
      })) return rc;
  HIPCK(hipGetLastError());
  g->last_kernel = std::string("generic_assemble(") + (gc.phi_in_lds ? "phi=LDS" : "phi=HBM") + ")";
  return 0;
}

// GROUP < 0: every form; else only the forms of that group (0 scalar second-order-free forms, 1 multi-field
// constant-coefficient forms, 2 the nonlinear demos), IGX_NOT_MINE for the others
// launch(form_tag<Form>()): the launcher of the entry -- the element kernels' (launch_generic) or the matrix-free operators' (launch_matfree)
template <class Form> struct form_tag { using type = Form; };
template <int DIM, int GROUP, class Launch>
static int dispatch_dim(IGX g, Launch &&launch) {
  const Space &s = g->s;
#define IGX_GROUP(gid, ...) do { if constexpr (GROUP < 0 || GROUP == (gid)) return launch(form_tag<__VA_ARGS__>()); else return IGX_NOT_MINE; } while (0)
  switch (s.form) {
  case IGX_FORM_POISSON:   IGX_GROUP(0, FormPoisson<DIM>);
  case IGX_FORM_POISSON_F: IGX_GROUP(0, FormPoissonF<DIM>);
  case IGX_FORM_L2PROJ_X2: IGX_GROUP(0, FormL2ProjX2<DIM>);
  case IGX_FORM_BOUNDARYINTEGRAL: IGX_GROUP(0, FormBoundaryIntegral<DIM>);
  case IGX_FORM_NITSCHE:          IGX_GROUP(0, FormNitsche<DIM>);
  case IGX_FORM_DER3:      IGX_GROUP(0, FormDer3<DIM>);
  case IGX_FORM_PROPERTY:  IGX_GROUP(0, FormProperty<DIM>);
  case IGX_FORM_SURFACE:
    if constexpr (GROUP < 0 || GROUP == 0) {
      if constexpr (DIM <= 2) return launch(form_tag<FormSurface<DIM>>());
      else return fail(IGX_ERR_ARG_WRONG, "the surface form needs dim = 1 or 2 (a curve or a surface in space)");
    } else return IGX_NOT_MINE;
  case IGX_FORM_ERRNORM:   IGX_GROUP(1, FormErrNorm<DIM>);
  case IGX_FORM_MASS:
    if constexpr (GROUP < 0 || GROUP == 1) {
      switch (s.dof) {
      case 1: return launch(form_tag<FormMass<DIM, 1>>());
      case 2: return launch(form_tag<FormMass<DIM, 2>>());
      case 3: return launch(form_tag<FormMass<DIM, 3>>());
      case 4: return launch(form_tag<FormMass<DIM, 4>>());
      default: return fail(IGX_ERR_SUP, "mass form is instantiated for dof 1..4");
      }
    } else return IGX_NOT_MINE;
  case IGX_FORM_ELASTICITY:
    if constexpr (GROUP < 0 || GROUP == 1) {
      if constexpr (DIM == 3) return launch(form_tag<FormElasticity>());
      else return fail(IGX_ERR_ARG_WRONG, "Elasticity3D form needs dim = 3");
    } else return IGX_NOT_MINE;
  case IGX_FORM_ELASTICITY_F:
    if constexpr (GROUP < 0 || GROUP == 1) {
      if constexpr (DIM == 3) return launch(form_tag<FormElasticityF>());
      else return fail(IGX_ERR_ARG_WRONG, "Elasticity3D form needs dim = 3");
    } else return IGX_NOT_MINE;
  case IGX_FORM_CAHNHILLIARD:
    if constexpr (GROUP < 0 || GROUP == 2) {
      if constexpr (DIM >= 2) return launch(form_tag<FormCahnHilliard<DIM>>());
      else return fail(IGX_ERR_ARG_WRONG, "Cahn-Hilliard form needs dim = 2 or 3");
    } else return IGX_NOT_MINE;
  case IGX_FORM_BRATU:     IGX_GROUP(2, FormBratu<DIM>);
  case IGX_FORM_NSVMS:
    if constexpr (GROUP < 0 || GROUP == 2) {
      if constexpr (DIM == 3) return launch(form_tag<FormNSVMS>());
      else return fail(IGX_ERR_ARG_WRONG, "NavierStokesVMS form needs dim = 3");
    } else return IGX_NOT_MINE;
  default: return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetForm...() first");   // IGACheckFormOp, include/petiga.h:925-936
  }
#undef IGX_GROUP
}

// IGAComputeScalar (src/petigacomp.c:35-98): the functionals of one dimension
template <int DIM>
static int dispatch_scalar(IGX g, int kind, const SpaceDev &S, const OutDev &out, int order) {
  switch (kind) {
  case IGX_SCALAR_VOLUME:  return launch_generic<ScalarVolume<DIM>, DIM>(g, S, out);
  case IGX_SCALAR_X2ERR:   return launch_generic<ScalarX2Err<DIM>, DIM>(g, S, out);
  case IGX_SCALAR_ERRNORM: return order >= 2 ? launch_generic<ScalarErrNorm<DIM, true>, DIM>(g, S, out) : launch_generic<ScalarErrNorm<DIM, false>, DIM>(g, S, out);
  default: return fail(IGX_ERR_ARG_OUTOFRANGE, "unknown scalar functional");
  }
}

// the entry points of this unit
int igx_tu_dispatch(std::integral_constant<int, IGX_TU_DIM>, std::integral_constant<int, IGX_TU_GROUP>, IGX g, const SpaceDev &S, const OutDev &out) {
  return dispatch_dim<IGX_TU_DIM, IGX_TU_GROUP>(g, [&](auto form) { return launch_generic<typename decltype(form)::type, IGX_TU_DIM>(g, S, out); });
}
int igx_tu_matfree(std::integral_constant<int, IGX_TU_DIM>, std::integral_constant<int, IGX_TU_GROUP>, IGX g, const SpaceDev &S, const OutDev &out, VsMode mode, const ActionCols *cols) {
  return dispatch_dim<IGX_TU_DIM, IGX_TU_GROUP>(g, [&](auto form) { return launch_matfree<typename decltype(form)::type, IGX_TU_DIM>(g, S, out, mode, cols); });
}
#if IGX_TU_GROUP < 0 || IGX_TU_GROUP == 2
int igx_tu_scalar(std::integral_constant<int, IGX_TU_DIM>, IGX g, int kind, const SpaceDev &S, const OutDev &out, int order) {
  return dispatch_scalar<IGX_TU_DIM>(g, kind, S, out, order);
}
#endif
