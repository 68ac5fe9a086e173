// rtc.hpp -- run-time compiled user forms (included by engine.hip, the main unit).
//
// PetIGA's point callbacks are arbitrary user functions (IGAFormSystem ... IGAFormIJacobian, include/petiga.h:153-197,
// registered through IGASetForm*, src/petigaform.c:388-833).  Host function pointers cannot run on the GPU and the built-in
// forms are a closed list, so the open end of the plugin API is source: the user hands over a HIP struct with the contract of
// forms.hpp (DOF, ORDER, NEED; mat() = un-weighted K block of a basis pair, vec() = un-weighted F entries of a basis
// function; zeroed outputs, row-major, src/petigapoint.c:427-462), IGXSetFormSource compiles
// generic_assemble<UserForm, dim> with hiprtc against the library's own headers (embedded at build time, rtc_sources.inc) and
// the seven drivers launch it like any built-in form: same closure, tabulation, boundary fix-up and coloured scatter.
// hiprtc is bound with dlopen, as RCCL is.  The compile itself needs no GPU (tests/test_rtc_forms.py checks the compile and
// its error log on the CPU; the launch is a GPU test against the oracle).
#include <dlfcn.h>
#include <unistd.h>
#include <map>
#include "rtc_sources.inc"
#include "module_launch.hpp"

namespace {

struct HiprtcApi {
  void *h = nullptr;
  int (*Create)(void **, const char *, const char *, int, const char **, const char **) = nullptr;
  int (*AddName)(void *, const char *) = nullptr;
  int (*Compile)(void *, int, const char **) = nullptr;
  int (*LogSize)(void *, size_t *) = nullptr;
  int (*Log)(void *, char *) = nullptr;
  int (*Lowered)(void *, const char *, const char **) = nullptr;
  int (*CodeSize)(void *, size_t *) = nullptr;
  int (*Code)(void *, char *) = nullptr;
  int (*Destroy)(void **) = nullptr;
  int (*Version)(int *, int *) = nullptr;      // hiprtcVersion(major, minor): part of the cache key
};
static HiprtcApi &hiprtc_api() { static HiprtcApi a; return a; }

static int load_hiprtc(std::string &err) {
  HiprtcApi &a = hiprtc_api();
  if (a.h) return 0;
  const char *env = getenv("IGX_HIPRTC_LIB");
  const char *names[] = {env, "libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"};
  for (int pass = 0; pass < 2 && !a.h; ++pass)
    for (const char *n : names) { if (!n || !*n) continue; a.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL | (pass == 0 ? RTLD_NOLOAD : 0)); if (a.h) break; }
  if (!a.h) {
    const char *why = dlerror();     // one call: the second would return NULL
    err = std::string("cannot load libhiprtc.so: ") + (why ? why : "not found");
    return IGX_ERR_LIB;
  }
  auto sym = [&](const char *n) { return dlsym(a.h, n); };
  a.Create = reinterpret_cast<decltype(a.Create)>(sym("hiprtcCreateProgram"));
  a.AddName = reinterpret_cast<decltype(a.AddName)>(sym("hiprtcAddNameExpression"));
  a.Compile = reinterpret_cast<decltype(a.Compile)>(sym("hiprtcCompileProgram"));
  a.LogSize = reinterpret_cast<decltype(a.LogSize)>(sym("hiprtcGetProgramLogSize"));
  a.Log = reinterpret_cast<decltype(a.Log)>(sym("hiprtcGetProgramLog"));
  a.Lowered = reinterpret_cast<decltype(a.Lowered)>(sym("hiprtcGetLoweredName"));
  a.CodeSize = reinterpret_cast<decltype(a.CodeSize)>(sym("hiprtcGetCodeSize"));
  a.Code = reinterpret_cast<decltype(a.Code)>(sym("hiprtcGetCode"));
  a.Destroy = reinterpret_cast<decltype(a.Destroy)>(sym("hiprtcDestroyProgram"));
  a.Version = reinterpret_cast<decltype(a.Version)>(sym("hiprtcVersion"));
  if (!a.Create || !a.AddName || !a.Compile || !a.LogSize || !a.Log || !a.Lowered || !a.CodeSize || !a.Code || !a.Destroy) { err = "libhiprtc.so lacks the expected API"; a = HiprtcApi(); return IGX_ERR_LIB; }
  return 0;
}

}  // namespace

// one program of a struct beyond the point-form kernel: the instantiations one family launches together (the groups of row fields of
// feature_assemble, one form_pencil / vec_sumfact / state_pencil / block_pencil, band_points + band_pt), built and loaded by rtc_instance
struct RtcInstance {
  std::vector<char> code;
  std::vector<std::string> lowered;
  hipModule_t module = nullptr; std::vector<hipFunction_t> func;      // (code without a module: compiled for IGXCheckFormSource, not yet launched)
  int meta[4] = {0, 0, 0, 0};          // the int[4] global the family asked to be read back (igx_feature_meta, igx_band_meta)
  bool guard_known = false, guard_ok = true; std::vector<double> guard_prm;     // band_pt: the struct's band_params_ok at the parameters it was last asked about
  bool failed = false; std::string why;     // band_pt under the automatic choice: the instantiation did not compile; the form stays on the feature kernel
  ~RtcInstance() { if (module) (void)hipModuleUnload(module); }
};

// one compiled user form for one dimension: code object + what the host-side launcher must know about the struct
struct RtcForm {
  std::string name, source, lowered;
  int dim = 0;
  std::vector<char> code;
  FormFacts facts;      // igx_user_meta[16] of the module by name (element_sweep.hpp); read by rtc_load
  hipModule_t module = nullptr; hipFunction_t func = nullptr;
  std::map<std::string, std::shared_ptr<RtcInstance>> instances;      // every family's, by the program's name expressions (rtc_key; the disk cache hashes the same text)
  ~RtcForm() { if (module) (void)hipModuleUnload(module); }
};

// Code-object cache on disk (IGX_RTC_CACHE_DIR): key = FNV-1a of the whole program text -- the library's own headers are part of
// it, so another library build never finds a stale object -- and of the name expressions.  File: [count][len, lowered name]...[code].
static unsigned long long rtc_fnv(const std::string &t, unsigned long long h = 1469598103934665603ull) {
  for (unsigned char ch : t) { h ^= ch; h *= 1099511628211ull; }
  return h;
}
// the options every program is compiled with: also part of the cache key
static const char *kRtcOpts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics"};
constexpr int kRtcNOpts = 4;
// key of a program: its whole text, the name expressions, the options above, the HIP this library was built against AND the version
// the loaded libhiprtc.so reports (it is bound at run time: another ROCm's compiler never finds this one's objects)
static unsigned long long rtc_program_key(const std::string &src, const std::vector<std::string> &exprs, unsigned long long seed) {
  std::string tool = "hip " + std::to_string(HIP_VERSION);
  for (int i = 0; i < kRtcNOpts; ++i) { tool += ' '; tool += kRtcOpts[i]; }
  { std::string e; int maj = 0, min = 0;
    if (load_hiprtc(e) == 0 && hiprtc_api().Version && hiprtc_api().Version(&maj, &min) == 0) tool += " hiprtc " + std::to_string(maj) + "." + std::to_string(min);
    else tool += " hiprtc ?"; }
  unsigned long long h = rtc_fnv(src, rtc_fnv(tool, seed));
  for (const std::string &x : exprs) h = rtc_fnv(x, h ^ 0x9e3779b97f4a7c15ull);
  return h;
}
static std::string rtc_cache_path(const std::string &src, const std::vector<std::string> &exprs) {
  const char *dir = getenv("IGX_RTC_CACHE_DIR");
  if (!dir || !*dir) return std::string();
  char name[64]; snprintf(name, sizeof(name), "/igx_%016llx.bin", rtc_program_key(src, exprs, 1469598103934665603ull));
  return std::string(dir) + name;
}
static bool rtc_cache_load(const std::string &path, size_t nexpr, std::vector<char> &code, std::vector<std::string> &lowered, unsigned long long check) {
  FILE *f = path.empty() ? nullptr : fopen(path.c_str(), "rb");
  if (!f) return false;
  bool ok = false;
  unsigned n = 0; unsigned long long stored = 0;
  // (the file starts with a second hash of the program -- another seed than the one in its name: a stale or foreign file is refused)
  if (fread(&stored, sizeof(stored), 1, f) == 1 && stored == check && fread(&n, sizeof(n), 1, f) == 1 && n == nexpr) {
    lowered.clear(); ok = true;
    for (unsigned i = 0; i < n && ok; ++i) {
      unsigned len = 0;
      ok = fread(&len, sizeof(len), 1, f) == 1 && len < (1u << 16);
      if (ok) { std::string t(len, '\0'); ok = len == 0 || fread(&t[0], 1, len, f) == len; lowered.push_back(t); }
    }
    unsigned long long cs = 0;
    ok = ok && fread(&cs, sizeof(cs), 1, f) == 1 && cs > 0 && cs < (1ull << 31);
    if (ok) { code.resize((size_t)cs); ok = fread(code.data(), 1, (size_t)cs, f) == cs; }
  }
  fclose(f);
  return ok;
}
static void rtc_cache_store(const std::string &path, const std::vector<char> &code, const std::vector<std::string> &lowered, unsigned long long check) {
  if (path.empty()) return;
  const std::string tmp = path + ".tmp" + std::to_string((long long)getpid());
  FILE *f = fopen(tmp.c_str(), "wb");
  if (!f) return;
  const unsigned n = (unsigned)lowered.size(); bool ok = fwrite(&check, sizeof(check), 1, f) == 1 && fwrite(&n, sizeof(n), 1, f) == 1;
  for (const std::string &t : lowered) { const unsigned len = (unsigned)t.size(); ok = ok && fwrite(&len, sizeof(len), 1, f) == 1 && (len == 0 || fwrite(t.data(), 1, len, f) == len); }
  const unsigned long long cs = code.size(); ok = ok && fwrite(&cs, sizeof(cs), 1, f) == 1 && fwrite(code.data(), 1, code.size(), f) == code.size();
  ok = (fclose(f) == 0) && ok;
  if (!ok || rename(tmp.c_str(), path.c_str()) != 0) (void)remove(tmp.c_str());     // (rename: concurrent ranks write the same object)
}

// the embedded headers a program needs beyond igx, forms, generic_kernel and feature_mfma, which every program has
enum RtcHeaders : unsigned { RTC_BASE = 0, RTC_GRAM = 1, RTC_VECSF = 2, RTC_BLOCK = 4, RTC_BAND = 8 };      // (band_pt.hpp builds on block_pencil.hpp)

// compiles `tail` behind the library headers and the user's source; returns the code object and the lowered names of `exprs`
static int rtc_build(const std::string &source, unsigned headers, const std::string &tail, const std::vector<std::string> &exprs,
                     std::vector<char> &code, std::vector<std::string> &lowered) {
  std::string src;
  src.reserve(source.size() + 400000);
  src += "#define IGX_RTC 1\n";
  src += kRtcSrc_igx; src += "\n"; src += kRtcSrc_forms; src += "\n"; src += kRtcSrc_generic; src += "\n"; src += kRtcSrc_feature; src += "\n";
  if (headers & RTC_GRAM) { src += kRtcSrc_pencil; src += "\n"; src += kRtcSrc_gram; src += "\n"; }
  if (headers & RTC_VECSF) { src += kRtcSrc_vecsf; src += "\n"; }
  if (headers & (RTC_BLOCK | RTC_BAND)) { src += kRtcSrc_pencil; src += "\n"; src += kRtcSrc_block; src += "\n"; }
  if (headers & RTC_BAND) { src += kRtcSrc_band; src += "\n"; }
  src += "using namespace igx;\n#line 1 \"user_form.hip\"\n";
  src += source;
  src += "\n";
  src += tail;
  const std::string cache = rtc_cache_path(src, exprs);
  const unsigned long long check = cache.empty() ? 0ull : rtc_program_key(src, exprs, 0x84222325cbf29ce4ull);
  if (rtc_cache_load(cache, exprs.size(), code, lowered, check)) return 0;
  std::string e; if (int rc = load_hiprtc(e)) return fail(rc, e);
  HiprtcApi &a = hiprtc_api();
  void *prog = nullptr;
  if (a.Create(&prog, src.c_str(), "igx_user_form.hip", 0, nullptr, nullptr) != 0) return fail(IGX_ERR_LIB, "hiprtcCreateProgram failed");
  for (const std::string &x : exprs) (void)a.AddName(prog, x.c_str());
  const int rc = a.Compile(prog, kRtcNOpts, kRtcOpts);
  if (rc != 0) {
    size_t n = 0; (void)a.LogSize(prog, &n); std::string log(n, '\0'); if (n) (void)a.Log(prog, &log[0]);
    (void)a.Destroy(&prog);
    return fail(IGX_ERR_USER, "the form source does not compile:\n" + log);
  }
  lowered.clear();
  for (const std::string &x : exprs) {
    const char *low = nullptr;
    if (a.Lowered(prog, x.c_str(), &low) != 0 || !low) { (void)a.Destroy(&prog); return fail(IGX_ERR_LIB, "hiprtcGetLoweredName failed"); }
    lowered.push_back(low);
  }
  size_t cs = 0;
  if (a.CodeSize(prog, &cs) != 0 || cs == 0) { (void)a.Destroy(&prog); return fail(IGX_ERR_LIB, "hiprtcGetCodeSize failed"); }
  code.resize(cs);
  if (a.Code(prog, code.data()) != 0) { (void)a.Destroy(&prog); return fail(IGX_ERR_LIB, "hiprtcGetCode failed"); }
  (void)a.Destroy(&prog);
  rtc_cache_store(cache, code, lowered, check);
  return 0;
}

static int rtc_compile(IGX g, const std::string &source, const std::string &name, int dim, std::shared_ptr<RtcForm> &out) {
  const std::string expr = "igx::generic_assemble<" + name + ", " + std::to_string(dim) + ">";
  std::string tail = "// what the host-side launcher reads back\n__device__ int igx_user_meta[16] = {" + name + "::DOF, " + name + "::ORDER, (int)" + name + "::NEED, igx::nscalar_of<" + name +
                     ">::v, igx::shape_order_of<" + name + ">::v, (int)igx::mat_need_of<" + name + ">::v, igx::mat_pair_mask_of<" + name + ">::v != 0ull, igx::has_boundary_of<" + name + ">::v, (int)igx::mat_test_mask_of<" +
                     name + ">::v, igx::mat_symmetric_of<" + name + ">::v, (int)igx::vec_test_mask_of<" + name + ">::v, igx::pencil_state_of<" + name + ">::nfeat, igx::fm_popcount(igx::mat_pair_mask_of<" + name + ">::v), igx::vec_zero_of<" + name + ">::v, igx::has_point_coef<" + name + ">::v, 0};\n";
  tail += "template __global__ void " + expr + "(igx::SpaceDev, igx::ParamsDev, igx::OutDev, igx::ColorRange, igx::Carve, double *, size_t);\n";
  std::shared_ptr<RtcForm> f(new RtcForm());
  std::vector<std::string> low;
  if (int rc = rtc_build(source, RTC_BASE, tail, {expr}, f->code, low)) return rc;
  f->lowered = low[0];
  f->name = name; f->source = source; f->dim = dim;
  out = f;
  return 0;
}

static int rtc_load(IGX g, RtcForm &f) {
  if (f.func) return 0;
  HIPCK(hipModuleLoadData(&f.module, f.code.data()));
  HIPCK(hipModuleGetFunction(&f.func, f.module, f.lowered.c_str()));
  hipDeviceptr_t p = nullptr; size_t n = 0;
  HIPCK(hipModuleGetGlobal(&p, &n, f.module, "igx_user_meta"));
  int meta[16];
  if (n != sizeof(meta)) return fail(IGX_ERR_LIB, "unexpected igx_user_meta size");
  HIPCK(hipMemcpy(meta, p, sizeof(meta), hipMemcpyDeviceToHost));
  f.facts = facts_from_meta(meta);
  return 0;
}

// ---- the store of a struct's instantiations and the one way into it.  A family says what its program is; rtc_instance finds it in
// F.instances or builds it (rtc_build: the disk cache or hiprtc), loads it when a driver is about to launch it, and keeps it.
// The program text is: the headers, the struct's source, `before`, one `template __global__ void X(sig);` per name expression, `after`.
struct RtcProgram {
  unsigned headers = RTC_BASE;
  std::vector<std::string> exprs; const char *sig = "";
  std::string before, after;        // the meta globals, static_assert and guard kernel of a family, on the side of the instantiations it has them
  const char *meta = nullptr;       // an int[4] global to read into RtcInstance::meta at the load
};

static const char *bool_name(bool b) { return b ? "true" : "false"; }

static int rtc_load_instance(RtcInstance &K, const char *meta_name) {
  HIPCK(hipModuleLoadData(&K.module, K.code.data()));
  for (const std::string &l : K.lowered) { hipFunction_t fn = nullptr; HIPCK(hipModuleGetFunction(&fn, K.module, l.c_str())); K.func.push_back(fn); }
  if (!meta_name) return 0;
  hipDeviceptr_t p = nullptr; size_t n = 0;
  HIPCK(hipModuleGetGlobal(&p, &n, K.module, meta_name));
  if (n != sizeof(K.meta)) return fail(IGX_ERR_LIB, std::string("unexpected ") + meta_name + " size");
  HIPCK(hipMemcpy(K.meta, p, sizeof(K.meta), hipMemcpyDeviceToHost));
  return 0;
}

// the key of a program in the store: its name expressions (band_points<F, degree> alone would not tell band_pt's geometries apart)
static std::string rtc_key(const RtcProgram &P) { std::string k; for (const std::string &x : P.exprs) { k += x; k += ';'; } return k; }
// load = false: the compile-only check (no GPU needed).  An entry that holds code is not built again: a driver loads what the check compiled.
static int rtc_instance(RtcForm &F, const RtcProgram &P, bool load, std::shared_ptr<RtcInstance> &K) {
  auto it = F.instances.find(rtc_key(P));
  if (it != F.instances.end() && !it->second->code.empty()) K = it->second;
  else {
    K.reset(new RtcInstance());
    std::string tail = P.before;
    for (const std::string &x : P.exprs) tail += "template __global__ void " + x + "(" + P.sig + ");\n";
    tail += P.after;
    if (int rc = rtc_build(F.source, P.headers, tail, P.exprs, K->code, K->lowered)) return rc;
    F.instances[rtc_key(P)] = K;
  }
  if (!load || K->module) return 0;
  const int rc = rtc_load_instance(*K, P.meta);
  if (rc) { if (K->module) (void)hipModuleUnload(K->module); K->module = nullptr; K->func.clear(); }      // (the next call loads again)
  return rc;
}

// MatZeroEntries of the running IGXCompute*, for the launchers that take it as a function (try_gram_mfma, block_pencil_run, band_pt_run)
static std::function<void()> zero_matrix_of(IGX g) { return g->zero_matrix ? g->zero_matrix : std::function<void()>([] {}); }

// the kernel arguments of generic_assemble, laid out as the kernarg segment is (natural alignment, in order)
struct RtcArgs { SpaceDev S; ParamsDev prm; OutDev out; ColorRange cr; Carve cv; double *phi_global; size_t phi_stride; };


// ---- the feature-GEMM kernel (feature_mfma.hpp) for a run-time form: launch_feature / launch_feature_ta / launch_feature_plan of
// dispatch_unit.hip with the form's constants read from the module.  Element mode only (no pencil walk), matrix / vector drivers.
struct RtcFeatArgs { SpaceDev S; ParamsDev prm; OutDev out; ColorRange cr; FCarve cv; };

// feature_assemble<UserForm, dim, TA, NW, I0, DOFI, HASM> for one wave layout: one function per group of row fields
// (DOF is passed in: it is read from the module on a GPU, and given by the caller for the compile-only check)
static int rtc_feature_module(RtcForm &F, int DIM, int DOF, int TA, int NW, int DOFI, bool HASM, bool load, std::shared_ptr<RtcInstance> &out) {
  RtcProgram P; P.sig = "igx::SpaceDev, igx::ParamsDev, igx::OutDev, igx::ColorRange, igx::FCarve"; P.meta = "igx_feature_meta";
  const std::string common = F.name + ", " + std::to_string(DIM) + ", " + std::to_string(TA) + ", " + std::to_string(NW) + ", ";
  const bool fuse = HASM && DOFI < DOF;   // all groups of row fields in one launch (feature_mfma.hpp, FUSE)
  for (int I0 = 0; I0 < ((HASM && !fuse) ? DOF : 1); I0 += DOFI)
    P.exprs.push_back("igx::feature_assemble<" + common + std::to_string(I0) + ", " + std::to_string(DOFI) + ", " + bool_name(HASM) + ", false, " + bool_name(fuse) + ">");
  const std::string nfs = "((igx::shape_order_of<" + F.name + ">::v >= 2) ? 1 + " + std::to_string(DIM) + " + " + std::to_string(DIM * DIM) + " : 1 + " + std::to_string(DIM) + ")";
  P.after = "__device__ int igx_feature_meta[4] = {igx::fm_min_waves<" + F.name + ", " + std::to_string(TA) + ", " + std::to_string(NW) + ", " + std::to_string(DOFI) + ", " + bool_name(HASM) +
            ", false>(), igx::fm_popcount((unsigned long long)(igx::phi_mask_of<" + F.name + ">::v & ((1u << " + nfs + ") - 1u))), igx::fm_mfma_per_kstep<" + F.name + ">(" + nfs + "), 0};\n";
  return rtc_instance(F, P, load, out);
}

// wave layouts of launch_feature_ta (dispatch_unit.hip): 8 waves at 4x4 tiles, except scalar matrix forms (4 waves with 4 tiles each);
// dof 4 at 4x4 tiles takes two launches of two row fields
static void rtc_feature_layout(int NE, int DOF, bool GRAM, bool HASM, int &TA, int &NW, int &DOFI) {
  TA = NE <= 16 ? 1 : (NE <= 32 ? 2 : (NE <= 64 ? 4 : (NE <= 128 ? 8 : 16)));
  NW = (TA >= 4) ? 8 : 4; DOFI = DOF;
  if (HASM) { if (TA == 8 && !GRAM) DOFI = 1; if (TA == 4 && DOF == 4 && !GRAM) DOFI = 2; if (TA == 4 && DOF == 1) NW = 4; }
}

static int launch_feature_rtc(IGX g, RtcForm &F, const SpaceDev &S, const OutDev &out, bool &done) {
  done = false;
  const Space &s = g->s;
  const int DIM = s.dim, DOF = F.facts.dof;
  if (DIM < 2 || DOF > 4) return 0;
  int NE = 1;
  for (int d = 0; d < 3; ++d) NE *= s.basis[d].nen;
  if (NE > 256) return 0;
  const bool SECOND = F.facts.second(), SECOND_S = F.facts.shape_order >= 2, GRAM = F.facts.gram != 0;
  if (NE > 64 && (DIM != 3 || GRAM || DOF > 2)) return 0;      // 8x8 tiles: p = 4 in 3-D, at most two accumulator sets per wave
  if (NE > 128 && DOF > 1) return 0;                           // 16 tile rows x two column panels: p = 5 in 3-D, one set
  if (GRAM && DOF * DOF > 16) return 0;
  const bool HASM = op_has_matrix(out.op);
  if (HASM && out.op == OP_SYSTEM && SECOND && !SECOND_S && (F.facts.need & NEED_HU) && !(F.facts.mat_need & NEED_HU)) return 0;   // (HU_HERE, feature_mfma.hpp)
  int TA, NW, DOFI; rtc_feature_layout(NE, DOF, GRAM, HASM, TA, NW, DOFI);
  std::shared_ptr<RtcInstance> K;
  if (int rc = rtc_feature_module(F, DIM, DOF, TA, NW, DOFI, HASM, true, K)) return rc;
  const FeatureFacts kf = feature_facts_from_meta(K->meta);      // igx_feature_meta[4] by name (element_sweep.hpp)
  const FeatureCarve fc = carve_feature(F.facts, s, out.op, TA, NW, HASM, std::max(kf.wgs_per_cu, 1), kf.phi_in_lds, 0);
  if (!fc.fits) return 0;   // the generic kernel takes it
  const FCarve &cv = fc.cv;
  RtcFeatArgs args; memset(&args, 0, sizeof(args));
  args.S = S; args.cv = cv; args.prm = params_of(s);
  // (no functionals, no second pass over axis 2, no pencil mode: element mode, one or several functions per colour)
  FeatureSweep fs;
  fs.HASM = HASM; fs.dom_name = "feature_assemble<element, hiprtc>";
  fs.flop_per_element = HASM ? 2048.0 * kf.mfma_per_kstep * TA * TA * (cv.QC * cv.nchunk / 4) : 0.0;
  if (int rc = sweep_feature(g, out, fs, [&](const OutDev &o, const ColorRange &cr, size_t nblocks, bool, int &launches) -> int {
        args.out = o; args.cr = cr;
        for (hipFunction_t fn : K->func) {
          HIPCK(module_launch(fn, (unsigned)nblocks, (unsigned)(64 * NW), fc.lds_bytes, g->stream, args));
          launches++;
        }
        return 0;
      })) return rc;
  if (HASM) g->last_kernel = std::string("feature_assemble<") + F.name + ">(hiprtc,mfma_f64_16x16x4,tiles=" + std::to_string(TA) + "x" + std::to_string(TA) + ",waves=" + char('0' + NW) +
                             ",rowfields/launch=" + char('0' + DOFI) + (DOFI < DOF ? std::string("x") + char('0' + DOF / DOFI) + " fused" : std::string()) + ",chunks=" + std::to_string(cv.nchunk) + ")";
  else g->last_kernel = std::string("feature_assemble<") + F.name + ">(hiprtc,vector only,waves=" + char('0' + NW) + ",chunks=" + std::to_string(cv.nchunk) + ")";
  done = true;
  return 0;
}

// ---- the pencil walk of gram_mfma.hpp for a run-time form (form_pencil): dof 1, first order, matrix integrand on the gradients only
// and symmetric (MAT_TEST_MASK = gradients, MAT_SYMMETRIC), load term on N only (VEC_TEST_MASK = 1), point data = x at most;
// dim 3, uniform degree 2 or 3 with p+1 Gauss points, System / Matrix drivers, axis 0 walkable, with or without a geometry.
// Everything around the kernel -- colours, segments, first touch, the Dirichlet fix-up inside the walk, boundary loads, the
// upper-face-first pass of a multi-rank assembly -- is try_gram_mfma itself.
static bool rtc_pencil_eligible(const Space &s, const RtcForm &F, const OutDev &out) {
  if (s.dim != 3 || F.facts.dof != 1 || F.facts.order >= 2 || F.facts.shape_order >= 2 || F.facts.nscalar > 0 || F.facts.has_boundary) return false;
  if ((F.facts.need & ~NEED_X) != 0u) return false;
  if ((F.facts.mat_test_mask & 0xfu) != 0xeu || !F.facts.mat_symmetric || (F.facts.vec_test_mask & 0xfu) != 0x1u) return false;
  if (out.op != OP_SYSTEM && out.op != OP_MATRIX) return false;
  if (s.nsd != 0 && s.nsd != 3) return false;
  const int deg = s.axis[0].p;
  if (deg != 2 && deg != 3) return false;
  for (int d = 0; d < 3; ++d) if (s.axis[d].p != deg || s.basis[d].nqp != deg + 1) return false;
  return true;
}

static const char *kPencilSig = "igx::SpaceDev, igx::OutDev, igx::PencilArgs, igx::ParamsDev";      // form_pencil and the state_pencil kernels
static int launch_pencil_rtc(IGX g, RtcForm &F, const SpaceDev &S, const OutDev &out, bool &done, bool compile_only = false, int sys_only = -1) {
  done = false;
  const Space &s = g->s;
  if (!compile_only && !rtc_pencil_eligible(s, F, out)) return 0;
  const int deg = s.axis[0].p;
  const bool sys = compile_only ? sys_only != 0 : out.op == OP_SYSTEM, ident = s.nsd == 0, rat = s.rational != 0;
  RtcProgram P; P.headers = RTC_GRAM; P.sig = kPencilSig;
  P.exprs = {std::string("igx::form_pencil<") + bool_name(sys) + ", " + std::to_string(deg) + ", " + bool_name(ident) + ", " + bool_name(rat) + ", " + F.name + ">"};
  std::shared_ptr<RtcInstance> K;
  if (int rc = rtc_instance(F, P, !compile_only, K)) return rc;
  if (compile_only) { done = true; return 0; }
  PencilModule mod; mod.prm = params_of(s);
  mod.fn = K->func[0]; mod.name = F.name;
  return try_gram_mfma(s, S, out, g->stream, false, g->last_kernel, g->last_launches, g_err, done, g->dom, zero_matrix_of(g), g->slab_done, &mod, g->face_done);
}

// ---- the sum-factorised vector kernel (vec_sumfact.hpp) for a run-time form: Vector / Function / IFunction in 3-D at nen, nqp <= 4
// per axis; the conditions of vec_sumfact_covers with the struct's constants read from the module
struct RtcVecArgs { SpaceDev S; ParamsDev prm; OutDev out; ColorRange cr; long long nelem; };
static bool rtc_vecsf_eligible(const Space &s, const RtcForm &F, const OutDev &out) {
  if (!s.env.vec_sumfact || s.dim != 3 || F.facts.nscalar > 0 || F.facts.has_boundary) return false;      // no functionals, no atboundary branch
  if (out.op != OP_VECTOR && out.op != OP_FUNCTION && out.op != OP_IFUNCTION) return false;
  if (s.dof != F.facts.dof || (s.nsd != 0 && s.nsd != 3)) return false;
  for (int d = 0; d < 3; ++d) {
    if (s.basis[d].nen > 4 || s.basis[d].nqp > 4) return false;
    for (int sd = 0; sd < 2; ++sd) { if (s.visit[d][sd]) return false; if (out.op != OP_VECTOR && s.load[d][sd].count) return false; }
  }
  return true;
}
// mode: the instantiation of that mode (igx.hpp: VsMode), in the layout vs_launch_of gives; the matrix-free modes' caller has asked
// matfree_refusal.  A struct has no ACTION_BATCH instantiation yet: its columns come one by one (compute_matfree)
static int launch_vecsf_rtc(IGX g, RtcForm &F, const SpaceDev &S, const OutDev &out, bool &done, VsMode mode = VsMode::VECTOR, bool compile_only = false) {
  done = false;
  const Space &s = g->s;
  const VsTraits t = vs_traits(mode);
  if (t.batch) return fail(IGX_ERR_PLIB, "a run-time struct has no instantiation of vec_sumfact on a block of columns");
  if (!compile_only && mode == VsMode::VECTOR && !rtc_vecsf_eligible(s, F, out)) return 0;
  const bool geo = s.nsd > 0 || s.rational;
  const VsLaunch L = vs_launch_of(s, mode, compile_only);
  RtcProgram P; P.headers = RTC_VECSF; P.sig = "igx::SpaceDev, igx::ParamsDev, igx::OutDev, igx::ColorRange, long long";
  // (the booleans up to the last that is set: the names the ABI tests instantiate)
  P.exprs = {std::string("igx::vec_sumfact<") + F.name + ", " + bool_name(geo) + ", " + std::to_string(L.ns) + (t.block ? ", false, true, true>" : (t.diagonal ? ", false, true>" : (t.action ? ", true>" : ">")))};
  std::shared_ptr<RtcInstance> K;
  if (int rc = rtc_instance(F, P, !compile_only, K)) return rc;
  if (compile_only) { done = true; return 0; }
  RtcVecArgs args; memset(&args, 0, sizeof(args));
  args.S = S; args.out = out; args.prm = params_of(s);
  int launches = 0;
  if (int rc = color_sweeps(s, SweepSpec(), [&](const ColorRange &cr) -> int {
    args.cr = cr; args.nelem = (long long)cr.count[0] * cr.count[1] * cr.count[2];
    HIPCK(module_launch(K->func[0], L.grid(args.nelem), L.threads, 0, g->stream, args));
    launches++;
    return 0;
  })) return rc;
  g->last_launches = launches;
  g->last_kernel = std::string("vec_sumfact<") + F.name + ">(hiprtc," + t.words + L.tail;
  done = true;
  return 0;
}

// ---- the Tangent of a nonlinear scalar struct on the pencil walk (gram_mfma.hpp: state_pencil<P, UserStruct>): the struct declares
// PENCIL_NFEAT / PENCIL_NC / pencil_coef / pencil_trial like FormCahnHilliard and FormBratu (forms.hpp); dof 1, dim 3, uniform degree
// 2 or 3 without a geometry, degree 2 on a mapped one (state_pencil_geo<2, RAT, UserStruct>), Jacobian / IJacobian drivers.
// Everything around the kernel is try_gram_mfma, as for form_pencil.
static int launch_state_rtc(IGX g, RtcForm &F, const SpaceDev &S, const OutDev &out, bool &done, bool compile_only = false) {
  done = false;
  const Space &s = g->s;
  const int deg = s.axis[0].p;
  if (s.dim != 3 || (deg != 2 && deg != 3)) return 0;
  // (the struct's constants are read from the loaded module: a compile-only check on a machine without a GPU takes the caller's word)
  if (!compile_only && (F.facts.pencil_nfeat <= 0 || F.facts.dof != 1 || F.facts.nscalar > 0 || F.facts.has_boundary || !s.env.state_pencil || (out.op != OP_JACOBIAN && out.op != OP_IJACOBIAN))) return 0;
  const bool geo = s.nsd != 0;
  if (geo && (s.nsd != 3 || deg != 2)) return 0;
  const bool pack = deg == 2 && s.env.p2_pack != 0;
  RtcProgram P; P.headers = RTC_GRAM; P.sig = kPencilSig;
  // p = 2: the packed-tile kernels, as for the built-in forms (IGX_P2_PACK=0: the layer-pair tiles, under another name)
  P.exprs = {pack ? (geo ? std::string("igx::state_pencil_geo_k<") + bool_name(s.rational) + ", " + F.name + ">"
                         : std::string("igx::state_pencil_k<") + F.name + ">")
                  : geo ? std::string("igx::state_pencil_geo<2, ") + bool_name(s.rational) + ", " + F.name + ">"
                        : std::string("igx::state_pencil<") + std::to_string(deg) + ", " + F.name + ">"};
  std::shared_ptr<RtcInstance> K;
  if (int rc = rtc_instance(F, P, !compile_only, K)) return rc;
  if (compile_only) { done = true; return 0; }
  PencilModule mod; mod.prm = params_of(s);
  mod.fn = K->func[0]; mod.name = F.name + ",hiprtc"; mod.state = true; mod.state_geo = geo;
  mod.extra_lds = pencil_state_bytes() + (geo ? pencil_sgeo_bytes() - pencil_geo_bytes() : 0);
  mod.pack = pack ? (geo ? 2 : 1) : 0;
  mod.flop_per_element = 2048.0 * F.facts.pencil_nfeat * (deg == 2 ? 7 * (pack ? 4 : 9) : 16 * 16);
  return try_gram_mfma(s, S, out, g->stream, false, g->last_kernel, g->last_launches, g_err, done, g->dom, zero_matrix_of(g), g->slab_done, &mod, g->face_done);
}

// ---- band rows by node layer (block_pencil.hpp) for a run-time struct: constant-coefficient multi-field forms (MAT_PAIR_MASK, 2 or 3
// fields, VEC_ZERO, first order, no atboundary branch), the conditions of bp_form_ok / block_pencil_covers with the struct's
// constants read from the module; colours, segments, first touch, boundary loads and the two-pass assembly are block_pencil_run
struct RtcBlockArgs { SpaceDev S; ParamsDev prm; OutDev out; BlockPencilArgs pa; };
static int launch_block_rtc(IGX g, RtcForm &F, const SpaceDev &S, const OutDev &out, bool &done, bool compile_only = false, int sys_only = -1) {
  done = false;
  const Space &s = g->s;
  if (s.dim != 3) return 0;
  if (!compile_only) {
    const int DOF = F.facts.dof;
    if (F.facts.npairs <= 0 || !F.facts.vec_zero || DOF < 2 || DOF > 3 || F.facts.order >= 2 || F.facts.shape_order >= 2 || F.facts.has_boundary || F.facts.nscalar > 0) return 0;
    if (!block_pencil_covers_space(s, S, out, DOF)) return 0;
  }
  const bool sysk = compile_only ? sys_only != 0 : out.op == OP_SYSTEM;
  RtcProgram P; P.headers = RTC_BLOCK; P.sig = "igx::SpaceDev, igx::ParamsDev, igx::OutDev, igx::BlockPencilArgs";
  P.exprs = {std::string("igx::block_pencil<") + F.name + ", 3, " + bool_name(sysk) + ">"};
  std::shared_ptr<RtcInstance> K;
  if (int rc = rtc_instance(F, P, !compile_only, K)) return rc;
  if (compile_only) { done = true; return 0; }
  const ParamsDev prm = params_of(s);
  hipStream_t stream = g->stream;
  int lrc = 0;
  const int rc = block_pencil_run(s, S, out, stream, g->last_kernel, g->last_launches, g_err, done, g->dom, zero_matrix_of(g), g->slab_done, F.facts.dof, F.facts.npairs,
                                  [&](bool, unsigned grid, size_t lds, const BlockPencilArgs &pa) {
                                    RtcBlockArgs a; memset(&a, 0, sizeof(a));
                                    a.S = S; a.prm = prm; a.out = out; a.pa = pa;
                                    if (lds > (size_t)160 * 1024 || module_launch(K->func[0], grid, 512, lds, stream, a) != hipSuccess) lrc = IGX_ERR_LIB;
                                  });
  if (rc == 0 && lrc) return fail(lrc, "block_pencil: launch of the run-time instantiation failed");
  if (rc == 0 && done) g->last_kernel = std::string("block_pencil<") + F.name + ">(hiprtc,mfma_f64_16x16x4,p=3,dof=" + char('0' + F.facts.dof) + ",band rows by node layer)";
  return rc;
}

static int rtc_generic_launch(IGX g, RtcForm &F, const SpaceDev &S, const OutDev &out);
// launch_generic (dispatch_unit.hip) with the form's constants read from the module instead of from a template parameter
// ---- band rows by node layer with point-dependent coefficients (band_pt.hpp) for a run-time struct: four fields, first order, the
// point coefficients separated from the basis functions (NCOEF, point_coef, mat_c; optionally mat_unit / BAND_NFEAT / BAND_NACC with
// their hooks, forms.hpp: FormNSVMS is the model); Matrix / Jacobian / IJacobian drivers.  The conditions of bpt_form_ok are checked
// on the constants read from the module; colours, segments, first touch and the two-pass assembly are band_pt_run.
struct RtcBandArgs { SpaceDev S; ParamsDev prm; OutDev out; BandArgs pa; };
static int launch_band_rtc(IGX g, RtcForm &F, const SpaceDev &S, const OutDev &out, bool &done, bool compile_only = false, int geo_only = -1) {
  done = false;
  const Space &s = g->s;
  if (s.dim != 3) return 0;
  if (!compile_only) {
    if (!F.facts.point_coef || F.facts.dof != 4 || F.facts.shape_order >= 2 || F.facts.has_boundary || F.facts.nscalar > 0 || F.facts.gram || (F.facts.mat_need & ~(NEED_U | NEED_G))) return 0;
    if (!band_pt_covers_space(s, S, out)) return 0;
  }
  const bool geo = compile_only ? (geo_only & 1) != 0 : s.nsd != 0, rat = compile_only ? (geo_only & 2) != 0 : s.rational != 0;
  const int deg = s.axis[0].p;
  if (deg != 2 && deg != 3) { if (compile_only) return fail(IGX_ERR_SUP, "band_pt needs degree 2 or 3"); return 0; }
  RtcProgram P; P.headers = RTC_BAND; P.sig = "igx::SpaceDev, igx::ParamsDev, igx::OutDev, igx::BandArgs"; P.meta = "igx_band_meta";      // (bpt_rec, bpt_products, the struct has its own band_params_ok)
  P.exprs = {std::string("igx::band_points<") + F.name + ", " + std::to_string(deg) + ">", std::string("igx::band_pt<") + F.name + ", " + bool_name(geo) + ", " + bool_name(rat) + ", " + std::to_string(deg) + ">"};
  P.before = "static_assert(igx::bpt_form_ok<" + F.name + ">(), \"band_pt: four fields, first order, NCOEF / point_coef / mat_c, no atboundary branch\");\n"
             "__device__ int igx_band_meta[4] = {igx::bpt_rec<" + F.name + ">(), igx::bpt_products<" + F.name + ">(), igx::band_nacc_of<" + F.name + ">::own ? 1 : 0, 0};\n"
             // the struct's own guard on the parameters (a struct with BAND_NACC hooks declares band_params_ok __host__ __device__)
             "__device__ double igx_band_prm[igx::MAXPARAM]; __device__ int igx_band_ok;\n"
             "template <class F> __device__ int igx_band_guard_of(const double *prm) { if constexpr (igx::band_nacc_of<F>::own) return F::band_params_ok(prm) ? 1 : 0; else return 1; }\n"
             "extern \"C\" __global__ void igx_band_guard() { igx_band_ok = igx_band_guard_of<" + F.name + ">(igx_band_prm); }\n";
  auto it = F.instances.find(rtc_key(P));
  if (it != F.instances.end() && it->second->failed && !compile_only && g->kernel_choice == 0) { g->rtc_note = it->second->why; return 0; }
  std::shared_ptr<RtcInstance> K;
  if (int rc = rtc_instance(F, P, !compile_only, K)) {
    // Under the automatic choice a struct whose band-row instantiation does not compile (the usual reason: a band_params_ok
    // that is not __host__ __device__, include/petiga_amd.h) is a struct the band-row kernel does not cover: the feature kernel
    // takes the assembly and the kernel name carries the reason.  Asked for by name (IGXSetKernel(4), IGXCheckFormSource) it fails.
    // (An entry with code is one that compiled and did not load: an error under every choice.)
    if (!K->code.empty() || compile_only || g->kernel_choice != 0) return rc;
    K->failed = true;
    K->why = "band_pt<" + F.name + "> did not compile (is band_params_ok declared __host__ __device__?): " + g_err.substr(0, 400);
    F.instances[rtc_key(P)] = K; g->rtc_note = K->why;
    return 0;
  }
  if (compile_only) { done = true; return 0; }
  const ParamsDev prm = params_of(s);
  hipStream_t stream = g->stream;
  // The struct's guard on its parameters, as the built-in path has it (band_pt.hpp: Form::band_params_ok): band_coef / band_finish
  // may divide by a parameter (FormNSVMS: 1 / nu), and a struct that says no stays on the feature kernel.  Evaluated by the
  // module's one-lane kernel whenever the parameters differ from the ones it was last asked about.
  if (K->meta[2] != 0) {
    const std::vector<double> now(prm.v, prm.v + MAXPARAM);
    if (!K->guard_known || now != K->guard_prm) {
      hipFunction_t gf = nullptr; hipDeviceptr_t pp = nullptr, po = nullptr; size_t n = 0; int ok = 0;
      HIPCK(hipModuleGetFunction(&gf, K->module, "igx_band_guard"));
      HIPCK(hipModuleGetGlobal(&pp, &n, K->module, "igx_band_prm"));
      if (n != sizeof(prm.v)) return fail(IGX_ERR_LIB, "unexpected igx_band_prm size");
      HIPCK(hipModuleGetGlobal(&po, &n, K->module, "igx_band_ok"));
      HIPCK(hipMemcpyAsync(pp, prm.v, sizeof(prm.v), hipMemcpyHostToDevice, stream));
      HIPCK(hipModuleLaunchKernel(gf, 1, 1, 1, 1, 1, 1, 0, stream, nullptr, nullptr));
      HIPCK(hipMemcpyAsync(&ok, po, sizeof(int), hipMemcpyDeviceToHost, stream));
      HIPCK(hipStreamSynchronize(stream));
      K->guard_known = true; K->guard_ok = ok != 0; K->guard_prm = now;
    }
    if (!K->guard_ok) return 0;       // done stays false: the caller goes on to the feature kernel
  }
  int lrc = 0;
  const int rc = band_pt_run(s, S, out, stream, g->last_kernel, g->last_launches, g_err, done, g->dom, zero_matrix_of(g), g->slab_done, K->meta[0], K->meta[1],
                             [&](bool points, unsigned grid, size_t lds, bool, bool, int, const BandArgs &pa) {
                               RtcBandArgs a; memset(&a, 0, sizeof(a));
                               a.S = S; a.prm = prm; a.out = out; a.pa = pa;
                               if (module_launch(K->func[points ? 0 : 1], grid, 256, lds, stream, a) != hipSuccess) lrc = IGX_ERR_LIB;
                             });
  if (rc == 0 && lrc) return fail(lrc, "band_pt: launch of the run-time instantiation failed");
  if (rc == 0 && done) g->last_kernel = std::string("band_pt<") + F.name + ">(hiprtc,mfma_f64_16x16x4,p=" + std::to_string(deg) + ",dof=4,band rows by node layer,point records)";
  return rc;
}

// mode: a matrix-free operator (compute_matfree), or VECTOR for the drivers that assemble
static int launch_generic_rtc(IGX g, const SpaceDev &S, const OutDev &out, VsMode mode) {
  Space &s = g->s;
  g->rtc_note.clear();
  if (!g->rtc || g->rtc->dim != s.dim) {
    std::shared_ptr<RtcForm> f;
    if (int rc = rtc_compile(g, g->rtc_source, g->rtc_name, s.dim, f)) return rc;
    g->rtc = f;
  }
  RtcForm &F = *g->rtc;
  if (int rc = rtc_load(g, F)) return rc;
  if (mode != VsMode::VECTOR) {      // the matrix-free operators: vec_sumfact's instantiation of the struct or a refusal, as for the built-in forms
    if (const MfRefusal r = matfree_refusal(s, g->kernel_choice, mode, &F.facts, MfCaller::STRUCT)) return fail(r.code, r.msg);
    const VsTraits t = vs_traits(mode);
    bool done = false;
    if (int rc = launch_vecsf_rtc(g, F, S, out, done, t.batch ? VsMode::ACTION : mode)) return rc;      // (a block's columns come one by one)
    return done ? 0 : fail(IGX_ERR_PLIB, std::string("vec_sumfact did not take a ") + (t.block ? "matrix block diagonal" : t.diagonal ? "matrix diagonal" : "matrix action") + " it covers");
  }
  if (F.facts.nscalar > 0) return fail(IGX_ERR_SUP, "a struct with NSCALAR is a functional: IGXComputeScalarSource");
  if (s.dof != F.facts.dof) return fail(IGX_ERR_ARG_WRONG, "form does not match the number of fields (dof)");
  // a struct of ORDER 3, or one that reads the property array / the point's shape table / third derivatives of the state: the general kernel (as launch_generic)
  if (F.facts.order >= 3 || (F.facts.need & (NEED_PROP | NEED_D3U | NEED_MAPX)) || (s.nsd && s.nsd != s.dim)) {      // (... or a geometry with nsd != dim)
    if (g->kernel_choice != 0 && g->kernel_choice != 1) return fail(IGX_ERR_SUP, "a form of order 3 or one that reads the property array runs on the general kernel only");
    if ((F.facts.need & NEED_PROP) && !S.npd) return fail(IGX_ERR_ARG_WRONGSTATE, "No property set");
    if ((F.facts.need & NEED_MAPX) && !s.nsd) return fail(IGX_ERR_ARG_WRONGSTATE, "No geometry set");
    if (F.facts.order >= 3 && s.order < 3) return fail(IGX_ERR_ARG_WRONGSTATE, "the form reads third derivatives (p->shape[3]): call IGASetOrder(iga,3) first");
    if (g->zero_matrix) g->zero_matrix();
    return rtc_generic_launch(g, F, S, out);
  }
  if (g->kernel_choice == 0) {   // vector-only drivers in 3-D: sum factorisation both ways (vec_sumfact.hpp)
    bool done = false;
    if (int rc = launch_vecsf_rtc(g, F, S, out, done)) return rc;
    if (done) return 0;
  }
  if ((g->kernel_choice == 0 && s.axis[0].p == 3) || g->kernel_choice == 4) {   // four-field structs with separated point coefficients: band rows by node layer (p = 2 on request)
    bool done = false;
    if (int rc = launch_band_rtc(g, F, S, out, done)) return rc;
    if (done) return 0;
  }
  if (g->kernel_choice == 0 || g->kernel_choice == 4) {   // constant-coefficient multi-field structs: band rows by node layer
    bool done = false;
    if (int rc = launch_block_rtc(g, F, S, out, done)) return rc;
    if (done) return 0;
    if (g->kernel_choice == 4) return fail(IGX_ERR_SUP, "the band-row kernels do not cover this run-time form / configuration (block_pencil: MAT_PAIR_MASK, 2 or 3 fields, VEC_ZERO, 3-D, p = 3, identity geometry, System / Matrix driver; band_pt: 4 fields, NCOEF / point_coef / mat_c, 3-D, p = 3, matrix-only driver)");
  }
  if (g->kernel_choice == 0 || g->kernel_choice == 2) {   // Tangents of scalar structs that opted in: the pencil walk with the state
    bool done = false;
    if (int rc = launch_state_rtc(g, F, S, out, done)) return rc;
    if (done) return 0;
  }
  if (g->kernel_choice == 0 || g->kernel_choice == 2) {   // scalar symmetric gradient forms: the pencil walk (combine before write)
    bool done = false;
    if (int rc = launch_pencil_rtc(g, F, S, out, done)) return rc;
    if (done) return 0;
    if (g->kernel_choice == 2) return fail(IGX_ERR_SUP, "the pencil kernel does not cover this run-time form / configuration (dof 1, gradients only, MAT_SYMMETRIC, VEC_TEST_MASK = 1, dim 3, p = 2 or 3)");
  }
  if (g->kernel_choice != 1) {   // the dense contraction on the matrix cores when the case is covered (as launch_generic does)
    bool done = false;
    if (int rc = launch_feature_rtc(g, F, S, out, done)) return rc;
    if (done) return 0;
    if (g->kernel_choice == 3) return fail(IGX_ERR_SUP, "the feature-GEMM kernel does not cover this case (needs dim >= 2 and nen <= 64; nen <= 128 with dof <= 2 and nen <= 256 with dof 1 in 3-D, no MAT_PAIR_MASK there)");
  }
  if (g->zero_matrix) g->zero_matrix();
  return rtc_generic_launch(g, F, S, out);
}

// the point-form kernel of a run-time struct: matrix / vector forms (coloured sweeps + boundary-form passes) and functionals
// (NSCALAR > 0: one sweep, a row of partial sums per element, as launch_generic does for the built-in ones)
static int rtc_generic_launch(IGX g, RtcForm &F, const SpaceDev &S, const OutDev &out) {
  Space &s = g->s;
  const size_t lds_limit = 64 * 1024;   // as launch_generic: beyond it Phi goes to an HBM slice and two workgroups share a CU
  const GenericCarve gc = carve_generic(F.facts, s, S.npd, out.op, lds_limit);
  if (gc.lds_bytes > lds_limit) return fail(IGX_ERR_SUP, "element work set of the run-time form exceeds 64 KiB of LDS");
  RtcArgs args; memset(&args, 0, sizeof(args));
  args.S = S; args.out = out; args.cv = gc.cv; args.phi_stride = gc.phi_doubles; args.prm = params_of(s);
  // matrix / vector forms: coloured sweeps + boundary-form passes; a struct with an atboundary branch supplies bmat / bvec
  // (HAS_BOUNDARY), any other is integrated over the face
  if (int rc = sweep_generic(g, g_err, gc, F.facts.nscalar > 0, [&](const ColorRange &cr, int bid, int64_t elem_base, size_t nblocks) -> int {
        args.cr = cr; args.phi_global = g->scratch.as<double>(); args.out.bid = bid; args.out.elem_base = elem_base;
        HIPCK(module_launch(F.func, (unsigned)nblocks, 256, gc.lds_bytes, g->stream, args));
        return 0;
      })) return rc;
  g->last_kernel = std::string("generic_assemble<") + F.name + "> (hiprtc," + (gc.phi_in_lds ? "phi=LDS" : "phi=HBM") + ")";
  return 0;
}

extern "C" int IGXSetFormSource(IGX g, const char *source, const char *struct_name, const double params[], int nparams) {
  NEEDIGA(g);
  if (!source || !struct_name || !*struct_name) return fail(IGX_ERR_ARG_WRONG, "null source / struct name");
  if (nparams < 0 || nparams > MAXPARAM || (nparams && !params)) return fail(IGX_ERR_ARG_OUTOFRANGE, "bad parameter list");
  if (g->s.dim < 1) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGASetDim() first");
  std::shared_ptr<RtcForm> f;
  if (int rc = rtc_compile(g, source, struct_name, g->s.dim, f)) return rc;     // compile errors surface here, with the log
  g->rtc = f; g->rtc_source = source; g->rtc_name = struct_name;
  g->s.form = IGX_FORM_SOURCE; g->s.params.assign(params ? params : nullptr, params ? params + nparams : nullptr);
  return 0;
}

// IGAComputeScalar (src/petigacomp.c:35-98) with the user's point functional given as source: a struct with DOF, ORDER, NEED,
// NSCALAR = n and scalar(p, S) -- the un-weighted integrand values at a point (IGAFormScalar, include/petiga.h:188-191); the
// engine multiplies by JW and sums over the rank's elements and, for visited faces, over their boundary passes (p.atboundary).
extern "C" int IGXComputeScalarSource(IGX g, IGXVec U, const char *source, const char *struct_name, const double params[], int nparams, int n, double S[]) {
  NEEDIGA(g);
  if (!source || !struct_name || !*struct_name) return fail(IGX_ERR_ARG_WRONG, "null source / struct name");
  if (!S || n < 1) return fail(IGX_ERR_ARG_WRONG, "null result array");
  if (nparams < 0 || nparams > MAXPARAM || (nparams && !params)) return fail(IGX_ERR_ARG_OUTOFRANGE, "bad parameter list");
  if (int rc = ensure_device(g)) return rc;
  Space &s = g->s;
  if (U && U->iga != g) return fail(IGX_ERR_ARG_WRONG, "state vector created by another IGX");
  // (one compiled functional is kept per IGX: the same source and struct are not compiled twice)
  if (!g->rtc_scalar || g->rtc_scalar->source != source || g->rtc_scalar->name != struct_name || g->rtc_scalar->dim != s.dim) {
    std::shared_ptr<RtcForm> f;
    if (int rc = rtc_compile(g, source, struct_name, s.dim, f)) return rc;
    g->rtc_scalar = f;
  }
  RtcForm &F = *g->rtc_scalar;
  if (int rc = rtc_load(g, F)) return rc;
  const int ns = F.facts.nscalar;
  if (ns < 1) return fail(IGX_ERR_ARG_WRONG, "the struct is not a functional (no NSCALAR)");
  if (n != ns) return fail(IGX_ERR_ARG_WRONG, "this functional returns " + std::to_string(ns) + " scalars");
  if (F.facts.dof != s.dof) return fail(IGX_ERR_ARG_WRONG, "functional does not match the number of fields (dof)");
  if ((F.facts.need & (NEED_U | NEED_GU | NEED_HU)) && !U) return fail(IGX_ERR_ARG_WRONG, "the functional reads the state: null vector");
  return reduce_scalars(g, ns, U, params, nparams, [&](const SpaceDev &Sd, const OutDev &out) { return rtc_generic_launch(g, F, Sd, out); }, S);
}

// the values of `gram` beyond 0 / 1 (the feature kernel without / with the Gram path), as include/petiga_amd.h documents them
enum RtcCheckKind { CHECK_PENCIL = 2, CHECK_VECSF = 3, CHECK_STATE = 4, CHECK_BLOCK = 5, CHECK_BAND = 6, CHECK_ACTION = 7, CHECK_DIAGONAL = 8, CHECK_BLOCK_DIAGONAL = 9 };

// Compile-only check of a run-time form against the kernels the drivers would launch for the axes set so far (no GPU needed):
// the point-form kernel was compiled by IGXSetFormSource; this adds the matrix-core kernel (feature_mfma.hpp) in the wave
// layout of the current degree, for the matrix drivers (with_matrix != 0) or the vector-only ones.
extern "C" int IGXCheckFormSource(IGX g, int with_matrix, int gram) {
  NEEDIGA(g);
  if (g->s.form != IGX_FORM_SOURCE || !g->rtc) return fail(IGX_ERR_ARG_WRONGSTATE, "Must call IGXSetFormSource() first");
  const Space &s = g->s;
  RtcForm &F = *g->rtc;
  bool done = false; OutDev o; memset(&o, 0, sizeof(o)); SpaceDev Sd; memset(&Sd, 0, sizeof(Sd));      // (compile only: the launchers read neither)
  if (gram == CHECK_BAND) {           // band_points + band_pt of a four-field struct with separated point coefficients: compile only (no geometry and NURBS)
    if (int rc = launch_band_rtc(g, F, Sd, o, done, true, 0)) return rc;
    if (!done) return fail(IGX_ERR_SUP, "band_pt needs dim 3");
    return launch_band_rtc(g, F, Sd, o, done, true, 3);
  }
  if (gram == CHECK_BLOCK) {           // block_pencil of a constant-coefficient multi-field struct (System and Matrix driver): compile only
    if (int rc = launch_block_rtc(g, F, Sd, o, done, true, 1)) return rc;
    if (!done) return fail(IGX_ERR_SUP, "block_pencil needs dim 3");
    return launch_block_rtc(g, F, Sd, o, done, true, 0);
  }
  if (gram == CHECK_STATE) {           // state_pencil of a struct with the PENCIL_* hooks, for the current degree: compile only
    if (int rc = launch_state_rtc(g, F, Sd, o, done, true)) return rc;
    return done ? 0 : fail(IGX_ERR_SUP, "state_pencil needs dim 3, dof 1, degree 2 or 3 (2 on a mapped geometry) and a struct with PENCIL_NFEAT / PENCIL_NC / pencil_coef / pencil_trial");
  }
  if (gram >= CHECK_ACTION && gram <= CHECK_BLOCK_DIAGONAL) {      // ... and its ACTION / DIAGONAL / DIAGONAL with BLOCK instantiation (IGXCompute*Action, *Diagonal, *BlockDiagonal of the struct) for the
    // layout the driver would launch: compile only, refused where the driver would refuse.  (The struct's constants are read from the loaded
    // module; without a GPU the kernel's static_assert names the cause.)
    const VsMode mode = gram == CHECK_ACTION ? VsMode::ACTION : gram == CHECK_DIAGONAL ? VsMode::DIAGONAL : VsMode::BLOCK_DIAGONAL;
    if (const MfRefusal r = matfree_refusal(s, g->kernel_choice, mode, gram != CHECK_ACTION && F.func ? &F.facts : nullptr, MfCaller::CHECK)) return fail(r.code, r.msg);
    return launch_vecsf_rtc(g, F, Sd, o, done, mode, true);
  }
  if (gram == CHECK_VECSF) {           // the sum-factorised vector kernel (vec_sumfact) of the struct, with and without a geometry: compile only
    if (s.dim != 3) return fail(IGX_ERR_SUP, "the sum-factorised vector kernel needs dim 3");
    return launch_vecsf_rtc(g, F, Sd, o, done, VsMode::VECTOR, true);
  }
  if (gram == CHECK_PENCIL) {           // the pencil walk's instantiation (form_pencil) for the current degree / geometry: compile only
    if (s.dim != 3 || (s.axis[0].p != 2 && s.axis[0].p != 3)) return fail(IGX_ERR_SUP, "the pencil walk needs dim 3 and degree 2 or 3");
    if (int rc = launch_pencil_rtc(g, F, Sd, o, done, true, 1)) return rc;      // System driver
    return launch_pencil_rtc(g, F, Sd, o, done, true, 0);                        // Matrix driver
  }
  if (s.dim < 2) return 0;   // dim 1: the point-form kernel only
  int NE = 1;
  for (int d = 0; d < s.dim; ++d) { if (s.axis[d].p < 1) return fail(IGX_ERR_ARG_WRONGSTATE, "set the axes (degrees) first"); NE *= s.axis[d].p + 1; }
  if (NE > 256 || (NE > 64 && (s.dim != 3 || gram || s.dof > 2)) || (NE > 128 && s.dof > 1)) return 0;
  int TA, NW, DOFI; rtc_feature_layout(NE, s.dof, gram != 0, with_matrix != 0, TA, NW, DOFI);
  std::shared_ptr<RtcInstance> K;
  return rtc_feature_module(F, s.dim, s.dof, TA, NW, DOFI, with_matrix != 0, false, K);
}
