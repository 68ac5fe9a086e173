// engine_objects.hpp -- what every translation unit of the library's device side shares: the last-error slot, the objects behind the C
// ABI's handles and the entry points that cross units.  The main unit (engine.hip: C ABI, set-up, drivers, the Gram walks, the loops) and
// the dispatch units (dispatch_unit.hip: the element-kernel instantiations of one dimension / form group) include it behind their kernel
// headers; the host headers of the main unit (exchange.hpp ... mat_ops_host.hpp) may use what stands here and what their own comments name.
#pragma once
#include <hip/hip_runtime.h>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>
#include "igx.hpp"
#include "first_touch.hpp"      // (DomInfo)

using namespace igx;

// The last-error text is one object for all units.
inline std::string &igx_err_slot() { static thread_local std::string e; return e; }
#define g_err igx_err_slot()
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
constexpr int IGX_NOT_MINE = -12345;    // a dispatch unit's answer for a form of another group
#define HIPCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(IGX_ERR_LIB, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

// ------------------------------------------------------------------ objects
struct DevBuf {
  void *p = nullptr; size_t bytes = 0;
  DevBuf() = default;
  // owns its allocation: movable, not copyable (a std::vector<DevBuf> that grows must MOVE its elements -- copied, the old elements'
  // destructors freed the memory the new ones pointed to: the exchange buffers of a rank whose refresh and reduction lists differ in
  // length, i.e. 4 and 8 ranks with a nonlinear form, before round 4)
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { if (p) (void)hipFree(p); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t n) { if (p) { (void)hipFree(p); p = nullptr; } bytes = n; if (!n) return 0; return hipMalloc(&p, n) == hipSuccess ? 0 : 1; }
  template <class T> int upload(const std::vector<T> &v) {
    if (alloc(v.size() * sizeof(T))) return 1;
    if (v.empty()) return 0;
    return hipMemcpy(p, v.data(), bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : 1;
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

struct AxisBufs { DevBuf tab, w, J, pt, off, rowmap, rcnt, P, rcol, prefix, bnd, knots, elof; };   // knots, elof: the knot vector and the element of every knot span (probe.hpp)


struct IgxComm;
struct RtcForm;
struct KrylovState;
struct NewtonState;
struct TimeStepState;
struct BlockVecState;
struct EigenState;
// IGXFastDiagSetUp's host result and the device copies IGXFastDiagApply makes of it at its first call
struct FastDiagState {
  FastDiag h;
  bool on_device = false;
  DevBuf tf[3][4], tb[3][4], s[3][4], count[3];     // [axis][combo]: forward table T[j][i] = U[j - first][i], backward T[i][j], beta lambda; [axis]: elements per function
  DevBuf work[2];                                   // two ping-pong buffers of the local vector's size
};
struct _p_IGX {
  Space s;
  bool on_device = false;
  AxisBufs ab[3];
  DevBuf X, W, A, fixtable, errflag, scratch;
  hipStream_t stream = nullptr;
  int kernel_choice = 0;
  _p_IGX() { s.env = read_env_switches(); kernel_choice = s.env.kernel; }   // environment switches are read here, once per IGX
  std::string last_kernel = "none";
  std::string rtc_note;           // why a run-time form was kept off a kernel it asked for (appended to the kernel name)
  bool timing = false;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // step begin, kernels begin/end, step end, dominant kernel begin/end
  double last_total_ms = 0, last_kernel_ms = 0; int last_launches = 0;
  std::function<void()> zero_matrix;   // MatZeroEntries of the running IGXCompute*, called by the kernel path that needs it
  std::function<void()> slab_done;     // set during an assembly with a communicator: marks "upper face of axis 2 assembled" on the engine stream
  DevBuf partials, dbgbuf, clkbuf;   // IGXComputeScalar: per-element partial sums + reduction stages
  DevBuf nsingular;                  // IGXBlockDiagonalInvert: the count of singular blocks
  DevBuf patch3_counters;            // the p = 3 patch walk's ticket counters, one per colour launch (the rows walk, gram_rows3.hpp, takes the first); zeroed on `stream` ahead of every assembly's launches (pencil_launch.hpp)
  DomInfo dom;
  int64_t nbrows = 0, nblocks = 0;
  std::shared_ptr<IgxComm> comm;   // transport of the ghost-row exchange (comm.hpp)
  // recorded on the engine stream when the elements next to the upper face of axis 2 have been assembled (pencil kernel, several
  // ranks): IGXReduceGhostRows starts the messages of that face behind it, under the launches of the other elements
  // slab_valid: bit 0 = the mark of axis 2 (slab_ev), bit 1 = axis 1, bit 2 = axis 0 (face_ev[1], face_ev[0]: the pencil walk's three passes)
  hipEvent_t slab_ev = nullptr; int slab_valid = 0; IGXMat slab_A = nullptr; IGXVec slab_b = nullptr;
  hipEvent_t face_ev[2] = {nullptr, nullptr};
  std::function<void(int)> face_done;  // marks "upper face of axis 1 / 0 assembled" (pencil_launch.hpp)
  std::shared_ptr<RtcForm> rtc; std::string rtc_source, rtc_name;   // run-time compiled user form (rtc.hpp)
  std::shared_ptr<RtcForm> rtc_scalar;                              // ... and the last user functional (IGXComputeScalarSource)
  std::shared_ptr<FastDiagState> fd;                                // fast diagonalisation (IGXFastDiagSetUp; fast_diag.hpp)
  DevBuf krscal;                                                    // IGXVecDot / IGXSolve: the slabs of partial sums, the record and the device scalars (krylov.hpp)
  std::shared_ptr<KrylovState> krylov;                              // IGXSolve's work vectors and preconditioner storage, kept between solves
  std::shared_ptr<NewtonState> newton;                              // IGXSolveNonlinear's work vectors, kept between solves
  std::shared_ptr<TimeStepState> timestep;                          // IGXTimeStep's work vectors, U_{n-1} and h_{n-1}, kept between calls
  std::shared_ptr<BlockVecState> blockvec;                          // IGXVecMDot / IGXVecMAXPY: the slab of partial tiles, the coefficient ring and the record (block_vec.hpp)
  std::shared_ptr<EigenState> eigen;                                // IGXEigenSolve's work vectors, kept between solves
  std::string self_timed;                                           // the value of last_kernel for which the call itself stored last_total_ms / last_kernel_ms (a solve loop; a probe of no points): IGXGetLastTiming keeps them
  int batched_actions = 0;                                          // IGXSetBatchedActions: IGXEigenSolve applies this IGX's action to its blocks in one call
  unsigned long long setup_gen = 0;                               // counts IGXSetUp calls: a probe made before the last one is stale (IGXProbeCreate)
  bool current(unsigned long long gen) const { return s.setup && gen == setup_gen; }   // the question every object made from an IGX asks: is it set up, and by the set-up I recorded?
};

struct _p_IGXMat {
  IGX iga; int bs; int64_t nbrows, nblocks;
  DevBuf browptr, bcolidx, val;
  DevBuf coo_i, coo_j;     // coordinate lists kept on the device for the hand-back (IGXMatGetCOODevice), or empty
  unsigned long long gen = 0;   // the IGX's setup_gen at IGXCreateMat: the pattern is that set-up's (IGXMatMult and its kin refuse a matrix of an earlier one)
};
struct _p_IGXVec { IGX iga; int64_t n; DevBuf a; };
// (KrylovState, NewtonState, TimeStepState, BlockVecState, EigenState: solve_loops.hpp, the main unit)

#define NEEDIGA(g) do { if (!(g)) return fail(IGX_ERR_ARG_WRONG, "null IGX"); } while (0)
#define AXISCK(g, i) do { NEEDIGA(g); if ((i) < 0 || (i) >= 3) return fail(IGX_ERR_ARG_OUTOFRANGE, "Index must be in range [0,2]"); } while (0)

// the dispatch units' entry points: kernel instantiations live there (one unit per dimension; three form groups for dim 3)
#define IGX_TU_ENTRIES(d, gr) \
  int igx_tu_dispatch(std::integral_constant<int, d>, std::integral_constant<int, gr>, IGX g, const SpaceDev &S, const OutDev &out); \
  int igx_tu_matfree(std::integral_constant<int, d>, std::integral_constant<int, gr>, IGX g, const SpaceDev &S, const OutDev &out, VsMode mode, const ActionCols *cols);
IGX_TU_ENTRIES(1, -1) IGX_TU_ENTRIES(2, -1) IGX_TU_ENTRIES(3, 0) IGX_TU_ENTRIES(3, 1) IGX_TU_ENTRIES(3, 2)
#undef IGX_TU_ENTRIES
int igx_tu_scalar(std::integral_constant<int, 1>, IGX g, int kind, const SpaceDev &S, const OutDev &out, int order);
int igx_tu_scalar(std::integral_constant<int, 2>, IGX g, int kind, const SpaceDev &S, const OutDev &out, int order);
int igx_tu_scalar(std::integral_constant<int, 3>, IGX g, int kind, const SpaceDev &S, const OutDev &out, int order);
