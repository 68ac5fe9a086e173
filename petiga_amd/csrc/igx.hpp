// igx.hpp -- internal types of libpetiga_amd (host discretisation + device descriptors).
// Reference citations are file:line of dalcinl/PetIGA @ 2025-04-04.
#pragma once
// IGX_RTC: this header is also the prelude of run-time compiled user forms (rtc.hpp): hiprtc has no standard library and no
// hip_runtime.h to include, so the host part is skipped and the few fixed-width types are spelled out.
#ifndef IGX_RTC
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/petiga_amd.h"
#else
typedef long long int64_t;
typedef int int32_t;
typedef unsigned long size_t;
#define IGX_ERR_USER 83
#define IGX_ACTION_MAXCOLS 16
#endif

namespace igx {

// Experiment hooks (cycle stamps, scatter / MFMA phase switches) are compiled into the kernels only with -DIGX_DEBUG.
#ifdef IGX_DEBUG
constexpr bool kDebug = true;
#else
constexpr bool kDebug = false;
#endif

#ifndef IGX_RTC
// Environment switches, read once when an IGX is created (IGXCreate / IGXCreateFromTables)
struct EnvSwitches {
  int kernel = 0;            // IGX_KERNEL=0..4 presets IGXSetKernel (the parity suite runs every case under two kernel families)
  int walk_axis = 0;         // IGX_WALK_AXIS: preferred walk axis of the pencil kernel
  int nseg = 0;              // IGX_NSEG: segments per pencil (0 = model)
  int clock_probe = 0;       // IGX_CLOCK_PROBE: the pencil kernel records shader-clock ticks against the 100 MHz wall clock (IGXGetClockProbe)
  int overlap = -1;          // IGX_OVERLAP: 0 = no face-first passes, the ghost-row exchange starts after the last launch; 1 = always; 2 = the face of axis 2
                             // alone (round 3); unset (-1): the pencil walk decides by cost against the size of the faces, the other kernels make their pass
  int fuse_groups = 1;       // IGX_FUSE_GROUPS=0: one launch per group of row fields again (NS-VMS p=3; experiment switch)
  int no_first_touch = 0;    // IGX_NO_FIRST_TOUCH: MatZeroEntries + read-modify-write everywhere (no meaning for the p = 3 rows walk, gram_rows3.hpp:
                             // it stores every entry once and reads none)
  int feature_lds_kb = 0;    // IGX_FEATURE_LDS_KB: LDS target of the feature kernel
  int block_pencil = 1;      // IGX_BLOCK_PENCIL=0: constant-coefficient multi-field forms stay on the feature kernel (block_pencil.hpp)
  int no_vec_pairs = 0;      // IGX_NO_VEC_PAIRS=1: vec_sumfact keeps one element per wavefront at p <= 2
  int state_pencil = 1;      // IGX_STATE_PENCIL=0: Tangents of scalar forms stay on the feature kernel (gram_mfma.hpp: state_pencil)
  int vec_sumfact = 1;       // IGX_VEC_SUMFACT=0: the vector-only drivers stay on the feature kernel (vec_sumfact.hpp)
  int free_run = -1;         // IGX_FREE_RUN=0/1: the pencil walk with / without its s_barrier ping-pong (-1: the launcher's choice)
  int p2_pack = 1;           // IGX_P2_PACK=0: the p = 2 walks keep one tile per pair of node layers (round 4) instead of the packed tiles
  int band_prio = 0, band_rmw_prio = 0;      // IGX_BAND_PRIO=k: band_pt raises the priority of a workgroup's first k layers; IGX_BAND_RMW_PRIO=1: ... of its read-add-writes
  int patch = 1;             // IGX_PATCH=0: the p = 2 Gram walk keeps one pencil and one window per wavefront (bit-repeatable) instead of the patches of
                             // 4 x 3 pencils with one shared window (gram_patch.hpp, round 6: + 23 % on config 2, the order of its LDS adds is not fixed)
  int small_wpb = 1;         // IGX_SMALL_WPB=0: launches that fill less than half the CUs keep eight-wavefront workgroups (pencil_launch.hpp, round 6)
  int patch3 = 1;            // IGX_PATCH3: the p = 3 Gram walk on the identity geometry -- 0 the pencil walk, 1 the patch walk where it pays (default),
                             // 2 the patch walk wherever it covers the configuration (gram_patch3.hpp, round 8)
  int patch3_persist = 1;    // IGX_PATCH3_PERSIST=0: the p = 3 patch walk launches one workgroup per (segment, patch) item, as before round 12; 1 (default):
                             // resident workgroups take their items from a counter by ticket (gram_patch3.hpp)
  int patch3_grid = 0;       // IGX_PATCH3_GRID=n: the ticket launch is n workgroups (test and experiment knob); 0: as many as the device holds, at most the items
  int patch3_order = 1;      // IGX_PATCH3_ORDER=0: tickets take the items in their natural order; 1 (default): the patches on a face of axis 1 or 2 first
  int rows3 = 1;             // IGX_ROWS3: the p = 3 Gram matrix gathered by rows, each entry stored once (gram_rows3.hpp, round 13) -- 0 never, 1 where it pays
                             // (default), 2 wherever it covers the configuration.  Chosen under IGX_PATCH3=1 only: IGX_PATCH3=0 is the pencil walk, 2 the patch walk
  int rows3_grid = 0;        // IGX_ROWS3_GRID=n: the rows walk is a ticket launch of n workgroups (test and experiment knob); 0: as many as the device holds
  int rows3_stage = 1;       // IGX_ROWS3_STAGE: the rows walk's full layers of regular tiles leave through LDS as contiguous spans (round 14) -- 0 never (a run
                             // lane stores its run), 1 where it pays (default), 2 wherever the rows walk runs
  int patch_state = 0;       // IGX_PATCH_STATE=1: the Tangent of a p = 2 state form walks patches of 4 x 2 pencils (state_patch_p2) instead of state_pencil_k
  int fuse_resid = 0;        // IGX_FUSE_RESID=1: IGXComputeIFunctionIJacobian takes the fused walk (state_pencil_kr) where it exists; default: the two
                             // drivers one after the other -- measured in round 6: the fused launch costs 2.5 ms more than the Tangent's, the
                             // Residual's own pass 2.1 ms per launch
  int gram_sumfact = 1;      // IGX_GRAM_SUMFACT=0: the p = 3 Gram walk on the identity geometry keeps its 480 MFMAs per element (pencil_mfma) instead of
                             // the sum-factorised walk-axis contraction (pencil_mfma_sf)
  int matmult_index = -1;    // IGX_MATMULT_INDEX: where IGXMatMult takes the column of an entry from -- 0 the per-axis tables (the closed form of k_bcolidx),
                             // 1 the matrix's bcolidx; unset (-1): the faster one as measured (profiles/matmult.txt) -- the tables where a sub-group takes a
                             // row (at most 128 doubles), bcolidx where a wavefront does (mat_ops.hpp)
  int combine = -1;          // IGX_COMBINE: element bricks of the feature kernel (-1 = automatic, 0 = one element per workgroup)
  int debug_feature = 0, debug_noflush = 0, debug_timing = 0, debug_noprio = 0;   // only honoured by -DIGX_DEBUG builds
};
EnvSwitches read_env_switches();

// ------------------------------------------------------------------ host discretisation
struct Axis {                 // struct _n_IGAAxis, include/petiga.h:80-96
  int p = 0, m = 0, periodic = 0, nel = 0, nnp = 0;
  std::vector<double> U;
  std::vector<int> span;
};

struct Basis1D {              // struct _n_IGABasis, include/petiga.h:122-141
  int nel = 0, nqp = 0, nen = 0;
  std::vector<int> offset;
  std::vector<double> detJac, weight, point, value;   // value: [nel][nqp][nen][5]
  std::vector<double> bnd_value[2];                   // [nen][5] at the first / last knot (bnd_value, include/petiga.h:136)
  double bnd_point[2] = {0, 0};
};

struct BC {                   // struct _IGAFormBC, include/petiga.h:220-225
  int count = 0;
  int field[64];
  double value[64];
};

struct Rule1D {               // struct _n_IGARule, include/petiga.h:91-99 (the size lives in Space::rule_nqp)
  int type = 0;               // IGXRuleType
  std::vector<double> x, w;   // IGX_RULE_USER: the rule on [-1, 1]
};

int  gauss_legendre(int q, double *X, double *W);
int  gauss_lobatto(int q, double *X, double *W);
int  rule_setup(const Rule1D &r, int nqp, double *X, double *W, std::string &err);
void bspline_ders(int span, double u, int p, int nders, const double *U, double *out /*[p+1][5]*/);
int  axis_init_uniform(Axis &ax, int N, double Ui, double Uf, int C, std::string &err);
int  axis_set_knots(Axis &ax, int m, const double *U, std::string &err);
void axis_finish(Axis &ax);   // spans + nnp from U
int  basis_init(Basis1D &b, const Axis &ax, const Rule1D &rule, int nqp, std::string &err);
int  partition(int size, int rank, int dim, const int N[3], int n[3], int coords[3]);
void distribute(int dim, const int size[3], const int rank[3], const int N[3], int n[3], int s[3]);
void stencil(const Axis &ax, int i, int *first, int *last);   // src/petigamat.c:197-233

// Per-axis index layout of the local matrix (row box, column box, position tables, colours)
struct AxisLayout {
  int p = 0, gstart = 0, gwidth = 1;
  int alias = 0;                    // periodic axis wrapped inside one rank
  int nrow = 1, ncol = 1;
  int cstart = 0;                   // unwrapped node index of local column 0 (non-alias)
  std::vector<int> rowmap;          // [gwidth] ghost index -> row index
  std::vector<int> rownode;         // [nrow]   global node (wrapped)
  std::vector<int> colnode;         // [ncol]   global node (wrapped)
  std::vector<int> rcnt;            // [nrow]   columns in the row's per-axis stencil
  std::vector<int> rcol;            // [nrow][2p+1] sorted local column indices (padded -1)
  std::vector<int> P;               // [gwidth][2p+1] position of column (row + d - p) in the row's list, or -1
  std::vector<int> owned;           // [nrow] 1 if this rank owns the row node on this axis
  int ncolors = 1;
  std::vector<int> color;           // [nel_local]
};

struct Space {
  int dim = 0, dof = 0, order = -1;
  Axis axis[3];
  int rule_nqp[3] = {-1, -1, -1};
  Rule1D rule[3];
  Basis1D basis[3];
  int comm_size = 1, comm_rank = 0;
  int proc_req[3] = {-1, -1, -1};
  int proc_sizes[3] = {1, 1, 1}, proc_ranks[3] = {0, 0, 0};
  int elem_sizes[3] = {1, 1, 1}, elem_start[3] = {0, 0, 0}, elem_width[3] = {1, 1, 1};
  int node_sizes[3] = {1, 1, 1}, node_lstart[3] = {0, 0, 0}, node_lwidth[3] = {1, 1, 1};
  int node_gstart[3] = {0, 0, 0}, node_gwidth[3] = {1, 1, 1};
  int nsd = 0, rational = 0;
  std::vector<double> geomX, geomW;       // ghosted local
  std::vector<double> netX, netW;         // global control net (geometry grid, natural order) kept for IGXWrite / re-partitioning
  int npd = 0;                            // iga->property: numbers per node of the property array (0: none)
  std::vector<double> netA, propA;        // ... on the global net [node][npd] (natural order) / ghosted local (iga->propertyA, include/petiga.h:350-353)
  int net_nsd = 0;
  BC value[3][2], load[3][2];
  bool visit[3][2] = {{false, false}, {false, false}, {false, false}};   // IGAFormSetBoundaryForm, src/petigaform.c:134
  IGXFormKind form = IGX_FORM_NONE;
  std::vector<double> params;
  bool setup = false;
  double link_gbs = 0;        // GB/s per direction of a face message as the communicator measured it (comm.hpp); 0: not measured
  AxisLayout lay[3];
  EnvSwitches env;
};

int  space_setup(Space &s, std::string &err);          // IGASetUp stages 1+3 (src/petiga.c:1111-1310,1450-1493)
int  space_layout(Space &s, std::string &err);         // AxisLayout for the three axes
int  exchange_supported(const Space &s, std::string &err);   // 0, or IGX_ERR_SUP when a periodic ghost layer would wrap onto its own rank

// Fast diagonalisation (IGXFastDiagSetUp, host.cpp; the contractions: fast_diag.hpp).  Per axis and per combination "first / last function
// fixed" (combo = lo + 2 * hi) that some field uses: the generalised eigenpairs K U = M U Lambda, U^T M U = I, of the axis' 1-D stiffness and
// mass matrices over its free functions.
constexpr int MAXFD = 8;         // fields (= MAXBC)
struct FastDiagEig {
  bool used = false;             // some field uses the combination
  int first = 0, m = 0;          // the free functions are first .. first + m - 1
  std::vector<double> lambda;    // [m] ascending
  std::vector<double> s;         // [m] beta_axis * lambda, rounded: the axis' share of a mode's denominator
  std::vector<double> U;         // [m][m] column-major: U[i + m * k] = component i of eigenvector k
};
struct FastDiag {
  double alpha = 0, beta[3] = {0, 0, 0};
  int n[3] = {1, 1, 1};                        // functions per axis (the vector's row box: one rank)
  int dof = 0;
  bool fixed[3][2][MAXFD];                     // [axis][side][field]: the face is a Dirichlet face of the field (never on a periodic axis)
  FastDiagEig eig[3][4];                       // [axis][combo]
  std::vector<double> count[3];                // [n]: elements that hold the function (their product over the axes: the fixed rows' diagonal)
  double thresh = 0;                           // modes with |alpha + sum beta lambda| <= thresh are zeroed
  int nzeroed = 0;
  int combo(int d, int f) const { return (fixed[d][0][f] ? 1 : 0) + (fixed[d][1][f] ? 2 : 0); }
};
void fast_diag_fixed_faces(const Space &s, bool fixed[3][2][MAXFD]);      // the Dirichlet faces as the element kernels read them
int  fast_diag_setup(const Space &s, double alpha, const double beta[3], FastDiag &fd, std::string &err);
// the dense symmetric-definite eigen-solver behind it (Cholesky in long double, cyclic Jacobi, refinement), also IGXEigenSolve's Rayleigh-Ritz step
int  generalised_eigen(int m, const std::vector<double> &M, const std::vector<double> &K, FastDiagEig &out, std::string &err);

// Transfer between nested spline spaces (IGXTransferCreate, host.cpp; the kernels: transfer.hpp).  Per axis the nf x nc matrix T with
// B^c_j = sum_i T[i][j] B^f_i, by rows as a band of at most p + 1 consecutive columns, and its transpose as CSR by coarse row.
struct TransferAxis {
  int p = 0, nf = 1, nc = 1, width = 1, periodic = 0;
  bool identity = true;            // nf = nc and every row is the unit row with the entry exactly 1.0
  std::vector<int> first, count;   // [nf] first non-zero column (folded into [0, nc) on a periodic axis: column (first + k) mod nc) and the band's length
  std::vector<int> ufirst;         // [nf] the same column before folding, shifted by a multiple of nc so that row 0's lies in [0, nc): the boxes' footprints
  std::vector<double> T;           // [nf][width], zero past count
  std::vector<int> pptr, pidx;     // the rows again as CSR with folded columns (the axis passes): [nf + 1], [pptr[nf]]
  std::vector<double> pval;
  std::vector<int> rptr, ridx;     // T^T as CSR by coarse row, fine rows ascending: [nc + 1], [rptr[nc]]
  std::vector<double> rval;
};
// 0, or IGX_ERR_ARG_OUTOFRANGE with the reason in err: the spaces are not nested.  The caller has checked degree, periodicity and clamped ends.
int  transfer_axis_setup(const Axis &coarse, const Axis &fine, int axis, TransferAxis &t, std::string &err);

#endif   // !IGX_RTC

// ------------------------------------------------------------------ device descriptors (POD, passed by value)
constexpr int MAXBC = 8;      // fields per face the device tables hold (dof <= 8 on the device path)
constexpr int NDER = 4;       // 1-D derivative slots kept on the device: orders 0..3

struct BCDev { int count; int field[MAXBC]; double value[MAXBC]; };

struct AxisDev {
  int nel, nqp, nen, p;
  int estart, esizes, periodic;
  int gwidth, nrow, ncol;
  const double *tab;   // [nel][nqp][nen][NDER]
  const double *w;     // [nel][nqp]
  const double *J;     // [nel]
  const double *pt;    // [nel][nqp]
  const double *bnd;   // [2 sides][nen][NDER] basis at the first / last knot of the axis
  double bndpt[2];
  const int *off;      // [nel]  ghost-local index of the element's first basis function
  const int *rowmap;   // [gwidth]
  int rwrap;           // rowmap in closed form: rowmap[i] = i < rwrap ? i : i - rwrap (a periodic axis wrapped inside the rank: nnp)
  const int *rcnt;     // [nrow]
  const int *P;        // [gwidth][2p+1]
  const int64_t *prefix;  // [nrow+1] exclusive prefix sums of rcnt
  int64_t tot;         // sum of rcnt
  int off_lin, off0;   // off in closed form: off[e] = off0 + e for every element of the rank (one new basis function per element: maximal continuity); else off_lin = 0
};

struct SpaceDev {
  int dim, dof, order, nsd, rational;
  AxisDev ax[3];
  const double *X;     // ghosted local [.][nsd] or null
  const double *W;     // ghosted local or null
  BCDev bcv[3][2], bcl[3][2];
  const double *fixtable;  // row-indexed [nrows][dof] or null
  const double *A;         // property array, ghosted local [.][npd], or null
  int npd;
};

struct ColorRange { int start[3], step[3], count[3]; };

enum Op { OP_SYSTEM = 0, OP_MATRIX, OP_VECTOR, OP_FUNCTION, OP_JACOBIAN, OP_IFUNCTION, OP_IJACOBIAN, OP_SCALAR,
          OP_MATRIX_ACTION, OP_JACOBIAN_ACTION, OP_IJACOBIAN_ACTION,        // Y = A X of the matrix the driver would assemble, matrix-free (vec_sumfact.hpp)
          OP_MATRIX_DIAGONAL, OP_JACOBIAN_DIAGONAL, OP_IJACOBIAN_DIAGONAL,    // D = diag A of the same matrix, matrix-free (vec_sumfact.hpp, DIAGONAL; vec is D)
          OP_MATRIX_BLOCK_DIAGONAL, OP_JACOBIAN_BLOCK_DIAGONAL, OP_IJACOBIAN_BLOCK_DIAGONAL };      // its dof x dof point blocks (DIAGONAL, BLOCK; bcol are the columns)

struct OutDev {
  const int64_t *browptr;  // null when no matrix output
  double *val;
  double *vec;             // null when no vector output
  const double *U, *V;     // row-indexed state vectors or null
  double shift, t;
  int op;
  int *errflag;
  int bid;                 // boundary-form pass: 2*axis+side (IGAElementNextForm, src/petigaelem.c:427); -1 = interior pass
  int first_touch;         // 1: the matrix was not zeroed: the first colour that reaches an entry stores it (feature kernel)
  int debug;               // experiment switches (IGX_DEBUG_FEATURE): 1 no scatter, 2 atomic scatter, 4 no MFMA phase
  long long *clk;          // IGX_CLOCK_PROBE: [ticks, wall ticks, elements] of workgroup 0 of the last pencil launch, or null
  long long *dbg;          // experiment: s_memtime stamps of workgroup 0 per phase (IGX_DEBUG_FEATURE & 8)
  int ft2_lo, ft2_hi, ft2_blocked;   // feature kernel, assembly in two passes over axis 2 (upper face first): first-touch rule of the pass; ft2_hi = 0: one pass
  int64_t elem_base;       // OP_SCALAR: index of this launch's first element in the per-element partial sums (vec)
  int vec_mode;            // vec_sumfact as a part of IGAComputeSystem next to a band-row kernel: 1 the whole vector (lifting of the Dirichlet values through
                           // SystemVectorOf<Form>, a fixed row takes its value), 2 the form's vec() alone with the fixed rows left at 0 (block_pencil lifts itself)
  const double *X;         // OP_*_ACTION: the row-indexed direction (vec is Y), else null
  double *bcol[MAXBC];     // OP_*_BLOCK_DIAGONAL: the dof block columns, bcol[j][node * dof + i] = A_(node,i),(node,j) (vec is bcol[0]), else null
};

// The matrix-free action on a block of vectors (vec_sumfact, BATCH): the directions and results of one launch, a kernel argument of its
// own beside OutDev (whose X and vec stay null).  nc columns, 1 .. IGX_ACTION_MAXCOLS; entries of X may repeat, those of Y may not.
struct ActionCols {
  const double *X[IGX_ACTION_MAXCOLS];
  double *Y[IGX_ACTION_MAXCOLS];
  int nc;
};

#ifndef IGX_RTC
// the drivers that assemble a matrix / a vector (IGAComputeSystem does both)
inline bool op_has_matrix(int op) { return op == OP_SYSTEM || op == OP_MATRIX || op == OP_JACOBIAN || op == OP_IJACOBIAN; }
inline bool op_has_vector(int op) { return op == OP_SYSTEM || op == OP_VECTOR || op == OP_FUNCTION || op == OP_IFUNCTION; }

// What one pass of vec_sumfact (vec_sumfact.hpp) forms: the vector of a vector-only driver, or one of the matrix-free operators -- Y = A X,
// the same on a block of columns in one launch, D = diag A, the dof x dof point blocks -- which run on that kernel or not at all
// (DESIGN.md 3.23).  The mode is named once, here; its traits are the only place that knows the kernel's four booleans.
enum class VsMode { VECTOR, ACTION, ACTION_BATCH, DIAGONAL, BLOCK_DIAGONAL };
struct VsTraits {
  bool action, diagonal, block, batch;      // vec_sumfact's template parameters ACTION, DIAGONAL, BLOCK, BATCH
  bool wide;                                // the layouts of one workgroup per element, 6 and 8 lanes per axis, exist (degrees 4 to 7)
  const char *words;                        // the mode's part of the kernel name
};
constexpr VsTraits vs_traits(VsMode m) {
  switch (m) {
  case VsMode::ACTION:         return {true, false, false, false, true, "matrix action: sum factorisation forward and backward, "};
  case VsMode::ACTION_BATCH:   return {true, false, false, true, true, "matrix action on a block: sum factorisation forward and backward, "};
  case VsMode::DIAGONAL:       return {false, true, false, false, true, "matrix diagonal: sum factorisation forward, product rows backward, "};
  case VsMode::BLOCK_DIAGONAL: return {false, true, true, false, true, "matrix block diagonal: sum factorisation forward, product rows backward per field pair, "};
  default:                     return {false, false, false, false, false, "vector only: sum factorisation forward and backward, "};
  }
}
// the mode of an op (ACTION_BATCH is the driver's choice for a block of columns), and the op of a mode for IGX_OP_MATRIX / _JACOBIAN / _IJACOBIAN
inline VsMode vs_mode_of(int op) {
  return op < OP_MATRIX_ACTION || op > OP_IJACOBIAN_BLOCK_DIAGONAL ? VsMode::VECTOR : op < OP_MATRIX_DIAGONAL ? VsMode::ACTION : op < OP_MATRIX_BLOCK_DIAGONAL ? VsMode::DIAGONAL : VsMode::BLOCK_DIAGONAL;
}
inline int matfree_op(VsMode m, int igx_op) { return (vs_traits(m).block ? OP_MATRIX_BLOCK_DIAGONAL : vs_traits(m).diagonal ? OP_MATRIX_DIAGONAL : OP_MATRIX_ACTION) + igx_op; }

// basis functions and points of axis d: the basis' once the space is set up, before that what the axes and rules set so far will give (src/petigabasis.c:103)
inline void vec_axis_sizes(const Space &s, int d, int &nen, int &nqp) {
  if (s.setup) { nen = s.basis[d].nen; nqp = s.basis[d].nqp; }
  else { nen = s.axis[d].p + 1; nqp = s.rule_nqp[d] > 0 ? s.rule_nqp[d] : s.axis[d].p + 1; }
}
// the largest of them over the three axes: up to 4 a wavefront holds an element (3: two), up to 6 and up to 8 a workgroup does
inline int vec_lanes_per_axis(const Space &s) {
  int m = 0;
  for (int d = 0; d < 3; ++d) { int nen, nqp; vec_axis_sizes(s, d, nen, nqp); m = nen > m ? nen : m; m = nqp > m ? nqp : m; }
  return m;
}
// The layout of a launch of vec_sumfact in a mode, for the built-in forms (try_vec_sumfact) and the run-time structs (launch_vecsf_rtc)
// alike.  compile_only (IGXCheckFormSource): the space may not be set up, the degrees decide.
struct VsLaunch {
  int ns;                  // lanes per axis: 3 two elements per wavefront (p <= 2), 4 one; 6 and 8 one workgroup per element (wide modes)
  unsigned threads;        // per workgroup (vs_layout<ns>::THREADS)
  const char *tail;        // the layout's part of the kernel name
  // (one pass per wavefront: the launch has a wavefront per unit -- UNITS = 1 in the kernel)
  unsigned grid(long long nelem) const { return ns > 4 ? (unsigned)nelem : (unsigned)((nelem + (ns == 3 ? 7 : 3)) / (ns == 3 ? 8 : 4)); }
};
inline VsLaunch vs_launch_of(const Space &s, VsMode m, bool compile_only = false) {
  const int lanes = vs_traits(m).wide ? vec_lanes_per_axis(s) : 4;      // (the vector-only drivers stay at 4 and below: vec_sumfact_covers)
  if (lanes > 6) return {8, 512, "one workgroup per element, 8 x 8 x 8 lanes)"};
  if (lanes > 4) return {6, 256, "one workgroup per element, 6 x 6 x 6 lanes)"};
  // at most three basis functions and points per axis (p <= 2): two elements per wavefront (54 of 64 lanes instead of 27)
  bool three = !s.env.no_vec_pairs;
  for (int d = 0; d < 3; ++d) three = three && (compile_only ? s.axis[d].p >= 1 && s.axis[d].p <= 2 : s.basis[d].nen <= 3 && s.basis[d].nqp <= 3);
  if (three) return {3, 256, "two elements per wavefront)"};
  return {4, 256, "one wavefront per element)"};
}
#endif

constexpr int MAXPARAM = 8;
struct ParamsDev { double v[MAXPARAM]; };

}  // namespace igx
