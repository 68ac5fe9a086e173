/*
 * petiga_amd.h -- C ABI of libpetiga_amd.so: the MI355X-native IGA element-assembly engine.
 *
 * This is the drop-in boundary for ONE path of dalcinl/PetIGA: the element loop behind
 *   IGAComputeSystem / IGAComputeMatrix / IGAComputeVector      (src/petigaksp.c:33,79,149)
 *   IGAComputeFunction / IGAComputeJacobian                     (src/petigasnes.c:23,82)
 *   IGAComputeIFunction / IGAComputeIJacobian                   (src/petigats.c:23,92)
 * i.e. IGANextElement -> IGAElementBuildTabulation -> point callback -> IGAPointAddMat ->
 * IGAElementFixSystem -> IGAElementAssembleMat, re-implemented as HIP kernels for gfx950.
 *
 * Everything is plain C: opaque handles, int/double scalars, raw pointers and sizes.  No PETSc,
 * torch or C++ types cross this boundary.  All citations are file:line of the reference tree.
 *
 * Two ways in:
 *   (1) IGXCreate + IGXAxis* + IGXSetUp ...   mirrors the PetIGA user API (include/petiga.h),
 *       so a test written against PetIGA reads the same against this library;
 *   (2) IGXCreateFromTables                    takes the tables a set-up PetIGA `IGA` already
 *       holds (struct _p_IGA, include/petiga.h:327-391) -- what IGAComputeSystem inside
 *       libpetiga would bind.
 *
 * Error convention: every function returns an int error code, 0 = success, non-zero values are
 * PETSc's own PetscErrorCode numbers for the same condition (include/petscerror.h) so the
 * adapter can `CHKERRQ` them unchanged.  IGXGetLastError() returns the message SETERRQ would print.
 */
#ifndef PETIGA_AMD_H
#define PETIGA_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* PetscErrorCode values reused verbatim */
#define IGX_ERR_SUP             56   /* PETSC_ERR_SUP             */
#define IGX_ERR_ORDER           58   /* PETSC_ERR_ORDER           */
#define IGX_ERR_ARG_WRONG       62   /* PETSC_ERR_ARG_WRONG       */
#define IGX_ERR_ARG_OUTOFRANGE  63   /* PETSC_ERR_ARG_OUTOFRANGE  */
#define IGX_ERR_ARG_WRONGSTATE  73   /* PETSC_ERR_ARG_WRONGSTATE  */
#define IGX_ERR_LIB             76   /* PETSC_ERR_LIB (HIP runtime failure) */
#define IGX_ERR_PLIB            77   /* PETSC_ERR_PLIB            */
#define IGX_ERR_USER            83   /* PETSC_ERR_USER (e.g. non-positive Jacobian, src/petigaelem.c:989-993) */
#define IGX_ERR_MEM             55   /* PETSC_ERR_MEM             */

#define IGX_DECIDE (-1)              /* PETSC_DECIDE */

typedef struct _p_IGX    *IGX;       /* replaces `IGA`  (include/petiga.h:327)                  */
typedef struct _p_IGXMat *IGXMat;    /* replaces the `Mat` of IGACreateMat (src/petigamat.c:345) */
typedef struct _p_IGXVec *IGXVec;    /* replaces the `Vec` of IGACreateVec (src/petigavec.c:78)  */

const char *IGXGetLastError(void);

/* ------------------------------------------------------------------------------------------
 * Device point forms.  PetIGA's point callbacks are host function pointers
 * (IGAFormSystem etc., include/petiga.h:153-197) and cannot run on the GPU; the engine keeps
 * their contract (point-wise, un-weighted integrand, K[a][i][b][j] / F[a][i] row-major,
 * src/petigapoint.c:451-462) and binds the function at compile time.  `params` replaces `ctx`.
 * ------------------------------------------------------------------------------------------ */
typedef enum {
  IGX_FORM_NONE        = 0,
  IGX_FORM_POISSON     = 1, /* System: demo/Poisson{1,2,3}D.c:3-23        K=grad.grad, F=N*1          params: none */
  IGX_FORM_MASS        = 2, /* System: test/IGACreate.c:45-63             K=Na*Nb (per field), F=N    params: none */
  IGX_FORM_L2PROJ_X2   = 3, /* System: test/IGAFixTable.c:25-43           K=Na*Nb, F=N*sum x^2        params: none */
  IGX_FORM_POISSON_F   = 4, /* System: test/IGAFixTable.c:45-64           K=grad.grad, F=N*(-2 dim)   params: none */
  IGX_FORM_ERRNORM     = 5, /* System: test/IGAErrNorm.c:54-75 (dof=4)    L2 projection of 1,Sx,Sx2,Px              */
  IGX_FORM_ELASTICITY  = 6, /* System: demo/Elasticity3D.c:13-46 (dof=3)  params: {lambda, mu}                      */
  IGX_FORM_CAHNHILLIARD= 7, /* IFunction/IJacobian: demo/CahnHilliard3D.c:55-179 (and the 2-D demo)
                               params: {theta, alpha, cbar, L0, lambda, tau}; L0<=0 selects the 2-D demo's 3*alpha scaling */
  IGX_FORM_NSVMS       = 8, /* IFunction/IJacobian: demo/NavierStokesVMS.c:78-244 (dof=4)
                               params: {nu, fx, fy, fz, dt}  (dt: the reference reads TSGetTimeStep at :85,:173) */
  IGX_FORM_BOUNDARYINTEGRAL = 9, /* System: demo/BoundaryIntegral.c:26-56  interior Laplace, F=N*1 on visited faces (Neumann) */
  IGX_FORM_NITSCHE     = 10,/* System: demo/NitscheMethod.c:69-110  Poisson with Nitsche terms on visited faces (normals,
                               normal mesh size through IGAPointFormInvGradGeomMap); params: {max degree k} */
  IGX_FORM_BRATU       = 11,/* Function/Jacobian and IFunction/IJacobian: demo/Bratu.c, demo/BratuFJ.F90:23-176  params: {lambda} */
  IGX_FORM_ELASTICITY_F = 12,/* System: demo/Elasticity3D.c's K with a body force, F[a][i] = N_a f_i   params: {lambda, mu, fx, fy, fz} */
  IGX_FORM_DER3 = 13,        /* System / Function on third derivatives (p->shape[3], IGAPointFormDer3: test/IGAGeometryMap.c:179,221): K = N N + k3 d3N : d3N,
                              * F = N (1 + |x|^2) + f3 c : d3N + u3 N c : d3u; params {k3, f3, u3}; the general kernel (order-3 tabulation) */
  IGX_FORM_SURFACE = 15,     /* System on a curve / surface in space (IGXSetGeometry with nsd > dim; demo/ClassicalShell.c:57-80 reads p->mapX the same way):
                              * Laplace-Beltrami + mass, load |H| (mean-curvature vector from p->mapX[1], p->mapX[2]); dim 1, 2; the general kernel */
  IGX_FORM_PROPERTY = 14,    /* System: Poisson with conductivity A[..][0] and source A[..][npd-1] of the property array (IGXSetProperty), interpolated
                              * at the point from p->property; the general kernel */
  IGX_FORM_SOURCE      = 100 /* a user form compiled at run time: IGXSetFormSource */
} IGXFormKind;

/* ------------------------------------------------------------------------------------------
 * (1) Mirror of the PetIGA set-up API
 * ------------------------------------------------------------------------------------------ */
int IGXCreate(IGX *iga);                                   /* IGACreate          src/petiga.c:32   */
int IGXDestroy(IGX *iga);                                  /* IGADestroy         src/petiga.c:79   */
int IGXSetDim(IGX iga,int dim);                            /* IGASetDim          src/petiga.c:281  */
int IGXSetDof(IGX iga,int dof);                            /* IGASetDof          src/petiga.c:334  */
int IGXSetOrder(IGX iga,int order);                        /* IGASetOrder        src/petiga.c:463  (clipped to [1,4]) */
int IGXSetQuadrature(IGX iga,int i,int q);                 /* IGASetQuadrature   src/petiga.c:530  */
/* Quadrature rule of an axis (IGARuleType, include/petiga.h:82-87).  LEGENDRE (q = 1..10) and LOBATTO (q = 2..10) carry the
 * doubles of the reference's tables (src/petigarule.c:182-319, :321-459); USER takes any rule on [-1,1]; REDUCED is Gauss-Legendre
 * with q points on the first and the last element of the axis and q - 1 on the others (src/petigabasis.c:144-171): the engine keeps
 * q slots per element and gives the last one of an interior element weight 0 (the reference trims it, src/petigaelem.c:764-776),
 * so the results are the reference's and the cost is that of the full rule. */
typedef enum { IGX_RULE_LEGENDRE = 0, IGX_RULE_LOBATTO = 1, IGX_RULE_REDUCED = 2, IGX_RULE_USER = 3 } IGXRuleType;
int IGXSetRuleType(IGX iga,int i,IGXRuleType type);        /* IGASetRuleType     src/petiga.c:500  */
int IGXSetRuleSize(IGX iga,int i,int nqp);                 /* IGASetRuleSize     src/petiga.c:515  */
int IGXSetRule(IGX iga,int i,int q,const double x[],const double w[]); /* IGAGetRule + IGARuleSetRule  src/petigarule.c:145 */
int IGXGetRule(IGX iga,int i,int *q,double x[],double w[]); /* IGAGetRule + IGARuleGetRule  src/petigarule.c:160: the rule IGXSetUp
                                                              will use (x, w may be NULL; room for *q entries: ask for q first) */
int IGXSetProcessors(IGX iga,int i,int processors);        /* IGASetProcessors   src/petiga.c:547  */
int IGXSetComm(IGX iga,int size,int rank);                 /* the (size,rank) of the MPI_Comm given to IGACreate */
int IGXAxisSetDegree(IGX iga,int i,int p);                 /* IGAAxisSetDegree   src/petigaaxis.c:168 */
int IGXAxisSetPeriodic(IGX iga,int i,int flag);            /* IGAAxisSetPeriodic src/petigaaxis.c:150 */
int IGXAxisInitUniform(IGX iga,int i,int N,double Ui,double Uf,int C); /* IGAAxisInitUniform src/petigaaxis.c:401 */
int IGXAxisSetKnots(IGX iga,int i,int m,const double U[]); /* IGAAxisSetKnots    src/petigaaxis.c:202 */
int IGXSetUp(IGX iga);                                     /* IGASetUp           src/petiga.c:1450 */

/* Geometry: control net on the geometry grid (n+1 points per axis, i0 fastest), Cartesian X[...][nsd]
 * and optional NURBS weights W (NULL = polynomial).  Stands for IGASetGeometryDim + the arrays
 * iga->geometryX / iga->rationalW that IGALoadGeometry fills (src/petigaio.c:201-356).
 * dim <= nsd <= 3.  nsd > dim (a curve or a surface in space, demo/ClassicalShell.c:154): the geometry map is tabulated, the inverse
 * map is not -- shape functions and measure stay parametric, a face's normal is its axis (src/petigaelem.c:966-1029) -- and the form
 * reads p->mapX[1], p->mapX[2] (NEED_MAPX: p.X1 [nsd][dim], p.X2 [nsd][dim][dim]); such assemblies run on the general kernel. */
int IGXSetGeometry(IGX iga,int nsd,const double X[],const double W[]);
/* Derivative order (IGASetOrder, src/petiga.c:463): forms that read third derivatives -- p->shape[3] ([nen][dim][dim][dim], include/petiga.h:657)
 * as the dim^3 numbers behind the Hessian in Na / Nb, IGAPointFormDer3 (include/petiga.h:731) as p.d3u with NEED_D3U -- declare ORDER = 3
 * and need IGXSetOrder(iga,3) (the default order is the largest degree, src/petiga.c:1472-1475); they run on the point-form kernel, which
 * then tabulates K2, Rationalize, GeometryMap, InverseMap and ShapeFunctions at order 3 (src/petigamapinv.f90.in:49-60,
 * src/petigamapshf.f90.in:60-72).  Every other form is tabulated as far as it reads, whatever the order set here. */
/* Property array: npd numbers per node of the geometry grid (natural order, [node][npd]); npd = 0 drops it.  Stands for
 * IGASetPropertyDim + iga->propertyA as IGALoadProperty fills it (src/petigaio.c:359-458).  A point's form sees the values of its
 * element's nodes as p->property [nen][npd] (IGAElementBuildClosure, src/petigaelem.c:745-752; include/petiga.h:662): forms that
 * read them (NEED_PROP) run on the general kernel.  IGXRead / IGXWrite carry the array (info bit 1 of the file, src/petigaio.c:38,105). */
int IGXSetProperty(IGX iga,int npd,const double A[]);
int IGXGetPropertyDim(IGX iga,int *npd);   /* IGAGetPropertyDim src/petigaio.c:384 */

int IGXSetBoundaryValue(IGX iga,int axis,int side,int field,double value); /* IGASetBoundaryValue src/petigaform.c:324 */
int IGXSetBoundaryLoad (IGX iga,int axis,int side,int field,double value); /* IGASetBoundaryLoad  src/petigaform.c:340 */
int IGXClearBoundary(IGX iga);                                             /* IGAFormClearBoundary src/petigaform.c:143 (all faces) */
/* boundary-form pass of face (axis,side): the form is also integrated over that face, one point layer at the face, with
 * p->atboundary / p->normal semantics (IGAElementNextForm src/petigaelem.c:427; normals src/petigaval.F90:45-99) */
int IGXSetBoundaryForm(IGX iga,int axis,int side,int flag);                /* IGASetBoundaryForm  src/petigaform.c:356 */
int IGXSetFixTable(IGX iga,IGXVec U);                                      /* IGASetFixTable      src/petigaform.c:273 (NULL clears) */

/* IGASetFormSystem / IGASetFormMatrix / ... (src/petigaform.c:388-833): kind + params replace (fn,ctx).
 * The one kind serves System/Matrix/Vector or Function/Jacobian/IFunction/IJacobian as the reference demo does. */
int IGXSetForm(IGX iga,IGXFormKind kind,const double params[],int nparams);

/* The open end of the plugin API (IGASetFormSystem(iga,fn,ctx) with an arbitrary user fn, src/petigaform.c:388-833): a point
 * form given as HIP source and compiled at run time (hiprtc) into the general element kernel.  `source` defines a struct
 * `struct_name` with the contract of the built-in forms (petiga_amd/csrc/forms.hpp, the device restatement of
 * include/petiga.h:153-197 + src/petigapoint.c:427-462):
 *     struct MyForm {
 *       static constexpr int DOF = 1, ORDER = 1;          // fields per node; 2 if second derivatives of N or of U are read, 3 for third
 *                                                         // ones (p->shape[3]: dim^3 numbers behind the Hessian in Na / Nb; IGXSetOrder(3))
 *       static constexpr unsigned NEED = NEED_X | NEED_U; // point data read: NEED_X x, NEED_U u, NEED_UT du/dt, NEED_GU grad u,
 *                                                         // NEED_HU hess u, NEED_G IGAPointFormInvGradGeomMap; on the point-form kernel
 *                                                         // only: NEED_D3U p.d3u (IGAPointFormDer3), NEED_PROP p.property [nen][npd] with
 *                                                         // the point's shape table p.shape [nen][nf], NEED_MAPX p.X1 / p.X2 (p->mapX[1], [2])
 *       static __device__ void mat(const PtView &p,const double *Na,const double *Nb,double *T); // T[i*DOF+j]: K block of (a,b)
 *       static __device__ void vec(const PtView &p,const double *Na,double *R);                  // R[i]: F entries of a
 *     };
 * Na / Nb: [0] N, [1+i] dN/dx_i, [1+dim+i*dim+j] d2N/dx_i dx_j; p.prm[] = params (the callback's ctx); the integrand is
 * un-weighted and mat() must be linear in Na and in Nb, as every IGAFormSystem/Jacobian is.  Compile errors come back as
 * PETSC_ERR_USER with the compiler log in IGXGetLastError().  The seven drivers then work as with a built-in form: on the
 * matrix cores (feature_assemble<MyForm,...>, compiled on first use for the wave layout of the degree, about half a second)
 * for dim >= 2 and (p+1)^dim <= 64 (in 3-D also p = 4, 5 for forms with at most two / one accumulator set), on the point-form
 * kernel otherwise or with IGXSetKernel(1).  IGX_RTC_CACHE_DIR in the
 * environment keeps the compiled code objects on disk for later processes.  Optional declarations that
 * speed the matrix-core kernel up, all bit masks over the feature index of Na / Nb:
 *       static constexpr unsigned MAT_TEST_MASK = ...;         // features of Na that mat() reads (others never enter the GEMM)
 *       static constexpr unsigned PHI_MASK = ...;              // features anything reads (others are not tabulated at all)
 *       static constexpr unsigned long long MAT_PAIR_MASK = ...; // bit 8f+g: mat() has a point-INDEPENDENT coefficient on
 *                                                              // Na[f]*Nb[g] and nothing else: Gram matrices on the matrix cores
 *       static constexpr unsigned pair_block_mask(int f,int g); // with MAT_PAIR_MASK: bit i*DOF+j set when the pair (f,g) reaches
 *                                                              // block entry (i,j) (x*0 does not fold under IEEE rules)
 *       static constexpr unsigned MAT_NEED = ...;              // subset of NEED that mat() reads (matrix-only drivers skip the rest)
 *       static constexpr bool MAT_SYMMETRIC = true;            // mat(p,Na,Nb) == mat(p,Nb,Na) at every point (the form's promise)
 *       static constexpr unsigned VEC_TEST_MASK = ...;         // features of Na that vec() reads
 * A scalar (DOF 1) first-order form with MAT_TEST_MASK = the gradients, MAT_SYMMETRIC and VEC_TEST_MASK = 1 (N) whose NEED is at
 * most NEED_X -- demo/Poisson3D.c's System, with any x-dependent or anisotropic diffusion tensor and load -- takes the pencil
 * walk of the headline kernel in 3-D at p = 2, 3 (form_pencil<MyForm>: combined band rows, first-touch stores, the Dirichlet
 * fix-up inside the walk, identity or mapped / NURBS geometry) instead of the element mode: IGXSetKernel(2) insists on it.
 * A struct with MAT_PAIR_MASK (and pair_block_mask), 2 or 3 fields and VEC_ZERO -- demo/Elasticity3D.c's System -- takes the band-row
 * kernel in 3-D at p = 3 on the identity geometry (block_pencil<MyForm>: the element loop turned inside out, each band row written
 * once per pencil), like the built-in form; IGXSetKernel(4) insists on it.
 * The vector-only drivers (Vector / Function / IFunction) of ANY struct without an atboundary branch run on the sum-factorised
 * kernel in 3-D at p <= 3 (vec_sumfact<MyForm>: nqp evaluations of vec() on unit test features instead of nen x nqp).
 * The Tangent (Jacobian / IJacobian) of a nonlinear scalar struct takes the same pencil walk when the struct splits it as
 * sum_f A_f(a) B_f(b) with the test side A = (N, dN/dx_0, dN/dx_1, dN/dx_2[, laplacian N]) and the trial side B carrying the point:
 *       static constexpr int PENCIL_NFEAT = 4 or 5, PENCIL_NC = <numbers per Gauss point, at most 9>;
 *       static __device__ void pencil_coef(const PtView &p,double JW,double *c);        // from u, grad u, diag hess u, shift, prm
 *       static __device__ void pencil_trial(const double *c,double N,const double *g,double lap,double *B);   // B[0..PENCIL_NFEAT)
 * (FormCahnHilliard / FormBratu in petiga_amd/csrc/forms.hpp are written this way; 3-D, p = 2 or 3, no geometry, dof 1.)
 * A four-field first-order struct that separates its point coefficients from the basis functions -- demo/NavierStokesVMS.c's
 * Tangent -- takes the band-row kernel with point records (band_points + band_pt<MyForm>, 3-D, p = 3; p = 2 with IGXSetKernel(4)):
 *       static constexpr int NCOEF = <coefficients per Gauss point>;
 *       static __device__ void point_coef(const PtView &p,double *c);                   // from the state and prm at the point
 *       static __device__ void mat_c(const double *c,const double *Na,const double *Nb,double *T);
 * and optionally mat_unit / BAND_NFEAT / BAND_NACC with band_coef / band_finish (FormNSVMS in petiga_amd/csrc/forms.hpp is the
 * model).  A struct with the BAND_NACC hooks also declares a guard on its parameters, evaluated on the DEVICE by a one-lane
 * kernel whenever the parameters change, so it must be callable there:
 *       __host__ __device__ static bool band_params_ok(const double *prm);      // false: stay on the feature kernel (e.g. nu = 0)
 * A guard that does not compile for the device (a plain host function) does not fail the assembly: the automatic choice falls
 * through to the feature kernel and IGXGetKernelName says why; IGXSetKernel(4) and IGXCheckFormSource(…, 6) report the compiler's log.
 *       static constexpr int SHAPE_ORDER = 1;                  // ORDER = 2 only for hess u: second derivatives of N are not kept
 *       static constexpr bool VEC_ZERO = true;                 // vec() returns zeros: the vector phase runs for the Dirichlet lifting only
 * Boundary-form passes (IGXSetBoundaryForm; `if (p->atboundary)` in the reference's callback, e.g. demo/NitscheMethod.c:69-110): a
 * struct that declares
 *       static constexpr bool HAS_BOUNDARY = true;
 *       static __device__ void bmat(const PtView &p,const double *Na,const double *Nb,double *T);   // the integrands at a point of a
 *       static __device__ void bvec(const PtView &p,const double *Na,double *R);                    // visited face (p.normal, p.boundary_id)
 * is integrated with bmat / bvec over the visited faces; a struct without them with its ordinary mat / vec, as the reference would. */
int IGXSetFormSource(IGX iga,const char *source,const char *struct_name,const double params[],int nparams);

/* On-disk formats (PETSc binary, big-endian): the discretisation + NURBS control net written by IGAWrite / igakit,
 * and a Vec in natural order.  IGXRead replaces dim, axes and geometry of `iga` (dof is kept); call IGXSetUp next. */
int IGXRead (IGX iga,const char filename[]);              /* IGARead     src/petigaio.c:141 -> IGALoad :11  */
int IGXWrite(IGX iga,const char filename[]);              /* IGAWrite    src/petigaio.c:171 -> IGASave :75  */
int IGXWriteVec(IGX iga,IGXVec vec,const char filename[]); /* IGAWriteVec src/petigaio.c:640 */
int IGXReadVec (IGX iga,IGXVec vec,const char filename[]); /* IGAReadVec  src/petigaio.c:690 */

/* sizes after IGXSetUp */
int IGXGetSizes(IGX iga,int elem_sizes[3],int elem_start[3],int elem_width[3],
                int node_sizes[3],int node_lstart[3],int node_lwidth[3],int node_gstart[3],int node_gwidth[3]);
int IGXGetProcessors(IGX iga,int proc_sizes[3],int proc_ranks[3]);
/* IGAGetBasis + struct _n_IGABasis (include/petiga.h:122-141): the 1-D tables IGXSetUp built for axis i, as the element loop
 * reads them (src/petigabasis.c:83-219): offset[nel], detJac[nel], weight[nel][nqp], point[nel][nqp], value[nel][nqp][nen][5].
 * Any array may be NULL; ask for the three sizes first. */
int IGXGetBasis(IGX iga,int i,int *nel,int *nqp,int *nen,int offset[],double detJac[],double weight[],double point[],double value[]);
int64_t IGXGetElementCount(IGX iga);   /* local elements */

/* ------------------------------------------------------------------------------------------
 * (2) Building the same object from a set-up PetIGA `IGA` (what libpetiga would pass)
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  /* per axis: struct _n_IGAAxis (include/petiga.h:80-96) */
  int           p, m, periodic, nel, nnp;
  const double *U;        /* [m+1] */
  const int    *span;     /* [nel] */
  /* per axis: struct _n_IGABasis (include/petiga.h:122-141) */
  int           nqp, nen;
  const int    *offset;   /* [nel]            */
  const double *detJac;   /* [nel]            */
  const double *weight;   /* [nel][nqp]       */
  const double *point;    /* [nel][nqp]       */
  const double *value;    /* [nel][nqp][nen][5] */
} IGXAxisTables;

typedef struct {
  int dim, dof, order;                       /* iga->dim, dof, order                              */
  IGXAxisTables axis[3];
  int proc_sizes[3], proc_ranks[3];          /* iga->proc_sizes/ranks                             */
  int elem_sizes[3], elem_start[3], elem_width[3];
  int node_sizes[3], node_lstart[3], node_lwidth[3], node_gstart[3], node_gwidth[3];
  int nsd;                                   /* iga->geometry (0 = none)                          */
  int rational;                              /* iga->rational                                     */
  const double *geometryX;                   /* ghosted local [gw2][gw1][gw0][nsd]  (iga->geometryX) */
  const double *rationalW;                   /* ghosted local [gw2][gw1][gw0]       (iga->rationalW) */
  /* appended in round 6 -- zero the whole struct before filling it (the adapter does: PetscMemzero), so that a field this header
   * grows later reads as "absent" */
  int property;                              /* iga->property: numbers per node (0 = none), include/petiga.h:350 */
  const double *propertyA;                   /* ghosted local [gw2][gw1][gw0][npd]  (iga->propertyA, include/petiga.h:353) */
} IGXTables;

int IGXCreateFromTables(const IGXTables *t,IGX *iga);

/* ------------------------------------------------------------------------------------------
 * Matrices and vectors (device resident)
 * ------------------------------------------------------------------------------------------ */
/* IGACreateMat (src/petigamat.c:345-549): exact pattern of the reference, block CSR with
 * dof x dof row-major blocks (AIJ for dof=1, BAIJ for dof>1, src/petiga.c:1328).  Rows are the
 * nodes of the local row box, columns are local column indices; see IGXMatGetLayout. */
int IGXCreateMat(IGX iga,IGXMat *mat);
int IGXMatDestroy(IGXMat *mat);
int IGXMatGetInfo(IGXMat mat,int64_t *nbrows,int64_t *nblocks,int *bs);
/* device pointers: browptr int64[nbrows+1], bcolidx int32[nblocks], val double[nblocks*bs*bs] */
int IGXMatGetDeviceArrays(IGXMat mat,const int64_t **browptr,const int32_t **bcolidx,double **val);
int IGXMatCopyToHost(IGXMat mat,int64_t *browptr,int32_t *bcolidx,double *val); /* any may be NULL */
/* per axis: number of row / column indices and the global node index each maps to
 * (rows: node index after periodic wrap; cols likewise) -- the LGMap of src/petigagrid.c:213 */
int IGXMatGetLayout(IGXMat mat,int nrow[3],int ncol[3]);
int IGXMatGetAxisMaps(IGXMat mat,int axis,int *rownode /*[nrow]*/,int *colnode /*[ncol]*/);

/* IGACreateVec (src/petigavec.c:78): one value per (row node, field), same row numbering as the matrix */
int IGXCreateVec(IGX iga,IGXVec *vec);
int IGXVecDestroy(IGXVec *vec);
int IGXVecGetSize(IGXVec vec,int64_t *n);
int IGXVecGetDeviceArray(IGXVec vec,double **array);
int IGXVecCopyToHost(IGXVec vec,double *host);
int IGXVecCopyFromHost(IGXVec vec,const double *host);

/* ------------------------------------------------------------------------------------------
 * The hot path.  Same meaning and argument order as the reference drivers; outputs are zeroed
 * first, then every local element's K_e/F_e is formed, BC-fixed and added (colour-ordered,
 * conflict-free, deterministic).  All work is enqueued on the engine's stream
 * (IGXSetStream); call IGXSynchronize before reading results through raw device pointers.
 * ------------------------------------------------------------------------------------------ */
int IGXComputeSystem   (IGX iga,IGXMat A,IGXVec b);                               /* src/petigaksp.c:149 */
int IGXComputeMatrix   (IGX iga,IGXMat A);                                        /* src/petigaksp.c:79  */
int IGXComputeVector   (IGX iga,IGXVec b);                                        /* src/petigaksp.c:33  */
int IGXComputeFunction (IGX iga,IGXVec U,IGXVec F);                               /* src/petigasnes.c:23 */
int IGXComputeJacobian (IGX iga,IGXVec U,IGXMat J);                               /* src/petigasnes.c:82 */
int IGXComputeIFunction(IGX iga,double a,IGXVec V,double t,IGXVec U,IGXVec F);    /* src/petigats.c:23   */
int IGXComputeIJacobian(IGX iga,double a,IGXVec V,double t,IGXVec U,IGXMat J);    /* src/petigats.c:92   */
/* The pair a Newton step asks for at one state -- SNESComputeFunction then SNESComputeJacobian on the same U (TS: the same a, V, t)
 * -- in ONE pass of the element loop (R_e and K_e share the tabulation and the state's point values).  F and J are
 * those of IGXComputeIFunction + IGXComputeIJacobian (IGXComputeFunction + IGXComputeJacobian).  With IGX_FUSE_RESID=1 in the
 * environment and where a fused kernel exists (state_pencil_kr: Cahn-Hilliard / Bratu, 3-D, p = 2, no geometry, no boundary
 * loads: config 4) the Residual rides on the Tangent's MFMAs as one more operand column; otherwise -- the default: the fused walk
 * measured 3 % slower than the two passes, DESIGN.md 3.1 -- the two drivers run one after the other.  IGXGetKernelName tells. */
int IGXComputeIFunctionIJacobian(IGX iga,double a,IGXVec V,double t,IGXVec U,IGXVec F,IGXMat J);
int IGXComputeFunctionJacobian(IGX iga,IGXVec U,IGXVec F,IGXMat J);
/* Matrix-free actions (no reference entry point: the product of the driver's matrix with a vector -- what MATSHELL / -snes_mf_operator
 * ask of an assembly engine once the matrix no longer fits).  Y = A X with A the matrix IGXComputeJacobian / IGXComputeIJacobian
 * assemble on this rank and, for IGXComputeMatrixAction, the matrix of IGXComputeSystem -- IGXComputeMatrix's K with the matrix
 * half of IGAElementFixSystem applied, i.e. K itself where no Dirichlet value is set (the operator a linear solve needs).
 * IGAElementFixJacobian in all three: a fixed column takes no contribution and a fixed row receives X_row once per local element
 * that holds the node (the element count on the diagonal).  No matrix is allocated and no
 * index is read: the direction's point values go through mat() in place of a trial function (every mat() is linear in Nb), one
 * more forward pass per field on the sum-factorised vector kernel (vec_sumfact, ACTION).  Y is zeroed and then assembled like any
 * vector, with the same row numbering; on several ranks X must hold its ghosts (IGXRefreshGhosts) and IGXReduceGhostRows(iga,NULL,Y)
 * completes the ghost rows.  Covered: 3-D, nen and nqp <= 8 per axis (degree <= 7; up to 4 one wavefront works on an element, up
 * to 6 and up to 8 one workgroup of 256 / 512 threads), identity / polynomial / NURBS geometry with nsd = 3, Dirichlet
 * values, periodic axes, every built-in or run-time form of order <= 2 without a boundary branch.  Everything else -- a boundary-form
 * pass, dim != 3, nsd != dim, order-3 or property forms, nen or nqp > 8, IGX_VEC_SUMFACT=0, an IGXSetKernel choice other than 0 -- returns
 * IGX_ERR_SUP with the reason: there is no fallback kernel.  Boundary loads do not enter a matrix and are ignored.  X == Y, a
 * vector of another IGX or a null vector: IGX_ERR_ARG_WRONG; no form set: IGX_ERR_ARG_WRONGSTATE. */
int IGXComputeMatrixAction   (IGX iga,IGXVec X,IGXVec Y);                                        /* Y = K X,    K of IGXComputeSystem    */
int IGXComputeJacobianAction (IGX iga,IGXVec U,IGXVec X,IGXVec Y);                               /* Y = J(U) X, J of IGXComputeJacobian  */
int IGXComputeIJacobianAction(IGX iga,double a,IGXVec V,double t,IGXVec U,IGXVec X,IGXVec Y);    /* J of IGXComputeIJacobian             */
/* The same actions on a block of vectors: Y_j = A X_j for j = 0 .. nx-1, 1 <= nx <= 48 (the block-vector limit of IGXVecMDot), in one
 * walk over the colours per chunk of IGX_ACTION_MAXCOLS columns (vec_sumfact, BATCH).  Nearly all an element costs does not
 * depend on the direction -- its rows, offsets, control points, the geometry chain, the state's point values, the Dirichlet flags, JW --
 * and is done once per element and chunk; the direction's forward pass, mat(), the way back and the scatter run per column, and the
 * launch count drops from colours x nx to colours x ceil(nx / 16) (IGXGetLastTiming).  The contract of the single action holds per column:
 * the Dirichlet rows; on several ranks every X_j holds its ghosts (IGXRefreshGhosts) and IGXReduceGhostRows(iga,NULL,Y_j) completes each
 * result; every Y_j is zeroed first (a NaN-filled Y is harmless).  A column's result does not depend on its place in the block nor on
 * its neighbours, bit for bit; entries of X may repeat.  A run-time struct (IGX_FORM_SOURCE) has no batched instantiation yet: its
 * columns go through the single-column kernel one by one inside the call (correct, no faster, colours x nx launches) and
 * IGXGetKernelName says "column by column".
 * Refusals, each decided before the first HIP call, in this order:
 *   1. a null iga, X or Y array, or a null state vector where the operator takes one: IGX_ERR_ARG_WRONG
 *   2. nx outside [1, 48]: IGX_ERR_ARG_OUTOFRANGE
 *   3. a null entry, or an entry (or state vector) of another IGX: IGX_ERR_ARG_WRONG
 *   4. a Y_j that repeats, equals any X_i, or is U or V: IGX_ERR_ARG_WRONG
 *   5. no form set: IGX_ERR_ARG_WRONGSTATE
 *   6. whatever the single action refuses for the space: IGX_ERR_SUP with its reason under the block call's name ("the matrix action
 *      on a block runs where the matrix action runs, and ..."); what it refuses for the form itself (order 3, a boundary branch) comes
 *      under the same name from the launcher.
 * IGXSetBatchedActions(stiff,1) makes IGXEigenSolve apply its operators through these calls: one block call on stiff and one on mass per
 * block in place of m single actions each.  Default 0: the solve is bit for bit the one without the call.  info->actions counts
 * columns either way; the kernel name carries the block action's name and the launch count the block calls' launches. */
#define IGX_ACTION_MAXCOLS 16         /* columns per launch of the block actions; IGXEigenSolve's largest block */
int IGXComputeMatrixActionBlock   (IGX iga,int nx,IGXVec X[],IGXVec Y[]);
int IGXComputeJacobianActionBlock (IGX iga,IGXVec U,int nx,IGXVec X[],IGXVec Y[]);
int IGXComputeIJacobianActionBlock(IGX iga,double a,IGXVec V,double t,IGXVec U,int nx,IGXVec X[],IGXVec Y[]);
int IGXSetBatchedActions(IGX iga,int flag);   /* default 0 */
/* Matrix-free diagonals (what MATOP_GET_DIAGONAL asks of a shell matrix: Jacobi, Chebyshev/Jacobi smoothing, diagonal scaling).
 * D = diag A with A exactly the operator the matching action applies, IGAElementFixJacobian included: a fixed dof holds the number
 * of local elements at its node, and a free field on a node whose other fields are fixed keeps its own entry.  Every mat() is
 * linear in Na and in Nb, and for a form that reads N and grad N only the diagonal factorises over the axes like the action: mat()
 * on the columns of the point's 4 x 4 geometry chain, folded into ten slots, goes back through the 1-D product rows (N^2, N N', N'^2)
 * (vec_sumfact, DIAGONAL) -- no matrix, no index, no probing vectors.  D is zeroed and then assembled like any
 * vector, with the same row numbering, bit-repeatable; on several ranks U and V must hold their ghosts and
 * IGXReduceGhostRows(iga,NULL,D) completes the ghost rows.  Covered: what the actions cover, for forms and run-time structs whose
 * shape features are of first order.  Second-order shape features (Cahn-Hilliard), a boundary-form pass, dim != 3, nsd != dim,
 * order-3 or property forms, nen or nqp > 8, IGX_VEC_SUMFACT=0, an IGXSetKernel choice other than 0 return IGX_ERR_SUP with the reason:
 * there is no fallback kernel.  D == U or V, a vector of another IGX or a null vector: IGX_ERR_ARG_WRONG; no form set:
 * IGX_ERR_ARG_WRONGSTATE.  The dof x dof point-block diagonal: IGXCompute*BlockDiagonal below. */
int IGXComputeMatrixDiagonal   (IGX iga,IGXVec D);                                               /* diag of the matrix of IGXComputeSystem   */
int IGXComputeJacobianDiagonal (IGX iga,IGXVec U,IGXVec D);                                      /* diag of IGXComputeJacobian's J(U)        */
int IGXComputeIJacobianDiagonal(IGX iga,double a,IGXVec V,double t,IGXVec U,IGXVec D);           /* diag of IGXComputeIJacobian's J          */
/* Matrix-free point-block diagonals (what PCPBJACOBI / MatInvertBlockDiagonal ask of a shell matrix): the dof x dof blocks
 * A_(a,i),(a,j) of every node a, A exactly the operator of the matching action and diagonal, IGAElementFixJacobian included: an
 * entry (i,j), i != j, with either field fixed at the node is exactly 0, a fixed (i,i) holds the number of local elements at the
 * node, a free field beside fixed ones keeps its own entries.  The container is nb = dof ordinary IGXVecs of this IGX, one per
 * block column: B[j][node*dof + i] = A_(node,i),(node,j) -- row numbering, IGXReduceGhostRows(iga,NULL,B[j]), IGXRefreshGhosts, the
 * copies and the index lists work on each column unchanged.  The point stage keeps the whole dof x dof tile mat() returns where the
 * diagonal keeps its diagonal, block row by block row, and every field pair goes back through the same product rows (vec_sumfact,
 * DIAGONAL + BLOCK).  The columns are zeroed and assembled in the fixed colour order, bit-repeatable; on several
 * ranks U and V must hold their ghosts and one IGXReduceGhostRows per column completes the owned rows.  Coverage and refusals are
 * the diagonals' (IGX_ERR_SUP with the diagonal's reason under the block diagonal's name); dof <= 8.  nb != dof, a null or repeated
 * entry of B, an entry of another IGX or one that is U or V: IGX_ERR_ARG_WRONG; no form set: IGX_ERR_ARG_WRONGSTATE.
 * IGXBlockDiagonalInvert replaces every local block by its inverse (Gauss-Jordan with partial pivoting, one thread per node; on
 * several ranks reduce and refresh each column first so that every local row holds its complete block).  A block with a zero or
 * non-finite pivot becomes the zero block and is counted in *nsingular, which synchronises the stream; NULL skips the count and
 * the synchronisation.  IGXBlockDiagonalApply: Y_node = B_node X_node for every local row; X == Y or X, Y among B:
 * IGX_ERR_ARG_WRONG. */
int IGXComputeMatrixBlockDiagonal   (IGX iga,int nb,IGXVec *B);
int IGXComputeJacobianBlockDiagonal (IGX iga,IGXVec U,int nb,IGXVec *B);
int IGXComputeIJacobianBlockDiagonal(IGX iga,double a,IGXVec V,double t,IGXVec U,int nb,IGXVec *B);
int IGXBlockDiagonalInvert(IGX iga,int nb,IGXVec *B,int64_t *nsingular /* may be NULL */);
int IGXBlockDiagonalApply (IGX iga,int nb,IGXVec *B,IGXVec X,IGXVec Y);   /* Y_node = B_node X_node */
/* Fast diagonalisation (Sangalli and Tani, SIAM J. Sci. Comput. 38, 2016): a preconditioner for the matrix-free operators whose quality
 * depends on neither the mesh nor the degree.  On the parametric tensor-product space the operator
 *   A0 = alpha M2 x M1 x M0 + beta[0] M2 x M1 x K0 + beta[1] M2 x K1 x M0 + beta[2] K2 x M1 x M0
 * (M_d, K_d the 1-D mass and stiffness matrices of axis d) is diagonal in the basis U2 x U1 x U0 of the 1-D generalised eigenvectors
 * K_d U_d = M_d U_d Lambda_d, U_d^T M_d U_d = I: A0^-1 R = (U2 x U1 x U0) [ (U2^T x U1^T x U0^T) R ./ (alpha + sum_d beta[d] lambda_d) ].
 * IT IGNORES THE GEOMETRY AND THE RATIONAL WEIGHTS: without a geometry it is the exact inverse of IGXComputeMatrixAction's operator for
 * Poisson (alpha = 0, beta = 1) and Mass (alpha = 1, beta = 0), field by field; on a mapped geometry a spectrally equivalent preconditioner.
 * IGXFastDiagSetUp runs after IGXSetUp and is host work only (no HIP call): M_d and K_d come from the axis' own tables (IGXGetBasis: offset,
 * detJac, weight, value[..][0], value[..][1]; a periodic axis wraps), so the inverse is exact for the rule set; any degree, continuity,
 * knot vector and rule size.  The fixed dofs are a union of faces (IGXSetBoundaryValue; never on a periodic axis), so the free dofs of a
 * field are a product of index ranges: per axis and per combination "first / last function fixed" some field uses, those functions are
 * dropped and the eigenproblem is solved by the library's own solver (Cholesky of M_d, cyclic Jacobi); fields with the same combination
 * share the result.  A mode with |alpha + sum_d beta[d] lambda_d| <= 1e-12 max|denominator| (the maximum over all fields) has its reciprocal
 * set to 0, a pseudo-inverse (the constant of pure-Neumann Poisson); *nzeroed (may be NULL) counts them over all fields.  alpha < 0, a
 * beta[d] < 0 and alpha = beta = 0: IGX_ERR_ARG_OUTOFRANGE.  The state belongs to the IGX: a second call replaces it, IGXSetUp drops it,
 * IGXDestroy frees it.
 * IGXFastDiagApply: per field f, Z[free dofs of f] = A0,f^-1 R[free dofs of f] and Z[fixed] = R[fixed] / count, the correctly rounded
 * quotient, count the number of elements at the node (the diagonal IGXComputeMatrixAction and IGXComputeMatrixDiagonal put there).  Fields
 * are independent (the vector Laplacian part of Elasticity, a multi-field Mass).  Z may be R.  Six contractions along the axes of the
 * vector on v_mfma_f64_16x16x4_f64 (fast_diag.hpp), no atomics, bit-repeatable; the device copies of the tables and two
 * work vectors of the local vector's size are made at the first call.  IGXSetTiming / IGXGetLastTiming / IGXGetKernelName cover it.
 * IGXFastDiagGetAxis hands back the eigen-system field `field` uses on `axis`: the index of its first free function, the number m of free
 * functions, Lambda ascending and U column-major m x m (either array may be NULL).
 * IGX_ERR_SUP with a reason that names fast diagonalisation: dim != 3, more than one rank on an axis (the transforms are global along an
 * axis), a fix table (IGXSetFixTable), dof > 8.  IGXFastDiagApply before IGXFastDiagSetUp: IGX_ERR_ORDER; after the set of Dirichlet
 * faces changed since IGXFastDiagSetUp: IGX_ERR_ARG_WRONGSTATE; null, foreign or wrong-sized vectors: IGX_ERR_ARG_WRONG. */
int IGXFastDiagSetUp (IGX iga,double alpha,const double beta[3],int *nzeroed);
int IGXFastDiagApply (IGX iga,IGXVec R,IGXVec Z);              /* Z = P R; Z may be R */
int IGXFastDiagGetAxis(IGX iga,int axis,int field,int *first,int *m,double lambda[],double U[]);

/* Vector algebra on IGXVec, for a caller without PETSc's Vec: what a Krylov iteration needs besides the operators above.  Every call is
 * enqueued on the engine's stream; the vectors of one call must belong to the same IGX (a null or foreign vector: IGX_ERR_ARG_WRONG).
 * Sweeps of 16-byte accesses with a scalar tail over a capped grid (krylov.hpp).  IGXVecAXPBY with b = 0 gives y = a x whatever y held.
 * IGXVecPointwiseDivide gives the correctly rounded quotients.  IGXVecDot and IGXVecNorm2 sum over the rows this rank OWNS (IGXChecksum's
 * rule; on one rank every row) and hand the number back, so they synchronise the stream; on several ranks the caller adds the parts, as
 * for IGXComputeScalar (for the norm: the squares), with IGXCommAllSum where it has no sum of its own.  The sums use no atomics: each workgroup adds its lanes in a fixed tree and stores one
 * partial, the partials are added in index order by a one-workgroup kernel: bitwise repeatable. */
int IGXVecSet  (IGXVec y,double value);
int IGXVecCopy (IGXVec x,IGXVec y);                       /* y = x */
int IGXVecScale(IGXVec y,double a);
int IGXVecAXPBY(IGXVec y,double a,IGXVec x,double b);     /* y = a x + b y */
int IGXVecPointwiseDivide(IGXVec z,IGXVec x,IGXVec d);    /* z = x ./ d, z may be x */
int IGXVecDot  (IGXVec x,IGXVec y,double *s);             /* over the rows this rank owns; synchronises */
int IGXVecNorm2(IGXVec x,double *s);

/* The Krylov loop on the matrix-free operators, resident on the device: A x = b with A the action `op` names at the state (a, V, t, U)
 * -- IGXComputeMatrixAction, IGXComputeJacobianAction (U) or IGXComputeIJacobianAction (a, V, t, U), through the same entry the call
 * itself takes -- by preconditioned CG or right-preconditioned BiCGStab, from the initial guess x holds on entry.  It is the native loop
 * of a caller without PETSc, not a KSP adapter.  The preconditioner: none; IGX_PC_JACOBI, the matching IGXCompute*Diagonal formed by the
 * solve at the same state; IGX_PC_PBJACOBI, the matching IGXCompute*BlockDiagonal formed and inverted by the solve (IGXBlockDiagonalInvert's
 * kernel); IGX_PC_FASTDIAG, the state of the caller's IGXFastDiagSetUp (alpha and beta are a modelling choice; without it: IGX_ERR_ORDER).
 * Stop test, on the recurrence residual: |r|_2 <= max(rtol |b|_2, atol), once per iteration (BiCGStab has no half-step exit).  A solve
 * that does not converge RETURNS 0: info->reason says why -- IGX_DIVERGED_ITS after maxit iterations, IGX_DIVERGED_BREAKDOWN for a zero or
 * non-finite denominator (CG: also p.Ap <= 0), IGX_DIVERGED_NAN for a NaN norm; b = 0 gives x = 0, 0 iterations, IGX_CONVERGED_ATOL.  x on
 * return is the iterate whose norm was tested; history (NULL, or maxit + 1 doubles) receives |r_k|_2, k = 0 .. iterations.
 * The vectors never leave the device: the sweeps between two operator calls are fused, each emits the partial sums the next one needs,
 * alpha, beta and omega are formed on the device from those slabs (krylov.hpp), and the host reads one small record per
 * iteration for the stop test.  Work vectors (4 for CG, 8 for BiCGStab, plus the diagonal or the dof block columns) are allocated at the
 * first solve and kept with the IGX while the method and the preconditioner need the same set; IGXSetUp drops them, IGXDestroy frees them.
 * Bitwise repeatable.  IGXSetTiming / IGXGetLastTiming cover the whole solve (total time, the operators' and preconditioners' own kernel
 * time, launches); IGXGetKernelName gives "krylov(<method>, pc=<..>, <the action's kernel name>, <k> iterations)".
 * On a partition (more than one rank, after IGXCommInitRCCL / IGXCommInitTransport) the same loop runs on every rank, collectively:
 *   contract   b is complete on the rows the rank owns (IGXComputeSystem, then IGXReduceGhostRows); U and V carry their ghosts, as for the
 *              actions.  Of b and of the guess in x only the owned rows are read: every sweep of the loop visits the owned entries alone
 *              (runs of contiguous doubles at a constant stride, krylov.hpp), so a ghost row is never summed and never written by a sweep.
 *   A(in,out)  IGXRefreshGhosts(in); the action; IGXReduceGhostRows(NULL,out): out is complete on the owned rows.
 *   Jacobi     the diagonal, IGXReduceGhostRows, IGXRefreshGhosts, once per solve: no local row holds a partial value.
 *   PBJacobi   every block column, IGXReduceGhostRows and IGXRefreshGhosts per column, then the invert and apply kernels as on one rank.
 *   rank sums  every group of partial sums is added across the ranks before anything reads it: each rank adds its slab in index order,
 *              one group of messages gathers the ranks' sums, and the slab is rewritten to hold rank r's sum in entry r (0 behind the last
 *              rank), so that the kernels that consume it add ((s_0 + s_1) + s_2) + ... -- the same bits on every rank.  alpha, beta,
 *              omega, the record and with them every decision of the host (stop, breakdown, NaN, b = 0) are bit-identical on all ranks.
 *   start      r = b - A(x); one rank sum of {r.r, b.b, the first r.z (CG) or rho (BiCGStab)}.
 *   CG step    p = z + beta p; A(p,Ap); p.Ap, rank sum; x += alpha p, r -= alpha Ap, r.r; z = M r with r.z; rank sum of {r.r, r.z}; the record.
 *   BiCGStab   p; y = M p; A(y,v); rhat.v, rank sum; s; z = M s; A(z,t); {t.s, t.t}, rank sum; x, r with {r.r, the next rho}, rank sum; the record.
 *   end        one IGXRefreshGhosts(x): x holds the solution on the owned rows and their values in its ghosts.
 * info and history are the same bits on every rank, and a second solve gives the same bits.  IGXGetKernelName then ends in
 * "<k> iterations, <R> ranks)".  IGXGetLastTiming's launches then count the sweeps, the operators' and preconditioners' kernels and the two
 * kernels of every rank sum; the pack and unpack kernels of IGXRefreshGhosts / IGXReduceGhostRows and the transport's own are not counted.
 * What the two exchanges refuse in the loop comes back under the solve's name like any operator's refusal.  The exchanges and the rank sums are stream-ordered on the exchange stream; nothing hides them under the
 * sweeps, and there is no pipelined or s-step variant.  A failure on one rank in the middle of the loop (a failed launch) leaves its
 * peers to the transport's timeout.  IGXSolveNonlinear, IGXTimeStep, IGXMultigrid, IGXEigenSolve and the block-vector calls still need one
 * rank on every axis, and so does IGX_PC_FASTDIAG (its solves run along whole axes).
 * IGX_ERR_SUP with a reason that names the Krylov solve: more than one rank on an axis without a communicator (the library has no sum
 * across ranks then), what the ghost-row exchange refuses (a periodic ghost layer that wraps onto its own rank), IGX_PC_FASTDIAG or more
 * than 256 ranks on a partition -- all decided before the first message from what every rank knows alike -- and
 * whatever the action, the diagonal, the block diagonal or fast diagonalisation refuse, with their reason.  x == b, null or foreign
 * vectors, U / V missing where op needs them, x a state vector: IGX_ERR_ARG_WRONG; maxit < 0, a negative tolerance, an unknown method,
 * operator or preconditioner: IGX_ERR_ARG_OUTOFRANGE; before IGXSetUp: IGX_ERR_ORDER; no form set: IGX_ERR_ARG_WRONGSTATE. */
typedef enum { IGX_SOLVE_CG = 0, IGX_SOLVE_BICGSTAB = 1 } IGXSolveMethod;
typedef enum { IGX_OP_MATRIX = 0, IGX_OP_JACOBIAN = 1, IGX_OP_IJACOBIAN = 2 } IGXSolveOperator;
typedef enum { IGX_PC_NONE = 0, IGX_PC_JACOBI = 1, IGX_PC_PBJACOBI = 2, IGX_PC_FASTDIAG = 3 } IGXSolvePC;
typedef enum { IGX_CONVERGED_RTOL = 1, IGX_CONVERGED_ATOL = 2, IGX_DIVERGED_ITS = -1, IGX_DIVERGED_BREAKDOWN = -2, IGX_DIVERGED_NAN = -3 } IGXSolveReason;
typedef struct { int method, op, pc; double a, t; IGXVec V, U; double rtol, atol; int maxit; } IGXSolveSpec;
typedef struct { int iterations, reason; double rnorm0, rnorm, bnorm; } IGXSolveInfo;
int IGXSolve(IGX iga,const IGXSolveSpec *spec,IGXVec b,IGXVec x,IGXSolveInfo *info,double *history /* NULL or [maxit+1]: |r_k|_2 */);
/* EXPERIMENTAL, for measurements only (scripts/solve_ranks_rate.py; like IGXCommLoopbackTest no part of the interface a caller builds on, and
 * free to change or go): the mean time in ms of reps launches of one fused sweep of IGXSolve's loops on vectors
 * of its own, after 3 untimed launches.  runs = 1: the sweep over the owned rows of this IGX's partition (runs of contiguous doubles; needs
 * IGXSetComm and IGXSetUp, no communicator); runs = 0: its contiguous sibling over the same number of entries.  It synchronises.  An
 * unknown sweep or form, reps < 1: IGX_ERR_ARG_OUTOFRANGE; before IGXSetUp: IGX_ERR_ORDER. */
typedef enum { IGX_SWEEP_RESID0 = 0, IGX_SWEEP_DOT, IGX_SWEEP_DOT2, IGX_SWEEP_JACOBI_RZ, IGX_SWEEP_CG_UPDATE, IGX_SWEEP_BICG_XR, IGX_SWEEP_CG_P,
               IGX_SWEEP_BICG_P, IGX_SWEEP_BICG_S, IGX_SWEEP_PDIV, IGX_SWEEP_SET, IGX_SWEEP_COUNT } IGXKrylovSweep;
int IGXKrylovSweepTime(IGX iga,int sweep,int runs,int reps,double *ms);

/* The assembled matrix as an operator, for a caller without PETSc's Mat: the product, the diagonals and the Krylov loop on an IGXMat, however
 * its values got there (any IGXCompute* driver that assembles, any form, dimension, degree or boundary pass: the product only reads them).
 * One rank on every axis: a column node index is then a row index of x (a periodic axis wrapped inside the rank included).  Everything is
 * enqueued on the engine's stream; nothing here synchronises but IGXMatSolve's record reads.
 * IGXMatMult: y = A x, y[r bs + i] = sum_k sum_j val[(browptr[r] + k) bs^2 + i bs + j] x[col(k) bs + j].  y is overwritten (NaN in y on entry
 *   does not survive); x is read only.  One launch of mat_mult (mat_ops.hpp): a sub-group of 8, 16 or 32 lanes or one wavefront per row, by
 *   the longest row; val is read once in 16-byte accesses; no atomics, the lanes of a row add in a fixed tree: bitwise repeatable, and a row's
 *   result depends on that row's values and the x it reads alone.  The column of an entry comes from the per-axis tables (the default
 *   where a sub-group takes a row) or from bcolidx (the default where a wavefront does); IGX_MATMULT_INDEX=0 / =1 in the environment when the IGX is created picks the tables /
 *   bcolidx for every block size (both give the same bits; profiles/matmult.txt has their times).  IGXGetKernelName starts with "mat_mult";
 *   IGXGetLastTiming reports one launch.
 * IGXMatGetDiagonal: d[r bs + i] = A[r][r][i][i].  IGXMatGetBlockDiagonal: nb = bs vectors, B[j][r bs + i] = A[r][r][i][j] -- the layout of
 *   IGXCompute*BlockDiagonal, so IGXBlockDiagonalInvert / IGXBlockDiagonalApply take them unchanged.  Copies, bit for bit, one launch each.
 * IGXMatSolve: IGXSolve's loop (the same code) with A(in, out) = IGXMatMult.  Of the spec it reads method, pc, rtol, atol and maxit; op, a, t,
 *   V and U are IGNORED (the matrix is what it is).  The preconditioner: none; IGX_PC_JACOBI from IGXMatGetDiagonal; IGX_PC_PBJACOBI from
 *   IGXMatGetBlockDiagonal and IGXBlockDiagonalInvert's kernel; IGX_PC_FASTDIAG, the state of the caller's IGXFastDiagSetUp on the matrix's
 *   IGX (without it: IGX_ERR_ORDER).  Stop test, outcomes, b = 0, maxit = 0, history, info and bit-repeatability are IGXSolve's.
 *   IGXGetKernelName gives "krylov(<method>, pc=<..>, mat_mult(...), <k> iterations)".  The work vectors are IGXSolve's store on the IGX,
 *   replaced under the same rule: a matrix-free solve before or after a matrix solve is unaffected.
 * Refusals, in this order, each decided before any HIP call:
 *   1. a null A, x or y (d; B; spec, b or x): IGX_ERR_ARG_WRONG.  IGXMatGetBlockDiagonal then: nb != bs, a null entry of B: IGX_ERR_ARG_WRONG
 *   2. a vector of another IGX than A's; a matrix made before the last IGXSetUp of its IGX (its pattern is that set-up's, whether or not the
 *      sizes changed); a vector whose size is not that of the IGX's present space: IGX_ERR_ARG_WRONG
 *   3. x == y (IGXMatSolve: x == b; IGXMatGetBlockDiagonal: an entry of B given twice): IGX_ERR_ARG_WRONG
 *   4. more than one rank on an axis: IGX_ERR_SUP with a reason that names the call and says "one rank"
 *   5. IGXMatSolve alone, with IGXSolve's codes: a negative or NaN tolerance, maxit < 0, an unknown method or preconditioner:
 *      IGX_ERR_ARG_OUTOFRANGE; IGX_PC_FASTDIAG without IGXFastDiagSetUp: IGX_ERR_ORDER; then whatever fast diagonalisation refuses, with its
 *      reason under the solve's name.
 * Out of scope: several ranks, the transposed product, y += A x, the stored matrix as the operator of the other solve loops. */
int IGXMatMult(IGXMat A,IGXVec x,IGXVec y);
int IGXMatGetDiagonal(IGXMat A,IGXVec d);
int IGXMatGetBlockDiagonal(IGXMat A,int nb,IGXVec B[]);
int IGXMatSolve(IGXMat A,const IGXSolveSpec *spec,IGXVec b,IGXVec x,IGXSolveInfo *info,double *history /* NULL or [maxit+1]: |r_k|_2 */);

/* The product on a block of vectors and the eigen solve on it.
 * IGXMatMultBlock: Y[j] = A X[j] for j < nx, 1 <= nx <= 48 (the block-vector limit of IGXCompute*ActionBlock).  The block is cut into chunks
 *   of NC columns, NC = 8 at bs <= 2, 4 at bs = 3 and 4, 2 at bs >= 5; what is left after the full chunks goes to the next narrower widths
 *   (NC/2, NC/4, .. 2) and a last single column to IGXMatMult's own kernel.  One launch of mat_mult_block (mat_ops.hpp) per chunk reads val,
 *   browptr, bcolidx and the axis tables once for all its columns.  IGXMatMultBlockPlan gives the widths of the launches of a (bs, nx) in
 *   order (widths: NULL or [nx]); it touches no device.  Column j of the result is BIT FOR BIT what IGXMatMult(A, X[j], Y[j]) stores: it does
 *   not depend on nx, on the column's place in the block, on the chunking or on the other columns (a NaN column of X makes its own column of Y
 *   NaN and no other).  Y is overwritten and never read; no atomics.  A vector may appear twice in X.  IGXGetLastTiming reports the number of
 *   chunk launches; IGXGetKernelName gives "mat_mult_block(bs=<bs>, <lanes per row>, columns from <the axis tables|bcolidx>, NC=<NC>)";
 *   IGX_MATMULT_INDEX picks the index variant as for IGXMatMult.
 *   Refusals, in this order, each decided before any launch: 1. a null A, X or Y: IGX_ERR_ARG_WRONG; 2. nx outside [1, 48]:
 *   IGX_ERR_ARG_OUTOFRANGE; 3. a null entry: IGX_ERR_ARG_WRONG; 4. IGXMatMult's rule 2 on all 2 nx vectors (foreign, stale, wrong size):
 *   IGX_ERR_ARG_WRONG; 5. a vector twice in Y; 6. a vector of X that is also in Y: IGX_ERR_ARG_WRONG; 7. more than one rank on an axis:
 *   IGX_ERR_SUP, in IGXMatMult's words under this call's name; 8. a block size above 8: IGX_ERR_SUP.
 * IGXMatEigenSolve: IGXEigenSolve's contract and loop (below, line by line: the same code) with A(block) and B(block) one IGXMatMultBlock
 *   each on the stored K and M (M == NULL: B = I).  The vectors belong to K's IGX; M comes from the same IGX or from another one on the same
 *   space.  T: none; IGX_PC_JACOBI / IGX_PC_PBJACOBI read out of K as in IGXMatSolve; IGX_PC_FASTDIAG the state of IGXFastDiagSetUp on K's
 *   IGX.  The start block's fixed rows (the Dirichlet faces of K's IGX) are zeroed first and stay exactly zero because a fixed row of the
 *   assembled K and M holds its diagonal alone (the element count) and a fixed column is zero in every other row.  Any dimension, degree and form the assembly takes: the loop needs nothing three-dimensional.
 *   Both matrices must be symmetric: the caller's responsibility.  info->actions counts columns (2 m per iteration with M, m without);
 *   IGXGetKernelName gives "eigen(lobpcg, block <m>, pc=<..>, mat_mult_block(...), <k> iterations)"; the work vectors are IGXEigenSolve's
 *   store on K's IGX, replaced under the same rule.
 *   Refusals, in this order, before the first HIP call: 1. a null K, spec, X, lambda or info: IGX_ERR_ARG_WRONG; 2. the spec's ranges
 *   (IGX_ERR_ARG_OUTOFRANGE) and nx != block (IGX_ERR_ARG_WRONG), as in IGXEigenSolve; 3. a null entry of X, then IGXMatMult's rule 2 for K
 *   and X, an entry of X given twice, then rule 2 for M: IGX_ERR_ARG_WRONG; 4. M's IGX differs from K's in dim, dof, then per axis degree,
 *   knots, periodicity, then the Dirichlet faces per field, then the stream; then a block size or pattern that differs: IGX_ERR_ARG_WRONG;
 *   5. more than one rank on an axis: IGX_ERR_SUP ("one rank"); 6. a fix table on either IGX: IGX_ERR_SUP; 7. a block size above 8:
 *   IGX_ERR_SUP; 8. IGX_PC_FASTDIAG: what fast diagonalisation itself refuses (dim != 3 among it) with its reason under this call's name:
 *   IGX_ERR_SUP; then no IGXFastDiagSetUp on K's IGX: IGX_ERR_ORDER.
 * Out of scope: several ranks, the transposed product, Y += A X, the block product inside IGXMatSolve, locking, interior eigenvalues. */
int IGXMatMultBlock(IGXMat A,int nx,IGXVec X[],IGXVec Y[]);
int IGXMatMultBlockPlan(int bs,int nx,int *nchunks,int widths[] /* NULL or [nx] */);

/* The Newton loop on the matrix-free operators, resident on the device: G(x) = 0 from the guess x holds on entry, for the nonlinear forms
 * (Bratu, Cahn-Hilliard, NS-VMS, Bratu as IFunction).  op = IGX_OP_JACOBIAN: G(U) = IGXComputeFunction(U), dG/dU the Jacobian at U.
 * op = IGX_OP_IJACOBIAN: G(U) = IGXComputeIFunction(a, a U + W, t, U), dG/dU = IGXComputeIJacobian(a, a U + W, t, U) -- with a = 1/dt and
 * W = -U_n/dt one call is a backward-Euler step, with other constants a generalized-alpha stage.  The residual goes through the entry
 * IGXComputeFunction / IGXComputeIFunction take, the linear solve is IGXSolve (method, pc, lin_atol, lin_maxit are its; its rtol is eta).
 * It is the native loop of a caller without PETSc, not a SNES adapter.  |.| is the 2-norm.
 * Start.  F = G(x), f = |F|, history[0] = f.  In this order: f is NaN: IGX_NEWTON_DIVERGED_FNORM_NAN; f <= atol:
 *   IGX_NEWTON_CONVERGED_FNORM_ABS with 0 iterations and x untouched bit for bit; maxit == 0: IGX_NEWTON_DIVERGED_MAX_IT.
 * Iteration k, the linear solve.  eta = lin_rtol under IGX_FORCING_CONSTANT.  Under IGX_FORCING_EW2 (Eisenstat-Walker, choice 2):
 *   eta_0 = lin_rtol, eta_k = 0.9 (f_k / f_{k-1})^2; if 0.9 eta_{k-1}^2 > 0.1, eta_k is not below that value; eta_k is at most 0.9.
 *   d = 0 (IGXVecSet's kernel); IGXSolve on J(x) d = F with rtol = eta, atol = lin_atol, maxit = lin_maxit at the state U = x and, for
 *   IGX_OP_IJACOBIAN, V = a x + W.  IGX_DIVERGED_BREAKDOWN or IGX_DIVERGED_NAN of that solve: IGX_NEWTON_DIVERGED_LINEAR_SOLVE, x stays the
 *   current iterate.  IGX_DIVERGED_ITS is an inexact step and is used as it is.
 * Iteration k, the line search.  lambda = 1.  Trial: x_t = x - lambda d, F_t = G(x_t), f_t = |F_t|.  IGX_LINESEARCH_BASIC accepts the first
 *   trial unless f_t is NaN: that gives IGX_NEWTON_DIVERGED_FNORM_NAN with x restored to the last accepted iterate bit for bit.
 *   IGX_LINESEARCH_BT accepts when f_t <= (1 - 1e-4 lambda) f (a non-finite f_t is not accepted); otherwise lambda /= 2, at most
 *   max_backtracks times; when the halvings are exhausted: IGX_NEWTON_DIVERGED_LINE_SEARCH with x restored bit for bit.
 * After an accepted trial.  snorm = lambda |d|, xnorm = |x|; the accepted F_t is the next F (no second evaluation); ++iterations,
 *   history[k+1] = f.  In this order: f is NaN: IGX_NEWTON_DIVERGED_FNORM_NAN; f <= atol: IGX_NEWTON_CONVERGED_FNORM_ABS; f <= rtol fnorm0:
 *   IGX_NEWTON_CONVERGED_FNORM_RELATIVE; snorm <= stol xnorm: IGX_NEWTON_CONVERGED_SNORM_RELATIVE; iterations >= maxit:
 *   IGX_NEWTON_DIVERGED_MAX_IT.
 * A solve that does not converge RETURNS 0: info->reason says why.  A call that returns an error code (a refusal passed on by the residual
 * or by IGXSolve in the middle of the loop) leaves x the last accepted iterate too.  info: linear_iterations is the sum over the inner solves (linear_its,
 * NULL or maxit ints, receives each), last_linear_reason the last one's IGXSolveReason, backtracks the halvings over the whole call,
 * function_evaluations every G formed: 1 + iterations + backtracks, and one more where the call ends on a trial that was not accepted.
 * Between two operator calls a trial is one sweep (newton.hpp): it saves the accepted iterate, forms x - lambda d in place
 * and V = a x + W (the rounded product plus W, never contracted) and emits the partial sums of d.d and x.x; the host reads one record of
 * three sums per function evaluation.  No atomics: bitwise repeatable.  Work vectors (F, F_t, d, the saved iterate, V) are kept with the
 * IGX like IGXSolve's; IGXSetUp drops them, IGXDestroy frees them.  IGXSetTiming / IGXGetLastTiming cover the whole call (total time, the
 * operators' kernel time summed over residuals and inner solves, launches); IGXGetKernelName gives
 * "newton(<basic|bt>, <the last inner solve's krylov(...) name>, <k> iterations)".
 * Refusals, decided before the first HIP call as in IGXSolve.  IGX_ERR_ARG_WRONG: a null spec or x, a foreign or wrong-sized vector, W
 * missing or W == x for IGX_OP_IJACOBIAN.  IGX_ERR_ARG_OUTOFRANGE: op == IGX_OP_MATRIX, an unknown op, method, pc, linesearch or forcing, a
 * negative or NaN tolerance, a negative maxit, lin_maxit or max_backtracks.  IGX_ERR_ORDER: before IGXSetUp; IGX_PC_FASTDIAG without
 * IGXFastDiagSetUp.  IGX_ERR_ARG_WRONGSTATE: no form set.  IGX_ERR_SUP with a reason that names the Newton solve: more than one rank on an
 * axis; whatever IGXSolve, the action or the vector driver refuse is passed on with their reason. */
typedef enum { IGX_NEWTON_CONVERGED_FNORM_ABS = 2, IGX_NEWTON_CONVERGED_FNORM_RELATIVE = 3, IGX_NEWTON_CONVERGED_SNORM_RELATIVE = 4,
               IGX_NEWTON_DIVERGED_LINEAR_SOLVE = -3, IGX_NEWTON_DIVERGED_FNORM_NAN = -4,
               IGX_NEWTON_DIVERGED_MAX_IT = -5, IGX_NEWTON_DIVERGED_LINE_SEARCH = -6 } IGXNewtonReason;   /* SNESConvergedReason's numbers */
typedef enum { IGX_LINESEARCH_BASIC = 0, IGX_LINESEARCH_BT = 1 } IGXNewtonLineSearch;
typedef enum { IGX_FORCING_CONSTANT = 0, IGX_FORCING_EW2 = 1 } IGXNewtonForcing;
typedef struct {
  int op;                       /* IGX_OP_JACOBIAN or IGX_OP_IJACOBIAN (IGX_OP_MATRIX: IGX_ERR_ARG_OUTOFRANGE) */
  double a, t; IGXVec W;        /* IJACOBIAN only: G(U) = IFunction(a, a U + W, t, U); dG/dU is IJacobian(a, a U + W, t, U) */
  int method, pc;               /* of the inner IGXSolve */
  double lin_rtol, lin_atol; int lin_maxit;
  int forcing;
  double rtol, atol, stol; int maxit;
  int linesearch, max_backtracks;
} IGXNewtonSpec;
typedef struct { int iterations, reason, linear_iterations, function_evaluations, backtracks, last_linear_reason;
                 double fnorm0, fnorm, snorm, xnorm; } IGXNewtonInfo;
int IGXSolveNonlinear(IGX iga,const IGXNewtonSpec *spec,IGXVec x,IGXNewtonInfo *info,
                      double *history /* NULL or [maxit+1]: |F_k|_2 */,int *linear_its /* NULL or [maxit] */);

/* The generalized-alpha time loop on the Newton solve, resident on the device: F(t, U, dU/dt) = 0, first order in time, for the forms with an
 * IFunction (Cahn-Hilliard, NS-VMS, Bratu as IFunction), from U = U_n and V = V_n = dU/dt at t0.  The scheme is (alpha_m, alpha_f, gamma):
 * the radius parametrisation of the reference's demos is alpha_m = (3 - rho) / (2 (1 + rho)), alpha_f = 1 / (1 + rho), gamma = 1/2 + alpha_m -
 * alpha_f (demo/CahnHilliard3D.c:281-287, demo/NavierStokesVMS.c:397-401: rho = 0.5); (1, 1, 1) is backward Euler.  It is the native loop of
 * a caller without PETSc, not a TS adapter.  fl(.) is one rounding to double; no product is contracted with a sum.
 * State.  t = t0, h = dt, steps = 0; U0, V0 the accepted state (copies of U and V); with resume = 0 no U_{n-1} is held.
 *   max_steps == 0: IGX_TS_CONVERGED_STEPS, and t0 == max_time: IGX_TS_CONVERGED_TIME, both with nothing launched and U, V untouched.
 * Step n -> n+1 begins with rejections = 0 (the limit max_rejections is per step) and tries attempts until one is accepted:
 * Attempt.  p = h (the proposed step).  If max_time - t <= (1 + 1e-9) h the attempt is shortened to end at max_time: h = max_time - t
 *   (exempt from dt_min).  That is t + h > max_time, and also a step that would end within 1e-9 h before max_time: the remainder it would
 *   leave is the rounding of t, and a step of that size divides rounding noise by h in V1.
 *   Stage (one sweep, ts_stage).  On the host a = alpha_m / (alpha_f gamma h) and c0 = 1 - alpha_m / gamma.
 *     W_i = fl(fl(c0 V0_i) - fl(a U0_i)), x_i = U0_i (the stage guess).
 *   Solve.  IGXSolveNonlinear with the caller's newton spec, op = IGX_OP_IJACOBIAN, that a, t = t_n + alpha_f h, W, on x.  The stage unknown
 *     is x = U_{n+alpha_f}; V = a x + W is then V_{n+alpha_m} (an identity: with U_{n+af} = U0 + af (U1 - U0), V1 = (U1 - U0) / (gamma h) +
 *     (1 - 1/gamma) V0 and V_{n+am} = V0 + am (V1 - V0) one gets V_{n+am} = a (x - U0) + (1 - am/gamma) V0).
 *   A negative IGXNewtonReason is a failed attempt (logged with wlte = -1).  adapt == 0: IGX_TS_DIVERGED_NONLINEAR_SOLVE.  Otherwise
 *     ++rejections, h = h / 4; rejections > max_rejections or h < dt_min: IGX_TS_DIVERGED_NONLINEAR_SOLVE; else the next attempt.
 *   Update (one sweep, ts_update) into two trial vectors, with c1 = 1 / alpha_f, c2 = 1 / (gamma h), c3 = 1 - 1 / gamma from the host:
 *     U1_i = fl(U0_i + fl(c1 fl(x_i - U0_i))),  V1_i = fl(fl(c2 fl(U1_i - U0_i)) + fl(c3 V0_i)),
 *     and the partial sums of U1 . U1.  An estimate exists when adapt != 0 and a U_{n-1} is held (not on the first step of a fresh start).
 *     Then, with r = 1 + h_{n-1} / h and d1 = r, d2 = r - 1, d3 = r (r - 1) from the host, the same sweep forms the second-order
 *     backward-difference estimate on unequal steps, e_i = fl(fl(fl(U1_i / d1) - fl(U0_i / d2)) + fl(Uprev_i / d3)) (correctly rounded
 *     quotients), and emits the partial sums of q_i^2, q_i = fl(e_i / fl(adapt_atol + fl(adapt_rtol max(|U1_i|, |fl(U1_i + e_i)|)))).
 *     The host reads ONE record of the two sums; unorm = sqrt(U1 . U1), wlte = sqrt(sum / n), n the vector's length.  No estimate: wlte = -1.
 *   unorm or wlte is NaN: IGX_TS_DIVERGED_NAN (logged, not accepted).
 *   No estimate: the attempt is accepted and the next step proposes p again (growth starts from the second step: start small).
 *   With an estimate: fac = min(10, max(0.1, 0.9 / sqrt(wlte))), 10 for wlte == 0.  wlte <= 1 accepts, and the next step proposes
 *     min(dt_max, max(dt_min, fac h)) -- or p again where the attempt was shortened.  Otherwise ++rejections, h = fac h;
 *     rejections > max_rejections or h < dt_min: IGX_TS_DIVERGED_STEP_REJECTED; else the next attempt.
 * Acceptance.  Uprev <- U0 <- U1 and V0 <- V1 by pointer among the work vectors, h_{n-1} = h; t += h (t = max_time exactly where the
 *   attempt was shortened); ++steps; dt_last = h; h = the next proposal.  t == max_time: IGX_TS_CONVERGED_TIME; else steps == max_steps:
 *   IGX_TS_CONVERGED_STEPS.
 * Return.  U and V receive the last accepted state, once (a failed or rejected attempt never touches it: a call that diverges hands back
 *   the last accepted state bit for bit, with every step accepted before it).  A call that does not converge RETURNS 0: info->reason says
 *   why.  info: steps, rejections and attempts over the whole call, the sums of the Newton solves' iterations, linear iterations and function
 *   evaluations, t, dt_last (the last accepted h, 0 for none), dt_next (the h the next step would propose: pass it as dt to continue),
 *   unorm = |U|_2 of the last accepted step (0 for none).  log (NULL, or nlog records) receives one record per ATTEMPT: t the time the
 *   attempt starts from, dt its h, wlte, accepted, and the Newton solve's iterations, reason and linear iterations; attempts past nlog
 *   are counted in info->attempts but not logged.
 * resume = 1 continues the previous call: its U_{n-1} and h_{n-1} are kept with the IGX, so the estimate is available at once; t0 and dt
 *   are still the caller's (pass info->t and info->dt_next).  Six steps in one call and three plus three with resume give the same bits.
 *   IGX_ERR_ORDER when the IGX holds none: no earlier call that accepted a step, after IGXSetUp, or a vector length that differs.
 * What the stepper does not do.  It does not form V_0: the caller gives it.  It does not change form parameters (the dt in NS-VMS's tau
 * stays what the caller set).  U must hold the Dirichlet values on entry: the residual pins the stage value, and with alpha_f < 1 a wrong
 * boundary value in U_n is extrapolated into U_{n+1} (PETSc's TSALPHA behaves the same way).  dt_min limits reductions only: the caller's
 * dt and the shortened last step are taken as they are.  Second-order-in-time forms are out of scope.
 * Work vectors (W, x, three rotating U and two rotating V) are kept with the IGX like the Newton solve's; IGXSetUp drops them, IGXDestroy
 * frees them.  No atomics: bitwise repeatable (timestep.hpp).  IGXSetTiming / IGXGetLastTiming cover the whole call (total
 * time, the operators' kernel time summed over the Newton solves, launches); IGXGetKernelName gives
 * "timestep(am=.., af=.., g=.., <the last newton(...) name>, <k> steps, <r> rejections)".
 * Refusals, decided before the first HIP call as in IGXSolveNonlinear.  IGX_ERR_ARG_WRONG: a null spec, U or V, a foreign or wrong-sized
 * vector, U == V.  IGX_ERR_ARG_OUTOFRANGE with a message that names IGXTimeStep and the member: newton.op != IGX_OP_IJACOBIAN; alpha_m,
 * alpha_f or gamma not finite or <= 0; dt <= 0 or NaN; max_time < t0 (or NaN); a negative max_steps or max_rejections; a negative or NaN
 * adapt_rtol, adapt_atol, dt_min or dt_max; dt_max < dt_min; adapt with both tolerances 0; and what IGXSolveNonlinear refuses in newton.
 * IGX_ERR_ORDER: before IGXSetUp; resume without a kept state; IGX_PC_FASTDIAG without IGXFastDiagSetUp.  IGX_ERR_ARG_WRONGSTATE: no form
 * set.  IGX_ERR_SUP with a reason that names the time stepper: more than one rank on an axis; whatever IGXSolveNonlinear refuses in the
 * loop is passed on with its reason under the stepper's name, and U, V hold the last accepted state (the entry state where no step was
 * accepted before it). */
typedef enum { IGX_TS_CONVERGED_TIME = 1, IGX_TS_CONVERGED_STEPS = 2,
               IGX_TS_DIVERGED_NONLINEAR_SOLVE = -1, IGX_TS_DIVERGED_STEP_REJECTED = -2, IGX_TS_DIVERGED_NAN = -3 } IGXTimeStepReason;
typedef struct {
  double alpha_m, alpha_f, gamma;      /* the scheme */
  double t0, dt, max_time; int max_steps;
  int adapt; double adapt_rtol, adapt_atol, dt_min, dt_max; int max_rejections;   /* per step */
  int resume;                          /* 0: a fresh start; 1: continue the previous call (its U_{n-1} and h_{n-1} are kept with the IGX) */
  IGXNewtonSpec newton;                /* op must be IGX_OP_IJACOBIAN; its a, t and W are the stepper's and are ignored */
} IGXTimeStepSpec;
typedef struct { double t, dt, wlte; int accepted, newton_iterations, newton_reason, linear_iterations; } IGXTimeStepLog;   /* one per ATTEMPT */
typedef struct { int steps, reason, rejections, attempts, newton_iterations, linear_iterations, function_evaluations;
                 double t, dt_last, dt_next, unorm; } IGXTimeStepInfo;
int IGXTimeStep(IGX iga,const IGXTimeStepSpec *spec,IGXVec U,IGXVec V,IGXTimeStepInfo *info,IGXTimeStepLog *log,int nlog);

/* Evaluation of a discrete field at arbitrary points, on the device (IGAProbe, src/petigaprobe.c; known-answer test test/IGAProbe.c): what
 * the field an IGXVec holds -- the result of IGXSolve, IGXSolveNonlinear, IGXTimeStep -- is at a point, where coefficients are not values.
 * IGXProbeCreate copies npts parametric points u [npts][dim] to the device and locates them there once, one launch for all points: per
 *   axis the span of IGA_FindSpan, U[k] <= u < U[k+1] by binary search in the knot vector; the upper end of the axis belongs to the last
 *   non-empty span, so at an interior knot the evaluation is from the right, and a knot of multiplicity > 1 never yields an empty span.
 *   order (0..3) is the highest derivative a later call may ask for (IGAProbeSetOrder).  The probe belongs to the IGX under IGXVec's
 *   lifetime rules (destroy it before the IGX); after another IGXSetUp it is stale and every call on it returns IGX_ERR_ORDER.  npts = 0 is
 *   legal, launches nothing and touches no device.
 * IGXProbeEvaluate: out [npts][dof][dim^der], entry [pt][c][i..] the derivative der (0..order) of field c, the full tensors in the layout of
 *   IGA_GetGrad / Hess / Der3 (src/petigaprobe.c:456-462).  Derivatives are with respect to the physical coordinates when a geometry with
 *   nsd = dim is set (rationalise -> geometry map -> inverse map -> shape functions, src/petigaprobe.c:346-423), parametric otherwise (no
 *   geometry, or nsd != dim as in the reference); rational weights enter whenever they are set.  One launch on the engine's stream, one
 *   point per lane over a grid capped at 2048 workgroups of 64 lanes (131072 points per turn of its grid-stride loop); the 1-D rows of
 *   values and derivatives up to the third are computed on the device at the point, the quotient rule and the chain through the map act
 *   once per point on the partial sums (probe.hpp).  The sum over basis functions runs in an order that depends on the
 *   point alone and no atomics are used: a point's result is bit-identical wherever it stands in the list, whatever the other points are,
 *   and from run to run.  The call copies the result back and synchronises.  IGXSetTiming / IGXGetLastTiming give the total time and the
 *   kernel's own time; IGXGetKernelName gives "probe(<dim>d, p=<..>, order=<der>, <identity|polynomial|rational>, <npts> points)".
 * IGXProbeGeomMap: x [npts][nsd], the geometry map at the points; without a geometry [npts][dim] = u (IGAProbeGeomMap).  IGXProbeGetInfo
 *   tells nsd to a caller whose geometry came from a file (IGXRead), with the probe's npts and order.  IGXProbeCreate and IGXProbeGeomMap
 *   are timed like IGXProbeEvaluate; a call on a probe of no points reports 0 ms and 0 launches.
 * Several ranks: a point is evaluated by the one rank whose element box (elem_start, elem_width) holds its element; every other rank
 *   writes zeros for it and IGXProbeGetLocal reports local = 0 there (the reference's non-collective behaviour, made unique), so adding
 *   out over the ranks gives the full answer and the local flags partition the points.  U must hold its ghosts (IGXRefreshGhosts), as for
 *   the actions; a periodic axis wrapped inside a rank goes through the row map the kernels use.
 * Refusals, all decided before the first HIP call, each reason naming the probe.  IGX_ERR_ARG_WRONG: a null pointer; a vector of another
 *   IGX or of another size (a vector of the probe's IGX changes size only through another IGXSetUp, after which the probe is stale and
 *   IGX_ERR_ORDER comes first: the size check guards a route added later).  IGX_ERR_ARG_OUTOFRANGE: order outside 0..3 (order 4 by name: the device keeps derivative slots 0..3); der
 *   outside 0..order; npts < 0; a point that is NaN or outside [U[p], U[n+1]] on some axis (the message gives the point's index and the
 *   axis).  IGX_ERR_ORDER: before IGXSetUp; a stale probe.  IGX_ERR_SUP: a degree above 7 on some axis. */
typedef struct _p_IGXProbe *IGXProbe;
int IGXProbeCreate  (IGX iga,int order,int64_t npts,const double *u /* host [npts][dim], parametric */,IGXProbe *prb);
int IGXProbeGetLocal(IGXProbe prb,int64_t *nlocal,unsigned char *local /* NULL or host [npts]: 1 = evaluated on this rank */);
int IGXProbeGeomMap (IGXProbe prb,double *x /* host [npts][nsd]; no geometry: [npts][dim] = u */);
int IGXProbeGetInfo (IGXProbe prb,int64_t *npts,int *order,int *nsd /* columns of IGXProbeGeomMap's x: the geometry's nsd, or dim */,
                     int64_t *points_per_turn /* of the kernel's grid-stride loop */);   /* any pointer may be NULL */
int IGXProbeEvaluate(IGXProbe prb,IGXVec U,int der,double *out /* host [npts][dof][dim^der] */);
int IGXProbeDestroy (IGXProbe *prb);

/* Transfer between nested spline spaces: prolongation and restriction of vectors.  No entry of the reference (its DMRefine_IGA /
 * DMCreateInterpolation_IGA are commented out in src/petigadm.c; the contract is the mathematical one below).
 * The pair: two set-up IGX, coarse and fine, with the same dim and dof and, on every axis, the same degree, the same periodicity and the
 *   same end knots (a clamped axis: its first and last p+1 knots; a periodic axis: U[p] and U[m-p]); every knot of the coarse axis appears
 *   in the fine axis with at least its multiplicity (h-refinement by knot insertion: several knots in one span, raised multiplicity, axes
 *   refined by different amounts or not at all).  Per axis there is then one nf x nc matrix T with B^c_j = sum_i T[i][j] B^f_i; a row has
 *   at most p+1 non-zeros, consecutive, non-negative, of sum 1; an unrefined axis gives the identity with entries exactly 1.0 and a
 *   clamped axis unit rows at both ends.  With vectors in the natural numbering [n2][n1][n0][dof], P = T2 (x) T1 (x) T0 (x) I_dof.
 * IGXTransferCreate builds the tables on the host, every row directly by de Boor's triangle on the blossom (p levels of convex
 *   combinations: rounding error O(p u) however many knots were inserted; no chain of single insertions), and touches no device; the
 *   first Prolong / Restrict uploads them.  On a periodic axis the rows are built on the unwrapped knot sequence of one period,
 *   U[p+1 .. p+nnp], and folded through the row map the kernels use (IGXMatGetAxisMaps: function i >= nnp is function i - nnp); the
 *   vectors hold the unique functions only.  The transfer belongs to both IGX under IGXVec's lifetime rules (destroy it before either);
 *   after another IGXSetUp on either one it is stale and every call on it returns IGX_ERR_ORDER.
 * IGXTransferGetAxis (host only): the table of one axis (0..2; an axis beyond dim is the 1 x 1 identity): nf, nc, width = p+1, and per fine
 *   row the first non-zero column first[i], the band's length count[i] and the entries T[i][0..count-1], zero past count.  On a periodic
 *   axis first[i] lies in [0, nc) and entry k belongs to column (first[i] + k) mod nc.  Any pointer may be NULL.
 * IGXTransferProlong: xf = P xc, or xf += P xc with add != 0 (a coarse-grid correction), one rounding for the addition.
 * IGXTransferRestrict: rc = P^T rf, the transpose that carries residuals (not an injection, not a projection).
 *   No Dirichlet masking happens inside: boundary rows move like any others.  The end rows of a clamped axis are unit rows, so a coarse
 *   vector's boundary values are copied along that axis; a value that is constant over the face arrives bit for bit where its products
 *   with the other axes' entries are exact (zero always; values of few bits on dyadic refinements), else within the rounding of a convex
 *   combination of equal numbers.  A multigrid caller zeroes the fixed rows of a restricted residual itself.
 *   On a rational geometry the library's basis is rational, R_j = w_j N_j / W: the vector of the SAME function on the fine space is
 *   (P (w_c * x_c)) / w_f entry by entry with the two nets' weights (the fine net being the refinement of the coarse one); P x_c itself is
 *   the same function only where the weights are constant.  The transfer never looks at a geometry.
 *   Work is enqueued on the FINE IGX's stream and both IGX must have the same stream set; nothing synchronises unless timing is on.
 *   Prolong runs one fused kernel where a box's coarse footprint fits its LDS budget (boxes of 16 x 8 x 8 fine rows, 64 KiB), else one
 *   pass per refined axis; Restrict runs one gather pass per refined axis (a coarse row sums over its fine rows in ascending order: rows
 *   of any length, no atomics).  Both are bit-repeatable, an entry does not depend on the box that computed it, identity axes add
 *   nothing, and a transfer without any refinement is a bit-for-bit copy both ways (petiga_amd/csrc/transfer.hpp).
 *   IGXSetTiming / IGXGetLastTiming / IGXGetKernelName on the fine IGX report the call (its own figures, as after a solve loop):
 *   "transfer_prolong(3d, p=3,3,3, 17x17x17 -> 33x33x33, dof 1, fused)" or "..., axis passes)", "transfer_restrict(... 33x33x33 -> 17x17x17 ...)".
 * IGXTransferSetPath (beyond the five calls of the contract): 0 automatic, 1 the fused kernel (IGX_ERR_SUP where the footprint does not
 *   fit), 2 the axis passes; IGXTransferGetInfo: the box's fine rows per axis, the fused kernel's LDS bytes, whether Prolong runs fused.
 * Refusals, all decided before the first HIP call, each reason naming the transfer, in this order.  IGXTransferCreate: a null pointer
 *   (IGX_ERR_ARG_WRONG); either IGX before IGXSetUp (IGX_ERR_ORDER); different dim, dof, then per axis degree, periodicity, then different
 *   streams (IGX_ERR_ARG_WRONG); more than one rank on an axis of either IGX, a degree above 7, a non-periodic axis that is not clamped
 *   (IGX_ERR_SUP); spaces not nested (IGX_ERR_ARG_OUTOFRANGE: the message gives the axis and the first coarse knot that is missing or short
 *   of multiplicity, or says that the end knots differ).  Prolong / Restrict: a null transfer (IGX_ERR_ARG_WRONG); a stale transfer
 *   (IGX_ERR_ORDER); a null vector, a vector of the wrong IGX, of the wrong size, the same vector twice, different streams
 *   (IGX_ERR_ARG_WRONG).  GetAxis / SetPath / GetInfo: null, stale, then the argument's range (IGX_ERR_ARG_OUTOFRANGE).
 * Out of scope: degree elevation (p- and k-refinement), several ranks.  The multigrid cycle on these transfers: IGXMultigrid, below. */
typedef struct _p_IGXTransfer *IGXTransfer;
int IGXTransferCreate (IGX coarse,IGX fine,IGXTransfer *tr);
int IGXTransferGetAxis(IGXTransfer tr,int axis,int *nf,int *nc,int *width /* p+1 */,
                       int first[] /* [nf] */,int count[] /* [nf] */,double T[] /* [nf][width], zero past count */);
int IGXTransferProlong (IGXTransfer tr,IGXVec xc,IGXVec xf,int add);
int IGXTransferRestrict(IGXTransfer tr,IGXVec rf,IGXVec rc);
int IGXTransferSetPath (IGXTransfer tr,int path /* 0 automatic, 1 fused, 2 axis passes */);
int IGXTransferGetInfo (IGXTransfer tr,int box[3],int64_t *lds_bytes,int *fused);   /* any pointer may be NULL */
int IGXTransferDestroy (IGXTransfer *tr);

/* Geometric multigrid on the matrix-free operators: one V-cycle as a preconditioner application, and IGXSolve's loop preconditioned by it.
 * No entry of the reference (PetIGA leaves multigrid to PCMG, which needs the interpolation its DM does not provide); the contract is the
 * one below.  One rank only.
 * The hierarchy: nlevels >= 2 set-up IGX, COARSEST FIRST, that the caller has prepared: every level has the same form with the same
 *   parameters, the same Dirichlet faces per field (their values play no part: the cycle acts on residuals), the geometry refined to its own
 *   knots (geometry.refine), the same stream, and each consecutive pair is a pair IGXTransferCreate accepts.  IGXMultigridCreate makes the
 *   nlevels - 1 transfers itself, allocates nothing on a device and takes no vector.  Lifetime and staleness are IGXTransfer's: destroy the
 *   multigrid before any of its levels; after IGXSetUp on any level every call on it returns IGX_ERR_ORDER.
 * Notation.  Levels l = 0 .. L-1.  A_l: the action `op` at the level's state (IGXMultigridSetState; IGX_OP_MATRIX needs none).  D_l: its
 *   diagonal (IGX_PC_JACOBI) or its inverted point blocks (IGX_PC_PBJACOBI), formed by IGXMultigridSetUp.  P_l: the transfer from level l-1
 *   to level l.  lambda_l: the estimate of the largest eigenvalue of D_l^-1 A_l.  fl(.) is one rounding to double; no product is contracted.
 * IGXMultigridSetUp, per level: work vectors (x b r d w, z with point blocks, and D or the dof block columns: kept with the multigrid), D_l,
 *   and lambda_l by power_its steps of the power method on D_l^-1 A_l from the fixed start vector v_i = sin(1 + i) (i the entry's index,
 *   written by the host): per step z = D^-1 A v, lambda = |z|_2 / |v|_2, v = (1 / |z|_2) z; lambda_l is the last step's.  The host reads
 *   two norms per step.  Then, on the host in double and in this order: theta = (hi + lo) lambda / 2, delta = (hi - lo) lambda / 2,
 *   sigma = theta / delta, rho_1 = 1 / sigma, rho_j = 1 / (2 sigma - rho_{j-1}).  Call it again after a state changed (SetState clears it).
 *   Level 0 with coarse_maxit == 0 and coarse_pc IGX_PC_JACOBI or IGX_PC_PBJACOBI holds the coarse preconditioner's D instead of the smoother's.
 *   The power method converges slowly from this start: 10 steps are 8 to 16 % short of the limit on 8^3 to 128^3 elements and hi = 1.1
 *   covers 10; measured on 128^3 elements, 10 steps leave the cycle no contraction and 40 give the counts of DESIGN.md 3.19.  Give
 *   power_its = 40 on meshes of 32^3 elements and beyond.
 * Smooth(l, b, x, zero guess), the Chebyshev iteration on [lo lambda_l, hi lambda_l] with D_l^-1 (PETSc's KSPCHEBYSHEV with PCJACOBI):
 *   step 1:            r = b, or w = A x and r = fl(b - w);  z = fl(r / D), the correctly rounded quotients (point blocks: z = B_node r_node,
 *                      IGXBlockDiagonalApply's kernel);  d = fl((1 / theta) z);  x = d, or x = fl(x + d)
 *   steps j = 2..degree: w = A d;  r = fl(r - w);  z = fl(r / D);  d = fl(fl((rho_j rho_{j-1}) d) + fl((2 rho_j / delta) z));  x = fl(x + d)
 *   The constants 1 / theta, rho_j rho_{j-1} and 2 rho_j / delta are formed on the host.  With the diagonal a step between two operator calls
 *   is ONE sweep (mg_cheb_first, mg_cheb_step: 8 doubles of traffic per entry); with point blocks it is r = r - w, the block apply and the
 *   update, three launches (petiga_amd/csrc/multigrid.hpp).
 * V(l, b):
 *   l = 0: the coarse solve.  coarse_maxit > 0: x = 0 (IGXVecSet's kernel), then IGXSolve on level 0 with coarse_method, coarse_pc,
 *     rtol = coarse_rtol, atol = 0, maxit = coarse_maxit at the level's state; its iterate is used whatever its reason (IGX_DIVERGED_ITS is
 *     an inexact coarse solve).  coarse_maxit == 0: x = M_0^-1 b, ONE application of coarse_pc; a whole cycle then contains no host read.
 *   l > 0:  1. x = Smooth(b, zero guess)
 *           2. w = A d, r = fl(r - w)                      (r is now b - A x up to rounding)
 *           3. b_{l-1} = P_l^T r (IGXTransferRestrict), then the rows of level l-1's Dirichlet faces are set to zero (mg_zero_fixed)
 *           4. e = V(l-1, b_{l-1})
 *           5. x = x + P_l e (IGXTransferProlong with add)
 *           6. x = Smooth(b, x)
 *   That is 2 degree actions per level and cycle.
 * Facts.  The coarse fixed rows are zero on entry, so they stay exactly zero through the smoother and through CG (a fixed row of A is
 *   count times the identity's and D holds the same count).  The clamped end rows of P are unit rows, so the correction is exactly zero on
 *   the fine level's fixed rows.  Fixed rows are eigenvectors of D^-1 A with eigenvalue 1: the smoother treats them like any row.  With the
 *   same polynomial before and after and a LINEAR coarse solve (coarse_maxit == 0) B is symmetric positive definite where A is.  An
 *   iterative coarse solve makes B only approximately linear: under CG give it a tight coarse_rtol (1e-12), or use BiCGStab outside.
 *   A Jacobi smoother is not robust in the degree on splines: the iteration counts are flat in the mesh but grow with p (about 3 to 4 times
 *   from p = 2 to p = 3), so at p = 3 the cycle pays off in operator applications on large meshes only.
 * IGXMultigridApply: z = B r, one V-cycle from a zero guess on the finest level, z != r; everything is enqueued on the levels' stream and,
 *   with timing off and coarse_maxit == 0, nothing touches the host.  Bit-repeatable.  IGXMultigridGetInfo: lambda_l, the length of level l's
 *   vectors and the launches the LAST cycle made on level l (its smoother and residuals, the transfers to and from the level below and the
 *   zeroing of that level's fixed rows; level 0: the coarse solve; 0 before the first cycle); their sum over the levels is what
 *   IGXGetLastTiming reports on the finest IGX after Apply.  Any pointer may be NULL.
 * IGXMultigridSolve: IGXSolve's loop (the same code: krylov_loop in solve_loops.hpp) on the finest level's action with z = B r as the
 *   preconditioner, CG or right-preconditioned BiCGStab, from the guess x holds.  Outcomes, the stop test, history, the b = 0 rule and
 *   IGXSolveInfo are IGXSolve's.  Its work vectors are kept with the multigrid.
 * IGXSetTiming / IGXGetLastTiming / IGXGetKernelName on the FINEST IGX report the call: "multigrid(3 levels, chebyshev-jacobi 2, coarse
 *   fastdiag x1, <the fine action's name>)" after Apply (an iterative coarse solve: "coarse cg+jacobi"), "krylov(cg, pc=multigrid(...),
 *   <action>, <k> iterations)" after Solve.  Kernel time is summed over the levels whose own IGX has timing on.
 * Refusals, each decided before the first HIP call, each reason naming the multigrid, in this order.
 *    1. null pointers (levels, a level, spec, mg; a null multigrid in the other calls): IGX_ERR_ARG_WRONG
 *    2. nlevels < 2: IGX_ERR_ARG_OUTOFRANGE
 *    3. the spec, all IGX_ERR_ARG_OUTOFRANGE: an unknown op or smoother_pc; degree < 1; lo, hi not finite with 0 < lo < hi; power_its < 1; an
 *       unknown coarse method or coarse pc; coarse_maxit < 0; a negative coarse_rtol; coarse_maxit == 0 with IGX_PC_NONE
 *    4. a level before IGXSetUp: IGX_ERR_ORDER (and, after Create, a stale multigrid in every call)
 *    5. no form on a level: IGX_ERR_ARG_WRONGSTATE
 *    6. different forms, or Dirichlet faces per field that differ between levels: IGX_ERR_ARG_WRONG
 *    7. a fix table on any level: IGX_ERR_SUP; then different streams: IGX_ERR_ARG_WRONG
 *    8. whatever IGXTransferCreate refuses, under its code, with the level pair in the message
 *    9. IGX_PC_FASTDIAG as coarse pc without IGXFastDiagSetUp on level 0: IGX_ERR_ORDER, at SetUp (so a caller may set it up after Create)
 *   10. Apply and Solve before SetUp: IGX_ERR_ORDER
 *   11. vectors that are null, foreign, of the wrong size or aliased: IGX_ERR_ARG_WRONG (Solve first refuses an unknown method, a negative
 *       maxit or tolerance with IGX_ERR_ARG_OUTOFRANGE, as IGXSolve does)
 *   12. a missing state for op != IGX_OP_MATRIX: IGX_ERR_ARG_WRONG, at SetUp
 *   13. what the actions or diagonals refuse (Cahn-Hilliard's diagonal): IGX_ERR_SUP with their reason under the multigrid's name
 * Out of scope: several ranks; degree elevation; the multigrid as pc of IGXSolveNonlinear and IGXTimeStep; singular operators (pure
 *   Neumann: no null-space handling); a restriction fused with the residual; W- and F-cycles. */
typedef struct _p_IGXMultigrid *IGXMultigrid;
typedef struct {
  int op;                    /* IGXSolveOperator, the same on every level */
  double a, t;               /* IGX_OP_IJACOBIAN only */
  int smoother_pc;           /* IGX_PC_JACOBI or IGX_PC_PBJACOBI: the D of the Chebyshev smoother */
  int degree;                /* Chebyshev steps per smoothing, >= 1; pre- and post-smoothing use the same */
  double lo, hi;             /* the smoother works on [lo lambda_l, hi lambda_l], 0 < lo < hi (PETSc's 0.1, 1.1) */
  int power_its;             /* power iterations for lambda_l, >= 1 */
  int coarse_method, coarse_pc;  /* level 0: IGXSolve's method and pc */
  double coarse_rtol; int coarse_maxit;   /* coarse_maxit == 0: ONE application of coarse_pc (not IGX_PC_NONE), no host read */
} IGXMultigridSpec;
int IGXMultigridCreate (int nlevels,IGX levels[] /* coarsest first */,const IGXMultigridSpec *spec,IGXMultigrid *mg);
int IGXMultigridSetState(IGXMultigrid mg,int level,IGXVec V,IGXVec U);     /* the state of level's operator; MATRIX needs none */
int IGXMultigridSetUp  (IGXMultigrid mg);   /* diagonals (inverted blocks) and lambda_l on every level; again after a state changed */
int IGXMultigridGetInfo(IGXMultigrid mg,int level,double *lambda,int64_t *n,int *launches_per_cycle);
int IGXMultigridApply  (IGXMultigrid mg,IGXVec r,IGXVec z);                /* z = B r: one V-cycle from a zero guess; z != r */
int IGXMultigridSolve  (IGXMultigrid mg,int method,double rtol,double atol,int maxit,IGXVec b,IGXVec x,IGXSolveInfo *info,double *history);
int IGXMultigridDestroy(IGXMultigrid *mg);
/* Beyond the seven calls of the contract, for scripts/multigrid_rate.py: one fused Chebyshev step (mg_cheb_step) against the four IGXVec
 * kernels it replaces (AXPBY, PointwiseDivide, AXPBY, AXPBY) on level's work vectors, `reps` launches of each between two events per round,
 * the two alternating; fused_ms / split_ms ([rounds] each) receive the time of ONE step per round.  After IGXMultigridSetUp, with the
 * diagonal as D (point blocks: IGX_ERR_SUP); it overwrites the level's x and d, which every cycle rewrites anyway. */
int IGXMultigridMeasureStep(IGXMultigrid mg,int level,int reps,int rounds,double *fused_ms,double *split_ms);

/* Block-vector algebra on blocks of IGXVec, petiga_amd/csrc/block_vec.hpp: PETSc's VecMDot and VecMAXPY for two blocks of 1 <= nx, ny <= 48
 * vectors of ONE IGX.
 *   IGXVecMDot   G[i][j] = X_i . Y_j, G on the host, row-major [nx][ny]; synchronises.  X and Y may share vectors (X == Y: a Gram
 *                matrix).  One pass over the rows on v_mfma_f64_16x16x4_f64 with the row as the contraction index; columns past nx / ny
 *                and rows past n feed zeros and are never read.  A capped grid; every workgroup adds its rows in a fixed order and stores
 *                its partial tile in its own slot, a finishing kernel adds the slots in index order: no atomics, bit-repeatable.
 *   IGXVecMAXPY  Y_j = beta Y_j + sum_i C[i][j] X_i, C on the host, row-major [nx][ny]; beta == 0 writes Y_j whatever it held
 *                (IGXVecAXPBY's rule).  Every entry starts from beta Y_j and adds the terms in ascending i.  Every Y_j must differ from
 *                every X_i and from the other Y.  Enqueued; C is copied before the call returns.
 * IGX_ERR_ARG_WRONG: a null array or entry, vectors of different IGX, an aliased Y.  IGX_ERR_ARG_OUTOFRANGE: nx or ny outside [1, 48].
 * IGX_ERR_SUP: several ranks on an axis (the solve loops' rule: the library has no sum across ranks).
 * IGXSetTiming / IGXGetLastTiming / IGXGetKernelName cover both calls. */
int IGXVecMDot (int nx,IGXVec X[],int ny,IGXVec Y[],double G[] /* host [nx][ny] */);
int IGXVecMAXPY(int ny,IGXVec Y[],int nx,IGXVec X[],const double C[] /* host [nx][ny] */,double beta);

/* The nev lowest eigenpairs of A x = lambda B x on the device, without SLEPc: LOBPCG (Knyazev, SIAM J. Sci. Comput. 23, 2001) with a block
 * of m = block columns, nev <= m <= 16.  A is IGXComputeMatrixAction of `stiff`; B that of `mass`, a second set-up IGX on the same space
 * (typically the Mass form), or the identity with mass == NULL.  Both forms must be symmetric (Poisson, Elasticity, Mass are): that is the
 * caller's responsibility.  IGX_OP_MATRIX only.  X holds the start block on entry and the B-orthonormal Ritz vectors on return; lambda is
 * ascending; resid (may be NULL) receives |A x_j - lambda_j B x_j|_2.  T is the preconditioner pc names, as in IGXSolve: none, the
 * diagonal, the inverted point blocks, or the state of the caller's IGXFastDiagSetUp on stiff.
 * Dirichlet rows: the solve first zeroes the start block's fixed rows (mg_zero_fixed).  A fixed row of either action then returns
 * count x 0 = 0 and every T maps 0 to 0 there, so the iteration stays in the free space with no further masking (the fact the multigrid
 * relies on): the returned vectors are exactly zero on the fixed rows.
 * The loop, with S = [X W P] (the first iteration and the one after a restart have no P):
 *   0. AX = A X, BX = B X (mass == NULL: BX is X, no action and no copy); G_A = X^T AX, G_B = X^T BX (two IGXVecMDot); Rayleigh-Ritz as in
 *      step 6 on X alone; X, AX, BX <- (.) C (IGXVecMAXPY into the second buffer set).  G_B not positive definite here: BREAKDOWN.
 *   1. R_j = AX_j - theta_j BX_j for the whole block in ONE sweep, which also emits the slab partials of |R_j|^2 and |AX_j|^2; a finishing
 *      kernel adds them in index order and the host reads ONE record of 2 m sums per iteration.  history[k][j] = |R_j| at iteration k.
 *   2. Column j has converged when |R_j| <= max(rtol |AX_j|, atol); the solve stops with IGX_EIGEN_CONVERGED when the columns 0 .. nev-1
 *      all have, with IGX_EIGEN_DIVERGED_NAN on a NaN norm, with IGX_EIGEN_DIVERGED_ITS after maxit iterations.  No locking: every column
 *      keeps iterating.
 *   3. W_j = T R_j (pc none: the sweep of step 1 writes R into W).
 *   4. AW = A W, BW = B W: with AX and BX carried along, 2 m actions per iteration (m with mass == NULL).
 *   5. G_A = S^T [AX AW AP], G_B = S^T [BX BW BP]: two IGXVecMDot launches of 3m x 3m (2m x 2m without P).
 *   6. Rayleigh-Ritz on the host: both matrices are symmetrised ((G + G^T) / 2) and scaled by d_i d_j with d = 1 / sqrt(diag G_B); the
 *      dense symmetric-definite solver (Cholesky in long double, cyclic Jacobi, refinement) gives the pairs of (G_A, G_B), of which the m
 *      lowest are taken, C = d .* U.  If G_B is not positive definite (or its diagonal not positive and finite) while P is present: P is
 *      dropped, restarts += 1, and the step is redone on [X W] from the same Gram blocks.  Without P: IGX_EIGEN_DIVERGED_BREAKDOWN.
 *   7. P' = [W P] C_WP, X' = X C_X + P', and the same for the A. and B. blocks (IGXVecMAXPY into the second buffer set, then the sets
 *      swap); theta = the m Ritz values; go to 1.
 * A solve that does not converge returns 0 with the reason in info, as IGXSolve does; X, lambda and resid then hold the last iterate.
 * info->actions counts the calls of either action, info->nconverged the columns among 0 .. nev-1 that met the test at the last iteration. Work vectors are kept with stiff between calls and dropped by IGXSetUp; the vectors
 * the mass action works on are the solver's business (the action of mass runs on stiff's vectors: same space, same layout).
 * IGXGetKernelName: "eigen(lobpcg, block 6, pc=fastdiag, <the action's name>, <k> iterations)"; IGXGetLastTiming: the whole solve with
 * the exact launch count.
 * Refusals, each decided before the first HIP call, each naming the eigen solve, in this order:
 *   1. a null stiff, spec, X, lambda or info: IGX_ERR_ARG_WRONG
 *   2. the spec: nev < 1; block < nev or block > 16; an unknown pc; a negative or NaN tolerance; maxit < 0: IGX_ERR_ARG_OUTOFRANGE;
 *      nx != block: IGX_ERR_ARG_WRONG
 *   3. stiff, then mass, before IGXSetUp: IGX_ERR_ORDER
 *   4. no form on stiff, then on mass: IGX_ERR_ARG_WRONGSTATE
 *   5. mass differs from stiff in dim, dof, then per axis degree, knots, periodicity, then the Dirichlet faces per field, then the
 *      stream: IGX_ERR_ARG_WRONG
 *   6. several ranks on an axis, or a fix table (IGXSetFixTable: its fixed rows are not a union of faces) on either: IGX_ERR_SUP
 *   7. an entry of X that is null, of another IGX than stiff, or repeated: IGX_ERR_ARG_WRONG
 *   8. IGX_PC_FASTDIAG without IGXFastDiagSetUp on stiff: IGX_ERR_ORDER
 *   9. whatever the actions or the diagonals refuse, with their reason under the eigen solve's name.
 * IGXSetBatchedActions(stiff,1) (above, with the block actions): steps 0 and 4 make one block call per operator in place of m single actions.
 * Out of scope: the batched actions as the default, a batched action of a run-time struct, locking of converged
 * columns, interior or largest eigenvalues, Jacobian operators at a state, several ranks, the multigrid as T. */
typedef enum { IGX_EIGEN_CONVERGED = 1, IGX_EIGEN_DIVERGED_ITS = -1, IGX_EIGEN_DIVERGED_BREAKDOWN = -2, IGX_EIGEN_DIVERGED_NAN = -3 } IGXEigenReason;
typedef struct { int nev, block, pc; double rtol, atol; int maxit; } IGXEigenSpec;
typedef struct { int iterations, reason, nconverged, restarts, actions; } IGXEigenInfo;
int IGXEigenSolve(IGX stiff,IGX mass /* NULL: B = I */,const IGXEigenSpec *spec,int nx,IGXVec X[] /* [block], of stiff */,
                  double lambda[] /* [block] */,double resid[] /* [block], may be NULL */,IGXEigenInfo *info,
                  double *history /* NULL or [maxit+1][block]: |r_j|_2 */);
/* the same loop on the stored matrices (stated with IGXMatMultBlock, above) */
int IGXMatEigenSolve(IGXMat K,IGXMat M /* NULL: B = I */,const IGXEigenSpec *spec,int nx,IGXVec X[] /* [block], of K's IGX */,
                     double lambda[] /* [block] */,double resid[] /* [block], may be NULL */,IGXEigenInfo *info,
                     double *history /* NULL or [maxit+1][block]: |r_j|_2 */);

/* Functionals of a discrete field: S[k] = sum over this rank's elements and points of JW * scalar_k(point)
 * (IGAComputeScalar, src/petigacomp.c:35-98, before its MPI_Allreduce: with several ranks the caller sums S over the
 * ranks, and U must hold the ghost rows' values).  The point callbacks are the ones the reference's tests use:
 *   IGX_SCALAR_VOLUME  n=2  test/IGAGeometryMap.c:383: S[0] volume of the mapped domain, S[1] area of the faces marked with
 *                           IGXSetBoundaryForm (boundary passes: normals, detS); U may be NULL
 *   IGX_SCALAR_X2ERR   n=1  src/petigacomp.c:102 (ErrorSqr) with Exact = sum x_i^2 (test/IGAFixTable.c:66), dof 1
 *   IGX_SCALAR_ERRNORM n=4  ErrorSqr with test/IGAErrNorm.c:26 as Exact, dof 4; params {k}: k=0 values, 1 gradients,
 *                           2 Hessians; U NULL gives the norms of the exact fields (squared, like IGAComputeErrorNorm
 *                           before its sqrt, src/petigacomp.c:160).
 * Sums are formed in a fixed order: bitwise repeatable. */
typedef enum { IGX_SCALAR_VOLUME = 1, IGX_SCALAR_X2ERR = 2, IGX_SCALAR_ERRNORM = 3 } IGXScalarKind;
int IGXComputeScalar(IGX iga,IGXVec U,int kind,const double params[],int nparams,int n,double S[]);
/* ... with the user's own point functional (IGAFormScalar, include/petiga.h:188-191; IGAComputeScalar's `Scalar` argument,
 * src/petigacomp.c:35) given as HIP source and compiled at run time like a form of IGXSetFormSource: a struct with
 *   static constexpr int DOF, ORDER, NSCALAR (= n); static constexpr unsigned NEED;
 *   static __device__ void scalar(const igx::PtView &p, double *S);     // un-weighted integrand values at the point
 * p carries x, u, grad u, hess u as NEED asks, prm = params, and atboundary / normal / boundary_id on the passes over faces marked
 * with IGXSetBoundaryForm (an error norm is this with |Exact(x) - u|^2: IGAComputeErrorNorm, src/petigacomp.c:122-186). */
int IGXComputeScalarSource(IGX iga,IGXVec U,const char *source,const char *struct_name,const double params[],int nparams,int n,double S[]);

/* engine controls */
int IGXSetStream(IGX iga,void *hipStream);      /* hipStream_t; NULL = default stream            */
int IGXSynchronize(IGX iga);
/* 0 = automatic; 1 = generic point-form kernel (no MFMA); 2 = MFMA gradient-Gram pencil kernel (Poisson, uniform
 * degree 2/3, no geometry); 3 = feature-GEMM element kernel (any form/geometry, dim >= 2, nen <= 64;
 * K_e on MFMA, vector-only operations share its tabulation); 4 = block pencil kernel (band rows by node layer:
 * constant-coefficient forms with 2 or 3 fields and F = 0, dim 3, p = 3, identity geometry, System / Matrix drivers;
 * the automatic choice takes it where it applies).  A forced kernel that does not cover the case answers PETSC_ERR_SUP. */
int IGXSetKernel(IGX iga,int which);
int IGXGetKernelName(IGX iga,char *buf,int len);
/* name of the kernel the last IGXCompute* used   */
/* time of the dominant kernel of the last IGXCompute* call, measured with HIP events on the
 * engine's stream (ms); IGXSetTiming(1) enables the events */
int IGXSetTiming(IGX iga,int flag);
int IGXGetLastTiming(IGX iga,double *total_ms,double *kernel_ms,int *launches);
/* the dominant kernel of the last IGXCompute* call: its name, the time of its launches (HIP events on the
 * engine's stream, ms), how many launches, how many elements they processed and the MFMA flops it
 * executes per element (for roofline accounting) */
int IGXGetDominantKernelTiming(IGX iga,char *name,int len,double *ms,int *launches,int64_t *elements,double *flop_per_element);

/* element colouring used by the scatter: colour of local element (i,j,k) and the number of
 * colours (bit-exact contract, tests/test_coloring.py) */
int IGXGetColoring(IGX iga,int ncolors[3]);
int IGXGetElementColor(IGX iga,int axis,int e);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU (one process per GPU): ghost-row exchange buffers.  Rank r's ghost rows (nodes it
 * holds but does not own) are packed per upper neighbour (send list, k < nsend); the owner adds
 * them (receive list, k < nrecv).  A message is mat_doubles values (if A given) followed by
 * vec_doubles values (if b given).  Replaces the stash traffic of MatAssemblyBegin/End and
 * VecAssemblyBegin/End (src/petigaksp.c:197-200).  These are the building blocks; IGXReduceGhostRows / IGXRefreshGhosts
 * below run the whole exchange inside the library (RCCL or a caller-provided transport).
 * ------------------------------------------------------------------------------------------ */
int IGXGetNeighborCount(IGX iga,int *nsend,int *nrecv);
int IGXGetNeighborInfo(IGX iga,int send /*1=send list,0=recv list*/,int k,int *rank,int64_t *mat_doubles,int64_t *vec_doubles);
int IGXPackGhostRows  (IGX iga,IGXMat A,IGXVec b,int k,double *devbuf);   /* A or b may be NULL */
int IGXUnpackGhostRows(IGX iga,IGXMat A,IGXVec b,int k,const double *devbuf);
/* Reverse direction, before a nonlinear assembly (IGAGetLocalVecArray / DMGlobalToLocal, src/petigavec.c:256-269): the
 * owner's values of a state vector travel to the ranks holding the node as a ghost.  Pack entry k of the RECEIVE list
 * (vec_doubles of that entry), send it to that rank, which unpacks it as entry k' of its SEND list (assignment). */
int IGXPackOwnerValues  (IGX iga,IGXVec v,int k,double *devbuf);
int IGXUnpackGhostValues(IGX iga,IGXVec v,int k,const double *devbuf);
/* 1 if this rank owns the node of local row (r0,r1,r2): after the exchange only owned rows are final */
int IGXRowOwned(IGX iga,int r0,int r1,int r2);

/* The transport, inside the library.  IGXReduceGhostRows = pack every send-list message, move them, add the received ones
 * (the whole of MatAssemblyBegin/End + VecAssemblyBegin/End, src/petigaksp.c:197-200); IGXRefreshGhosts = the owner's values
 * of a state vector to the ranks that hold the node as a ghost (DMGlobalToLocal in IGAGetLocalVecArray,
 * src/petigavec.c:256-269).  Both are enqueued: packs, transfers and unpacks run on the library's exchange stream, which
 * waits for the engine stream's last launch and is waited for by its next one (events); the host never blocks.
 *   IGXCommInitRCCL: grouped ncclSend / ncclRecv (RCCL over xGMI).  librccl.so is bound with dlopen (an already loaded copy
 *     is reused; `librccl_path` or $IGX_RCCL_LIB name another).  Rank 0 calls IGXCommGetUniqueId and the caller broadcasts
 *     the 128 bytes (MPI_Bcast in PetIGA, torch.distributed in bench.py); size and rank are those of IGXSetComm.
 *   IGXCommInitTransport: a host callback that moves the packed DEVICE buffers (test transport: gloo; an MPI caller).
 *     It is called after the exchange stream has been synchronised and must return with the receive buffers filled. */
typedef struct { char internal[128]; } IGXUniqueId;       /* = ncclUniqueId */
typedef int (*IGXTransportFn)(void *ctx,int nsend,const int send_peer[],double *const send_buf[],const int64_t send_count[],
                              int nrecv,const int recv_peer[],double *const recv_buf[],const int64_t recv_count[]);
int IGXCommGetUniqueId(IGXUniqueId *id,const char *librccl_path /* may be NULL */);
int IGXCommInitRCCL(IGX iga,const IGXUniqueId *id,const char *librccl_path /* may be NULL */);
int IGXCommInitTransport(IGX iga,IGXTransportFn fn,void *ctx);
int IGXCommDestroy(IGX iga);
int IGXReduceGhostRows(IGX iga,IGXMat A,IGXVec b);        /* A or b may be NULL */
int IGXRefreshGhosts(IGX iga,IGXVec v);
int IGXCommGetLastBytes(IGX iga,int64_t *bytes_sent);      /* of the last exchange */
/* The sum across ranks, ordered by rank: vals[i] becomes ((v_0[i] + v_1[i]) + v_2[i]) + ... with v_r the values rank r passed, in place,
 * for 1 <= n <= 64 doubles.  Every rank's values travel to every other rank in ONE group of ncclRecv / ncclSend on the exchange stream (one
 * call of the host transport with every other rank as peer), and every rank adds them in rank order on the host: all ranks get the same
 * bits.  Collective over the communicator and blocking: it is what finishes IGXVecDot, IGXVecNorm2 (the squares) and IGXChecksum on a
 * partition.  IGXSolve adds its inner products by the same rule through the same gather, without leaving the device (below).
 * Refusals, in this order: null iga or vals: IGX_ERR_ARG_WRONG; n outside [1, 64]: IGX_ERR_ARG_OUTOFRANGE; before IGXSetUp: IGX_ERR_ORDER;
 * more than one rank and no communicator: IGX_ERR_ARG_WRONGSTATE; more than 256 ranks: IGX_ERR_SUP.  On one rank it returns 0, leaves
 * vals as they are and touches no device. */
int IGXCommAllSum(IGX iga,int n,double vals[]);
/* The rate (GB/s per direction) a face message of the ghost-row reduction travels at, as the face-first decision of the pencil
 * walks uses it: IGXCommInitRCCL times one grouped ncclSend / ncclRecv of IGX_LINK_PROBE_MB (default 64) MB with
 * every face neighbour, all faces at once, after an untimed one that pays the connection set-up; $IGX_LINK_GBS overrides it.
 * source: 0 the constant 60 (no probe: one rank, no face neighbour, a host transport), 1 measured, 2 $IGX_LINK_GBS;
 * probe_ms / faces: the timed group and the face messages per direction it held.  Any pointer may be NULL. */
int IGXCommGetLinkRate(IGX iga,double *gbs,int *source,double *probe_ms,int *faces);
/* Passes of the last pencil-walk assembly over the rank's box: 1, or 1 + the upper faces (axes 2, 1, 0) that were assembled first
 * so that their messages travel under the rest (the decision: extra passes' cost against largest face / link rate). */
int IGXGetFacePasses(IGX iga,int *passes);
/* one rank sends n doubles to itself through the RCCL path (binding, communicator, streams and events on a single GPU) */
int IGXCommLoopbackTest(IGX iga,int64_t n,double *maxdiff);
/* What the bound transport itself reports: kind 1 = RCCL, 2 = host callback (0: none bound); ranks = ncclCommCount of the RCCL
 * communicator (the number of ranks RCCL actually connected; MPI_Comm_size of the reference's communicator, src/petiga.c:1111),
 * the size given to IGXSetComm for a host transport. */
int IGXCommGetRanks(IGX iga,int *kind,int *ranks);

/* ------------------------------------------------------------------------------------------
 * Hand-back to PETSc (used by adapter/petiga_amd_petsc.c).  PETSc assembles device matrices from coordinate
 * lists: MatSetPreallocationCOO(A,n,coo_i,coo_j) once, MatSetValuesCOO(A,v,ADD_VALUES) per assembly with v on the device.
 * The engine's value array (IGXMatGetDeviceArrays) is that v; IGXMatGetCOO gives the index pair of every stored scalar in
 * the same order (block by block, row-major inside a block).  numbering 0: natural, node*dof+field with axis 0 fastest
 * (IGA_Grid_LocalIndices, src/petigagrid.c); 1: PETSc's, i.e. PetIGA's AO (AOCreateMemoryScalable over the ranks' owned boxes,
 * src/petigagrid.c:185-199).  owned_only: entries of rows this rank does not own get -1, which MatSetPreallocationCOO ignores
 * (use after IGXReduceGhostRows; without it PETSc itself moves the not-owned rows, as MatAssemblyBegin/End always did).
 * Arrays have nblocks*bs*bs (matrix) / vector-size entries, on the device (on_device != 0) or on the host.
 * IGXVecCopyFromGhosted / ToGhosted: the rank's ghosted local array [gw2][gw1][gw0][dof] (IGAGetLocalVecArray,
 * src/petigavec.c:256-269) to / from an IGXVec: identical unless a periodic axis is wrapped inside the rank.
 * IGXMatGetCOODevice: the same lists kept on the device by the matrix (freed by IGXMatFreeCOO / IGXMatDestroy), in the caller's
 * index width (index_bytes 8, or 4 for a PETSc with 32-bit PetscInt; PETSC_ERR_ARG_OUTOFRANGE when an index does not fit):
 * what a device Mat type's MatSetPreallocationCOO takes without 2 x 8 bytes per stored scalar of host staging on this side.
 * on_device copies (IGXVecCopyFromGhosted / ToGhosted, IGXMatGetCOO, IGXVecGetIndices) are ordered on the IGX's own stream:
 * a caller on another stream calls IGXSynchronize first (or shares the stream, IGXSetStream). */
int IGXMatGetCOO(IGXMat A,int numbering,int owned_only,int64_t *coo_i,int64_t *coo_j,int on_device);
int IGXMatGetCOODevice(IGXMat A,int numbering,int owned_only,int index_bytes,void **coo_i,void **coo_j);
int IGXMatFreeCOO(IGXMat A);
int IGXDeviceToHost(void *host,const void *dev,size_t bytes);   /* hipMemcpy for a caller without the HIP headers (the adapter) */
int IGXVecGetIndices(IGXVec v,int numbering,int owned_only,int64_t *idx,int on_device);
int IGXVecGetGhostedSize(IGXVec v,int64_t *n);
int IGXVecCopyFromGhosted(IGXVec v,const double *array,int on_device);
int IGXVecCopyToGhosted(IGXVec v,double *array,int on_device);

/* Checksums of an assembled system over the rows this rank OWNS (after the ghost-row reduction only those are final):
 * S[0] = sum A_ij, S[1] = sum |A_ij|, S[2] = sum b_i, S[3] = sum b_i^2; A or b may be NULL.  Added over the ranks of any
 * partition they equal the single-rank values up to rounding: bench.py asserts exactly that on its N > 1 path, the PetIGA
 * adapter can use it as a MatNorm-free sanity check.  Fixed summation order (bitwise repeatable). */
int IGXChecksum(IGX iga,IGXMat A,IGXVec b,double S[4]);

/* Compile-only check of a run-time form (no GPU needed): IGXSetFormSource compiles the point-form kernel; this compiles the
 * matrix-core kernel the drivers would launch for the degrees set so far (dim >= 2, (p+1)^dim <= 64; 3-D: <= 256), for the matrix drivers
 * (with_matrix != 0) or the vector-only ones.  gram != 0 when the struct declares MAT_PAIR_MASK (it decides the wave layout at
 * dof = 4; on a GPU the flag is read from the compiled module).  gram == 2: the pencil walk's instantiations instead (form_pencil,
 * System and Matrix driver, for the current degree and geometry; dim 3, p = 2 or 3).  gram == 3: the sum-factorised vector kernel
 * (vec_sumfact<MyForm>: Vector / Function / IFunction in 3-D at p <= 3) for the current geometry kind.  gram == 4: state_pencil<p, MyForm>
 * (the Tangent of a scalar struct with the PENCIL_* hooks, below).  gram == 5: block_pencil<MyForm> (System and Matrix driver) of a
 * constant-coefficient multi-field struct.  gram == 6: band_points + band_pt<MyForm> (Matrix / Jacobian / IJacobian of a four-field
 * struct that separates its point coefficients: NCOEF, point_coef, mat_c), without a geometry and on a NURBS map.
 * gram == 7: the ACTION instantiation of vec_sumfact<MyForm> (IGXCompute*Action of the struct) for the current geometry kind.
 * gram == 8: its DIAGONAL instantiation (IGXCompute*Diagonal of the struct; first-order shape features) likewise.  Both compile the
 * layout the driver would launch for the degrees and quadrature sizes set so far (one wavefront per element up to nen, nqp = 4, one
 * workgroup per element with 6 x 6 x 6 or 8 x 8 x 8 lanes above) and return IGX_ERR_SUP with the driver's reason where it would refuse.
 * gram == 9: DIAGONAL with BLOCK (IGXCompute*BlockDiagonal of the struct), the same way.
 * Returns 0 or IGX_ERR_USER with the compiler's log. */
int IGXCheckFormSource(IGX iga,int with_matrix,int gram);

/* Evidence of the overlap of the ghost-row exchange with the assembly: after IGXReduceGhostRows of an assembly
 * that formed the upper face of axis 2 first, the time in ms by which that face's messages were packed BEFORE the assembly's
 * last launch finished (positive: they travelled under the remaining launches).  PETSC_ERR_ARG_WRONGSTATE when the last
 * reduction did not start early (one rank on axis 2, IGX_OVERLAP=0, another kernel path). */
int IGXCommGetOverlap(IGX iga,double *ms);
/* ... and how many of the three phases of that reduction (upper faces of axes 2, 1, 0) were packed behind a face mark of the
 * assembly instead of its last launch: the pencil walk of a rank with upper neighbours on three axes marks all three. */
int IGXCommGetEarlyPhases(IGX iga,int *n);

/* Shader clock under load.  With IGX_CLOCK_PROBE=1 in the environment at IGXCreate, the first and the last workgroup of every
 * pencil-kernel launch add their s_memtime ticks and the ticks of the constant 100 MHz s_memrealtime counter over their walk to
 * two sums; this returns the ratio (MHz) and the elements those wavefronts walked since the previous call, and clears the sums.  The MFMA roofline in bench.py is quoted against the
 * nominal 2400 MHz peak; this figure says what the chip actually sustained while the kernel ran. */
int IGXGetClockProbe(IGX iga,double *shader_mhz,int64_t *elements);

/* The p = 3 patch walk's ticket order, host side (no device is touched).  For a mesh of n1 x n2 elements on axes 1 and 2 walked in nseg
 * segments, colour (cx, cy) of the patches has *nitems items (segment, patch), item = segment x patches + patch; 0: the colour has no
 * patch.  With cap > 0, items[t] is the item that ticket t walks and faces[t] whether its patch lies on a face of axis 1 or 2, for
 * t < min(*nitems, cap); order 0 is the natural order, 1 the faces first (IGX_PATCH3_ORDER). */
int IGXPatch3TicketOrder(int n1,int n2,int nseg,int cx,int cy,int order,int cap,int *nitems,int *items,int *faces);

/* The p = 3 rows walk's staged tile-layer, host side (no device is touched).  On a full layer of a regular tile of 3 x 3 node columns the
 * nine finished rows are staged in a buffer of *doubles doubles in memory order before they are stored (IGX_ROWS3_STAGE); *offset is
 * where the entry (node column col = 0 .. 8 of the tile, column offsets dy, dx, d = -3 .. 3 on axes 2, 1, 0) lies in it. */
int IGXRows3StageOffset(int col,int dy,int dx,int d,int *offset,int *doubles);

/* library / device info for logs */
int IGXGetDeviceInfo(char *buf,int len);

#ifdef __cplusplus
}
#endif
#endif /* PETIGA_AMD_H */
