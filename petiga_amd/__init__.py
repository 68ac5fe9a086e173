"""petiga_amd -- MI355X-native IGA element-assembly engine (one hot path of dalcinl/PetIGA).

This package is a thin ctypes view of the C ABI in include/petiga_amd.h; all compute is in
libpetiga_amd.so (hand-written HIP for gfx950).  There is no CPU or PyTorch fallback: if the
library is missing or no GPU is visible, the compute calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SCALARS = dict(volume=1, x2err=2, errnorm=3)
FORMS = dict(none=0, poisson=1, mass=2, l2proj_x2=3, poisson_f=4, errnorm=5, elasticity=6, cahnhilliard=7, nsvms=8, boundary_integral=9, nitsche=10, bratu=11, elasticity_f=12, der3=13, property=14, surface=15)
RULE_TYPES = dict(legendre=0, lobatto=1, reduced=2, user=3)      # IGARuleType, include/petiga.h:82-87

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class IGXAxisTables(C.Structure):
    _fields_ = [("p", C.c_int), ("m", C.c_int), ("periodic", C.c_int), ("nel", C.c_int), ("nnp", C.c_int),
                ("U", _dp), ("span", _ip), ("nqp", C.c_int), ("nen", C.c_int), ("offset", _ip),
                ("detJac", _dp), ("weight", _dp), ("point", _dp), ("value", _dp)]


class IGXTables(C.Structure):
    _fields_ = [("dim", C.c_int), ("dof", C.c_int), ("order", C.c_int), ("axis", IGXAxisTables * 3),
                ("proc_sizes", C.c_int * 3), ("proc_ranks", C.c_int * 3),
                ("elem_sizes", C.c_int * 3), ("elem_start", C.c_int * 3), ("elem_width", C.c_int * 3),
                ("node_sizes", C.c_int * 3), ("node_lstart", C.c_int * 3), ("node_lwidth", C.c_int * 3),
                ("node_gstart", C.c_int * 3), ("node_gwidth", C.c_int * 3),
                ("nsd", C.c_int), ("rational", C.c_int), ("geometryX", _dp), ("rationalW", _dp),
                ("property", C.c_int), ("propertyA", _dp)]


class IGXSolveSpec(C.Structure):
    _fields_ = [("method", C.c_int), ("op", C.c_int), ("pc", C.c_int), ("a", C.c_double), ("t", C.c_double), ("V", C.c_void_p), ("U", C.c_void_p),
                ("rtol", C.c_double), ("atol", C.c_double), ("maxit", C.c_int)]


class IGXSolveInfo(C.Structure):
    _fields_ = [("iterations", C.c_int), ("reason", C.c_int), ("rnorm0", C.c_double), ("rnorm", C.c_double), ("bnorm", C.c_double)]


class IGXMultigridSpec(C.Structure):
    _fields_ = [("op", C.c_int), ("a", C.c_double), ("t", C.c_double), ("smoother_pc", C.c_int), ("degree", C.c_int), ("lo", C.c_double), ("hi", C.c_double),
                ("power_its", C.c_int), ("coarse_method", C.c_int), ("coarse_pc", C.c_int), ("coarse_rtol", C.c_double), ("coarse_maxit", C.c_int)]


class IGXEigenSpec(C.Structure):
    _fields_ = [("nev", C.c_int), ("block", C.c_int), ("pc", C.c_int), ("rtol", C.c_double), ("atol", C.c_double), ("maxit", C.c_int)]


class IGXEigenInfo(C.Structure):
    _fields_ = [("iterations", C.c_int), ("reason", C.c_int), ("nconverged", C.c_int), ("restarts", C.c_int), ("actions", C.c_int)]


class IGXNewtonSpec(C.Structure):
    _fields_ = [("op", C.c_int), ("a", C.c_double), ("t", C.c_double), ("W", C.c_void_p), ("method", C.c_int), ("pc", C.c_int),
                ("lin_rtol", C.c_double), ("lin_atol", C.c_double), ("lin_maxit", C.c_int), ("forcing", C.c_int),
                ("rtol", C.c_double), ("atol", C.c_double), ("stol", C.c_double), ("maxit", C.c_int), ("linesearch", C.c_int), ("max_backtracks", C.c_int)]


class IGXNewtonInfo(C.Structure):
    _fields_ = [("iterations", C.c_int), ("reason", C.c_int), ("linear_iterations", C.c_int), ("function_evaluations", C.c_int), ("backtracks", C.c_int),
                ("last_linear_reason", C.c_int), ("fnorm0", C.c_double), ("fnorm", C.c_double), ("snorm", C.c_double), ("xnorm", C.c_double)]


class IGXTimeStepSpec(C.Structure):
    _fields_ = [("alpha_m", C.c_double), ("alpha_f", C.c_double), ("gamma", C.c_double), ("t0", C.c_double), ("dt", C.c_double), ("max_time", C.c_double),
                ("max_steps", C.c_int), ("adapt", C.c_int), ("adapt_rtol", C.c_double), ("adapt_atol", C.c_double), ("dt_min", C.c_double), ("dt_max", C.c_double),
                ("max_rejections", C.c_int), ("resume", C.c_int), ("newton", IGXNewtonSpec)]


class IGXTimeStepLog(C.Structure):
    _fields_ = [("t", C.c_double), ("dt", C.c_double), ("wlte", C.c_double), ("accepted", C.c_int), ("newton_iterations", C.c_int), ("newton_reason", C.c_int),
                ("linear_iterations", C.c_int)]


class IGXTimeStepInfo(C.Structure):
    _fields_ = [("steps", C.c_int), ("reason", C.c_int), ("rejections", C.c_int), ("attempts", C.c_int), ("newton_iterations", C.c_int), ("linear_iterations", C.c_int),
                ("function_evaluations", C.c_int), ("t", C.c_double), ("dt_last", C.c_double), ("dt_next", C.c_double), ("unorm", C.c_double)]


SOLVE_METHODS = dict(cg=0, bicgstab=1)
SOLVE_OPERATORS = dict(matrix=0, jacobian=1, ijacobian=2)
SOLVE_PCS = dict(none=0, jacobi=1, pbjacobi=2, fastdiag=3)
KRYLOV_SWEEPS = ("resid0", "dot", "dot2", "jacobi_rz", "cg_update", "bicg_xr", "cg_p", "bicg_p", "bicg_s", "pdiv", "set")      # IGXKrylovSweep, in the header's order
SOLVE_REASONS = {1: "converged_rtol", 2: "converged_atol", -1: "diverged_its", -2: "diverged_breakdown", -3: "diverged_nan"}
EIGEN_REASONS = {1: "converged", -1: "diverged_its", -2: "diverged_breakdown", -3: "diverged_nan", 0: "iterating"}
NEWTON_LINESEARCHES = dict(basic=0, bt=1)
NEWTON_FORCINGS = dict(constant=0, ew2=1)
NEWTON_REASONS = {2: "converged_fnorm_abs", 3: "converged_fnorm_relative", 4: "converged_snorm_relative", -3: "diverged_linear_solve", -4: "diverged_fnorm_nan",
                  -5: "diverged_max_it", -6: "diverged_line_search", 0: "iterating"}
TS_REASONS = {1: "converged_time", 2: "converged_steps", -1: "diverged_nonlinear_solve", -2: "diverged_step_rejected", -3: "diverged_nan", 0: "iterating"}
TS_LOG_DTYPE = np.dtype([("t", "f8"), ("dt", "f8"), ("wlte", "f8"), ("accepted", "i4"), ("newton_iterations", "i4"), ("newton_reason", "i4"), ("linear_iterations", "i4")])


def alpha_scheme(rho_inf=None, scheme=None, alpha=None):
    """(alpha_m, alpha_f, gamma) of IGXTimeStep: from the spectral radius at infinity (the parametrisation TSALPHA's radius option sets),
    scheme="backward_euler" = (1, 1, 1), or the three numbers passed through.  With nothing given: rho_inf = 0.5, the reference demos' choice."""
    if sum(v is not None for v in (rho_inf, scheme, alpha)) > 1:
        raise ValueError("give one of rho_inf, scheme and alpha")
    if alpha is not None:
        am, af, g = (float(v) for v in alpha)
        return am, af, g
    if scheme is not None:
        if scheme != "backward_euler":
            raise ValueError("unknown scheme %r" % (scheme,))
        return 1.0, 1.0, 1.0
    rho = 0.5 if rho_inf is None else float(rho_inf)
    am, af = (3.0 - rho) / (2.0 * (1.0 + rho)), 1.0 / (1.0 + rho)
    return am, af, 0.5 + am - af


# IGXTransportFn (include/petiga_amd.h): the host-callback transport of the ghost-row exchange
TRANSPORT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _ip, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, _ip, C.POINTER(C.c_void_p), C.POINTER(C.c_int64))


class IGXError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("IGX error %d: %s" % (code, msg))
        self.code = code


def lib(build_if_needed=False):
    """Load libpetiga_amd.so.  torch (if importable) is imported first so both share one HIP runtime."""
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(_HERE, "libpetiga_amd_debug.so" if os.environ.get("IGX_USE_DEBUG_LIB") else "libpetiga_amd.so")   # the -DIGX_DEBUG experiment build
    named = bool(os.environ.get("IGX_LIB"))
    if named:      # another build of this same library (A/B measurements, scripts/headline_ab.py): it is the one that is loaded, never rebuilt
        so = os.path.abspath(os.environ["IGX_LIB"])
    elif build_if_needed:
        so = _build.build()
    if not os.path.exists(so):
        raise ImportError("libpetiga_amd.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        import torch  # noqa: F401  (same libamdhip64 for both)
    except Exception:
        pass
    L = C.CDLL(so)
    V = C.c_void_p
    L.IGXGetLastError.restype = C.c_char_p
    L.IGXGetElementCount.restype = C.c_int64
    L.IGXGetElementCount.argtypes = [V]
    sig = {
        "IGXCreate": [C.POINTER(V)], "IGXDestroy": [C.POINTER(V)], "IGXSetDim": [V, C.c_int], "IGXSetDof": [V, C.c_int],
        "IGXSetOrder": [V, C.c_int], "IGXSetQuadrature": [V, C.c_int, C.c_int], "IGXSetRuleType": [V, C.c_int, C.c_int], "IGXSetRuleSize": [V, C.c_int, C.c_int],
        "IGXSetRule": [V, C.c_int, C.c_int, _dp, _dp], "IGXGetRule": [V, C.c_int, _ip, _dp, _dp],
        "IGXGetBasis": [V, C.c_int, _ip, _ip, _ip, _ip, _dp, _dp, _dp, _dp], "IGXSetProcessors": [V, C.c_int, C.c_int],
        "IGXSetComm": [V, C.c_int, C.c_int], "IGXAxisSetDegree": [V, C.c_int, C.c_int], "IGXAxisSetPeriodic": [V, C.c_int, C.c_int],
        "IGXAxisInitUniform": [V, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int], "IGXAxisSetKnots": [V, C.c_int, C.c_int, _dp],
        "IGXSetUp": [V], "IGXSetGeometry": [V, C.c_int, _dp, _dp], "IGXSetProperty": [V, C.c_int, _dp], "IGXGetPropertyDim": [V, C.POINTER(C.c_int)],
        "IGXComputeScalar": [V, V, C.c_int, _dp, C.c_int, C.c_int, _dp],
        "IGXComputeScalarSource": [V, V, C.c_char_p, C.c_char_p, _dp, C.c_int, C.c_int, _dp],
        "IGXRead": [V, C.c_char_p], "IGXWrite": [V, C.c_char_p], "IGXWriteVec": [V, V, C.c_char_p], "IGXReadVec": [V, V, C.c_char_p],
        "IGXSetBoundaryValue": [V, C.c_int, C.c_int, C.c_int, C.c_double], "IGXSetBoundaryLoad": [V, C.c_int, C.c_int, C.c_int, C.c_double],
        "IGXClearBoundary": [V], "IGXSetBoundaryForm": [V, C.c_int, C.c_int, C.c_int], "IGXSetFixTable": [V, V], "IGXSetForm": [V, C.c_int, _dp, C.c_int],
        "IGXGetSizes": [V] + [_ip] * 8, "IGXGetProcessors": [V, _ip, _ip],
        "IGXCreateMat": [V, C.POINTER(V)], "IGXMatDestroy": [C.POINTER(V)],
        "IGXMatGetInfo": [V, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ip],
        "IGXMatGetDeviceArrays": [V, C.POINTER(V), C.POINTER(V), C.POINTER(V)],
        "IGXMatCopyToHost": [V, V, V, V], "IGXMatGetLayout": [V, _ip, _ip], "IGXMatGetAxisMaps": [V, C.c_int, _ip, _ip],
        "IGXCreateVec": [V, C.POINTER(V)], "IGXVecDestroy": [C.POINTER(V)], "IGXVecGetSize": [V, C.POINTER(C.c_int64)],
        "IGXVecGetDeviceArray": [V, C.POINTER(V)], "IGXVecCopyToHost": [V, _dp], "IGXVecCopyFromHost": [V, _dp],
        "IGXComputeSystem": [V, V, V], "IGXComputeMatrix": [V, V], "IGXComputeVector": [V, V],
        "IGXComputeFunction": [V, V, V], "IGXComputeJacobian": [V, V, V],
        "IGXComputeIFunction": [V, C.c_double, V, C.c_double, V, V], "IGXComputeIJacobian": [V, C.c_double, V, C.c_double, V, V],
        "IGXComputeIFunctionIJacobian": [V, C.c_double, V, C.c_double, V, V, V], "IGXComputeFunctionJacobian": [V, V, V, V],
        "IGXComputeMatrixAction": [V, V, V], "IGXComputeJacobianAction": [V, V, V, V],
        "IGXComputeIJacobianAction": [V, C.c_double, V, C.c_double, V, V, V],
        "IGXComputeMatrixActionBlock": [V, C.c_int, C.POINTER(V), C.POINTER(V)], "IGXComputeJacobianActionBlock": [V, V, C.c_int, C.POINTER(V), C.POINTER(V)],
        "IGXComputeIJacobianActionBlock": [V, C.c_double, V, C.c_double, V, C.c_int, C.POINTER(V), C.POINTER(V)], "IGXSetBatchedActions": [V, C.c_int],
        "IGXComputeMatrixDiagonal": [V, V], "IGXComputeJacobianDiagonal": [V, V, V],
        "IGXComputeIJacobianDiagonal": [V, C.c_double, V, C.c_double, V, V],
        "IGXComputeMatrixBlockDiagonal": [V, C.c_int, C.POINTER(V)], "IGXComputeJacobianBlockDiagonal": [V, V, C.c_int, C.POINTER(V)],
        "IGXComputeIJacobianBlockDiagonal": [V, C.c_double, V, C.c_double, V, C.c_int, C.POINTER(V)],
        "IGXBlockDiagonalInvert": [V, C.c_int, C.POINTER(V), C.POINTER(C.c_int64)], "IGXBlockDiagonalApply": [V, C.c_int, C.POINTER(V), V, V],
        "IGXFastDiagSetUp": [V, C.c_double, _dp, _ip], "IGXFastDiagApply": [V, V, V],
        "IGXFastDiagGetAxis": [V, C.c_int, C.c_int, _ip, _ip, _dp, _dp],
        "IGXVecSet": [V, C.c_double], "IGXVecCopy": [V, V], "IGXVecScale": [V, C.c_double], "IGXVecAXPBY": [V, C.c_double, V, C.c_double],
        "IGXVecPointwiseDivide": [V, V, V], "IGXVecDot": [V, V, _dp], "IGXVecNorm2": [V, _dp],
        "IGXVecMDot": [C.c_int, C.POINTER(V), C.c_int, C.POINTER(V), _dp], "IGXVecMAXPY": [C.c_int, C.POINTER(V), C.c_int, C.POINTER(V), _dp, C.c_double],
        "IGXEigenSolve": [V, V, C.POINTER(IGXEigenSpec), C.c_int, C.POINTER(V), _dp, _dp, C.POINTER(IGXEigenInfo), _dp],
        "IGXSolve": [V, C.POINTER(IGXSolveSpec), V, V, C.POINTER(IGXSolveInfo), _dp],
        "IGXSolveNonlinear": [V, C.POINTER(IGXNewtonSpec), V, C.POINTER(IGXNewtonInfo), _dp, _ip],
        "IGXTimeStep": [V, C.POINTER(IGXTimeStepSpec), V, V, C.POINTER(IGXTimeStepInfo), C.POINTER(IGXTimeStepLog), C.c_int],
        "IGXProbeCreate": [V, C.c_int, C.c_int64, _dp, C.POINTER(V)], "IGXProbeGetLocal": [V, C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)],
        "IGXProbeGeomMap": [V, _dp], "IGXProbeGetInfo": [V, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64)], "IGXProbeEvaluate": [V, V, C.c_int, _dp], "IGXProbeDestroy": [C.POINTER(V)],
        "IGXTransferCreate": [V, V, C.POINTER(V)], "IGXTransferGetAxis": [V, C.c_int, _ip, _ip, _ip, _ip, _ip, _dp], "IGXTransferProlong": [V, V, V, C.c_int],
        "IGXTransferRestrict": [V, V, V], "IGXTransferSetPath": [V, C.c_int], "IGXTransferGetInfo": [V, _ip, C.POINTER(C.c_int64), _ip], "IGXTransferDestroy": [C.POINTER(V)],
        "IGXMultigridCreate": [C.c_int, C.POINTER(V), C.POINTER(IGXMultigridSpec), C.POINTER(V)], "IGXMultigridSetState": [V, C.c_int, V, V], "IGXMultigridSetUp": [V],
        "IGXMultigridGetInfo": [V, C.c_int, _dp, C.POINTER(C.c_int64), _ip], "IGXMultigridApply": [V, V, V],
        "IGXMultigridSolve": [V, C.c_int, C.c_double, C.c_double, C.c_int, V, V, C.POINTER(IGXSolveInfo), _dp], "IGXMultigridDestroy": [C.POINTER(V)],
        "IGXMultigridMeasureStep": [V, C.c_int, C.c_int, C.c_int, _dp, _dp],
        "IGXSetStream": [V, V], "IGXSynchronize": [V], "IGXSetKernel": [V, C.c_int], "IGXGetKernelName": [V, C.c_char_p, C.c_int],
        "IGXSetTiming": [V, C.c_int], "IGXGetLastTiming": [V, _dp, _dp, _ip],
        "IGXGetDominantKernelTiming": [V, C.c_char_p, C.c_int, _dp, _ip, C.POINTER(C.c_int64), _dp],
        "IGXGetColoring": [V, _ip], "IGXGetElementColor": [V, C.c_int, C.c_int],
        "IGXGetNeighborCount": [V, _ip, _ip], "IGXGetNeighborInfo": [V, C.c_int, C.c_int, _ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
        "IGXPackGhostRows": [V, V, V, C.c_int, V], "IGXUnpackGhostRows": [V, V, V, C.c_int, V], "IGXRowOwned": [V, C.c_int, C.c_int, C.c_int],
        "IGXPackOwnerValues": [V, V, C.c_int, V], "IGXUnpackGhostValues": [V, V, C.c_int, V],
        "IGXChecksum": [V, V, V, _dp], "IGXCommGetOverlap": [V, _dp], "IGXCheckFormSource": [V, C.c_int, C.c_int], "IGXGetClockProbe": [V, _dp, C.POINTER(C.c_int64)], "IGXSetFormSource": [V, C.c_char_p, C.c_char_p, _dp, C.c_int],
        "IGXMatGetCOO": [V, C.c_int, C.c_int, V, V, C.c_int], "IGXMatGetCOODevice": [V, C.c_int, C.c_int, C.c_int, C.POINTER(V), C.POINTER(V)], "IGXMatFreeCOO": [V],
        "IGXVecGetIndices": [V, C.c_int, C.c_int, V, C.c_int],
        "IGXVecGetGhostedSize": [V, C.POINTER(C.c_int64)], "IGXVecCopyFromGhosted": [V, V, C.c_int], "IGXVecCopyToGhosted": [V, V, C.c_int],
        "IGXCommGetUniqueId": [C.c_void_p, C.c_char_p], "IGXCommInitRCCL": [V, C.c_void_p, C.c_char_p], "IGXCommInitTransport": [V, TRANSPORT_FN, C.c_void_p],
        "IGXCommDestroy": [V], "IGXReduceGhostRows": [V, V, V], "IGXRefreshGhosts": [V, V], "IGXCommGetLastBytes": [V, C.POINTER(C.c_int64)],
        "IGXCommLoopbackTest": [V, C.c_int64, _dp], "IGXCommGetRanks": [V, C.POINTER(C.c_int), C.POINTER(C.c_int)], "IGXCommGetEarlyPhases": [V, C.POINTER(C.c_int)],
        "IGXCommGetLinkRate": [V, _dp, _ip, _dp, _ip], "IGXGetFacePasses": [V, _ip], "IGXCommAllSum": [V, C.c_int, _dp],
        "IGXKrylovSweepTime": [V, C.c_int, C.c_int, C.c_int, _dp],
        "IGXMatMult": [V, V, V], "IGXMatGetDiagonal": [V, V], "IGXMatGetBlockDiagonal": [V, C.c_int, C.POINTER(V)],
        "IGXMatSolve": [V, C.POINTER(IGXSolveSpec), V, V, C.POINTER(IGXSolveInfo), _dp],
        "IGXMatMultBlock": [V, C.c_int, C.POINTER(V), C.POINTER(V)], "IGXMatMultBlockPlan": [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "IGXMatEigenSolve": [V, V, C.POINTER(IGXEigenSpec), C.c_int, C.POINTER(V), _dp, _dp, C.POINTER(IGXEigenInfo), _dp],
        "IGXGetDeviceInfo": [C.c_char_p, C.c_int], "IGXCreateFromTables": [V, C.POINTER(V)],
        "IGXPatch3TicketOrder": [C.c_int] * 7 + [_ip, _ip, _ip],
        "IGXRows3StageOffset": [C.c_int] * 4 + [_ip, _ip],
    }
    missing = []
    for name, args in sig.items():
        if named and not hasattr(L, name):      # an older build of the library under A/B: it lacks newer entry points
            missing.append(name)
            continue
        f = getattr(L, name)
        f.argtypes = args
        f.restype = C.c_int
    if named:      # say which library this is and what it cannot do, here, not as an AttributeError far from the cause
        import sys
        print("petiga_amd: loaded IGX_LIB=%s%s" % (so, (" -- it lacks %d entry point(s) of include/petiga_amd.h: %s" % (len(missing), ", ".join(missing))) if missing else ""), file=sys.stderr)
    _LIB = L
    return L


def _ck(rc):
    if rc:
        raise IGXError(rc, lib().IGXGetLastError().decode())


PROBE_GRID_POINTS = 2048 * 64      # points one turn of the probe kernel's grid-stride loop covers: Probe.info()["points_per_turn"] is the library's own figure


class Probe:
    """IGXProbe: a set of parametric points [npts, dim], located on the device once (IGX.probe).  It keeps its IGX alive."""

    def __init__(self, iga, points, order=0):
        self.iga = iga
        self.h = C.c_void_p()
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim == 1:
            pts = pts.reshape(-1, iga.dim)
        assert pts.ndim == 2 and pts.shape[1] == iga.dim, "points: [npts, dim]"
        self.npts, self.order = pts.shape[0], int(order)
        _ck(lib().IGXProbeCreate(iga.h, int(order), self.npts, pts.ctypes.data_as(_dp) if self.npts else None, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().IGXProbeDestroy(C.byref(self.h))
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def local(self):
        """bool [npts]: the point's element lies in this rank's element box (it is evaluated here; elsewhere it yields zeros)"""
        flags = np.zeros(self.npts, dtype=np.uint8)
        n = C.c_int64()
        _ck(lib().IGXProbeGetLocal(self.h, C.byref(n), flags.ctypes.data_as(C.POINTER(C.c_ubyte)) if self.npts else None))
        assert n.value == int(flags.sum())
        return flags.astype(bool)

    def geom_map(self):
        """[npts, nsd]: the geometry map at the points; without a geometry the points themselves"""
        x = np.empty((self.npts, self.info()["nsd"]))
        _ck(lib().IGXProbeGeomMap(self.h, x.ctypes.data_as(_dp)))
        return x

    def info(self):
        """IGXProbeGetInfo: npts, order, nsd (the columns of geom_map) and points_per_turn of the kernel's grid-stride loop"""
        n, o, d, t = C.c_int64(), C.c_int(), C.c_int(), C.c_int64()
        _ck(lib().IGXProbeGetInfo(self.h, C.byref(n), C.byref(o), C.byref(d), C.byref(t)))
        return dict(npts=n.value, order=o.value, nsd=d.value, points_per_turn=t.value)

    def evaluate(self, U, der=0, out=None):
        """[npts, dof, dim, ...] (der axes of length dim): derivative der of every field of the vector U at the points"""
        dim, dof = self.iga.dim, self.iga.dof
        shape = (self.npts, dof) + (dim,) * max(int(der), 0)
        if out is None:
            out = np.empty(shape)
        assert out.shape == shape and out.dtype == np.float64 and out.flags.c_contiguous
        _ck(lib().IGXProbeEvaluate(self.h, U.h if U is not None else None, int(der), out.ctypes.data_as(_dp)))
        return out


TRANSFER_PATHS = {"auto": 0, "fused": 1, "axis": 2}


class Transfer:
    """IGXTransfer: prolongation and restriction between a coarse IGX and a fine one on nested knot vectors (IGX.transfer on the fine
    object).  It keeps both alive; its tables are built on the host, the first prolong / restrict uploads them."""

    def __init__(self, fine, coarse):
        self.fine, self.coarse = fine, coarse
        self.h = C.c_void_p()
        _ck(lib().IGXTransferCreate(coarse.h if coarse is not None else None, fine.h, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().IGXTransferDestroy(C.byref(self.h))
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def axis(self, i):
        """IGXTransferGetAxis: (first [nf], count [nf], T [nf, p+1]) of axis i; on a periodic axis entry k of row r is column (first[r] + k) mod nc"""
        nf, nc, w = C.c_int(), C.c_int(), C.c_int()
        _ck(lib().IGXTransferGetAxis(self.h, int(i), C.byref(nf), C.byref(nc), C.byref(w), None, None, None))
        first, count, T = np.empty(nf.value, dtype=np.int32), np.empty(nf.value, dtype=np.int32), np.empty((nf.value, w.value))
        _ck(lib().IGXTransferGetAxis(self.h, int(i), None, None, None, first.ctypes.data_as(_ip), count.ctypes.data_as(_ip), T.ctypes.data_as(_dp)))
        return first, count, T

    def sizes(self, i):
        """(nf, nc, width) of axis i"""
        nf, nc, w = C.c_int(), C.c_int(), C.c_int()
        _ck(lib().IGXTransferGetAxis(self.h, int(i), C.byref(nf), C.byref(nc), C.byref(w), None, None, None))
        return nf.value, nc.value, w.value

    def set_path(self, path):
        """"auto", "fused" (IGXError where a box's coarse footprint does not fit the LDS budget) or "axis": the kernel prolong runs"""
        _ck(lib().IGXTransferSetPath(self.h, TRANSFER_PATHS[path] if isinstance(path, str) else int(path)))
        return self

    def info(self):
        """IGXTransferGetInfo: the fused kernel's box (fine rows per axis), its LDS bytes and whether prolong runs fused"""
        box, lds, fused = (C.c_int * 3)(), C.c_int64(), C.c_int()
        _ck(lib().IGXTransferGetInfo(self.h, box, C.byref(lds), C.byref(fused)))
        return dict(box=tuple(box), lds_bytes=lds.value, fused=bool(fused.value))

    def prolong(self, xc, xf, add=False):
        """xf = P xc (add: xf += P xc)"""
        _ck(lib().IGXTransferProlong(self.h, xc.h if xc is not None else None, xf.h if xf is not None else None, int(bool(add))))
        return xf

    def restrict(self, rf, rc):
        """rc = P^T rf"""
        _ck(lib().IGXTransferRestrict(self.h, rf.h if rf is not None else None, rc.h if rc is not None else None))
        return rc


class Multigrid:
    """IGXMultigrid: a V-cycle over the set-up IGX `levels` (coarsest first; IGX.multigrid on the finest object) with a Chebyshev smoother on
    the diagonal ("jacobi") or the point blocks ("pbjacobi") of the action `op`, as a preconditioner (apply) and under CG / BiCGStab (solve).
    coarse: a dict of method, pc, rtol, maxit for level 0; maxit = 0 is ONE application of pc.  power_its: the steps of the power method for
    lambda; give 40 on meshes of 32^3 elements and beyond (10 underestimate lambda by more than hi covers there).  It keeps its levels alive."""

    def __init__(self, levels, op="matrix", smoother="jacobi", degree=2, lo=0.1, hi=1.1, power_its=10, coarse=None, a=0.0, t=0.0):
        code = lambda table, v: table[v] if isinstance(v, str) else int(v)
        c = dict(method="cg", pc="jacobi", rtol=1e-12, maxit=1000)
        c.update(coarse or {})
        self.levels = list(levels)
        self.spec = IGXMultigridSpec(code(SOLVE_OPERATORS, op), float(a), float(t), code(SOLVE_PCS, smoother), int(degree), float(lo), float(hi), int(power_its),
                                     code(SOLVE_METHODS, c["method"]), code(SOLVE_PCS, c["pc"]), float(c["rtol"]), int(c["maxit"]))
        self.h = C.c_void_p()
        self._states = {}
        hs = (C.c_void_p * max(len(self.levels), 1))(*[g.h.value if g is not None else None for g in self.levels])
        _ck(lib().IGXMultigridCreate(len(self.levels), hs, C.byref(self.spec), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().IGXMultigridDestroy(C.byref(self.h))
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, level, U=None, V=None):
        """the state of level's operator: U for "jacobian", V and U for "ijacobian" (the multigrid keeps the vectors alive)"""
        _ck(lib().IGXMultigridSetState(self.h, int(level), V.h if V is not None else None, U.h if U is not None else None))
        self._states[int(level)] = (U, V)
        return self

    def setup(self):
        """IGXMultigridSetUp: the diagonals (inverted blocks) and lambda on every level; again after a state changed"""
        _ck(lib().IGXMultigridSetUp(self.h))
        return self

    def info(self, level):
        """IGXMultigridGetInfo: dict(lambda_, n, launches) of a level; launches: what the last cycle spent there"""
        lam, n, k = C.c_double(), C.c_int64(), C.c_int()
        _ck(lib().IGXMultigridGetInfo(self.h, int(level), C.byref(lam), C.byref(n), C.byref(k)))
        return dict(lambda_=lam.value, n=n.value, launches=k.value)

    def measure_step(self, level, reps=200, rounds=7):
        """IGXMultigridMeasureStep: (fused_ms [rounds], split_ms [rounds]), the time of one fused Chebyshev step and of the four IGXVec kernels
        it replaces on the level's work vectors, the two alternating round by round"""
        fused, split = np.zeros(int(rounds)), np.zeros(int(rounds))
        _ck(lib().IGXMultigridMeasureStep(self.h, int(level), int(reps), int(rounds), fused.ctypes.data_as(_dp), split.ctypes.data_as(_dp)))
        return fused, split

    def apply(self, r, z):
        """z = B r: one V-cycle from a zero guess"""
        _ck(lib().IGXMultigridApply(self.h, r.h if r is not None else None, z.h if z is not None else None))
        return z

    def solve(self, b, x, method="cg", rtol=1e-10, atol=0.0, maxit=1000, history=False):
        """IGXMultigridSolve: the finest level's A x = b by CG or BiCGStab preconditioned by the cycle, from the guess x holds; returns
        the dict IGX.solve returns"""
        info = IGXSolveInfo()
        hist = np.zeros(max(int(maxit), 0) + 1) if history else None
        _ck(lib().IGXMultigridSolve(self.h, SOLVE_METHODS[method] if isinstance(method, str) else int(method), float(rtol), float(atol), int(maxit),
                                    b.h if b is not None else None, x.h if x is not None else None, C.byref(info), hist.ctypes.data_as(_dp) if history else None))
        out = dict(iterations=info.iterations, reason=info.reason, reason_name=SOLVE_REASONS.get(info.reason, str(info.reason)),
                   rnorm0=info.rnorm0, rnorm=info.rnorm, bnorm=info.bnorm)
        if history:
            out["history"] = hist[:info.iterations + 1].copy()
        return out


class Vec:
    def __init__(self, iga):
        self.iga = iga
        self.h = C.c_void_p()
        _ck(lib().IGXCreateVec(iga.h, C.byref(self.h)))
        n = C.c_int64()
        _ck(lib().IGXVecGetSize(self.h, C.byref(n)))
        self.n = n.value

    def __del__(self):
        try:
            lib().IGXVecDestroy(C.byref(self.h))
        except Exception:
            pass

    def set(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.n
        _ck(lib().IGXVecCopyFromHost(self.h, a.ctypes.data_as(_dp)))
        return self

    def get(self):
        a = np.empty(self.n)
        _ck(lib().IGXVecCopyToHost(self.h, a.ctypes.data_as(_dp)))
        return a

    def device_ptr(self):
        p = C.c_void_p()
        _ck(lib().IGXVecGetDeviceArray(self.h, C.byref(p)))
        return p.value

    # vector algebra on the device (enqueued on the engine's stream; dot and norm hand a number back and so synchronise)
    def fill(self, value): _ck(lib().IGXVecSet(self.h, float(value))); return self
    def copy_from(self, x): _ck(lib().IGXVecCopy(x.h, self.h)); return self
    def scale(self, a): _ck(lib().IGXVecScale(self.h, float(a))); return self
    def axpby(self, a, x, b=1.0): _ck(lib().IGXVecAXPBY(self.h, float(a), x.h, float(b))); return self      # self = a x + b self
    def pointwise_divide(self, x, d): _ck(lib().IGXVecPointwiseDivide(self.h, x.h, d.h)); return self      # self = x ./ d

    def dot(self, y):
        """over the rows this rank owns; on several ranks the caller adds the parts"""
        s = C.c_double(0)
        _ck(lib().IGXVecDot(self.h, y.h, C.byref(s)))
        return s.value

    def norm(self):
        s = C.c_double(0)
        _ck(lib().IGXVecNorm2(self.h, C.byref(s)))
        return s.value

    def indices(self, numbering=0, owned_only=False):
        """Global index of every entry (natural or PETSc numbering), -1 for not-owned rows when owned_only."""
        idx = np.empty(self.n, dtype=np.int64)
        _ck(lib().IGXVecGetIndices(self.h, numbering, int(owned_only), idx.ctypes.data, 0))
        return idx

    def ghosted_size(self):
        n = C.c_int64()
        _ck(lib().IGXVecGetGhostedSize(self.h, C.byref(n)))
        return n.value

    def set_from_ghosted(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.ghosted_size()
        _ck(lib().IGXVecCopyFromGhosted(self.h, a.ctypes.data, 0))
        return self

    def get_ghosted(self):
        a = np.empty(self.ghosted_size())
        _ck(lib().IGXVecCopyToGhosted(self.h, a.ctypes.data, 0))
        return a


def _vec_array(vs):
    return (C.c_void_p * max(len(vs), 1))(*[v.h.value if v is not None else None for v in vs])


def _mdot(X, Y):
    """IGXVecMDot: G [len(X), len(Y)] with G[i, j] = X[i] . Y[j], in one pass over the rows on the FP64 matrix cores (1 to 48 vectors of one
    IGX per block; X and Y may share vectors); synchronises"""
    X, Y = list(X), list(Y)
    G = np.zeros((max(len(X), 1), max(len(Y), 1)))
    _ck(lib().IGXVecMDot(len(X), _vec_array(X), len(Y), _vec_array(Y), G.ctypes.data_as(_dp)))
    return G[:len(X), :len(Y)]


def _maxpy(Y, X, Cm, beta=0.0):
    """IGXVecMAXPY: Y[j] = beta Y[j] + sum_i Cm[i, j] X[i] (beta == 0 writes Y[j] whatever it held); every Y[j] differs from every X[i]"""
    X, Y = list(X), list(Y)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64)
    assert Cm.shape == (len(X), len(Y)), "C: [len(X), len(Y)]"
    _ck(lib().IGXVecMAXPY(len(Y), _vec_array(Y), len(X), _vec_array(X), Cm.ctypes.data_as(_dp), float(beta)))
    return Y


Vec.mdot = staticmethod(_mdot)
Vec.maxpy = staticmethod(_maxpy)


def mat_mult_block_plan(bs, nx):
    """IGXMatMultBlockPlan: the widths of the launches Mat.mult_block makes for nx columns at block size bs, in order (a width of 1 is Mat.mult's
    own kernel); host only"""
    n, w = C.c_int(0), (C.c_int * max(int(nx), 1))()
    _ck(lib().IGXMatMultBlockPlan(int(bs), int(nx), C.byref(n), w))
    return [int(w[k]) for k in range(n.value)]


class Mat:
    def __init__(self, iga):
        self.iga = iga
        self.h = C.c_void_p()
        _ck(lib().IGXCreateMat(iga.h, C.byref(self.h)))
        a, b, c = C.c_int64(), C.c_int64(), C.c_int()
        _ck(lib().IGXMatGetInfo(self.h, C.byref(a), C.byref(b), C.byref(c)))
        self.nbrows, self.nblocks, self.bs = a.value, b.value, c.value

    def __del__(self):
        try:
            lib().IGXMatDestroy(C.byref(self.h))
        except Exception:
            pass

    def device_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _ck(lib().IGXMatGetDeviceArrays(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def host(self, values_only=False):
        val = np.empty(self.nblocks * self.bs * self.bs)
        if values_only:
            _ck(lib().IGXMatCopyToHost(self.h, None, None, val.ctypes.data))
            return val
        rp = np.empty(self.nbrows + 1, dtype=np.int64)
        ci = np.empty(self.nblocks, dtype=np.int32)
        _ck(lib().IGXMatCopyToHost(self.h, rp.ctypes.data, ci.ctypes.data, val.ctypes.data))
        return rp, ci, val

    def coo(self, numbering=0, owned_only=False):
        """(coo_i, coo_j) of every stored scalar in the order of the value array (IGXMatGetCOO)."""
        n = self.nblocks * self.bs * self.bs
        ci, cj = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        _ck(lib().IGXMatGetCOO(self.h, numbering, int(owned_only), ci.ctypes.data, cj.ctypes.data, 0))
        return ci, cj

    def coo_device(self, numbering=0, owned_only=False, index_bytes=8):
        """Device pointers of the coordinate lists the matrix keeps for the hand-back (IGXMatGetCOODevice); free_coo() drops them."""
        pi, pj = C.c_void_p(), C.c_void_p()
        _ck(lib().IGXMatGetCOODevice(self.h, numbering, int(owned_only), index_bytes, C.byref(pi), C.byref(pj)))
        return pi.value, pj.value

    def free_coo(self): _ck(lib().IGXMatFreeCOO(self.h))

    # the stored matrix as an operator (one rank on every axis): the product, the diagonals, IGXSolve's loop on it
    def mult(self, x, y): _ck(lib().IGXMatMult(self.h, x.h if x is not None else None, y.h if y is not None else None))      # y = A x
    def diagonal(self, d): _ck(lib().IGXMatGetDiagonal(self.h, d.h if d is not None else None))

    def block_diagonal(self, B):
        """IGXMatGetBlockDiagonal: column j of every node's bs x bs diagonal block into B[j] (the layout of compute_*_block_diagonal)."""
        _ck(lib().IGXMatGetBlockDiagonal(self.h, len(B), (C.c_void_p * max(len(B), 1))(*[b.h.value if b is not None else None for b in B])))

    def solve(self, b, x, method="cg", pc="none", rtol=1e-10, atol=0.0, maxit=1000, history=False):
        """IGXMatSolve: A x = b on the device with A this matrix (y = A x by mult), from the guess x holds.  Returns what IGX.solve returns."""
        code = lambda table, v: table[v] if isinstance(v, str) else int(v)
        spec = IGXSolveSpec(code(SOLVE_METHODS, method), 0, code(SOLVE_PCS, pc), 0.0, 0.0, None, None, float(rtol), float(atol), int(maxit))
        info = IGXSolveInfo()
        hist = np.zeros(max(int(maxit), 0) + 1) if history else None
        _ck(lib().IGXMatSolve(self.h, C.byref(spec), b.h if b is not None else None, x.h if x is not None else None, C.byref(info),
                              hist.ctypes.data_as(_dp) if history else None))
        out = dict(iterations=info.iterations, reason=info.reason, reason_name=SOLVE_REASONS.get(info.reason, str(info.reason)),
                   rnorm0=info.rnorm0, rnorm=info.rnorm, bnorm=info.bnorm)
        if history:
            out["history"] = hist[:info.iterations + 1].copy()
        return out

    def mult_block(self, X, Y):
        """IGXMatMultBlock: Y[j] = A X[j] for lists of Vecs of one length (1 .. 48); column j is bit for bit what mult(X[j], Y[j]) stores."""
        if len(X) != len(Y):
            raise ValueError("the block product takes as many results as vectors, got %d and %d" % (len(Y), len(X)))
        _ck(lib().IGXMatMultBlock(self.h, len(X), _vec_array(X), _vec_array(Y)))

    def eigen(self, nev, mass=None, block=None, pc="none", rtol=1e-8, atol=0.0, maxit=200, X0=None, history=False):
        """IGXMatEigenSolve: the nev lowest eigenpairs of K x = lambda M x by LOBPCG on the device, K this matrix, M the Mat `mass` on the
        same space (None: the identity).  X0: the start block, a list of block Vecs of this matrix's IGX (default: as IGX.eigen).  Returns
        what IGX.eigen returns."""
        nev = int(nev)
        m = min(16, nev + 2) if block is None else int(block)
        X = X0
        if X is None:
            X = []
            if 1 <= nev <= m <= 16:      # (otherwise the call refuses the specification before it looks at the block)
                rng = np.random.default_rng(0)
                for _ in range(m):
                    v = self.iga.create_vec()
                    X.append(v.set(rng.standard_normal(v.n)))
        X = list(X)
        spec = IGXEigenSpec(nev, m, SOLVE_PCS[pc] if isinstance(pc, str) else int(pc), float(rtol), float(atol), int(maxit))
        info = IGXEigenInfo()
        lam, res = np.zeros(max(m, 1)), np.zeros(max(m, 1))
        hist = np.zeros((max(int(maxit), 0) + 1, max(m, 1))) if history else None
        _ck(lib().IGXMatEigenSolve(self.h, mass.h if mass is not None else None, C.byref(spec), len(X), _vec_array(X), lam.ctypes.data_as(_dp), res.ctypes.data_as(_dp),
                                   C.byref(info), hist.ctypes.data_as(_dp) if history else None))
        out = {k: getattr(info, k) for k, _ in IGXEigenInfo._fields_}
        out["reason_name"] = EIGEN_REASONS.get(info.reason, str(info.reason))
        out["lambda"], out["X"], out["resid"] = lam[:m].copy(), X, res[:m].copy()
        if history:
            out["history"] = hist[:info.iterations + 1, :m].copy()
        return out

    def layout(self):
        nrow, ncol = (C.c_int * 3)(), (C.c_int * 3)()
        _ck(lib().IGXMatGetLayout(self.h, nrow, ncol))
        maps = []
        for d in range(3):
            r = np.empty(nrow[d], dtype=np.int32)
            c = np.empty(ncol[d], dtype=np.int32)
            _ck(lib().IGXMatGetAxisMaps(self.h, d, r.ctypes.data_as(_ip), c.ctypes.data_as(_ip)))
            maps.append((r, c))
        return list(nrow), list(ncol), maps

    def to_coo_global(self):
        """(rows, cols, vals) in global natural numbering (node*dof+field), one entry per stored scalar."""
        rp, ci, val = self.host()
        nrow, ncol, maps = self.layout()
        ns = self.iga.sizes()["node_sizes"]
        bs = self.bs
        r = np.arange(self.nbrows, dtype=np.int64)
        r0, r1, r2 = r % nrow[0], (r // nrow[0]) % nrow[1], r // (nrow[0] * nrow[1])
        grow = maps[0][0][r0].astype(np.int64) + ns[0] * (maps[1][0][r1].astype(np.int64) + ns[1] * maps[2][0][r2].astype(np.int64))
        c = ci.astype(np.int64)
        c0, c1, c2 = c % ncol[0], (c // ncol[0]) % ncol[1], c // (ncol[0] * ncol[1])
        gcol = maps[0][1][c0].astype(np.int64) + ns[0] * (maps[1][1][c1].astype(np.int64) + ns[1] * maps[2][1][c2].astype(np.int64))
        brow = np.repeat(grow, np.diff(rp))
        ii, jj = np.meshgrid(np.arange(bs), np.arange(bs), indexing="ij")
        rows = (brow[:, None, None] * bs + ii[None]).reshape(-1)
        cols = (gcol[:, None, None] * bs + jj[None]).reshape(-1)
        return rows, cols, val.copy()

    def to_scipy_global(self):
        """Global natural-order CSR (node*dof+field) -- the Mat PETSc would hold on one rank."""
        import scipy.sparse as sp
        rows, cols, vals = self.to_coo_global()
        n = int(np.prod(self.iga.sizes()["node_sizes"])) * self.bs
        return sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()


class IGX:
    """Mirror of the PetIGA calls a driver program makes around IGAComputeSystem & friends."""

    def __init__(self, dim=None, dof=None, _handle=None):
        self.h = C.c_void_p()
        if _handle is not None:
            self.h = _handle
            return
        _ck(lib().IGXCreate(C.byref(self.h)))
        if dim is not None:
            self.set_dim(dim)
        if dof is not None:
            self.set_dof(dof)

    def __del__(self):
        try:
            lib().IGXDestroy(C.byref(self.h))
        except Exception:
            pass

    @classmethod
    def from_tables(cls, tables):
        """IGXCreateFromTables: the route a set-up PetIGA `IGA` takes."""
        h = C.c_void_p()
        _ck(lib().IGXCreateFromTables(C.byref(tables), C.byref(h)))
        g = cls(_handle=h)
        g.dim, g.dof = tables.dim, tables.dof
        return g

    def set_dim(self, dim): _ck(lib().IGXSetDim(self.h, dim)); self.dim = dim
    def set_dof(self, dof): _ck(lib().IGXSetDof(self.h, dof)); self.dof = dof
    def set_order(self, o): _ck(lib().IGXSetOrder(self.h, o))
    def set_quadrature(self, i, q): _ck(lib().IGXSetQuadrature(self.h, i, q))
    def set_rule_type(self, i, kind): _ck(lib().IGXSetRuleType(self.h, i, RULE_TYPES[kind] if isinstance(kind, str) else kind))
    def set_rule_size(self, i, q): _ck(lib().IGXSetRuleSize(self.h, i, q))

    def set_rule(self, i, x, w):
        x, w = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
        assert x.shape == w.shape and x.ndim == 1
        _ck(lib().IGXSetRule(self.h, i, len(x), x.ctypes.data_as(_dp), w.ctypes.data_as(_dp)))

    def rule(self, i):
        q = C.c_int(0)
        _ck(lib().IGXGetRule(self.h, i, C.byref(q), None, None))
        x, w = np.zeros(q.value), np.zeros(q.value)
        _ck(lib().IGXGetRule(self.h, i, C.byref(q), x.ctypes.data_as(_dp), w.ctypes.data_as(_dp)))
        return x, w
    def set_comm(self, size, rank):
        _ck(lib().IGXSetComm(self.h, size, rank))
        self._comm = (size, rank)

    def comm_size(self): return getattr(self, "_comm", (1, 0))[0]
    def set_processors(self, i, n): _ck(lib().IGXSetProcessors(self.h, i, n))

    def axis_uniform(self, i, p, N, C_=-1, Ui=0.0, Uf=1.0, periodic=False):
        _ck(lib().IGXAxisSetDegree(self.h, i, p))
        _ck(lib().IGXAxisSetPeriodic(self.h, i, int(periodic)))
        _ck(lib().IGXAxisInitUniform(self.h, i, N, Ui, Uf, C_))

    def axis_knots(self, i, p, U, periodic=False):
        U = np.ascontiguousarray(U, dtype=np.float64)
        _ck(lib().IGXAxisSetDegree(self.h, i, p))
        _ck(lib().IGXAxisSetPeriodic(self.h, i, int(periodic)))
        _ck(lib().IGXAxisSetKnots(self.h, i, len(U) - 1, U.ctypes.data_as(_dp)))

    def setup(self): _ck(lib().IGXSetUp(self.h))
    def read(self, filename): _ck(lib().IGXRead(self.h, str(filename).encode()))
    def write(self, filename): _ck(lib().IGXWrite(self.h, str(filename).encode()))
    def write_vec(self, vec, filename): _ck(lib().IGXWriteVec(self.h, vec.h, str(filename).encode()))
    def read_vec(self, vec, filename): _ck(lib().IGXReadVec(self.h, vec.h, str(filename).encode()))

    def set_geometry(self, X, W=None):
        X = np.ascontiguousarray(X, dtype=np.float64)
        Wp = None if W is None else np.ascontiguousarray(W, dtype=np.float64)
        _ck(lib().IGXSetGeometry(self.h, X.shape[-1], X.ctypes.data_as(_dp), None if Wp is None else Wp.ctypes.data_as(_dp)))

    def set_property(self, A):
        """IGASetPropertyDim + the property array on the geometry grid, natural order [..][npd] (None drops it)."""
        if A is None:
            _ck(lib().IGXSetProperty(self.h, 0, None)); return
        A = np.ascontiguousarray(A, dtype=np.float64)
        _ck(lib().IGXSetProperty(self.h, A.shape[-1], A.ctypes.data_as(_dp)))

    def property_dim(self):
        n = C.c_int(0); _ck(lib().IGXGetPropertyDim(self.h, C.byref(n))); return n.value

    def set_boundary_value(self, axis, side, field, value): _ck(lib().IGXSetBoundaryValue(self.h, axis, side, field, value))
    def set_boundary_load(self, axis, side, field, value): _ck(lib().IGXSetBoundaryLoad(self.h, axis, side, field, value))
    def clear_boundary(self): _ck(lib().IGXClearBoundary(self.h))
    def set_boundary_form(self, axis, side, flag=True): _ck(lib().IGXSetBoundaryForm(self.h, axis, side, int(bool(flag))))
    def set_fixtable(self, vec): _ck(lib().IGXSetFixTable(self.h, vec.h if vec is not None else None))

    def set_form(self, kind, params=()):
        p = np.ascontiguousarray(params, dtype=np.float64)
        _ck(lib().IGXSetForm(self.h, FORMS[kind] if isinstance(kind, str) else kind, p.ctypes.data_as(_dp) if p.size else None, p.size))

    def set_form_source(self, source, struct_name, params=()):
        """A user point form as HIP source (the contract of petiga_amd/csrc/forms.hpp), compiled at run time with hiprtc."""
        p = np.ascontiguousarray(params, dtype=np.float64)
        _ck(lib().IGXSetFormSource(self.h, source.encode(), struct_name.encode(), p.ctypes.data_as(_dp) if p.size else None, p.size))

    def sizes(self):
        arrs = [(C.c_int * 3)() for _ in range(8)]
        _ck(lib().IGXGetSizes(self.h, *arrs))
        names = ["elem_sizes", "elem_start", "elem_width", "node_sizes", "node_lstart", "node_lwidth", "node_gstart", "node_gwidth"]
        out = {k: list(a) for k, a in zip(names, arrs)}
        ps, pr = (C.c_int * 3)(), (C.c_int * 3)()
        _ck(lib().IGXGetProcessors(self.h, ps, pr))
        out["proc_sizes"], out["proc_ranks"] = list(ps), list(pr)
        return out

    def basis(self, i):
        """The 1-D tables of axis i (IGAGetBasis): offset, detJac, weight, point, value[nel][nqp][nen][5]."""
        n = [C.c_int(0) for _ in range(3)]
        _ck(lib().IGXGetBasis(self.h, i, C.byref(n[0]), C.byref(n[1]), C.byref(n[2]), None, None, None, None, None))
        nel, nqp, nen = (v.value for v in n)
        off = np.zeros(nel, dtype=np.int32)
        J, w, pt, val = np.zeros(nel), np.zeros((nel, nqp)), np.zeros((nel, nqp)), np.zeros((nel, nqp, nen, 5))
        _ck(lib().IGXGetBasis(self.h, i, None, None, None, off.ctypes.data_as(_ip), J.ctypes.data_as(_dp), w.ctypes.data_as(_dp), pt.ctypes.data_as(_dp), val.ctypes.data_as(_dp)))
        return dict(nel=nel, nqp=nqp, nen=nen, offset=off, detJac=J, weight=w, point=pt, value=val)

    def compute_scalar(self, kind, U=None, params=()):
        """IGAComputeScalar for one of the built-in functionals; returns the rank-local sums."""
        k = SCALARS[kind] if isinstance(kind, str) else kind
        n = 4 if k == SCALARS["errnorm"] else (2 if k == SCALARS["volume"] else 1)
        out = np.zeros(n)
        p = np.ascontiguousarray(params, dtype=np.float64)
        _ck(lib().IGXComputeScalar(self.h, U.h if U is not None else None, k, p.ctypes.data_as(_dp) if p.size else None, p.size, n, out.ctypes.data_as(_dp)))
        return out

    def compute_scalar_source(self, source, struct_name, n, U=None, params=()):
        """IGAComputeScalar with the user's point functional as HIP source (a struct with NSCALAR = n and scalar(p, S))."""
        out = np.zeros(n)
        p = np.ascontiguousarray(params, dtype=np.float64)
        _ck(lib().IGXComputeScalarSource(self.h, U.h if U is not None else None, source.encode(), struct_name.encode(),
                                         p.ctypes.data_as(_dp) if p.size else None, p.size, n, out.ctypes.data_as(_dp)))
        return out

    def element_count(self): return lib().IGXGetElementCount(self.h)
    def create_mat(self): return Mat(self)
    def create_vec(self): return Vec(self)

    def compute_system(self, A, b): _ck(lib().IGXComputeSystem(self.h, A.h, b.h))
    def compute_matrix(self, A): _ck(lib().IGXComputeMatrix(self.h, A.h))
    def compute_vector(self, b): _ck(lib().IGXComputeVector(self.h, b.h))
    def compute_function(self, U, F): _ck(lib().IGXComputeFunction(self.h, U.h, F.h))
    def compute_jacobian(self, U, J): _ck(lib().IGXComputeJacobian(self.h, U.h, J.h))
    def compute_ifunction(self, a, V, t, U, F): _ck(lib().IGXComputeIFunction(self.h, a, V.h, t, U.h, F.h))
    def compute_ijacobian(self, a, V, t, U, J): _ck(lib().IGXComputeIJacobian(self.h, a, V.h, t, U.h, J.h))

    def compute_ifunction_ijacobian(self, a, V, t, U, F, J):
        """F and J of one Newton step in one pass of the walk where a fused kernel exists (IGXComputeIFunctionIJacobian)."""
        _ck(lib().IGXComputeIFunctionIJacobian(self.h, a, V.h, t, U.h, F.h, J.h))

    def compute_function_jacobian(self, U, F, J): _ck(lib().IGXComputeFunctionJacobian(self.h, U.h, F.h, J.h))

    # matrix-free actions: Y = A X with A the matrix compute_matrix / compute_jacobian / compute_ijacobian would assemble (no matrix is formed)
    def compute_matrix_action(self, X, Y): _ck(lib().IGXComputeMatrixAction(self.h, X.h, Y.h))
    def compute_jacobian_action(self, U, X, Y): _ck(lib().IGXComputeJacobianAction(self.h, U.h, X.h, Y.h))
    def compute_ijacobian_action(self, a, V, t, U, X, Y): _ck(lib().IGXComputeIJacobianAction(self.h, a, V.h, t, U.h, X.h, Y.h))
    # the same actions on a block: X and Y are lists of Vecs of one length (1 .. 48), Y[j] = A X[j], IGX_ACTION_MAXCOLS = 16 columns per launch
    @staticmethod
    def _block(X, Y):
        if len(X) != len(Y):
            raise ValueError("the block action takes as many results as directions, got %d and %d" % (len(Y), len(X)))
        return len(X), (C.c_void_p * max(len(X), 1))(*[x.h.value for x in X]), (C.c_void_p * max(len(Y), 1))(*[y.h.value for y in Y])
    def compute_matrix_action_block(self, X, Y): _ck(lib().IGXComputeMatrixActionBlock(self.h, *self._block(X, Y)))
    def compute_jacobian_action_block(self, U, X, Y): _ck(lib().IGXComputeJacobianActionBlock(self.h, U.h, *self._block(X, Y)))
    def compute_ijacobian_action_block(self, a, V, t, U, X, Y): _ck(lib().IGXComputeIJacobianActionBlock(self.h, a, V.h, t, U.h, *self._block(X, Y)))
    def set_batched_actions(self, flag):
        """flag = 1: IGXEigenSolve on this IGX (as stiff) applies both operators through the block actions; 0 (the default): column by column"""
        _ck(lib().IGXSetBatchedActions(self.h, int(flag)))
    # matrix-free diagonals: D = diag A of the operator the matching action applies (a fixed dof holds its element count)
    def compute_matrix_diagonal(self, D): _ck(lib().IGXComputeMatrixDiagonal(self.h, D.h))
    def compute_jacobian_diagonal(self, U, D): _ck(lib().IGXComputeJacobianDiagonal(self.h, U.h, D.h))
    def compute_ijacobian_diagonal(self, a, V, t, U, D): _ck(lib().IGXComputeIJacobianDiagonal(self.h, a, V.h, t, U.h, D.h))
    # matrix-free point-block diagonals: B is a list of dof Vecs, B[j][node * dof + i] = A_(node,i),(node,j) of the same operator
    @staticmethod
    def _cols(B): return len(B), (C.c_void_p * max(len(B), 1))(*[b.h.value for b in B])
    def compute_matrix_block_diagonal(self, B): _ck(lib().IGXComputeMatrixBlockDiagonal(self.h, *self._cols(B)))
    def compute_jacobian_block_diagonal(self, U, B): _ck(lib().IGXComputeJacobianBlockDiagonal(self.h, U.h, *self._cols(B)))
    def compute_ijacobian_block_diagonal(self, a, V, t, U, B): _ck(lib().IGXComputeIJacobianBlockDiagonal(self.h, a, V.h, t, U.h, *self._cols(B)))
    def block_diagonal_invert(self, B, count=True):
        """B <- the inverse of every block, in place; returns the number of singular blocks (zeroed), or None with count=False (no synchronisation)"""
        n = C.c_int64(0)
        _ck(lib().IGXBlockDiagonalInvert(self.h, *self._cols(B), C.byref(n) if count else None))
        return int(n.value) if count else None
    def block_diagonal_apply(self, B, X, Y): _ck(lib().IGXBlockDiagonalApply(self.h, *self._cols(B), X.h, Y.h))
    # fast diagonalisation: the exact inverse of alpha M + sum_d beta_d K_d on the parametric space, field by field (ignores the geometry)
    def fast_diag_setup(self, alpha, beta):
        """host work only; returns the number of modes whose reciprocal denominator was set to 0 (a pseudo-inverse)"""
        nz = C.c_int(0)
        _ck(lib().IGXFastDiagSetUp(self.h, float(alpha), (C.c_double * 3)(*[float(b) for b in beta]), C.byref(nz)))
        return int(nz.value)
    def fast_diag_apply(self, R, Z): _ck(lib().IGXFastDiagApply(self.h, R.h, Z.h))
    def fast_diag_get_axis(self, axis, field=0):
        """(first free function, m, Lambda [m] ascending, U [m, m] with U[:, k] eigenvector k) of the eigen-system `field` uses on `axis`"""
        first, m = C.c_int(0), C.c_int(0)
        _ck(lib().IGXFastDiagGetAxis(self.h, axis, field, C.byref(first), C.byref(m), None, None))
        lam, U = np.zeros(m.value), np.zeros(m.value * m.value)
        _ck(lib().IGXFastDiagGetAxis(self.h, axis, field, None, None, lam.ctypes.data_as(_dp), U.ctypes.data_as(_dp)))
        return int(first.value), int(m.value), lam, U.reshape(m.value, m.value).T.copy()

    def solve(self, b, x, method="cg", op="matrix", pc="none", rtol=1e-10, atol=0.0, maxit=1000, a=0.0, t=0.0, V=None, U=None, history=False):
        """IGXSolve: A x = b on the device with A the action `op` names at the state (a, V, t, U), from the guess x holds.  Returns a dict of
        the info fields (iterations, reason, reason_name, rnorm0, rnorm, bnorm) and, with history=True, |r_k| for k = 0 .. iterations.
        On a partition (set_comm and a communicator) every rank calls it: b complete on the owned rows (reduce_ghost_rows), U and V with their
        ghosts; only the owned rows of b and x are read, x returns with its ghosts refreshed, and the info and the history are the same bits on
        every rank (the inner products are added across the ranks in rank order).  pc="fastdiag" needs one rank on every axis."""
        code = lambda table, v: table[v] if isinstance(v, str) else int(v)
        spec = IGXSolveSpec(code(SOLVE_METHODS, method), code(SOLVE_OPERATORS, op), code(SOLVE_PCS, pc), float(a), float(t),
                            V.h if V is not None else None, U.h if U is not None else None, float(rtol), float(atol), int(maxit))
        info = IGXSolveInfo()
        hist = np.zeros(max(int(maxit), 0) + 1) if history else None
        _ck(lib().IGXSolve(self.h, C.byref(spec), b.h if b is not None else None, x.h if x is not None else None, C.byref(info),
                           hist.ctypes.data_as(_dp) if history else None))
        out = dict(iterations=info.iterations, reason=info.reason, reason_name=SOLVE_REASONS.get(info.reason, str(info.reason)),
                   rnorm0=info.rnorm0, rnorm=info.rnorm, bnorm=info.bnorm)
        if history:
            out["history"] = hist[:info.iterations + 1].copy()
        return out

    def krylov_sweep_time(self, sweep, runs, reps=20):
        """IGXKrylovSweepTime: the mean time in ms of `reps` launches of the fused sweep `sweep` (a name of KRYLOV_SWEEPS or its index), over the
        owned rows of this IGX's partition (runs=True) or as the contiguous kernel over as many entries (runs=False)."""
        ms = C.c_double(0.0)
        _ck(lib().IGXKrylovSweepTime(self.h, KRYLOV_SWEEPS.index(sweep) if isinstance(sweep, str) else int(sweep), int(bool(runs)), int(reps), C.byref(ms)))
        return ms.value

    def eigen(self, nev, mass=None, block=None, pc="none", rtol=1e-8, atol=0.0, maxit=200, X=None, history=False):
        """IGXEigenSolve: the nev lowest eigenpairs of A x = lambda B x by LOBPCG on the device, A this IGX's matrix action, B that of the
        IGX `mass` on the same space (None: the identity).  block (default min(16, nev + 2)) columns iterate; X: the start block, a list of
        block Vecs (default: numpy.random.default_rng(0).standard_normal, written from the host).  Returns a dict: "lambda" [block]
        ascending, "X" (the Vecs, B-orthonormal Ritz vectors), "resid" [block], the info fields (iterations, reason, reason_name, nconverged,
        restarts, actions) and, with history=True, "history" [iterations + 1, block] of |r_j|."""
        nev = int(nev)
        m = min(16, nev + 2) if block is None else int(block)
        if X is None:
            X = []
            if 1 <= nev <= m <= 16:      # (otherwise the call refuses the specification before it looks at the block)
                rng = np.random.default_rng(0)
                for _ in range(m):
                    v = self.create_vec()
                    X.append(v.set(rng.standard_normal(v.n)))
        X = list(X)
        spec = IGXEigenSpec(nev, m, SOLVE_PCS[pc] if isinstance(pc, str) else int(pc), float(rtol), float(atol), int(maxit))
        info = IGXEigenInfo()
        lam, res = np.zeros(max(m, 1)), np.zeros(max(m, 1))
        hist = np.zeros((max(int(maxit), 0) + 1, max(m, 1))) if history else None
        _ck(lib().IGXEigenSolve(self.h, mass.h if mass is not None else None, C.byref(spec), len(X), _vec_array(X), lam.ctypes.data_as(_dp), res.ctypes.data_as(_dp),
                                C.byref(info), hist.ctypes.data_as(_dp) if history else None))
        out = {k: getattr(info, k) for k, _ in IGXEigenInfo._fields_}
        out["reason_name"] = EIGEN_REASONS.get(info.reason, str(info.reason))
        out["lambda"], out["X"], out["resid"] = lam[:m].copy(), X, res[:m].copy()
        if history:
            out["history"] = hist[:info.iterations + 1, :m].copy()
        return out

    def solve_nonlinear(self, x, op="jacobian", W=None, a=0.0, t=0.0, method="bicgstab", pc="none", lin_rtol=1e-5, lin_atol=0.0, lin_maxit=1000,
                        forcing="constant", rtol=1e-8, atol=0.0, stol=0.0, maxit=50, linesearch="basic", max_backtracks=10):
        """IGXSolveNonlinear: Newton's method on G(x) = 0 on the device from the guess x holds, G the residual `op` names -- "jacobian":
        compute_function(x); "ijacobian": compute_ifunction(a, a x + W, t, x) -- with solve() as the linear solve.  Returns a dict of the
        info fields (iterations, reason, reason_name, linear_iterations, function_evaluations, backtracks, last_linear_reason, fnorm0, fnorm,
        snorm, xnorm), history (|F_k| for k = 0 .. iterations) and linear_its (the inner iterations of each step)."""
        code = lambda table, v: table[v] if isinstance(v, str) else int(v)
        spec = IGXNewtonSpec(code(SOLVE_OPERATORS, op), float(a), float(t), W.h if W is not None else None, code(SOLVE_METHODS, method), code(SOLVE_PCS, pc),
                             float(lin_rtol), float(lin_atol), int(lin_maxit), code(NEWTON_FORCINGS, forcing), float(rtol), float(atol), float(stol), int(maxit),
                             code(NEWTON_LINESEARCHES, linesearch), int(max_backtracks))
        info = IGXNewtonInfo()
        hist, lin = np.zeros(max(int(maxit), 0) + 1), np.full(max(int(maxit), 1), -1, dtype=np.int32)
        _ck(lib().IGXSolveNonlinear(self.h, C.byref(spec), x.h if x is not None else None, C.byref(info), hist.ctypes.data_as(_dp), lin.ctypes.data_as(_ip)))
        out = {k: getattr(info, k) for k, _ in IGXNewtonInfo._fields_}
        out["reason_name"] = NEWTON_REASONS.get(info.reason, str(info.reason))
        out["history"] = hist[:info.iterations + 1].copy()
        out["linear_its"] = lin[lin >= 0].astype(int)      # one per inner solve: a step that ends the call in its line search or its solve has one too
        return out

    def time_step(self, U, V, dt, max_time=float("inf"), max_steps=1, rho_inf=None, scheme=None, alpha=None, t0=0.0, adapt=False, adapt_rtol=1e-3, adapt_atol=1e-3,
                  dt_min=0.0, dt_max=float("inf"), max_rejections=10, resume=False, nlog=None, method="bicgstab", pc="none", lin_rtol=1e-5, lin_atol=0.0,
                  lin_maxit=1000, forcing="constant", rtol=1e-8, atol=0.0, stol=0.0, maxit=50, linesearch="basic", max_backtracks=10):
        """IGXTimeStep: generalized-alpha steps on the device from U = U_n, V = dU/dt at t0, each stage one solve_nonlinear(op="ijacobian") with
        the Newton keywords given here.  The scheme: rho_inf (default 0.5), scheme="backward_euler" or alpha=(alpha_m, alpha_f, gamma).  U and V
        hold the last accepted state on return.  Returns a dict of the info fields (steps, reason, reason_name, rejections, attempts,
        newton_iterations, linear_iterations, function_evaluations, t, dt_last, dt_next, unorm) and log, a structured array with one record
        per attempt (t, dt, wlte, accepted, newton_iterations, newton_reason, linear_iterations)."""
        code = lambda table, v: table[v] if isinstance(v, str) else int(v)
        am, af, g = alpha_scheme(rho_inf, scheme, alpha)
        newton = IGXNewtonSpec(SOLVE_OPERATORS["ijacobian"], 0.0, 0.0, None, code(SOLVE_METHODS, method), code(SOLVE_PCS, pc), float(lin_rtol), float(lin_atol),
                               int(lin_maxit), code(NEWTON_FORCINGS, forcing), float(rtol), float(atol), float(stol), int(maxit),
                               code(NEWTON_LINESEARCHES, linesearch), int(max_backtracks))
        spec = IGXTimeStepSpec(am, af, g, float(t0), float(dt), float(max_time), int(max_steps), int(bool(adapt)), float(adapt_rtol), float(adapt_atol),
                               float(dt_min), float(dt_max), int(max_rejections), int(bool(resume)), newton)
        if nlog is None:
            nlog = max(int(max_steps), 0) * (max(int(max_rejections), 0) + 1 if adapt else 1)
        nlog = min(max(int(nlog), 1), 1 << 16)
        log = (IGXTimeStepLog * nlog)()
        info = IGXTimeStepInfo()
        _ck(lib().IGXTimeStep(self.h, C.byref(spec), U.h if U is not None else None, V.h if V is not None else None, C.byref(info), log, nlog))
        out = {k: getattr(info, k) for k, _ in IGXTimeStepInfo._fields_}
        out["reason_name"] = TS_REASONS.get(info.reason, str(info.reason))
        out["log"] = np.frombuffer(log, dtype=TS_LOG_DTYPE, count=min(info.attempts, nlog)).copy()
        return out

    def probe(self, points, order=0):
        """IGXProbeCreate: a Probe of the parametric points [npts, dim]; order (0..3) is the highest derivative evaluate() may be asked for."""
        return Probe(self, points, order)

    def transfer(self, coarse):
        """IGXTransferCreate: a Transfer from the IGX `coarse` to this one; the knot vectors must be nested (h-refinement by knot insertion)."""
        return Transfer(self, coarse)

    def multigrid(self, coarser_levels, **kw):
        """IGXMultigridCreate: a Multigrid over `coarser_levels` (coarsest first) and this IGX as the finest level; keywords: Multigrid's."""
        return Multigrid(list(coarser_levels) + [self], **kw)

    def set_stream(self, stream): _ck(lib().IGXSetStream(self.h, stream))
    def synchronize(self): _ck(lib().IGXSynchronize(self.h))
    def set_kernel(self, which): _ck(lib().IGXSetKernel(self.h, which))
    def set_timing(self, flag=True): _ck(lib().IGXSetTiming(self.h, int(flag)))

    def kernel_name(self):
        buf = C.create_string_buffer(1024)
        _ck(lib().IGXGetKernelName(self.h, buf, 1024))
        return buf.value.decode()

    def last_timing(self):
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        _ck(lib().IGXGetLastTiming(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def dominant_kernel(self):
        buf = C.create_string_buffer(128)
        ms, n, el, fl = C.c_double(), C.c_int(), C.c_int64(), C.c_double()
        _ck(lib().IGXGetDominantKernelTiming(self.h, buf, 128, C.byref(ms), C.byref(n), C.byref(el), C.byref(fl)))
        return dict(name=buf.value.decode(), ms=ms.value, launches=n.value, elements=el.value, executed_flop_per_element=fl.value)

    def neighbors(self, send):
        """[(peer rank, matrix doubles, vector doubles)] of the send (upper) or receive (lower) list."""
        ns, nr = C.c_int(), C.c_int()
        _ck(lib().IGXGetNeighborCount(self.h, C.byref(ns), C.byref(nr)))
        out = []
        for k in range(ns.value if send else nr.value):
            r, m, v = C.c_int(), C.c_int64(), C.c_int64()
            _ck(lib().IGXGetNeighborInfo(self.h, int(send), k, C.byref(r), C.byref(m), C.byref(v)))
            out.append((r.value, m.value, v.value))
        return out

    # -- the exchange inside the library (RCCL, or a host-callback transport)
    @staticmethod
    def comm_unique_id(librccl=None):
        buf = C.create_string_buffer(128)
        _ck(lib().IGXCommGetUniqueId(buf, librccl.encode() if librccl else None))
        return buf.raw

    def comm_init_rccl(self, unique_id, librccl=None):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _ck(lib().IGXCommInitRCCL(self.h, buf, librccl.encode() if librccl else None))

    def comm_init_transport(self, pyfn):
        """pyfn(send=[(peer, devptr, count)], recv=[(peer, devptr, count)]) moves the packed device buffers."""
        def tramp(ctx, ns, sp, sb, sn, nr, rp, rb, rn):
            try:
                pyfn([(sp[i], sb[i], sn[i]) for i in range(ns)], [(rp[i], rb[i], rn[i]) for i in range(nr)])
                return 0
            except Exception as e:      # never unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        self._transport = TRANSPORT_FN(tramp)     # keep the trampoline alive
        _ck(lib().IGXCommInitTransport(self.h, self._transport, None))

    def comm_destroy(self): _ck(lib().IGXCommDestroy(self.h))
    def reduce_ghost_rows(self, A=None, b=None): _ck(lib().IGXReduceGhostRows(self.h, A.h if A is not None else None, b.h if b is not None else None))
    def refresh_ghosts(self, v): _ck(lib().IGXRefreshGhosts(self.h, v.h))

    def comm_all_sum(self, values):
        """IGXCommAllSum: the sum of `values` (1 to 64 numbers) over all ranks, added in rank order -- the same bits on every rank.  Collective
        and blocking; on one rank the values come back as they are.  It finishes Vec.dot, Vec.norm (the squares) and checksum on a partition."""
        v = np.array(values, dtype=np.float64).ravel()
        _ck(lib().IGXCommAllSum(self.h, int(v.size), v.ctypes.data_as(_dp)))
        return v

    def comm_last_bytes(self):
        n = C.c_int64()
        _ck(lib().IGXCommGetLastBytes(self.h, C.byref(n)))
        return n.value

    def comm_ranks(self):
        """(transport kind: "rccl" / "host" / None, ranks the transport itself reports: ncclCommCount for RCCL)."""
        k, n = C.c_int(0), C.c_int(0)
        _ck(lib().IGXCommGetRanks(self.h, C.byref(k), C.byref(n)))
        return {0: None, 1: "rccl", 2: "host"}[k.value], n.value

    def comm_loopback_test(self, n=1 << 20):
        d = C.c_double()
        _ck(lib().IGXCommLoopbackTest(self.h, n, C.byref(d)))
        return d.value

    def pack_ghost_rows(self, A, b, k, devptr): _ck(lib().IGXPackGhostRows(self.h, A.h if A else None, b.h if b else None, k, devptr))
    def unpack_ghost_rows(self, A, b, k, devptr): _ck(lib().IGXUnpackGhostRows(self.h, A.h if A else None, b.h if b else None, k, devptr))
    def pack_owner_values(self, v, k, devptr): _ck(lib().IGXPackOwnerValues(self.h, v.h, k, devptr))
    def unpack_ghost_values(self, v, k, devptr): _ck(lib().IGXUnpackGhostValues(self.h, v.h, k, devptr))
    def row_owned(self, r0, r1=0, r2=0): return bool(lib().IGXRowOwned(self.h, r0, r1, r2))

    def checksum(self, A=None, b=None):
        """[sum A, sum |A|, sum b, sum b^2] over the rows this rank owns."""
        out = np.zeros(4)
        _ck(lib().IGXChecksum(self.h, A.h if A is not None else None, b.h if b is not None else None, out.ctypes.data_as(_dp)))
        return out

    def check_form_source(self, with_matrix=True, gram=False):
        """Compile-only check of the run-time form against the kernels the drivers would launch for the current degrees (no GPU needed)."""
        # gram: False / True = the struct declares MAT_PAIR_MASK; 2, 3, 4 = the pencil walk / the vector kernel / state_pencil instead; 7 = the vector kernel's ACTION instantiation (compute_*_action); 8 = its DIAGONAL instantiation (compute_*_diagonal); 9 = DIAGONAL with BLOCK (compute_*_block_diagonal)
        _ck(lib().IGXCheckFormSource(self.h, 1 if with_matrix else 0, int(gram)))

    def comm_overlap_ms(self):
        """ms by which the upper face of axis 2 was packed before the end of the assembly in the last reduce_ghost_rows."""
        ms = C.c_double(0)
        _ck(lib().IGXCommGetOverlap(self.h, C.byref(ms)))
        return ms.value

    def comm_link_rate(self):
        """(GB/s per direction, source, probe ms, faces): what the face-first decision uses (IGXCommGetLinkRate)."""
        gbs, src, ms, faces = C.c_double(0), C.c_int(0), C.c_double(0), C.c_int(0)
        _ck(lib().IGXCommGetLinkRate(self.h, C.byref(gbs), C.byref(src), C.byref(ms), C.byref(faces)))
        return gbs.value, ("constant", "measured", "env")[src.value], ms.value, faces.value

    def face_passes(self):
        n = C.c_int(0)
        _ck(lib().IGXGetFacePasses(self.h, C.byref(n)))
        return n.value

    def comm_early_phases(self):
        """phases (upper faces of axes 2, 1, 0) of the last reduce_ghost_rows that were packed behind a face mark of the assembly"""
        n = C.c_int(0)
        _ck(lib().IGXCommGetEarlyPhases(self.h, C.byref(n)))
        return n.value

    def clock_probe(self):
        """(shader MHz, elements walked) over the probe workgroups of the pencil-kernel launches since the last call; needs IGX_CLOCK_PROBE=1 at creation."""
        mhz, ne = C.c_double(0), C.c_int64(0)
        _ck(lib().IGXGetClockProbe(self.h, C.byref(mhz), C.byref(ne)))
        return mhz.value, ne.value

    def coloring(self):
        nc = (C.c_int * 3)()
        _ck(lib().IGXGetColoring(self.h, nc))
        return list(nc)

    def element_color(self, axis, e): return lib().IGXGetElementColor(self.h, axis, e)


def device_info():
    buf = C.create_string_buffer(256)
    lib().IGXGetDeviceInfo(buf, 256)
    return buf.value.decode()


def patch3_ticket_order(n1, n2, nseg, cx, cy, order=1):
    """The p = 3 patch walk's ticket -> item map of colour (cx, cy) on a mesh of n1 x n2 elements (axes 1, 2) in nseg segments, from the
    library's own helper (host side, no device): (items, faces) as int arrays over the tickets; empty when the colour has no patch."""
    n = C.c_int(0)
    _ck(lib().IGXPatch3TicketOrder(n1, n2, nseg, cx, cy, order, 0, C.byref(n), None, None))
    items, faces = np.zeros(max(n.value, 1), dtype=np.int32), np.zeros(max(n.value, 1), dtype=np.int32)
    _ck(lib().IGXPatch3TicketOrder(n1, n2, nseg, cx, cy, order, n.value, C.byref(n), items.ctypes.data_as(_ip), faces.ctypes.data_as(_ip)))
    return items[:n.value], faces[:n.value]


def rows3_stage_offset(col, dy, dx, d):
    """Where the entry (node column col of the tile, dy, dx, d) lies in the p = 3 rows walk's staged tile-layer, and the buffer's doubles,
    from the function the kernel itself calls (host side, no device)."""
    off, n = C.c_int(0), C.c_int(0)
    _ck(lib().IGXRows3StageOffset(col, dy, dx, d, C.byref(off), C.byref(n)))
    return off.value, n.value
