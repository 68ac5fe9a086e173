"""Where the matrix-free operators run and what they say where they do not: one table for the actions (IGXCompute*Action), the actions
on a block (IGXCompute*ActionBlock), the diagonals, the point-block diagonals and IGXSolve on top of them.  A row is
(form or struct, call, condition) -> (code, the exact message), or -> (the exact kernel name, launches) where the pass runs.  The messages
and the order in which the rules answer are part of the library's behaviour (include/petiga_amd.h); the table pins them:
  a built-in form the action covers      the space answers first (boundary-form faces, dim, nsd, lanes, IGX_VEC_SUMFACT, IGXSetKernel), then dof
  a built-in form it does not cover      faces, dim, then the form (order 3 / property / map derivatives, then boundary branch or functionals);
                                         IGXSetKernel is not asked
  a run-time struct                      NSCALAR and dof before anything else; its boundary message has no "or functionals"
  the diagonals                          the action's space rules under "the matrix diagonal runs where ...", then the form: general, boundary,
                                         second-order shape features; then dof
  block diagonal, block action, IGXSolve the same reasons under their own prefixes (an IGX_ERR_ARG_WRONG keeps its plain text)
A geometry with nsd < dim cannot be given (IGXSetGeometry refuses it), so the action's nsd rule is out of reach of the C ABI; the row
"nsd 2 on dim 3" pins that refusal, and the row "dim 2 with nsd 3" that dim answers before nsd.
Every case creates its own IGX; a refusal launches nothing (the kernel name stays "none")."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ARG_WRONG, OUTOFRANGE, SUP = 62, 63, 56

A_VISIT = "the matrix action does not cover boundary-form passes (IGXSetBoundaryForm): it runs on vec_sumfact alone"
A_DIM = "the matrix action needs dim = 3 (vec_sumfact: sum factorisation in three dimensions)"
A_KERNEL = "the matrix action runs on vec_sumfact alone: IGXSetKernel must leave the choice automatic (0)"
A_GENERAL = "the matrix action does not cover forms of order 3 or forms that read the property array or the geometry map's derivatives"
A_BOUNDARY_RTC = "the matrix action does not cover forms with a boundary branch"
A_BOUNDARY = A_BOUNDARY_RTC + " or functionals"
D_WHERE = "the matrix diagonal runs where the matrix action runs, and "
D_SECOND = ("the matrix diagonal does not cover forms with second-order shape features (Cahn-Hilliard's Laplacian): six product rows per axis "
            "and 55 coefficient slots per point are another kernel")
D_GENERAL = "the matrix diagonal does not cover forms of order 3 or forms that read the property array or the geometry map's derivatives"
D_BOUNDARY_RTC = "the matrix diagonal does not cover forms with a boundary branch"
D_BOUNDARY = D_BOUNDARY_RTC + " or functionals"
B_WHERE = "the matrix block diagonal runs where the matrix diagonal runs, and "
AB_WHERE = "the matrix action on a block runs where the matrix action runs, and "
K_WHERE = "the Krylov solve runs where its operator and its preconditioner run, and "
DOF = "form does not match the number of fields (dof)"
NSCALAR = "a struct with NSCALAR is a functional: IGXComputeScalarSource"
NSD = "Number of space dimensions must be in range [dim,3]"
CH = (1.5, 200.0, 0.63, 1.0, 1.0 / 48.0, 1.0)

STRUCTS = r"""
struct UserDiffusion {
  static constexpr int DOF = 1, ORDER = 1; static constexpr unsigned NEED = NEED_X;
  static constexpr unsigned MAT_TEST_MASK = 0xEu, VEC_TEST_MASK = 0x1u;
  static __device__ void mat(const PtView &p, const double *Na, const double *Nb, double *T) {
    const double d00 = 1.0 + p.x[0], d11 = 2.0, d22 = 1.0 + p.x[1] * p.x[2], d01 = 0.3 * p.x[0];
    T[0] = d00 * Na[1] * Nb[1] + d11 * Na[2] * Nb[2] + d22 * Na[3] * Nb[3] + d01 * (Na[1] * Nb[2] + Na[2] * Nb[1]);
  }
  static __device__ void vec(const PtView &p, const double *Na, double *R) { R[0] = Na[0] * p.prm[0]; }
};
struct UserBiharmonic2 {      // SHAPE_ORDER 2 (from ORDER), two fields
  static constexpr int DOF = 2, ORDER = 2; static constexpr unsigned NEED = NEED_U;
  static __device__ void mat(const PtView &p, const double *Na, const double *Nb, double *T) {
    const double la = Na[4] + Na[8] + Na[12], lb = Nb[4] + Nb[8] + Nb[12];
    T[0] = la * lb + p.shift * Na[0] * Nb[0]; T[1] = Na[0] * Nb[1] * p.u[0]; T[2] = Na[2] * Nb[0]; T[3] = Na[0] * Nb[0] + la * lb;
  }
  static __device__ void vec(const PtView &, const double *Na, double *R) { R[0] = Na[0]; R[1] = 0.0; }
};
struct UserNeumann {          // a boundary branch
  static constexpr int DOF = 1, ORDER = 1; static constexpr unsigned NEED = 0;
  static constexpr bool HAS_BOUNDARY = true;
  static __device__ void mat(const PtView &, const double *Na, const double *Nb, double *T) { T[0] = Na[1] * Nb[1] + Na[2] * Nb[2] + Na[3] * Nb[3]; }
  static __device__ void vec(const PtView &, const double *, double *R) { R[0] = 0.0; }
  static __device__ void bmat(const PtView &, const double *, const double *, double *T) { T[0] = 0.0; }
  static __device__ void bvec(const PtView &, const double *Na, double *R) { R[0] = Na[0]; }
};
struct UserVolume {           // a functional
  static constexpr int DOF = 1, ORDER = 1, NSCALAR = 1; static constexpr unsigned NEED = 0;
  static __device__ void scalar(const PtView &, double *S) { S[0] = 1.0; }
};
"""


def _map(p, n):
    """a smooth polynomial perturbation of the unit cube on the space's own control net, axis 0 fastest"""
    t = np.linspace(0.0, 1.0, n + p)
    z, y, x = np.meshgrid(t, t, t, indexing="ij")
    s = 0.03 * np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)
    return np.stack([x + s, y - s, z + s], axis=-1).reshape(-1, 3)


def _space(p=2, n=4, dim=3, dof=1, geometry=False):
    import petiga_amd as P
    g = P.IGX(dim, dof)
    for i in range(dim):
        g.axis_uniform(i, p, n)
    g.setup()
    if geometry:
        g.set_geometry(_map(p, n))
    return g


def _form(g, form):
    if form.startswith("User"):
        g.set_form_source(STRUCTS, form, (0.7,))
    else:
        g.set_form(form, CH if form == "cahnhilliard" else ())
    return g


def _call(g, kind):
    """one call of the kind on fresh vectors; the results on the host"""
    n = g.create_vec().n
    rng = np.random.default_rng(5)
    vec = lambda: g.create_vec().set(rng.standard_normal(n))
    state = g_state = None
    if kind.endswith("@state"):      # the IJacobian drivers (Cahn-Hilliard)
        kind = kind[:-6]
        state, g_state = g.create_vec().set(0.63 + 0.05 * rng.standard_normal(n)), g.create_vec().set(0.01 * rng.standard_normal(n))
    if kind == "action":
        X, Y = vec(), [g.create_vec()]
        g.compute_matrix_action(X, Y[0])
    elif kind.startswith("block") and kind != "block_diagonal":      # block1, block3, block17: the action on that many columns
        k = int(kind[5:])
        X, Y = [vec() for _ in range(k)], [g.create_vec() for _ in range(k)]
        g.compute_matrix_action_block(X, Y)
    elif kind == "diagonal":
        Y = [g.create_vec()]
        g.compute_ijacobian_diagonal(250.0, g_state, 0.0, state, Y[0]) if state is not None else g.compute_matrix_diagonal(Y[0])
    elif kind == "block_diagonal":
        Y = [g.create_vec() for _ in range(g.dof)]
        g.compute_ijacobian_block_diagonal(250.0, g_state, 0.0, state, Y) if state is not None else g.compute_matrix_block_diagonal(Y)
    else:      # solve-none, solve-jacobi, solve-pbjacobi
        b, Y = vec(), [g.create_vec()]
        kw = dict(op="ijacobian", a=250.0, U=state, V=g_state) if state is not None else {}
        g.solve(b, Y[0], method="cg", pc=kind[6:], rtol=1e-30, maxit=5, **kw)
    g.synchronize()
    return [y.get().copy() for y in Y]


# ---------------------------------------------------------------- refusals
def _visit(g): g.set_boundary_form(0, 1, True)
def _kernel2(g): g.set_kernel(2)
def _none(g): pass


def _under(kinds, msg, diag_msg=None):
    """the reason under every call's own name: {kind: message}"""
    diag_msg = diag_msg if diag_msg is not None else D_WHERE + msg
    out = {"action": msg, "block3": AB_WHERE + msg, "diagonal": diag_msg, "block_diagonal": B_WHERE + diag_msg,
           "solve-none": K_WHERE + msg, "solve-jacobi": K_WHERE + diag_msg, "solve-pbjacobi": K_WHERE + B_WHERE + diag_msg}
    return {k: out[k] for k in kinds}


ALL = ("action", "block3", "diagonal", "block_diagonal", "solve-none", "solve-jacobi", "solve-pbjacobi")
REFUSALS = []      # (id, space keywords, form, condition, kind, code, message)


def _rows(name, kw, form, cond, table, code=SUP):
    for kind, msg in table.items():
        REFUSALS.append(pytest.param(kw, form, cond, kind, code, msg, id="%s-%s" % (name, kind)))


# a boundary-form face: the space's first rule, under every name (IGXSolve asks the space before its preconditioner)
_rows("poisson-face", {}, "poisson", _visit, {**_under(ALL, A_VISIT), "solve-jacobi": K_WHERE + A_VISIT, "solve-pbjacobi": K_WHERE + A_VISIT})
# dim 2 (with and without a geometry of nsd 3: dim answers before nsd)
_rows("poisson-dim2", dict(dim=2), "poisson", _none, _under(("action", "block3", "diagonal", "block_diagonal", "solve-none"), A_DIM))
# IGXSetKernel(2) on a form the action covers ...
_rows("poisson-kernel2", {}, "poisson", _kernel2, {**_under(ALL, A_KERNEL), "solve-jacobi": K_WHERE + A_KERNEL, "solve-pbjacobi": K_WHERE + A_KERNEL})
# ... and on forms it does not: the action answers with the form and does not ask IGXSetKernel, the diagonals ask the space first
_rows("der3-kernel2", {}, "der3", _kernel2, {"action": A_GENERAL, "block3": AB_WHERE + A_KERNEL, "diagonal": D_WHERE + A_KERNEL, "block_diagonal": B_WHERE + D_WHERE + A_KERNEL})
_rows("property-kernel2", {}, "property", _kernel2, {"action": A_GENERAL, "block3": AB_WHERE + A_KERNEL, "diagonal": D_WHERE + A_KERNEL, "block_diagonal": B_WHERE + D_WHERE + A_KERNEL})
_rows("nitsche-kernel2", {}, "nitsche", _kernel2, {"action": A_BOUNDARY, "block3": AB_WHERE + A_KERNEL, "diagonal": D_WHERE + A_KERNEL, "block_diagonal": B_WHERE + D_WHERE + A_KERNEL,
                                                   "solve-none": K_WHERE + A_KERNEL})
_rows("property", {}, "property", _none, _under(("action", "block3", "diagonal", "block_diagonal"), A_GENERAL, D_GENERAL))
# the same forms with the choice left automatic: the form's own rules, under every name
_rows("der3", {}, "der3", _none, _under(("action", "block3", "diagonal", "block_diagonal", "solve-none"), A_GENERAL, D_GENERAL))
_rows("nitsche", {}, "nitsche", _none, _under(("action", "block3", "diagonal", "block_diagonal", "solve-none", "solve-jacobi"), A_BOUNDARY, D_BOUNDARY))
_rows("nitsche-face", {}, "nitsche", _visit, _under(("action", "diagonal"), A_VISIT))
# Cahn-Hilliard: the action covers it, the diagonals do not
_rows("cahnhilliard", {}, "cahnhilliard", _none, {"diagonal@state": D_SECOND, "block_diagonal@state": B_WHERE + D_SECOND,
                                                   "solve-jacobi@state": K_WHERE + D_SECOND, "solve-pbjacobi@state": K_WHERE + B_WHERE + D_SECOND})
# dof: after the space and the form, IGX_ERR_ARG_WRONG under no prefix
_rows("poisson-dof2", dict(dof=2), "poisson", _none, {k: DOF for k in ("action", "block3", "diagonal", "block_diagonal", "solve-none", "solve-jacobi")}, ARG_WRONG)
_rows("poisson-dof2-face", dict(dof=2), "poisson", _visit, _under(("action", "diagonal"), A_VISIT))
# run-time structs: NSCALAR and dof before anything else (the face and IGXSetKernel included), then the space, then the struct
# (the block action asks the space before it reaches the struct, so its rows leave the space alone; each row here is a compilation, hence few)
_rows("struct-nscalar-face", {}, "UserVolume", _visit, {"action": NSCALAR, "block_diagonal": NSCALAR})
_rows("struct-nscalar", {}, "UserVolume", _none, {"block3": AB_WHERE + NSCALAR, "solve-none": K_WHERE + NSCALAR})
_rows("struct-dof2-kernel2", dict(dof=2), "UserDiffusion", _kernel2, {"action": DOF, "diagonal": DOF}, ARG_WRONG)
_rows("struct-dof2", dict(dof=2), "UserDiffusion", _none, {"block3": DOF}, ARG_WRONG)
_rows("struct-boundary", {}, "UserNeumann", _none, _under(("action", "block3", "diagonal", "block_diagonal", "solve-none"), A_BOUNDARY_RTC, D_BOUNDARY_RTC))
_rows("struct-boundary-face", {}, "UserNeumann", _visit, _under(("action", "block3"), A_VISIT))
_rows("struct-second", dict(dof=2), "UserBiharmonic2", _none, {"diagonal": D_SECOND, "block_diagonal": B_WHERE + D_SECOND})
_rows("struct-kernel2", {}, "UserDiffusion", _kernel2, _under(("diagonal", "block_diagonal"), A_KERNEL))


@pytest.mark.parametrize("kw,form,cond,kind,code,message", REFUSALS)
def test_refusal(kw, form, cond, kind, code, message):
    import petiga_amd as P
    g = _form(_space(**kw), form)
    cond(g)
    with pytest.raises(P.IGXError) as e:
        _call(g, kind)
    got = (e.value.code, P.lib().IGXGetLastError().decode())
    print(got)
    assert got == (code, message)
    assert g.kernel_name() == "none"      # nothing was launched


def test_nsd_below_dim_cannot_be_set():
    import petiga_amd as P
    g = _space()
    with pytest.raises(P.IGXError) as e:
        g.set_geometry(_map(2, 4)[:, :2])
    assert e.value.code == OUTOFRANGE and P.lib().IGXGetLastError().decode() == NSD
    g2 = _space(dim=2)      # dim 2 with nsd 3: a surface in space; dim answers before nsd
    t = np.linspace(0.0, 1.0, 6)
    y, x = np.meshgrid(t, t, indexing="ij")
    g2.set_geometry(np.stack([x, y, 0.1 * x * y], axis=-1).reshape(-1, 3))
    g2.set_form("poisson")
    with pytest.raises(P.IGXError) as e:
        _call(g2, "action")
    assert e.value.code == SUP and P.lib().IGXGetLastError().decode() == A_DIM


# ---------------------------------------------------------------- passes that run
WORDS = {"action": "matrix action: sum factorisation forward and backward, ",
         "block": "matrix action on a block: sum factorisation forward and backward, ",
         "bycolumn": "matrix action on a block, column by column: sum factorisation forward and backward, ",
         "diagonal": "matrix diagonal: sum factorisation forward, product rows backward, ",
         "block_diagonal": "matrix block diagonal: sum factorisation forward, product rows backward per field pair, "}
LAYOUT = {2: "two elements per wavefront)", 3: "one wavefront per element)", 4: "one workgroup per element, 6 x 6 x 6 lanes)", 6: "one workgroup per element, 8 x 8 x 8 lanes)"}
SIZES = {2: 4, 3: 4, 4: 2, 6: 2}      # elements per axis: two elements per wavefront, one wavefront per element, the 6- and 8-lane workgroups
KINDS = ("action", "block1", "block3", "block17", "diagonal", "block_diagonal")
RUNS = [pytest.param("poisson", p, geo, kind, id="poisson-p%d-%s-%s" % (p, "map" if geo else "id", kind)) for p in SIZES for geo in (False, True) for kind in KINDS]
# a run-time struct: every call at p = 2, with a geometry and at the 6-lane layout the action alone (each is a compilation)
RUNS += [pytest.param("UserDiffusion", 2, False, kind, id="struct-p2-id-%s" % kind) for kind in ("action", "block3", "diagonal", "block_diagonal")]
RUNS += [pytest.param("UserDiffusion", 2, True, "action", id="struct-p2-map-action"), pytest.param("UserDiffusion", 4, False, "action", id="struct-p4-id-action")]


@pytest.mark.parametrize("form,p,geo,kind", RUNS)
def test_pass_runs_under_its_name(form, p, geo, kind):
    g = _form(_space(p, SIZES[p], geometry=geo), form)
    for d in range(3):
        g.set_boundary_value(d, 0, 0, 0.0)
    Y = _call(g, kind)
    c = g.coloring()
    colours = c[0] * c[1] * c[2]
    struct = form.startswith("User")
    cols = int(kind[5:]) if kind.startswith("block") and kind != "block_diagonal" else 0
    words = WORDS[("bycolumn" if struct else "block") if cols else kind]
    name = ("vec_sumfact<%s>(hiprtc," % form if struct else "vec_sumfact(") + words + LAYOUT[p]
    launches = colours * (cols if struct else -(-cols // 16)) if cols else colours
    got = (g.kernel_name(), g.last_timing()[2])
    print(got)
    assert got == (name, launches)
    assert all(np.all(np.isfinite(y)) and y.any() for y in Y)
