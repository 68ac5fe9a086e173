"""The cases of IGXSolve on a partition, shared by tests/test_solve_ranks_abi.py (the count rule on the CPU) and tests/test_gpu_solve_ranks.py
(the device loop on 2 and 4 ranks): the smallest spaces on which the owned rows of a rank take every run shape of krylov.hpp -- one
contiguous prefix (cut on axis 2 only), runs of dof * nown0 doubles with an odd length and an odd start (cut on axis 0, dof 3), runs of
either kind on four ranks (2 x 2 x 1), and a periodic seam.  Each case names its solves as (method, preconditioner)."""
import ctypes as C

import numpy as np

ALL6 = [(d, s) for d in range(3) for s in range(2)]
CH = (1.5, 200.0, 0.63, 1.0, 1.0 / 108.0, 1.0)      # the Cahn-Hilliard context of tests/test_gpu_matrix_action_ranks.py
CH_SHIFT = 1e3
EL = (1.5, 0.8)
BRATU = 3.5
CASES = {
    "poisson-axis2": dict(form="poisson", dof=1, p=3, N=(6, 5, 9), periodic=(0, 0, 0), procs=(1, 1, 2), rtol=1e-10, maxit=400,
                          bcs=[(d, s, 0, 1.0 + d) for d, s in ALL6], solves=[("cg", "none"), ("cg", "jacobi")]),
    "elasticity-axis0": dict(form="elasticity", dof=3, p=2, N=(5, 4, 4), periodic=(0, 0, 0), procs=(2, 1, 1), rtol=1e-10, maxit=600,
                             bcs=[(0, 0, 0, 0.0), (0, 0, 1, 0.0), (0, 0, 2, 0.0), (0, 1, 0, 0.1)], solves=[("cg", "jacobi"), ("cg", "pbjacobi")]),
    "bratu-2x2": dict(form="bratu", dof=1, p=2, N=(6, 6, 5), periodic=(0, 0, 0), procs=(2, 2, 1), rtol=1e-9, maxit=400,
                      bcs=[(d, s, 0, 0.0) for d, s in ALL6], solves=[("bicgstab", "jacobi")]),
    "ch-seam-axis2": dict(form="cahnhilliard", dof=1, p=2, N=(6, 6, 8), periodic=(1, 1, 1), procs=(1, 1, 2), rtol=1e-9, maxit=400,
                          bcs=[], solves=[("bicgstab", "none")]),
}
# Past one item per wavefront.  A sweep that emits a sum runs 256 workgroups of 8 wavefronts, so only with more than 2048 (run, chunk) items
# does a wavefront take a second item and step its position: many short runs (one chunk each: the run counters step and wrap), runs of three
# chunks (2048 is no multiple of 3: the chunk counter carries into the run counters), and on the top rank one run of more than 2048
# chunks (more chunks than wavefronts).  Too large for the oracle's matrix: the one-rank engine's host loop is their only yardstick.
LONG_CASES = {
    "poisson-many-runs": dict(form="poisson", dof=1, p=2, N=(5, 50, 50), periodic=(0, 0, 0), procs=(2, 1, 1), rtol=0.0, maxit=2,
                              bcs=[(d, s, 0, 0.0) for d, s in ALL6], solves=[("cg", "jacobi"), ("bicgstab", "none")]),
    "poisson-long-runs": dict(form="poisson", dof=1, p=2, N=(521, 31, 31), periodic=(0, 0, 0), procs=(2, 1, 1), rtol=0.0, maxit=2,
                              bcs=[(d, s, 0, 0.0) for d, s in ALL6], solves=[("cg", "jacobi"), ("bicgstab", "none")]),
}
EVERY = dict(CASES, **LONG_CASES)
FORM_PARAMS = {"poisson": (), "elasticity": EL, "bratu": (BRATU,), "cahnhilliard": CH}


def world(name):
    return int(np.prod(EVERY[name]["procs"]))


def states(name, n):
    """(U, V) of the case's operator: the random state the Jacobian is taken at (None where the operator has none)"""
    rng = np.random.default_rng(5)
    form = EVERY[name]["form"]
    if form == "bratu":
        return 0.3 * rng.standard_normal(n), None
    if form == "cahnhilliard":
        return 0.63 + 0.05 * (2 * rng.random(n) - 1), rng.standard_normal(n)
    return None, None


def solve_keywords(name, U=None, V=None):
    """the keywords of IGX.solve that name the case's operator at its state (U, V: the engine's vectors)"""
    form = EVERY[name]["form"]
    if form == "bratu":
        return dict(op="jacobian", U=U)
    if form == "cahnhilliard":
        return dict(op="ijacobian", a=CH_SHIFT, t=0.0, V=V, U=U)
    return dict(op="matrix")


def configure(g, name, comm=None):
    """axes, partition, set-up and Dirichlet values of the case on an oracle or an engine; comm = (world, rank) for an engine on a partition"""
    c = EVERY[name]
    if comm is not None:
        g.set_comm(*comm)
        for i in range(3):
            g.set_processors(i, c["procs"][i])
    for i in range(3):
        g.axis_uniform(i, c["p"], c["N"][i], periodic=bool(c["periodic"][i]))
    g.setup()
    for bc in c["bcs"]:
        g.set_boundary_value(*bc)
    return g


def oracle_system(name):
    """(the oracle's matrix of the case as CSR, its right-hand side): the assembled load where the form has one, a fixed random vector otherwise"""
    import oracle_api as O
    c = CASES[name]
    orc = configure(O.OracleIGA(3, c["dof"]), name)
    n = orc.global_size()
    U, V = states(name, n)
    if c["form"] == "poisson":
        A, b = orc.compute_system("orc_form_poisson")
    elif c["form"] == "elasticity":
        A, b = orc.compute_system("orc_form_elasticity", O.ElasticityCtx(*EL))
    elif c["form"] == "bratu":
        A, b = orc.compute_jacobian("orc_form_bratu_jacobian", C.c_double(BRATU), U), None
    else:
        A, b = orc.compute_ijacobian("orc_form_ch_tangent", O.CahnHilliardCtx(*CH), CH_SHIFT, V, 0.0, U), None
    b = np.random.default_rng(41).standard_normal(n) if b is None else np.array(b, dtype=float)
    return A.scipy().tocsr(), b


def owned_sets(name):
    """per rank the global entries it owns, in its own local order, from IGX.sizes() of engines set up on the partition (no device needed)"""
    import petiga_amd as P
    c = CASES[name]
    out = []
    for rank in range(world(name)):
        s = configure(P.IGX(3, c["dof"]), name, comm=(world(name), rank)).sizes()
        ns, lo, wd = s["node_sizes"], s["node_lstart"], s["node_lwidth"]
        i0, i1, i2 = (np.arange(lo[d], lo[d] + wd[d]) % ns[d] for d in range(3))
        node = (i0[None, None, :] + ns[0] * (i1[None, :, None] + ns[1] * i2[:, None, None])).ravel()
        out.append((node[:, None] * c["dof"] + np.arange(c["dof"])[None, :]).ravel())
    return out


def rank_ordered_dot(sets):
    """the inner product of a partitioned solve: each rank's plain sum over the entries it owns, the ranks' sums added in rank order"""
    def dot(a, b):
        s = 0.0
        for idx in sets:
            s += float(np.dot(a[idx], b[idx]))
        return s
    return dot


def preconditioner(A, pc, dof):
    if pc == "none":
        return lambda v: v.copy()
    if pc == "jacobi":
        D = A.diagonal()
        return lambda v: v / D
    n = A.shape[0]
    dense = A.toarray().reshape(n // dof, dof, n // dof, dof)
    inv = np.linalg.inv(np.stack([dense[i, :, i, :] for i in range(n // dof)]))
    return lambda v: np.einsum("nij,nj->ni", inv, v.reshape(-1, dof)).reshape(-1)
