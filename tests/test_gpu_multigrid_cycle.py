"""IGXMultigridApply on the GPU (include/petiga_amd.h; petiga_amd/csrc/multigrid.hpp): one V-cycle against the host loop of
tests/multigrid_ref.py on the SAME engines' operators (actions, diagonals, transfers, coarse preconditioner; one host copy each way per
call), with lambda_l taken from IGXMultigridGetInfo.  The sweeps round every product, quotient and sum on its own, as numpy does, so with a
linear coarse solve (coarse_maxit = 0) the two agree BIT FOR BIT in every entry, with the diagonal and with the point blocks (the block
apply is the engine's kernel on both sides).
  cases          p = 2, 4^3 -> 8^3 -> 16^3; p = 3, 4^3 -> 8^3 (n = 1331, an odd length); a periodic axis; one axis unrefined and one refined
                 3 x; mixed Dirichlet and free faces; p = 2, 21^3 -> 63^3 (n = 274 625: odd, and past the KR_G cap of 256 workgroups of
                 512 pairs), one cycle only
  lambda         against the host's own power iteration (np.linalg.norm): only the summation order of two norms per step differs.
                 LAMBDA_RTOL = 8 x the largest relative deviation seen on an MI355X
  exact zeros    the host loop's trace (the engine's restriction, numpy's mask) has exact zeros on the coarse fixed rows and in the
                 correction on the fine fixed rows; the device equals that loop bit for bit and differs from the unmasked loop
  accounting     launches_per_cycle summed over the levels = the count written down from the loop below = last_timing()'s
  symmetry       with an iterative coarse solve (CG + Jacobi, coarse_rtol = 1e-12) x.By = y.Bx within the CPU test's bound
  refusals       that need vectors or a device
Every test prints what it sees before it asserts (run with -s)."""
import functools

import numpy as np
import pytest

import multigrid_ref as M
import transfer_ref as TR

pytestmark = pytest.mark.gpu
ARG_WRONG, ORDER, SUP = 62, 58, 56
ALL6 = [(d, s) for d in range(3) for s in range(2)]
LAMBDA_RTOL = 8 * 2.4e-16      # measured: the largest relative deviation on the cases of test_lambda_against_the_host_power_iteration is 2.344e-16 (p = 2, n = 1000)

# name -> (p, elements per axis of every level (coarsest first), periodic axes, Dirichlet faces)
CASES = {
    "p2-three-levels": (2, [(4, 4, 4), (8, 8, 8), (16, 16, 16)], (), ALL6),
    "p3-odd-length": (3, [(4, 4, 4), (8, 8, 8)], (), ALL6),
    "periodic-axis": (2, [(4, 4, 4), (8, 8, 8)], (1,), [(0, 0), (0, 1), (2, 0), (2, 1)]),
    "unrefined-and-3x": (2, [(3, 5, 2), (6, 5, 6)], (), ALL6),
    "mixed-faces": (2, [(4, 4, 4), (8, 8, 8)], (), [(0, 0), (1, 1), (2, 0), (2, 1)]),
    "past-the-grid-cap": (2, [(21, 21, 21), (63, 63, 63)], (), ALL6),
}


def poisson_level(p, N, periodic=(), faces=ALL6, dof=1, geometry=None):
    import petiga_amd as P
    g = P.IGX(3, dof)
    for i in range(3):
        g.axis_knots(i, p, TR.uniform_knots(p, N[i], periodic=i in periodic), periodic=i in periodic)
    g.setup()
    if geometry is not None:
        g.set_geometry(*geometry)
    for d, s in faces:
        for f in range(dof):
            g.set_boundary_value(d, s, f, 0.0)
    g.set_form("poisson")
    return g


@functools.lru_cache(maxsize=None)
def engines(name):
    p, Ns, periodic, faces = CASES[name]
    return [poisson_level(p, N, periodic, faces) for N in Ns]


def fixed_of(faces, dof=1):
    return [(d, s, f) for d, s in faces for f in range(dof)]


def device_and_host(levels, fixed, coarse, degree=2, smoother="jacobi", **kw):
    """(the set-up Multigrid, the host Hierarchy with the device's lambdas)"""
    if coarse["pc"] == "fastdiag":
        levels[0].fast_diag_setup(0.0, [1.0, 1.0, 1.0])
    mg = levels[-1].multigrid(levels[:-1], smoother=smoother, degree=degree, coarse=coarse, **kw).setup()
    h = M.engine_callables(levels, fixed, smoother=smoother, coarse=coarse, degree=degree, **kw)
    h.setup(lambdas=[mg.info(l)["lambda_"] for l in range(len(levels))])
    return mg, h


def rhs_of(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


@pytest.mark.parametrize("name,coarse_pc", [("p2-three-levels", "fastdiag"), ("p2-three-levels", "jacobi"), ("p3-odd-length", "fastdiag"), ("periodic-axis", "jacobi"),
                                            ("unrefined-and-3x", "fastdiag"), ("mixed-faces", "jacobi"), ("past-the-grid-cap", "fastdiag")])
def test_one_cycle_equals_the_host_loop_bit_for_bit(name, coarse_pc):
    levels = engines(name)
    p, Ns, periodic, faces = CASES[name]
    mg, h = device_and_host(levels, fixed_of(faces), dict(pc=coarse_pc, maxit=0), degree=3 if name == "p3-odd-length" else 2)
    fine = levels[-1]
    n = fine.create_vec().n
    r, z = fine.create_vec().set(rhs_of(n, 7)), fine.create_vec()
    mg.apply(r, z)
    fine.synchronize()
    name_ = fine.kernel_name()
    E = z.get().copy()
    R = h.apply(r.get())
    differ = int(np.count_nonzero(E != R))
    print("%s, coarse %s x1: n = %d, lambda %s, %d of %d entries differ (max |E - R| = %.3e, max |R| = %.3e); %s"
          % (name, coarse_pc, n, ["%.6f" % mg.info(l)["lambda_"] for l in range(1, len(levels))], differ, n, np.abs(E - R).max(), np.abs(R).max(), name_))
    assert np.all(np.isfinite(E)) and np.abs(E).max() > 0
    assert differ == 0
    # the exact zeros of the loop the device equals, and the unmasked loop is another one
    for l in range(len(levels) - 1):
        cm = M.fixed_mask([TR.nnp_of(p, TR.uniform_knots(p, Ns[l][i], periodic=i in periodic), i in periodic) for i in range(3)], 1, fixed_of(faces))
        assert not h.trace[("restricted", l)][cm].any()
    fm = M.fixed_mask([TR.nnp_of(p, TR.uniform_knots(p, Ns[-1][i], periodic=i in periodic), i in periodic) for i in range(3)], 1, fixed_of(faces))
    assert fm.size == n and not h.trace[("correction", len(levels) - 1)][fm].any()
    if name != "past-the-grid-cap":
        h.wrong = "unmasked"
        assert np.count_nonzero(h.apply(r.get()) != E) > 0
        h.wrong = None
        z2 = fine.create_vec()
        mg.apply(r, z2)
        fine.synchronize()
        assert np.array_equal(z2.get(), E), "two applies differ"
    assert name_.startswith("multigrid(%d levels, chebyshev-jacobi %d, coarse %s x1, vec_sumfact" % (len(levels), mg.spec.degree, coarse_pc)), name_
    mg.close()


def test_point_blocks_equal_the_host_loop_bit_for_bit():
    """elasticity (dof 3) with the Chebyshev smoother on the inverted point blocks, 4^3 -> 8^3, one application of the blocks as the coarse solve"""
    from test_gpu_matrix_action import EL
    faces = [(0, 0), (0, 1)]
    levels = [poisson_level(2, N, faces=faces, dof=3) for N in ((4, 4, 4), (8, 8, 8))]
    for g in levels:
        g.set_form("elasticity", EL)
    mg, h = device_and_host(levels, fixed_of(faces, 3), dict(pc="pbjacobi", maxit=0), degree=3, smoother="pbjacobi")
    fine = levels[-1]
    n = fine.create_vec().n
    r, z = fine.create_vec().set(rhs_of(n, 11)), fine.create_vec()
    mg.apply(r, z)
    fine.synchronize()
    name_ = fine.kernel_name()
    E, R = z.get().copy(), h.apply(r.get())
    print("elasticity, point blocks, degree 3: n = %d, lambda %.6f, %d entries differ (max |E - R| = %.3e); %s"
          % (n, mg.info(1)["lambda_"], np.count_nonzero(E != R), np.abs(E - R).max(), name_))
    assert n == 3000 and np.abs(E).max() > 0 and np.array_equal(E, R)
    assert name_.startswith("multigrid(2 levels, chebyshev-pbjacobi 3, coarse pbjacobi x1, ")
    mg.close()


def test_lambda_against_the_host_power_iteration():
    worst = 0.0
    for name in ("p2-three-levels", "p3-odd-length", "periodic-axis", "mixed-faces"):
        levels = engines(name)
        mg, h = device_and_host(levels, fixed_of(CASES[name][3]), dict(pc="jacobi", maxit=0))
        for l in range(1, len(levels)):
            dev = mg.info(l)["lambda_"]
            host = M.estimate_lambda(h.levels[l].A, h.levels[l].dinv, h.levels[l].n, 10)
            rel = abs(dev - host) / host
            worst = max(worst, rel)
            print("%s level %d (n = %d): lambda %.15g, the host's %.15g, relative deviation %.3e" % (name, l, h.levels[l].n, dev, host, rel))
            assert 1.0 < dev < 2.0 * (CASES[name][0] + 1)
        mg.close()
    print("largest relative deviation %.3e (LAMBDA_RTOL = %.3e)" % (worst, LAMBDA_RTOL))
    assert worst <= LAMBDA_RTOL


def cycle_count(L_A, n_restrict, n_prolong, faces, degree, coarse):
    """the launches of one cycle, level by level, written down from V(l, b) in the header: level 0 is the coarse application; above it
    pre-smoothing mg_cheb_first + (degree - 1) (A, mg_cheb_step); A, mg_resid; the restriction's passes and mg_zero_fixed; the
    prolongation; A, mg_resid, mg_cheb_first + (degree - 1) (A, mg_cheb_step)"""
    out = [coarse]
    for l in range(1, len(L_A)):
        steps = (degree - 1) * (L_A[l] + 1)
        out.append(1 + steps + L_A[l] + 1 + n_restrict[l - 1] + (1 if faces else 0) + n_prolong[l - 1] + L_A[l] + 1 + 1 + steps)
    return out


@pytest.mark.parametrize("name,coarse_pc,degree", [("p2-three-levels", "fastdiag", 2), ("unrefined-and-3x", "jacobi", 3)])
def test_launches_per_cycle(name, coarse_pc, degree):
    levels = engines(name)
    faces = CASES[name][3]
    mg, _ = device_and_host(levels, fixed_of(faces), dict(pc=coarse_pc, maxit=0), degree=degree)
    L_A, n_r, n_p = [], [], []
    for l, g in enumerate(levels):
        X, Y = g.create_vec().set(rhs_of(g.create_vec().n, l)), g.create_vec()
        g.compute_matrix_action(X, Y)
        L_A.append(g.last_timing()[2])
        if l:
            t = g.transfer(levels[l - 1])
            refined = sum(1 for d in range(3) if t.sizes(d)[0] != t.sizes(d)[1])
            n_r.append(max(refined, 1))
            n_p.append(1 if t.info()["fused"] else max(refined, 1))
            t.close()
    want = cycle_count(L_A, n_r, n_p, faces, degree, 6 if coarse_pc == "fastdiag" else 1)
    fine = levels[-1]
    r, z = fine.create_vec().set(rhs_of(fine.create_vec().n, 3)), fine.create_vec()
    mg.apply(r, z)
    got = [mg.info(l)["launches"] for l in range(len(levels))]
    total = fine.last_timing()[2]
    print("%s: L_A %s, restriction passes %s, prolongation launches %s: per level %s, the count %s; last_timing %d" % (name, L_A, n_r, n_p, got, want, total))
    assert got == want and total == sum(want)
    fine.set_timing(True)
    mg.apply(r, z)
    ms, kernel, launches = fine.last_timing()
    fine.set_timing(False)
    print("  timed: %.3f ms, the finest level's operators %.3f ms, %d launches" % (ms, kernel, launches))
    assert launches == sum(want) and 0 < kernel <= ms
    mg.close()


def test_symmetric_with_an_iterative_coarse_solve():
    levels = engines("p2-three-levels")
    mg = levels[-1].multigrid(levels[:-1], coarse=dict(method="cg", pc="jacobi", rtol=1e-12, maxit=500)).setup()
    fine = levels[-1]
    n = fine.create_vec().n
    fm = M.fixed_mask([18] * 3, 1, fixed_of(ALL6))
    worst = 0.0
    for seed in (1, 2):
        x, y = rhs_of(n, seed), rhs_of(n, seed + 10)
        X, Y, BX, BY = fine.create_vec().set(x), fine.create_vec().set(y), fine.create_vec(), fine.create_vec()
        mg.apply(X, BX)
        mg.apply(Y, BY)
        fine.synchronize()
        Bx, By = BX.get(), BY.get()
        gap = abs(x @ By - y @ Bx) / (np.linalg.norm(x) * np.linalg.norm(By))
        worst = max(worst, gap)
    print("iterative coarse solve (cg+jacobi to 1e-12): |x.By - y.Bx| / (|x| |By|) <= %.3e; %s" % (worst, fine.kernel_name()))
    assert worst <= 1e-12
    assert fine.kernel_name().startswith("multigrid(3 levels, chebyshev-jacobi 2, coarse cg+jacobi, vec_sumfact")
    assert fm.size == n
    mg.close()


def test_refusals_that_need_vectors_or_a_device():
    import petiga_amd as P
    from test_gpu_matrix_action import CH
    levels = engines("p3-odd-length")
    fine = levels[-1]
    mg = fine.multigrid(levels[:-1], coarse=dict(pc="jacobi", maxit=0))
    r, z = fine.create_vec(), fine.create_vec()
    with pytest.raises(P.IGXError) as e:      # 10. before SetUp
        mg.apply(r, z)
    assert e.value.code == ORDER and "IGXMultigridSetUp" in str(e.value)
    mg.setup()
    for args in ((r, r), (r, None), (levels[0].create_vec(), z), (r, levels[0].create_vec())):      # 11. aliased, null, foreign (and so of another size)
        with pytest.raises(P.IGXError) as e:
            mg.apply(*args)
        assert e.value.code == ARG_WRONG and "multigrid" in str(e.value), str(e.value)
        with pytest.raises(P.IGXError) as e:
            mg.solve(*args)
        assert e.value.code == ARG_WRONG and "multigrid" in str(e.value), str(e.value)
    mg.apply(r.set(rhs_of(r.n, 1)), z)          # ... and a covered call after them
    assert np.abs(z.get()).max() > 0
    mg.close()
    # 12. a state of another IGX, and 13. what a diagonal refuses: Cahn-Hilliard's, under the multigrid's name
    ch = [poisson_level(2, N, faces=()) for N in ((2, 2, 2), (4, 4, 4))]
    for g in ch:
        g.set_form("cahnhilliard", CH)
    m2 = ch[1].multigrid(ch[:1], op="ijacobian", a=250.0, coarse=dict(pc="jacobi", maxit=0))
    with pytest.raises(P.IGXError) as e:
        m2.set_state(0, U=ch[1].create_vec(), V=ch[0].create_vec())
    assert e.value.code == ARG_WRONG and "multigrid" in str(e.value)
    for l, g in enumerate(ch):
        n = g.create_vec().n
        m2.set_state(l, U=g.create_vec().set(0.5 + 0.1 * rhs_of(n, l)), V=g.create_vec().set(0.1 * rhs_of(n, l + 5)))
    with pytest.raises(P.IGXError) as e:
        m2.setup()
    print("Cahn-Hilliard's diagonal: %s" % e.value)
    assert e.value.code == SUP and "second-order" in str(e.value) and "multigrid" in str(e.value)
    m2.close()
