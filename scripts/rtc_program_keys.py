"""The programs the run-time path (petiga_amd/csrc/rtc.hpp) hands to hiprtc, named by what the disk cache calls them.  With IGX_RTC_CACHE_DIR set
to a fresh directory, every set_form_source / check_form_source call of the compile-only tests (tests/test_rtc_forms.py,
test_rtc_boundary_scalar.py, test_rtc_band_pt.py, test_matrix_free_high_degree_abi.py: the default check with and without a matrix and
kinds 2 to 9) is made once, and after each call the cache files that appeared are printed: name, size, SHA-256.  A file's name is the hash of
the whole program text, the name expressions, the options and the hiprtc version, so two builds of the library that print the same names
compile the same programs: run it on both (IGX_LIB=<the other build>) and compare (profiles/rtc_instances.txt).  No GPU needed.

    python scripts/rtc_program_keys.py [--out file]"""
import argparse
import hashlib
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cache = tempfile.mkdtemp(prefix="igx_rtc_keys_")
    os.environ["IGX_RTC_CACHE_DIR"] = cache
    import petiga_amd as P
    from common import make_pair, warped_geometry
    import test_rtc_forms as TF
    import test_rtc_boundary_scalar as TB
    import test_rtc_band_pt as TP
    from test_gpu_matrix_action import USER_DIFFUSION
    from test_matrix_diagonal_abi import USER_BIHARMONIC

    lines = ["library: %s" % os.environ.get("IGX_LIB", "this tree's")]
    seen = set()

    def call(label, fn):
        try:
            fn()
            status = ""
        except P.IGXError as e:
            status = "  (refused: code %d)" % e.code
        new = sorted(set(os.listdir(cache)) - seen)
        seen.update(new)
        lines.append("%s%s" % (label, status))
        for f in new:
            data = open(os.path.join(cache, f), "rb").read()
            lines.append("    %s %8d %s" % (f, len(data), hashlib.sha256(data).hexdigest()))
        print("\n".join(lines[-1 - len(new):]), flush=True)

    def space(dim, dof, p, n, geo=None, nqp=None):
        """a space set up as the tests set it up, on the identity or a warped geometry ('poly' / 'nurbs')"""
        orc, g = make_pair(dim, dof, p, n, nqp=nqp)
        if geo:
            g.set_geometry(*warped_geometry(orc, dim, seed=1, rational=(geo == "nurbs"), amp=0.05))
        return g

    def checks(label, g, src, name, params, kinds):
        call("%s set_form_source %s" % (label, name), lambda: g.set_form_source(src, name, params))
        for with_matrix, kind in kinds:
            call("%s check(%s, %d) %s" % (label, with_matrix, kind, name), lambda: g.check_form_source(with_matrix, kind))

    both = lambda kind: [(True, kind), (False, kind)]
    # tests/test_rtc_forms.py
    for dim in (1, 2, 3):
        checks("forms point-form dim %d" % dim, P.IGX(dim, 1), TF.ADVECTION_DIFFUSION, "AdvDiff<%d>" % dim, (1.0, 0.5, 0.25), [])
    for dim, p, dof, src, name, gram in ((2, 2, 1, TF.ADVECTION_DIFFUSION, "AdvDiff<2>", 0), (3, 3, 1, TF.ADVECTION_DIFFUSION, "AdvDiff<3>", 0), (3, 5, 1, TF.ADVECTION_DIFFUSION, "AdvDiff<3>", 0),
                                         (3, 2, 3, TF.USER_ELASTICITY, "UserElasticity<0>", 0), (3, 3, 3, TF.USER_ELASTICITY, "UserElasticity<1>", 1), (3, 2, 1, TF.ADVECTION_DIFFUSION, "AdvDiff<3>", 0)):
        checks("forms feature dim %d p %d" % (dim, p), space(dim, dof, p, 4), src, name, (1.0, 0.5, 0.25), both(gram))
    for p, geo in ((3, None), (2, None), (3, "nurbs")):
        g = space(3, 1, p, 8, geo)
        checks("forms pencil p %d %s" % (p, geo), g, TF.USER_POISSON, "UserPoisson", (1.0,), [(True, 2)])
        checks("forms pencil p %d %s" % (p, geo), g, TF.USER_POISSON, "UserDiffusion", (0.7,), [(True, 2)])
    # the three families of tests/test_rtc_forms.py's store test on one IGX: the third call finds what the first built
    checks("forms store p 2", space(3, 1, 2, 4), TF.USER_POISSON, "UserPoisson", (1.0,), [(True, 2), (False, 3), (True, 2)])
    # tests/test_rtc_boundary_scalar.py
    for dim in (2, 3):
        checks("boundary nitsche dim %d" % dim, space(dim, 1, 2, 4), TB.NITSCHE, "UserNitsche<%d>" % dim, (2.0,), both(0))
    checks("boundary vec_sumfact", space(3, 1, 2, 4), TB.BRATU3, "UserBratu3", (3.5,), [(False, 3)])
    for p in (2, 3):
        g = space(3, 1, p, 8)
        checks("boundary state p %d" % p, g, TB.BRATU3_WALK, "UserBratu3Walk", (3.5,), [(True, 4)])
        checks("boundary state p %d, no hooks" % p, g, TB.BRATU3, "UserBratu3", (3.5,), [(True, 4)])
    for geo in ("poly", "nurbs"):
        checks("boundary state p 2 %s" % geo, space(3, 1, 2, [6, 5, 4], geo), TB.BRATU3_WALK, "UserBratu3Walk", (3.5,), [(True, 4)])
    checks("boundary block_pencil", space(3, 3, 3, 8), TB.ELASTICITY_BANDS, "UserElasticityBands", (1.5, 0.8), [(True, 5)])
    # tests/test_rtc_band_pt.py
    full, name = TP.builtin_text_as_source()
    host_src, host_name = TP._host_only_guard_source()
    for src, nm, deg in ((TP.PLAIN_VMS, "UserVMS", 3), (full, name, 3), (full, name, 2), (host_src, host_name, 3)):
        checks("band_pt p %d" % deg, space(3, 4, deg, 8), src, nm, (TP.NU, TP.FX, 0.0, 0.0, TP.DT), [(True, 6)])
    # tests/test_matrix_free_high_degree_abi.py (and kind 9 on the same spaces)
    for label, p, nqp, geo in (("p4-identity", 4, None, None), ("p6-rational", 6, None, "nurbs"), ("p3-nqp5", 3, 5, None), ("p3-nqp9", 3, 9, None)):
        checks("high degree %s" % label, space(3, 1, p, [2, 2, 2], geo, nqp), USER_DIFFUSION, "UserDiffusion", (0.7,), [(True, 7), (True, 8), (True, 9)])
    checks("high degree biharmonic p 4", space(3, 1, 4, 2), USER_BIHARMONIC, "UserBiharmonic", (), [(True, 7), (True, 8)])
    lines.append("%d files" % len(seen))
    print(lines[-1])
    shutil.rmtree(cache, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
