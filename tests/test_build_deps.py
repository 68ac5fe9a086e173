"""What petiga_amd/build.py reads from the compiler's depfiles, without compiling anything: a depfile in Makefile syntax with continuation
lines gives the paths it lists, and a product is stale with no depfile, with a dependency newer than it and with a dependency that no
longer exists, and fresh otherwise.  The files are made here, their modification times set with os.utime."""
import os

from petiga_amd import build as B

DEPFILE = ("{obj}: engine.hip \\\n"
           "  igx.hpp ../../include/petiga_amd.h \\\n"
           "  {far} \\\n"
           "  with\\ space.hpp\n")


def _tree(tmp_path):
    base = tmp_path / "petiga_amd" / "csrc"
    base.mkdir(parents=True)
    (tmp_path / "include").mkdir()
    far = tmp_path / "far" / "hip_runtime.h"                       # an absolute path, as a system header comes
    far.parent.mkdir()
    deps = [base / "engine.hip", base / "igx.hpp", tmp_path / "include" / "petiga_amd.h", far, base / "with space.hpp"]
    obj = tmp_path / "unit.o"
    for k, f in enumerate(deps):
        f.write_text("")
        os.utime(f, (1000 + k, 1000 + k))
    obj.write_text("")
    os.utime(obj, (2000, 2000))
    dep = tmp_path / "unit.o.d"
    dep.write_text(DEPFILE.format(obj=obj, far=far))
    return base, obj, dep, deps


def test_a_depfile_with_continuation_lines_gives_the_listed_paths(tmp_path):
    base, obj, dep, deps = _tree(tmp_path)
    got = B.read_depfile(str(dep))
    assert got == ["engine.hip", "igx.hpp", "../../include/petiga_amd.h", str(deps[3]), "with space.hpp"]
    assert [os.path.realpath(os.path.join(str(base), d)) for d in got] == [os.path.realpath(str(d)) for d in deps]


def test_stale_and_fresh(tmp_path):
    base, obj, dep, deps = _tree(tmp_path)
    stale = lambda: B.deps_newer(str(dep), str(obj), str(base))
    assert not stale()                                              # every dependency is older than the object
    for d in deps:                                                  # ... each of them newer, the relative and the absolute ones alike
        old = os.stat(d).st_mtime
        os.utime(d, (3000, 3000))
        assert stale(), d
        os.utime(d, (old, old))
        assert not stale()
    os.utime(deps[1], (2000, 2000))                                 # as old as the object: not newer
    assert not stale()
    for d in (deps[1], deps[3]):                                    # a dependency that no longer exists
        os.rename(d, str(d) + ".gone")
        assert stale(), d
        os.rename(str(d) + ".gone", d)
        assert not stale()
    os.remove(dep)                                                  # no depfile
    assert stale()
    dep.write_text(DEPFILE.format(obj=obj, far=deps[3]))
    assert not stale()
    os.remove(obj)                                                  # no product
    assert stale()
