"""The library's source stamp covers every file the one hipcc command reads: build.DEPS is every *.hip / *.hpp under csrc/
and every *.h under include/, and each #include "..." reachable from imcoal_fwd.hip names one of them - a header outside
those folders would be compiled in without being hashed, and a stale library would pass the stamp check."""
import os
import re

from imcoalhmm_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def test_deps_are_the_source_folders():
    csrc = os.path.join(build.PKG, "csrc")
    include = os.path.join(os.path.dirname(build.PKG), "include")
    want = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".hpp"))]
    want += [os.path.join(include, f) for f in os.listdir(include) if f.endswith(".h")]
    assert build.DEPS == sorted(want) and build.SRC in build.DEPS and build.HDR in build.DEPS
    assert len({os.path.basename(f) for f in build.DEPS}) == len(build.DEPS)     # (the digest names files by their base name)


def test_every_reachable_include_is_a_dep():
    deps = {os.path.realpath(f) for f in build.DEPS}
    seen, todo = set(), [os.path.realpath(build.SRC)]
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        assert path in deps, "%s is included but not in build.DEPS" % path
        for name in INCLUDE.findall(open(path).read()):
            target = os.path.realpath(os.path.join(os.path.dirname(path), name))
            assert os.path.exists(target), "%s includes %s, which does not exist" % (path, name)
            todo.append(target)
    assert len(seen) > 30 and any(p.endswith("options_host.hpp") for p in seen) and any(p.endswith("kernels_zip4.hpp") for p in seen)


def test_engine_headers_are_host_parts_of_the_one_translation_unit():
    """Every engine_*.hpp is included from imcoal_fwd.hip exactly once and from nowhere else, and holds neither a kernel
    (those live in kernels_*.hpp) nor a piece of the C ABI (that is imcoal_fwd.hip's)."""
    csrc = os.path.join(build.PKG, "csrc")
    engine = sorted(f for f in os.listdir(csrc) if f.startswith("engine_") and f.endswith(".hpp"))
    assert engine
    includes = {os.path.basename(f): INCLUDE.findall(open(f).read()) for f in build.DEPS}
    for name in engine:
        assert includes["imcoal_fwd.hip"].count(name) == 1, name
        others = [f for f, inc in includes.items() if f != "imcoal_fwd.hip" and any(os.path.basename(i) == name for i in inc)]
        assert not others, (name, others)
        text = open(os.path.join(csrc, name)).read()
        assert 'extern "C"' not in text and "__global__" not in text, name
