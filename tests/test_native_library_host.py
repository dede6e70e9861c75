"""Host-side checks of _native.Library, the one loader class behind the six fused-kernel libraries: every library keeps the
source hash, the source list and the built file it had before the class existed; the class itself does what it says on a toy
library compiled with cc in a temporary directory; and each loader module still offers the names its callers use, now as
aliases of one Library object."""
import ctypes
import fnmatch
import glob
import importlib
import os
import re

import pytest

from gym_uav_collision_avoidance_amd import _native

PACKAGE = "gym_uav_collision_avoidance_amd"
# module -> (source_hash() with no HIPCC / ARCH / HIPFLAGS override, len(_sources())) before the loaders shared a class.  The
# entries of _clip_lib, _gae_lib and _ppo_lib moved once since, on purpose: when their block reduction, ring view and
# entry-point plumbing went into the headers of common_csrc/, their code changed and the shared headers joined their sources
# (0c0bee4070800ce1, 8ca5c55ca3b9bf76 and 48649d4f3524b361 with 3 sources each before that).  Those of _actor_lib, _prio_lib and
# _keywalk_lib moved once as well, on purpose: when the replay ring's view and the n-step walk of their three replay units went
# into common_csrc/ too (17c0e2c29cadcdb4 with 23 sources, 3e2046d3591a64b0 with 4 and f39cb6f50fa5a02e with 4 before that).
# _lib did not move.
IDENTITY = {"_lib": ("c85b3516db0d8e1b", 18), "_actor_lib": ("c6725b15f59f1983", 26), "_prio_lib": ("75c3f7d1033d0f00", 6),
            "_keywalk_lib": ("6da2580c17538898", 7), "_clip_lib": ("d2bdf6f7b75e018d", 5), "_gae_lib": ("6112f570b1b9d4de", 6),
            "_ppo_lib": ("8c24b70afaec9246", 5)}
DECLARED = [m for m in IDENTITY if m != "_lib"]
# the libraries that share the headers of common_csrc/ -> the headers each one's source includes, in the order it declares
SHARED = {"_clip_lib": ("uavx_block_reduce.hpp", "uavx_entry.hpp"), "_ppo_lib": ("uavx_block_reduce.hpp", "uavx_entry.hpp"),
          "_gae_lib": ("uavx_block_reduce.hpp", "uavx_entry.hpp", "uavx_ring_view.hpp"),
          "_norm_lib": ("uavx_block_reduce.hpp", "uavx_entry.hpp", "uavx_ring_view.hpp"),
          "_actor_lib": ("uavx_entry.hpp", "uavx_replay_ring.hpp", "uavx_replay_walk.hpp"),
          "_prio_lib": ("uavx_entry.hpp", "uavx_replay_ring.hpp"),
          "_keywalk_lib": ("uavx_entry.hpp", "uavx_replay_ring.hpp", "uavx_replay_walk.hpp")}
# the three replay units; the actor library has eleven .hip files, and uavx_replay.hip is the one that shares
REPLAY = {"_actor_lib": "uavx_replay.hip", "_prio_lib": "uavx_prio.hip", "_keywalk_lib": "uavx_keywalk.hip"}


def _module(name):
    return importlib.import_module(f"{PACKAGE}.{name}")


def test_every_library_keeps_its_identity(monkeypatch):
    for var in ("HIPCC", "ARCH", "HIPFLAGS"):                  # they enter the hash
        monkeypatch.delenv(var, raising=False)
    for name, (srchash, n) in IDENTITY.items():
        m = _module(name)
        assert m.source_hash() == srchash, name
        assert len(m._sources()) == n and all(os.path.isfile(f) for f in m._sources()), name
        if os.path.exists(m.LIB_PATH):
            assert m._up_to_date(), f"{m.LIB_PATH} would be rebuilt on its first load"


# ---- the class, on a toy library ------------------------------------------------------------------------------------------

TOY_C = """/* a toy unit */
#include "toy.h"
#ifndef TOY_SRC_HASH
#define TOY_SRC_HASH ""
#endif
__attribute__((used)) static const char kBuildInfo[] = "TOY_SRC_HASH=" TOY_SRC_HASH;
int toy_version(void) { return TOY_VERSION; }
int toy_add(int a, int b) { return a + b; }
"""
TOY_H = "#define TOY_VERSION 1\nint toy_version(void);\nint toy_add(int a, int b);\n"
TOY_MAKEFILE = """OUT ?= libtoy.so
SRCHASH ?=
$(OUT): toy.hip toy.h
\tcc -O1 -x c -fPIC -shared -DTOY_SRC_HASH='"$(SRCHASH)"' -o $@ toy.hip
"""
TOY_FUNCTIONS = {"toy_version": (ctypes.c_int, []), "toy_add": (ctypes.c_int, [ctypes.c_int, ctypes.c_int])}


def _toy(tmp_path, abi=1):
    unit = _native.Unit("toy", str(tmp_path / "toy.h"), "toy_version", abi, TOY_FUNCTIONS)
    return _native.Library(str(tmp_path), "libtoy.so", b"TOY_SRC_HASH", [unit])


def test_library_class_on_a_toy_library(tmp_path, monkeypatch):
    src = tmp_path / "toy.hip"                                 # C, under the one suffix sources() looks for
    src.write_text(TOY_C)
    (tmp_path / "toy.h").write_text(TOY_H)
    (tmp_path / "Makefile").write_text(TOY_MAKEFILE)
    before = sorted(os.listdir(tmp_path))
    lib = _toy(tmp_path)
    assert sorted(os.listdir(tmp_path)) == before              # constructing it touches nothing
    assert lib.csrc == str(tmp_path) and lib.path == str(tmp_path / "libtoy.so")
    assert lib.sources() == [str(src), str(tmp_path / "toy.h")]

    makes = []
    run = _native.subprocess.run
    monkeypatch.setattr(_native.subprocess, "run", lambda cmd, **kw: (makes.append(cmd), run(cmd, **kw))[1])
    assert not lib.loaded()
    L = lib.load()                                             # builds: there is no library yet
    assert lib.loaded() and len(makes) == 1 and os.path.exists(lib.path) and lib.up_to_date()
    assert lib.load() is L and len(makes) == 1                 # the cached handle; no second make
    assert L.toy_add(2, 3) == 5
    for name, (restype, argtypes) in TOY_FUNCTIONS.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes

    srchash = lib.source_hash()
    src.write_text(TOY_C.replace("a toy unit", "the same unit,   reworded"))
    assert lib.source_hash() == srchash and lib.up_to_date()   # a comment is not code
    src.write_text(TOY_C.replace("a + b", "b + a"))
    assert lib.source_hash() != srchash and not lib.up_to_date()
    assert lib.build() == lib.path and lib.up_to_date() and len(makes) == 2
    assert lib.build() == lib.path and len(makes) == 2         # up to date: nothing to do unless forced
    lib.build(force=True)
    assert len(makes) == 3 and lib.up_to_date()
    srchash = lib.source_hash()
    (tmp_path / "Makefile").write_text(TOY_MAKEFILE.replace("-O1", "-O2"))
    assert lib.source_hash() != srchash and not lib.up_to_date()          # the recipe is part of the identity
    (tmp_path / "Makefile").write_text(TOY_MAKEFILE.replace("OUT ?=", "# where to\nOUT ?="))
    assert lib.source_hash() == srchash and lib.up_to_date()              # its comments are not

    newer = _toy(tmp_path, abi=2)
    with pytest.raises(RuntimeError) as e:
        newer.load()
    assert str(e.value) == (f"{lib.path} speaks toy ABI version 1, this package binds 2: rebuild it "
                            f"(`make -B -C {tmp_path}`)")
    assert not newer.loaded()

    assert lib.check(0, "toy_call") is None
    with pytest.raises(RuntimeError) as e:
        lib.check(-1, "toy_call")
    assert str(e.value) == "uavx: toy_call failed: invalid argument (-1)"
    for rc, word in ((-2, "HIP error"), (-3, "unsupported"), (-4, "unknown error"), (7, "unknown error")):
        with pytest.raises(RuntimeError, match=re.escape(f"uavx: toy_call failed: {word} ({rc})")):
            lib.check(rc, "toy_call")

    src.write_text(TOY_C.replace("return a + b;", "return a +;"))
    with pytest.raises(RuntimeError, match=r"uavx: building .*libtoy\.so failed \(make exit [1-9]\d*\)"):
        lib.build()
    assert glob.glob(str(tmp_path / "*.tmp*")) == []
    assert os.path.exists(lib.path) and not lib.up_to_date()   # the last good build stays in place, and stays stale


TOY_SHARED = "/* what two toys would share */\nstatic int toy_twice(int a) { return a + a; }\n"


def test_library_class_with_a_shared_source(tmp_path):
    shared = tmp_path / "elsewhere" / "toy_shared.hpp"         # a path passes through, as csrc does
    shared.parent.mkdir()
    shared.write_text(TOY_SHARED)
    src = tmp_path / "toy.hip"
    src.write_text('#include "elsewhere/toy_shared.hpp"\n' + TOY_C.replace("a + b", "toy_twice(a) + b - a"))
    (tmp_path / "toy.h").write_text(TOY_H)
    (tmp_path / "Makefile").write_text(TOY_MAKEFILE)
    plain = _toy(tmp_path)
    lib = _native.Library(str(tmp_path), "libtoy.so", b"TOY_SRC_HASH", plain.units, shared=(str(shared),))
    assert plain.shared == [] and plain.sources() == [str(src), str(tmp_path / "toy.h")]      # the default: as before
    assert lib.sources() == plain.sources() + [str(shared)]                                    # last, behind the unit headers
    assert lib.source_hash() != plain.source_hash()
    assert lib.load().toy_add(2, 3) == 5 and lib.up_to_date()
    srchash = lib.source_hash()
    shared.write_text(TOY_SHARED.replace("what two toys would share", "the same,   reworded"))
    assert lib.source_hash() == srchash and lib.up_to_date()   # a comment is not code, there neither
    shared.write_text(TOY_SHARED.replace("a + a", "2 * a"))
    assert lib.source_hash() != srchash and not lib.up_to_date()
    assert plain.source_hash() != srchash                      # the library without `shared` never saw the file
    # a name is a file of the package's common_csrc/
    named = _native.Library(str(tmp_path), "libtoy.so", b"TOY_SRC_HASH", plain.units, shared=("uavx_entry.hpp",))
    assert named.sources()[-1] == os.path.join(_native.PACKAGE, "common_csrc", "uavx_entry.hpp")


# ---- one copy of what the clip, gae, ppo and norm libraries share, and of what the three replay units share -------------------

@pytest.mark.parametrize("name", sorted(SHARED))
def test_shared_headers_are_sources_and_the_only_copy(name):
    m = _module(name)
    common = os.path.join(_native.PACKAGE, "common_csrc")
    assert sorted(os.listdir(common)) == sorted(set(sum(SHARED.values(), ())))                  # headers only: no Makefile
    assert not any(w in f for f in os.listdir(common) for w in ("norm", "gae", "ppo", "clip"))
    hip, = glob.glob(os.path.join(m.CSRC, REPLAY.get(name, "*.hip")))
    text = open(hip).read()
    included = re.findall(r'^#include "\.\./common_csrc/([^"]+)"$', text, re.M)
    assert tuple(included) == SHARED[name]                     # what it includes is what it declares ...
    assert m._sources()[-len(included):] == [os.path.join(common, h) for h in included]         # ... last in its sources
    for h in included:                                         # no shared header includes a further one
        assert "common_csrc" not in open(os.path.join(common, h)).read().split("#pragma once", 1)[1], h
    hdr = re.search(r"^HDR := (.*)$", open(os.path.join(m.CSRC, "Makefile")).read(), re.M).group(1).split()
    assert hdr[-len(included):] == [f"../common_csrc/{h}" for h in included]
    for word in ("__shfl_down", "hipGetLastError", "hipLaunchKernelGGL", "kBuildInfo"):
        assert word not in text, word
    # no definition of these (a return type in front of the name), only calls
    assert not re.search(r"\b(bool|T|double|uint32_t|Column)\s+(aligned|unit|block_sum|total|flags|column)\s*\(", text)
    if "uavx_ring_view.hpp" in included:                       # (uavx_clip.hip has a plan of its own: a group's block numbers)
        assert "bool plan(" not in text
    if name in REPLAY:
        # no window function, no field-by-field fill of the view from the public ring, no copy of the walk's resolution loop
        assert not re.search(r"\b\w+\s+(window|span_of|steps_of|replay_view|nstep_walk)\s*\([^;{]*\)\s*\{", text)
        assert "count_dev ?" not in text and not re.search(r"= *\(int32_t\) *ring->", text) and "ring->obs" not in text
        assert "run ? Rt : R" not in text and "sched_barrier" not in text
        walk = open(os.path.join(common, "uavx_replay_walk.hpp")).read()
        assert walk.count("run ? Rt : R") == 1 and ("nstep_walk<" in text) == ("uavx_replay_walk.hpp" in included)


# ---- the six modules' surface ---------------------------------------------------------------------------------------------

NAMES = ("LIB", "CSRC", "LIB_PATH", "HEADER", "ABI_VERSION", "SYMBOLS", "load", "loaded", "build", "source_hash", "_sources",
         "_up_to_date", "check")
ACTOR_NAMES = ("UNITS", "Unit", "check_critic", "check_wgrad", "OK", "ERR_INVALID_ARG", "ERR_HIP", "ERR_UNSUPPORTED",
               "ERR_NOT_PACKED") + tuple(f"{p}_{s}" for p in ("CRITIC", "GRAD", "OPTIM", "REPLAY", "ACTION_GRAD", "POLICY_GRAD",
                                                                "LEARNER", "EXPLORE", "NSTEP", "WGRAD")
                                         for s in ("HEADER", "SYMBOLS", "ABI_VERSION"))


@pytest.mark.parametrize("name", DECLARED)
def test_module_surface(name):
    m = _module(name)
    missing = [n for n in NAMES + (ACTOR_NAMES if name == "_actor_lib" else ("FUNCTIONS",)) if not hasattr(m, n)]
    assert not missing, missing
    assert isinstance(m.LIB, _native.Library) and not hasattr(m, "_lib_handle")
    assert (m.CSRC, m.LIB_PATH) == (m.LIB.csrc, m.LIB.path)
    assert m.CSRC == os.path.join(os.path.dirname(os.path.abspath(m.__file__)), name[1:-4] + "_csrc")
    assert os.path.dirname(m.LIB_PATH) == m.CSRC and fnmatch.fnmatchcase(os.path.basename(m.LIB_PATH), "libuavx_*.so")
    assert m.SYMBOLS[0].endswith("_version") and m.HEADER == m.LIB.units[0].header and os.path.isfile(m.HEADER)
    assert m.ABI_VERSION == m.LIB.units[0].abi
    if name == "_actor_lib":
        assert m.LIB.units == m.UNITS and len(m.UNITS) == 11 and m.Unit is _native.Unit
        assert m.SYMBOLS == tuple(m.UNITS[0].functions) and m.WGRAD_SYMBOLS == tuple(m.UNITS[10].functions)
    else:
        assert len(m.LIB.units) == 1 and m.LIB.units[0].functions is m.FUNCTIONS and m.SYMBOLS == tuple(m.FUNCTIONS)
    for alias, method in (("load", "load"), ("loaded", "loaded"), ("build", "build"), ("source_hash", "source_hash"),
                          ("_sources", "sources"), ("_up_to_date", "up_to_date")):
        assert getattr(m, alias) == getattr(m.LIB, method), alias
    L = m.load()
    assert m.loaded() and m.load() is L
    for u in m.LIB.units:
        assert u.version == next(iter(u.functions)) and getattr(L, u.version)() == u.abi
        for symbol, (restype, argtypes) in u.functions.items():
            f = getattr(L, symbol)
            assert f.restype is restype and list(f.argtypes) == list(argtypes), symbol
    with pytest.raises(RuntimeError, match=re.escape("uavx: that failed: ")):
        m.check(-1, "that")
    assert m.check(0, "that") is None
