"""What the tail of the 4-UAV one-step kernel runs on its straight-line path, read from the built libuavx.so (disassembly only:
nothing runs, no GPU needed).

csrc/uavx_multi_step.hpp (UAVX_TAILCOLD, UAVX_DONEROW; profiles/r14_tail_ab.md): the rare events (flags word, arrival,
collision, non-finite reward) sit behind ONE scalar branch, and the done bytes leave as one write-through dword per env.  The
compiler decides where blocks are laid out, and each part is one -D away, so this test reads the instructions.
Straight-line path: everything in front of s_endpgm (what is laid out behind it is reached by a branch only).

  * the only atomic there is the wavefront's step counter (one no-return global_atomic_add; replacing it by a load and a
    write-through store measured slower and was dropped); the rare counters' three atomics are in the cold block;
  * no buffer_store_byte there outside an EXEC-masked region (the per-lane done store is gone; the fallback for a caller's
    unaligned array is reached by a branch), and one write-through buffer_store_dword under the leaders' mask (the done row)."""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("step_kernel<4, false, false, 1, 1>", "step_kernel<4, true, false, 1, 1>")   # float32 / float64 commands


def _kernel_resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr


@pytest.fixture(scope="module")
def listings():
    """{demangled kernel name: [instruction text, ...]} of the HEADLINE kernels, from llvm-objdump on the gfx950 code object."""
    from gym_uav_collision_avoidance_amd import _lib
    lib = _lib.build()
    kr = _kernel_resources()
    objdump = os.path.join(kr.LLVM, "llvm-objdump")
    if not os.path.exists(objdump):
        pytest.fail(f"{objdump} not found (UAVX_LLVM_BIN names the ROCm LLVM tools)")
    symbols = {r["name"]: r["symbol"] for r in kr.kernel_table(lib) if r["name"] in HEADLINE}
    assert sorted(symbols) == sorted(HEADLINE), sorted(symbols)
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        for co in kr.device_objects(lib, wd):
            text = subprocess.run([objdump, "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(symbols.values()), co],
                                  capture_output=True, text=True, check=True).stdout
            for name, sym in symbols.items():
                m = re.search(r"^[0-9a-f]+ <" + re.escape(sym) + r">:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, re.M | re.S)
                if m:
                    out[name] = [ln.split("//")[0].strip() for ln in m.group(1).splitlines() if ln.strip() and not ln.rstrip().endswith(":")]
    assert sorted(out) == sorted(HEADLINE), sorted(out)
    return out


def _straight_line(ins):
    return ins[:next(k for k, t in enumerate(ins) if t.startswith("s_endpgm"))]


def _masked(path, k):
    """Is instruction k inside an EXEC-masked region: an s_and_saveexec in front of it with no restore of EXEC in between?"""
    for t in reversed(path[:k]):
        if t.startswith("s_and_saveexec"):
            return True
        if t.startswith(("s_or_b64 exec", "s_mov_b64 exec")):
            return False
    return False


@pytest.mark.parametrize("name", HEADLINE)
def test_rare_counters_are_behind_the_branch(listings, name):
    path = _straight_line(listings[name])
    atomics = [t for t in path if t.startswith(("global_atomic", "buffer_atomic", "flat_atomic"))]
    cold = [t for t in listings[name][len(path):] if t.startswith("global_atomic_add")]
    print(name, "straight-line:", atomics, "behind s_endpgm:", cold)
    assert len(atomics) == 1 and atomics[0].startswith("global_atomic_add "), (name, atomics)   # the step counter (no return)
    assert len(cold) >= 3, (name, cold)   # reach, coll and the non-finite tripwire


@pytest.mark.parametrize("name", HEADLINE)
def test_no_per_lane_done_byte_store_on_the_straight_line_path(listings, name):
    path = _straight_line(listings[name])
    bytes_ = [(k, t) for k, t in enumerate(path) if t.startswith("buffer_store_byte")]
    assert all(_masked(path, k) for k, _ in bytes_), (name, bytes_)
    wt = [(k, t) for k, t in enumerate(path) if t.split()[0] == "buffer_store_dword" and "sc1" in t.split()]
    assert len(wt) == 1 and all(_masked(path, k) for k, _ in wt), (name, wt)   # the done row, under the leaders' mask
