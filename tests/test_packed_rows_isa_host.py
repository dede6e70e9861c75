"""Which vector stores the 4-UAV one-step kernel leaves with, read from the built libuavx.so (disassembly only: nothing runs, no
GPU needed).

A kernel boundary writes back what the launch left dirty in the L2s, so step_kernel<4, ...> stores its outputs write-through
(sc1), and narrow write-through stores are slow, so positions and rewards leave as quad-packed 16-byte rows
(csrc/uavx_multi_step.hpp, UAVX_PACKWT; profiles/r13_packed_rows_ab.md).  The compiler is free to merge, split or move stores
and the A/B switch is one -D away, so this test reads the instructions: on the straight-line path (everything in front of
s_endpgm; what the compiler lays out behind it is reached by a branch only)

  * no buffer_store_dwordx2 at all (the 8-byte position store is gone);
  * no plain buffer_store_dword outside an EXEC-masked rare branch (the flags word; the reward fallback for a caller's
    unaligned array is laid out behind s_endpgm or under a mask of its own);
  * every buffer_store_dwordx4 carries sc1, and there are six of them: velocity, position row, reward row, three observation
    rounds."""
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
def test_outputs_leave_as_16_byte_write_through_rows(listings, name):
    path = _straight_line(listings[name])
    stores = [(k, t) for k, t in enumerate(path) if t.startswith("buffer_store")]
    print(name, [t for _, t in stores])
    assert not [t for _, t in stores if t.startswith("buffer_store_dwordx2")], (name, stores)
    plain = [(k, t) for k, t in stores if t.split()[0] == "buffer_store_dword" and "sc1" not in t.split()]
    assert all(_masked(path, k) for k, _ in plain), (name, plain)
    assert len(plain) <= 2, (name, plain)   # the flags word, and the reward fallback if it was laid out in line
    rows = [t for _, t in stores if t.startswith("buffer_store_dwordx4")]
    assert all("sc1" in t.split() for t in rows), (name, rows)
    assert len(rows) == 6, (name, rows)
