"""Where step_kernel's scalar argument loads sit in the machine code of the built libuavx.so (disassembly only: nothing runs,
no GPU needed).

A 65 536 x 4 step launch is one co-resident round of one-wavefront workgroups that all wait for the same things at the same
time, so a scalar load of the argument segment that is issued BEHIND the wait for the state loads is a second, fully exposed
memory round trip for the whole launch.  step_kernel therefore fetches what its straight-line path needs itself
(fetch_step_args, csrc/uavx_multi_step.hpp) behind the state loads and in front of that wait.  The compiler is free to undo
that (it sinks a load to its first use, and any remaining read of a plain kernel argument gives it a load of its own to place),
so this test reads the instructions, not the source.

Before this fetch the headline kernel had eleven s_load between its first `s_waitcnt vmcnt(0)` and its first ds_write, one of
them (s_load_dwordx8 at 0x38: tau, rtau, amax, vmax) followed at once by `s_waitcnt lgkmcnt(0)`; profiles/r12_karg_ab.md has
both listings."""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the variants that fetch (step_fetches() in csrc/uavx_multi_step.hpp): every plain one; the first is the headline kernel
FETCHING = ("step_kernel<4, false, false, 1, 1>", "step_kernel<4, true, false, 1, 1>", "step_kernel<1, false, false, 1, 1>",
            "step_kernel<2, false, false, 1, 1>", "step_kernel<5, false, false, 1, 1>", "step_kernel<8, false, false, 1, 1>",
            "step_kernel<8, false, false, 1, 2>", "step_kernel<0, false, false, 1, 1>")


def _kernel_resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr


@pytest.fixture(scope="module")
def listings():
    """{demangled kernel name: [instruction text, ...]} of the FETCHING kernels, from llvm-objdump on the gfx950 code object."""
    from gym_uav_collision_avoidance_amd import _lib
    lib = _lib.build()
    kr = _kernel_resources()
    objdump = os.path.join(kr.LLVM, "llvm-objdump")
    if not os.path.exists(objdump):
        pytest.fail(f"{objdump} not found (UAVX_LLVM_BIN names the ROCm LLVM tools)")
    symbols = {r["name"]: r["symbol"] for r in kr.kernel_table(lib) if r["name"] in FETCHING}
    assert sorted(symbols) == sorted(FETCHING), sorted(symbols)
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        for co in kr.device_objects(lib, wd):
            text = subprocess.run([objdump, "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(symbols.values()), co],
                                  capture_output=True, text=True, check=True).stdout
            for name, sym in symbols.items():
                m = re.search(r"^[0-9a-f]+ <" + re.escape(sym) + r">:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, re.M | re.S)
                if m:
                    # "\ts_load_dwordx8 s[12:19], s[6:7], 0x38    // 000000001234: " -> the instruction alone
                    out[name] = [ln.split("//")[0].strip() for ln in m.group(1).splitlines() if ln.strip() and not ln.rstrip().endswith(":")]
    assert sorted(out) == sorted(FETCHING), sorted(out)
    return out


def _stretches(ins):
    """(front, stretch): the instructions between the compatibility prologue's s_branch and the first `s_waitcnt vmcnt(0)`, and
    those between that wait and the first ds_write."""
    start = next(k for k, t in enumerate(ins) if t.startswith("s_branch")) + 1
    wait = next(k for k in range(start, len(ins)) if ins[k].startswith("s_waitcnt") and "vmcnt(0)" in ins[k])
    lds = next(k for k in range(wait, len(ins)) if ins[k].startswith("ds_write"))
    return ins[start:wait], ins[wait + 1:lds]


@pytest.mark.parametrize("name", FETCHING)
def test_scalar_loads_ride_under_the_first_state_round_trip(listings, name):
    front, stretch = _stretches(listings[name])
    loads = [t for t in stretch if t.startswith("s_load_")]
    print(name, "front:", [t for t in front if t.startswith(("s_load_", "buffer_load", "global_load", "s_waitcnt"))], "behind:", loads)
    # at most the prev_ovr pointer in its rare branch
    assert len(loads) <= 1, (name, loads)
    assert all("0xd8" in t for t in loads), (name, loads)
    for k, t in enumerate(stretch[:-1]):
        if t.startswith("s_load_"):
            assert not (stretch[k + 1].startswith("s_waitcnt") and "lgkmcnt(0)" in stretch[k + 1]), (name, stretch[k:k + 2])
    # and the fetch itself is where it was written: behind the state loads, in front of the wait for them
    vec = [k for k, t in enumerate(front) if t.startswith(("buffer_load", "global_load"))]
    fetch = [k for k, t in enumerate(front) if t.startswith("s_load_")]
    assert len(vec) >= 4 and len(fetch) >= 1 and min(fetch) > max(vec), (name, front)
    assert any(t.startswith("s_load_dwordx8") and t.endswith("0x38") for t in front), (name, front)
