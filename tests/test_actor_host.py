"""Host-side checks of the fused actor library (libuavx_actor.so, include/uavx_actor.h): builds for gfx950 without a GPU,
exports what its header declares, rejects bad arguments before touching a device, and its kernels neither spill nor use
scratch."""
import ctypes
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _alib():
    from gym_uav_collision_avoidance_amd import _actor_lib
    _actor_lib.build()
    return _actor_lib


def test_actor_library_cross_compiles():
    a = _alib()
    assert os.path.exists(a.LIB_PATH)
    assert a._up_to_date()
    blob = open(a.LIB_PATH, "rb").read()
    assert f"UAVX_ACTOR_SRC_HASH={a.source_hash()}".encode() in blob


def test_actor_library_exports_every_declared_symbol():
    a = _alib()
    hdr = open(os.path.join(ROOT, "include", "uavx_actor.h")).read()
    declared = set(re.findall(r"\b(uavx_actor_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(a.SYMBOLS), declared ^ set(a.SYMBOLS)
    lib = a.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_actor_version() == 1
    assert lib.uavx_actor_strerror(a.ERR_INVALID_ARG) == b"invalid argument"
    assert lib.uavx_actor_strerror(a.ERR_UNSUPPORTED) == b"no kernel compiled for these dimensions"


def test_actor_env_library_source_untouched():
    """The actor library lives apart from csrc/: the environment library's source hash does not see it."""
    from gym_uav_collision_avoidance_amd import _lib
    import glob
    assert not glob.glob(os.path.join(ROOT, "gym_uav_collision_avoidance_amd", "csrc", "*actor*"))
    assert "uavx_actor" not in open(os.path.join(ROOT, "include", "uavx.h")).read()
    assert len(_lib.source_hash()) == 16


def test_actor_bad_arguments_rejected_before_any_device_call():
    a = _alib()
    lib = a.load()
    h = ctypes.c_void_p()
    create = lambda *args: lib.uavx_actor_create(*args, ctypes.byref(h))
    assert create(3, a.F32, 10, 256, 256, 2) == a.ERR_INVALID_ARG          # unknown kind
    assert create(-1, a.F32, 10, 256, 256, 2) == a.ERR_INVALID_ARG
    assert create(a.SAC, 2, 10, 256, 256, 2) == a.ERR_INVALID_ARG          # unknown precision
    assert create(a.TD3, a.F32, 10, 0, 256, 2) == a.ERR_INVALID_ARG        # empty layer
    assert create(a.TD3, a.F32, 10, 256, -4, 2) == a.ERR_INVALID_ARG
    assert create(a.TD3, a.F32, 11, 256, 256, 2) == a.ERR_UNSUPPORTED      # not the env's observation
    assert create(a.TD3, a.F32, 10, 256, 256, 3) == a.ERR_UNSUPPORTED
    assert create(a.TD3, a.F32, 10, 128, 256, 2) == a.ERR_UNSUPPORTED      # no register tile compiled for 128 units
    assert create(a.DDPG, a.BF16, 10, 256, 300, 2) == a.ERR_UNSUPPORTED
    assert h.value is None
    assert lib.uavx_actor_create(a.TD3, a.F32, 10, 256, 256, 2, None) == a.ERR_INVALID_ARG
    buf = ctypes.c_void_p(16)     # never dereferenced: every call below fails its argument check first
    assert lib.uavx_actor_forward(None, buf, 4, 10, None, 0.0, a.DETERMINISTIC, buf, 2, None) == a.ERR_INVALID_ARG
    assert lib.uavx_actor_pack(None, buf, buf, buf, buf, buf, buf, None, None, None) == a.ERR_INVALID_ARG
    assert lib.uavx_actor_destroy(None) == a.ERR_INVALID_ARG


def test_actor_kernels_no_spills_no_scratch():
    a = _alib()
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernel_table(a.LIB_PATH)
    names = sorted(r["name"] for r in rows)
    assert sum(n.startswith("uavx_actor_k::actor_fwd<") for n in names) == 4, names
    assert any(n.startswith("uavx_actor_k::pack_kernel") for n in names), names
    for r in rows:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0, r
    # the waves per SIMD each forward tile was compiled for (its last template argument) are what its registers allow
    for r in rows:
        m = re.match(r"uavx_actor_k::actor_fwd<\d+, \w+, \d+, \d+, (\d+)>", r["name"])
        if m:
            assert r["waves_per_simd"] >= int(m.group(1)), r



def test_actor_create_accepts_exactly_the_documented_hidden_sizes():
    """hidden1 241..256 (SAC / TD3) or 385..400 (DDPG) and hidden2 1..4096, for both precisions (tests/fused_ref.py)."""
    from fused_ref import check_hidden_range
    a = _alib()
    lib = a.load()
    check_hidden_range(lib.uavx_actor_create, lib.uavx_actor_destroy, a.OK, a.ERR_INVALID_ARG, a.ERR_UNSUPPORTED, a.ERR_HIP)
