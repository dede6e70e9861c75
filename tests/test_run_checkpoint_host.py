"""DeviceReplay.state_dict / load_state_dict and checkpoint.save_run / load_run on the CPU: the ring round
trip in place, the file format, the refusals and the atomic write.  The GPU side is tests/test_gpu_run_checkpoint.py."""
import os
import types

import pytest
import torch

from gym_uav_collision_avoidance_amd import checkpoint
from gym_uav_collision_avoidance_amd.checkpoint import load_run, save_run
from gym_uav_collision_avoidance_amd.replay import DeviceReplay

E, N, T = 6, 2, 5
RING = ("obs", "act", "rew", "done", "skip", "trunc", "ended")
FACTS = ("L", "num_envs", "num_agents", "num_learners", "packed")


def _ring(horizon=T, seed=None, **kw):
    """A DeviceReplay over a stub env (the constructor reads num_envs, num_agents and device); seed: random bits in every
    ring tensor and a count past one wrap."""
    mem = DeviceReplay(types.SimpleNamespace(num_envs=E, num_agents=N, device="cpu"), horizon, **kw)
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        for name in RING:
            t = getattr(mem, name)
            t.view(torch.uint8).copy_(torch.randint(0, 256, t.view(torch.uint8).shape, generator=g, dtype=torch.uint8))
        mem.count = 2 * mem.L + 3
    return mem


def _bits(mem):
    return {name: getattr(mem, name).view(torch.uint8).clone() for name in RING}


def _same_bits(a, b):
    return all(torch.equal(a[name], b[name]) for name in RING)


def test_ring_round_trip_in_place():
    src, dst = _ring(seed=1), _ring()
    sd = src.state_dict()
    assert set(sd) == set(RING) | set(FACTS) | {"count"}
    assert all(sd[name].device.type == "cpu" and sd[name].data_ptr() != getattr(src, name).data_ptr() for name in RING)
    assert (sd["L"], sd["num_envs"], sd["num_agents"], sd["num_learners"], sd["packed"]) == (T + 1, E, N, N, False)
    ptrs = {name: getattr(dst, name).data_ptr() for name in RING}
    assert dst.load_state_dict(sd) is dst
    assert _same_bits(_bits(dst), _bits(src)) and dst.count == src.count == 2 * (T + 1) + 3
    assert {name: getattr(dst, name).data_ptr() for name in RING} == ptrs           # copied in place
    assert torch.equal(dst.state.view(torch.int32), src.state.view(torch.int32))    # random bits hold NaNs: as integers


@pytest.mark.parametrize("kw,field", [(dict(horizon=T + 1), "L"), (dict(num_learners=1), "num_learners"),
                                      (dict(packed_flags=True), "packed")])
def test_ring_of_another_shape_is_refused_unmodified(kw, field):
    sd = _ring(seed=2).state_dict()
    other = _ring(seed=3, **kw)
    before, count = _bits(other), other.count
    with pytest.raises(ValueError, match=f"uavx: .*{field}"):
        other.load_state_dict(sd)
    assert _same_bits(_bits(other), before) and other.count == count


def test_ring_with_a_damaged_tensor_is_refused_unmodified():
    sd = _ring(seed=2).state_dict()
    sd["ended"] = sd["ended"][:-1]
    other = _ring(seed=3)
    before = _bits(other)
    with pytest.raises(ValueError, match="uavx: .*'ended'"):
        other.load_state_dict(sd)
    assert _same_bits(_bits(other), before)


def test_file_round_trip_of_the_memory_and_extra(tmp_path):
    path = str(tmp_path / "run.pt")
    src, dst = _ring(seed=4), _ring()
    gen = torch.Generator().manual_seed(11)
    torch.rand(5, generator=gen)
    extra = {"t": 17, "note": "mid-episode", "beta": 0.4, "nested": [1, 2.5, None, True]}
    assert save_run(path, memory=src, generator=gen, extra=extra) == path
    blob = torch.load(path, weights_only=True)                        # nothing but tensors and built-in types
    assert blob["format"] == 1 and set(blob) == {"format", "include_memory", "extra", "memory", "generator"}
    assert torch.equal(blob["generator"], gen.get_state())
    other = torch.Generator().manual_seed(99)
    assert load_run(path, memory=dst, generator=other) == extra
    assert _same_bits(_bits(dst), _bits(src)) and dst.count == src.count
    assert torch.equal(other.get_state(), gen.get_state())
    assert torch.equal(torch.rand(3, generator=other), torch.rand(3, generator=gen))
    assert os.listdir(tmp_path) == ["run.pt"]


def test_extra_takes_plain_values_only(tmp_path):
    path = str(tmp_path / "run.pt")
    with pytest.raises(TypeError, match="uavx: .*extra"):
        save_run(path, memory=_ring(seed=4), extra={"when": types.SimpleNamespace()})
    with pytest.raises(TypeError, match="uavx: .*extra"):
        save_run(path, memory=_ring(seed=4), extra=[1, 2])
    assert os.listdir(tmp_path) == []


def test_refusals(tmp_path):
    path = str(tmp_path / "run.pt")
    src = _ring(seed=5)
    gen = torch.Generator().manual_seed(1)
    save_run(path, memory=src, extra={"t": 1})
    dst = _ring(seed=6)
    before = _bits(dst)
    with pytest.raises(ValueError, match="uavx: .*generator"):        # asked for, not in the file
        load_run(path, memory=dst, generator=gen)
    with pytest.raises(ValueError, match="uavx: .*memory"):           # in the file, not asked for
        load_run(path)
    assert _same_bits(_bits(dst), before)
    blob = torch.load(path, weights_only=True)
    blob["format"] = 2
    torch.save(blob, path)
    with pytest.raises(ValueError, match="uavx: .*format"):
        load_run(path, memory=dst)
    torch.save([1, 2, 3], path)
    with pytest.raises(ValueError, match="uavx: .*format"):
        load_run(path, memory=dst)
    assert _same_bits(_bits(dst), before)


def test_a_file_without_the_memory_refuses_a_ring(tmp_path):
    path = str(tmp_path / "run.pt")
    gen = torch.Generator().manual_seed(1)
    save_run(path, memory=_ring(seed=5), generator=gen, extra={"t": 3}, include_memory=False)
    blob = torch.load(path, weights_only=True)
    assert "memory" not in blob and blob["include_memory"] is False
    dst = _ring(seed=6)
    before, count = _bits(dst), dst.count
    with pytest.raises(ValueError, match="uavx: .*include_memory=False"):
        load_run(path, memory=dst, generator=gen)
    assert _same_bits(_bits(dst), before) and dst.count == count
    assert load_run(path, generator=gen) == {"t": 3}                  # the caller's ring is left as it is


def test_a_failed_write_leaves_the_previous_file(tmp_path, monkeypatch):
    path = str(tmp_path / "run.pt")
    save_run(path, memory=_ring(seed=7), extra={"t": 1})
    with open(path, "rb") as f:
        earlier = f.read()
    real = torch.save

    def half_way(obj, f, *a, **k):
        f.write(b"half of a file")
        f.flush()
        raise OSError("disk full")

    monkeypatch.setattr(checkpoint.torch, "save", half_way)
    with pytest.raises(OSError, match="disk full"):
        save_run(path, memory=_ring(seed=8), extra={"t": 2})
    monkeypatch.setattr(checkpoint.torch, "save", real)
    with open(path, "rb") as f:
        assert f.read() == earlier
    assert os.listdir(tmp_path) == ["run.pt"]
    dst = _ring()
    assert load_run(path, memory=dst) == {"t": 1}
    assert _same_bits(_bits(dst), _bits(_ring(seed=7)))
