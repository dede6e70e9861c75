"""save_run / load_run: one file that stops a whole training run and continues it bit for bit.

    save_run(path, env=venv.env, memory=mem, agent=agent, exploration=ex, generator=gen, extra={"t": t})
    extra = load_run(path, env=venv.env, memory=mem, agent=agent, exploration=ex, generator=gen)

A run's state lives in five objects, each with a state_dict() of its own: the worlds (BatchedMultiUAVWorld2D: the
uavx_save snapshot), the replay ring (DeviceReplay), the learner with its prioritized sampler (FusedSAC / FusedTD3 /
FusedDDPG), the acting side (Exploration) and the torch.Generator the sampler and the kernels' noise draw from.  save_run
puts them into ONE torch.save file that holds nothing but tensors and built-in types, so load_run reads it with
torch.load(..., weights_only=True); load_run restores them into objects built from the same constructor arguments, in place,
so that the continued run computes what the uninterrupted one would have.  Neither is on the step or update path: one
synchronisation and some copies, no kernel."""
import os
import tempfile

import torch

FORMAT = 1
PARTS = ("env", "memory", "agent", "exploration", "generator")      # load_run's restore order: the generator last
_PLAIN = (type(None), bool, int, float, str)


def _plain(x, where):
    """x with every tensor detached and on the CPU, refusing what torch.load(weights_only=True) would not read back."""
    if torch.is_tensor(x):
        return x.detach().cpu()
    if type(x) in _PLAIN:
        return x
    if type(x) is dict:
        for k in x:
            if type(k) not in (str, int):
                raise TypeError(f"uavx: save_run keeps tensors and built-in types only: {where} has a key {k!r}")
        return {k: _plain(v, f"{where}[{k!r}]") for k, v in x.items()}
    if type(x) in (list, tuple):
        return type(x)(_plain(v, f"{where}[{i}]") for i, v in enumerate(x))
    raise TypeError(f"uavx: save_run keeps tensors and built-in types only: {where} is a {type(x).__name__}")


def _synchronize(*objs):
    """Waits for every GPU the given parts live on."""
    seen = set()
    for o in objs:
        dev = getattr(o, "device", None)
        if dev is None and o is not None and hasattr(o, "obs"):
            dev = o.obs.device                               # a DeviceReplay
        if dev is not None and torch.device(dev).type == "cuda" and torch.device(dev) not in seen:
            seen.add(torch.device(dev))
            torch.cuda.synchronize(torch.device(dev))


def _write_atomic(path, blob):
    """torch.save into a temporary file beside `path`, flushed to the disk, then renamed over it: a failure on the way leaves
    the previous file as it was and no temporary behind."""
    path = os.fspath(path)
    folder = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(dir=folder, prefix=os.path.basename(path) + ".", suffix=".tmp")
    try:
        with os.fdopen(fd, "wb") as f:
            torch.save(blob, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except FileNotFoundError:
            pass
        raise


def save_run(path, env=None, memory=None, agent=None, exploration=None, generator=None, extra=None, include_memory=True):
    """Writes the state of the given parts of a run to `path`, atomically.  Every part is optional: env (a
    BatchedMultiUAVWorld2D, e.g. UAVVectorEnv.env), memory (a DeviceReplay), agent (a fused learner; its prioritized
    sampler's table goes with it), exploration (an Exploration), generator (a torch.Generator), extra (a dict of plain
    Python values, e.g. the loop index).  The call synchronises once and copies to the host.

    include_memory=False leaves the ring and the priority table out of the file, which is then a few megabytes however long
    the horizon.  A run resumed from such a file starts from an EMPTY ring that the caller refills: it keeps its networks,
    optimisers, worlds and noise streams, but it is NOT the bit-exact continuation of the run that was stopped."""
    if extra is not None and type(extra) is not dict:
        raise TypeError(f"uavx: save_run takes extra as a dict of plain Python values, not {type(extra).__name__}")
    if not include_memory:
        memory = None
    _synchronize(env, memory, agent, exploration)
    blob = {"format": FORMAT, "include_memory": bool(include_memory), "extra": _plain(extra or {}, "extra")}
    if env is not None:
        blob["env"] = _plain(env.state_dict(), "env")
    if memory is not None:
        blob["memory"] = _plain(memory.state_dict(), "memory")
    if agent is not None:
        blob["agent"] = _plain(agent.state_dict(include_sampler=include_memory), "agent")
    if exploration is not None:
        blob["exploration"] = _plain(exploration.state_dict(), "exploration")
    if generator is not None:
        blob["generator"] = generator.get_state().cpu()
    _write_atomic(path, blob)
    return path


def load_run(path, env=None, memory=None, agent=None, exploration=None, generator=None):
    """Restores the parts save_run wrote into the given objects, built from the same constructor arguments as the saved
    ones, and returns the file's `extra`.  The parts given must be the parts the file holds: one missing on either side is
    refused before anything is restored, as is a file of an unknown format, and memory= for a file written with
    include_memory=False (the caller's ring is then left as it is).  Each part refuses a state of another shape or
    configuration itself.  Restored in the order env, ring, learner (with its sampler), exploration, generator; everything is
    copied in place, the learner drops its captured graphs (capture() again before run()), and the call returns when its
    copies are done."""
    blob = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    if not isinstance(blob, dict) or blob.get("format") != FORMAT:
        got = blob.get("format") if isinstance(blob, dict) else type(blob).__name__
        raise ValueError(f"uavx: {os.fspath(path)!r} is not a run file of format {FORMAT} (format = {got!r})")
    given = dict(zip(PARTS, (env, memory, agent, exploration, generator)))
    if memory is not None and not blob.get("include_memory", True):
        raise ValueError("uavx: this run file was written with include_memory=False and holds no ring: call load_run "
                         "without memory= and refill a fresh one")
    for part, obj in given.items():
        if obj is not None and part not in blob:
            raise ValueError(f"uavx: load_run was given {part}=, which this run file does not hold")
        if obj is None and part in blob:
            raise ValueError(f"uavx: this run file holds the {part}, which load_run was not given ({part}=)")
    for part in PARTS[:-1]:
        if given[part] is not None:
            given[part].load_state_dict(blob[part])
    if generator is not None:
        generator.set_state(blob["generator"])
    _synchronize(env, memory, agent, exploration)
    return blob["extra"]
