"""train_state -- save and resume a whole training run, bit for bit.

The reference keeps a 5-element checkpoint (ddpg_agent.py:158-161: normalizer mean / std + the actor) and only wished for more
(:54-62, "load the data to continue the training", commented out).  A *training state* is everything the run's future depends
on: both networks and their targets, Adam m / v / step, all of both normalizers, the device MT19937 stream, the replay buffer's
episodes and counters (library side: hp_state_capture / hp_state_fetch / hp_state_restore, csrc/state.hip), plus the host side of
a run: numpy's global RandomState, success_rates, savetime, the epoch reached and the caller's opaque `extra` bytes.

File: ONE uncompressed .npz of named arrays a person can open with numpy --

    actor critic actor_target critic_target adam_{actor,critic}_{m,v}      float32, named_parameters() order (utils.py:18-27)
    adam_step  o_norm_* g_norm_*  rng_key rng_pos  buffer_{obs,ag,g,actions}  buffer_counters
    np_random_key  success_rates  extra  manifest
    explore_stream_{keys,pos,has_gauss,gauss}      only when the agent explores with one stream per environment
                                                   (ddpg_agent.enable_explore_streams): uint32 [n, 624], int32 [n], int32 [n], float64 [n]

`manifest` is JSON text: format version, dims, capacity, T, rank, world size, library ABI, dtype / shape / checksum (A, B) of every
device array, and the host scalars.  It is written to a temporary name and renamed, so a killed process never leaves a half-written
state under the final name.

Checksum of an array: its bytes as little-endian 64-bit words w_0 .. w_{n-1} (zero-padded to 8 bytes), A = sum w_i mod 2^64,
B = sum (i + 1) w_i mod 2^64.  The device computes it on the snapshot at capture and again on the uploaded bytes at restore
(k_checksum); `checksum()` below is its numpy twin, so

    python -m rl_arm_under_sparse_reward_amd.train_state verify FILE

checks a state file on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
import zipfile

import numpy as np

FORMAT_VERSION = 1
_DTYPES = {0: "<f4", 1: "<f8", 2: "<i8", 3: "<u4", 4: "<i4"}        # hp_state_section.dtype
_NORM_FIELDS = ("local_sum", "local_sumsq", "local_count", "total_sum", "total_sumsq", "total_count", "mean", "std")
_MASK = (1 << 64) - 1


class StateError(ValueError):
    """A training-state file that cannot be used; the message names the array or manifest field at fault."""


# ---------------------------------------------------------------------------------------------------- checksum (numpy twin)
def checksum(data) -> tuple[int, int]:
    """(A, B) of `data` (bytes or any array): the numpy twin of the device's k_checksum."""
    raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8) if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
    pad = (-raw.size) % 8
    if pad:
        raw = np.concatenate([raw, np.zeros(pad, np.uint8)])
    w = raw.view("<u8")
    a = b = 0
    step = 1 << 20                      # a chunk at a time: the index vector of a 150 MB section would be another 150 MB
    with np.errstate(over="ignore"):
        for i in range(0, w.size, step):
            c = w[i:i + step]
            a += int(c.sum(dtype=np.uint64))
            b += int((c * np.arange(i + 1, i + 1 + c.size, dtype=np.uint64)).sum(dtype=np.uint64))
    return a & _MASK, b & _MASK


# ---------------------------------------------------------------------------------------------------- what the dims imply
def expected_shapes(dims: dict) -> dict:
    """name -> (dtype, shape) of every device array of a state with these dims (models.py:11-44, normalizer.py:12-20,
    replay_buffer.py:23-27)."""
    o, g, a, H, T, cs = (int(dims[k]) for k in ("obs", "goal", "action", "hidden", "T", "current_size"))
    na = H * (o + g) + H + 2 * (H * H + H) + a * H + a
    nc = H * (o + g + a) + H + 2 * (H * H + H) + H + 1
    out = {"actor": ("<f4", (na,)), "critic": ("<f4", (nc,)), "actor_target": ("<f4", (na,)), "critic_target": ("<f4", (nc,)),
           "adam_actor_m": ("<f4", (na,)), "adam_actor_v": ("<f4", (na,)), "adam_critic_m": ("<f4", (nc,)),
           "adam_critic_v": ("<f4", (nc,)), "adam_step": ("<i8", (1,))}
    for pre, n in (("o_norm", o), ("g_norm", g)):
        for f in _NORM_FIELDS:
            out[f"{pre}_{f}"] = ("<f8" if f == "std" else "<f4", (1,) if f.endswith("count") else (n,))
    out.update({"rng_key": ("<u4", (624,)), "rng_pos": ("<i4", (1,)),
                "buffer_obs": ("<f8", (cs, T + 1, o)), "buffer_ag": ("<f8", (cs, T + 1, g)), "buffer_g": ("<f8", (cs, T, g)),
                "buffer_actions": ("<f8", (cs, T, a)), "buffer_counters": ("<i8", (2,))})
    return out


def stream_shapes(n: int) -> dict:
    """name -> (dtype, shape) of the arrays that carry n per-environment exploration streams (random.DeviceRandomStreams): numpy's
    legacy state of every stream -- key, position, has_gauss, cached normal.  A state saved without such streams has none of
    them and no 'explore_streams' field in its manifest."""
    n = int(n)
    return {"explore_stream_keys": ("<u4", (n, 624)), "explore_stream_pos": ("<i4", (n,)),
            "explore_stream_has_gauss": ("<i4", (n,)), "explore_stream_gauss": ("<f8", (n,))}


STREAM_ARRAYS = tuple(stream_shapes(0))
DEVICE_ARRAYS = tuple(expected_shapes({"obs": 1, "goal": 1, "action": 1, "hidden": 1, "T": 1, "current_size": 0}))


# ---------------------------------------------------------------------------------------------------- file
def _write_npz(f, arrays):
    np.savez(f, **arrays)


def write_state(path, arrays: dict, manifest: dict):
    """One uncompressed .npz under `path`, via a temporary name in the same directory + rename."""
    path = os.fspath(path)
    payload = dict(arrays)
    payload["manifest"] = np.array(json.dumps(manifest, sort_keys=True))
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            _write_npz(f, payload)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    return path


def read_state(path):
    """-> (arrays, manifest).  Nothing is executed: the file holds arrays and JSON text only (allow_pickle=False)."""
    try:
        with np.load(os.fspath(path), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
    except (zipfile.BadZipFile, EOFError, OSError, ValueError, KeyError) as e:
        raise StateError(f"{path}: not a readable training state ({type(e).__name__}: {e})") from e
    if "manifest" not in arrays:
        raise StateError(f"{path}: array 'manifest' is missing")
    try:
        manifest = json.loads(str(arrays.pop("manifest")[()]))
    except ValueError as e:
        raise StateError(f"{path}: 'manifest' is not JSON ({e})") from e
    if manifest.get("format") != FORMAT_VERSION:
        raise StateError(f"{path}: manifest 'format' is {manifest.get('format')!r}, this build reads {FORMAT_VERSION}")
    return arrays, manifest


def _check_array(where, name, arrays, listed, want, implied_by, sums, entry=True):
    """One array of a state: present, listed in the manifest, of the dtype and shape `implied_by` implies (`want`) and
    (entry=True) its manifest entry records, and (sums=True) summing to the (A, B) recorded there."""
    if name not in arrays:
        raise StateError(f"{where}: array '{name}' is missing")
    if name not in listed:
        raise StateError(f"{where}: manifest has no entry for array '{name}'")
    a, (dt, shape) = arrays[name], want
    if a.dtype.newbyteorder("<") != np.dtype(dt) or tuple(a.shape) != tuple(shape):
        raise StateError(f"{where}: array '{name}' is {a.dtype} {tuple(a.shape)}, {implied_by} imply {np.dtype(dt)} {tuple(shape)}")
    if entry and (listed[name]["dtype"] != dt or tuple(listed[name]["shape"]) != tuple(shape)):
        raise StateError(f"{where}: manifest entry of array '{name}' ({listed[name]['dtype']} {tuple(listed[name]['shape'])}) "
                         f"contradicts its dims ({dt} {tuple(shape)})")
    if sums:
        got, said = checksum(a), [int(x) for x in listed[name]["sum"]]
        if list(got) != said:
            raise StateError(f"{where}: array '{name}' sums to ({got[0]:016x}, {got[1]:016x}), the manifest says "
                             f"({said[0]:016x}, {said[1]:016x})")


def check_arrays(arrays, manifest, sums=True, where="state"):
    """Every device array present, shaped as the manifest's dims imply and as the manifest records, and (sums=True) its bytes
    summing to the manifest's (A, B).  Raises StateError naming the array."""
    want = expected_shapes(manifest["dims"])
    listed = manifest["arrays"]
    for name in DEVICE_ARRAYS:
        _check_array(where, name, arrays, listed, want[name], "the manifest's dims", sums)
    if int(arrays["buffer_counters"][0]) != int(manifest["dims"]["current_size"]):
        raise StateError(f"{where}: array 'buffer_counters' says current_size {int(arrays['buffer_counters'][0])}, "
                         f"the manifest {manifest['dims']['current_size']}")
    for name in ("np_random_key", "success_rates", "extra"):
        if name not in arrays:
            raise StateError(f"{where}: array '{name}' is missing")
    check_stream_arrays(arrays, manifest, where=where)


def check_stream_arrays(arrays, manifest, where="state"):
    """The per-environment exploration streams of a state: all four arrays or none, as the manifest's 'explore_streams' field
    says, shaped for its stream count, positions inside [0, 624], and summing to what it records (they are a few KB per stream and
    reach the device by a plain copy, so their sums are always checked here, on the host)."""
    rec = manifest.get("explore_streams")
    if rec is None:
        extra = [n for n in STREAM_ARRAYS if n in arrays]
        if extra:
            raise StateError(f"{where}: array '{extra[0]}' is present but the manifest has no 'explore_streams' field")
        return
    want = stream_shapes(rec["n"])
    for name in STREAM_ARRAYS:
        _check_array(where, name, arrays, rec["arrays"], want[name], f"{rec['n']} streams", True, entry=False)
    pos = arrays["explore_stream_pos"]
    if pos.size and (int(pos.min()) < 0 or int(pos.max()) > 624):
        raise StateError(f"{where}: array 'explore_stream_pos' holds a position outside [0, 624]")


def stream_record(keys, pos, has_gauss, gauss):
    """(arrays, manifest field) of n exploration streams, as a state file stores them."""
    n = int(np.asarray(pos).size)
    arrays = {}
    for (name, (dt, shape)), a in zip(stream_shapes(n).items(), (keys, pos, has_gauss, gauss)):
        arrays[name] = np.ascontiguousarray(a, dtype=dt).reshape(shape)
    rec = {"n": n, "arrays": {k: {"dtype": stream_shapes(n)[k][0], "shape": list(a.shape), "sum": list(checksum(a))}
                              for k, a in arrays.items()}}
    return arrays, rec


def verify(path):
    """Check a state file without a GPU; returns its manifest."""
    arrays, manifest = read_state(path)
    check_arrays(arrays, manifest, sums=True, where=os.fspath(path))
    return manifest


def rank_path(path, rank):
    """`state.npz` -> `state_rank3.npz`: every rank of a data-parallel run keeps its own file (its buffer is its episode shard)."""
    root, ext = os.path.splitext(os.fspath(path))
    return f"{root}_rank{int(rank)}{ext}"


# ---------------------------------------------------------------------------------------------------- device side
def _dims_of(agent, current_size):
    ep = agent.env_params
    return {"obs": int(ep["obs"]), "goal": int(ep["goal"]), "action": int(ep["action"]), "hidden": 256,
            "T": int(agent.buffer._dev.T), "capacity": int(agent.buffer._dev.size), "current_size": int(current_size)}


def _layout(agent, current_size=-1):
    from . import _lib
    secs = (_lib.StateSection * _lib.STATE_SECTIONS)()
    n, total = C.c_int32(_lib.STATE_SECTIONS), C.c_size_t()
    _lib.check(agent.lib.hp_state_layout(agent.h, agent.buffer._dev.h, agent.o_norm.h, agent.g_norm.h, int(current_size), secs,
                                         C.byref(n), C.byref(total)))
    return [(s.name.decode(), _DTYPES[s.dtype], int(s.count), int(s.offset)) for s in secs[:n.value]], int(total.value)


class PendingSave:
    """A capture in flight (`save_training_state(wait=False)`): the device part was snapshotted in stream order when this object
    was made, the host part (numpy's stream, success_rates, savetime) copied at the same moment; training may go on.
    `.result()` waits for the drain, writes the file and returns its path.  While it is outstanding a second capture on the same
    agent raises (HP_ERR_STATE)."""

    def __init__(self, agent, path, extra=None, epoch=0, cycle=0):
        from . import _lib
        self.agent, self.path, self._done = agent, os.fspath(path), None
        agent._flush_updates()
        ticket, nbytes = C.c_uint64(), C.c_size_t()
        _lib.check(agent.lib.hp_state_capture(*agent._handles(), C.byref(ticket), C.byref(nbytes)))
        self.ticket, self.nbytes = ticket.value, nbytes.value
        # (no library call between the capture and this: the buffer's size is the captured one)
        self.sections, total = _layout(agent, -1)
        assert total == self.nbytes, (total, self.nbytes)
        st = np.random.get_state()
        gauss = agent.rng._gauss
        self.host = {"np_random": {"pos": int(st[2]), "has_gauss": int(st[3]), "cached_gaussian": float(st[4])},
                     "rng_gauss": [int(gauss[0]), float(gauss[1])], "savetime": int(agent.savetime), "epoch": int(epoch),
                     "cycle": int(cycle)}
        self.host_arrays = {"np_random_key": np.array(st[1], dtype=np.uint32),
                            "success_rates": np.array(agent.success_rates, dtype=np.float64),
                            "extra": np.frombuffer(bytes(extra or b""), dtype=np.uint8).copy()}
        streams = getattr(agent, "explore_streams", None)
        if streams is not None:
            # copied now (a few KB per stream; synchronises), so rollouts that follow a wait=False capture do not move them
            stream_arrays, self.host["explore_streams"] = stream_record(*streams.get_arrays())
            self.host_arrays.update(stream_arrays)

    def done(self):
        return self._done is not None

    def result(self):
        if self._done is not None:
            return self._done
        from . import _lib
        agent = self.agent
        blob = np.empty(self.nbytes, np.uint8)
        sums = (C.c_uint64 * (2 * _lib.STATE_SECTIONS))()
        done = C.c_int32()
        fetch = object.__getattribute__(agent.lib, "_cdll").hp_state_fetch      # no flush of deferred updates in front of a wait
        _lib.check(fetch(agent.h, self.ticket, 1, blob.ctypes.data_as(C.c_void_p), blob.size, sums, C.byref(done)))
        off_counters = next(o for n, _, _, o in self.sections if n == "buffer_counters")
        cs = int(blob[off_counters:off_counters + 8].view("<i8")[0])
        dims = _dims_of(agent, cs)
        want = expected_shapes(dims)
        arrays, listed = {}, {}
        for i, (name, dt, count, off) in enumerate(self.sections):
            a = blob[off:off + count * np.dtype(dt).itemsize].view(dt).reshape(want[name][1])
            dev = (int(sums[2 * i]), int(sums[2 * i + 1]))
            if checksum(a) != dev:      # what left the device is what the device summed
                raise StateError(f"save: array '{name}' arrived with sums {checksum(a)}, the device computed {dev}")
            arrays[name] = a
            listed[name] = {"dtype": dt, "shape": list(a.shape), "sum": [dev[0], dev[1]]}
        manifest = {"format": FORMAT_VERSION, "dims": dims, "rank": int(agent.comm.rank), "world_size": int(agent.comm.world_size),
                    "abi": int(_lib.ABI_VERSION), "arrays": listed, **self.host}
        arrays.update(self.host_arrays)
        self._done = write_state(self.path, arrays, manifest)
        return self._done


def save(agent, path, wait=True, extra=None, epoch=0, cycle=0):
    h = PendingSave(agent, path, extra=extra, epoch=epoch, cycle=cycle)
    return h.result() if wait else h


def load(agent, path, verify_host=False):
    """Restore `agent` (its networks, optimizers, normalizers, random stream and replay buffer) and the host side of the run
    from a state file; returns (extra bytes, manifest).  A file that does not fit the agent -- dims, capacity, T, rank, world size
    -- or whose bytes do not sum on the DEVICE to what the manifest records is refused before anything is changed."""
    from . import _lib
    arrays, manifest = read_state(path)
    where = os.fspath(path)
    if int(manifest.get("abi", -1)) != _lib.ABI_VERSION:
        raise StateError(f"{where}: written with library ABI {manifest.get('abi')}, this build has {_lib.ABI_VERSION}")
    for key, have in (("rank", agent.comm.rank), ("world_size", agent.comm.world_size)):
        if int(manifest[key]) != int(have):
            raise StateError(f"{where}: {key} of the state is {manifest[key]}, this process has {have} "
                             "(every rank loads its own file; re-sharding is not supported)")
    mine = _dims_of(agent, manifest["dims"]["current_size"])
    for key in ("obs", "goal", "action", "hidden", "T", "capacity"):
        if int(manifest["dims"][key]) != mine[key]:
            raise StateError(f"{where}: {key} of the state is {manifest['dims'][key]}, the receiver has {mine[key]}")
    streams, rec = getattr(agent, "explore_streams", None), manifest.get("explore_streams")
    names = ", ".join(f"'{n}'" for n in STREAM_ARRAYS)
    if streams is not None and rec is None:
        raise StateError(f"{where}: the agent explores with one stream per environment, but the state was saved without: arrays "
                         f"{names} are missing")
    if streams is None and rec is not None:
        raise StateError(f"{where}: the state carries {rec['n']} per-environment exploration streams (arrays {names}), but the "
                         "agent has none: call enable_explore_streams() (args.explore_streams) before loading")
    if streams is not None and int(rec["n"]) != len(streams):
        raise StateError(f"{where}: array 'explore_stream_keys' holds {rec['n']} streams, the agent has {len(streams)} environments")
    check_arrays(arrays, manifest, sums=verify_host, where=where)
    agent._flush_updates()
    sections, total = _layout(agent, mine["current_size"])
    blob = np.zeros(total, np.uint8)
    sums = (C.c_uint64 * (2 * _lib.STATE_SECTIONS))()
    for i, (name, dt, count, off) in enumerate(sections):
        a = np.ascontiguousarray(arrays[name], dtype=dt).reshape(-1)
        if a.size != count:
            raise StateError(f"{where}: array '{name}' has {a.size} elements, the receiver's layout {count}")
        blob[off:off + a.nbytes] = a.view(np.uint8)
        sums[2 * i], sums[2 * i + 1] = (int(x) for x in manifest["arrays"][name]["sum"])
    d = manifest["dims"]
    dims = _lib.StateDims(obs_dim=d["obs"], goal_dim=d["goal"], act_dim=d["action"], hidden=d["hidden"], T=d["T"], reserved=0,
                          capacity=d["capacity"], current_size=d["current_size"])
    try:
        _lib.check(agent.lib.hp_state_restore(*agent._handles(), C.byref(dims), blob.ctypes.data_as(C.c_void_p), blob.size, sums))
    except ValueError as e:
        raise StateError(f"{where}: {e}") from e
    # host side of the run
    r = manifest["np_random"]
    np.random.set_state(("MT19937", arrays["np_random_key"], int(r["pos"]), int(r["has_gauss"]), float(r["cached_gaussian"])))
    agent.rng.seeded = True
    agent.rng._gauss = (int(manifest["rng_gauss"][0]), float(manifest["rng_gauss"][1]))
    if streams is not None:
        streams.set_arrays(*(arrays[n] for n in STREAM_ARRAYS))
    agent.success_rates = [float(x) for x in arrays["success_rates"]]
    agent.savetime = int(manifest["savetime"])
    return arrays["extra"].tobytes(), manifest


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) != 2 or argv[0] != "verify":
        print("usage: python -m rl_arm_under_sparse_reward_amd.train_state verify FILE", file=sys.stderr)
        return 2
    try:
        m = verify(argv[1])
    except StateError as e:
        print(f"FAILED: {e}", file=sys.stderr)
        return 1
    d = m["dims"]
    print(f"ok: {argv[1]}: format {m['format']}, rank {m['rank']}/{m['world_size']}, epoch {m['epoch']}, "
          f"{d['current_size']}/{d['capacity']} episodes of T={d['T']}, obs/goal/action {d['obs']}/{d['goal']}/{d['action']}, "
          f"{len(m['arrays'])} arrays verified")
    return 0


if __name__ == "__main__":
    sys.exit(main())
