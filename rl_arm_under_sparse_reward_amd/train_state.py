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
    reset_stream_{keys,pos,has_gauss,gauss}        only when the agent's environment is reset on the device
                                                   (device_env.NativePointMassVecEnv.enable_device_reset): the same four, one
                                                   reset stream per environment; manifest field 'reset_streams'

`manifest` is JSON text: format version, dims, capacity, T, rank, world size, library ABI, dtype / shape / checksum (A, B) of every
device array, and the host scalars.  It is written to a temporary name and renamed, so a killed process never leaves a half-written
state under the final name.

Checksum of an array: its bytes as little-endian 64-bit words w_0 .. w_{n-1} (zero-padded to 8 bytes), A = sum w_i mod 2^64,
B = sum (i + 1) w_i mod 2^64.  The device computes it on the snapshot at capture and again on the uploaded bytes at restore
(k_checksum); `checksum()` below is its numpy twin, so

    python -m rl_arm_under_sparse_reward_amd.train_state verify FILE

checks a state file on a machine without a GPU.

Delta states.  A full save writes the whole replay buffer again (149 MB of rows per rank at the reference's size, against 3 MB
stored between two epochs).  `save(agent, path, base=FULL)` writes a *delta* instead: every small array under the names above, and
the buffer as the episodes written since the full state FULL was captured --

    buffer_delta_slots                      int64 [n_dirty], ascending
    buffer_delta_{obs,ag,g,actions}         float64 [n_dirty, ...]: the rows of those slots
    buffer_counters, host arrays, exploration- and reset-stream arrays as in a full state

with manifest format 2, "kind": "delta", its own "capture_epoch", "dims" with the NEW current_size and
"base": {name, lineage, capture_epoch, current_size, sums of the base's four buffer arrays}.  A full state's manifest carries
"lineage" (a 64-bit id made at an agent's first save -- a hash of that state's checksums -- and kept across resumes) and "capture_epoch" (the buffer epoch the
capture recorded, csrc/state.hip); one without them -- written before deltas existed -- cannot serve as a base.  The base of a
delta is always a full state.  `compose(base, delta)` (pure numpy) rebuilds what a full state taken at the delta's instant
holds; `load()` of a delta composes and then restores as ever.

    python -m rl_arm_under_sparse_reward_amd.train_state verify DELTA [--base BASE]
    python -m rl_arm_under_sparse_reward_amd.train_state flatten BASE DELTA OUT
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import sys
import zipfile

import numpy as np

FORMAT_VERSION = 1
DELTA_FORMAT_VERSION = 2            # a delta: refused by a reader that knows format 1 only
BUFFER_ARRAYS = ("buffer_obs", "buffer_ag", "buffer_g", "buffer_actions")
DELTA_ROW_ARRAYS = ("buffer_delta_obs", "buffer_delta_ag", "buffer_delta_g", "buffer_delta_actions")
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


def stream_shapes(n: int, family: str = "explore") -> dict:
    """name -> (dtype, shape) of the arrays that carry n per-environment streams (random.DeviceRandomStreams) of one family --
    'explore': the exploration streams, 'reset': the environments' reset streams: numpy's legacy state of every stream -- key,
    position, has_gauss, cached normal.  A state saved without the streams of a family has none of its arrays and no
    '<family>_streams' field in its manifest."""
    n = int(n)
    return {f"{family}_stream_keys": ("<u4", (n, 624)), f"{family}_stream_pos": ("<i4", (n,)),
            f"{family}_stream_has_gauss": ("<i4", (n,)), f"{family}_stream_gauss": ("<f8", (n,))}


def _family(name, find, saved_without, agent_without):
    """One family of per-environment streams: how to find the agent's (`find(agent)` -> DeviceRandomStreams or None), its array
    names, its manifest field, and what load() says when agent and state disagree about it."""
    return {"find": find, "arrays": tuple(stream_shapes(0, name)), "field": f"{name}_streams",
            "saved_without": saved_without, "agent_without": agent_without}


# in the order load() refuses them
STREAM_FAMILIES = {
    "explore": _family(
        "explore", lambda agent: getattr(agent, "explore_streams", None),
        "the agent explores with one stream per environment, but the state was saved without: arrays {names} are missing",
        "the state carries {n} per-environment exploration streams (arrays {names}), but the agent has none: call "
        "enable_explore_streams() (args.explore_streams) before loading"),
    # the environments' reset generators (device_env: enable_device_reset); None: no such environment, or it is reset on the host
    "reset": _family(
        "reset", lambda agent: getattr(getattr(agent, "vec_env", None), "reset_streams", None),
        "the agent's environment is reset on the device, but the state was saved without reset streams: arrays {names} are missing",
        "the state carries {n} per-environment reset streams (arrays {names}), but the agent's environment is reset on the host: "
        "call vec_env.enable_device_reset() (args.device_reset) before loading"),
}
STREAM_ARRAYS = STREAM_FAMILIES["explore"]["arrays"]
RESET_STREAM_ARRAYS = STREAM_FAMILIES["reset"]["arrays"]
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


def _read_npz(path, take):
    """take(the open .npz); whatever makes the file unreadable becomes a StateError."""
    try:
        with np.load(os.fspath(path), allow_pickle=False) as z:
            return take(z)
    except (zipfile.BadZipFile, EOFError, OSError, ValueError, KeyError) as e:
        raise StateError(f"{path}: not a readable training state ({type(e).__name__}: {e})") from e


def read_state(path):
    """-> (arrays, manifest).  Nothing is executed: the file holds arrays and JSON text only (allow_pickle=False)."""
    arrays = _read_npz(path, lambda z: {k: z[k] for k in z.files})
    if "manifest" not in arrays:
        raise StateError(f"{path}: array 'manifest' is missing")
    try:
        manifest = json.loads(str(arrays.pop("manifest")[()]))
    except ValueError as e:
        raise StateError(f"{path}: 'manifest' is not JSON ({e})") from e
    fmt, kind = manifest.get("format"), manifest.get("kind", "full")
    if (fmt, kind) not in ((FORMAT_VERSION, "full"), (DELTA_FORMAT_VERSION, "delta")):
        raise StateError(f"{path}: manifest 'format' is {fmt!r} ('kind' {kind!r}), this build reads {FORMAT_VERSION} (full states) "
                         f"and {DELTA_FORMAT_VERSION} (deltas)")
    return arrays, manifest


def read_manifest(path):
    """The manifest alone (the arrays of an .npz are read on access: a 150 MB base costs nothing here)."""
    return _read_npz(path, lambda z: json.loads(str(z["manifest"][()])))


def is_delta(manifest) -> bool:
    return manifest.get("kind", "full") == "delta"


def delta_path(path):
    """`state.npz` -> `state.delta.npz`: the cumulative delta learn() keeps beside its base (args.state_full_every)."""
    root, ext = os.path.splitext(os.fspath(path))
    return f"{root}.delta{ext}"


def delta_shapes(dims: dict, n_dirty: int) -> dict:
    """name -> (dtype, shape) of the arrays that stand for the buffer in a delta of n_dirty episodes."""
    o, g, a, T, n = int(dims["obs"]), int(dims["goal"]), int(dims["action"]), int(dims["T"]), int(n_dirty)
    return {"buffer_delta_slots": ("<i8", (n,)), "buffer_delta_obs": ("<f8", (n, T + 1, o)), "buffer_delta_ag": ("<f8", (n, T + 1, g)),
            "buffer_delta_g": ("<f8", (n, T, g)), "buffer_delta_actions": ("<f8", (n, T, a))}


def base_key(manifest, where="state"):
    """What names a full state as a base: (lineage, capture_epoch, current_size, sums of its four buffer arrays)."""
    if is_delta(manifest):
        raise StateError(f"{where}: manifest 'kind' is 'delta': the base of a delta must be a full state (no delta on a delta)")
    if "lineage" not in manifest or "capture_epoch" not in manifest:
        raise StateError(f"{where}: manifest has no 'lineage' / 'capture_epoch': this full state was written before delta states "
                         "existed and cannot serve as a base (load it and save a new full state)")
    return {"lineage": str(manifest["lineage"]), "capture_epoch": int(manifest["capture_epoch"]),
            "current_size": int(manifest["dims"]["current_size"]),
            "sums": {n: [int(x) for x in manifest["arrays"][n]["sum"]] for n in BUFFER_ARRAYS}}


def _key_tuple(key):
    return (key["lineage"], key["capture_epoch"], key["current_size"], tuple(tuple(key["sums"][n]) for n in BUFFER_ARRAYS))


def cites(delta_manifest, base_manifest, where="base"):
    """Does the delta cite this full state as its base?  The first thing that disagrees -- 'lineage', 'capture_epoch',
    'current_size', or the name of the buffer array whose sums differ -- or None.  StateError when the state cannot be a base."""
    key, cited = base_key(base_manifest, where=where), delta_manifest["base"]
    for field in ("lineage", "capture_epoch", "current_size"):
        if key[field] != type(key[field])(cited[field]):
            return field
    for name in BUFFER_ARRAYS:
        if key["sums"][name] != [int(x) for x in cited["sums"][name]]:
            return name
    return None


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


def _check_listed(arrays, manifest, sums, where, shapes, implied_by="the manifest's dims"):
    """The device arrays of `shapes` (name -> (dtype, shape), implied by `implied_by`), each as _check_array checks one."""
    for name, want in shapes.items():
        _check_array(where, name, arrays, manifest["arrays"], want, implied_by, sums)


def _check_state(arrays, manifest, sums, where, *groups):
    """What a full state and a delta are checked for alike: the device arrays of every (shapes, implied_by) group, buffer_counters
    against the manifest's current_size, the host arrays, the per-environment streams."""
    for group in groups:
        _check_listed(arrays, manifest, sums, where, *group)
    if int(arrays["buffer_counters"][0]) != int(manifest["dims"]["current_size"]):
        raise StateError(f"{where}: array 'buffer_counters' says current_size {int(arrays['buffer_counters'][0])}, "
                         f"the manifest {manifest['dims']['current_size']}")
    for name in ("np_random_key", "success_rates", "extra"):
        if name not in arrays:
            raise StateError(f"{where}: array '{name}' is missing")
    check_stream_arrays(arrays, manifest, where=where)


def check_arrays(arrays, manifest, sums=True, where="state"):
    """Every device array present, shaped as the manifest's dims imply and as the manifest records, and (sums=True) its bytes
    summing to the manifest's (A, B).  Raises StateError naming the array."""
    _check_state(arrays, manifest, sums, where, (expected_shapes(manifest["dims"]),))


def check_stream_arrays(arrays, manifest, where="state"):
    """The per-environment streams of a state, family by family (exploration streams: field 'explore_streams'; the environments'
    reset streams: 'reset_streams'): all four arrays or none, as the manifest's field says, shaped for its stream count, positions
    inside [0, 624], and summing to what it records (they are a few KB per stream and reach the device by a plain copy, so their
    sums are always checked here, on the host)."""
    for family, fam in STREAM_FAMILIES.items():
        field, names = fam["field"], fam["arrays"]
        rec = manifest.get(field)
        if rec is None:
            extra = [n for n in names if n in arrays]
            if extra:
                raise StateError(f"{where}: array '{extra[0]}' is present but the manifest has no '{field}' field")
            continue
        want = stream_shapes(rec["n"], family)
        for name in names:
            _check_array(where, name, arrays, rec["arrays"], want[name], f"{rec['n']} streams", True, entry=False)
        pos = arrays[f"{family}_stream_pos"]
        if pos.size and (int(pos.min()) < 0 or int(pos.max()) > 624):
            raise StateError(f"{where}: array '{family}_stream_pos' holds a position outside [0, 624]")


def stream_record(keys, pos, has_gauss, gauss, family="explore"):
    """(arrays, manifest field) of n streams of one family, as a state file stores them."""
    n = int(np.asarray(pos).size)
    arrays, shapes = {}, stream_shapes(n, family)
    for (name, (dt, shape)), a in zip(shapes.items(), (keys, pos, has_gauss, gauss)):
        arrays[name] = np.ascontiguousarray(a, dtype=dt).reshape(shape)
    rec = {"n": n, "arrays": {k: {"dtype": shapes[k][0], "shape": list(a.shape), "sum": list(checksum(a))}
                              for k, a in arrays.items()}}
    return arrays, rec


def check_delta_arrays(arrays, manifest, sums=True, where="delta"):
    """A delta by itself: every small device array as the dims imply, the slot list and the four row arrays shaped for
    manifest['n_dirty'] and (sums=True) summing to what the manifest records, the slot list strictly ascending inside
    [0, current_size) and holding every slot of the grown region [base current_size, current_size)."""
    dims, n = manifest["dims"], int(manifest["n_dirty"])
    small = {name: want for name, want in expected_shapes(dims).items() if name not in BUFFER_ARRAYS}
    _check_state(arrays, manifest, sums, where, (small,), (delta_shapes(dims, n), f"the manifest's dims and n_dirty {n}"))
    cs, cs0 = int(dims["current_size"]), int(manifest["base"]["current_size"])
    if not 0 <= cs0 <= cs:
        raise StateError(f"{where}: manifest 'base' has current_size {cs0}, the delta {cs}: a buffer does not shrink")
    slots = arrays["buffer_delta_slots"]
    if n and (int(slots[0]) < 0 or int(slots[-1]) >= cs or int(slots.min()) < 0 or int(slots.max()) >= cs):
        raise StateError(f"{where}: array 'buffer_delta_slots' holds a slot outside [0, {cs})")
    if n > 1 and not bool(np.all(np.diff(slots) > 0)):
        raise StateError(f"{where}: array 'buffer_delta_slots' is not strictly ascending")
    grown = np.arange(cs0, cs, dtype=np.int64)
    if grown.size and not np.array_equal(slots[slots >= cs0], grown):
        raise StateError(f"{where}: array 'buffer_delta_slots' does not list every slot of the grown region [{cs0}, {cs})")


def compose(base_path, delta_path_, sums=True):
    """Base + delta -> (arrays, manifest) of the full state taken at the delta's instant, as `read_state` returns one.  Pure
    numpy.  Refused, naming the array or field: a base that is a delta or has no lineage, a lineage / capture_epoch / current_size /
    buffer sum of the base that is not what the delta cites, any delta array that does not sum to its manifest entry, a slot list
    that is not strictly ascending inside [0, current_size) or misses part of the grown region."""
    base_where, where = os.fspath(base_path), os.fspath(delta_path_)
    arrays, manifest = read_state(where)
    if not is_delta(manifest):
        raise StateError(f"{where}: manifest 'kind' is not 'delta'")
    b_arrays, b_manifest = read_state(base_where)
    key, cited = base_key(b_manifest, where=base_where), manifest["base"]
    off = cites(manifest, b_manifest, where=base_where)
    if off in BUFFER_ARRAYS:
        raise StateError(f"{base_where}: array '{off}' of the base sums to {tuple(key['sums'][off])}, the delta {where} cites "
                         f"{tuple(cited['sums'][off])}: not the state this delta was taken against")
    if off is not None:
        raise StateError(f"{base_where}: '{off}' of the base is {key[off]!r}, the delta {where} cites {cited[off]!r}")
    for f in ("obs", "goal", "action", "hidden", "T", "capacity"):
        if int(b_manifest["dims"][f]) != int(manifest["dims"][f]):
            raise StateError(f"{base_where}: {f} of the base is {b_manifest['dims'][f]}, of the delta {manifest['dims'][f]}")
    want0 = expected_shapes(b_manifest["dims"])      # the base's rows are what its manifest (and so the delta) says
    _check_listed(b_arrays, b_manifest, sums, base_where, {name: want0[name] for name in BUFFER_ARRAYS})
    check_delta_arrays(arrays, manifest, sums=sums, where=where)
    dims, cs0 = manifest["dims"], key["current_size"]
    want, slots = expected_shapes(dims), arrays["buffer_delta_slots"]
    out = {k: v for k, v in arrays.items() if not k.startswith("buffer_delta_")}
    listed = {k: v for k, v in manifest["arrays"].items() if not k.startswith("buffer_delta_")}
    for name, rows in zip(BUFFER_ARRAYS, DELTA_ROW_ARRAYS):
        dt, shape = want[name]
        full = np.empty(shape, dt)
        full[:cs0] = b_arrays[name]
        full[slots] = arrays[rows]
        out[name] = full
        listed[name] = {"dtype": dt, "shape": list(shape), "sum": list(checksum(full))}
    composed = {k: v for k, v in manifest.items() if k not in ("kind", "base", "n_dirty", "arrays", "format")}
    composed.update({"format": FORMAT_VERSION, "arrays": listed})
    ordered = {name: out[name] for name in DEVICE_ARRAYS}
    ordered.update({k: v for k, v in out.items() if k not in ordered})
    return ordered, composed


def flatten(base_path, delta_path_, out_path):
    """Write compose(base, delta) as a full state: what save_training_state(out_path) would have written at the delta's instant
    (it keeps the delta's lineage and capture_epoch, so it can serve as a base where the delta was loaded)."""
    arrays, manifest = compose(base_path, delta_path_)
    return write_state(out_path, arrays, manifest)


def default_base(path, manifest):
    """The base a delta names, taken beside the delta."""
    return os.path.join(os.path.dirname(os.fspath(path)), manifest["base"]["name"])


def verify(path, base=None):
    """Check a state file without a GPU; returns its manifest.  A delta is checked together with its base (default: the name its
    manifest records, beside it)."""
    arrays, manifest = read_state(path)
    if is_delta(manifest):
        compose(base or default_base(path, manifest), path)
        return manifest
    check_arrays(arrays, manifest, sums=True, where=os.fspath(path))
    return manifest


def rank_path(path, rank):
    """`state.npz` -> `state_rank3.npz`: every rank of a data-parallel run keeps its own file (its buffer is its episode shard)."""
    root, ext = os.path.splitext(os.fspath(path))
    return f"{root}_rank{int(rank)}{ext}"


# ---------------------------------------------------------------------------------------------------- device side
def _dims_of(agent, current_size):
    ep = agent.env_params
    return {"obs": int(ep["obs"]), "goal": int(ep["goal"]), "action": int(ep["action"]),
            "hidden": int(ep.get("hidden", 256)),     # the width ddpg_agent gave hp_agent_create
            "T": int(agent.buffer._dev.T), "capacity": int(agent.buffer._dev.size), "current_size": int(current_size)}


def _layout(agent, n=-1, delta=False):
    """([(name, dtype, count, offset) of every section], blob bytes) as the library lays out a full state of n episodes (-1: the
    buffer's current_size) or (delta=True) a delta with room for n dirty episodes."""
    from . import _lib
    room = _lib.STATE_DELTA_SECTIONS if delta else _lib.STATE_SECTIONS
    entry = agent.lib.hp_state_layout_delta if delta else agent.lib.hp_state_layout
    secs, count, total = (_lib.StateSection * room)(), C.c_int32(room), C.c_size_t()
    _lib.check(entry(agent.h, agent.buffer._dev.h, agent.o_norm.h, agent.g_norm.h, int(n), secs, C.byref(count), C.byref(total)))
    return [(s.name.decode(), _DTYPES[s.dtype], int(s.count), int(s.offset)) for s in secs[:count.value]], int(total.value)


def _buffer_counts(agent):
    """(current_size, episodes stored so far) from the buffer's host mirror: no wait."""
    cs, nts, T = C.c_int64(), C.c_int64(), C.c_int32()
    from . import _lib
    _lib.check(agent.lib.hp_buffer_info(agent.buffer._dev.h, None, C.byref(cs), C.byref(nts), C.byref(T)))
    return int(cs.value), int(nts.value) // int(T.value)


def _epochs(agent):
    """(capture_epoch of the agent's latest capture, the buffer's epoch, min_since)."""
    from . import _lib
    c, e, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _lib.check(agent.lib.hp_state_epochs(agent.h, agent.buffer._dev.h, C.byref(c), C.byref(e), C.byref(m)))
    return int(c.value), int(e.value), int(m.value)


def _known(agent):
    """Full states this process saved from or loaded into `agent`, as delta bases: key -> (since_epoch of the buffer in THIS
    process, episodes stored when it was captured)."""
    if not hasattr(agent, "_state_known"):
        agent._state_known, agent._state_lineage = {}, None
    return agent._state_known


def _lineage(agent, listed):
    """The run's 64-bit id: made at an agent's first save, kept from then on and across resumes (load() takes the file's).  It is
    a hash of that first state's checksums -- as good as random between runs, while two runs that are bit-identical agree, so
    their files still compare equal."""
    _known(agent)
    if agent._state_lineage is None:
        text = json.dumps([int(agent.comm.rank), sorted((k, v["sum"]) for k, v in listed.items())])
        agent._state_lineage = hashlib.sha256(text.encode()).hexdigest()[:16]
    return agent._state_lineage


def known_base(agent, base_path):
    """(key, since_epoch, episodes) of the full state at base_path if a delta can be taken against it now; StateError otherwise:
    not a full state with a lineage, not saved or loaded by this agent in this process, or older than the last restore."""
    where = os.fspath(base_path)
    key = base_key(read_manifest(where), where=where)
    rec = _known(agent).get(_key_tuple(key))
    if rec is None:
        raise StateError(f"{where}: 'lineage' {key['lineage']} / 'capture_epoch' {key['capture_epoch']} is not a state this agent "
                         "saved or loaded in this process: which rows changed since it is not known (save a full state first)")
    if rec[0] < _epochs(agent)[2]:
        raise StateError(f"{where}: 'capture_epoch' {key['capture_epoch']} is older than the load_training_state done since: which "
                         "rows changed since it is not known any more (save a full state first)")
    return key, rec[0], rec[1]


class PendingSave:
    """A capture in flight (`save_training_state(wait=False)`): the device part was snapshotted in stream order when this object
    was made, the host part (numpy's stream, success_rates, savetime) copied at the same moment; training may go on.
    `.result()` waits for the drain, writes the file and returns its path.  While it is outstanding a second capture on the same
    agent raises (HP_ERR_STATE).  base = the path of a full state this agent saved or loaded: a delta against it."""

    def __init__(self, agent, path, extra=None, epoch=0, cycle=0, base=None):
        from . import _lib
        self.agent, self.path, self._done, self.base = agent, os.fspath(path), None, None
        if base is not None:       # refused before anything is captured
            key, since, episodes0 = known_base(agent, base)
            self.base = dict(key, name=os.path.basename(os.fspath(base)))
        agent._flush_updates()
        ticket, nbytes = C.c_uint64(), C.c_size_t()
        cs, self.episodes = _buffer_counts(agent)
        if base is None:
            _lib.check(agent.lib.hp_state_capture(*agent._handles(), C.byref(ticket), C.byref(nbytes)))
            # (no library call that stores between the capture and this: the buffer's size is the captured one)
            self.sections, total = _layout(agent, -1)
        else:
            self.max_dirty = min(self.episodes - episodes0, cs)
            _lib.check(agent.lib.hp_state_capture_delta(*agent._handles(), since, self.max_dirty, C.byref(ticket), C.byref(nbytes)))
            self.sections, total = _layout(agent, self.max_dirty, delta=True)
        self.ticket, self.nbytes = ticket.value, nbytes.value
        assert total == self.nbytes, (total, self.nbytes)
        self.capture_epoch = _epochs(agent)[0]
        st = np.random.get_state()
        gauss = agent.rng._gauss
        self.host = {"np_random": {"pos": int(st[2]), "has_gauss": int(st[3]), "cached_gaussian": float(st[4])},
                     "rng_gauss": [int(gauss[0]), float(gauss[1])], "savetime": int(agent.savetime), "epoch": int(epoch),
                     "cycle": int(cycle)}
        self.host_arrays = {"np_random_key": np.array(st[1], dtype=np.uint32),
                            "success_rates": np.array(agent.success_rates, dtype=np.float64),
                            "extra": np.frombuffer(bytes(extra or b""), dtype=np.uint8).copy()}
        for family, fam in STREAM_FAMILIES.items():
            streams = fam["find"](agent)
            if streams is not None:
                # copied now (a few KB per stream; synchronises), so rollouts that follow a wait=False capture do not move them
                stream_arrays, self.host[fam["field"]] = stream_record(*streams.get_arrays(), family=family)
                self.host_arrays.update(stream_arrays)

    def done(self):
        return self._done is not None

    def result(self):
        if self._done is not None:
            return self._done
        from . import _lib
        agent, delta = self.agent, self.base is not None
        blob = np.empty(self.nbytes, np.uint8)
        sums = (C.c_uint64 * (2 * len(self.sections)))()
        done = C.c_int32()
        fetch = object.__getattribute__(agent.lib, "_cdll").hp_state_fetch      # no flush of deferred updates in front of a wait
        try:
            _lib.check(fetch(agent.h, self.ticket, 1, blob.ctypes.data_as(C.c_void_p), blob.size, sums, C.byref(done)))
        except ValueError as e:
            raise StateError(f"save: {e}") from e
        offs = {n: o for n, _, _, o in self.sections}
        cs = int(blob[offs["buffer_counters"]:offs["buffer_counters"] + 8].view("<i8")[0])
        dims = _dims_of(agent, cs)
        want = expected_shapes(dims)
        n_dirty = 0
        if delta:
            n_dirty, overflow, cap, _ = (int(x) for x in blob[offs["buffer_delta_header"]:offs["buffer_delta_header"] + 32].view("<i8"))
            if overflow or n_dirty > self.max_dirty or cap != self.capture_epoch:
                raise StateError(f"save: array 'buffer_delta_header' says n_dirty {n_dirty}, overflow {overflow}, capture_epoch {cap}; "
                                 f"the host sized the delta for {self.max_dirty} episodes at capture_epoch {self.capture_epoch}")
            want.update(delta_shapes(dims, n_dirty))
        arrays, listed = {}, {}
        for i, (name, dt, count, off) in enumerate(self.sections):
            dev = (int(sums[2 * i]), int(sums[2 * i + 1]))
            used = int(np.prod(want[name][1])) if name in want else count     # a delta's slot / row sections: the used prefix
            a = blob[off:off + used * np.dtype(dt).itemsize].view(dt)
            if checksum(a) != dev:      # what left the device is what the device summed
                raise StateError(f"save: array '{name}' arrived with sums {checksum(a)}, the device computed {dev}")
            if name == "buffer_delta_header":
                continue                # its fields go into the manifest
            arrays[name] = a.reshape(want[name][1])
            listed[name] = {"dtype": dt, "shape": list(arrays[name].shape), "sum": [dev[0], dev[1]]}
        manifest = {"format": FORMAT_VERSION, "dims": dims, "rank": int(agent.comm.rank), "world_size": int(agent.comm.world_size),
                    "abi": int(_lib.ABI_VERSION), "arrays": listed, "lineage": _lineage(agent, listed), "capture_epoch": self.capture_epoch,
                    **self.host}
        if delta:
            manifest.update({"format": DELTA_FORMAT_VERSION, "kind": "delta", "n_dirty": n_dirty, "base": self.base})
            rows = sum(arrays[n].nbytes for n in DELTA_ROW_ARRAYS)
            per_ep = 8 * ((dims["T"] + 1) * (dims["obs"] + dims["goal"]) + dims["T"] * (dims["goal"] + dims["action"]))
            assert rows == n_dirty * per_ep, (rows, n_dirty, per_ep)
        arrays.update(self.host_arrays)
        self._done = write_state(self.path, arrays, manifest)
        if not delta:                   # from now on a delta can be taken against this file
            _known(agent)[_key_tuple(base_key(manifest))] = (self.capture_epoch, self.episodes)
        return self._done


def save(agent, path, wait=True, extra=None, epoch=0, cycle=0, base=None):
    h = PendingSave(agent, path, extra=extra, epoch=epoch, cycle=cycle, base=base)
    return h.result() if wait else h


def load(agent, path, verify_host=False, base=None):
    """Restore `agent` (its networks, optimizers, normalizers, random stream and replay buffer) and the host side of the run
    from a state file; returns (extra bytes, manifest).  A file that does not fit the agent -- dims, capacity, T, rank, world size
    -- or whose bytes do not sum on the DEVICE to what the manifest records is refused before anything is changed.  A delta is
    composed with its base first (`base`, default: the name the delta records, beside it), on the host, and then restored like
    the full state it stands for."""
    from . import _lib
    where = os.fspath(path)
    manifest = read_manifest(where)
    if is_delta(manifest):
        arrays, manifest = compose(base or default_base(where, manifest), where, sums=True)
    else:
        arrays, manifest = read_state(path)
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
    live = {}                           # family -> the agent's streams that the state will be put into
    for family, fam in STREAM_FAMILIES.items():
        streams, rec = fam["find"](agent), manifest.get(fam["field"])
        names = ", ".join(f"'{n}'" for n in fam["arrays"])
        if streams is not None and rec is None:
            raise StateError(f"{where}: " + fam["saved_without"].format(names=names))
        if streams is None and rec is not None:
            raise StateError(f"{where}: " + fam["agent_without"].format(n=rec["n"], names=names))
        if streams is not None and int(rec["n"]) != len(streams):
            raise StateError(f"{where}: array '{family}_stream_keys' holds {rec['n']} streams, the agent has {len(streams)} environments")
        if streams is not None:
            live[family] = streams
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
    # Delta bases: the stamps started over, so every state this agent knew is now older than the restore (known_base says so);
    # the state just loaded (a full file, or the full state a delta stands for -- `flatten` writes that one out) is known from here
    # on, and the run keeps its lineage
    known = _known(agent)
    if "lineage" in manifest and "capture_epoch" in manifest:
        agent._state_lineage = str(manifest["lineage"])
        known[_key_tuple(base_key(manifest))] = (_epochs(agent)[2], _buffer_counts(agent)[1])
    # host side of the run
    r = manifest["np_random"]
    np.random.set_state(("MT19937", arrays["np_random_key"], int(r["pos"]), int(r["has_gauss"]), float(r["cached_gaussian"])))
    agent.rng.seeded = True
    agent.rng._gauss = (int(manifest["rng_gauss"][0]), float(manifest["rng_gauss"][1]))
    for family, streams in live.items():
        streams.set_arrays(*(arrays[n] for n in STREAM_FAMILIES[family]["arrays"]))
    agent.success_rates = [float(x) for x in arrays["success_rates"]]
    agent.savetime = int(manifest["savetime"])
    return arrays["extra"].tobytes(), manifest


_USAGE = ("usage: python -m rl_arm_under_sparse_reward_amd.train_state verify FILE [--base BASE]\n"
          "       python -m rl_arm_under_sparse_reward_amd.train_state flatten BASE DELTA OUT")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    base = None
    if len(argv) == 4 and argv[0] == "verify" and argv[2] == "--base":
        base, argv = argv[3], argv[:2]
    if not ((len(argv) == 2 and argv[0] == "verify") or (len(argv) == 4 and argv[0] == "flatten")):
        print(_USAGE, file=sys.stderr)
        return 2
    try:
        if argv[0] == "flatten":
            flatten(argv[1], argv[2], argv[3])
            m, what = verify(argv[3]), f"{argv[3]} = {argv[1]} + {argv[2]}"
        else:
            m, what = verify(argv[1], base=base), argv[1]
    except StateError as e:
        print(f"FAILED: {e}", file=sys.stderr)
        return 1
    d = m["dims"]
    kind = f"delta of {m['n_dirty']} episodes over {base or m['base']['name']}, " if is_delta(m) else ""
    print(f"ok: {what}: format {m['format']}, {kind}rank {m['rank']}/{m['world_size']}, epoch {m['epoch']}, "
          f"{d['current_size']}/{d['capacity']} episodes of T={d['T']}, obs/goal/action {d['obs']}/{d['goal']}/{d['action']}, "
          f"{len(m['arrays'])} arrays verified")
    return 0


if __name__ == "__main__":
    sys.exit(main())
