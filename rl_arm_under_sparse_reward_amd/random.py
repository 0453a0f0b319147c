"""Device-resident twin of numpy's legacy *global* RandomState.

The reference draws every sampled index from the process-global `np.random`
(her.py:24-31, replay_buffer.py:64,67), seeded with `seed + rank` (train.py:36).  Here
the stream lives in HBM next to the kernels that consume it; this module mirrors the
numpy calls a reference-style script uses to control it:

    seed(s)          <-> np.random.seed(s)
    advance(n)       <-> np.random.bytes(4 * n), thrown away (jump-ahead: no walk to the new position)
    get_state()      <-> np.random.get_state()      (same 5-tuple)
    set_state(st)    <-> np.random.set_state(st)

so a script can hand the stream back and forth, e.g. `random.set_state(np.random.get_state())`
before the learner phase and `np.random.set_state(random.get_state())` after it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def legacy_state(state):
    """numpy's legacy state tuple (3 or 5 fields; numpy accepts the 3-tuple too) -> (key uint32 [624], pos, has_gauss, gauss);
    the two refusals carry numpy's messages."""
    if state[0] != "MT19937":
        raise ValueError("set_state can only be used with legacy MT19937 state instances.")
    key = np.ascontiguousarray(state[1], dtype=np.uint32)
    if key.shape != (624,):
        raise ValueError("state must be 624 longs")
    has, val = (int(state[3]), float(state[4])) if len(state) >= 5 else (0, 0.0)
    return key, int(state[2]), has, val


class DeviceRandomState:
    def __init__(self, seed=None, ctx=None):
        self.ctx = ctx or _lib.Context.default()
        self.lib = self.ctx.lib
        self.h = C.c_void_p()
        _lib.check(self.lib.hp_rng_create(self.ctx.h, C.byref(self.h)))
        self.seeded = False       # seed() / set_state() called (a fresh stream carries numpy's default key, seed 5489)
        # numpy's legacy state also carries a cached Gaussian (has_gauss, cached_gaussian).  It lives on the device next to
        # (key, pos), where the normal draws of the exploration noise (csrc/mt19937_wave.h) read and write it; randint /
        # random_sample never touch it, in numpy either.  `_gauss` is a view of it; the host copy below is reused until a
        # device draw of normals may have changed it (`_gauss_stale`), so reading it costs no device round trip otherwise
        self._gauss_host, self._gauss_stale = (0, 0.0), False
        if seed is not None:
            self.seed(seed)

    def seed(self, seed):
        seed = int(seed)
        if not 0 <= seed <= 2**32 - 1:
            raise ValueError("Seed must be between 0 and 2**32 - 1")     # numpy's message
        _lib.check(self.lib.hp_rng_seed(self.h, C.c_uint32(seed)))
        self.seeded = True
        self._gauss_host, self._gauss_stale = (0, 0.0), False            # numpy's seed() drops the cached normal (hp_rng_seed too)

    @property
    def _gauss(self):
        """(has_gauss, cached_gaussian) of the device stream (hp_rng_get_gauss; synchronises only after a device draw of normals)."""
        if self._gauss_stale:
            has, val = C.c_int32(), C.c_double()
            _lib.check(self.lib.hp_rng_get_gauss(self.h, C.byref(has), C.byref(val)))
            self._gauss_host, self._gauss_stale = (int(has.value), float(val.value)), False
        return self._gauss_host

    @_gauss.setter
    def _gauss(self, gauss):
        gauss = (int(gauss[0]), float(gauss[1]))
        _lib.check(self.lib.hp_rng_set_gauss(self.h, C.c_int32(gauss[0]), C.c_double(gauss[1])))
        self._gauss_host, self._gauss_stale = (1 if gauss[0] else 0, gauss[1]), False

    def mark_normals_drawn(self):
        """A device kernel drew normals from this stream (rollout steps with exploration): the cached Gaussian must be read back."""
        self._gauss_stale = True

    def get_state(self):
        key = np.empty(624, np.uint32)
        pos = C.c_int32()
        _lib.check(self.lib.hp_rng_get_state(self.h, _lib.ptr(key, C.c_uint32), C.byref(pos)))
        gauss = self._gauss
        return ("MT19937", key, int(pos.value), int(gauss[0]), float(gauss[1]))

    def set_state(self, state):
        if isinstance(state, dict):     # numpy's dict form: its bit generator is not named by field 0 of a tuple
            state = ("MT19937", state["state"]["key"], state["state"]["pos"], state.get("has_gauss", 0), state.get("gauss", 0.0))
        key, pos, has, val = legacy_state(state)
        _lib.check(self.lib.hp_rng_set_state(self.h, _lib.ptr(key, C.c_uint32), C.c_int32(pos)))
        self.seeded = True
        self._gauss = (has, val)

    def advance(self, n_words):
        """Skip `n_words` 32-bit words as if they had been drawn and thrown away (hp_rng_advance): the state afterwards is
        numpy's after `bytes(4 * n_words)`, reached by jump-ahead instead of by generating the words."""
        n_words = int(n_words)
        if n_words < 0:
            raise ValueError("advance: n_words must be non-negative")
        _lib.check(self.lib.hp_rng_advance(self.h, C.c_uint64(n_words)))

    def set_parallel(self, min_batch=None):
        """hp_rng_set_parallel: sampler index draws of at least `min_batch` transitions take the parallel form of the reference's
        draw (None: the library's measured crossover; 0: off).  Same stream, same indices, same state afterwards."""
        if min_batch is None:
            min_batch = _lib.PARALLEL_DRAW_MIN_BATCH
        _lib.check(self.lib.hp_rng_set_parallel(self.h, C.c_int64(int(min_batch))))

    def parallel_info(self):
        """(min_batch, n_parallel, n_fallback): the threshold in force (0 = off) and how many sampler draws the parallel kernels
        committed / the sequential kernel behind them did (hp_rng_parallel_info; synchronises)."""
        m, p, f = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.lib.hp_rng_parallel_info(self.h, C.byref(m), C.byref(p), C.byref(f)))
        return m.value, p.value, f.value

    # test hooks: the two primitive draws of the hot path, executed on the device
    def randint(self, low, high=None, size=1):
        if high is None:
            low, high = 0, low
        out = np.empty(int(size), np.int64)
        _lib.check(self.lib.hp_rng_randint(self.h, int(low), int(high), int(size), _lib.ptr(out, C.c_int64)))
        return out

    def uniform(self, size=1):
        out = np.empty(int(size), np.float64)
        _lib.check(self.lib.hp_rng_uniform(self.h, int(size), _lib.ptr(out, C.c_double)))
        return out

    def standard_normal(self, size=1):
        """np.random.randn(size) on the device (legacy polar method, cached second normal included)."""
        out = np.empty(int(size), np.float64)
        _lib.check(self.lib.hp_rng_standard_normal(self.h, int(size), _lib.ptr(out, C.c_double)))
        self._gauss_stale = True
        return out

    def binomial1(self, p, size=1):
        """np.random.binomial(1, p, size) on the device (legacy inversion)."""
        from .device_env import binomial1_qn
        out = np.empty(int(size), np.int64)
        _lib.check(self.lib.hp_rng_binomial1(self.h, float(p), binomial1_qn(p)[0], int(size), _lib.ptr(out, C.c_int64)))
        return out

    def __del__(self):
        try:
            self.lib.hp_rng_destroy(self.h)
        except Exception:
            pass


class DeviceRandomStreams:
    """n device random streams, one per environment of a vectorised simulator (csrc/rng_streams.hip): stream i is
    `np.random.RandomState(seeds[i])`, by default `RandomState(base_seed + i)` -- the reference's `seed + rank` (train.py:34-39)
    with an environment where the reference has a rank.  States are numpy's `get_state()` 5-tuples, cached normal included.
    `ddpg_agent.enable_explore_streams` hands one of these to the rollout steps (hp_rollout_step_streams)."""

    def __init__(self, n, seeds=None, base_seed=None, ctx=None):
        self.ctx = ctx or _lib.Context.default()
        self.lib = self.ctx.lib
        self.n = int(n)
        self.h = C.c_void_p()
        _lib.check(self.lib.hp_streams_create(self.ctx.h, C.c_int64(self.n), C.byref(self.h)))
        if seeds is not None or base_seed is not None:
            self.seed(seeds=seeds, base_seed=base_seed)

    def __len__(self):
        return self.n

    def seed(self, seeds=None, base_seed=None):
        """Stream i := RandomState(seeds[i]), or RandomState(base_seed + i); cached normals are dropped, as numpy's seed() does."""
        if (seeds is None) == (base_seed is None):
            raise ValueError("seed: give either a list of seeds or a base seed")
        if seeds is None:
            base = int(base_seed)
            if not (0 <= base and base + self.n - 1 <= 2**32 - 1):
                raise ValueError("Seed must be between 0 and 2**32 - 1")     # numpy's message
            _lib.check(self.lib.hp_streams_seed(self.h, None, C.c_int64(self.n), C.c_uint32(base)))
            return
        wide = np.asarray(seeds, dtype=np.int64).reshape(-1)
        if wide.size and (wide.min() < 0 or wide.max() > 2**32 - 1):
            raise ValueError("Seed must be between 0 and 2**32 - 1")
        arr = np.ascontiguousarray(wide, dtype=np.uint32)
        # (a list of the wrong length is the library's error to name)
        _lib.check(self.lib.hp_streams_seed(self.h, _lib.ptr(arr, C.c_uint32), C.c_int64(arr.size), C.c_uint32(0)))

    def get_state(self, i):
        key = np.empty(624, np.uint32)
        pos, has, val = C.c_int32(), C.c_int32(), C.c_double()
        _lib.check(self.lib.hp_streams_get_state(self.h, C.c_int64(int(i)), _lib.ptr(key, C.c_uint32), C.byref(pos), C.byref(has),
                                                 C.byref(val)))
        return ("MT19937", key, int(pos.value), int(has.value), float(val.value))

    def set_state(self, i, state):
        key, pos, has, val = legacy_state(state)
        _lib.check(self.lib.hp_streams_set_state(self.h, C.c_int64(int(i)), _lib.ptr(key, C.c_uint32), C.c_int32(pos), C.c_int32(has),
                                                 C.c_double(val)))

    def get_arrays(self):
        """All states as four arrays: keys uint32 [n, 624], pos int32 [n], has_gauss int32 [n], gauss float64 [n] (what a
        training state stores)."""
        keys, pos = np.empty((self.n, 624), np.uint32), np.empty(self.n, np.int32)
        has, val = np.empty(self.n, np.int32), np.empty(self.n, np.float64)
        _lib.check(self.lib.hp_streams_get_all(self.h, _lib.ptr(keys, C.c_uint32), _lib.ptr(pos, C.c_int32), _lib.ptr(has, C.c_int32),
                                               _lib.ptr(val, C.c_double)))
        return keys, pos, has, val

    def set_arrays(self, keys, pos, has_gauss, gauss):
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        pos, has = np.ascontiguousarray(pos, dtype=np.int32).reshape(-1), np.ascontiguousarray(has_gauss, dtype=np.int32).reshape(-1)
        val = np.ascontiguousarray(gauss, dtype=np.float64).reshape(-1)
        if keys.shape != (self.n, 624) or not (pos.size == has.size == val.size == self.n):
            raise ValueError(f"set_arrays: {self.n} streams need keys [{self.n}, 624] and {self.n} positions / cached normals")
        _lib.check(self.lib.hp_streams_set_all(self.h, _lib.ptr(keys, C.c_uint32), _lib.ptr(pos, C.c_int32), _lib.ptr(has, C.c_int32),
                                               _lib.ptr(val, C.c_double)))

    def get_states(self):
        keys, pos, has, val = self.get_arrays()
        return [("MT19937", keys[i].copy(), int(pos[i]), int(has[i]), float(val[i])) for i in range(self.n)]

    def set_states(self, states):
        states = list(states)
        if len(states) != self.n:
            raise ValueError(f"set_states: {len(states)} states for {self.n} streams")
        self.set_arrays(np.stack([np.asarray(s[1], dtype=np.uint32) for s in states]), [s[2] for s in states],
                        [s[3] if len(s) >= 5 else 0 for s in states], [s[4] if len(s) >= 5 else 0.0 for s in states])

    def __del__(self):
        try:
            self.lib.hp_streams_destroy(self.h)
        except Exception:
            pass


_global = None


def global_state() -> DeviceRandomState:
    """The process-global stream (created on first use), like numpy's `np.random` singleton."""
    global _global
    if _global is None:
        _global = DeviceRandomState()
    return _global


def seed(s):
    global_state().seed(s)


def get_state():
    return global_state().get_state()


def set_state(state):
    global_state().set_state(state)
