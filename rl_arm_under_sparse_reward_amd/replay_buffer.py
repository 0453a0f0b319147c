"""replay_buffer -- drop-in mirror of the reference's replay_buffer.py with storage in HBM.

    replay_buffer(env_params, buffer_size, sample_func)
    .store_episode([mb_obs, mb_ag, mb_g, mb_actions])
    .sample(batch_size) -> dict of ndarrays
    attrs: size, T, current_size, n_transitions_stored, buffers

(replay_buffer.py:10-71).  `sample_func` must be the bound `sample_her_transitions` of this
package's her_sampler (that is what ddpg_agent.py:47 passes); its parameters select the
device kernel.  Arbitrary Python sample functions are refused: there is no host path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import random as _random

_WHICH = {"obs": 0, "ag": 1, "g": 2, "actions": 3}


class DeviceEpisodeBuffer:
    """Thin owner of one hp_buffer handle (float64 episodes in HBM)."""

    def __init__(self, size_episodes, T, obs_dim, goal_dim, act_dim, ctx=None):
        self.ctx = ctx or _lib.Context.default()
        self.lib = self.ctx.lib
        self.h = C.c_void_p()
        self.size, self.T = int(size_episodes), int(T)
        self.dims = {"obs": int(obs_dim), "ag": int(goal_dim), "g": int(goal_dim), "actions": int(act_dim)}
        _lib.check(self.lib.hp_buffer_create(self.ctx.h, self.size, self.T, obs_dim, goal_dim, act_dim,
                                             C.byref(self.h)))

    def info(self):
        s, c, n, t = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(self.lib.hp_buffer_info(self.h, C.byref(s), C.byref(c), C.byref(n), C.byref(t)))
        return s.value, c.value, n.value, t.value

    def _checked(self, episode_batch):
        """float64 C-contiguous views of the four episode arrays, shapes validated like numpy's broadcast would
        (replay_buffer.py:39-42 raises ValueError on a wrong T or dimension)."""
        if len(episode_batch) != 4:
            raise ValueError("episode_batch must be [mb_obs, mb_ag, mb_g, mb_actions]")
        obs, ag, g, act = (_lib.as_f64(a) for a in episode_batch)
        n = obs.shape[0] if obs.ndim else 0
        T = self.T
        want = {"obs": (n, T + 1, self.dims["obs"]), "ag": (n, T + 1, self.dims["ag"]),
                "g": (n, T, self.dims["g"]), "actions": (n, T, self.dims["actions"])}
        for name, a in (("obs", obs), ("ag", ag), ("g", g), ("actions", act)):
            if a.shape != want[name]:
                raise ValueError(f"could not broadcast input array from shape {a.shape} into shape {want[name]}")
        return obs, ag, g, act, n

    def store(self, rng, episode_batch):
        obs, ag, g, act, n = self._checked(episode_batch)
        d = C.c_double
        _lib.check(self.lib.hp_buffer_store(self.h, rng.h, _lib.ptr(obs, d), _lib.ptr(ag, d), _lib.ptr(g, d),
                                            _lib.ptr(act, d), n))
        return n

    def stage(self, episode_batch):
        """Upload episodes into the device staging area without storing them (the temporary dict of
        ddpg_agent._update_normalizer, ddpg_agent.py:187-203)."""
        obs, ag, g, act, n = self._checked(episode_batch)
        d = C.c_double
        _lib.check(self.lib.hp_buffer_stage(self.h, _lib.ptr(obs, d), _lib.ptr(ag, d), _lib.ptr(g, d),
                                            _lib.ptr(act, d), n))
        return n

    def last_slots(self, n):
        out = np.empty(n, np.int64)
        _lib.check(self.lib.hp_buffer_last_slots(self.h, _lib.ptr(out, C.c_int64), n))
        return out

    def read(self, key, first=0, n=None):
        n = self.size - first if n is None else n
        steps = self.T + 1 if key in ("obs", "ag") else self.T
        out = np.empty((n, steps, self.dims[key]), np.float64)
        _lib.check(self.lib.hp_buffer_read(self.h, _WHICH[key], first, n, _lib.ptr(out, C.c_double)))
        return out

    def sample(self, rng, batch, future_p, sq_threshold, with_indices=False):
        B = int(batch)
        od, gd, ad = self.dims["obs"], self.dims["g"], self.dims["actions"]
        tr = {"obs": np.empty((B, od)), "ag": np.empty((B, gd)), "g": np.empty((B, gd)),
              "actions": np.empty((B, ad)), "obs_next": np.empty((B, od)), "ag_next": np.empty((B, gd))}
        r = np.empty((B, 1), np.float32)
        o = _lib.SampleOut()
        for k, a in tr.items():
            setattr(o, k, _lib.ptr(a, C.c_double))
        o.r = _lib.ptr(r, C.c_float)
        dense = float(sq_threshold) < 0
        r64 = np.empty((B, 1), np.float64) if dense else None
        if dense:
            o.r64 = _lib.ptr(r64, C.c_double)
        idx = None
        if with_indices:
            idx = {"e": np.empty(B, np.int64), "t": np.empty(B, np.int64), "future_t": np.empty(B, np.int64),
                   "her": np.empty(B, np.uint8)}
            o.e, o.t, o.future_t = (_lib.ptr(idx[k], C.c_int64) for k in ("e", "t", "future_t"))
            o.her = _lib.ptr(idx["her"], C.c_uint8)
        _lib.check(self.lib.hp_buffer_sample(self.h, rng.h, B, float(future_p), float(sq_threshold), C.byref(o)))
        # her.py:38 expand_dims(reward_func(...), 1): float32 for the sparse reward; the dense branch of compute_reward
        # returns -d in float64 (:89-90), computed by the same kernel (r holds its float32 narrowing, the learner's input)
        tr["r"] = r64 if dense else r
        if with_indices:
            idx["her"] = idx["her"].astype(bool)
            return tr, idx
        return tr

    def enable_f32_rows(self):
        """hp_buffer_enable_f32_rows: build (and from now on maintain) the float32 throughput mirror that
        `sample_device(..., f32_rows=True)` reads.  The float64 arrays stay the source of truth."""
        _lib.check(self.lib.hp_buffer_enable_f32_rows(self.h))
        self.f32_rows = True

    def sample_device(self, rng, o_norm, g_norm, batch, future_p, sq_threshold, clip_obs, with_indices=False, f32_rows=False, fast=None):
        """hp_buffer_sample_dev: the minibatch as the learner consumes it (ddpg_agent.py:227-243) in torch CUDA tensors
        allocated here: x, x_next [B, obs+goal], actions [B, act], r [B, 1], float32.  The kernels run on TORCH's current stream,
        which the context borrows for this call (_lib.Context.torch_bridge: behind what the context's own stream held; the own
        stream catches up when it is next used): the context is not rebound, so a fused learner on the same context keeps
        replaying its cached graphs, and no host synchronisation happens.  The context's lock is held while the call runs, so
        another thread's library call on this context (a feeder's store) waits for it."""
        import torch

        B = int(batch)
        dev = torch.device("cuda", self.ctx.device_id)
        ldx = self.dims["obs"] + self.dims["g"]
        out = {"x": torch.empty((B, ldx), dtype=torch.float32, device=dev),
               "x_next": torch.empty((B, ldx), dtype=torch.float32, device=dev),
               "actions": torch.empty((B, self.dims["actions"]), dtype=torch.float32, device=dev),
               "r": torch.empty((B, 1), dtype=torch.float32, device=dev)}
        o = _lib.SampleDevOut()
        for k, t in out.items():
            setattr(o, k, t.data_ptr())
        idx = None
        if with_indices:
            idx = {k: torch.empty(B, dtype=torch.int64, device=dev) for k in ("e", "t", "future_t")}
            idx["her"] = torch.empty(B, dtype=torch.uint8, device=dev)
            for k, t in idx.items():
                setattr(o, k, t.data_ptr())
        fn = self.lib.hp_buffer_sample_dev_f32 if f32_rows else self.lib.hp_buffer_sample_dev
        with self.ctx.torch_bridge():
            if fast is not None:     # (seed, call): counter-based index draw inside the gather kernel, no hp_rng (hp_buffer_sample_dev_fast)
                _lib.check(self.lib.hp_buffer_sample_dev_fast(self.h, o_norm.h, g_norm.h, B, float(future_p), float(sq_threshold),
                                                              float(clip_obs), int(fast[0]), int(fast[1]), 1 if f32_rows else 0, C.byref(o)))
            else:
                _lib.check(fn(self.h, rng.h, o_norm.h, g_norm.h, B, float(future_p), float(sq_threshold), float(clip_obs), C.byref(o)))
        return (out, idx) if with_indices else out

    def __del__(self):
        try:
            self.lib.hp_buffer_destroy(self.h)
        except Exception:
            pass


class _BuffersView:
    """`replay_buffer.buffers` in the reference is a dict of numpy arrays; here it is a read-only
    view that copies the requested array back from HBM."""

    def __init__(self, dev):
        self._dev = dev

    def keys(self):
        return _WHICH.keys()

    def __getitem__(self, key):
        return self._dev.read(key)

    def __iter__(self):
        return iter(_WHICH)

    def __len__(self):
        return 4


class replay_buffer:
    def __init__(self, env_params, buffer_size, sample_func, rng=None, ctx=None):
        self.env_params = env_params
        self.T = env_params['max_timesteps']
        self.size = int(buffer_size // self.T)                      # replay_buffer.py:16
        self.sample_func = sample_func
        sampler = getattr(sample_func, "__self__", None)
        if sample_func is not None and not hasattr(sampler, "sq_threshold"):
            raise TypeError(
                "sample_func must be her_sampler(...).sample_her_transitions from "
                "rl_arm_under_sparse_reward_amd.her: sampling runs on the device and there is no "
                "host fallback for arbitrary Python sample functions")
        self._sampler = sampler
        self._rng = rng or (sampler.rng if sampler is not None and sampler._rng is not None else None)
        print("Buffer_size:", self.size, "max_timesteps:", self.T, "env_params:", self.env_params)  # :22
        self._dev = DeviceEpisodeBuffer(self.size, self.T, env_params['obs'], env_params['goal'],
                                        env_params['action'], ctx=ctx)
        self.buffers = _BuffersView(self._dev)

    @property
    def rng(self):
        return self._rng or _random.global_state()

    @property
    def current_size(self):
        return self._dev.info()[1]

    @property
    def n_transitions_stored(self):
        return self._dev.info()[2]

    def store_episode(self, episode_batch):
        """replay_buffer.py:32-43 (+ _get_storage_idx :57-71 on the device).  A `device_env.DeviceEpisodes` handle is stored out
        of its device block (hp_buffer_store_dev): no host copy."""
        if hasattr(episode_batch, "block") and hasattr(episode_batch, "numpy"):
            _lib.check(self._dev.lib.hp_buffer_store_dev(self._dev.h, self.rng.h, C.c_void_p(episode_batch.block),
                                                         len(episode_batch)))
            return
        self._dev.store(self.rng, episode_batch)

    def sample(self, batch_size):
        """replay_buffer.py:46-55."""
        if self._sampler is None:
            raise TypeError("replay_buffer was built without a sample_func")
        return self._dev.sample(self.rng, batch_size, self._sampler.future_p, self._sampler.sq_threshold)

    def enable_f32_rows(self):
        """Opt into the sampler's throughput mode (SURVEY 8b `storage_dtype = fp32`; hp_buffer_enable_f32_rows): a float32
        mirror of observations + actions, one (episode, timestep) per 128-byte line, kept current behind every store_episode;
        `sample_device(..., f32_rows=True)` then reads it.  Everything else keeps reading the reference's float64 arrays."""
        self._dev.enable_f32_rows()

    def enable_fast_draw(self, seed):
        """Opt into the counter-based index draw (SURVEY 8b `rng_mode` = Philox; hp_buffer_sample_dev_fast) for
        `sample_device(..., fast_draw=True)`: every call takes the next counter value under this seed (a rank passes seed + rank).
        NOT the reference's random stream: her.py:24-33's four draws come from Philox4x32-10 keyed by (seed, call, transition),
        so a minibatch is one kernel launch whatever its size (the MT19937 draw of 2^18 transitions is a 2 ms sequential kernel)."""
        self._fast_seed, self._fast_calls = int(seed), 0

    def enable_parallel_draw(self, min_batch=None):
        """Opt into the parallel form of the index draw (hp_rng_set_parallel) for `sample()` and `sample_device()` calls of at
        least `min_batch` transitions (None: the library's measured crossover; 0 switches it off again).  Unlike
        enable_fast_draw this IS the reference's random stream: her.py:24-33's four draws take the same MT19937 words in the
        same order, indices and outputs are bit-identical and `get_state()` afterwards is the same -- the stream is only entered
        at many offsets at once (jump-ahead) instead of being walked by one workgroup.  The mode belongs to the stream
        (`self.rng`): buffers that share it share the setting."""
        self.rng.set_parallel(min_batch)

    def sample_device(self, batch_size, o_norm, g_norm, clip_obs=200, f32_rows=False, fast_draw=False):
        """`sample(batch_size)` followed by the learner's preprocessing (ddpg_agent.py:227-243: _preproc_og, both
        normalizers, concatenate, float32 tensors) in one gather kernel with device outputs: a dict of torch CUDA tensors
        `x` (inputs_norm_tensor), `x_next` (inputs_next_norm_tensor), `actions` (actions_tensor), `r` (r_tensor, [B, 1]).
        Same draws from the same stream and bit-identical float32 values as sample() + normalize() on the host; nothing
        crosses PCIe.  o_norm / g_norm: this package's normalizer objects; clip_obs: arguments.py:87.
        f32_rows=True (after enable_f32_rows()): the throughput mode -- indices, relabelled goals, rewards, goal columns and
        actions still bit-identical, observation columns those of float32-rounded observations, ~half the bytes.
        fast_draw=True (after enable_fast_draw(seed)): the indices come from the counter-based draw inside the gather kernel
        instead of the reference's MT19937 stream (which is then not consumed); everything downstream of the indices unchanged."""
        if self._sampler is None:
            raise TypeError("replay_buffer was built without a sample_func")
        fast = None
        if fast_draw:
            if getattr(self, "_fast_seed", None) is None:
                raise RuntimeError("sample_device(fast_draw=True): enable_fast_draw(seed) first")
            fast = (self._fast_seed, self._fast_calls)
            self._fast_calls += 1
        return self._dev.sample_device(self.rng, o_norm, g_norm, batch_size, self._sampler.future_p,
                                       self._sampler.sq_threshold, clip_obs, f32_rows=f32_rows, fast=fast)
