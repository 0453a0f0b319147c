"""Helpers shared by tests that need no device: a synthetic training state with its manifest, per-environment stream arrays, and
goal pairs laid out as episodes."""
import numpy as np

from rl_arm_under_sparse_reward_amd import train_state as ts

DIMS = {"obs": 5, "goal": 2, "action": 3, "hidden": 32, "T": 4, "capacity": 7, "current_size": 3}


def synthetic_state(seed=0):
    rs = np.random.RandomState(seed)
    arrays, listed = {}, {}
    for name, (dt, shape) in ts.expected_shapes(DIMS).items():
        if name == "buffer_counters":
            a = np.array([DIMS["current_size"], DIMS["current_size"] * DIMS["T"]], dt)
        elif np.dtype(dt).kind == "f":
            a = rs.normal(size=shape).astype(dt)
        else:
            a = rs.randint(0, 2 ** 31 - 1, size=shape).astype(dt)
        arrays[name] = a
        listed[name] = {"dtype": dt, "shape": list(shape), "sum": list(ts.checksum(a))}
    st = np.random.RandomState(9).get_state()
    arrays.update({"np_random_key": st[1].astype(np.uint32), "success_rates": np.array([0.25, 0.5]),
                   "extra": np.frombuffer(b"opaque", np.uint8).copy()})
    manifest = {"format": ts.FORMAT_VERSION, "dims": dict(DIMS), "rank": 0, "world_size": 1, "abi": 4, "arrays": listed,
                "np_random": {"pos": int(st[2]), "has_gauss": 0, "cached_gaussian": 0.0}, "rng_gauss": [0, 0.0], "savetime": 2,
                "epoch": 2, "cycle": 0}
    return arrays, manifest


def stream_arrays(n, pending=(1,)):
    """States of RandomState(40 + i) after a few draws; the streams in `pending` hold a cached normal."""
    keys, pos, has, val = np.empty((n, 624), np.uint32), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n)
    for i in range(n):
        rs = np.random.RandomState(40 + i)
        rs.randn(3 if i in pending else 4)
        rs.uniform(size=i)
        st = rs.get_state()
        keys[i], pos[i], has[i], val[i] = st[1], st[2], st[3], st[4]
    return keys, pos, has, val


def pairs_as_episodes(pair_ag, pair_g, T):
    """Goal pairs [m, goal] laid out as m // T episodes of T steps: step t of episode e compares pair e * T + t, i.e.
    ag[e, t + 1] = pair_ag[e * T + t] and g[e, t] = pair_g[e * T + t]; ag[e, 0] takes part in nothing."""
    n, gd = pair_ag.shape[0] // T, pair_ag.shape[1]
    ag = np.zeros((n, T + 1, gd))
    ag[:, 1:] = pair_ag[:n * T].reshape(n, T, gd)
    return ag, np.ascontiguousarray(pair_g[:n * T].reshape(n, T, gd))
