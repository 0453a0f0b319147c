"""Device rollout path, the parts that need no GPU: the tensor twin of the stand-in environment, the wave-block layout, and the
specification of the three legacy draws the device kernel restates (csrc/mt19937_wave.h), checked against numpy here."""
import math

import numpy as np
import pytest
import torch

from conftest import bits
from rl_arm_under_sparse_reward_amd.device_env import (NativePointMassVecEnv, NativePushBlockVecEnv, PointMassVecEnv, binomial1_qn,
                                                       wave_layout)
from rl_arm_under_sparse_reward_amd.feeder import _Layout
from rl_arm_under_sparse_reward_amd.synthetic import PointMassGoalEnv


def test_point_mass_vec_env_equals_n_host_envs_bit_for_bit():
    n, seed, T = 5, 11, 100
    vec = PointMassVecEnv(n, seed=seed, device="cpu", max_timesteps=T)
    host = [PointMassGoalEnv(seed=seed + i, max_timesteps=T) for i in range(n)]
    assert vec.is_device_vec_env and vec.n_envs == n and vec.env_params == host[0].env_params
    rs = np.random.RandomState(3)
    for _episode in range(2):
        o = vec.reset()
        ho = [e.reset() for e in host]
        for t in range(T + 1):
            for key in ("observation", "achieved_goal", "desired_goal"):
                got = o[key].numpy()
                assert got.dtype == np.float64 and o[key].is_contiguous()
                assert np.array_equal(bits(got), bits(np.stack([h[key] for h in ho]))), (t, key)
            if t == T:
                break
            a = (rs.uniform(-0.7, 0.7, (n, 4)) * (1.0 if t % 7 else 30.0)).astype(np.float32)   # some steps hit the walls
            o, r, _, info = vec.step(torch.from_numpy(a))
            hs = [e.step(a[i]) for i, e in enumerate(host)]
            ho = [s[0] for s in hs]
            assert np.array_equal(info["is_success"].numpy(), np.array([s[3]["is_success"] for s in hs], np.float32))
            assert np.array_equal(r.numpy(), np.array([s[1] for s in hs], np.float32))


def test_reward_function_takes_numpy_arrays_like_the_host_env():
    """her_sampler probes `compute_reward` with numpy arrays: the vec env answers those with the host environment's arithmetic."""
    rs = np.random.RandomState(0)
    ag, g = rs.uniform(0, 0.1, (50, 3)), rs.uniform(0, 0.1, (50, 3))
    for reward_type in ("sparse", "dense"):
        vec, host = PointMassVecEnv(2, device="cpu", reward_type=reward_type), PointMassGoalEnv(reward_type=reward_type)
        got, want = vec.compute_reward(ag, g, None), host.compute_reward(ag, g, None)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        assert np.array_equal(vec.compute_reward(torch.from_numpy(ag), torch.from_numpy(g), None).numpy(), want)


def test_partial_wave_resets_only_the_first_environments():
    vec = PointMassVecEnv(3, seed=5, device="cpu")
    o = vec.reset(2)
    assert o["observation"].shape == (2, 27)
    want = PointMassGoalEnv(seed=7)
    assert np.array_equal(vec.reset()["achieved_goal"].numpy()[2], want.reset()["achieved_goal"])   # env 2 untouched by the wave of 2


def test_point_mass_works_on_the_first_active_rows_of_wider_state_tensors():
    """The rule of the shared base, on the plain class: with state tensors widened to n_envs rows (what `enable_device_reset` does
    to a native environment) and `active` = 3, `step` and `_observation` read and write rows 0-2 in place, leave rows 3-4 alone,
    and give the bits of a 3-environment `PointMassVecEnv` handed the same actions."""
    n, k, seed = 5, 3, 9
    wide, ref = PointMassVecEnv(n, seed=seed, device="cpu"), PointMassVecEnv(k, seed=seed, device="cpu")
    o_w, o_r = wide.reset(k), ref.reset()
    sentinel = {}
    for j, name in enumerate(wide.state_names):
        t = getattr(wide, name)
        f = torch.full((n, 3), -7.0 - j, dtype=torch.float64)
        f[:k] = t
        setattr(wide, name, f)
        sentinel[name] = f[k:].clone()
    wide.active = k
    o_w = wide._observation()
    tensors = {name: getattr(wide, name) for name in wide.state_names}
    rs = np.random.RandomState(4)
    for t in range(12):
        for key in ("observation", "achieved_goal", "desired_goal"):
            assert o_w[key].shape[0] == k and o_w[key].is_contiguous()
            assert np.array_equal(bits(o_w[key].numpy()), bits(o_r[key].numpy())), (t, key)
        a = torch.from_numpy((rs.uniform(-0.7, 0.7, (k, 4)) * (1.0 if t % 5 else 30.0)).astype(np.float32))   # some steps hit the walls
        (o_w, r_w, _, i_w), (o_r, r_r, _, i_r) = wide.step(a), ref.step(a)
        assert r_w.shape == (k,) and torch.equal(r_w, r_r) and torch.equal(i_w["is_success"], i_r["is_success"])
        for name in wide.state_names:
            w = getattr(wide, name)
            assert w is tensors[name] and tuple(w.shape) == (n, 3), name                 # in place: the same tensors, still wide
            assert np.array_equal(bits(w[:k].numpy()), bits(getattr(ref, name).numpy())), (t, name)
            assert np.array_equal(bits(w[k:].numpy()), bits(sentinel[name].numpy())), (t, name)
    assert float(wide.vel[:k].abs().sum()) > 0       # the rows did move


def test_a_native_class_is_its_kind_and_nothing_else():
    """What keeps the duplication from growing back: the native classes inherit reset, step, the observation and the descriptor
    (`_NativeEnv`, the vectorised parent) and define only their kind."""
    for cls, kind in ((NativePointMassVecEnv, 1), (NativePushBlockVecEnv, 2)):
        assert not {"reset", "step", "_observation", "native_desc"} & set(vars(cls)), sorted(vars(cls))
        assert vars(cls)["kind"] == kind
        env = cls(3, seed=2, device="cpu")
        env.reset(2)
        d = env.native_desc()
        assert d["kind"] == kind and d["params"] == env.params()
        assert [t is getattr(env, name) and t.is_contiguous() for t, name in zip(d["state"], env.state_names)] == [True] * len(env.state_names)
        with pytest.raises(ValueError, match=r"n_active outside \[1, n_envs\]"):
            env.reset(4)


@pytest.mark.parametrize("shape", [(2, 100, 27, 3, 4), (7, 13, 10, 2, 3)])
def test_wave_block_offsets_equal_the_feeder_layout(shape):
    lay, mine = _Layout(*shape), wave_layout(*shape)
    assert (mine["obs"], mine["ag"], mine["g"], mine["actions"], mine["elems"]) == (lay.o_obs, lay.o_ag, lay.o_g, lay.o_act,
                                                                                    lay.slot_elems)


def test_binomial_qn_helper():
    for p in (0.0, 0.3, 0.5):
        assert binomial1_qn(p) == (math.exp(math.log(1 - p)), False)
    assert binomial1_qn(0.7) == (math.exp(math.log(1 - (1.0 - 0.7))), True)
    assert binomial1_qn(1.0) == (1.0, True)
    with pytest.raises(ValueError):
        binomial1_qn(1.5)


# ---- the specification: numpy's legacy draws restated on raw 32-bit words ------------------------------------------------------
class LegacyDraws:
    """randn / uniform / binomial(1, p) of numpy's legacy RandomState on a stream of 32-bit words (`next32`), with the cached
    second normal.  This is what csrc/mt19937_wave.h implements; tests/test_gpu_device_rollout.py checks the kernel against it
    through numpy itself."""

    def __init__(self, rs):
        self.rs = rs                      # only .randint-free raw words are taken from it: rs.bytes(4)
        self.has_gauss, self.gauss = 0, 0.0

    def next32(self):
        return int.from_bytes(self.rs.bytes(4), "little")

    def double(self):
        a, b = self.next32() >> 5, self.next32() >> 6
        return (a * 67108864.0 + b) / 9007199254740992.0

    def randn(self):
        if self.has_gauss:
            v, self.has_gauss, self.gauss = self.gauss, 0, 0.0
            return v
        while True:
            x1 = 2.0 * self.double() - 1.0
            x2 = 2.0 * self.double() - 1.0
            r2 = x1 * x1 + x2 * x2
            if r2 < 1.0 and r2 != 0.0:
                break
        f = math.sqrt(-2.0 * math.log(r2) / r2)
        self.gauss, self.has_gauss = f * x1, 1
        return f * x2

    def uniform(self, low, high):
        return low + (high - low) * self.double()

    def binomial1(self, eps):
        qn, reflected = binomial1_qn(eps)
        p = 1.0 - eps if reflected else eps
        q = 1.0 - p
        bound = 1                          # min(n, np + 10 sqrt(npq + 1)) with n = 1
        X, px, U = 0, qn, self.double()
        while U > px:
            X += 1
            if X > bound:
                X, px, U = 0, qn, self.double()
            else:
                U -= px
                px = ((1 - X + 1) * p * px) / (X * q)
        return 1 - X if reflected else X

    def select_actions(self, pi, noise_eps, random_eps, amax):
        """ddpg_agent._select_actions (:174-184) on a float32 policy output"""
        ad = pi.shape[0]
        action = pi.copy()
        action += noise_eps * amax * np.array([self.randn() for _ in range(ad)])
        action = np.clip(action, -amax, amax)
        ra = np.array([self.uniform(-amax, amax) for _ in range(ad)])
        action += np.int64(self.binomial1(random_eps)) * (ra - action)
        return action


def numpy_select_actions(rs, pi, noise_eps, random_eps, amax):
    ad = pi.shape[0]
    action = pi.copy()
    action += noise_eps * amax * rs.randn(ad)
    action = np.clip(action, -amax, amax)
    ra = rs.uniform(low=-amax, high=amax, size=ad)
    action += rs.binomial(1, random_eps, 1)[0] * (ra - action)
    return action


@pytest.mark.parametrize("act_dim", [3, 4])
@pytest.mark.parametrize("random_eps", [0.3, 0.7, 0.0, 1.0])
def test_restated_draws_match_numpy(act_dim, random_eps):
    a, b = np.random.RandomState(123), np.random.RandomState(123)
    spec = LegacyDraws(b)
    prs = np.random.RandomState(9)
    for _ in range(2000):
        pi = prs.uniform(-0.5, 0.5, act_dim).astype(np.float32)
        want = numpy_select_actions(a, pi, 0.2, random_eps, 0.5)
        got = spec.select_actions(pi, 0.2, random_eps, 0.5)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    sa = a.get_state()
    sb = b.get_state()
    assert np.array_equal(sa[1], sb[1]) and sa[2] == sb[2]
    assert (sa[3], sa[4]) == (spec.has_gauss, spec.gauss)
