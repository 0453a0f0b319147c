"""Helpers shared by the -m gpu update tests (one update against the oracle, teacher-forced parity, the minibatch an update
gathers, the HER sampler, the parallel draw): a learner without an environment, the launch log of a sequence, the hyperparameters
away from the reference's defaults, the launch structures of one update, and goal pairs on the success radius."""
import numpy as np

from gpu_common import ENV_PARAMS, fresh_rng
from oracle.her_replay import compute_reward
from rl_arm_under_sparse_reward_amd.arguments import Args
from rl_arm_under_sparse_reward_amd.ddpg_agent import ddpg_agent

# Every hyperparameter the learner reads, as in tests/golden/ddpg_update_hparams.npz (tools/gen_golden.py DDPG_HPARAMS): gamma 0.9
# (clip_return 10), action_l2 0.5, unequal learning rates (a swapped per-element rate selection in an optimizer kernel is invisible
# at 1e-3 / 1e-3), polyak 0.9, and clips that bite -- clip_obs 0.8 clips ~16% of the raw values, clip_range 1.5 ~17% of the
# normalised ones; action_max 0.7 is not a power of two, so a dropped or reordered division by it is not exact.
HP = dict(gamma=0.9, action_l2=0.5, lr_actor=3e-4, lr_critic=2e-3, polyak=0.9, clip_range=1.5, clip_obs=0.8)
HP_ENV = dict(ENV_PARAMS, action_max=0.7)

# launch structures of one update: switch name -> environment read by hp_agent_create
LAUNCH = {"default": {}, "split": {"RLARM_SPLIT": "1"}, "slab8_rows8": {"RLARM_SLAB_ROWS": "8"},
          "slab8_rows16": {"RLARM_SLAB_ROWS": "16"}, "slab32": {"RLARM_ENGINE": "slab32"}, "dw64": {"RLARM_DW64": "s3"},
          "adam_unfused": {"RLARM_FUSE_ADAM": "0"}, "layers": {"RLARM_ENGINE": "layers"},
          "slab32_dw64": {"RLARM_ENGINE": "slab32", "RLARM_DW64": "s3"}}


def make_agent(batch=256, n_eps=64, seed=125, replay_k=4, env_params=None, **kw):
    args = Args(batch_size=batch, buffer_size=n_eps * 100, replay_k=replay_k, **kw)
    rng = fresh_rng(seed)
    return ddpg_agent(args, None, dict(env_params or ENV_PARAMS), rng=rng), rng


def klog(open_, updates, close=(), prologue=()):
    """The dict update_kernels returns, from runs of identical updates: updates = [(kernels, count), ...]."""
    return {"open": list(open_), "prologue": list(prologue), "updates": [list(k) for k, c in updates for _ in range(c)],
            "close": list(close)}


# The whole launch log of a sequence, per engine shape and switch.
UPDATE_KLOG = {
    ("", 256, 40): klog(["k_draw_plan"], [(["k_fb_split8<0>", "k_gemm_lds_adam"], 40)], prologue=["k_fb_split8<0>"]),
    ("", 256, 4): klog(["k_draw_plan"], [(["k_fb_slab8", "k_gemm_lds_adam"], 4)]),
    ("", 256, 1): klog(["k_draw_plan"], [(["k_fb_slab8", "k_gemm_lds_adam"], 1)]),
    ("RLARM_SPLIT=0", 256, 40): klog(["k_draw_plan"], [(["k_fb_slab8", "k_gemm_lds_adam"], 40)]),
    ("RLARM_SPLIT=1", 256, 4): klog(["k_draw_plan"], [(["k_fb_split8<0>", "k_gemm_lds_adam"], 4)], prologue=["k_fb_split8<0>"]),
    ("RLARM_SPLIT=1", 256, 1): klog(["k_draw_plan"], [(["k_fb_split8<0>", "k_gemm_lds_adam"], 1)], prologue=["k_fb_split8<0>"]),
    # the last update has nothing left to draw or gather: no riders
    ("", 512, 40): klog(["k_draw_plan"], [(["k_fb_slab8", "k_gemm_lds_adam_ride_u"], 39), (["k_fb_slab8", "k_gemm_lds_adam_u"], 1)]),
    ("", 1024, 40): klog(["k_draw_plan"], [(["k_fb_slab8", "k_gemm_lds_adam_ride"], 39), (["k_fb_slab8", "k_gemm_lds_adam"], 1)]),
    ("", 2048, 40): klog(["k_draw_plan"], [(["k_fb_slab8", "k_dw64_adam"], 40)]),
    ("", 4096, 40): klog(["k_draw_plan"], [(["k_gather_fused", "k_fb_slab32", "k_dw64_adam"], 1), (["k_fb_slab32", "k_dw64_adam"], 39)]),
    ("RLARM_ENGINE=layers", 256, 4): klog(["k_draw_plan"], [(["k_gather_fused"] + ["k_gemm_lds"] * 16, 4)]),
    ("RLARM_FUSE_ADAM=0", 256, 4): klog(["k_draw_plan"], [(["k_fb_slab8", "k_gemm_lds", "k_adam_frag4"], 4)]),
    ("RLARM_FUSE_ADAM=0", 1024, 4): klog(["k_draw_plan"], [(["k_fb_slab8", "k_gemm_lds_ride", "k_adam_frag4"], 3),
                                                           (["k_fb_slab8", "k_gemm_lds", "k_adam_frag4"], 1)]),
    ("RLARM_FUSE_ADAM=0", 4096, 4): klog(["k_draw_plan"], [(["k_gather_fused", "k_fb_slab32", "k_dw64", "k_adam_frag4"], 1),
                                                           (["k_fb_slab32", "k_dw64", "k_adam_frag4"], 3)]),
}


def set_launch(name, monkeypatch):
    monkeypatch.setenv("RLARM_KEEP_GRADS", "1")
    for kk, v in LAUNCH[name].items():
        monkeypatch.setenv(kk, v)


def expect_engine(agent, launch, engine):
    """The engine a case is about, asserted, so that a change of the default table cannot move the case elsewhere silently."""
    e = agent.engine()
    assert e["engine"] == engine, (launch, e)
    first = agent.update_kernels(1)["updates"][0][0]
    if launch == "split":
        assert first.startswith("k_fb_split8"), (launch, first)
    elif engine == "slab8":
        assert first == "k_fb_slab8", (launch, first)
    return e


def threshold_pairs(gd, seed=5):
    """Pairs (ag, g) of width gd whose distance lies within three ulps of the 0.05 radius, on both sides of it and on it where
    the arithmetic allows, with the reward bits the oracle's compute_reward gives them on the CPU."""
    rs = np.random.RandomState(seed)
    u = rs.normal(size=(4096, gd))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    g = rs.uniform(0, 0.3, (4096, gd)) if gd > 1 else np.zeros((4096, 1))
    scale = 0.05 * (1.0 + rs.randint(-6, 7, (4096, 1)) * 2.0 ** -52)
    ag = g + u * scale
    d = np.sqrt(np.sum(np.square(ag - g), axis=-1))
    ulps = (d.view(np.int64) - np.float64(0.05).view(np.int64))
    keep = np.abs(ulps) <= 3
    ag, g, ulps = ag[keep], g[keep], ulps[keep]
    assert len(ag) >= 64 and (ulps > 0).any() and (ulps <= 0).any(), (gd, len(ag))
    r = compute_reward(ag, g, 0.05, "sparse")
    assert r.dtype == np.float32 and len(set(r.view(np.uint32))) == 2, gd
    return ag, g, r.view(np.uint32)


def pairs_as_one_step_episodes(ag, g, od, ad):
    M, gd = ag.shape
    agm = np.zeros((M, 2, gd)); agm[:, 1, :] = ag
    return [np.zeros((M, 2, od)), agm, g[:, None, :].copy(), np.zeros((M, 1, ad))]
