"""Hyper-parameters of the hot path, named like the reference's live config
(arguments.py:74-106 `Args`; the argparse variant there is dead code)."""
from __future__ import annotations

from dataclasses import dataclass


@dataclass
class Args:
    n_epochs: int = 200
    n_cycles: int = 50
    n_batches: int = 40
    seed: int = 125
    replay_strategy: str = "future"
    clip_return: float = 50.0          # unused by the reference too (it uses 1/(1-gamma))
    save_dir: str = "saved_models/"
    noise_eps: float = 0.01
    random_eps: float = 0.3
    buffer_size: float = 1e6 * 1 / 2
    replay_k: int = 4
    clip_obs: float = 200
    batch_size: int = 256
    gamma: float = 0.98
    action_l2: float = 1
    lr_actor: float = 0.001
    lr_critic: float = 0.001
    polyak: float = 0.95
    n_test_rollouts: int = 25
    clip_range: float = 5
    cuda: bool = True                   # informational: the learner always runs on the MI355X
    num_rollouts_per_mpi: int = 2
    add_demo: bool = False
    demo_name: str = "bmirobot_1000_push_demo.npz"
    demo_source: str = "file"           # add_demo: "file" = preload demo_name (the reference); "device" = generate demo_episodes
                                        # scripted demonstrations on the device (device_env.generate_demos; a native environment)
    demo_episodes: int = 1000           # get_demo_data_push.py:13 demo_num
    demo_max_episodes: int = 10000      # get_demo_data_push.py:27: episodes attempted at most
    train_type: str = "push"
    env_name: str = "bmirobot_push seed125"
    distance_threshold: float = 0.05    # bmirobot_push_F.py:20 / bmirobot_pickandplace_v2.py:19
    reward_type: str = "sparse"         # bmirobot_push_F.py:9; "dense" = -distance (compute_reward :89-90)
    share_numpy_stream: bool = True     # learn(): one random stream for exploration + sampler, like the reference's np.random
    explore_streams: bool = False       # device rollouts: one exploration stream per environment (RandomState(seed + rank * n_envs + i))
    device_reset: bool = False          # native device environments: reset on the device, all waves of a call in one launch
    eval_metrics: bool = False          # learn(): also keep return, goal distances and first success of every evaluation (agent.eval_metrics)
    eval_critic: bool = False           # learn(): also audit the critic on every evaluation's episodes, Q beside the discounted return (agent.eval_critic)
    audit_policy: bool = False          # learn(): once per epoch, audit the policy on the last cycle's exploring episodes, pi(s) and Q(s, pi(s)) beside the recorded actions (agent.policy_audit)
    audit_actor_signal: bool = False    # learn(): once per epoch, audit the actor's learning signal on the last cycle's exploring episodes, dQ/da at pi(s) beside the regulariser and the recorded actions (agent.actor_signal_audit)
    audit_bellman: object = False       # learn(): False, "desired" or "final" -- once per epoch, audit the critic's TD error on the last cycle's exploring episodes under the desired goal or under each episode's final achieved goal (agent.bellman_audit)
    state_full_every: int = 0           # learn() with args.state_path: 0 = every save is a full state; k >= 1 = every k-th save
                                        # rewrites the base, the saves between rewrite one cumulative delta beside it (train_state.py)
    grad_reduce: str = "sum"            # data-parallel gradient exchange: "sum" = utils.py:47 (reference), or "mean"
