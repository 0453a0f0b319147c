"""The cases of the Bellman audit's tests (test_episode_bellman_cpu.py, test_gpu_episode_bellman.py) and their inputs.  No tests
here."""
import numpy as np

SHAPES = [(27, 3, 4, 0.5), (10, 3, 4, 1.0), (5, 2, 1, 2.0), (13, 3, 3, 0.25)]       # obs, goal, act, max_action
BLOCKS = [(3, 5), (1, 1), (2, 70)]      # 15 rows: the last slab holds three, slabs straddle episodes, step T-1 reads obs[T] across the
                                        # T + 1 / T strides; one row whose next state is the final observation; the stats chunk wraps
CLIPS = [0.8, float("inf")]             # a clip_obs that bites, and none
GOALS = ["desired", "final"]
KINDS = ["sparse", "dense"]
THRESHOLD = 0.3
INPUT_SEED = 23


def block_inputs(shape, block, seed=INPUT_SEED):
    """(obs [n, T+1, od], ag [n, T+1, gd], g [n, T, gd], actions [n, T, ad]) float64 of one case.  The closing observation is read
    (it is the last step's next state).  The achieved goals lie around the desired ones at distances on both sides of THRESHOLD, so
    a sparse reward takes both values; g varies along an episode, so the two goal modes differ in every row."""
    od, gd, ad, amax = shape
    n, T = block
    rs = np.random.RandomState(seed + 7 * od + 100 * n + T)
    obs = rs.normal(0.1, 0.6, (n, T + 1, od))
    g = rs.normal(0.2, 0.5, (n, T, gd))
    ag = np.concatenate([g[:, :1], g], axis=1) + rs.normal(0, THRESHOLD / np.sqrt(gd), (n, T + 1, gd))
    return obs, ag, g, rs.uniform(-amax, amax, (n, T, ad))


def goals_of(ag, g, goal):
    """G [n, T, gd]: the goal every step is taken under"""
    return g if goal == "desired" else np.repeat(ag[:, -1:], g.shape[1], axis=1)
