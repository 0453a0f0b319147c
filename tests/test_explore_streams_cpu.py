"""Per-environment exploration streams without a device: how a training state carries them (train_state.write_state / read_state /
verify on synthetic arrays), the default of the switch, the ABI table, and the draw kernel's device assembly (no scratch)."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from cpu_common import stream_arrays, synthetic_state
from kernel_metadata import kernel_metadata
from rl_arm_under_sparse_reward_amd import train_state as ts
from rl_arm_under_sparse_reward_amd.arguments import Args


def state_with_streams(n=3):
    arrays, manifest = synthetic_state()
    extra, manifest["explore_streams"] = ts.stream_record(*stream_arrays(n))
    arrays.update(extra)
    return arrays, manifest


def test_the_switch_is_off_by_default():
    assert Args().explore_streams is False


def test_a_state_with_streams_round_trips_and_verifies(tmp_path):
    arrays, manifest = state_with_streams(3)
    assert manifest["explore_streams"]["n"] == 3 and sorted(manifest["explore_streams"]["arrays"]) == sorted(ts.STREAM_ARRAYS)
    assert arrays["explore_stream_has_gauss"].tolist() == [0, 1, 0] and arrays["explore_stream_gauss"][1] != 0.0
    path = ts.write_state(tmp_path / "s.npz", arrays, manifest)
    back, m = ts.read_state(path)
    assert m == manifest
    want = stream_arrays(3)
    for name, a in zip(ts.STREAM_ARRAYS, want):
        assert back[name].dtype == np.dtype(ts.stream_shapes(3)[name][0]) and np.array_equal(back[name], a), name
    assert ts.verify(path)["explore_streams"]["n"] == 3
    assert ts.main(["verify", path]) == 0


def test_a_state_without_streams_is_written_as_before(tmp_path):
    arrays, manifest = synthetic_state()
    path = ts.write_state(tmp_path / "s.npz", arrays, manifest)
    back, m = ts.read_state(path)
    assert "explore_streams" not in m and not [k for k in back if k.startswith("explore_stream")]
    assert sorted(back) == sorted(arrays)
    ts.verify(path)


@pytest.mark.parametrize("name", ts.STREAM_ARRAYS)
def test_verify_names_a_missing_or_damaged_stream_array(tmp_path, name):
    arrays, manifest = state_with_streams(4)
    gone = {k: v for k, v in arrays.items() if k != name}
    with pytest.raises(ts.StateError, match=f"array '{name}' is missing"):
        ts.verify(ts.write_state(tmp_path / "gone.npz", gone, manifest))
    bad = dict(arrays)
    bad[name] = arrays[name].copy()
    flat = bad[name].reshape(-1).view(np.uint8)
    flat[flat.size // 2] ^= 0x04
    with pytest.raises(ts.StateError, match=f"array '{name}'"):
        ts.verify(ts.write_state(tmp_path / "bad.npz", bad, manifest))
    short = dict(arrays)
    short[name] = arrays[name][:3]
    with pytest.raises(ts.StateError, match=f"array '{name}' is .* 4 streams imply"):
        ts.verify(ts.write_state(tmp_path / "short.npz", short, manifest))


def test_verify_refuses_stream_arrays_the_manifest_does_not_list(tmp_path):
    arrays, manifest = state_with_streams(2)
    del manifest["explore_streams"]
    with pytest.raises(ts.StateError, match="array 'explore_stream_keys' is present but the manifest has no 'explore_streams'"):
        ts.verify(ts.write_state(tmp_path / "s.npz", arrays, manifest))


def test_verify_refuses_a_position_outside_the_key(tmp_path):
    keys, pos, has, val = stream_arrays(2)
    pos[1] = 625
    arrays, manifest = synthetic_state()
    extra, manifest["explore_streams"] = ts.stream_record(keys, pos, has, val)
    arrays.update(extra)
    with pytest.raises(ts.StateError, match="'explore_stream_pos' holds a position outside"):
        ts.verify(ts.write_state(tmp_path / "s.npz", arrays, manifest))


def test_ctypes_table_binds_the_stream_entry_points():
    from rl_arm_under_sparse_reward_amd import _lib
    names = {"hp_streams_create", "hp_streams_seed", "hp_streams_get_state", "hp_streams_set_state",
             "hp_streams_get_all", "hp_streams_set_all", "hp_streams_destroy", "hp_rollout_step_streams"}
    assert names <= set(_lib.PROTOTYPES) and not (names & _lib.DEBUG_SYMBOLS)
    # hp_rollout_step's arguments, the stream array in place of the single stream
    assert _lib.PROTOTYPES["hp_rollout_step_streams"] == _lib.PROTOTYPES["hp_rollout_step"]
    header = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    assert re.search(r"#define\s+HP_ABI_VERSION\s+4\b", header)


def test_the_stream_step_kernel_uses_no_scratch(tmp_path):
    """The device assembly of csrc/rollout.hip, compiled as the Makefile compiles it: k_rollout_step_streams (and the
    single-stream kernel beside it) have private_segment_fixed_size 0, and one workgroup's LDS lets 16 of them share a CU."""
    meta = kernel_metadata(tmp_path, "rollout.hip")
    streams = [k for k in meta if "k_rollout_step_streams" in k]
    assert len(streams) == 1 and any("k_rollout_step" in k and "streams" not in k for k in meta), sorted(meta)
    for k, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (k, m)
    assert 16 * meta[streams[0]]["group_segment_fixed_size"] <= 160 * 1024
