"""Host side of sonar_slam_amd.mapping.MapBatch, no device: the update planner (flat (session, key, pose) lists -> per-map
ordered groups -> apply rounds), argument checks, the refusals and load_yaml."""
import os
import types

import pytest

from sonar_slam_amd import mapping
from sonar_slam_amd.pose2 import Pose2

HERE = os.path.dirname(os.path.abspath(__file__))


def _kfs(n, missed=()):
    return [None if k in missed else types.SimpleNamespace(k=k, pose=Pose2(float(k), 0.0, 0.0)) for k in range(n)]


def _gate():
    return mapping.Mapping().pose_changed       # the defaults: 0.5 m, 0.05 rad


def _plan(keyframes, flat):
    gates = [_gate() for _ in keyframes]
    return mapping.plan_updates(keyframes, gates, [f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat])


def apply_rounds(wave, dec):
    """the schedule sfe_mapset_refit is specified to follow for one wave (tests/test_gpu_map_batch.py holds the device's own
    launch counter to its length): round i holds the i-th apply of every
    session (a refit is two applies, subtract then add; a first fit is one) -> [round][(session, keyframe, sign)]"""
    rounds = []
    for s, group in wave:
        i = 0
        for kf, _ in group:
            for sign in ((-1, +1) if dec else (+1,)):
                while len(rounds) <= i:
                    rounds.append([])
                rounds[i].append((s, kf, sign))
                i += 1
    return rounds


def _moved(k, d=1.0):
    return Pose2(float(k) + d, 0.0, 0.0)


def test_planner_groups_by_session_in_list_order():
    kfs = [_kfs(4), _kfs(4)]
    flat = [(0, 2, _moved(2)), (1, 0, _moved(0)), (0, 0, _moved(0)), (1, 3, _moved(3)), (0, 1, _moved(1))]
    waves = _plan(kfs, flat)
    assert len(waves) == 1
    assert [(s, [kf.k for kf, _ in g]) for s, g in waves[0]] == [(0, [2, 0, 1]), (1, [0, 3])]
    assert kfs[0][2].pose.x() == 3.0 and kfs[1][3].pose.x() == 4.0       # accepted keyframes carry their new pose


def test_a_repeated_key_splits_its_sessions_group_only():
    kfs = [_kfs(3), _kfs(3)]
    flat = [(0, 0, _moved(0)), (1, 0, _moved(0)), (0, 1, _moved(1)), (0, 0, _moved(0, 5.0)), (1, 1, _moved(1)),
            (0, 2, _moved(2))]
    waves = _plan(kfs, flat)
    assert [[(s, [kf.k for kf, _ in g]) for s, g in w] for w in waves] == [[(0, [0, 1]), (1, [0, 1])], [(0, [0, 2])]]
    assert kfs[0][0].pose.x() == 5.0
    # ... and its first group is still fitted at the pose listed there, not at the one it has moved on to
    assert [p.x() for _, p in waves[0][0][1]] == [1.0, 2.0] and [p.x() for _, p in waves[1][0][1]] == [5.0, 3.0]


def test_a_repeated_key_is_gated_against_the_pose_it_just_took():
    kfs = [_kfs(2)]
    waves = _plan(kfs, [(0, 0, _moved(0)), (0, 0, _moved(0, 1.1))])      # 0.1 m from the pose taken a moment ago: unchanged
    assert [[(s, [kf.k for kf, _ in g]) for s, g in w] for w in waves] == [[(0, [0])]]
    assert kfs[0][0].pose.x() == 1.0


def test_missed_keys_and_unchanged_poses_drop_out():
    kfs = [_kfs(4, missed=(1,)), _kfs(4)]
    flat = [(0, 0, _moved(0)), (0, 1, _moved(1)), (0, 2, _moved(2, 0.2)), (1, 2, Pose2(2.0, 0.0, 0.01)),
            (1, 3, Pose2(3.0, 0.0, 0.06)), (0, 3, _moved(3))]
    waves = _plan(kfs, flat)
    assert [[(s, [kf.k for kf, _ in g]) for s, g in w] for w in waves] == [[(0, [0, 3]), (1, [3])]]
    assert kfs[0][2].pose.x() == 2.0 and kfs[1][2].pose.theta() == 0.0   # the rejected ones keep their pose
    # nothing accepted at all: no wave, no device call
    assert _plan([_kfs(2)], [(0, 0, Pose2(0.0, 0.0, 0.0))]) == []


def test_a_key_beyond_the_keyframes_is_an_error_and_lengths_must_agree():
    with pytest.raises(AssertionError):
        _plan([_kfs(2)], [(0, 2, _moved(2))])
    with pytest.raises(ValueError, match="2 sessions, 1 keys"):
        mapping.plan_updates([_kfs(2)], [_gate()], [0, 0], [1], [_moved(1), _moved(1)])


def test_apply_rounds_have_the_width_of_the_sessions_still_applying():
    kfs = [_kfs(5), _kfs(5), _kfs(5)]
    flat = [(0, k, _moved(k)) for k in range(5)] + [(1, k, _moved(k)) for k in range(2)] + [(2, 4, _moved(4))]
    (wave,) = _plan(kfs, flat)
    rounds = apply_rounds(wave, dec=True)
    # a refit is subtract then add: 5, 2 and 1 keyframes -> 10 rounds, not 2 * 8 launches
    assert len(rounds) == 10
    assert [len(r) for r in rounds] == [3, 3, 2, 2, 1, 1, 1, 1, 1, 1]
    assert [sign for _, _, sign in rounds[0]] == [-1, -1, -1] and [sign for _, _, sign in rounds[1]] == [1, 1, 1]
    # inside one session the order is the call's: (k0 -, k0 +, k1 -, k1 +, ...)
    mine = [(kf.k, sign) for r in rounds for s, kf, sign in r if s == 1]
    assert mine == [(0, -1), (0, 1), (1, -1), (1, 1)]
    # no session twice in a round (a round's jobs never share a grid)
    assert all(len({s for s, _, _ in r}) == len(r) for r in rounds)
    adds = apply_rounds(wave, dec=False)
    assert [len(r) for r in adds] == [3, 2, 1, 1, 1] and {sign for r in adds for _, _, sign in r} == {1}


def test_constructor_checks_its_arguments():
    for bad in (dict(n_sessions=0), dict(max_keyframes=0), dict(max_pixels=0)):
        with pytest.raises(ValueError, match="must be positive"):
            mapping.MapBatch(None, **dict(dict(n_sessions=2, max_keyframes=4), **bad))
    with pytest.raises(TypeError, match="unknown setting 'resolutoin'"):
        mapping.MapBatch(None, 2, 4, resolutoin=0.1)
    b = mapping.MapBatch(None, 3, 7, inc=25.0, hit_prob=0.7)
    assert (b.S, b.max_keyframes, b.inc, b.hit_prob) == (3, 7, 25.0, 0.7)
    ref = mapping.Mapping()
    for name in mapping.SETTINGS:
        if name not in ("inc", "hit_prob"):
            assert getattr(b, name) == getattr(ref, name), name
    with pytest.raises(RuntimeError, match="configure"):
        b.add_keyframes([0], [0], [Pose2(0, 0, 0)], None, [[]])
    with pytest.raises(RuntimeError, match="configure"):
        b.update_poses([0], [0], [Pose2(0, 0, 0)])


def test_refusals():
    b = mapping.MapBatch(None, 2, 4)
    with pytest.raises(NotImplementedError, match="get_occupancy_grid2"):
        b.get_occupancy_grid2()
    with pytest.raises(NotImplementedError, match="get_intensity_grid"):
        b.get_intensity_grid()
    b.pub_intensity = True
    with pytest.raises(NotImplementedError, match="pub_intensity"):
        b.configure()                                   # refused before any device is looked for
    with pytest.raises(NotImplementedError, match="pub_intensity"):
        mapping.MapBatch(None, 2, 4, pub_intensity=True).configure()


def test_load_yaml_sets_what_mapping_load_yaml_sets():
    path = os.path.join(HERE, "golden", "mapping.yaml")
    b = mapping.MapBatch(None, 2, 4)
    b.configure = lambda: None          # the device set is not needed to read the settings
    b.load_yaml(path)
    m = mapping.Mapping()
    m.configure = lambda: None
    m.load_yaml(path)
    for name in mapping.SETTINGS:
        assert getattr(b, name) == getattr(m, name), name
    assert (b.x0, b.y0, b.width, b.height, b.inflation_angle, b.min_rotation) == (-100.0, -100.0, 200.0, 200.0, 0.04, 0.015)
    assert b.inflation_range == 0.5 and b.inflation_radius == 0.5        # the node's quirk, as in Mapping


def test_session_views_are_configured_through_the_batch():
    v = mapping._SessionMap(mapping.MapBatch(None, 1, 1), 0)
    with pytest.raises(RuntimeError, match="MapBatch.configure"):
        v.configure()
    with pytest.raises(RuntimeError, match="MapBatch.load_yaml"):
        v.load_yaml("x.yaml")
