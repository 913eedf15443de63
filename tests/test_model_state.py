"""CPU: the host-side state the three trainable models share (multiposenet_amd/model_state.py) - state_dict round trips,
pads, key handling, variable sharing and the arena layouts. Needs no HIP library."""
import hashlib

import numpy as np
import pytest
import torch

from multiposenet_amd import model_state, net, prn, retinanet


class _State(model_state.ModelState):
    def __init__(self, shapes, order=None, pads=None):
        self.device, self.dtype = torch.device("cpu"), torch.float32
        self._init_state(shapes, order, pads)


class _PrnStyle(_State):
    ignore_unknown = True


def _keypoint(dm):
    shapes, pads = net.internal_shapes(dm)          # (as KeypointNet lays out its arenas)
    return _State(shapes, pads=pads)


def _detector():
    shapes = retinanet.head_variable_shapes(1.0)    # (as PersonDetectorNet does)
    return _State(shapes, order=retinanet._arena_order(shapes))


def _noisy(values, seed):
    rs = np.random.RandomState(seed)
    return {k: (v + rs.randn(*v.shape)).astype(np.float32) for k, v in values.items()}


def test_round_trip_with_a_padded_stem_keeps_reference_shapes_and_zero_pads():
    s = _keypoint(0.75)
    assert s._pads                                           # 24 stem channels, 32 in the arena
    values = _noisy(net.initial_values(3, 0.75), 4)
    v0 = s.var_version
    s.load_state_dict(values)
    assert s.var_version == v0 + 1
    sd = s.state_dict()
    names = list(net.variable_shapes(0.75))
    assert list(sd) == [k for k in names if net.is_trainable(k)] + [k for k in names if not net.is_trainable(k)]
    for k, v in values.items():
        np.testing.assert_array_equal(sd[k], v, err_msg=k)
    # garbage in the pads is reset by the next load; the reference-shaped part round-trips
    for k in s._pads:
        s.vars.get(k, s.stats.get(k)).fill_(7.0)
    s.load_state_dict(sd)
    for k, (axis, n) in s._pads.items():
        full = s.vars.get(k, s.stats.get(k))
        assert full.shape[axis] == 32 and n == 24, k
        assert not full.narrow(axis, n, full.shape[axis] - n).any(), k
        np.testing.assert_array_equal(s.unpad(k, full).numpy(), values[k], err_msg=k)


def test_strict_load_raises_on_unknown_and_missing_names():
    assert not net.KeypointNet.ignore_unknown and not retinanet.PersonDetectorNet.ignore_unknown
    s = _keypoint(1.0)
    values = net.initial_values(0)
    with pytest.raises(KeyError, match="unknown variable"):
        s.load_state_dict(dict(values, **{"MobilenetV1/Logits/weights": np.zeros(3, np.float32)}))
    partial = {k: v for k, v in values.items() if k != "final_bn/moving_mean"}
    with pytest.raises(KeyError, match="missing variables"):
        s.load_state_dict(partial)
    with pytest.raises(ValueError, match="heatmaps/bias"):
        s.load_state_dict(dict(values, **{"heatmaps/bias": np.zeros(17, np.float32)}))
    s.load_state_dict(dict(partial, **{"MobilenetV1/Logits/weights": np.zeros(3, np.float32)}), strict=False)
    np.testing.assert_array_equal(s.state_dict()["heatmaps/bias"], values["heatmaps/bias"])


def test_prn_style_load_ignores_unknown_names_and_holds_variables_only():
    assert prn.PoseResidualNet.ignore_unknown
    shapes = prn.variable_shapes(8, 6, 17, 64)
    s = _PrnStyle(shapes)
    values = _noisy(prn.initial_values(1, h=8, w=6, c=17, hidden=64), 2)
    slots = {f"{k}/Adam": np.ones_like(v) for k, v in values.items()}
    s.load_state_dict(dict(values, global_step=np.int64(3), **slots))
    sd = s.state_dict()
    assert list(sd) == list(shapes) and not s.stats
    for k, v in values.items():
        np.testing.assert_array_equal(sd[k], v, err_msg=k)
    with pytest.raises(KeyError, match="missing variables"):
        s.load_state_dict({k: v for k, v in values.items() if k != "PRN/fc2/biases"})


def test_detector_views_and_state_dict_follow_reference_order_not_arena_order():
    shapes = retinanet.head_variable_shapes(1.0)
    s = _detector()
    assert list(s._train_arena.offsets) != [k for k in shapes if net.is_trainable(k)]      # (the arena is reordered)
    assert list(s.vars) == [k for k in shapes if net.is_trainable(k)]
    assert list(s.stats) == [k for k in shapes if not net.is_trainable(k)]
    values = _noisy(retinanet.initial_head_values(0), 1)
    s.load_state_dict(values)
    sd = s.state_dict()
    assert list(sd) == list(s.vars) + list(s.stats)
    for k, v in values.items():
        np.testing.assert_array_equal(sd[k], v, err_msg=k)


def test_shared_variables_are_the_same_objects_and_move_one_version():
    a = _PrnStyle(prn.variable_shapes(8, 6, 17, 64))
    # every attribute _init_state creates is listed for sharing (a new piece of state cannot be forgotten)
    assert set(vars(a)) - {"device", "dtype", "convs"} == set(model_state.ModelState._SHARED)
    b = _PrnStyle.__new__(_PrnStyle)
    b.share_variables(a)
    for name in model_state.ModelState._SHARED:
        assert getattr(b, name) is getattr(a, name), name
    v = a.var_version
    b.mark_variables_changed()
    assert a.var_version == b.var_version == v + 1


def _digest(arena):
    return hashlib.sha256(repr(list(arena.offsets.items())).encode()).hexdigest()[:16], arena.size


@pytest.mark.parametrize("build,want", [
    (lambda: _keypoint(1.0), (("e9c651a93200e97d", 5521492), ("9e117576e49c3522", 25088))),
    (lambda: _keypoint(0.75), (("c6256074ca114b50", 4070340), ("905c96d739760779", 19648))),
    (_detector, (("64ef80b6ccea8ab5", 2391456), ("26f5a1027142c67b", 6656))),
    (lambda: _PrnStyle(prn.variable_shapes(8, 6, 17, 64)), (("3d64bcc00709d155", 105328), ("4f53cda18c2baa0c", 0))),
], ids=["keypoint-1.0", "keypoint-0.75", "detector-head", "prn"])
def test_arena_layouts_are_unchanged(build, want):
    """Offsets, sizes and order of every arena as the models lay them out (the data-parallel exchange ranges, the detector's
    adjacent tower batch-norm pairs and the adjacent heatmaps kernel + bias depend on them): digests of the layouts."""
    s = build()
    assert (_digest(s._train_arena), _digest(s._stat_arena)) == want
    assert all(o % 4 == 0 for o, _, _ in s._train_arena.offsets.values())
