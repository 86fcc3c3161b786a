"""d2r_pcd_build without a device: everything it refuses before it touches one, the label range of the Python path, and the host
path of get_vis_pcds left as it was."""
import ctypes as C
import inspect

import numpy as np
import pytest

from dream2real_amd import _lib
from dream2real_amd import pcd_visual_model as pvm
from tests import pcd_build_cases as pc

INVALID = -1


def _call(lib, over=(), ctx=None, **kw):
    """d2r_pcd_build on 2 frames of 8 x 6 with a null context unless given; `over` names arguments passed as NULL."""
    n, w, h = kw.get("n", 2), kw.get("w", 8), kw.get("h", 6)
    a = dict(rgb=np.zeros((2, 6, 8, 3), np.uint8), depth=np.ones((2, 6, 8), np.uint16), labels=np.zeros((2, 6, 8), np.uint8),
             poses=np.tile(np.eye(4).reshape(1, 16), (2, 1)), K=np.array([50.0, 0, 4, 0, 50, 3, 0, 0, 1]),
             bounds=np.array(kw.get("bounds", [-1.0, -1, -1, 1, 1, 1]), np.float64), views=np.array(kw.get("views", [0, 1]), np.uint32),
             ids=np.array(kw.get("ids", [0, 1]), np.uint8))
    if "poses" in kw:
        a["poses"] = np.asarray(kw["poses"], np.float64)
    p = {k: (None if k in over else _lib.ptr(v)) for k, v in a.items()}
    out = (C.c_void_p * 4)(*([0xdead] * 4))
    rc = lib.d2r_pcd_build(ctx, p["rgb"], p["depth"], p["labels"], C.c_uint32(n), C.c_uint32(w), C.c_uint32(h), p["poses"], p["K"], p["bounds"],
                           C.c_double(kw.get("voxel", 0.002)), p["views"], C.c_uint32(kw.get("n_views", a["views"].size)), p["ids"],
                           C.c_uint32(kw.get("n_objs", a["ids"].size)), None if "out" in over else out)
    return rc, lib.d2r_last_error(None).decode(), [out[i] for i in range(4)]


def test_refusals_need_no_device():
    lib = _lib.load()
    for name in ("rgb", "depth", "labels", "poses", "K", "bounds", "views", "ids", "out"):
        rc, msg, _ = _call(lib, over=(name,))
        assert rc == INVALID and "null argument" in msg, name
    for kw in (dict(n=0), dict(w=0), dict(h=0), dict(n_views=0), dict(n_objs=0)):
        rc, msg, out = _call(lib, **kw)
        assert rc == INVALID and "at least" in msg, kw
    rc, msg, out = _call(lib, views=[0, 2])
    assert rc == INVALID and "view index 2" in msg and out[:2] == [None, None]
    rc, msg, _ = _call(lib, ids=[3, 3])
    assert rc == INVALID and "twice" in msg
    for voxel in (-0.002, float("nan"), float("inf")):
        rc, msg, _ = _call(lib, voxel=voxel)
        assert rc == INVALID and "voxel" in msg
    bad = np.tile(np.eye(4).reshape(1, 16), (2, 1))
    bad[1, 7] = np.inf
    rc, msg, _ = _call(lib, poses=bad)
    assert rc == INVALID and "poses" in msg
    # all of it in order and no context: the last thing asked for
    rc, msg, out = _call(lib)
    assert rc == INVALID and "null context" in msg and out[:2] == [None, None] and out[2] == 0xdead


def test_the_21_bit_refusal():
    """extent / voxel + 2 must stay below 2^21 on every axis: 4194.3 m at 0.002 does not, 4194.2 m does (and then fails on the
    missing context, the next check)."""
    lib = _lib.load()
    for axis in range(3):
        b = [-1.0, -1, -1, 1, 1, 1]
        b[3 + axis] = b[axis] + 0.002 * (2 ** 21 - 2)
        rc, msg, _ = _call(lib, bounds=b)
        assert rc == INVALID and "21 bits" in msg and msg.endswith(str(axis)), (axis, msg)
        b[3 + axis] = b[axis] + 0.002 * (2 ** 21 - 3)
        rc, msg, _ = _call(lib, bounds=b)
        assert rc == INVALID and "null context" in msg
    b = [-1.0, -1, -1, np.inf, 1, 1]
    assert _call(lib, bounds=b)[0] == INVALID and "21 bits" in _call(lib, bounds=b)[1]
    rc, msg, _ = _call(lib, bounds=b, voxel=0.0)                # without voxels there is no index to fit
    assert "null context" in msg
    n = C.c_uint32(7)
    assert lib.d2r_pcd_size(None, C.byref(n)) == INVALID and lib.d2r_pcd_read(None, None, None, None) == INVALID
    assert lib.d2r_pcd_build_get_timing(None, None) == INVALID


def test_labels_above_255_are_a_value_error():
    c = pc.case(40, 30)
    labels = [m.copy() for m in c["labels"]]
    labels[1][0, 0] = 256
    with pytest.raises(ValueError, match="0 .. 255"):
        pvm.get_vis_pcds(c["rgbs"], c["depths"], list(c["poses"]), c["K"], labels, 3, c["bounds"], use_cache=False, ctx=object())
    labels[1][0, 0] = -1
    with pytest.raises(ValueError, match="0 .. 255"):
        pvm.get_vis_pcds(c["rgbs"], c["depths"], list(c["poses"]), c["K"], labels, 3, c["bounds"], use_cache=False, ctx=object())


def test_host_path_without_a_context_is_unchanged():
    p = inspect.signature(pvm.get_vis_pcds).parameters["ctx"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    K = np.array([[30.0, 0, 15.5], [0, 31.0, 11.5], [0, 0, 1]])
    depth = np.full((24, 32), 0.8, np.float32)
    depth[5:15, 10:25] = 0.5
    rgb = np.zeros((24, 32, 3), np.uint8)
    rgb[..., 0] = np.arange(32, dtype=np.uint8)[None] * 5
    rgb[..., 1] = np.arange(24, dtype=np.uint8)[:, None] * 7
    masks = np.zeros((24, 32), np.int64)
    masks[2:22, 5:30] = 1
    T0, T1 = np.eye(4), np.eye(4)
    T1[:3, 3] = [0.01, 0, 0]
    bounds = [[-1, -1, 0], [1, 1, 0.6]]
    c = dict(rgbs=[rgb, rgb], depths=[depth, depth], labels=np.stack([masks, masks]), poses=np.stack([T0, T1]), K=K, bounds=bounds)
    args = (c["rgbs"], c["depths"], [T0, T1], K, [masks, masks], 2, bounds)
    for pcds_type, views, voxel in ((0, (1,), 0.0), (1, (0, 1), pvm.FRAME_VOXEL_SIZE)):
        got = pvm.get_vis_pcds(*args, use_cache=False, pcds_type=pcds_type, single_view_idx=1)
        want = pc.host_clouds(pc.host_segments(c, voxel, views=views, obj_ids=(0, 1)))
        assert len(got[1]) > 0
        for g, (wx, wc) in zip(got, want):
            np.testing.assert_array_equal(g.xyz, wx)
            np.testing.assert_array_equal(g.rgb, wc)
