"""CPU-only checks of the 2-D point-mass path: the nine 2-D scene classes exist with the reference's constructor defaults and limits,
pack into the primitive tables recorded from the reference (tests/golden/scenes_2d.npz), and the C ABI rejects a bad 2-D scene
descriptor before any device work."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import torch_robotics_amd as tra
from helpers import gold
from torch_robotics_amd import _abi, _lib
from torch_robotics_amd.environments import EnvBase, planar_tables

CPU = dict(device=torch.device("cpu"), dtype=torch.float32)
NAMES = ["EnvSimple2D", "EnvDense2D", "EnvNarrowPassageDense2D", "EnvSquare2D", "EnvCircle2D", "EnvGridCircles2D",
         "EnvSimple2DExtraObjects", "EnvDense2DExtraObjects", "EnvNarrowPassageDense2DExtraObjects"]
# the reference's per-scene defaults (grid on by default, default cell size) and constructor names
DEFAULTS = {"EnvSimple2D": (True, "EnvDense2D"), "EnvDense2D": (True, "EnvDense2D"), "EnvNarrowPassageDense2D": (False, "EnvDense2D"),
            "EnvSquare2D": (False, "EnvSquare2D"), "EnvCircle2D": (True, "EnvDense2D"), "EnvGridCircles2D": (False, "EnvGridCircles2D"),
            "EnvSimple2DExtraObjects": (True, "EnvSimple2DExtraObjects"), "EnvDense2DExtraObjects": (True, "EnvDense2DExtraObjects"),
            "EnvNarrowPassageDense2DExtraObjects": (False, "EnvNarrowPassageDense2DExtraObjects")}


def default_of(cls, arg):
    for c in cls.__mro__:
        p = inspect.signature(c.__init__).parameters
        if arg in p:
            return p[arg].default
        if c is EnvBase:
            break
    raise AssertionError(arg)


@pytest.fixture(scope="module")
def scenes():
    return gold("scenes_2d")


@pytest.mark.parametrize("name", NAMES)
def test_scene_class_defaults_and_limits(name, scenes):
    cls = getattr(tra, name)
    on, env_name = DEFAULTS[name]
    assert default_of(cls, "precompute_sdf_obj_fixed") == on == bool(scenes[f"{name}/grid_on"])
    assert np.float32(default_of(cls, "sdf_cell_size")) == scenes[f"{name}/cell"]
    env = cls(tensor_args=CPU, precompute_sdf_obj_fixed=False)
    assert env.name == env_name and env.dim == 2 and env.grid_map_sdf_obj_fixed is None
    np.testing.assert_array_equal(env.limits_np, scenes[f"{name}/limits"])


@pytest.mark.parametrize("name", NAMES)
def test_scene_packs_into_the_recorded_tables(name, scenes):
    """The kernels' host tables -- object poses, rows (type, cx, cy, hx, hy, r) -- from the reference's recorded fields: half sizes
    sizes / 2, rounding radius 0.15 * min size, fixed objects before the extra objects."""
    env = getattr(tra, name)(tensor_args=CPU, precompute_sdf_obj_fixed=False)
    objs = list(env.obj_fixed_list or []) + list(env.obj_extra_list or [])
    assert [int(o in (env.obj_extra_list or [])) for o in objs] == scenes[f"{name}/obj_extra"].tolist()
    objects, prims = planar_tables(objs)
    fields, rec = scenes[f"{name}/fields"], scenes[f"{name}/prims"]
    assert len(prims) == len(rec) == int(fields[:, 3].sum())
    kinds = np.repeat(fields[:, 2], fields[:, 3])
    expect_type = np.array([{0: _abi.PRIM_SPHERE, 1: _abi.PRIM_ROUNDED_BOX, 2: _abi.PRIM_SHARP_BOX}[int(k)] for k in kinds])
    np.testing.assert_array_equal(prims[:, 0], expect_type)
    np.testing.assert_array_equal(prims[:, 1:3], rec[:, :2])
    sph = kinds == 0
    np.testing.assert_array_equal(prims[sph, 5], rec[sph, 2])
    np.testing.assert_array_equal(prims[~sph, 3:5], rec[~sph, 2:4] / np.float32(2))
    rounded = kinds == 1
    np.testing.assert_array_equal(prims[rounded, 5], rec[rounded, 2:4].min(1) * np.float32(0.15))
    for k, (pos, R, b, e) in enumerate(objects):
        np.testing.assert_array_equal(pos, scenes[f"{name}/obj_pos"][k])
        np.testing.assert_array_equal(R, np.eye(3, dtype=np.float32))         # every recorded scene object has the identity pose
        assert (b, e) == (int(fields[fields[:, 0] == k, 3].sum() and fields[fields[:, 0] < k, 3].sum()),
                          int(fields[fields[:, 0] <= k, 3].sum()))


def test_scene_table_missing_is_a_clear_error(monkeypatch, tmp_path):
    from torch_robotics_amd import environments
    monkeypatch.setattr(environments, "SCENES_2D_PATH", tmp_path / "absent.npz")
    monkeypatch.setattr(environments, "_scenes_2d", None)
    with pytest.raises(FileNotFoundError, match="scenes_2d.npz|absent.npz"):
        tra.EnvDense2D(tensor_args=CPU, precompute_sdf_obj_fixed=False)


def test_point_mass_task_is_2d():
    robot = tra.RobotPointMass(tensor_args=CPU)
    task = tra.PlanningTask(env=tra.EnvNarrowPassageDense2D(tensor_args=CPU), robot=robot, tensor_args=CPU)
    assert task._planar and robot.q_dim == 2 and robot.df_collision_self is None
    np.testing.assert_array_equal(task.df_collision_objects._margin_vector(1), np.float32(0.01) + np.float32(0.01))


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def _desc():
    d = _abi.Scene2DDesc()
    d.abi_version = _abi.TRK_ABI_VERSION
    objs = (_abi.Object2D * 1)()
    objs[0].R = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    objs[0].prim_begin, objs[0].prim_end = 0, 1
    prims = (_abi.Prim2D * 1)()
    prims[0].type, prims[0].radius = _abi.PRIM_SPHERE, 0.2
    d.n_objects, d.objects, d.n_prims, d.prims = 1, objs, 1, prims
    d.margin = 0.02
    return d, (objs, prims)


def test_scene2d_descriptor_validation_without_gpu(trk):
    """Every malformed descriptor is refused with a status before any device work (no GPU needed to see it)."""
    h = C.c_void_p()
    assert trk.trk_scene2d_create(None, C.byref(h)) == _abi.TRK_ERR_INVALID_ARG
    d, keep = _desc()
    d.abi_version = 99
    assert trk.trk_scene2d_create(C.byref(d), C.byref(h)) == _abi.TRK_ERR_INVALID_ARG
    d, keep = _desc()
    keep[0][0].prim_end = 5                                     # past n_prims
    assert trk.trk_scene2d_create(C.byref(d), C.byref(h)) == _abi.TRK_ERR_INVALID_ARG
    assert b"primitive range" in trk.trk_last_error()
    d, keep = _desc()
    keep[1][0].type = 7
    assert trk.trk_scene2d_create(C.byref(d), C.byref(h)) == _abi.TRK_ERR_INVALID_ARG
    d, keep = _desc()
    d.n_objects = _abi.TRK_PLANAR_MAX_OBJECTS + 1
    assert trk.trk_scene2d_create(C.byref(d), C.byref(h)) == _abi.TRK_ERR_UNSUPPORTED
    d, keep = _desc()
    d.has_grid = 1                                              # no cells, no dims
    assert trk.trk_scene2d_create(C.byref(d), C.byref(h)) == _abi.TRK_ERR_INVALID_ARG
    d, keep = _desc()
    d.margin = float("nan")
    assert trk.trk_scene2d_create(C.byref(d), C.byref(h)) == _abi.TRK_ERR_INVALID_ARG
    assert not h.value
    # the launch entry points refuse a null scene / bad sizes the same way
    assert trk.trk_scene2d_cost_grad(None, None, 4, 0, None, None, None) == _abi.TRK_ERR_INVALID_ARG
    assert trk.trk_scene2d_collision(None, None, -1, float("nan"), None, None) == _abi.TRK_ERR_INVALID_ARG
    assert trk.trk_scene2d_collision_via(None, None, 1, 1, 2, 5, None, None, 0.0, None, None) == _abi.TRK_ERR_INVALID_ARG
    assert trk.trk_grid2d_precompute(None, None, None, None, None, None) == _abi.TRK_ERR_INVALID_ARG
    assert trk.trk_scene2d_sdf_points(None, None, 1, None, None, None) == _abi.TRK_ERR_INVALID_ARG


def test_scene2d_struct_layouts_match_header():
    import subprocess
    import tempfile
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    src = '#include <stdio.h>\n#include "trk.h"\nint main(){printf("%zu %zu %zu\\n",sizeof(TrkPrim2D),sizeof(TrkObject2D),sizeof(TrkScene2DDesc));}'
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.run(["gcc", "-I", str(root / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")], check=True)
        out = subprocess.run([str(Path(d) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(t) for t in (_abi.Prim2D, _abi.Object2D, _abi.Scene2DDesc)]
