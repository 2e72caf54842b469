"""Scene description: analytic SDF primitives, posed objects, voxel SDF grid, 3-D and 2-D scenes.

Mirrors the data side of `torch_robotics/environments/` (primitives.py, grid_map_sdf.py,
env_base.py, env_spheres_3d.py, env_table_shelf.py, env_maze_boxes_3d.py,
env_spheres_3d_extra_objects.py, and the nine 2-D scenes env_*_2d*.py).  Objects hold plain numbers; every distance evaluation goes to
the HIP kernels through a `CostHandle` (there is no torch arithmetic here).
"""
from __future__ import annotations

import itertools
from copy import copy
from pathlib import Path
from typing import List

import numpy as np
import torch

from . import _abi, ops
from .costmodel import panda_box_base_points, CostModelSpec, box_prims, grid_object, make_object, sphere_prims
from .kinmodel import quat_wxyz_to_rot

DEFAULT_TENSOR_ARGS = {"device": torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"),
                       "dtype": torch.float32}


def _np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


_version_counter = itertools.count(1)


def scene_version(df_obj_list) -> tuple:
    """What a device cost model built from these objects depends on: identity AND pose version of every ObjectField, identity
    of a grid's tensors.  The reference evaluates each object from its current pose on every call (primitives.py:387-405), so
    every cache of a `CostHandle` is keyed by this and a moved object rebuilds it.  Integers only -- this runs on every cost
    evaluation: an ObjectField takes a fresh version number whenever `pos` / `ori` are assigned (`set_position_orientation`
    or the attributes).  The pose arrays and the primitives' centre / radius / size arrays are read-only (`obj.pos[0] = ...`,
    `field.centers[0] = ...` raise: assign a new array or call `set_position_orientation`), and the key carries the version number
    of every primitive field's latest geometry assignment, so a re-assigned `field.centers` rebuilds the device model as well."""
    return tuple((id(o), id(o.sdf_tensor)) if isinstance(o, GridMapSDF)
                 else (id(o), o._version) + tuple(k for f in o.fields for k in f.array_ids()) for o in df_obj_list)


class PrimitiveShapeField:
    def __init__(self, dim=3, tensor_args=None):
        self.dim = dim
        self.tensor_args = DEFAULT_TENSOR_ARGS if tensor_args is None else tensor_args

    def prims(self) -> List[dict]:
        raise NotImplementedError

    _ARRAYS = ()

    def __setattr__(self, name, value):
        # the geometry arrays are read-only copies: an in-place edit raises instead of leaving a stale device model behind
        if name in self._ARRAYS:
            value = np.array(value, dtype=np.float32)
            value.setflags(write=False)
            object.__setattr__(self, "_geometry_version", next(_version_counter))
        object.__setattr__(self, name, value)

    def array_ids(self) -> tuple:
        """what scene_version adds for this field: the number its latest geometry assignment took"""
        return (getattr(self, "_geometry_version", 0),)

    @ops.host_round_trip
    def compute_signed_distance(self, x):
        return ObjectField([self]).compute_signed_distance(x)


class MultiSphereField(PrimitiveShapeField):                 # primitives.py:88-121
    _ARRAYS = ("centers", "radii")

    def __init__(self, centers, radii, tensor_args=None):
        centers = _np(centers).astype(np.float32)
        super().__init__(dim=centers.shape[-1], tensor_args=tensor_args)
        self.centers, self.radii = centers.reshape(-1, self.dim), _np(radii).astype(np.float32).reshape(-1)

    def prims(self):
        c = self.centers if self.dim == 3 else np.concatenate([self.centers, np.zeros((len(self.centers), 1), np.float32)], 1)
        return sphere_prims(c, self.radii)

    def prims2d(self) -> np.ndarray:
        """rows (type, cx, cy, hx, hy, radius) of the 2-D kernels (csrc/trk_planar.hip)"""
        c, r = self.centers.reshape(-1, 2), self.radii.reshape(-1)
        z = np.zeros(len(c), np.float32)
        return np.stack([np.full(len(c), _abi.PRIM_SPHERE, np.float32), c[:, 0], c[:, 1], z, z, r], 1).astype(np.float32)


class MultiSharpBoxField(PrimitiveShapeField):               # primitives.py:197-228
    rounded = False
    _ARRAYS = ("centers", "sizes", "half_sizes", "radius")

    def __init__(self, centers, sizes, tensor_args=None):
        centers = _np(centers).astype(np.float32)
        super().__init__(dim=centers.shape[-1], tensor_args=tensor_args)
        self.centers, self.sizes = centers.reshape(-1, self.dim), _np(sizes).astype(np.float32).reshape(-1, self.dim)
        self.half_sizes = self.sizes / np.float32(2)

    def prims(self):
        if self.dim != 3:
            raise NotImplementedError("2-D boxes enter the 2-D scene tables (prims2d), not a 3-D cost model")
        return box_prims(self.centers, self.sizes, rounded=self.rounded)

    def prims2d(self) -> np.ndarray:
        """rows (type, cx, cy, hx, hy, radius): half sizes sizes / 2 and, rounded, radius 0.15 * min size, in fp32 (primitives.py:212, 321)"""
        c, h = self.centers.reshape(-1, 2), self.half_sizes.reshape(-1, 2)
        r = self.radius.reshape(-1) if self.rounded else np.zeros(len(c), np.float32)
        t = _abi.PRIM_ROUNDED_BOX if self.rounded else _abi.PRIM_SHARP_BOX
        return np.stack([np.full(len(c), t, np.float32), c[:, 0], c[:, 1], h[:, 0], h[:, 1], r], 1).astype(np.float32)


class MultiBoxField(MultiSharpBoxField):                     # rounded boxes, primitives.py:304-334
    rounded = True

    def __init__(self, centers, sizes, tensor_args=None):
        super().__init__(centers, sizes, tensor_args=tensor_args)
        self.radius = self.sizes.min(-1) * np.float32(0.15)


MultiRoundedBoxField = MultiBoxField


class _SDFPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cm):
        sdf, grad = ops.sdf_points(cm, x, want_grad=True)
        ctx.save_for_backward(grad)
        return sdf

    @staticmethod
    def backward(ctx, gs):
        (grad,) = ctx.saved_tensors
        return (gs.unsqueeze(-1) * grad).sum(1), None


class _SDFPoints2D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scene):
        sdf, grad = ops.planar_sdf_points(scene, x, want_grad=True)
        ctx.save_for_backward(grad)
        return sdf

    @staticmethod
    def backward(ctx, gs):
        (grad,) = ctx.saved_tensors
        return (gs.unsqueeze(-1) * grad).sum(1), None


def _planar_sdf(scene, x):
    """per-df-object signed distances (N, n_df) of points x (..., 2), differentiable w.r.t. x"""
    flat = x.reshape(-1, 2)
    if torch.is_grad_enabled() and x.requires_grad:
        return _SDFPoints2D.apply(flat.contiguous(), scene)
    return ops.planar_sdf_points(scene, flat)


def planar_tables(obj_list):
    """The 2-D kernels' host tables of ObjectFields: ([(pos, R, prim_begin, prim_end)], prims (k, 6) float32)."""
    objects, rows, k = [], [], 0
    for o in obj_list:
        p = np.concatenate([f.prims2d() for f in o.fields], 0) if o.fields else np.zeros((0, 6), np.float32)
        objects.append((o.pos, quat_wxyz_to_rot(o.ori), k, k + len(p)))
        rows.append(p)
        k += len(p)
    return objects, (np.concatenate(rows, 0) if rows else np.zeros((0, 6), np.float32))


def planar_scene(df_obj_list, device, ws=None, margin=0.0) -> "ops.Scene2DHandle":
    """A 2-D scene handle of df objects in the order of EnvBase.get_df_obj_list: at most one GridMapSDF, first, then ObjectFields."""
    grid = None
    objs = list(df_obj_list)
    if objs and isinstance(objs[0], GridMapSDF):
        grid = objs.pop(0).planar_grid(device)
    if any(isinstance(o, GridMapSDF) for o in objs):
        raise NotImplementedError("a 2-D scene evaluates one SDF grid, ahead of its analytic objects (EnvBase.get_df_obj_list's order)")
    objects, prims = planar_tables(objs)
    return ops.Scene2DHandle(objects, prims, ops.compute_device(device), grid=grid, ws=ws, margin=margin)


class ObjectField(PrimitiveShapeField):                      # primitives.py:346-420
    def __init__(self, primitive_fields, name="object", pos=None, ori=None, reference_frame="base"):
        assert primitive_fields is not None and isinstance(primitive_fields, list)
        super().__init__(dim=primitive_fields[0].dim, tensor_args=primitive_fields[0].tensor_args)
        self.name, self.fields, self.reference_frame = name, primitive_fields, reference_frame
        assert (pos is None and ori is None) or (np.size(_np(pos)) == 3 and np.size(_np(ori)) == 4)
        self.pos = np.zeros(3, np.float32) if pos is None else pos
        self.ori = np.array([1, 0, 0, 0], np.float32) if ori is None else ori

    # pose attributes: every assignment takes a new version number (scene_version) and drops the object's own cost model
    @property
    def pos(self):
        return self._pos

    @pos.setter
    def pos(self, value):
        self._pos = _np(value).astype(np.float32).reshape(3)
        self._pos.setflags(write=False)     # an in-place edit would not be seen by scene_version: it raises instead (assign a new pose)
        self._version, self._cm = next(_version_counter), None

    @property
    def ori(self):
        return self._ori

    @ori.setter
    def ori(self, value):
        self._ori = _np(value).astype(np.float32).reshape(4)
        self._ori.setflags(write=False)
        self._version, self._cm = next(_version_counter), None

    def set_position_orientation(self, pos=None, ori=None):
        if pos is not None:
            assert len(pos) == 3
            self.pos = pos
        if ori is not None:
            assert len(ori) == 4, "quaternion wxyz"
            self.ori = ori

    def as_object(self) -> dict:
        prims = list(itertools.chain.from_iterable(f.prims() for f in self.fields))
        return make_object(prims, self.pos, quat_wxyz_to_rot(self.ori))

    @ops.host_round_trip
    def compute_signed_distance(self, x):
        """x (..., 3) -- or (..., 2) for a 2-D object -- on the GPU -> (...) signed distance (differentiable w.r.t. x)."""
        if self.dim == 2:
            key = ("2d", x.device, self._version) + tuple(k for f in self.fields for k in f.array_ids())
            if self._cm is None or self._cm_key != key:
                self._cm, self._cm_key = planar_scene([self], x.device), key
            return _planar_sdf(self._cm, x).reshape(x.shape[:-1])
        # keyed by the device, the pose version AND the primitive fields' geometry versions: `field.centers = new` must be seen here
        key = (x.device, self._version) + tuple(k for f in self.fields for k in f.array_ids())
        if self._cm is None or self._cm_key != key:
            self._cm = ops.CostHandle(CostModelSpec(n_links_in=1, objects=[self.as_object()]), x.device)
            self._cm_key = key
        flat = x.reshape(-1, 3)
        if torch.is_grad_enabled() and x.requires_grad:
            return _SDFPoints.apply(flat.contiguous(), self._cm).reshape(x.shape[:-1])
        return ops.sdf_points(self._cm, flat).reshape(x.shape[:-1])

    compute_signed_distance_impl = compute_signed_distance


class GraspedObject(ObjectField):                             # objects.py:10-34
    """An object rigidly held by the end effector; pos / ori are relative to `reference_frame` (a robot link)."""

    def __init__(self, primitive_fields, **kwargs):
        assert len(primitive_fields) == 1                       # only one primitive type
        super().__init__(primitive_fields, **kwargs)
        if not isinstance(primitive_fields[0], MultiBoxField):
            raise NotImplementedError                           # objects.py:29-30
        self.geometry_size = primitive_fields[0].sizes[0]

    def get_base_points_for_collision(self):
        raise NotImplementedError


class GraspedObjectPandaBox(GraspedObject):                  # objects.py:37-89
    def __init__(self, tensor_args=None, **kwargs):
        fields = [MultiBoxField(np.zeros((1, 3), np.float32), np.array([[0.05, 0.05, 0.15]], np.float32), tensor_args=tensor_args)]
        super().__init__(fields, name="GraspedObjectPandaBox", pos=np.array([0.0, 0.0, 0.11], np.float32),
                         ori=np.array([0, 0.7071081, 0, 0.7071055], np.float32), reference_frame="panda_hand", **kwargs)
        self.base_points_for_collision = self.get_base_points_for_collision()
        self.n_base_points_for_collision = len(self.base_points_for_collision)

    def get_base_points_for_collision(self):
        """The 8 vertices and 6 face centres of the box, in the object frame (objects.py:57-89), fp32."""
        return torch.from_numpy(panda_box_base_points(self.fields[0].sizes[0]))


class GridMapSDF:                                            # grid_map_sdf.py:9-117
    """Voxel SDF + stored gradients; built by the `trk_grid_precompute` kernel."""

    def __init__(self, limits, cell_size, obj_list, tensor_args=None):
        self.tensor_args = DEFAULT_TENSOR_ARGS if tensor_args is None else tensor_args
        self.limits = torch.as_tensor(_np(limits), dtype=torch.float32)
        self.dim = self.limits.shape[-1]
        if self.dim not in (2, 3):
            raise NotImplementedError("GridMapSDF: 2-D and 3-D grids only")
        self.obj_list = obj_list
        self.cell_size = cell_size
        map_dim = torch.abs(self.limits[1] - self.limits[0])                  # fp32, as grid_map_sdf.py:24-27
        self.map_dim = map_dim
        self.cmap_dim = torch.ceil(map_dim / cell_size).to(torch.int64)
        self.sdf_tensor = None
        self.grad_sdf_tensor = None
        self.precompute_sdf()

    def precompute_sdf(self):
        if self.dim == 2:
            # one float4 (sdf, gx, gy, 0) per cell (trk_grid2d_precompute): a lookup is one 16-byte gather; the reference-shaped
            # sdf_tensor (nx, ny) / grad_sdf_tensor (nx, ny, 2) are views of it
            dev = ops.compute_device(self.tensor_args["device"])
            self.cells = ops.grid2d_precompute(planar_scene(self.obj_list, dev), self.cmap_dim.numpy(), self.limits[0].numpy(),
                                               self.limits[1].numpy())
            self.sdf_tensor, self.grad_sdf_tensor = self.cells[..., 0], self.cells[..., 1:3]
            return
        spec = CostModelSpec(n_links_in=1, objects=[o.as_object() for o in self.obj_list])
        cm = ops.CostHandle(spec, ops.compute_device(self.tensor_args["device"]))      # the grid lives where it is computed and queried: on the GPU
        self.sdf_tensor, self.grad_sdf_tensor = ops.grid_precompute(
            cm, self.cmap_dim.numpy(), self.limits[0].numpy(), self.limits[1].numpy())

    def planar_grid(self, device) -> dict:
        """the grid of a 2-D scene handle (ops.Scene2DHandle)"""
        if self.dim != 2:
            raise NotImplementedError("a 3-D grid enters a 3-D cost model (grid_dict)")
        return dict(cells=self.cells.to(ops.compute_device(device)), lim_min=self.limits[0].numpy(), map_dim=self.map_dim.numpy())

    def grid_dict(self) -> dict:
        return dict(dims=self.cmap_dim.numpy().astype(np.int32), lim_min=self.limits[0].numpy(),
                    map_dim=self.map_dim.numpy(), sdf=self.sdf_tensor, grad=self.grad_sdf_tensor)

    def _query_handle(self, device):
        if getattr(self, "_qcm", None) is None or self._qcm.device != torch.device(device):
            spec = CostModelSpec(n_links_in=1, objects=[grid_object()])
            spec.grid = self.grid_dict()
            self._qcm = ops.CostHandle(spec, device)
        return self._qcm

    @ops.host_round_trip
    def compute_signed_distance(self, X, **kwargs):           # grid_map_sdf.py:81-114
        """Nearest-lower-cell lookup; differentiable w.r.t. X with the STORED gradient of that cell, like the reference's
        `sdf[idx] + (X * g).sum() - (X.detach() * g).sum()`."""
        if self.dim == 2:
            if getattr(self, "_q2d", None) is None or self._q2d[0] != str(X.device):
                self._q2d = (str(X.device), planar_scene([self], X.device))
            return _planar_sdf(self._q2d[1], X).reshape(X.shape[:-1])
        cm = self._query_handle(X.device)
        flat = X.reshape(-1, 3)
        if torch.is_grad_enabled() and X.requires_grad:
            return _SDFPoints.apply(flat.contiguous(), cm).reshape(X.shape[:-1])
        return ops.sdf_points(cm, flat).reshape(X.shape[:-1])

    __call__ = compute_signed_distance


class EnvBase:                                               # env_base.py:17-100
    def __init__(self, name="NameEnvBase", limits=None, obj_fixed_list=None, obj_extra_list=None,
                 precompute_sdf_obj_fixed=False, sdf_cell_size=0.005, tensor_args=None, **kwargs):
        self.tensor_args = DEFAULT_TENSOR_ARGS if tensor_args is None else tensor_args
        self.name = name
        assert limits is not None
        self.limits_np = _np(limits).astype(np.float32)
        self.limits = torch.as_tensor(self.limits_np, **self.tensor_args)
        self.dim = len(self.limits_np[0])
        for lst in (obj_fixed_list, obj_extra_list):
            for obj in lst or []:
                assert isinstance(obj, ObjectField), "Objects must be instances of ObjectField class"
        self.obj_fixed_list, self.obj_extra_list = obj_fixed_list, obj_extra_list
        self.obj_all_list = list(itertools.chain(obj_fixed_list or [], obj_extra_list or []))
        self.grid_map_sdf_obj_fixed = None
        if precompute_sdf_obj_fixed:
            self.grid_map_sdf_obj_fixed = GridMapSDF(self.limits_np, sdf_cell_size, self.obj_fixed_list,
                                                     tensor_args=self.tensor_args)

    def get_obj_list(self):
        return self.obj_all_list

    def get_df_obj_list(self, return_extra_objects_only=False):          # env_base.py:75-88
        out = []
        if not return_extra_objects_only:
            if self.grid_map_sdf_obj_fixed is not None:
                out.append(self.grid_map_sdf_obj_fixed)
            else:
                out.extend(self.obj_fixed_list or [])
        if self.obj_extra_list is not None:
            out.extend(self.obj_extra_list)
        return out

    @ops.host_round_trip
    def compute_sdf(self, x, reshape_shape=None):             # env_base.py:140-169
        """Signed distance of the scene (min over the fixed objects -- or their precomputed grid -- and the extra objects) at
        points x (..., 3); differentiable w.r.t. x.  One `trk_sdf_points` launch for all objects."""
        objs = self.get_df_obj_list()
        if not objs:
            return None
        if self.dim == 2:
            # the per-object distances come from one kernel launch; the reference folds them with torch.minimum (ties share the
            # gradient), which is what is done with them here
            key = ("2d", str(x.device), scene_version(objs))
            if getattr(self, "_sdf_cm", None) is None or self._sdf_cm[0] != key:
                self._sdf_cm = (key, planar_scene(objs, x.device))
            per_obj = _planar_sdf(self._sdf_cm[1], x)
            sdf = per_obj[:, 0]
            for k in range(1, per_obj.shape[1]):
                sdf = torch.minimum(sdf, per_obj[:, k])
            return sdf.reshape(reshape_shape) if reshape_shape else sdf.reshape(x.shape[:-1])
        key = (str(x.device), scene_version(objs))
        if getattr(self, "_sdf_cm", None) is None or self._sdf_cm[0] != key:
            spec = CostModelSpec(n_links_in=1)
            spec.objects, spec.grid = objects_to_spec_parts(objs)
            self._sdf_cm = (key, ops.CostHandle(spec, x.device))
        cm = self._sdf_cm[1]
        flat = x.reshape(-1, 3)
        if torch.is_grad_enabled() and x.requires_grad:
            per_obj = _SDFPoints.apply(flat.contiguous(), cm)
        else:
            per_obj = ops.sdf_points(cm, flat)
        sdf = per_obj.reshape(flat.shape[0], -1).min(dim=1).values
        return sdf.reshape(reshape_shape) if reshape_shape else sdf.reshape(x.shape[:-1])

    def add_obj(self, obj):                                   # env_base.py:90-92
        raise NotImplementedError

    def zero_grad(self):
        pass


def objects_to_spec_parts(df_obj_list):
    """[ObjectField | GridMapSDF, ...] -> (objects list, grid dict or None) for a CostModelSpec."""
    objects, grid = [], None
    for df in df_obj_list:
        if isinstance(df, GridMapSDF):
            objects.append(grid_object())
            grid = df.grid_dict()
        else:
            objects.append(df.as_object())
    return objects, grid


class EnvSpheres3D(EnvBase):                                 # env_spheres_3d.py:11-49 (scene data)
    def __init__(self, name="EnvDense2D", tensor_args=None, **kwargs):
        centers = np.array([[-0.3, 0.3, 0.85], [-0.35, -0.25, 0.45], [-0.45, 0.15, 0.0], [0.45, 0.35, 0.0],
                            [0.55, 0.35, 0.55], [0.65, -0.4, 0.25], [0.2, -0.35, 0.5], [0.35, 0.0, 0.9],
                            [0.0, -0.3, 0.0], [0.0, 0.45, 0.35]], np.float32)
        spheres = MultiSphereField(centers, np.full(10, 0.15, np.float32), tensor_args=tensor_args)
        super().__init__(name=name, limits=np.array([[-1, -1, -1], [1, 1, 1]], np.float32),
                         obj_fixed_list=[ObjectField([spheres], "spheres")], tensor_args=tensor_args, **kwargs)


class EnvSpheres3DExtraObjects(EnvSpheres3D):               # env_spheres_3d_extra_objects.py:12-58
    def __init__(self, tensor_args=None, **kwargs):
        extra = MultiSphereField(np.array([[0.25, 0.0, 0.0], [0.0, 0.5, 0.5], [0.0, -0.5, 0.0], [-0.25, -0.5, 0.5],
                                           [-0.25, 0.0, 0.75]]), np.full(5, 0.15), tensor_args=tensor_args)
        super().__init__(name=self.__class__.__name__, obj_extra_list=[ObjectField([extra], "extra-objects")],
                         tensor_args=tensor_args, **kwargs)


def create_table_object_field(tensor_args=None):             # env_table_shelf.py:14-20
    return ObjectField([MultiBoxField(np.array([(0.0, 0.0, 0.0)]), np.array([(0.56, 0.90, 0.80)]), tensor_args=tensor_args)], "table")


def create_shelf_field(tensor_args=None):                    # env_table_shelf.py:23-69
    width, height, depth, side = 0.80, 2.05, 0.28, 0.02
    shelf_width, shelf_height, shelf_depth = width - 2 * side, 0.015, depth
    centers = [(side / 2, depth / 2, height / 2)]
    sizes = [(side, depth, height)]
    centers.append((side + shelf_width + side / 2, depth / 2, height / 2)); sizes.append((side, depth, height))
    centers.append((side + shelf_width / 2, depth + side / 2, height / 2)); sizes.append((shelf_width, side, height))
    centers.append((side + shelf_width / 2, depth / 2, shelf_height / 2)); sizes.append((shelf_width, shelf_depth, shelf_height))
    centers.append((side + shelf_width / 2, depth / 2, height - shelf_height / 2)); sizes.append((shelf_width, shelf_depth, shelf_height))
    centers.append((side + shelf_width / 2, depth / 2, 0.82 + shelf_height / 2)); sizes.append((shelf_width, shelf_depth, shelf_height))
    for plus_height in [0.23, 0.255, 0.225, 0.225]:
        center = list(copy(centers[-1]))
        center[-1] += plus_height
        centers.append(center); sizes.append((shelf_width, shelf_depth, shelf_height))
    return ObjectField([MultiBoxField(np.array(centers), np.array(sizes), tensor_args=tensor_args)], "shelf")


class EnvTableShelf(EnvBase):                                # env_table_shelf.py:72-102
    def __init__(self, tensor_args=None, **kwargs):
        table = create_table_object_field(tensor_args)
        ts = table.fields[0].sizes[0]
        d_table, theta = 0.10, np.deg2rad(90)
        table.set_position_orientation(pos=(d_table + ts[1].item() / 2, 0, -ts[2].item() / 2),
                                       ori=[np.cos(theta / 2), 0, 0, np.sin(theta / 2)])
        shelf = create_shelf_field(tensor_args)
        shelf.set_position_orientation(pos=(d_table, 0.15 + ts[0].item() / 2, -ts[2].item()))
        super().__init__(name=self.__class__.__name__, limits=np.array([[-1, -1, -1], [1.5, 1.0, 1.5]], np.float32),
                         obj_fixed_list=[table, shelf], tensor_args=tensor_args, **kwargs)


def create_3d_rectangles_objects(tensor_args=None):          # env_maze_boxes_3d.py:11-52
    hs = 0.2
    rects = [(-0.75, -1.0, -0.75 + hs, -0.3), (-0.75, 0.3, -0.75 + hs, 1.0), (-0.75, -0.15, -0.75 + hs, 0.15),
             (-hs / 2 - 0.2, -1, hs / 2 - 0.2, -1 + 0.05), (-hs / 2 - 0.2, -1 + 0.2, hs / 2 - 0.2, 1 - 0.2),
             (-hs / 2 - 0.2, 1 - 0.05, hs / 2 - 0.2, 1),
             (-hs / 2 + 0.2, -1.0, hs / 2 + 0.2, -0.3), (-hs / 2 + 0.2, 0.3, hs / 2 + 0.2, 1.0),
             (-hs / 2 + 0.2, -0.15, hs / 2 + 0.2, 0.15),
             (0.75 - hs, -1, 0.75, -0.6), (0.75 - hs, -0.5, 0.75, -0.2), (0.75 - hs, -0.1, 0.75, 0.1),
             (0.75 - hs, 0.2, 0.75, 0.5), (0.75 - hs, 0.6, 0.75, 1)]
    centers, sizes = [], []
    for bl_x, bl_y, tr_x, tr_y in rects:
        centers.append((bl_x + abs(tr_x - bl_x) / 2, bl_y + abs(tr_y - bl_y) / 2, 0))
        sizes.append((abs(tr_x - bl_x), abs(tr_y - bl_y), 1.95))
    return [ObjectField([MultiBoxField(np.array(centers), np.array(sizes), tensor_args=tensor_args)], "boxes")]


class EnvMazeBoxes3D(EnvBase):                               # env_maze_boxes_3d.py:55-66
    def __init__(self, tensor_args=None, **kwargs):
        super().__init__(name=self.__class__.__name__, limits=np.array([[-1, -1, -1], [1, 1, 1]], np.float32),
                         obj_fixed_list=create_3d_rectangles_objects(tensor_args), tensor_args=tensor_args, **kwargs)


# ------------------------------------------------------------------------------------------------------------------------------
# 2-D scenes (env_simple_2d.py, env_dense_2d.py, env_narrow_passage_dense_2d.py, env_square_2d.py, env_circle_2d.py,
# env_grid_circles_2d.py and the three *_extra_objects.py).  Their obstacle tables are data of the reference: they are read from the
# recorded fixture tests/golden/scenes_2d.npz (tools/gen_golden_2d.py), not restated here.
# ------------------------------------------------------------------------------------------------------------------------------
SCENES_2D_PATH = Path(__file__).resolve().parent.parent / "tests" / "golden" / "scenes_2d.npz"
_FIELD_KIND_2D = {0: MultiSphereField, 1: MultiBoxField, 2: MultiSharpBoxField}
_scenes_2d = None


def load_scene_2d(name: str, tensor_args=None) -> dict:
    """The recorded tables of one 2-D scene -> dict(limits (2, 2), grid_on, cell, fixed=[ObjectField], extra=[ObjectField])."""
    global _scenes_2d
    if _scenes_2d is None:
        if not SCENES_2D_PATH.exists():
            raise FileNotFoundError(f"{SCENES_2D_PATH} is missing: the 2-D scenes read their obstacle tables from it (a repository "
                                    f"checkout carries it; tools/gen_golden_2d.py records it from the reference)")
        with np.load(SCENES_2D_PATH) as z:
            _scenes_2d = {k: z[k] for k in z.files}
    z = _scenes_2d
    if f"{name}/limits" not in z:
        raise KeyError(f"scenes_2d.npz has no scene {name!r}")
    fields, prims = z[f"{name}/fields"], z[f"{name}/prims"]
    n_obj = len(z[f"{name}/obj_pos"])
    per_obj = [[] for _ in range(n_obj)]
    row = 0
    for o, _, kind, n in fields:                   # rows (object, field, kind, n primitives), primitives in the same order
        p = prims[row:row + n]
        row += n
        cls = _FIELD_KIND_2D[int(kind)]
        per_obj[int(o)].append(cls(p[:, :2], p[:, 2] if kind == 0 else p[:, 2:4], tensor_args=tensor_args))
    out = dict(limits=z[f"{name}/limits"], grid_on=bool(z[f"{name}/grid_on"]), cell=float(z[f"{name}/cell"]), fixed=[], extra=[])
    for k in range(n_obj):
        obj = ObjectField(per_obj[k], str(z[f"{name}/obj_name"][k]), pos=z[f"{name}/obj_pos"][k], ori=z[f"{name}/obj_ori"][k])
        out["extra" if z[f"{name}/obj_extra"][k] else "fixed"].append(obj)
    return out


class _Env2D(EnvBase):
    """A recorded 2-D scene: `_SCENE` names its tables; the subclasses keep the reference's constructor arguments and defaults."""
    _SCENE = None

    def _init_2d(self, name, tensor_args, **kwargs):
        t = load_scene_2d(self._SCENE, tensor_args)
        EnvBase.__init__(self, name=name, limits=t["limits"], obj_fixed_list=t["fixed"], tensor_args=tensor_args, **kwargs)


class EnvSimple2D(_Env2D):                                   # env_simple_2d.py: 15 spheres, grid 400 x 400
    _SCENE = "EnvSimple2D"

    def __init__(self, name="EnvDense2D", tensor_args=None, precompute_sdf_obj_fixed=True, sdf_cell_size=0.005, **kwargs):
        self._init_2d(name, tensor_args, precompute_sdf_obj_fixed=precompute_sdf_obj_fixed, sdf_cell_size=sdf_cell_size, **kwargs)


class EnvDense2D(_Env2D):                                    # env_dense_2d.py: 16 spheres + 14 rounded boxes, grid 400 x 400
    _SCENE = "EnvDense2D"

    def __init__(self, name="EnvDense2D", tensor_args=None, precompute_sdf_obj_fixed=True, sdf_cell_size=0.005, **kwargs):
        self._init_2d(name, tensor_args, precompute_sdf_obj_fixed=precompute_sdf_obj_fixed, sdf_cell_size=sdf_cell_size, **kwargs)


class EnvNarrowPassageDense2D(_Env2D):                       # env_narrow_passage_dense_2d.py: 8 spheres + 11 boxes, analytic
    _SCENE = "EnvNarrowPassageDense2D"

    def __init__(self, name="EnvDense2D", tensor_args=None, **kwargs):
        self._init_2d(name, tensor_args, **kwargs)


class EnvSquare2D(_Env2D):                                   # env_square_2d.py: 1 rounded box, analytic
    _SCENE = "EnvSquare2D"

    def __init__(self, tensor_args=None, **kwargs):
        self._init_2d(self.__class__.__name__, tensor_args, **kwargs)


class EnvCircle2D(_Env2D):                                   # env_circle_2d.py: 1 sphere, grid 400 x 400
    _SCENE = "EnvCircle2D"

    def __init__(self, name="EnvDense2D", tensor_args=None, precompute_sdf_obj_fixed=True, sdf_cell_size=0.005, **kwargs):
        self._init_2d(name, tensor_args, precompute_sdf_obj_fixed=precompute_sdf_obj_fixed, sdf_cell_size=sdf_cell_size, **kwargs)


class EnvGridCircles2D(_Env2D):                              # env_grid_circles_2d.py: 7 x 7 spheres, analytic
    _SCENE = "EnvGridCircles2D"

    def __init__(self, tensor_args=None, **kwargs):
        self._init_2d(self.__class__.__name__, tensor_args, **kwargs)


def _extra_objects(scene, tensor_args):
    return load_scene_2d(scene, tensor_args)["extra"]


class EnvSimple2DExtraObjects(EnvSimple2D):                 # env_simple_2d_extra_objects.py: + 9 spheres, 3 boxes
    def __init__(self, tensor_args=None, **kwargs):
        super().__init__(name=self.__class__.__name__, obj_extra_list=_extra_objects("EnvSimple2DExtraObjects", tensor_args),
                         tensor_args=tensor_args, **kwargs)


class EnvDense2DExtraObjects(EnvDense2D):                   # env_dense_2d_extra_objects.py: + 3 spheres, 4 boxes
    def __init__(self, tensor_args=None, **kwargs):
        super().__init__(name=self.__class__.__name__, obj_extra_list=_extra_objects("EnvDense2DExtraObjects", tensor_args),
                         tensor_args=tensor_args, **kwargs)


class EnvNarrowPassageDense2DExtraObjects(EnvNarrowPassageDense2D):   # env_narrow_passage_dense_2d_extra_objects.py: + 8 spheres, 6 boxes
    def __init__(self, tensor_args=None, **kwargs):
        super().__init__(name=self.__class__.__name__,
                         obj_extra_list=_extra_objects("EnvNarrowPassageDense2DExtraObjects", tensor_args),
                         tensor_args=tensor_args, **kwargs)


SCENES_2D = (EnvSimple2D, EnvDense2D, EnvNarrowPassageDense2D, EnvSquare2D, EnvCircle2D, EnvGridCircles2D,
             EnvSimple2DExtraObjects, EnvDense2DExtraObjects, EnvNarrowPassageDense2DExtraObjects)
