"""cg-raytracer_amd: MI355X-native BVH traversal + ray/triangle intersection (the hot path of
mgokbulut/CG-RayTracer) behind a C-ABI (include/cgrt.h).

This module is the thin Python host used by tests/ and bench.py: a ctypes binding of ``libcgrt.so``
(built in-tree by ``build_native()`` / ``__graft_entry__.build()``).  There is no CPU fallback: if the
library is missing, or no HIP device is usable, calls raise.

The directory name contains a hyphen, so it is loaded under the module name ``cg_raytracer_amd``
(see ``__graft_entry__.load_package``).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import warnings
from typing import Optional, Tuple

import numpy as np

from . import scenes, tiling  # noqa: F401  (re-export)
from .scenes import SceneData

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", os.environ.get("CGRT_LIB_NAME", "libcgrt.so"))  # CGRT_LIB_NAME: experiment builds
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

NO_PRIM = 0xFFFFFFFF

RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("direction", np.float32, 3), ("t", np.float32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("prim_id", np.uint32), ("material_id", np.int32), ("hit", np.uint32)])
assert RAY_DTYPE.itemsize == 28 and HIT_DTYPE.itemsize == 16
# include/cgrt.h CgrtClosest: one closest-point answer (32 bytes); bary = {u, v, w}, the weights of the triangle's three vertices
CLOSEST_DTYPE = np.dtype([("point", np.float32, 3), ("dist2", np.float32), ("prim_id", np.uint32), ("bary", np.float32, 3)])
assert CLOSEST_DTYPE.itemsize == 32
# include/cgrt.h CgrtCrossing: one surface crossing of a ray (8 bytes); an unused entry of a slot is {+inf, NO_PRIM}
CROSSING_DTYPE = np.dtype([("t", np.float32), ("prim_id", np.uint32)])
assert CROSSING_DTYPE.itemsize == 8
# include/cgrt.h CgrtNeighbor: one triangle within a query point's radius (8 bytes); an unused entry of a slot is {+inf, NO_PRIM}
NEIGHBOR_DTYPE = np.dtype([("dist2", np.float32), ("prim_id", np.uint32)])
assert NEIGHBOR_DTYPE.itemsize == 8
# include/cgrt.h CgrtSurfaceSample: one surface sample (32 bytes); point, prim_id and bary at CLOSEST_DTYPE's offsets
SURFACE_SAMPLE_DTYPE = np.dtype([("point", np.float32, 3), ("mesh_id", np.uint32), ("prim_id", np.uint32), ("bary", np.float32, 3)])
assert SURFACE_SAMPLE_DTYPE.itemsize == 32
# include/cgrt.h CgrtPointNeighbor: one data point within a query point's radius (8 bytes); an unused entry of a slot is {+inf, NO_PRIM}
POINT_NEIGHBOR_DTYPE = np.dtype([("dist2", np.float32), ("index", np.uint32)])
assert POINT_NEIGHBOR_DTYPE.itemsize == 8
# include/cgrt.h CgrtPointFrame
POINT_FRAME_DTYPE = np.dtype([("centroid", np.float32, 3), ("used", np.uint32), ("normal", np.float32, 3), ("lambda0", np.float32),
                              ("tangent_u", np.float32, 3), ("lambda1", np.float32), ("tangent_v", np.float32, 3), ("lambda2", np.float32)])
assert POINT_FRAME_DTYPE.itemsize == 64
POINTS_SKIP_SAME_INDEX = 1  # include/cgrt.h CGRT_POINTS_SKIP_SAME_INDEX
ISO_INSIDE_ABOVE = 1  # include/cgrt.h CGRT_ISO_INSIDE_ABOVE
FIELD_CLAMP = 1  # include/cgrt.h CGRT_FIELD_CLAMP
MARCH_MISS, MARCH_HIT, MARCH_EXHAUSTED, MARCH_NONFINITE = 0, 1, 2, 3  # include/cgrt.h CGRT_MARCH_*
# CgrtGridHit as a numpy record
GRID_HIT_DTYPE = np.dtype([("t", np.float32), ("value", np.float32), ("steps", np.uint32), ("status", np.uint32), ("gradient", np.float32, 3),
                           ("reserved", np.uint32)])
_SLOT_RECORDS = {"crossings": CROSSING_DTYPE, "neighbors": NEIGHBOR_DTYPE}  # the slot-list entries (Scene._slots_*) by the name in their symbols
# Scene.inside_tensor's default directions: three fixed generic ones (no component zero, none along an axis, a face diagonal or a space
# diagonal, pairwise far from parallel), so that a ray through an edge or a vertex of an axis-aligned or diagonal-symmetric mesh is the
# exception in at most one of them
INSIDE_DIRECTIONS = ((0.5310871, 0.2178203, 0.8188417), (-0.3319057, 0.9047763, -0.2670293), (0.6834621, -0.5712349, -0.4544671))


class SdfParams(C.Structure):
    """include/cgrt.h CgrtSdfParams."""
    _fields_ = [("max_dist2", C.c_float), ("ndirs", C.c_uint32), ("dirs", (C.c_float * 3) * 7)]


class Grid(C.Structure):
    """include/cgrt.h CgrtGrid: point (ix, iy, iz) = origin + (float)i * spacing per component; dims = (nx, ny, nz)."""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("dims", C.c_uint32 * 3)]


class WindingParams(C.Structure):
    """include/cgrt.h CgrtWindingParams."""
    _fields_ = [("beta", C.c_float), ("threshold", C.c_float)]


def _winding_params(beta: float = 2.0, threshold: float = 0.5) -> WindingParams:
    """CgrtWindingParams; the library checks beta (>= 1, +inf allowed, 0 = its default)."""
    p = WindingParams()
    p.beta, p.threshold = float(beta), float(threshold)
    return p


class SampleParams(C.Structure):
    """include/cgrt.h CgrtSampleParams."""
    _fields_ = [("seed", C.c_uint64), ("first", C.c_uint64), ("strata", C.c_uint64)]


def _sample_params(seed: int = 0, first: int = 0, strata: int = 0) -> SampleParams:
    """CgrtSampleParams; 64-bit unsigned values (ValueError otherwise), the library checks first and strata against n."""
    for name, v in (("seed", seed), ("first", first), ("strata", strata)):
        if not 0 <= int(v) < 1 << 64:
            raise ValueError(f"{name} must be in 0 .. 2^64 - 1")
    p = SampleParams()
    p.seed, p.first, p.strata = int(seed), int(first), int(strata)
    return p


class PoissonParams(C.Structure):
    """include/cgrt.h CgrtPoissonParams."""
    _fields_ = [("min_dist2", C.c_float), ("seed", C.c_uint64), ("priority", C.c_void_p)]


def _poisson_params(min_dist2: float, seed: int = 0, priority_ptr: int = 0) -> PoissonParams:
    """CgrtPoissonParams; seed a 64-bit unsigned value (ValueError otherwise), priority a raw address or 0; the library checks min_dist2."""
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed must be in 0 .. 2^64 - 1")
    p = PoissonParams()
    p.min_dist2, p.seed, p.priority = float(min_dist2), int(seed), (int(priority_ptr) or None)
    return p


class PointNeighbor(C.Structure):
    """include/cgrt.h CgrtPointNeighbor."""
    _fields_ = [("dist2", C.c_float), ("index", C.c_uint32)]


class PointQuery(C.Structure):
    """include/cgrt.h CgrtPointQuery."""
    _fields_ = [("radius2", C.c_void_p), ("max_dist2", C.c_float), ("flags", C.c_uint32)]


class PointFrame(C.Structure):
    """include/cgrt.h CgrtPointFrame."""
    _fields_ = [("centroid", C.c_float * 3), ("used", C.c_uint32), ("normal", C.c_float * 3), ("lambda0", C.c_float),
                ("tangent_u", C.c_float * 3), ("lambda1", C.c_float), ("tangent_v", C.c_float * 3), ("lambda2", C.c_float)]


def _point_query(radius2_ptr: int = 0, max_dist2: float = float("inf"), skip_same_index: bool = False) -> PointQuery:
    """CgrtPointQuery; radius2 a raw address or 0; the library checks max_dist2."""
    q = PointQuery()
    q.radius2, q.max_dist2, q.flags = (int(radius2_ptr) or None), float(max_dist2), (POINTS_SKIP_SAME_INDEX if skip_same_index else 0)
    return q


class IsoParams(C.Structure):
    """include/cgrt.h CgrtIsoParams."""
    _fields_ = [("iso", C.c_float), ("flags", C.c_uint32)]


def _iso_params(iso: float = 0.0, inside_above: bool = False) -> IsoParams:
    """CgrtIsoParams; the library checks iso (finite)."""
    p = IsoParams()
    p.iso, p.flags = float(iso), (ISO_INSIDE_ABOVE if inside_above else 0)
    return p


class FieldParams(C.Structure):
    """include/cgrt.h CgrtFieldParams."""
    _fields_ = [("outside", C.c_float), ("flags", C.c_uint32)]


class MarchParams(C.Structure):
    """include/cgrt.h CgrtMarchParams."""
    _fields_ = [("iso", C.c_float), ("relax", C.c_float), ("min_step", C.c_float), ("hit_eps", C.c_float), ("max_steps", C.c_uint32),
                ("refine", C.c_uint32), ("flags", C.c_uint32)]


class GridHit(C.Structure):
    """include/cgrt.h CgrtGridHit."""
    _fields_ = [("t", C.c_float), ("value", C.c_float), ("steps", C.c_uint32), ("status", C.c_uint32), ("gradient", C.c_float * 3),
                ("reserved", C.c_uint32)]


def _field_params(outside=float("nan"), clamp: bool = False) -> FieldParams:
    """CgrtFieldParams; outside a float or a numpy float32 whose bits are kept as they are."""
    p = FieldParams()
    C.memmove(C.byref(p), np.asarray(outside, np.float32).tobytes(), 4)
    p.flags = FIELD_CLAMP if clamp else 0
    return p


def _march_params(iso: float = 0.0, relax: float = 1.0, min_step: float = 1e-4, hit_eps: float = 1e-4, max_steps: int = 256, refine: int = 0,
                  inside_above: bool = False) -> MarchParams:
    """CgrtMarchParams; max_steps and refine 32-bit unsigned values (ValueError otherwise), the library checks the rest."""
    for name, v in (("max_steps", max_steps), ("refine", refine)):
        if not 0 <= int(v) < 1 << 32:
            raise ValueError(f"{name} must be in 0 .. 2^32 - 1")
    p = MarchParams()
    p.iso, p.relax, p.min_step, p.hit_eps = float(iso), float(relax), float(min_step), float(hit_eps)
    p.max_steps, p.refine, p.flags = int(max_steps), int(refine), (ISO_INSIDE_ABOVE if inside_above else 0)
    return p


def _sdf_params(max_dist2: float = float("inf"), directions=None) -> SdfParams:
    """CgrtSdfParams from max_dist2 and the parity directions (None: the library's defaults, INSIDE_DIRECTIONS).  ValueError for what
    the structure cannot hold (no directions, more than 7, not (k, 3)); the library checks the values."""
    p = SdfParams()
    p.max_dist2 = float(max_dist2)
    if directions is not None:
        d = np.asarray(directions, np.float32)
        if d.ndim != 2 or d.shape[1] != 3 or not 1 <= len(d) <= 7:
            raise ValueError("directions must be (k, 3) with k in 1..7")
        if len(d) % 2 == 0:
            raise ValueError("an odd number of directions is needed for a majority")
        p.ndirs = len(d)
        for j, row in enumerate(d):
            p.dirs[j][:] = [float(x) for x in row]
    return p


def _sdf_grid_struct(origin, spacing, dims) -> Grid:
    """CgrtGrid from origin (3,), spacing (3,) and dims = (nx, ny, nz)."""
    o, sp = np.asarray(origin, np.float32).reshape(3), np.asarray(spacing, np.float32).reshape(3)
    d = [int(x) for x in dims]
    if len(d) != 3 or min(d) < 0 or max(d) > 0xFFFFFFFF:
        raise ValueError("dims must be (nx, ny, nz)")
    g = Grid()
    g.origin[:], g.spacing[:], g.dims[:] = [float(x) for x in o], [float(x) for x in sp], d
    return g


def sdf_grid_points(origin, spacing, dims) -> np.ndarray:
    """The float32 points of a CgrtGrid in result order, (nx * ny * nz, 3): point (ix, iy, iz) = origin + float32(i) * spacing per
    component (the product rounded, then the sum) at row (iz * ny + iy) * nx + ix."""
    o, sp = np.asarray(origin, np.float32).reshape(3), np.asarray(spacing, np.float32).reshape(3)
    nx, ny, nz = (int(x) for x in dims)
    ax = [o[c] + np.arange(m, dtype=np.float32) * sp[c] for c, m in enumerate((nx, ny, nz))]  # (float32 throughout: each operation rounds)
    p = np.empty((nz, ny, nx, 3), np.float32)
    p[..., 0], p[..., 1], p[..., 2] = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
    return p.reshape(-1, 3)


class CgrtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"cgrt error {code}: {msg}")
        self.code = code


class Counters(C.Structure):
    _fields_ = [
        ("rays", C.c_uint64),
        ("inner_visits", C.c_uint64),
        ("leaf_visits", C.c_uint64),
        ("tri_tests", C.c_uint64),
        ("sub_visits", C.c_uint64),
        ("cert_boxes", C.c_uint64),
        ("fallback_rays", C.c_uint64),
        ("tree_rays", C.c_uint64),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RenderStats(C.Structure):
    _fields_ = [("primary_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("reflection_rays", C.c_uint64), ("levels", C.c_int32),
                ("device_ms", C.c_float), ("soft_shadow_rays", C.c_uint64)]


class MultiStats(C.Structure):
    _fields_ = [("replicas", C.c_int32), ("kernel_ms_max", C.c_float), ("download_ms_max", C.c_float), ("wall_ms", C.c_double),
                ("rays", C.c_uint64 * 64)]


class SoftShadows(C.Structure):
    _fields_ = [("spherical", C.c_void_p), ("unit_vectors", C.c_void_p), ("nspherical", C.c_uint32), ("samples", C.c_uint32),
                ("nunits", C.c_uint32), ("seed", C.c_uint32), ("closest_hit", C.c_int32)]


class LightSets(C.Structure):  # CgrtLightSets: CSR arrays, one offset array per light kind
    _fields_ = [("nsets", C.c_uint32), ("lights", C.c_void_p), ("light_offsets", C.c_void_p), ("spherical", C.c_void_p),
                ("spherical_offsets", C.c_void_p)]


AOV_NAMES = ("depth", "normal", "position", "albedo", "prim_id", "material_id", "mask")


class AovOut(C.Structure):  # CgrtAovOut: device pointers of the wanted geometry-buffer planes (NULL: not wanted)
    _fields_ = [(k, C.c_void_p) for k in AOV_NAMES] + [("chw", C.c_int)]

    @staticmethod
    def from_pointers(ptrs, chw: bool = False) -> "AovOut":
        """From a dict plane name -> device address (0 / None / absent: not wanted).  ValueError for an unknown name."""
        a = AovOut()
        for k, p in ptrs.items():
            if k not in AOV_NAMES:
                raise ValueError(f"unknown geometry buffer {k!r}; the planes are {AOV_NAMES}")
            if p:
                setattr(a, k, p)
        a.chw = 1 if chw else 0
        return a


class Camera(C.Structure):
    _fields_ = [
        ("look_at", C.c_float * 3),
        ("euler", C.c_float * 3),
        ("distance", C.c_float),
        ("fovy", C.c_float),
        ("aspect", C.c_float),
    ]

    @staticmethod
    def from_array(a) -> "Camera":
        a = np.asarray(a, np.float32)
        cam = Camera()
        cam.look_at[:] = a[0:3]
        cam.euler[:] = a[3:6]
        cam.distance, cam.fovy, cam.aspect = float(a[6]), float(a[7]), float(a[8])
        return cam


class RayCamera(C.Structure):
    """CgrtRayCamera (include/cgrt.h): the ray of pixel (x, y) has origin and unnormalised direction affine in
    (x + x_off, y + y_off).  The constructors compute in float64 and round each field to float32 once; a non-finite field is a
    ValueError."""

    _fields_ = [
        ("origin", C.c_float * 3), ("origin_dx", C.c_float * 3), ("origin_dy", C.c_float * 3),
        ("dir", C.c_float * 3), ("dir_dx", C.c_float * 3), ("dir_dy", C.c_float * 3),
        ("x_off", C.c_int32), ("y_off", C.c_int32),
    ]  # fmt: skip
    FLOAT_FIELDS = ("origin", "origin_dx", "origin_dy", "dir", "dir_dx", "dir_dy")

    @staticmethod
    def from_fields(origin, origin_dx, origin_dy, dir, dir_dx, dir_dy, x_off: int = 0, y_off: int = 0) -> "RayCamera":  # noqa: A002
        c = RayCamera()
        for k, v in zip(RayCamera.FLOAT_FIELDS, (origin, origin_dx, origin_dy, dir, dir_dx, dir_dy)):
            v = np.asarray(v, np.float64).reshape(3)
            with np.errstate(over="ignore"):
                f = v.astype(np.float32)
            if not np.isfinite(f).all():
                raise ValueError(f"RayCamera.{k} is not finite: {v}")
            getattr(c, k)[:] = f
        c.x_off, c.y_off = int(x_off), int(y_off)
        return c

    @staticmethod
    def from_pinhole(K, cam_to_world, convention: str = "opencv") -> "RayCamera":
        """A pinhole with the 3x3 intrinsic matrix K (any upper-triangular K: skew and non-square pixels included) and the camera-to-world
        pose (3x4 or 4x4).  Pixel (x, y) looks through image point (x + 0.5, y + 0.5): direction = R @ F @ K^-1 @ (x + 0.5, y + 0.5, 1)
        with F = identity for "opencv" (camera x right, y down, z forward: COLMAP) and diag(1, -1, -1) for "opengl" (x right, y up, z
        backward: NeRF-style transforms.json).  Image row 0 is the top row in both."""
        if convention not in ("opencv", "opengl"):
            raise ValueError(f"convention must be 'opencv' or 'opengl', not {convention!r}")
        K = np.asarray(K, np.float64)
        P = np.asarray(cam_to_world, np.float64)
        if K.shape != (3, 3) or P.shape not in ((3, 4), (4, 4)):
            raise ValueError("K must be 3x3 and cam_to_world 3x4 or 4x4")
        M = P[:3, :3] @ (np.diag([1.0, -1.0, -1.0]) if convention == "opengl" else np.eye(3)) @ np.linalg.inv(K)
        zero = np.zeros(3)
        return RayCamera.from_fields(P[:3, 3], zero, zero, M @ np.array([0.5, 0.5, 1.0]), M[:, 0], M[:, 1])

    @staticmethod
    def orthographic(origin, right, up, forward, pixel_size) -> "RayCamera":
        """Parallel rays along `forward`; pixel (x, y) starts at origin + (x + 0.5) * sx * right + (y + 0.5) * sy * up, where `origin` is
        the outer corner of pixel (0, 0) on the image plane, `up` the direction in which y grows, and pixel_size = s or (sx, sy)."""
        sx, sy = np.broadcast_to(np.asarray(pixel_size, np.float64), (2,)) if np.ndim(pixel_size) else (float(pixel_size),) * 2
        o, r, u = (np.asarray(v, np.float64).reshape(3) for v in (origin, right, up))
        zero = np.zeros(3)
        return RayCamera.from_fields(o + 0.5 * sx * r + 0.5 * sy * u, sx * r, sy * u, forward, zero, zero)

    @staticmethod
    def from_trackball(cam, W: int, H: int) -> "RayCamera":
        """The ray camera closest to the Trackball camera `cam` (a Camera or its 9 floats) for W x H frames: Trackball::generateRay's
        position, rotation and image plane evaluated in float64 from the camera's float32 fields.  Close to cgrt_generate_rays, not
        bit-identical: the formula differs."""
        a = (camera_array([cam])[0] if isinstance(cam, Camera) else np.asarray(cam, np.float32).reshape(9)).astype(np.float64)
        h = a[3:6] * 0.5
        (cx, cy, cz), (sx, sy, sz) = np.cos(h), np.sin(h)
        w, q = cx * cy * cz + sx * sy * sz, np.array([sx * cy * cz - cx * sy * sz, cx * sy * cz + sx * cy * sz, cx * cy * sz - sx * sy * cz])

        def rot(v):  # glm: v + 2 * (w * (q x v) + q x (q x v))
            uv = np.cross(q, v)
            return v + 2.0 * (w * uv + np.cross(q, uv))

        half_h = np.tan(a[7] / 2.0)
        half_w = a[8] * half_h
        zero = np.zeros(3)
        # ndc = p / size * 2 - 1; camera-space direction (-ndc.x * half_w, ndc.y * half_h, 1)
        return RayCamera.from_fields(a[0:3] + rot(np.array([0.0, 0.0, -a[6]])), zero, zero, rot(np.array([half_w, -half_h, 1.0])),
                                     rot(np.array([-2.0 * half_w / W, 0.0, 0.0])), rot(np.array([0.0, 2.0 * half_h / H, 0.0])))

    def tile(self, x_off: int, y_off: int) -> "RayCamera":
        """The same camera for a tile whose pixel (0, 0) is pixel (x_off, y_off) of this camera's frame (offsets add up)."""
        c = RayCamera.from_buffer_copy(self)
        c.x_off, c.y_off = self.x_off + int(x_off), self.y_off + int(y_off)
        return c

    def as_array(self) -> np.ndarray:
        """The 80 bytes as a (20,) float32 array (the offsets' bits in the last two elements)."""
        return np.frombuffer(bytes(self), np.float32).copy()


def raycam_array(cams) -> np.ndarray:
    """A batch of ray cameras as a contiguous (B, 20) float32 array of CgrtRayCamera records (the two int32 offsets by bit pattern):
    from a RayCamera, a sequence of RayCamera, or such an array (ValueError otherwise)."""
    if isinstance(cams, RayCamera):
        cams = [cams]
    if isinstance(cams, np.ndarray):
        a = np.ascontiguousarray(cams)
        if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != 20:
            raise ValueError(f"ray cameras as an array must be (B, 20) float32 records, not {a.dtype} {a.shape}")
        return a
    cams = list(cams)
    if not all(isinstance(c, RayCamera) for c in cams):
        raise ValueError("cams must be a RayCamera, a sequence of RayCamera or a (B, 20) float32 array of records")
    return np.ascontiguousarray(np.stack([c.as_array() for c in cams]) if cams else np.zeros((0, 20), np.float32))


HOST_LIB_PATH = os.path.join(_HERE, "lib", "libcgrt_host.so")

_surface_fn = None


def _surface_function():
    """The torch.autograd.Function behind interpolate_hits_tensor / surface_views_tensor / surface_raycams_tensor when attr requires grad
    (DESIGN.md sections 5.23 and 5.28): apply(attr, forward, backward, which=None, reproducible=False).  forward(attr.detach()) is the ordinary, non-recording call (a
    tensor, or a tuple of which entry `which` is the attribute and the others, the barycentrics, are marked non-differentiable);
    backward(grad) is the matching *_grad_tensor call on torch.cuda.current_stream().  Only attr gets a gradient: rays, hits, planes and
    cameras are held as given and are not differentiable.  With `reproducible` the backward call is the bitwise-reproducible entry, and
    deterministic mode has nothing to object to."""
    global _surface_fn
    if _surface_fn is not None:
        return _surface_fn
    import torch
    from torch.autograd.function import once_differentiable

    class SurfaceAttribute(torch.autograd.Function):
        @staticmethod
        def forward(ctx, attr, forward, backward, which=None, reproducible=False):
            ctx.backward_call, ctx.which, ctx.reproducible = backward, which, reproducible
            res = forward(attr.detach())
            if which is not None:
                ctx.mark_non_differentiable(*(t for k, t in enumerate(res) if k != which))
            return res

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            if not ctx.reproducible and torch.are_deterministic_algorithms_enabled():
                msg = ("the surface-attribute backward adds into the table with float atomics: the order of the additions into one element "
                       "is unspecified and the last bits of the gradient may differ from run to run")
                if torch.is_deterministic_algorithms_warn_only_enabled():
                    warnings.warn(msg, UserWarning, stacklevel=2)
                else:
                    raise RuntimeError(msg + " (torch.use_deterministic_algorithms(True) is set)")
            g = grads[0 if ctx.which is None else ctx.which]
            return ctx.backward_call(g.contiguous()), None, None, None, None

    _surface_fn = SurfaceAttribute
    return _surface_fn


_grid_fn = None


def _grid_function():
    """The torch.autograd.Function behind sample_grid_tensor when values or points requires grad:
    apply(values, points, forward, backward, want, reproducible=False) -> the tensors named by `want`, in its order.  With `reproducible`
    the backward call is the bitwise-reproducible entry and deterministic mode has nothing to object to.
    forward(values, points) is the
    ordinary, non-recording call on detached tensors and returns a dict that always holds 'gradient'; backward(points, grad_value,
    grad_gradient) is the sample_grid_grad_tensor call on torch.cuda.current_stream().  'value' and 'gradient' are differentiable with
    respect to values; 'value' with respect to points, as grad_value[:, None] * gradient; the 'gradient' output is held constant in the
    points; 'inside' is not differentiable."""
    global _grid_fn
    if _grid_fn is not None:
        return _grid_fn
    import torch
    from torch.autograd.function import once_differentiable

    class GridSample(torch.autograd.Function):
        @staticmethod
        def forward(ctx, values, points, forward, backward, want, reproducible=False):
            ctx.backward_call, ctx.want, ctx.reproducible = backward, want, reproducible
            ctx.set_materialize_grads(False)
            res = forward(values.detach(), points.detach())
            ctx.save_for_backward(points, res["gradient"])
            if "inside" in want:
                ctx.mark_non_differentiable(res["inside"])
            return tuple(res[w] for w in want)

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            by_name = dict(zip(ctx.want, grads))
            gv, gg = by_name.get("value"), by_name.get("gradient")
            points, gradient = ctx.saved_tensors
            grad_values = grad_points = None
            if ctx.needs_input_grad[0] and (gv is not None or gg is not None):
                if not ctx.reproducible and torch.are_deterministic_algorithms_enabled():
                    msg = ("the grid-sample backward adds into the volume with float atomics: the order of the additions into one element "
                           "is unspecified and the last bits of the gradient may differ from run to run")
                    if torch.is_deterministic_algorithms_warn_only_enabled():
                        warnings.warn(msg, UserWarning, stacklevel=2)
                    else:
                        raise RuntimeError(msg + " (torch.use_deterministic_algorithms(True) is set)")
                grad_values = ctx.backward_call(points, None if gv is None else gv.contiguous(), None if gg is None else gg.contiguous())
            if ctx.needs_input_grad[1] and gv is not None:
                grad_points = gv[:, None] * gradient
            return grad_values, grad_points, None, None, None, None

    _grid_fn = GridSample
    return _grid_fn


def build_native(verbose: bool = False) -> str:
    """Compile libcgrt.so for gfx950 in-tree (hipcc cross-compiles without a GPU), then the C++ host mirror of the
    reference interface (libcgrt_host.so + the headless `render` tool, g++)."""
    for sub in ("csrc", "host"):
        r = subprocess.run(["make", "-C", os.path.join(_HERE, sub)], capture_output=True, text=True)
        if verbose or r.returncode:
            print(r.stdout[-4000:], r.stderr[-4000:])
        if r.returncode:
            raise RuntimeError(f"building {sub} failed")
    return LIB_PATH


_lib: Optional[C.CDLL] = None

# every symbol include/cgrt.h declares
EXPORTS = [
    "cgrt_scene_create", "cgrt_scene_destroy", "cgrt_set_leaf_accel", "cgrt_num_subnodes", "cgrt_set_primary_mode", "cgrt_set_kernel_shape", "cgrt_get_kernel_shape", "cgrt_set_render_prediction", "cgrt_set_frame_hints", "cgrt_set_frame_gate", "cgrt_debug_frame_gate", "cgrt_set_frame_order", "cgrt_debug_set_frame_order", "cgrt_debug_get_frame_order", "cgrt_debug_build_frame_order", "cgrt_debug_set_hint_thresholds", "cgrt_debug_hint_counts", "cgrt_debug_render_path", "cgrt_set_fast_tree", "cgrt_scene_set_walk", "cgrt_scene_walk", "cgrt_scene_build_info", "cgrt_num_levels", "cgrt_num_nodes", "cgrt_get_nodes", "cgrt_leaf_prims",
    "cgrt_build_seconds", "cgrt_device_bytes", "cgrt_intersect_batch", "cgrt_set_call_combining", "cgrt_debug_combiner_stats", "cgrt_intersect_brute_batch", "cgrt_intersect_batch_device", "cgrt_trace_primary",
    "cgrt_trace_primary_device", "cgrt_generate_rays", "cgrt_render", "cgrt_render_soft", "cgrt_render_mapped", "cgrt_render_rank", "cgrt_render_counted", "cgrt_trace_primary_multi", "cgrt_render_multi", "cgrt_render_aa", "cgrt_render_aa_mapped", "cgrt_render_multi_aa", "cgrt_render_device", "cgrt_debug_export_frame", "cgrt_shade_rays", "cgrt_shade_rays_device", "cgrt_trace_primary_views_device", "cgrt_render_views", "cgrt_render_views_device", "cgrt_render_light_sets", "cgrt_render_light_sets_device", "cgrt_render_views_light_sets", "cgrt_render_views_light_sets_device", "cgrt_enqueue_render_views_light_sets_device", "cgrt_enqueue_render_device", "cgrt_enqueue_render_views_device", "cgrt_render_aov_device", "cgrt_render_views_aov_device", "cgrt_enqueue_render_aov_device", "cgrt_enqueue_render_views_aov_device", "cgrt_generate_rays_raycam", "cgrt_trace_primary_raycams_device", "cgrt_render_raycams_device", "cgrt_enqueue_render_raycams_device", "cgrt_render_raycams_light_sets_device", "cgrt_enqueue_shade_rays_device", "cgrt_enqueue_stats", "cgrt_debug_strided_waves", "cgrt_occluded", "cgrt_occluded_device", "cgrt_in_shadow", "cgrt_in_shadow_device", "cgrt_soft_lit", "cgrt_soft_lit_device", "cgrt_hit_barycentrics", "cgrt_hit_barycentrics_device", "cgrt_interpolate_hits", "cgrt_interpolate_hits_device", "cgrt_surface_views_device", "cgrt_surface_raycams_device", "cgrt_interpolate_hits_grad", "cgrt_interpolate_hits_grad_device", "cgrt_surface_views_grad_device", "cgrt_surface_raycams_grad_device", "cgrt_surface_grad_repro_workspace", "cgrt_interpolate_hits_grad_repro", "cgrt_interpolate_hits_grad_repro_device", "cgrt_surface_views_grad_repro_device", "cgrt_surface_raycams_grad_repro_device", "cgrt_closest_points", "cgrt_closest_points_device", "cgrt_closest_points_brute", "cgrt_debug_closest_work", "cgrt_count_crossings", "cgrt_count_crossings_device", "cgrt_list_crossings", "cgrt_list_crossings_device", "cgrt_list_crossings_brute", "cgrt_debug_crossing_work", "cgrt_count_neighbors", "cgrt_count_neighbors_device", "cgrt_list_neighbors", "cgrt_list_neighbors_device", "cgrt_list_neighbors_brute", "cgrt_debug_neighbor_work", "cgrt_signed_distance", "cgrt_signed_distance_device", "cgrt_signed_distance_grid", "cgrt_signed_distance_grid_device", "cgrt_debug_sdf_work", "cgrt_debug_set_sdf_grid_mapping", "cgrt_winding_numbers", "cgrt_winding_numbers_device", "cgrt_winding_numbers_grid", "cgrt_winding_numbers_grid_device", "cgrt_winding_numbers_brute", "cgrt_debug_winding_work", "cgrt_debug_get_winding_tree", "cgrt_sample_surface", "cgrt_sample_surface_device", "cgrt_triangle_areas", "cgrt_debug_get_sample_table", "cgrt_poisson_disk", "cgrt_poisson_disk_device", "cgrt_poisson_disk_workspace", "cgrt_poisson_disk_brute", "cgrt_debug_poisson_work", "cgrt_point_grid_workspace", "cgrt_point_grid_build_device", "cgrt_count_point_neighbors", "cgrt_count_point_neighbors_device", "cgrt_list_point_neighbors", "cgrt_list_point_neighbors_device", "cgrt_list_point_neighbors_brute", "cgrt_debug_point_neighbor_work", "cgrt_point_frames", "cgrt_point_frames_device", "cgrt_point_frames_brute", "cgrt_isosurface_workspace", "cgrt_isosurface_count_device", "cgrt_isosurface_device", "cgrt_isosurface", "cgrt_debug_isosurface_work", "cgrt_sample_grid", "cgrt_sample_grid_device", "cgrt_march_grid", "cgrt_march_grid_device", "cgrt_debug_march_work", "cgrt_sample_grid_grad", "cgrt_sample_grid_grad_device", "cgrt_sample_grid_grad_repro_workspace", "cgrt_sample_grid_grad_repro", "cgrt_sample_grid_grad_repro_device", "cgrt_count_primary", "cgrt_count_batch", "cgrt_debug_wave_times", "cgrt_debug_trace_shadow", "cgrt_debug_soft_lit", "cgrt_debug_fastdiv_check", "cgrt_debug_gather_calibration", "cgrt_debug_check_layout", "cgrt_debug_layout_hash", "cgrt_debug_node_pack", "cgrt_debug_node_unpack", "cgrt_debug_get_subnodes", "cgrt_set_build_threads", "cgrt_record_sizes",
    "cgrt_ray_triangle_batch", "cgrt_ray_plane_batch", "cgrt_ray_box_batch", "cgrt_ray_sphere_batch",
    "cgrt_triangle_plane_batch", "cgrt_point_in_triangle_batch", "cgrt_device_count", "cgrt_last_error", "cgrt_version", "cgrt_source_hash",
]  # fmt: skip


def lib() -> C.CDLL:
    """Load libcgrt.so; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        try:  # not shipped with this checkout: compile it now (hipcc, gfx950); there is no other path to fall back to
            build_native()
        except Exception as e:  # noqa: BLE001
            raise RuntimeError(f"{LIB_PATH} is missing and could not be built: {e}") from e
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.cgrt_last_error.restype = C.c_char_p
    L.cgrt_version.restype = C.c_char_p
    L.cgrt_source_hash.restype = C.c_char_p
    L.cgrt_scene_create.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, i32, C.POINTER(vp)]
    L.cgrt_scene_destroy.argtypes = [vp]
    L.cgrt_scene_destroy.restype = None
    for f in (L.cgrt_num_levels, L.cgrt_num_nodes):
        f.argtypes = [vp]
    L.cgrt_set_leaf_accel.argtypes = [i32, i32]
    L.cgrt_num_subnodes.argtypes = [vp]
    L.cgrt_debug_check_layout.argtypes = [vp]
    L.cgrt_debug_layout_hash.argtypes = [vp, C.POINTER(u64)]
    L.cgrt_debug_node_pack.argtypes = [vp, vp, u32, vp]
    L.cgrt_debug_node_pack.restype = None
    L.cgrt_debug_node_unpack.argtypes = [vp, vp, vp, C.POINTER(u32)]
    L.cgrt_debug_node_unpack.restype = None
    L.cgrt_debug_get_subnodes.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(u32), vp, C.POINTER(u32)]
    L.cgrt_set_build_threads.argtypes = [i32]
    L.cgrt_set_primary_mode.argtypes = [i32]
    L.cgrt_set_fast_tree.argtypes = [i32]
    L.cgrt_set_kernel_shape.argtypes = [i32, u64]
    L.cgrt_set_render_prediction.argtypes = [i32]
    L.cgrt_set_frame_hints.argtypes = [i32]
    L.cgrt_set_frame_gate.argtypes = [i32]
    L.cgrt_set_frame_order.argtypes = [i32]
    L.cgrt_debug_set_frame_order.argtypes = [vp] + [i32] * 8 + [C.POINTER(C.c_uint16), C.c_uint32]
    L.cgrt_debug_get_frame_order.argtypes = [vp, C.POINTER(C.c_uint16), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(i32)]
    L.cgrt_debug_build_frame_order.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint16)]
    L.cgrt_debug_frame_gate.argtypes = [vp, C.POINTER(Camera), i32, i32, C.POINTER(i32)]
    L.cgrt_debug_set_hint_thresholds.argtypes = [u32, u32]
    L.cgrt_debug_render_path.argtypes = [C.c_void_p]
    L.cgrt_get_kernel_shape.argtypes = [C.POINTER(i32), C.POINTER(u64)]
    L.cgrt_scene_set_walk.argtypes = [vp, i32]
    L.cgrt_scene_walk.argtypes = [vp]
    L.cgrt_scene_build_info.argtypes = [vp, vp]
    L.cgrt_get_nodes.argtypes = [vp, vp, vp]
    L.cgrt_leaf_prims.argtypes = [vp, i32, vp, u32]
    L.cgrt_leaf_prims.restype = C.c_int64
    L.cgrt_build_seconds.argtypes = [vp]
    L.cgrt_build_seconds.restype = C.c_double
    L.cgrt_device_bytes.argtypes = [vp]
    L.cgrt_device_bytes.restype = u64
    L.cgrt_intersect_batch.argtypes = [vp, vp, u64, vp, vp]
    L.cgrt_intersect_brute_batch.argtypes = [vp, vp, u64, i32, vp, vp]
    L.cgrt_set_call_combining.argtypes = [i32]
    L.cgrt_debug_combiner_stats.argtypes = [vp, vp]
    L.cgrt_intersect_batch_device.argtypes = [vp, vp, u64, vp, vp, vp]
    L.cgrt_trace_primary.argtypes = [vp, C.POINTER(Camera)] + [i32] * 8 + [vp, vp]
    L.cgrt_trace_primary_device.argtypes = [vp, C.POINTER(Camera)] + [i32] * 8 + [vp, vp, vp]
    L.cgrt_generate_rays.argtypes = [vp, C.POINTER(Camera)] + [i32] * 6 + [vp]
    L.cgrt_render.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, u32, i32, vp, C.POINTER(RenderStats)]
    L.cgrt_render_counted.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, u32, i32, vp, C.POINTER(RenderStats), C.POINTER(Counters)]
    L.cgrt_render_soft.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, u32, C.POINTER(SoftShadows), i32, vp, C.POINTER(RenderStats)]
    L.cgrt_render_mapped.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, u32, C.POINTER(SoftShadows), i32, C.POINTER(vp), C.POINTER(RenderStats)]
    L.cgrt_render_rank.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, u32, C.POINTER(SoftShadows), i32, i32, i32, vp, C.POINTER(RenderStats)]
    L.cgrt_trace_primary_multi.argtypes = [C.POINTER(vp), i32, C.POINTER(Camera), i32, i32, vp, vp, C.POINTER(MultiStats)]
    L.cgrt_render_multi.argtypes = [C.POINTER(vp), i32, C.POINTER(Camera), i32, i32, vp, u32, C.POINTER(SoftShadows), i32, vp, C.POINTER(RenderStats)]
    L.cgrt_render_aa.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, u32, C.POINTER(SoftShadows), i32, i32, i32, vp, C.POINTER(RenderStats)]
    L.cgrt_render_aa_mapped.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, u32, C.POINTER(SoftShadows), i32, C.POINTER(vp), C.POINTER(RenderStats)]
    L.cgrt_render_multi_aa.argtypes = [C.POINTER(vp), i32, C.POINTER(Camera), i32, i32, vp, u32, C.POINTER(SoftShadows), i32, vp, C.POINTER(RenderStats)]
    L.cgrt_render_device.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, u32, C.POINTER(SoftShadows), i32, i32, i32, i32, vp, i32, u64, vp,
                                     C.POINTER(RenderStats)]
    L.cgrt_debug_export_frame.argtypes = [i32, vp, i32, i32, i32, u64, vp]
    L.cgrt_shade_rays.argtypes = [vp, vp, u64, vp, u32, C.POINTER(SoftShadows), i32, vp, C.POINTER(RenderStats)]
    L.cgrt_shade_rays_device.argtypes = [vp, vp, u64, vp, u32, C.POINTER(SoftShadows), i32, vp, vp, C.POINTER(RenderStats)]
    L.cgrt_trace_primary_views_device.argtypes = [vp, vp, u32, i32, i32, vp, vp, vp]
    L.cgrt_render_views.argtypes = [vp, vp, u32, i32, i32, vp, u32, C.POINTER(SoftShadows), i32, vp, C.POINTER(RenderStats)]
    L.cgrt_render_views_device.argtypes = [vp, vp, u32, i32, i32, vp, u32, C.POINTER(SoftShadows), i32, vp, i32, vp, C.POINTER(RenderStats)]
    L.cgrt_render_light_sets.argtypes = [vp, C.POINTER(Camera), i32, i32, C.POINTER(LightSets), C.POINTER(SoftShadows), i32, vp, C.POINTER(RenderStats)]
    L.cgrt_render_light_sets_device.argtypes = [vp, C.POINTER(Camera), i32, i32, C.POINTER(LightSets), C.POINTER(SoftShadows), i32, vp, i32, vp,
                                                C.POINTER(RenderStats)]
    L.cgrt_render_views_light_sets.argtypes = [vp, vp, u32, i32, i32, C.POINTER(LightSets), C.POINTER(SoftShadows), i32, vp, C.POINTER(RenderStats)]
    L.cgrt_render_views_light_sets_device.argtypes = [vp, vp, u32, i32, i32, C.POINTER(LightSets), C.POINTER(SoftShadows), i32, vp, i32, vp,
                                                      C.POINTER(RenderStats)]
    L.cgrt_enqueue_render_views_light_sets_device.argtypes = [vp, vp, u32, i32, i32, C.POINTER(LightSets), C.POINTER(SoftShadows), i32, vp, i32,
                                                              vp, C.POINTER(u64)]
    L.cgrt_enqueue_render_device.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, u32, C.POINTER(SoftShadows), i32, i32, i32, i32, vp, i32, u64,
                                             vp, C.POINTER(u64)]
    L.cgrt_enqueue_render_views_device.argtypes = [vp, vp, u32, i32, i32, vp, u32, C.POINTER(SoftShadows), i32, vp, i32, vp, C.POINTER(u64)]
    L.cgrt_enqueue_shade_rays_device.argtypes = [vp, vp, u64, vp, u32, C.POINTER(SoftShadows), i32, vp, vp, C.POINTER(u64)]
    L.cgrt_render_aov_device.argtypes = L.cgrt_render_device.argtypes + [C.POINTER(AovOut)]
    L.cgrt_render_views_aov_device.argtypes = L.cgrt_render_views_device.argtypes + [C.POINTER(AovOut)]
    L.cgrt_enqueue_render_aov_device.argtypes = L.cgrt_enqueue_render_device.argtypes + [C.POINTER(AovOut)]
    L.cgrt_enqueue_render_views_aov_device.argtypes = L.cgrt_enqueue_render_views_device.argtypes + [C.POINTER(AovOut)]
    L.cgrt_generate_rays_raycam.argtypes = [vp, vp, i32, i32, vp]
    L.cgrt_trace_primary_raycams_device.argtypes = L.cgrt_trace_primary_views_device.argtypes
    L.cgrt_render_raycams_device.argtypes = L.cgrt_render_views_aov_device.argtypes
    L.cgrt_enqueue_render_raycams_device.argtypes = L.cgrt_enqueue_render_views_aov_device.argtypes
    L.cgrt_render_raycams_light_sets_device.argtypes = L.cgrt_render_views_light_sets_device.argtypes
    L.cgrt_enqueue_stats.argtypes = [vp, u64, C.POINTER(RenderStats)]
    L.cgrt_debug_strided_waves.argtypes = []
    L.cgrt_occluded.argtypes = [vp, vp, u64, vp]
    L.cgrt_occluded_device.argtypes = [vp, vp, u64, vp, vp]
    L.cgrt_in_shadow.argtypes = [vp, vp, u64, vp, u32, vp]
    L.cgrt_in_shadow_device.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    L.cgrt_soft_lit.argtypes = [vp, vp, u64, C.POINTER(SoftShadows), vp]
    L.cgrt_soft_lit_device.argtypes = [vp, vp, u64, C.POINTER(SoftShadows), vp, vp]
    L.cgrt_hit_barycentrics.argtypes = [vp, vp, vp, u64, vp]
    L.cgrt_hit_barycentrics_device.argtypes = [vp, vp, vp, u64, vp, vp]
    L.cgrt_interpolate_hits.argtypes = [vp, vp, vp, u64, vp, u32, vp]
    L.cgrt_interpolate_hits_device.argtypes = [vp, vp, vp, u64, vp, u32, vp, vp]
    L.cgrt_surface_views_device.argtypes = [vp, vp, u32, i32, i32, vp, vp, vp, u32, vp, vp, i32, vp]
    L.cgrt_surface_raycams_device.argtypes = L.cgrt_surface_views_device.argtypes
    L.cgrt_interpolate_hits_grad.argtypes = [vp, vp, vp, u64, vp, u32, vp]
    L.cgrt_interpolate_hits_grad_device.argtypes = [vp, vp, vp, u64, vp, u32, vp, vp]
    L.cgrt_surface_views_grad_device.argtypes = [vp, vp, u32, i32, i32, vp, vp, vp, u32, i32, vp, vp]
    L.cgrt_surface_raycams_grad_device.argtypes = L.cgrt_surface_views_grad_device.argtypes
    L.cgrt_surface_grad_repro_workspace.argtypes = [vp, u32, C.POINTER(C.c_uint64)]
    L.cgrt_interpolate_hits_grad_repro.argtypes = L.cgrt_interpolate_hits_grad.argtypes
    L.cgrt_interpolate_hits_grad_repro_device.argtypes = [vp, vp, vp, u64, vp, u32, vp, vp, u64, vp]
    L.cgrt_surface_views_grad_repro_device.argtypes = [vp, vp, u32, i32, i32, vp, vp, vp, u32, i32, vp, vp, u64, vp]
    L.cgrt_surface_raycams_grad_repro_device.argtypes = L.cgrt_surface_views_grad_repro_device.argtypes
    L.cgrt_closest_points.argtypes = [vp, vp, u64, C.c_float, vp]
    L.cgrt_closest_points_brute.argtypes = [vp, vp, u64, C.c_float, vp]
    L.cgrt_closest_points_device.argtypes = [vp, vp, u64, C.c_float, vp, vp]
    L.cgrt_debug_closest_work.argtypes = [vp, vp, u64, C.c_float, vp]
    L.cgrt_count_crossings.argtypes = [vp, vp, u64, vp]
    L.cgrt_count_crossings_device.argtypes = [vp, vp, u64, vp, vp]
    L.cgrt_list_crossings.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp]
    L.cgrt_list_crossings_brute.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp]
    L.cgrt_list_crossings_device.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp, vp]
    L.cgrt_debug_crossing_work.argtypes = [vp, vp, u64, vp]
    L.cgrt_count_neighbors.argtypes = [vp, vp, u64, vp, C.c_float, vp]
    L.cgrt_count_neighbors_device.argtypes = [vp, vp, u64, vp, C.c_float, vp, vp]
    L.cgrt_list_neighbors.argtypes = [vp, vp, u64, vp, C.c_float, vp, u32, vp, u64, vp]
    L.cgrt_list_neighbors_brute.argtypes = [vp, vp, u64, vp, C.c_float, vp, u32, vp, u64, vp]
    L.cgrt_list_neighbors_device.argtypes = [vp, vp, u64, vp, C.c_float, vp, u32, vp, u64, vp, vp]
    L.cgrt_debug_neighbor_work.argtypes = [vp, vp, u64, vp, C.c_float, u32, vp]
    L.cgrt_signed_distance.argtypes = [vp, vp, u64, C.POINTER(SdfParams), vp, vp]
    L.cgrt_signed_distance_device.argtypes = [vp, vp, u64, C.POINTER(SdfParams), vp, vp, vp]
    L.cgrt_signed_distance_grid.argtypes = [vp, C.POINTER(Grid), C.POINTER(SdfParams), vp, vp]
    L.cgrt_signed_distance_grid_device.argtypes = [vp, C.POINTER(Grid), C.POINTER(SdfParams), vp, vp, vp]
    L.cgrt_debug_sdf_work.argtypes = [vp, vp, u64, C.POINTER(SdfParams), i32, vp]
    L.cgrt_debug_set_sdf_grid_mapping.argtypes = [i32]
    L.cgrt_winding_numbers.argtypes = [vp, vp, u64, C.POINTER(WindingParams), vp, vp]
    L.cgrt_winding_numbers_device.argtypes = [vp, vp, u64, C.POINTER(WindingParams), vp, vp, vp]
    L.cgrt_winding_numbers_grid.argtypes = [vp, C.POINTER(Grid), C.POINTER(WindingParams), vp, vp]
    L.cgrt_winding_numbers_grid_device.argtypes = [vp, C.POINTER(Grid), C.POINTER(WindingParams), vp, vp, vp]
    L.cgrt_winding_numbers_brute.argtypes = [vp, vp, u64, C.POINTER(WindingParams), vp, vp]
    L.cgrt_debug_winding_work.argtypes = [vp, vp, u64, C.POINTER(WindingParams), vp]
    L.cgrt_debug_get_winding_tree.argtypes = [vp, vp, vp, C.POINTER(u32), vp]
    L.cgrt_sample_surface.argtypes = [vp, u64, C.POINTER(SampleParams), vp, vp, u32, vp]
    L.cgrt_sample_surface_device.argtypes = [vp, u64, C.POINTER(SampleParams), vp, vp, u32, vp, vp]
    for f in (L.cgrt_poisson_disk, L.cgrt_poisson_disk_brute):
        f.argtypes = [vp, vp, u64, C.POINTER(PoissonParams), vp, C.POINTER(u64)]
    L.cgrt_poisson_disk_device.argtypes = [vp, vp, u64, C.POINTER(PoissonParams), vp, C.POINTER(u64), vp, u64, vp]
    L.cgrt_poisson_disk_workspace.argtypes = [vp, u64, C.POINTER(u64)]
    L.cgrt_debug_poisson_work.argtypes = [vp, vp, u64, C.POINTER(PoissonParams), vp]
    pq = C.POINTER(PointQuery)
    L.cgrt_point_grid_workspace.argtypes = [vp, u64, C.POINTER(u64)]
    L.cgrt_point_grid_build_device.argtypes = [vp, vp, u64, C.c_float, vp, u64, vp]
    L.cgrt_count_point_neighbors_device.argtypes = [vp, vp, u64, vp, u64, pq, vp, vp]
    L.cgrt_list_point_neighbors_device.argtypes = [vp, vp, u64, vp, u64, pq, vp, u32, vp, u64, vp, vp]
    L.cgrt_count_point_neighbors.argtypes = [vp, vp, u64, C.c_float, vp, u64, pq, vp]
    L.cgrt_list_point_neighbors.argtypes = [vp, vp, u64, C.c_float, vp, u64, pq, vp, u32, vp, u64, vp]
    L.cgrt_list_point_neighbors_brute.argtypes = [vp, vp, u64, vp, u64, pq, vp, u32, vp, u64, vp]
    L.cgrt_debug_point_neighbor_work.argtypes = [vp, vp, u64, C.c_float, vp, u64, pq, u32, vp]
    L.cgrt_point_frames_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, pq, u32, vp, vp, vp, vp]
    L.cgrt_point_frames.argtypes = [vp, vp, u64, C.c_float, vp, u64, pq, u32, vp, vp, vp]
    L.cgrt_point_frames_brute.argtypes = [vp, vp, u64, vp, u64, pq, u32, vp, vp, vp]
    gp, ip = C.POINTER(Grid), C.POINTER(IsoParams)
    L.cgrt_isosurface_workspace.argtypes = [vp, gp, C.POINTER(u64)]
    L.cgrt_isosurface_count_device.argtypes = [vp, gp, vp, ip, vp, vp, u64, vp]
    L.cgrt_isosurface_device.argtypes = [vp, gp, vp, ip, vp, u64, vp, u64, vp, vp, u64, vp]
    L.cgrt_isosurface.argtypes = [vp, gp, vp, ip, vp, u64, vp, u64, vp]
    L.cgrt_debug_isosurface_work.argtypes = [vp, gp, vp, ip, vp]
    fp, mp = C.POINTER(FieldParams), C.POINTER(MarchParams)
    L.cgrt_sample_grid.argtypes = [vp, gp, vp, vp, u64, fp, vp, vp, vp]
    L.cgrt_sample_grid_device.argtypes = [vp, gp, vp, vp, u64, fp, vp, vp, vp, vp]
    L.cgrt_march_grid.argtypes = [vp, gp, vp, vp, u64, mp, vp]
    L.cgrt_march_grid_device.argtypes = [vp, gp, vp, vp, u64, mp, vp, vp]
    L.cgrt_debug_march_work.argtypes = [vp, gp, vp, vp, u64, mp, vp]
    L.cgrt_sample_grid_grad.argtypes = [vp, gp, vp, u64, fp, vp, vp, vp]
    L.cgrt_sample_grid_grad_device.argtypes = [vp, gp, vp, u64, fp, vp, vp, vp, vp]
    L.cgrt_sample_grid_grad_repro_workspace.argtypes = [vp, gp, C.POINTER(C.c_uint64)]
    L.cgrt_sample_grid_grad_repro.argtypes = L.cgrt_sample_grid_grad.argtypes
    L.cgrt_sample_grid_grad_repro_device.argtypes = [vp, gp, vp, u64, fp, vp, vp, vp, vp, u64, vp]
    L.cgrt_triangle_areas.argtypes = [vp, vp, C.POINTER(C.c_double)]
    L.cgrt_debug_get_sample_table.argtypes = [vp, vp, C.POINTER(u32)]
    L.cgrt_count_primary.argtypes = [vp, C.POINTER(Camera)] + [i32] * 8 + [C.POINTER(Counters)]
    L.cgrt_count_batch.argtypes = [vp, vp, u64, C.POINTER(Counters)]
    L.cgrt_debug_gather_calibration.argtypes = [i32, u64, i32]
    L.cgrt_debug_fastdiv_check.argtypes = [i32, vp, vp, u64, vp, vp]
    L.cgrt_debug_wave_times.argtypes = [vp, C.POINTER(Camera), i32, i32, vp, u64]
    L.cgrt_debug_trace_shadow.argtypes = [vp, vp, vp, u64, i32, u32, u64, u64, vp, u64, u64, u64, vp, vp, vp]
    L.cgrt_debug_soft_lit.argtypes = [vp, vp, vp, vp, u64, C.POINTER(SoftShadows), i32, i32, vp]
    L.cgrt_record_sizes.argtypes = [C.POINTER(u32)] * 4
    L.cgrt_record_sizes.restype = None
    L.cgrt_ray_triangle_batch.argtypes = [i32, vp, vp, u64, vp, vp, vp]
    L.cgrt_ray_plane_batch.argtypes = [i32, vp, vp, u64, vp, vp]
    L.cgrt_ray_box_batch.argtypes = [i32, vp, vp, u64, vp, vp, vp]
    L.cgrt_ray_sphere_batch.argtypes = [i32, vp, vp, u64, vp, vp, vp]
    L.cgrt_triangle_plane_batch.argtypes = [i32, vp, u64, vp]
    L.cgrt_point_in_triangle_batch.argtypes = [i32, vp, u64, vp]
    _lib = L
    return L


def _check(rc: int) -> None:
    if rc != 0:
        raise CgrtError(rc, lib().cgrt_last_error().decode())


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _vp(v):
    """A raw address or stream handle (an integer) as a pointer argument; 0 is NULL."""
    return C.c_void_p(v) if v else None


def _f32(a, shape) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))


def as_rays(origin, direction, t=None) -> np.ndarray:
    o = np.asarray(origin, np.float32).reshape(-1, 3)
    d = np.asarray(direction, np.float32).reshape(-1, 3)
    r = np.zeros(len(o), RAY_DTYPE)
    r["origin"], r["direction"] = o, d
    r["t"] = np.float32(np.finfo(np.float32).max) if t is None else np.asarray(t, np.float32)
    return r


def _as_ray_array(rays) -> np.ndarray:
    """RAY_DTYPE array from a RAY_DTYPE array or an (n, 7) float32 array {origin, direction, t} (viewed, never cast
    element by element)."""
    a = np.asarray(rays)
    if a.dtype != RAY_DTYPE:
        a = np.ascontiguousarray(a, np.float32)
        if a.ndim != 2 or a.shape[1] != 7:
            raise ValueError("rays must be a RAY_DTYPE array or an (n, 7) float32 array")
        a = a.view(RAY_DTYPE).reshape(-1)
    return np.ascontiguousarray(a)


def node_pack(boxes, refs, leaf_index: int = 0) -> np.ndarray:
    """cgrt_debug_node_pack: four child boxes (4, 6) {lower.xyz, upper.xyz}, four references and a leaf index -> the node's 32 words."""
    b = _f32(boxes, (4, 6))
    r = np.ascontiguousarray(refs, dtype=np.uint32).reshape(4)
    words = np.zeros(32, dtype=np.uint32)
    lib().cgrt_debug_node_pack(_ptr(b), _ptr(r), leaf_index, _ptr(words))
    return words


def node_unpack(words):
    """cgrt_debug_node_unpack: a node's 32 words -> (boxes (4, 6), refs (4,), leaf index) through the builder's load helpers."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(32)
    boxes = np.zeros((4, 6), dtype=np.float32)
    refs = np.zeros(4, dtype=np.uint32)
    li = C.c_uint32()
    lib().cgrt_debug_node_unpack(_ptr(w), _ptr(boxes), _ptr(refs), C.byref(li))
    return boxes, refs, li.value


def record_sizes() -> dict:
    v = [C.c_uint32() for _ in range(4)]
    lib().cgrt_record_sizes(*[C.byref(x) for x in v])
    return dict(zip(("node", "tri", "sub", "hit"), (int(x.value) for x in v)))


def set_leaf_accel(enabled: bool = True, sub_leaf_tris: int = 0) -> None:
    """Process-wide build option for scenes created afterwards (results are identical either way)."""
    _check(lib().cgrt_set_leaf_accel(1 if enabled else 0, sub_leaf_tris))


def set_primary_mode(mode: int) -> None:
    """0 = one wave per 8x8 tile, 1 = persistent waves with lane refill (same results)."""
    _check(lib().cgrt_set_primary_mode(int(mode)))


def set_kernel_shape(mode: int = -1, max_rays: int = 0) -> None:
    """-1 = by launch size (short lists are laid out sparsely: include/cgrt.h), 0 = 64 rays per wave always, 1 = quad per ray
    (16 per wave, frames too), 2 = 16 rays per wave for every list, 3 = 4 rays per wave for every list; max_rays = 0 keeps the
    threshold.  Same results whatever the shape."""
    _check(lib().cgrt_set_kernel_shape(int(mode), int(max_rays)))


def set_frame_hints(mode: int = -1) -> None:
    """Primary frames: -1 by frame size, 0 off, 1 the previous frame's hard tiles first, 2 hard tiles as four 16-ray waves; same pixels."""
    _check(lib().cgrt_set_frame_hints(int(mode)))


def set_frame_order(mode: int = -1) -> None:
    """Primary frames: -1 the library's policy (order tables for whole frames and large shares: include/cgrt.h), 0 off, 1 on wherever a
    frame qualifies; same pixels."""
    _check(lib().cgrt_set_frame_order(int(mode)))


def debug_build_frame_order(ticks) -> np.ndarray:
    """cgrt_debug_build_frame_order: the device builder's table for injected per-position ticks (uint16, padded to 8)."""
    t = np.ascontiguousarray(ticks, np.uint32)
    out = np.empty((len(t) + 7) // 8 * 8, np.uint16)
    _check(lib().cgrt_debug_build_frame_order(t.ctypes.data_as(C.POINTER(C.c_uint32)), len(t), out.ctypes.data_as(C.POINTER(C.c_uint16))))
    return out


def set_frame_gate(enabled: bool = True) -> None:
    """Camera frames: waves whose pixels all lie outside the root box's screen rectangle write their misses without tracing (default),
    or every pixel takes the per-pixel root gate; same bytes either way."""
    _check(lib().cgrt_set_frame_gate(1 if enabled else 0))


def debug_set_hint_thresholds(dense_ticks: int = 0, sparse_ticks: int = 0) -> None:
    _check(lib().cgrt_debug_set_hint_thresholds(int(dense_ticks), int(sparse_ticks)))


def set_render_prediction(enabled: bool = True) -> None:
    """cgrt_render*: size a frame's launches from the scene's previous frame of the same shape (default) or wait for the device's
    counts inside every frame; same pixels."""
    _check(lib().cgrt_set_render_prediction(1 if enabled else 0))


def kernel_shape() -> Tuple[int, int]:
    m, r = C.c_int(), C.c_uint64()
    _check(lib().cgrt_get_kernel_shape(C.byref(m), C.byref(r)))
    return int(m.value), int(r.value)


def set_call_combining(enabled: bool = True) -> None:
    """Small cgrt_intersect_batch calls of concurrent threads share one launch (default) or launch one by one; same results."""
    _check(lib().cgrt_set_call_combining(1 if enabled else 0))


def set_build_threads(threads: int = 0) -> None:
    """Worker threads of the host builders for scenes created afterwards (0 = hardware concurrency); the arrays do not depend on it."""
    _check(lib().cgrt_set_build_threads(int(threads)))


def set_fast_tree(mode: int) -> None:
    """Process-wide build option: -1 = fast tree for scenes with fat leaves (default), 0 = never, 1 = whenever possible."""
    _check(lib().cgrt_set_fast_tree(int(mode)))


def source_hash() -> str:
    """sha256[:16] of the sources the loaded library was built from (include/cgrt.h cgrt_source_hash)."""
    return lib().cgrt_source_hash().decode()


def device_count() -> int:
    return int(lib().cgrt_device_count())


# cgrt_render_device's output formats (include/cgrt.h CGRT_FRAME_*)
FRAME_FORMATS = {"rgb": 0, "chw": 1, "rgba8": 2}


def _frame_format(format) -> int:
    """"rgb" / "chw" / "rgba8" -> CGRT_FRAME_*; an int is passed through as it is (the library checks it)."""
    if isinstance(format, str):
        if format not in FRAME_FORMATS:
            raise ValueError(f"format must be one of {sorted(FRAME_FORMATS)}, not {format!r}")
        return FRAME_FORMATS[format]
    return int(format)


def rgba8_of(rgb, W: int, H: int) -> np.ndarray:
    """CGRT_FRAME_RGBA8 in numpy, for checking: the reference's 8-bit screen image (Screen::writeBitmapToFile, screen.cpp:38-49) of the
    frame rgb ((W*H, 3), index y*W + x) -- row H-1-y, bytes R, G, B, 255, each (uint8)(min(max(v, 0), 1) * 255.0f) in float32, truncated;
    a NaN channel gives 0.  Returns (H, W, 4) uint8."""
    v = np.asarray(rgb, np.float32).reshape(H, W, 3)
    with np.errstate(invalid="ignore"):
        c = np.where(v > 0, np.where(v < 1, v, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    out = np.empty((H, W, 4), np.uint8)
    out[..., :3] = (c * np.float32(255.0)).astype(np.uint8)[::-1]
    out[..., 3] = 255
    return out


def hip_runtimes() -> list:
    """Files of the HIP runtime (libamdhip64) this process has mapped.  torch ships a copy of its own; a process that has opened a
    second one (by another name) holds two runtimes, and streams and buffers of one mean nothing to the other."""
    found = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split(None, 5)
            if len(parts) == 6 and "libamdhip64" in os.path.basename(parts[5].strip()):
                found.add(os.path.realpath(parts[5].strip()))
    return sorted(found)


_one_runtime_seen = False


def _check_one_hip_runtime() -> None:
    """render_tensor's check that torch's streams and buffers belong to the runtime libcgrt.so uses: the process must map exactly one
    HIP runtime.  Reading /proc/self/maps costs about as much as the frame's host overhead, so the check runs until it first
    succeeds and not again: the runtime libcgrt.so is bound to stays the same for the life of the process."""
    global _one_runtime_seen
    if _one_runtime_seen:
        return
    runtimes = hip_runtimes()
    if len(runtimes) != 1:
        raise RuntimeError(f"the process maps {len(runtimes)} HIP runtimes ({runtimes}); render_tensor needs exactly one")
    _one_runtime_seen = True


def _frame_tensor_row_bytes(out, fmt: int, W: int, H: int, device: int) -> int:
    """Validates a caller's output tensor for Scene.render_tensor and returns its row pitch in bytes (ValueError otherwise)."""
    import torch

    if not isinstance(out, torch.Tensor):
        raise ValueError("out must be a torch tensor")
    dtype, shape = (torch.uint8, (H, W, 4)) if fmt == 2 else (torch.float32, ((3, H, W) if fmt == 1 else (H, W, 3)))
    if out.dtype != dtype:
        raise ValueError(f"out has dtype {out.dtype}, format needs {dtype}")
    if tuple(out.shape) != shape:
        raise ValueError(f"out has shape {tuple(out.shape)}, format needs {shape}")
    if out.device.type != "cuda" or out.device.index != device:
        raise ValueError(f"out is on {out.device}, the scene on cuda:{device}")
    st, es = out.stride(), out.element_size()
    if fmt == 1:  # (3, H, W): (H * s, s, 1); the plane stride is H rows
        s = st[1] if H > 1 else st[0]
        ok, pitched = (st[2] == 1 or W == 1) and st[0] == H * s, True
    else:  # (H, W, 3 | 4): (s, 3 | 4, 1); one row has no pitch
        s = st[0]
        ok, pitched = st[2] == 1 and (st[1] == shape[2] or W == 1), H > 1
    row_bytes = s * es
    if not ok or out.data_ptr() % 4 or (pitched and (row_bytes < W * (12 if fmt == 0 else 4) or row_bytes % 4)):
        raise ValueError(f"out's strides {st} (or its alignment) do not fit the format's row layout")
    return row_bytes if pitched else 0


def camera_array(cams) -> np.ndarray:
    """A batch of cameras for the *_views entries as a contiguous CgrtCamera array: from a (B, 9) float32 array in the layout of
    Camera.from_array (look_at, euler, distance, fovy, aspect) or a sequence of Camera.  Returns a (B, 9) float32 array (ValueError
    otherwise)."""
    if isinstance(cams, np.ndarray) or not all(isinstance(c, Camera) for c in cams):
        a = np.ascontiguousarray(np.asarray(cams, np.float32))
        if a.ndim != 2 or a.shape[1] != 9:
            raise ValueError(f"cams must be a (B, 9) float32 array or a sequence of Camera, not shape {a.shape}")
        return a
    a = np.empty((len(cams), 9), np.float32)
    for i, c in enumerate(cams):
        a[i, 0:3], a[i, 3:6], a[i, 6:9] = c.look_at[:], c.euler[:], (c.distance, c.fovy, c.aspect)
    return a


def unit_vector_table(n: int = 1 << 16, seed: int = 0) -> np.ndarray:
    """n draws of the reference's randomUnitVector() (main.cpp:46-59: three N(0,1) floats, glm::normalize) as input data
    for render_soft.  Any generator will do -- the table is data, not part of the parity contract."""
    g = np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)
    d = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    inv = np.float32(1.0) / np.sqrt(d, dtype=np.float32)
    return np.ascontiguousarray(g * inv[:, None], dtype=np.float32)


class Scene:
    """Owns a CgrtScene: the host mirror of ``BoundingVolumeHierarchy(Scene*)`` (bvh.h:39-48)."""

    def __init__(self, sd: SceneData, device: int = 0):
        self.sd = sd
        self._h = C.c_void_p()
        pn = _f32(sd.pos_nrm, (-1, 6))
        tri = np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
        tm = np.ascontiguousarray(sd.tri_mesh, np.uint32)
        mats = _f32(sd.materials, (-1, 8))
        sph = _f32(sd.spheres, (-1, 5))
        _check(
            lib().cgrt_scene_create(
                _ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats), _ptr(sph) if len(sph) else None,
                len(sph), device, C.byref(self._h),
            )
        )  # fmt: skip
        self.device = device

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            lib().cgrt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:
        if lib is not None and C is not None:  # module globals are already gone when the interpreter is shutting down
            self.close()

    def hint_counts(self):
        """Lengths of the three rotating hard lists of the primary frames' hints (diagnostics)."""
        out = (C.c_uint32 * 3)()
        _check(lib().cgrt_debug_hint_counts(self._h, out))
        return [int(v) for v in out]

    def debug_set_frame_order(self, W: int, H: int, table=None, rect=None, rank: int = 0, nranks: int = 1) -> None:
        """cgrt_debug_set_frame_order: install `table` for the next launches of that shape (None: back to the policy)."""
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
        if table is None:
            _check(lib().cgrt_debug_set_frame_order(self._h, int(W), int(H), x0, y0, x1, y1, int(rank), int(nranks), None, 0))
            return
        t = np.ascontiguousarray(table, np.uint16)
        _check(lib().cgrt_debug_set_frame_order(self._h, int(W), int(H), x0, y0, x1, y1, int(rank), int(nranks),
                                                t.ctypes.data_as(C.POINTER(C.c_uint16)), len(t)))

    def debug_get_frame_order(self):
        """cgrt_debug_get_frame_order: (table in use or None, state 0 none / 1 profiled / 2 active, launches since the profile frame)."""
        n, st = C.c_uint32(0), (C.c_int * 2)()
        _check(lib().cgrt_debug_get_frame_order(self._h, None, 0, C.byref(n), st))
        if n.value == 0:
            return None, int(st[0]), int(st[1])
        out = np.empty(n.value, np.uint16)
        _check(lib().cgrt_debug_get_frame_order(self._h, out.ctypes.data_as(C.POINTER(C.c_uint16)), n.value, C.byref(n), st))
        return out, int(st[0]), int(st[1])

    def frame_gate(self, cam, W: int, H: int):
        """cgrt_debug_frame_gate: (x0, y0, x1, y1) -- every pixel of the W x H frame outside it misses the mesh root gate ((0, 0, 0, 0):
        every pixel does) -- or None when the host computes no rectangle for this camera (the frame is not gated).  Host-only scenes too."""
        out = (C.c_int * 5)()
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(lib().cgrt_debug_frame_gate(self._h, C.byref(c), int(W), int(H), out))
        return (int(out[0]), int(out[1]), int(out[2]), int(out[3])) if out[4] else None

    def last_render_path(self) -> int:
        """0 = the last render() sized every list exactly, 1 = drawn as the previous frame predicted, 2 = predicted, too small, drawn again."""
        return int(lib().cgrt_debug_render_path(self._h))

    # ---- certified walk (same results as the exact walk) ----
    def set_walk(self, certified: bool) -> None:
        _check(lib().cgrt_scene_set_walk(self._h, 1 if certified else 0))

    def walk(self) -> int:
        """1 = certified walk (fast tree + certificate, exact walk as fallback), 0 = exact walk only."""
        return int(lib().cgrt_scene_walk(self._h))

    def build_info(self) -> dict:
        """What the host builder decided: fast tree built?, leaves with a degenerate float plane, finite geometry?, leaf count."""
        out = np.zeros(4, np.uint32)
        _check(lib().cgrt_scene_build_info(self._h, _ptr(out)))
        return dict(fast_tree=bool(out[0]), wild_leaves=int(out[1]), geometry_finite=bool(out[2]), leaves=int(out[3]))

    # ---- introspection ----
    def num_levels(self) -> int:
        return int(lib().cgrt_num_levels(self._h))

    def num_subnodes(self) -> int:
        return int(lib().cgrt_num_subnodes(self._h))

    def build_seconds(self) -> float:
        return float(lib().cgrt_build_seconds(self._h))

    def device_bytes(self) -> int:
        return int(lib().cgrt_device_bytes(self._h))

    def nodes(self) -> Tuple[np.ndarray, np.ndarray]:
        n = int(lib().cgrt_num_nodes(self._h))
        meta = np.zeros((n, 5), np.int32)
        boxes = np.zeros((n, 6), np.float32)
        if n:
            _check(lib().cgrt_get_nodes(self._h, _ptr(meta), _ptr(boxes)))
        return meta, boxes

    def leaf_prims(self, node: int) -> np.ndarray:
        n = int(lib().cgrt_leaf_prims(self._h, node, None, 0))
        out = np.zeros(n, np.uint32)
        if n:
            lib().cgrt_leaf_prims(self._h, node, _ptr(out), n)
        return out

    # ---- hot path ----
    def intersect(self, rays: np.ndarray, want_normals: bool = True):
        """Batched BoundingVolumeHierarchy::intersect. Returns (hits[HIT_DTYPE], normals or None)."""
        rays = _as_ray_array(rays)
        hits = np.zeros(len(rays), HIT_DTYPE)
        normals = np.zeros((len(rays), 3), np.float32) if want_normals else None
        _check(lib().cgrt_intersect_batch(self._h, _ptr(rays), len(rays), _ptr(hits), _ptr(normals)))
        return hits, normals

    def intersect_brute(self, rays: np.ndarray, mesh: int = -1, want_normals: bool = True):
        """cgrt_intersect_brute_batch: every triangle, no tree (ray_tracing.cpp:202-213). mesh < 0: all meshes + spheres."""
        rays = _as_ray_array(rays)
        hits = np.zeros(len(rays), HIT_DTYPE)
        normals = np.zeros((len(rays), 3), np.float32) if want_normals else None
        _check(lib().cgrt_intersect_brute_batch(self._h, _ptr(rays), len(rays), mesh, _ptr(hits), _ptr(normals)))
        return hits, normals

    def trace_primary(self, cam, W: int, H: int, rect=None, rank: int = 0, nranks: int = 1, want_normals: bool = False):
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
        hits = np.zeros(W * H, HIT_DTYPE)
        hits["prim_id"] = NO_PRIM
        hits["material_id"] = -1
        hits["t"] = np.nan  # pixels this call does not own stay marked
        normals = np.zeros((W * H, 3), np.float32) if want_normals else None
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(lib().cgrt_trace_primary(self._h, C.byref(c), W, H, x0, y0, x1, y1, rank, nranks, _ptr(hits), _ptr(normals)))
        return hits, normals

    def trace_primary_device(self, cam, W, H, d_hits_ptr: int, rect=None, rank=0, nranks=1, d_normals_ptr: int = 0, stream: int = 0):
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(
            lib().cgrt_trace_primary_device(
                self._h, C.byref(c), W, H, x0, y0, x1, y1, rank, nranks, C.c_void_p(d_hits_ptr),
                C.c_void_p(d_normals_ptr) if d_normals_ptr else None, C.c_void_p(stream) if stream else None,
            )
        )  # fmt: skip

    def intersect_device(self, d_rays_ptr: int, n: int, d_hits_ptr: int, d_normals_ptr: int = 0, stream: int = 0):
        _check(
            lib().cgrt_intersect_batch_device(
                self._h, C.c_void_p(d_rays_ptr), n, C.c_void_p(d_hits_ptr), C.c_void_p(d_normals_ptr) if d_normals_ptr else None,
                C.c_void_p(stream) if stream else None,
            )
        )  # fmt: skip

    def check_layout(self) -> None:
        """cgrt_debug_check_layout: raises when a reference of the record arrays is inconsistent."""
        _check(lib().cgrt_debug_check_layout(self._h))

    def subnodes(self) -> dict:
        """cgrt_debug_get_subnodes: the 4-wide nodes as the device reads them -- `words` (n, 32) uint32, one row per 128-byte node;
        `sub_base` the record index of node 0; `fast_root`; `leaf_roots` the record index of every reference leaf's accelerator root
        (0xffffffff: none)."""
        L = lib()
        n = self.num_subnodes()
        words = np.zeros((n // 2, 32), dtype=np.uint32)
        base, root, nleaves = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(L.cgrt_debug_get_subnodes(self._h, None, None, None, None, C.byref(nleaves)))
        roots = np.zeros(max(nleaves.value, 1), dtype=np.uint32)
        _check(L.cgrt_debug_get_subnodes(self._h, _ptr(words) if n else None, C.byref(base), C.byref(root), _ptr(roots), None))
        return {"words": words, "sub_base": base.value, "fast_root": root.value, "leaf_roots": roots[: nleaves.value]}

    def layout_hash(self) -> int:
        """cgrt_debug_layout_hash: FNV-1a over every array the device reads."""
        h = C.c_uint64()
        _check(lib().cgrt_debug_layout_hash(self._h, C.byref(h)))
        return int(h.value)

    def render(self, cam, W: int, H: int, lights=None, max_level: int = 2):
        """cgrt_render: the whole shading/recursion driver on the device. Returns (rgb[W*H,3], stats dict)."""
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        rgb = np.zeros((W * H, 3), np.float32)
        st = RenderStats()
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(lib().cgrt_render(self._h, C.byref(c), W, H, _ptr(lights), len(lights), max_level, _ptr(rgb), C.byref(st)))
        return rgb, {k: getattr(st, k) for k, _ in st._fields_}

    def render_mapped(self, cam, W: int, H: int, lights=None, max_level: int = 2):
        """cgrt_render_mapped: the frame stays in the scene's pinned staging memory; returns (a COPY of it as rgb[W*H,3], stats)
        -- the copy is for the caller's convenience here, the C caller reads the pinned frame in place."""
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        st = RenderStats()
        ptr = C.c_void_p()
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(lib().cgrt_render_mapped(self._h, C.byref(c), W, H, _ptr(lights), len(lights), None, max_level, C.byref(ptr), C.byref(st)))
        rgb = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(W * H, 3)).copy()
        return rgb, {k: getattr(st, k) for k, _ in st._fields_}

    def render_counted(self, cam, W: int, H: int, lights=None, max_level: int = 2):
        """cgrt_render_counted: (rgb, stats, {"primary" / "shadow" / "mirror": counters dict}) of an instrumented frame."""
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        rgb = np.zeros((W * H, 3), np.float32)
        st = RenderStats()
        work = (Counters * 3)()
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(lib().cgrt_render_counted(self._h, C.byref(c), W, H, _ptr(lights), len(lights), max_level, _ptr(rgb), C.byref(st), work))
        return rgb, {k: getattr(st, k) for k, _ in st._fields_}, dict(zip(("primary", "shadow", "mirror"), (w.as_dict() for w in work)))

    def render_soft(self, cam, W: int, H: int, spherical, units, samples: int = 200, seed: int = 0, lights=None, max_level: int = 2,
                    closest_hit: bool = False):
        """cgrt_render_soft: + spherical lights (n x 7 {position, radius, color}) sampled with `samples` shadow rays per hit
        (main.cpp:168-218); `units` (n x 3) are the randomUnitVector() draws, see unit_vector_table()."""
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        spherical = _f32(spherical, (-1, 7))
        units = _f32(units, (-1, 3))
        rgb = np.zeros((W * H, 3), np.float32)
        st = RenderStats()
        q = SoftShadows(spherical.ctypes.data, units.ctypes.data, len(spherical), samples, len(units), seed, int(closest_hit))
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(lib().cgrt_render_soft(self._h, C.byref(c), W, H, _ptr(lights), len(lights), C.byref(q), max_level, _ptr(rgb), C.byref(st)))
        return rgb, {k: getattr(st, k) for k, _ in st._fields_}

    def render_rank(self, cam, W: int, H: int, rank: int, nranks: int, rgb: Optional[np.ndarray] = None, lights=None, max_level: int = 2,
                    spherical=None, units=None, samples: int = 200, seed: int = 0):
        """cgrt_render_rank: this rank's super-tiles of the frame (shading included); other pixels of `rgb` are kept."""
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        rgb = np.zeros((W * H, 3), np.float32) if rgb is None else rgb
        assert rgb.dtype == np.float32 and rgb.size == W * H * 3 and rgb.flags.c_contiguous
        st = RenderStats()
        q = None
        if spherical is not None:
            spherical, units = _f32(spherical, (-1, 7)), _f32(units, (-1, 3))
            q = C.byref(SoftShadows(spherical.ctypes.data, units.ctypes.data, len(spherical), samples, len(units), seed, 0))
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(lib().cgrt_render_rank(self._h, C.byref(c), W, H, _ptr(lights), len(lights), q, max_level, rank, nranks, _ptr(rgb), C.byref(st)))
        return rgb, {k: getattr(st, k) for k, _ in st._fields_}

    def render_aa(self, cam, W: int, H: int, lights=None, max_level: int = 2, spherical=None, units=None, samples: int = 200, seed: int = 0,
                  rank: int = 0, nranks: int = 1, mapped: bool = False, rgb: Optional[np.ndarray] = None):
        """cgrt_render_aa / cgrt_render_aa_mapped: the reference's 2x2 anti-aliasing (main.cpp:663-687) -- 4 sub-samples per pixel,
        summed in loop order and divided by 5.0f.  rank/nranks: this rank's 32x32-pixel blocks only, other pixels of `rgb` are
        kept.  mapped=True (whole frame only) reads the scene's pinned frame and returns a copy.  Returns (rgb[W*H,3], stats dict)."""
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        st = RenderStats()
        q = None
        if spherical is not None:
            spherical, units = _f32(spherical, (-1, 7)), _f32(units, (-1, 3))
            q = C.byref(SoftShadows(spherical.ctypes.data, units.ctypes.data, len(spherical), samples, len(units), seed, 0))
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        if mapped:
            if nranks != 1 or rgb is not None:
                raise ValueError("render_aa(mapped=True) returns the whole frame: rank/nranks/rgb do not apply")
            ptr = C.c_void_p()
            _check(lib().cgrt_render_aa_mapped(self._h, C.byref(c), W, H, _ptr(lights), len(lights), q, max_level, C.byref(ptr), C.byref(st)))
            rgb = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(W * H, 3)).copy()
        else:
            rgb = np.zeros((W * H, 3), np.float32) if rgb is None else rgb
            assert rgb.dtype == np.float32 and rgb.size == W * H * 3 and rgb.flags.c_contiguous
            _check(lib().cgrt_render_aa(self._h, C.byref(c), W, H, _ptr(lights), len(lights), q, max_level, rank, nranks, _ptr(rgb), C.byref(st)))
        return rgb, {k: getattr(st, k) for k, _ in st._fields_}

    def render_device(self, cam, W: int, H: int, d_out_ptr: int, format="rgb", row_bytes: int = 0, stream: int = 0, aa: bool = False,
                      lights=None, max_level: int = 2, spherical=None, units=None, samples: int = 200, seed: int = 0, rank: int = 0,
                      nranks: int = 1) -> dict:
        """cgrt_render_device: the frame of render_soft (aa=False) / render_aa (aa=True) written by a device kernel into the device buffer
        at d_out_ptr (format "rgb" (H, W, 3) f32, "chw" (3, H, W) f32 or "rgba8" (H, W, 4) u8 flipped; row_bytes 0 = packed), enqueued on
        the hipStream_t `stream` (0 = default stream).  Raw integers, as trace_primary_device.  Returns the stats dict."""
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        st = RenderStats()
        q = None
        if spherical is not None:
            spherical, units = _f32(spherical, (-1, 7)), _f32(units, (-1, 3))
            q = C.byref(SoftShadows(spherical.ctypes.data, units.ctypes.data, len(spherical), samples, len(units), seed, 0))
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(
            lib().cgrt_render_device(
                self._h, C.byref(c), W, H, _ptr(lights), len(lights), q, max_level, 1 if aa else 0, rank, nranks,
                C.c_void_p(d_out_ptr) if d_out_ptr else None, _frame_format(format), int(row_bytes), C.c_void_p(stream) if stream else None,
                C.byref(st),
            )
        )  # fmt: skip
        return {k: getattr(st, k) for k, _ in st._fields_}

    def render_tensor(self, cam, W: int, H: int, format="rgb", out=None, stream=None, **kw):
        """render_device into a torch tensor: (H, W, 3) f32, (3, H, W) f32 or (H, W, 4) u8 on cuda:<device> -- `out` (any row stride, e.g.
        a slice of a larger canvas; validated before any call, ValueError) or a new tensor (zeros when nranks > 1), rendered on `stream`
        (default: torch.cuda.current_stream()).  Other keywords as render_device.  Returns (tensor, stats dict).
        Import torch before the library is first used (lib()): torch then brings the one HIP runtime both use; the other way round
        torch finds no device."""
        out, fmt, row_bytes, stream = self._frame_tensor(W, H, format, out, stream, kw.get("nranks", 1))
        st = self.render_device(cam, W, H, out.data_ptr(), format=fmt, row_bytes=row_bytes, stream=stream.cuda_stream, **kw)
        return out, st

    def _frame_tensor(self, W, H, format, out, stream, nranks):
        """render_tensor's checks of `out` (ValueError) and its new tensor: (out, format code, row pitch, stream)."""
        import torch

        fmt = _frame_format(format)
        row_bytes = 0
        if out is not None:
            row_bytes = _frame_tensor_row_bytes(out, fmt, W, H, self.device)
        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        if out is None:
            shape, dtype = {0: ((H, W, 3), torch.float32), 1: ((3, H, W), torch.float32), 2: ((H, W, 4), torch.uint8)}[fmt]
            with torch.cuda.stream(stream):  # (allocated, and zeroed, on the stream the frame is exported on)
                out = (torch.zeros if nranks > 1 else torch.empty)(shape, dtype=dtype, device=dev)
        return out, fmt, row_bytes, stream

    # ---- multi-view frames (include/cgrt.h cgrt_*_views*) ----
    def trace_views_device(self, cams, W: int, H: int, d_hits_ptr: int, d_normals_ptr: int = 0, stream: int = 0) -> None:
        """cgrt_trace_primary_views_device: the primary hits of B cameras ((B, 9) array or sequence of Camera) into B*W*H CgrtHit at
        d_hits_ptr (and B*W*H*3 floats at d_normals_ptr), view b's pixel (x, y) at b*W*H + y*W + x; asynchronous on `stream`."""
        a = camera_array(cams)
        _check(
            lib().cgrt_trace_primary_views_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, C.c_void_p(d_hits_ptr) if d_hits_ptr else None,
                C.c_void_p(d_normals_ptr) if d_normals_ptr else None, C.c_void_p(stream) if stream else None,
            )
        )  # fmt: skip

    def render_views(self, cams, W: int, H: int, lights=None, max_level: int = 2, spherical=None, units=None, samples: int = 200,
                     seed: int = 0):
        """cgrt_render_views: view b of the result is render_soft (render without spherical lights) of cams[b], bit for bit; one primary
        launch and one wavefront for all views.  Returns (rgb[B, W*H, 3], stats dict summed over the views)."""
        a = camera_array(cams)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        rgb = np.zeros((len(a), W * H, 3), np.float32)
        st = RenderStats()
        _check(lib().cgrt_render_views(self._h, _ptr(a) if len(a) else None, len(a), W, H, _ptr(lights), len(lights), q, max_level, _ptr(rgb),
                                       C.byref(st)))
        return rgb, {k: getattr(st, k) for k, _ in st._fields_}

    def render_views_device(self, cams, W: int, H: int, d_out_ptr: int, format="rgb", stream: int = 0, lights=None, max_level: int = 2,
                            spherical=None, units=None, samples: int = 200, seed: int = 0) -> dict:
        """cgrt_render_views_device: the views exported into device memory at d_out_ptr, view b at b * (packed frame bytes), each in the
        packed layout of render_device's `format`; enqueued on the hipStream_t `stream`.  Raw integers, as render_device.  Returns stats."""
        a = camera_array(cams)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        st = RenderStats()
        _check(
            lib().cgrt_render_views_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, _ptr(lights), len(lights), q, max_level,
                C.c_void_p(d_out_ptr) if d_out_ptr else None, _frame_format(format), C.c_void_p(stream) if stream else None, C.byref(st),
            )
        )  # fmt: skip
        return {k: getattr(st, k) for k, _ in st._fields_}

    def render_views_tensor(self, cams, W: int, H: int, format="rgb", out=None, stream=None, **kw):
        """render_views_device into a torch tensor on cuda:<device>: (B, H, W, 3) f32, (B, 3, H, W) f32 or (B, H, W, 4) u8 -- `out`
        (contiguous, of exactly that shape and dtype; validated before any call, ValueError) or a new tensor, rendered on `stream`
        (default: torch.cuda.current_stream()).  Other keywords as render_views.  Returns (tensor, stats dict)."""
        a, out, fmt, stream = self._views_tensor(cams, W, H, format, out, stream)
        st = self.render_views_device(a, W, H, out.data_ptr(), format=fmt, stream=stream.cuda_stream, **kw)
        return out, st

    def _views_tensor(self, cams, W, H, format, out, stream):
        """render_views_tensor's checks of `out` (ValueError) and its new tensor: (camera array, out, format code, stream)."""
        a = camera_array(cams)
        out, fmt, stream = self._batch_tensor((len(a),), W, H, format, out, stream)
        return a, out, fmt, stream

    def _batch_tensor(self, lead, W, H, format, out, stream):
        """The checks of `out` (ValueError) for a batch of frames exported back to back (views, light sets, views x light sets), with the
        leading shape `lead` ((B,) or (V, S)), and its new tensor: (out, format code, stream)."""
        import torch

        fmt = _frame_format(format)
        lead = tuple(lead)
        shape, dtype = {0: (lead + (H, W, 3), torch.float32), 1: (lead + (3, H, W), torch.float32), 2: (lead + (H, W, 4), torch.uint8)}.get(
            fmt, (None, None))
        if shape is None:
            raise ValueError(f"format must be one of {sorted(FRAME_FORMATS)}, not {format!r}")
        if out is not None:
            if not isinstance(out, torch.Tensor):
                raise ValueError("out must be a torch tensor")
            if out.dtype != dtype:
                raise ValueError(f"out has dtype {out.dtype}, format needs {dtype}")
            if tuple(out.shape) != shape:
                raise ValueError(f"out has shape {tuple(out.shape)}, format needs {shape}")
            if not out.is_contiguous():
                raise ValueError("out must be contiguous")
            if out.device.type != "cuda" or out.device.index != self.device:
                raise ValueError(f"out is on {out.device}, the scene on cuda:{self.device}")
        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        if out is None:
            with torch.cuda.stream(stream):  # (allocated on the stream the frames are exported on)
                out = torch.empty(shape, dtype=dtype, device=dev)
        return out, fmt, stream

    # ---- light sets (include/cgrt.h cgrt_render_light_sets*) ----
    @staticmethod
    def _light_sets_arg(light_sets, spherical_sets):
        """The CgrtLightSets argument built from B arrays of point lights (L_b x 6) and None or B arrays of spherical lights (S_b x 7), and the
        CSR arrays it points into, which the caller keeps alive.  ValueError for sequences of different lengths or bad shapes."""

        def csr(seq, width, what):
            arrs = []
            for b, x in enumerate(seq):
                a = np.asarray(x, np.float32)
                if a.size == 0:
                    a = a.reshape(0, width)
                if a.ndim != 2 or a.shape[1] != width:
                    raise ValueError(f"{what}[{b}] has shape {a.shape}, expected (n, {width})")
                arrs.append(a)
            offsets = np.zeros(len(arrs) + 1, np.uint32)
            if arrs:
                offsets[1:] = np.cumsum([len(a) for a in arrs])
            flat = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros((0, width), np.float32), np.float32)
            return flat, offsets

        light_sets = list(light_sets)
        lights, loff = csr(light_sets, 6, "light_sets")
        sph, soff = None, None
        if spherical_sets is not None:
            spherical_sets = list(spherical_sets)
            if len(spherical_sets) != len(light_sets):
                raise ValueError(f"{len(light_sets)} light sets but {len(spherical_sets)} spherical sets")
            sph, soff = csr(spherical_sets, 7, "spherical_sets")
        q = LightSets(len(light_sets), lights.ctypes.data if len(lights) else None, loff.ctypes.data,
                      sph.ctypes.data if sph is not None and len(sph) else None, soff.ctypes.data if soff is not None else None)
        return q, (lights, loff, sph, soff)

    def _light_sets_soft(self, spherical_sets, units, samples: int, seed: int):
        """The sampling parameters of a light-set batch (CgrtSoftShadows without lights; None when no set has spherical lights)."""
        if spherical_sets is None or units is None:
            return None, ()
        units = _f32(units, (-1, 3))
        return C.byref(SoftShadows(None, units.ctypes.data, 0, samples, len(units), seed, 0)), (units,)

    def render_light_sets(self, cam, W: int, H: int, light_sets, spherical_sets=None, units=None, samples: int = 200, seed: int = 0,
                          max_level: int = 2):
        """cgrt_render_light_sets: frame b of the result is render_soft (render without spherical lights) of cam under light_sets[b] (and
        spherical_sets[b]), bit for bit; the batch traces the ray tree once and every distinct light position once.  light_sets: B arrays
        (L_b, 6); spherical_sets: None or B arrays (S_b, 7).  Returns (rgb[B, W*H, 3], stats dict of the batch)."""
        q, keep = self._light_sets_arg(light_sets, spherical_sets)  # noqa: F841
        s, keep_s = self._light_sets_soft(spherical_sets, units, samples, seed)  # noqa: F841
        rgb = np.zeros((q.nsets, W * H, 3), np.float32)
        st = RenderStats()
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(lib().cgrt_render_light_sets(self._h, C.byref(c), W, H, C.byref(q), s, max_level, _ptr(rgb), C.byref(st)))
        return rgb, {k: getattr(st, k) for k, _ in st._fields_}

    def render_light_sets_device(self, cam, W: int, H: int, d_out_ptr: int, light_sets, spherical_sets=None, units=None, samples: int = 200,
                                 seed: int = 0, max_level: int = 2, format="rgb", stream: int = 0) -> dict:
        """cgrt_render_light_sets_device: the sets' frames exported into device memory at d_out_ptr, set b at b * (packed frame bytes), each
        in the packed layout of render_device's `format`; enqueued on the hipStream_t `stream`.  Raw integers, as render_device.  Returns
        the stats dict."""
        q, keep = self._light_sets_arg(light_sets, spherical_sets)  # noqa: F841
        s, keep_s = self._light_sets_soft(spherical_sets, units, samples, seed)  # noqa: F841
        st = RenderStats()
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(
            lib().cgrt_render_light_sets_device(
                self._h, C.byref(c), W, H, C.byref(q), s, max_level, C.c_void_p(d_out_ptr) if d_out_ptr else None, _frame_format(format),
                C.c_void_p(stream) if stream else None, C.byref(st),
            )
        )  # fmt: skip
        return {k: getattr(st, k) for k, _ in st._fields_}

    def render_light_sets_tensor(self, cam, W: int, H: int, light_sets, format="rgb", out=None, stream=None, **kw):
        """render_light_sets_device into a torch tensor on cuda:<device>: (B, H, W, 3) f32, (B, 3, H, W) f32 or (B, H, W, 4) u8 -- `out`
        (contiguous, of exactly that shape and dtype; validated before any call, ValueError) or a new tensor, rendered on `stream`
        (default: torch.cuda.current_stream()).  Other keywords as render_light_sets.  Returns (tensor, stats dict)."""
        light_sets = list(light_sets)
        self._light_sets_arg(light_sets, kw.get("spherical_sets"))  # (ValueError before anything is allocated)
        out, fmt, stream = self._batch_tensor((len(light_sets),), W, H, format, out, stream)
        st = self.render_light_sets_device(cam, W, H, out.data_ptr(), light_sets, format=fmt, stream=stream.cuda_stream, **kw)
        return out, st

    # ---- multi-view light sets (include/cgrt.h cgrt_render_views_light_sets*) ----
    def render_views_light_sets(self, cams, W: int, H: int, light_sets, spherical_sets=None, units=None, samples: int = 200, seed: int = 0,
                                max_level: int = 2):
        """cgrt_render_views_light_sets: frame (v, s) of the result is render_soft (render without spherical lights) of cams[v] under
        light_sets[s] (and spherical_sets[s]), bit for bit; one wavefront for all views, shadow rays once per distinct light position.
        cams as render_views, the sets as render_light_sets.  Returns (rgb[V, S, W*H, 3], stats dict of the batch)."""
        a = camera_array(cams)
        q, keep = self._light_sets_arg(light_sets, spherical_sets)  # noqa: F841
        s, keep_s = self._light_sets_soft(spherical_sets, units, samples, seed)  # noqa: F841
        rgb = np.zeros((len(a), q.nsets, W * H, 3), np.float32)
        st = RenderStats()
        _check(lib().cgrt_render_views_light_sets(self._h, _ptr(a) if len(a) else None, len(a), W, H, C.byref(q), s, max_level, _ptr(rgb),
                                                  C.byref(st)))
        return rgb, {k: getattr(st, k) for k, _ in st._fields_}

    def render_views_light_sets_device(self, cams, W: int, H: int, d_out_ptr: int, light_sets, spherical_sets=None, units=None,
                                       samples: int = 200, seed: int = 0, max_level: int = 2, format="rgb", stream: int = 0) -> dict:
        """cgrt_render_views_light_sets_device: the V x S frames exported into device memory at d_out_ptr, frame (v, s) at (v * S + s) *
        (packed frame bytes), each in the packed layout of render_device's `format`; enqueued on the hipStream_t `stream`.  Raw integers, as
        render_device.  Returns the stats dict."""
        a = camera_array(cams)
        q, keep = self._light_sets_arg(light_sets, spherical_sets)  # noqa: F841
        s, keep_s = self._light_sets_soft(spherical_sets, units, samples, seed)  # noqa: F841
        st = RenderStats()
        _check(
            lib().cgrt_render_views_light_sets_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, C.byref(q), s, max_level, C.c_void_p(d_out_ptr) if d_out_ptr else None,
                _frame_format(format), C.c_void_p(stream) if stream else None, C.byref(st),
            )
        )  # fmt: skip
        return {k: getattr(st, k) for k, _ in st._fields_}

    def _views_light_sets_tensor(self, cams, W, H, light_sets, spherical_sets, format, out, stream):
        """The checks (ValueError, before any call) and the (V, S, ...) tensor of the *_views_light_sets_tensor forms: (cams, sets, the
        CgrtLightSets argument and the arrays it points into, out, format code, stream)."""
        a = camera_array(cams)
        light_sets = list(light_sets)
        q, keep = self._light_sets_arg(light_sets, spherical_sets)
        out, fmt, stream = self._batch_tensor((len(a), len(light_sets)), W, H, format, out, stream)
        return a, light_sets, (q, keep), out, fmt, stream

    def render_views_light_sets_tensor(self, cams, W: int, H: int, light_sets, format="rgb", out=None, stream=None, **kw):
        """render_views_light_sets_device into a torch tensor on cuda:<device>: (V, S, H, W, 3) f32, (V, S, 3, H, W) f32 or (V, S, H, W, 4)
        u8 -- `out` (contiguous, of exactly that shape and dtype; validated before any call, ValueError) or a new tensor, rendered on
        `stream` (default: torch.cuda.current_stream()).  Other keywords as render_views_light_sets.  Returns (tensor, stats dict)."""
        a, light_sets, _, out, fmt, stream = self._views_light_sets_tensor(cams, W, H, light_sets, kw.get("spherical_sets"), format, out, stream)
        st = self.render_views_light_sets_device(a, W, H, out.data_ptr(), light_sets, format=fmt, stream=stream.cuda_stream, **kw)
        return out, st

    def _soft_arg(self, spherical, units, samples: int, seed: int):
        """The CgrtSoftShadows argument (None without spherical lights) and the arrays it points into, which the caller keeps alive."""
        if spherical is None:
            return None, ()
        spherical, units = _f32(spherical, (-1, 7)), _f32(units, (-1, 3))
        return C.byref(SoftShadows(spherical.ctypes.data, units.ctypes.data, len(spherical), samples, len(units), seed, 0)), (spherical, units)

    def shade_rays(self, rays, lights=None, max_level: int = 2, spherical=None, units=None, samples: int = 200, seed: int = 0):
        """cgrt_shade_rays: getFinalColor (main.cpp:298-310) of each of the caller's rays (a RAY_DTYPE array or (n, 7) float32 {origin,
        direction, t}), recursion cut at max_level; spherical lights as render_soft, sample smp of ray i hashed with pixel i.
        Returns (rgb[n, 3], stats dict)."""
        r = _as_ray_array(rays)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841  (keep: the arrays q points into)
        rgb = np.zeros((len(r), 3), np.float32)
        st = RenderStats()
        _check(lib().cgrt_shade_rays(self._h, _ptr(r), len(r), _ptr(lights), len(lights), q, max_level, _ptr(rgb), C.byref(st)))
        return rgb, {k: getattr(st, k) for k, _ in st._fields_}

    def shade_rays_device(self, d_rays_ptr: int, n: int, d_rgb_ptr: int, stream: int = 0, lights=None, max_level: int = 2, spherical=None,
                          units=None, samples: int = 200, seed: int = 0) -> dict:
        """cgrt_shade_rays_device: n rays (7 floats each) at d_rays_ptr shaded into n x 3 floats at d_rgb_ptr, ordered on the hipStream_t
        `stream` (0 = default stream).  Raw integers, as render_device.  Returns the stats dict."""
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        st = RenderStats()
        _check(
            lib().cgrt_shade_rays_device(
                self._h, C.c_void_p(d_rays_ptr) if d_rays_ptr else None, int(n), _ptr(lights), len(lights), q, max_level,
                C.c_void_p(d_rgb_ptr) if d_rgb_ptr else None, C.c_void_p(stream) if stream else None, C.byref(st),
            )
        )  # fmt: skip
        return {k: getattr(st, k) for k, _ in st._fields_}

    def shade_rays_tensor(self, rays, out=None, stream=None, **kw):
        """shade_rays on torch tensors: rays (..., 7) float32, contiguous, on cuda:<device> -> colours (..., 3) float32, e.g. (H, W, 7)
        rays give an (H, W, 3) image.  Into `out` (validated before any call, ValueError, as render_tensor validates its output) or a new
        tensor, ordered on `stream` (default: torch.cuda.current_stream()).  Other keywords as shade_rays.  Returns (tensor, stats dict)."""
        out, n, stream = self._rays_tensor(rays, out, stream)
        if n == 0:  # (an empty tensor has no address to pass: the call would touch nothing anyway)
            return out, {k: 0 for k, _ in RenderStats._fields_}
        st = self.shade_rays_device(rays.data_ptr(), n, out.data_ptr(), stream=stream.cuda_stream, **kw)
        return out, st

    def _rays_tensor(self, rays, out, stream):
        """shade_rays_tensor's checks of `rays` and `out` (ValueError) and its new tensor: (out, number of rays, stream)."""
        import torch

        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        if not isinstance(rays, torch.Tensor) or rays.dim() < 1 or rays.shape[-1] != 7:
            raise ValueError("rays must be a torch tensor of shape (..., 7)")
        if rays.dtype != torch.float32:
            raise ValueError(f"rays has dtype {rays.dtype}, needs torch.float32")
        if rays.device.type != "cuda" or rays.device.index != self.device:
            raise ValueError(f"rays is on {rays.device}, the scene on cuda:{self.device}")
        if not rays.is_contiguous():
            raise ValueError("rays must be contiguous")
        n = rays.numel() // 7
        shape = tuple(rays.shape[:-1]) + (3,)
        if out is not None:
            if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape:
                raise ValueError(f"out must be a torch tensor of shape {shape}")
            if not out.is_contiguous():
                raise ValueError("out must be contiguous")
            if n:  # render_tensor's check of an (H, W, 3) f32 frame: dtype, device, strides, alignment
                _frame_tensor_row_bytes(out.view(1, n, 3), FRAME_FORMATS["rgb"], n, 1, self.device)
        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        if out is None:
            with torch.cuda.stream(stream):  # (allocated on the stream the colours are written on)
                out = torch.empty(shape, dtype=torch.float32, device=dev)
        return out, n, stream

    # ---- enqueued frames (include/cgrt.h cgrt_enqueue_*) ----
    # These return as soon as the frame is enqueued on `stream`; the tensors the frame reads or writes must stay alive, and unused by other
    # streams, until it has run there.  A tensor made on another stream (rays written elsewhere, an `out` allocated elsewhere) needs the
    # usual torch handling: make `stream` wait for its producer (stream.wait_stream) and call tensor.record_stream(stream), so that the
    # caching allocator does not hand its memory out again while the frame still uses it.  The host arrays (cameras, lights, soft-shadow
    # tables) are copied by the call.
    def enqueue_render_tensor(self, cam, W: int, H: int, format="rgb", out=None, stream=None, aa: bool = False, lights=None, max_level: int = 2,
                              spherical=None, units=None, samples: int = 200, seed: int = 0, rank: int = 0, nranks: int = 1):
        """render_tensor without waiting for the GPU (cgrt_enqueue_render_device): same checks (ValueError before any call), same bytes,
        the whole frame on `stream` (default: torch.cuda.current_stream()).  Returns (tensor, ticket); enqueue_stats(ticket) gives the
        stats dict."""
        out, fmt, row_bytes, stream = self._frame_tensor(W, H, format, out, stream, nranks)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        t = C.c_uint64()
        _check(
            lib().cgrt_enqueue_render_device(
                self._h, C.byref(c), W, H, _ptr(lights), len(lights), q, max_level, 1 if aa else 0, rank, nranks, C.c_void_p(out.data_ptr()),
                fmt, int(row_bytes), C.c_void_p(stream.cuda_stream) if stream.cuda_stream else None, C.byref(t),
            )
        )  # fmt: skip
        return out, t.value

    def enqueue_render_views_tensor(self, cams, W: int, H: int, format="rgb", out=None, stream=None, lights=None, max_level: int = 2,
                                    spherical=None, units=None, samples: int = 200, seed: int = 0):
        """render_views_tensor without waiting for the GPU (cgrt_enqueue_render_views_device).  Returns (tensor, ticket)."""
        a, out, fmt, stream = self._views_tensor(cams, W, H, format, out, stream)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        t = C.c_uint64()
        _check(
            lib().cgrt_enqueue_render_views_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, _ptr(lights), len(lights), q, max_level, C.c_void_p(out.data_ptr()), fmt,
                C.c_void_p(stream.cuda_stream) if stream.cuda_stream else None, C.byref(t),
            )
        )  # fmt: skip
        return out, t.value

    def enqueue_render_views_light_sets_tensor(self, cams, W: int, H: int, light_sets, format="rgb", out=None, stream=None, spherical_sets=None,
                                               units=None, samples: int = 200, seed: int = 0, max_level: int = 2):
        """render_views_light_sets_tensor without waiting for the GPU (cgrt_enqueue_render_views_light_sets_device): same checks (ValueError
        before any call), same bytes, the whole batch on `stream`.  With one camera it is the enqueued light-set batch.  Returns (tensor,
        ticket); enqueue_stats(ticket) gives the stats dict."""
        a, light_sets, (q, keep), out, fmt, stream = self._views_light_sets_tensor(cams, W, H, light_sets, spherical_sets, format, out, stream)
        s, keep_s = self._light_sets_soft(spherical_sets, units, samples, seed)  # noqa: F841
        t = C.c_uint64()
        _check(
            lib().cgrt_enqueue_render_views_light_sets_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, C.byref(q), s, max_level, C.c_void_p(out.data_ptr()), fmt,
                C.c_void_p(stream.cuda_stream) if stream.cuda_stream else None, C.byref(t),
            )
        )  # fmt: skip
        return out, t.value

    def enqueue_shade_rays_tensor(self, rays, out=None, stream=None, lights=None, max_level: int = 2, spherical=None, units=None,
                                  samples: int = 200, seed: int = 0):
        """shade_rays_tensor without waiting for the GPU (cgrt_enqueue_shade_rays_device): the frame starts behind everything on `stream`
        (the kernel that wrote `rays`, when it ran there).  rays written on another stream: stream.wait_stream(that stream) first, and
        rays.record_stream(stream), as for any torch op.  Returns (tensor, ticket).  An empty list enqueues no work but still gets a ticket
        (its stats are zero); an empty tensor has no device address, so the call is handed the ticket's own address for d_rgb, which the
        entry's NULL check accepts and nothing reads when n == 0."""
        out, n, stream = self._rays_tensor(rays, out, stream)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        t = C.c_uint64()
        _check(
            lib().cgrt_enqueue_shade_rays_device(
                self._h, C.c_void_p(rays.data_ptr()) if n else None, n, _ptr(lights), len(lights), q, max_level,
                C.c_void_p(out.data_ptr() if n else C.addressof(t)), C.c_void_p(stream.cuda_stream) if stream.cuda_stream else None, C.byref(t),
            )
        )  # fmt: skip
        return out, t.value

    def enqueue_stats(self, ticket: int) -> dict:
        """cgrt_enqueue_stats: waits for the enqueued frame `ticket` and returns its stats dict (CgrtError CGRT_E_ARG for a ticket that was
        never issued or has left the scene's ring of the last 8 enqueued frames)."""
        st = RenderStats()
        _check(lib().cgrt_enqueue_stats(self._h, int(ticket), C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    # ---- geometry buffers of a device frame (include/cgrt.h CgrtAovOut, cgrt_*_aov_device) ----
    @staticmethod
    def _aov_arg(aov, chw):
        """The CgrtAovOut argument: None (NULL), an AovOut, or a dict plane name -> device address."""
        if aov is None:
            return None
        return C.byref(aov if isinstance(aov, AovOut) else AovOut.from_pointers(aov, chw))

    def render_aov_device(self, cam, W: int, H: int, d_out_ptr: int, aov, chw: bool = False, format="rgb", row_bytes: int = 0, stream: int = 0,
                          aa: bool = False, lights=None, max_level: int = 2, spherical=None, units=None, samples: int = 200, seed: int = 0,
                          rank: int = 0, nranks: int = 1) -> dict:
        """cgrt_render_aov_device: render_device, and the geometry buffers of the frame's primary rays -- `aov`, a dict plane name (AOV_NAMES)
        -> device address of a packed plane: (H, W) f32 depth, u32 prim_id, i32 material_id, u8 mask; (H, W, 3) f32 normal, position, albedo,
        or (3, H, W) with chw; (2H, 2W) with aa -- written by the same call from the frame's own level 0.  Raw integers.  Returns stats."""
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        st = RenderStats()
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(
            lib().cgrt_render_aov_device(
                self._h, C.byref(c), W, H, _ptr(lights), len(lights), q, max_level, 1 if aa else 0, rank, nranks,
                C.c_void_p(d_out_ptr) if d_out_ptr else None, _frame_format(format), int(row_bytes), C.c_void_p(stream) if stream else None,
                C.byref(st), self._aov_arg(aov, chw),
            )
        )  # fmt: skip
        return {k: getattr(st, k) for k, _ in st._fields_}

    def render_views_aov_device(self, cams, W: int, H: int, d_out_ptr: int, aov, chw: bool = False, format="rgb", stream: int = 0, lights=None,
                                max_level: int = 2, spherical=None, units=None, samples: int = 200, seed: int = 0) -> dict:
        """cgrt_render_views_aov_device: render_views_device, and the views' geometry buffers with a leading view axis: (B, H, W),
        (B, H, W, 3) or (B, 3, H, W).  Raw integers, as render_aov_device.  Returns stats."""
        a = camera_array(cams)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        st = RenderStats()
        _check(
            lib().cgrt_render_views_aov_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, _ptr(lights), len(lights), q, max_level,
                C.c_void_p(d_out_ptr) if d_out_ptr else None, _frame_format(format), C.c_void_p(stream) if stream else None, C.byref(st),
                self._aov_arg(aov, chw),
            )
        )  # fmt: skip
        return {k: getattr(st, k) for k, _ in st._fields_}

    def _aov_plan(self, lead, W, H, aovs, chw, aov_out):
        """The checks of `aovs` / `aov_out` (ValueError, before any call): the planes as a dict name -> (shape, dtype, caller's tensor or
        None), shape lead + (H, W) (+ (3,), or lead + (3, H, W) with chw); a caller's tensor is contiguous, of exactly that shape and
        dtype, on the scene's device."""
        import torch

        names = (aovs,) if isinstance(aovs, str) else tuple(aovs)
        if not names or len(set(names)) != len(names) or any(k not in AOV_NAMES for k in names):
            raise ValueError(f"aovs must be a non-empty subset of {AOV_NAMES} without repeats, not {aovs!r}")
        aov_out = {} if aov_out is None else aov_out
        if not isinstance(aov_out, dict) or any(k not in names for k in aov_out):
            raise ValueError(f"aov_out must be a dict of tensors whose keys are among the requested planes {names}")
        lead = tuple(lead)
        one, three = lead + (H, W), lead + ((3, H, W) if chw else (H, W, 3))
        plan = {}
        for k in names:
            shape = three if k in ("normal", "position", "albedo") else one
            dtype = torch.uint8 if k == "mask" else torch.int32 if k in ("prim_id", "material_id") else torch.float32
            t = aov_out.get(k)
            if t is not None:
                if not isinstance(t, torch.Tensor):
                    raise ValueError(f"aov_out[{k!r}] must be a torch tensor")
                if t.dtype != dtype:
                    raise ValueError(f"aov_out[{k!r}] has dtype {t.dtype}, the plane needs {dtype}")
                if t.shape != shape:
                    raise ValueError(f"aov_out[{k!r}] has shape {tuple(t.shape)}, the plane needs {shape}")
                if not t.is_contiguous():
                    raise ValueError(f"aov_out[{k!r}] must be contiguous")
                if not t.is_cuda or t.get_device() != self.device:
                    raise ValueError(f"aov_out[{k!r}] is on {t.device}, the scene on cuda:{self.device}")
            plan[k] = (shape, dtype, t)
        return plan

    def _aov_tensors(self, plan, stream, zero=False):
        """The planes of an _aov_plan as tensors: the caller's, or new ones allocated on `stream` (zeros when `zero`: other ranks' pixels
        are not written)."""
        import torch

        if all(t is not None for _, _, t in plan.values()):
            return {k: t for k, (_, _, t) in plan.items()}
        dev = torch.device("cuda", self.device)
        with torch.cuda.stream(stream):
            return {k: t if t is not None else (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=dev)
                    for k, (shape, dtype, t) in plan.items()}

    def render_aov_tensor(self, cam, W: int, H: int, aovs=AOV_NAMES, chw: bool = False, format="rgb", out=None, aov_out=None, stream=None, **kw):
        """render_tensor, and the frame's geometry buffers as torch tensors on cuda:<device>: `aovs` is a subset of AOV_NAMES; depth f32,
        prim_id i32 (the u32 id's bits: 0xffffffff, a miss, reads -1), material_id i32, mask u8 of shape (H, W); normal, position, albedo f32
        of shape (H, W, 3), or (3, H, W) with chw; (2H, 2W) with aa=True (the sub-sample frame).  aov_out: dict name -> caller's tensor for
        some or all of them (validated before any call, ValueError).  Other keywords as render_device.  Returns (tensor, stats, planes)."""
        k = 2 if kw.get("aa") else 1
        nranks = kw.get("nranks", 1)
        plan = self._aov_plan((), k * W, k * H, aovs, chw, aov_out)
        out, fmt, row_bytes, stream = self._frame_tensor(W, H, format, out, stream, nranks)
        planes = self._aov_tensors(plan, stream, zero=nranks > 1)
        st = self.render_aov_device(cam, W, H, out.data_ptr(), {n: t.data_ptr() for n, t in planes.items()}, chw=chw, format=fmt,
                                    row_bytes=row_bytes, stream=stream.cuda_stream, **kw)
        return out, st, planes

    def render_views_aov_tensor(self, cams, W: int, H: int, aovs=AOV_NAMES, chw: bool = False, format="rgb", out=None, aov_out=None, stream=None,
                                **kw):
        """render_views_tensor, and the views' geometry buffers: (B, H, W), (B, H, W, 3) or (B, 3, H, W) tensors, as render_aov_tensor.
        Returns (tensor, stats, planes)."""
        plan = self._aov_plan((len(camera_array(cams)),), W, H, aovs, chw, aov_out)
        a, out, fmt, stream = self._views_tensor(cams, W, H, format, out, stream)
        planes = self._aov_tensors(plan, stream)
        st = self.render_views_aov_device(a, W, H, out.data_ptr(), {n: t.data_ptr() for n, t in planes.items()}, chw=chw, format=fmt,
                                          stream=stream.cuda_stream, **kw)
        return out, st, planes

    def enqueue_render_aov_tensor(self, cam, W: int, H: int, aovs=AOV_NAMES, chw: bool = False, format="rgb", out=None, aov_out=None, stream=None,
                                  aa: bool = False, lights=None, max_level: int = 2, spherical=None, units=None, samples: int = 200, seed: int = 0,
                                  rank: int = 0, nranks: int = 1):
        """render_aov_tensor without waiting for the GPU (cgrt_enqueue_render_aov_device): the whole frame and its planes on `stream`, under
        the rules of enqueue_render_tensor.  Returns (tensor, ticket, planes)."""
        k = 2 if aa else 1
        plan = self._aov_plan((), k * W, k * H, aovs, chw, aov_out)
        out, fmt, row_bytes, stream = self._frame_tensor(W, H, format, out, stream, nranks)
        planes = self._aov_tensors(plan, stream, zero=nranks > 1)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        t = C.c_uint64()
        _check(
            lib().cgrt_enqueue_render_aov_device(
                self._h, C.byref(c), W, H, _ptr(lights), len(lights), q, max_level, 1 if aa else 0, rank, nranks, C.c_void_p(out.data_ptr()),
                fmt, int(row_bytes), C.c_void_p(stream.cuda_stream) if stream.cuda_stream else None, C.byref(t),
                self._aov_arg({n: p.data_ptr() for n, p in planes.items()}, chw),
            )
        )  # fmt: skip
        return out, t.value, planes

    def enqueue_render_views_aov_tensor(self, cams, W: int, H: int, aovs=AOV_NAMES, chw: bool = False, format="rgb", out=None, aov_out=None,
                                        stream=None, lights=None, max_level: int = 2, spherical=None, units=None, samples: int = 200,
                                        seed: int = 0):
        """render_views_aov_tensor without waiting for the GPU (cgrt_enqueue_render_views_aov_device).  Returns (tensor, ticket, planes)."""
        plan = self._aov_plan((len(camera_array(cams)),), W, H, aovs, chw, aov_out)
        a, out, fmt, stream = self._views_tensor(cams, W, H, format, out, stream)
        planes = self._aov_tensors(plan, stream)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        t = C.c_uint64()
        _check(
            lib().cgrt_enqueue_render_views_aov_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, _ptr(lights), len(lights), q, max_level, C.c_void_p(out.data_ptr()), fmt,
                C.c_void_p(stream.cuda_stream) if stream.cuda_stream else None, C.byref(t),
                self._aov_arg({n: p.data_ptr() for n, p in planes.items()}, chw),
            )
        )  # fmt: skip
        return out, t.value, planes

    # ---- ray cameras (include/cgrt.h CgrtRayCamera, cgrt_*_raycam*) ----
    def generate_rays_raycam(self, cam: "RayCamera", W: int, H: int) -> np.ndarray:
        """cgrt_generate_rays_raycam: the W*H rays of a ray camera's frame, row-major, as a RAY_DTYPE array."""
        a = raycam_array(cam)
        if len(a) != 1:
            raise ValueError("generate_rays_raycam takes one camera")
        rays = np.zeros(max(W, 0) * max(H, 0), RAY_DTYPE)
        _check(lib().cgrt_generate_rays_raycam(self._h, _ptr(a), W, H, _ptr(rays)))
        return rays

    def trace_raycams_device(self, cams, W: int, H: int, d_hits_ptr: int, d_normals_ptr: int = 0, stream: int = 0) -> None:
        """cgrt_trace_primary_raycams_device: trace_views_device for B ray cameras (a RayCamera, a sequence of them or raycam_array's
        records); asynchronous on `stream`, the cameras reusable at once."""
        a = raycam_array(cams)
        _check(
            lib().cgrt_trace_primary_raycams_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, C.c_void_p(d_hits_ptr) if d_hits_ptr else None,
                C.c_void_p(d_normals_ptr) if d_normals_ptr else None, C.c_void_p(stream) if stream else None,
            )
        )  # fmt: skip

    def render_raycams_device(self, cams, W: int, H: int, d_out_ptr: int, format="rgb", stream: int = 0, lights=None, max_level: int = 2,
                              spherical=None, units=None, samples: int = 200, seed: int = 0, aov=None, chw: bool = False) -> dict:
        """cgrt_render_raycams_device: render_views_device for B ray cameras; with `aov` (a dict plane name -> device address, as
        render_views_aov_device) the views' geometry buffers are written by the same call.  Raw integers.  Returns stats."""
        a = raycam_array(cams)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        st = RenderStats()
        _check(
            lib().cgrt_render_raycams_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, _ptr(lights), len(lights), q, max_level,
                C.c_void_p(d_out_ptr) if d_out_ptr else None, _frame_format(format), C.c_void_p(stream) if stream else None, C.byref(st),
                self._aov_arg(aov, chw),
            )
        )  # fmt: skip
        return {k: getattr(st, k) for k, _ in st._fields_}

    def render_raycams_light_sets_device(self, cams, W: int, H: int, d_out_ptr: int, light_sets, spherical_sets=None, units=None,
                                         samples: int = 200, seed: int = 0, max_level: int = 2, format="rgb", stream: int = 0) -> dict:
        """cgrt_render_raycams_light_sets_device: render_views_light_sets_device for B ray cameras.  Returns the stats dict."""
        a = raycam_array(cams)
        q, keep = self._light_sets_arg(light_sets, spherical_sets)  # noqa: F841
        s, keep_s = self._light_sets_soft(spherical_sets, units, samples, seed)  # noqa: F841
        st = RenderStats()
        _check(
            lib().cgrt_render_raycams_light_sets_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, C.byref(q), s, max_level, C.c_void_p(d_out_ptr) if d_out_ptr else None,
                _frame_format(format), C.c_void_p(stream) if stream else None, C.byref(st),
            )
        )  # fmt: skip
        return {k: getattr(st, k) for k, _ in st._fields_}

    def render_raycams_tensor(self, cams, W: int, H: int, format="rgb", out=None, stream=None, aovs=None, chw: bool = False, aov_out=None,
                              light_sets=None, **kw):
        """render_views_tensor for B ray cameras: (B, H, W, 3) f32, (B, 3, H, W) f32 or (B, H, W, 4) u8 on cuda:<device>, `out` and
        `stream` as there.  aovs= (a subset of AOV_NAMES; chw, aov_out as render_views_aov_tensor) also returns the geometry buffers:
        (tensor, stats, planes).  light_sets= (a sequence of light arrays; spherical_sets and the other keywords as
        render_views_light_sets_tensor) renders every camera under every set: a (B, S, ...) tensor; not together with aovs.  Otherwise
        the keywords are render_views'.  Returns (tensor, stats dict)."""
        a = raycam_array(cams)
        if light_sets is not None:
            if aovs is not None:
                raise ValueError("geometry buffers do not depend on the lights: render them without light_sets")
            light_sets = list(light_sets)
            self._light_sets_arg(light_sets, kw.get("spherical_sets"))  # (its checks, before any call)
            out, fmt, stream = self._batch_tensor((len(a), len(light_sets)), W, H, format, out, stream)
            st = self.render_raycams_light_sets_device(a, W, H, out.data_ptr(), light_sets, format=fmt, stream=stream.cuda_stream, **kw)
            return out, st
        plan = None if aovs is None else self._aov_plan((len(a),), W, H, aovs, chw, aov_out)
        out, fmt, stream = self._batch_tensor((len(a),), W, H, format, out, stream)
        if plan is None:
            return out, self.render_raycams_device(a, W, H, out.data_ptr(), format=fmt, stream=stream.cuda_stream, **kw)
        planes = self._aov_tensors(plan, stream)
        st = self.render_raycams_device(a, W, H, out.data_ptr(), format=fmt, stream=stream.cuda_stream,
                                        aov={n: t.data_ptr() for n, t in planes.items()}, chw=chw, **kw)
        return out, st, planes

    def enqueue_render_raycams_tensor(self, cams, W: int, H: int, format="rgb", out=None, stream=None, aovs=None, chw: bool = False,
                                      aov_out=None, lights=None, max_level: int = 2, spherical=None, units=None, samples: int = 200,
                                      seed: int = 0):
        """render_raycams_tensor without waiting for the GPU (cgrt_enqueue_render_raycams_device), under the rules of
        enqueue_render_views_tensor.  Returns (tensor, ticket), with aovs= (tensor, ticket, planes)."""
        a = raycam_array(cams)
        plan = None if aovs is None else self._aov_plan((len(a),), W, H, aovs, chw, aov_out)
        out, fmt, stream = self._batch_tensor((len(a),), W, H, format, out, stream)
        planes = None if plan is None else self._aov_tensors(plan, stream)
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        t = C.c_uint64()
        _check(
            lib().cgrt_enqueue_render_raycams_device(
                self._h, _ptr(a) if len(a) else None, len(a), W, H, _ptr(lights), len(lights), q, max_level, C.c_void_p(out.data_ptr()), fmt,
                C.c_void_p(stream.cuda_stream) if stream.cuda_stream else None, C.byref(t),
                None if planes is None else self._aov_arg({n: p.data_ptr() for n, p in planes.items()}, chw),
            )
        )  # fmt: skip
        return (out, t.value) if planes is None else (out, t.value, planes)

    # ---- visibility queries (include/cgrt.h cgrt_occluded*, cgrt_in_shadow*, cgrt_soft_lit*) ----
    def occluded(self, rays) -> np.ndarray:
        """cgrt_occluded: the bool BoundingVolumeHierarchy::intersect returns for each ray (a RAY_DTYPE array or (n, 7) float32), the ray's
        t included (a segment query sets t to its length).  Returns an (n,) bool array."""
        r = _as_ray_array(rays)
        hit = np.zeros(len(r), np.uint8)
        _check(lib().cgrt_occluded(self._h, _ptr(r), len(r), _ptr(hit)))
        return hit.view(np.bool_)

    def occluded_device(self, d_rays_ptr: int, n: int, d_hit_ptr: int, stream: int = 0) -> None:
        """cgrt_occluded_device: n rays (7 floats each) at d_rays_ptr -> n bytes at d_hit_ptr, enqueued on the hipStream_t `stream`."""
        _check(lib().cgrt_occluded_device(self._h, _vp(d_rays_ptr), int(n),
                                          _vp(d_hit_ptr), _vp(stream)))

    def in_shadow(self, points, lights=None) -> np.ndarray:
        """cgrt_in_shadow: pointInShadow (main.cpp:104-135) of every point ((n, 3) float32) and point light ((nlights, 6) {position,
        colour}; default: the scene's).  Returns an (n, nlights) bool array."""
        p = _f32(points, (-1, 3))
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        out = np.zeros((len(p), len(lights)), np.uint8)
        _check(lib().cgrt_in_shadow(self._h, _ptr(p), len(p), _ptr(lights), len(lights), _ptr(out)))
        return out.view(np.bool_)

    def in_shadow_device(self, d_points_ptr: int, n: int, d_out_ptr: int, stream: int = 0, lights=None) -> None:
        """cgrt_in_shadow_device: n points (3 floats each) at d_points_ptr -> n * nlights bytes at d_out_ptr, ordered on `stream`."""
        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        _check(lib().cgrt_in_shadow_device(self._h, _vp(d_points_ptr), int(n), _ptr(lights), len(lights),
                                           _vp(d_out_ptr), _vp(stream)))

    def _soft_query(self, spherical, units, samples: int, seed: int, closest_hit: bool):
        spherical, units = _f32(spherical, (-1, 7)), _f32(units, (-1, 3))
        q = SoftShadows(spherical.ctypes.data, units.ctypes.data, len(spherical), samples, len(units), seed, 1 if closest_hit else 0)
        return q, (spherical, units)

    def soft_lit(self, points, spherical, units, samples: int = 200, seed: int = 0, closest_hit: bool = False) -> np.ndarray:
        """cgrt_soft_lit: of the `samples` soft-shadow rays of each spherical light ((nspherical, 7)), how many reach each point ((n, 3));
        sample smp of point i draws as render_soft's pixel i at level 0.  Returns an (n, nspherical) uint32 array."""
        p = _f32(points, (-1, 3))
        q, keep = self._soft_query(spherical, units, samples, seed, closest_hit)
        lit = np.zeros((len(p), len(keep[0])), np.uint32)
        _check(lib().cgrt_soft_lit(self._h, _ptr(p), len(p), C.byref(q), _ptr(lit)))
        return lit

    def soft_lit_device(self, d_points_ptr: int, n: int, d_lit_ptr: int, spherical, units, samples: int = 200, seed: int = 0,
                        closest_hit: bool = False, stream: int = 0) -> None:
        """cgrt_soft_lit_device: n points at d_points_ptr -> n * nspherical u32 counts at d_lit_ptr, ordered on `stream`."""
        q, keep = self._soft_query(spherical, units, samples, seed, closest_hit)  # noqa: F841
        _check(lib().cgrt_soft_lit_device(self._h, _vp(d_points_ptr), int(n), C.byref(q),
                                          _vp(d_lit_ptr), _vp(stream)))

    def _query_tensor(self, x, width: int, name: str, out, out_shape, out_dtypes):
        """Validates a *_tensor query's input ((..., width) float32, contiguous, on the scene's device) and its optional `out` before any
        call (ValueError otherwise).  Returns n."""
        import torch

        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] != width:
            raise ValueError(f"{name} must be a torch tensor of shape (..., {width})")
        if x.dtype != torch.float32:
            raise ValueError(f"{name} has dtype {x.dtype}, needs torch.float32")
        if x.device.type != "cuda" or x.device.index != self.device:
            raise ValueError(f"{name} is on {x.device}, the scene on cuda:{self.device}")
        if not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if out is not None:
            if not isinstance(out, torch.Tensor) or tuple(out.shape) != out_shape:
                raise ValueError(f"out must be a torch tensor of shape {out_shape}")
            if out.dtype not in out_dtypes:
                raise ValueError(f"out has dtype {out.dtype}, needs one of {out_dtypes}")
            if out.device.type != "cuda" or out.device.index != self.device:
                raise ValueError(f"out is on {out.device}, the scene on cuda:{self.device}")
            if not out.is_contiguous() or (out.element_size() == 4 and out.data_ptr() % 4):
                raise ValueError("out must be contiguous (and 4-byte aligned for counts)")
        return x.numel() // width

    def _torch_stream(self, stream):
        """(the scene's torch device, the torch stream of this call: `stream`, or None for that device's current stream)."""
        import torch

        dev = torch.device("cuda", self.device)
        return dev, (torch.cuda.current_stream(dev) if stream is None else stream)

    def _tensor_call(self, out, shape, dtype, stream, call):
        import torch

        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        if out is None:
            with torch.cuda.stream(stream):  # (allocated on the stream the answers are written on)
                out = torch.empty(shape, dtype=dtype, device=dev)
        if out.numel():  # (an empty tensor has no address to pass: the call would touch nothing anyway)
            call(out, stream.cuda_stream)
        return out

    def occluded_tensor(self, rays, out=None, stream=None):
        """occluded on torch tensors: rays (..., 7) float32 on cuda:<device> -> (...) torch.bool (out may also be torch.uint8),
        enqueued on `stream` (default: torch.cuda.current_stream())."""
        import torch

        shape = tuple(rays.shape[:-1]) if isinstance(rays, torch.Tensor) else ()
        n = self._query_tensor(rays, 7, "rays", out, shape, (torch.bool, torch.uint8))
        return self._tensor_call(out, shape, torch.bool, stream, lambda o, s: self.occluded_device(rays.data_ptr(), n, o.data_ptr(), stream=s))

    def in_shadow_tensor(self, points, lights=None, out=None, stream=None):
        """in_shadow on torch tensors: points (..., 3) float32 on cuda:<device> -> (..., nlights) torch.bool (out may also be
        torch.uint8), ordered on `stream` (default: torch.cuda.current_stream()); lights as in_shadow (a host array)."""
        import torch

        lights = _f32(self.sd.point_lights if lights is None else lights, (-1, 6))
        shape = (tuple(points.shape[:-1]) if isinstance(points, torch.Tensor) else ()) + (len(lights),)
        n = self._query_tensor(points, 3, "points", out, shape, (torch.bool, torch.uint8))
        return self._tensor_call(out, shape, torch.bool, stream,
                                 lambda o, s: self.in_shadow_device(points.data_ptr(), n, o.data_ptr(), stream=s, lights=lights))

    def soft_lit_tensor(self, points, spherical, units, samples: int = 200, seed: int = 0, closest_hit: bool = False, out=None, stream=None):
        """soft_lit on torch tensors: points (..., 3) float32 on cuda:<device> -> (..., nspherical) torch.int32 counts (at most 2^24, the
        sample cap), ordered on `stream` (default: torch.cuda.current_stream())."""
        import torch

        spherical = _f32(spherical, (-1, 7))
        shape = (tuple(points.shape[:-1]) if isinstance(points, torch.Tensor) else ()) + (len(spherical),)
        n = self._query_tensor(points, 3, "points", out, shape, (torch.int32,))
        return self._tensor_call(out, shape, torch.int32, stream,
                                 lambda o, s: self.soft_lit_device(points.data_ptr(), n, o.data_ptr(), spherical, units, samples=samples,
                                                                   seed=seed, closest_hit=closest_hit, stream=s))

    # ---- surface attributes (include/cgrt.h cgrt_hit_barycentrics*, cgrt_interpolate_hits*, cgrt_surface_*_device) ----
    @staticmethod
    def _as_hit_array(hits, n: int) -> np.ndarray:
        h = np.ascontiguousarray(hits)
        if h.dtype != HIT_DTYPE or h.ndim != 1 or len(h) != n:
            raise ValueError(f"hits must be a HIT_DTYPE array with one entry per ray ({n})")
        return h

    def hit_barycentrics(self, rays, hits) -> np.ndarray:
        """cgrt_hit_barycentrics: where inside its triangle each ray hit.  rays (RAY_DTYPE or (n, 7) float32) and hits (HIT_DTYPE) are what
        intersect took and returned.  Returns (n, 3) float32 {alpha, beta, gamma}, the weights of tri[prim_id][0..2] -- the area ratios
        of ray_tracing.cpp:94-96, not renormalised; zeros for a miss, a sphere hit or an out-of-range prim_id."""
        r = _as_ray_array(rays)
        h = self._as_hit_array(hits, len(r))
        bary = np.zeros((len(r), 3), np.float32)
        _check(lib().cgrt_hit_barycentrics(self._h, _ptr(r), _ptr(h), len(r), _ptr(bary)))
        return bary

    def interpolate_hits(self, rays, hits, attr) -> np.ndarray:
        """cgrt_interpolate_hits: a per-vertex table attr ((nverts, C) float32, row v = vertex v of pos_nrm, C in 1..256) carried to every
        hit: (alpha * attr[i0] + beta * attr[i1]) + gamma * attr[i2] per channel.  Returns (n, C) float32, zeros where hit_barycentrics
        gives zeros."""
        r = _as_ray_array(rays)
        h = self._as_hit_array(hits, len(r))
        a = self._attr_array(attr)
        out = np.zeros((len(r), a.shape[1]), np.float32)
        _check(lib().cgrt_interpolate_hits(self._h, _ptr(r), _ptr(h), len(r), _ptr(a), a.shape[1], _ptr(out)))
        return out

    def _attr_array(self, attr) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(attr, np.float32))
        nverts = len(_f32(self.sd.pos_nrm, (-1, 6)))
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        if a.ndim != 2 or a.shape[0] != nverts:
            raise ValueError(f"attr must have one row per vertex: ({nverts}, C), not {a.shape}")
        return a

    def hit_barycentrics_device(self, d_rays_ptr: int, d_hits_ptr: int, n: int, d_bary_ptr: int, stream: int = 0) -> None:
        """cgrt_hit_barycentrics_device: n rays (28 bytes each) and hits (16 bytes each) -> n x 3 floats at d_bary_ptr, enqueued on the
        hipStream_t `stream`.  Raw integers."""
        _check(lib().cgrt_hit_barycentrics_device(self._h, _vp(d_rays_ptr), _vp(d_hits_ptr), int(n), _vp(d_bary_ptr), _vp(stream)))

    def interpolate_hits_device(self, d_rays_ptr: int, d_hits_ptr: int, n: int, d_attr_ptr: int, channels: int, d_out_ptr: int,
                                stream: int = 0) -> None:
        """cgrt_interpolate_hits_device: d_attr_ptr is an (nverts, channels) float32 table in device memory; n x channels floats go to
        d_out_ptr, enqueued on `stream`.  Raw integers."""
        _check(lib().cgrt_interpolate_hits_device(self._h, _vp(d_rays_ptr), _vp(d_hits_ptr), int(n), _vp(d_attr_ptr), int(channels),
                                                  _vp(d_out_ptr), _vp(stream)))

    def surface_views_device(self, cams, W: int, H: int, d_depth_ptr: int, d_prim_id_ptr: int, d_bary_ptr: int = 0, d_attr_ptr: int = 0,
                             channels: int = 0, d_out_ptr: int = 0, chw: bool = False, stream: int = 0, raycams: bool = False) -> None:
        """cgrt_surface_views_device (raycams: cgrt_surface_raycams_device): the barycentrics (d_bary_ptr) and / or an interpolated
        attribute (d_attr_ptr, channels, d_out_ptr) of every pixel of B frames from their (B, H, W) depth and prim_id planes; the primary
        rays are regenerated from the cameras.  Raw integers; enqueued on `stream`."""
        a = raycam_array(cams) if raycams else camera_array(cams)
        f = lib().cgrt_surface_raycams_device if raycams else lib().cgrt_surface_views_device
        _check(f(self._h, _ptr(a) if len(a) else None, len(a), W, H, _vp(d_depth_ptr), _vp(d_prim_id_ptr), _vp(d_attr_ptr), int(channels),
                 _vp(d_bary_ptr), _vp(d_out_ptr), 1 if chw else 0, _vp(stream)))

    def _device_tensor(self, t, name: str, dtypes, shape=None):
        """A *_tensor argument: a contiguous torch tensor of one of `dtypes` (and of `shape`) on the scene's device (ValueError)."""
        import torch

        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if t.dtype not in dtypes:
            raise ValueError(f"{name} has dtype {t.dtype}, needs one of {dtypes}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, needs {tuple(shape)}")
        if t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError(f"{name} is on {t.device}, the scene on cuda:{self.device}")
        if not t.is_contiguous() or t.data_ptr() % 4:
            raise ValueError(f"{name} must be contiguous and 4-byte aligned")
        return t

    def _attr_tensor(self, attr):
        import torch

        nverts = len(_f32(self.sd.pos_nrm, (-1, 6)))
        if isinstance(attr, torch.Tensor) and attr.dim() == 2 and attr.shape[0] == nverts and 1 <= attr.shape[1] <= 256:
            return self._device_tensor(attr, "attr", (torch.float32,))
        raise ValueError(f"attr must be a torch tensor of shape ({nverts}, C), C in 1..256")

    def _hits_tensor(self, rays, hits):
        """The checks of a ray list's tensors: rays (..., 7) float32; hits in HIT_DTYPE layout, 16 bytes per ray -- (..., 4) of a 4-byte
        dtype (as intersect_device's hits viewed as int32) or (..., 16) uint8.  Returns (lead shape, n)."""
        import torch

        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        if not isinstance(rays, torch.Tensor) or rays.dim() < 1 or rays.shape[-1] != 7:
            raise ValueError("rays must be a torch tensor of shape (..., 7)")
        self._device_tensor(rays, "rays", (torch.float32,))
        lead = tuple(rays.shape[:-1])
        if not isinstance(hits, torch.Tensor) or hits.dim() < 1 or hits.shape[-1] * hits.element_size() != HIT_DTYPE.itemsize or \
                tuple(hits.shape[:-1]) != lead:
            raise ValueError(f"hits must be a torch tensor of shape {lead + (4,)} (a 4-byte dtype) or {lead + (16,)} (uint8): HIT_DTYPE records")
        self._device_tensor(hits, "hits", (torch.int32, torch.float32, torch.uint8) + ((torch.uint32,) if hasattr(torch, "uint32") else ()))
        return lead, rays.numel() // 7

    def hit_barycentrics_tensor(self, rays, hits, out=None, stream=None):
        """hit_barycentrics on torch tensors of cuda:<device>: rays (..., 7) float32, hits (..., 4) int32 / float32 (or (..., 16) uint8)
        holding HIT_DTYPE records -> (..., 3) float32, into `out` or a new tensor, enqueued on `stream` (default:
        torch.cuda.current_stream())."""
        import torch

        lead, n = self._hits_tensor(rays, hits)
        if out is not None:
            self._device_tensor(out, "out", (torch.float32,), lead + (3,))
        return self._tensor_call(out, lead + (3,), torch.float32, stream,
                                 lambda o, s: self.hit_barycentrics_device(rays.data_ptr(), hits.data_ptr(), n, o.data_ptr(), stream=s))

    def interpolate_hits_tensor(self, rays, hits, attr, out=None, stream=None, reproducible: bool = False):
        """interpolate_hits on torch tensors: attr is an (nverts, C) float32 tensor on cuda:<device> (any per-vertex table: colours,
        texture coordinates, features; it may be a contiguous view into a larger allocation) -> (..., C) float32.  reproducible: when
        attr requires grad, the recorded backward is the bitwise-reproducible entry (it runs under
        torch.use_deterministic_algorithms(True)); the forward is the same either way."""
        import torch

        lead, n = self._hits_tensor(rays, hits)
        attr = self._attr_tensor(attr)
        ch = attr.shape[1]
        if attr.requires_grad and torch.is_grad_enabled():  # recorded: the output carries a grad_fn (interpolate_hits_grad_tensor)
            if out is not None:
                raise ValueError("out= cannot be combined with an attr that requires grad")
            return _surface_function().apply(
                attr, lambda a: self.interpolate_hits_tensor(rays, hits, a, stream=stream),
                lambda g: self.interpolate_hits_grad_tensor(rays, hits, g, reproducible=reproducible), None, bool(reproducible))
        if out is not None:
            self._device_tensor(out, "out", (torch.float32,), lead + (ch,))
        return self._tensor_call(out, lead + (ch,), torch.float32, stream,
                                 lambda o, s: self.interpolate_hits_device(rays.data_ptr(), hits.data_ptr(), n, attr.data_ptr(), ch,
                                                                           o.data_ptr(), stream=s))

    # ---- surface attributes: gradients back to the table (include/cgrt.h cgrt_interpolate_hits_grad*, cgrt_surface_*_grad_device;
    # DESIGN.md section 5.23) ----
    def surface_grad_repro_workspace(self, channels: int) -> int:
        """cgrt_surface_grad_repro_workspace: the bytes of device memory a reproducible gradient call with `channels` channels needs."""
        b = C.c_uint64(0)
        _check(lib().cgrt_surface_grad_repro_workspace(self._h, int(channels), C.byref(b)))
        return int(b.value)

    def interpolate_hits_grad(self, rays, hits, grad_out, grad_attr=None, reproducible: bool = False) -> np.ndarray:
        """cgrt_interpolate_hits_grad, the adjoint of interpolate_hits with respect to attr: grad_out ((n, C) float32) is the gradient
        with respect to interpolate_hits' result; alpha / beta / gamma times each valid item's row is ADDED into rows tri[prim_id][0..2]
        of grad_attr -- a C-contiguous (nverts, C) float32 array that is accumulated into in place, or None for a new zero array.
        Returns grad_attr.  The order of the additions into one element is unspecified (last bits may differ from run to run), unless
        reproducible: then cgrt_interpolate_hits_grad_repro, whose result is defined to the last bit (include/cgrt.h)."""
        r = _as_ray_array(rays)
        h = self._as_hit_array(hits, len(r))
        g = np.ascontiguousarray(np.asarray(grad_out, np.float32))
        if g.ndim == 1:
            g = g.reshape(-1, 1)
        if g.ndim != 2 or g.shape[0] != len(r):
            raise ValueError(f"grad_out must have one row per ray: ({len(r)}, C), not {g.shape}")
        nverts = len(_f32(self.sd.pos_nrm, (-1, 6)))
        if grad_attr is None:
            grad_attr = np.zeros((nverts, g.shape[1]), np.float32)
        elif not (isinstance(grad_attr, np.ndarray) and grad_attr.dtype == np.float32 and grad_attr.flags.c_contiguous
                  and grad_attr.flags.writeable and grad_attr.shape == (nverts, g.shape[1])):
            raise ValueError(f"grad_attr must be a writeable C-contiguous float32 array of shape ({nverts}, {g.shape[1]})")
        f = lib().cgrt_interpolate_hits_grad_repro if reproducible else lib().cgrt_interpolate_hits_grad
        _check(f(self._h, _ptr(r), _ptr(h), len(r), _ptr(g), g.shape[1], _ptr(grad_attr)))
        return grad_attr

    def interpolate_hits_grad_device(self, d_rays_ptr: int, d_hits_ptr: int, n: int, d_grad_out_ptr: int, channels: int,
                                     d_grad_attr_ptr: int, stream: int = 0, reproducible: bool = False, d_workspace_ptr: int = 0,
                                     workspace_bytes: int = 0) -> None:
        """cgrt_interpolate_hits_grad_device: n x channels floats at d_grad_out_ptr are added, weighted, into the (nverts, channels)
        float32 table at d_grad_attr_ptr; enqueued on `stream`.  Raw integers.  reproducible: cgrt_interpolate_hits_grad_repro_device
        with the caller's workspace (surface_grad_repro_workspace(channels) bytes of device memory, 8-byte aligned, this call's alone)."""
        if reproducible:
            _check(lib().cgrt_interpolate_hits_grad_repro_device(self._h, _vp(d_rays_ptr), _vp(d_hits_ptr), int(n), _vp(d_grad_out_ptr),
                                                                 int(channels), _vp(d_grad_attr_ptr), _vp(d_workspace_ptr),
                                                                 int(workspace_bytes), _vp(stream)))
            return
        _check(lib().cgrt_interpolate_hits_grad_device(self._h, _vp(d_rays_ptr), _vp(d_hits_ptr), int(n), _vp(d_grad_out_ptr), int(channels),
                                                       _vp(d_grad_attr_ptr), _vp(stream)))

    def surface_views_grad_device(self, cams, W: int, H: int, d_depth_ptr: int, d_prim_id_ptr: int, d_grad_out_ptr: int, channels: int,
                                  d_grad_attr_ptr: int, chw: bool = False, stream: int = 0, raycams: bool = False,
                                  reproducible: bool = False, d_workspace_ptr: int = 0, workspace_bytes: int = 0) -> None:
        """cgrt_surface_views_grad_device (raycams: cgrt_surface_raycams_grad_device): the gradient (B, H, W, channels) -- (B, channels,
        H, W) with chw -- of B frames' interpolated attribute, added into the table at d_grad_attr_ptr.  Raw integers; enqueued.
        reproducible: the *_grad_repro_device twin with the caller's workspace, as interpolate_hits_grad_device takes it."""
        a = raycam_array(cams) if raycams else camera_array(cams)
        if reproducible:
            f = lib().cgrt_surface_raycams_grad_repro_device if raycams else lib().cgrt_surface_views_grad_repro_device
            _check(f(self._h, _ptr(a) if len(a) else None, len(a), W, H, _vp(d_depth_ptr), _vp(d_prim_id_ptr), _vp(d_grad_out_ptr),
                     int(channels), 1 if chw else 0, _vp(d_grad_attr_ptr), _vp(d_workspace_ptr), int(workspace_bytes), _vp(stream)))
            return
        f = lib().cgrt_surface_raycams_grad_device if raycams else lib().cgrt_surface_views_grad_device
        _check(f(self._h, _ptr(a) if len(a) else None, len(a), W, H, _vp(d_depth_ptr), _vp(d_prim_id_ptr), _vp(d_grad_out_ptr), int(channels),
                 1 if chw else 0, _vp(d_grad_attr_ptr), _vp(stream)))

    def _grad_attr_tensor(self, grad_attr, channels: int, stream):
        """The table a *_grad_tensor call accumulates into and the stream it runs on: the caller's (nverts, C) tensor, or new zeros."""
        import torch

        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        nverts = len(_f32(self.sd.pos_nrm, (-1, 6)))
        if grad_attr is None:
            with torch.cuda.stream(stream):
                grad_attr = torch.zeros((nverts, channels), dtype=torch.float32, device=dev)
        else:
            self._device_tensor(grad_attr, "grad_attr", (torch.float32,), (nverts, channels))
        return grad_attr, stream

    @staticmethod
    def _repro_workspace_tensor(nbytes, stream):
        """(workspace, keywords) of a reproducible *_grad_device call that needs `nbytes` (its family's *_grad_repro_workspace): the
        workspace is a torch.uint8 tensor allocated on the call's stream, which the caller holds until the call has enqueued its passes
        -- from then on the caching allocator hands the block only to work that the same stream runs later.  nbytes None, the float
        form: (None, {})."""
        if nbytes is None:
            return None, {}
        import torch

        with torch.cuda.stream(stream):
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=stream.device)
        return ws, {"reproducible": True, "d_workspace_ptr": ws.data_ptr(), "workspace_bytes": nbytes}

    def interpolate_hits_grad_tensor(self, rays, hits, grad_out, grad_attr=None, stream=None, reproducible: bool = False):
        """interpolate_hits_grad on torch tensors: rays, hits as interpolate_hits_tensor took them, grad_out (..., C) float32; added into
        grad_attr ((nverts, C) float32 on the device, or None for a new zero tensor), which is returned.  Enqueued on `stream` (default:
        torch.cuda.current_stream()).  interpolate_hits_tensor calls this in its backward when attr requires grad.  reproducible: the
        bitwise-reproducible entry, its workspace allocated here on the call's stream."""
        import torch

        lead, n = self._hits_tensor(rays, hits)
        if not isinstance(grad_out, torch.Tensor) or grad_out.dim() != len(lead) + 1 or tuple(grad_out.shape[:-1]) != lead or \
                not 1 <= grad_out.shape[-1] <= 256:
            raise ValueError(f"grad_out must be a torch tensor of shape {lead + ('C',)}, C in 1..256")
        self._device_tensor(grad_out, "grad_out", (torch.float32,))
        ch = grad_out.shape[-1]
        grad_attr, stream = self._grad_attr_tensor(grad_attr, ch, stream)
        if n:
            ws, kw = self._repro_workspace_tensor(self.surface_grad_repro_workspace(ch) if reproducible else None, stream)
            self.interpolate_hits_grad_device(rays.data_ptr(), hits.data_ptr(), n, grad_out.data_ptr(), ch, grad_attr.data_ptr(),
                                              stream=stream.cuda_stream, **kw)
            del ws  # (held until here: the passes are enqueued)
        return grad_attr

    # ---- closest-point queries (include/cgrt.h cgrt_closest_points*) ----
    def _closest_host(self, f, points, max_dist2: float) -> np.ndarray:
        p = _f32(points, (-1, 3))
        out = np.zeros(len(p), CLOSEST_DTYPE)
        _check(f(self._h, _ptr(p), len(p), float(max_dist2), _ptr(out)))
        return out

    def closest_points(self, points, max_dist2: float = float("inf")) -> np.ndarray:
        """cgrt_closest_points: the nearest point of the scene's triangles for every query point ((n, 3) float32) within the squared
        radius max_dist2 (inf: unbounded).  Returns a CLOSEST_DTYPE array {point, dist2, prim_id, bary = {u, v, w}}; a query that finds
        nothing (or is not finite) gets {0, +inf, NO_PRIM, 0}.  Equal distances go to the smaller prim_id.  Spheres are ignored."""
        return self._closest_host(lib().cgrt_closest_points, points, max_dist2)

    def closest_points_brute(self, points, max_dist2: float = float("inf")) -> np.ndarray:
        """cgrt_closest_points_brute: closest_points by testing every triangle in turn (validation; the same bytes)."""
        return self._closest_host(lib().cgrt_closest_points_brute, points, max_dist2)

    def closest_points_device(self, d_points_ptr: int, n: int, d_out_ptr: int, max_dist2: float = float("inf"), stream: int = 0) -> None:
        """cgrt_closest_points_device: n points (3 floats each) at d_points_ptr -> n CLOSEST_DTYPE records (32 bytes each) at d_out_ptr,
        enqueued on the hipStream_t `stream`.  Raw integers."""
        _check(lib().cgrt_closest_points_device(self._h, _vp(d_points_ptr), int(n), float(max_dist2), _vp(d_out_ptr), _vp(stream)))

    def closest_points_tensor(self, points, max_dist2: float = float("inf"), out=None, stream=None):
        """closest_points on torch tensors: points (n, 3) float32 on cuda:<device> -> an (n, 8) float32 tensor of CLOSEST_DTYPE records
        (`out`, or a new one), enqueued on `stream` (default: torch.cuda.current_stream()).  Returns a dict of views of it: 'point'
        (n, 3), 'dist2' (n,), 'prim_id' (n,) int32 (-1 = NO_PRIM), 'bary' (n, 3), and 'out' itself."""
        import torch

        n = self._points_tensor(points)
        if out is not None:
            self._device_tensor(out, "out", (torch.float32,), (n, 8))
        o = self._tensor_call(out, (n, 8), torch.float32, stream,
                              lambda t, s: self.closest_points_device(points.data_ptr(), n, t.data_ptr(), max_dist2=max_dist2, stream=s))
        return {"point": o[:, 0:3], "dist2": o[:, 3], "prim_id": o.view(torch.int32)[:, 4], "bary": o[:, 5:8], "out": o}

    def debug_closest_work(self, points, max_dist2: float = float("inf")):
        """cgrt_debug_closest_work: (node steps, triangles evaluated) of closest_points' search, summed over the queries (a separate
        counting launch)."""
        p = _f32(points, (-1, 3))
        w = np.zeros(2, np.uint64)
        _check(lib().cgrt_debug_closest_work(self._h, _ptr(p), len(p), float(max_dist2), _ptr(w)))
        return int(w[0]), int(w[1])

    # ---- crossing queries (include/cgrt.h cgrt_count_crossings*, cgrt_list_crossings*) ----
    # The slot lists of crossings and neighbours are one layer.  `kind` ("crossings" / "neighbors") names the C entries (cgrt_count_<kind>,
    # cgrt_list_<kind>, cgrt_list_<kind>_brute) and the record dtype (_SLOT_RECORDS); `lead` is what those entries take between the scene and
    # the slot arguments -- (rays, n) or (points, n, radius2, max_dist2) -- as ctypes arguments of arrays the caller keeps alive.
    def _slots_count(self, kind, lead) -> np.ndarray:
        counts = np.zeros(lead[1], np.uint32)
        _check(getattr(lib(), f"cgrt_count_{kind}")(self._h, *lead, _ptr(counts)))
        return counts

    def _slots_host(self, kind, lead, offsets, k: int, want_counts: bool = True, brute: bool = False):
        """One cgrt_list_<kind> call into slots from `offsets` or of k records each: (records, counts or None)."""
        m = int(offsets[-1]) if offsets is not None else lead[1] * k
        out = np.zeros(m, _SLOT_RECORDS[kind])
        counts = np.zeros(lead[1], np.uint32) if want_counts else None
        f = getattr(lib(), f"cgrt_list_{kind}_brute" if brute else f"cgrt_list_{kind}")
        _check(f(self._h, *lead, _ptr(offsets), int(k), _ptr(out), m, _ptr(counts)))
        return out, counts

    def _slots_full(self, kind, lead, counts, brute: bool = False):
        """The full lists from the full counts: (offsets (n + 1,) int64, records)."""
        off = np.zeros(lead[1] + 1, np.uint64)
        np.cumsum(counts, dtype=np.uint64, out=off[1:])
        out, _ = self._slots_host(kind, lead, off, 0, want_counts=False, brute=brute)
        return off.astype(np.int64), out

    def _slots_list(self, kind, lead, offsets, want_counts: bool):
        if offsets is not None:
            return self._slots_host(kind, lead, np.ascontiguousarray(offsets, np.uint64), 0, want_counts)
        return self._slots_full(kind, lead, self._slots_count(kind, lead))

    def _slots_brute(self, kind, lead, offsets, k: int):
        if offsets is None and not k:
            _, c = self._slots_host(kind, lead, None, 1, brute=True)  # k = 1 only to obtain the counts
            return self._slots_full(kind, lead, c, brute=True)
        off = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
        out, counts = self._slots_host(kind, lead, off, k, brute=True)
        return (out.reshape(lead[1], k) if off is None else out), counts

    def _slots_first(self, kind, lead, k: int, want_counts: bool):
        if k < 1:
            raise ValueError("k must be at least 1")
        out, counts = self._slots_host(kind, lead, None, k, want_counts)
        return out.reshape(lead[1], k), counts

    def _slots_full_tensor(self, n: int, stream, count, list_device):
        """The full lists on torch tensors: count(stream) gives the (n,) int32 counts, list_device(d_out_ptr, capacity, d_offsets_ptr, stream
        handle) lists into the slots of their prefix sums.  (offsets (n + 1,) int64, records (m, 2) float32)."""
        import torch

        dev, stream = self._torch_stream(stream)
        counts = count(stream)
        with torch.cuda.stream(stream):
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
            m = int(offsets[-1].item())
            records = torch.empty((m, 2), dtype=torch.float32, device=dev)
        if n and m:
            list_device(records.data_ptr(), m, offsets.data_ptr(), stream.cuda_stream)
        return offsets, records

    def _slots_first_tensor(self, n: int, k: int, want_counts: bool, out, stream, list_device):
        """k records per query on torch tensors: list_device(d_out_ptr, d_counts_ptr, stream handle) fills the (n, k, 2) float32 records
        (`out`, or a new tensor) and, if wanted, the (n,) int32 counts.  (records, counts or None)."""
        import torch

        if k < 1:
            raise ValueError("k must be at least 1")
        if out is not None:
            self._device_tensor(out, "out", (torch.float32,), (n, k, 2))
        dev, stream = self._torch_stream(stream)
        counts = None
        if want_counts:
            with torch.cuda.stream(stream):
                counts = torch.empty((n,), dtype=torch.int32, device=dev)
        cp = counts.data_ptr() if want_counts and n else 0
        return self._tensor_call(out, (n, k, 2), torch.float32, stream, lambda o, s: list_device(o.data_ptr(), cp, s)), counts

    def count_crossings(self, rays) -> np.ndarray:
        """cgrt_count_crossings: for every ray (RAY_DTYPE or (n, 7) float32, taken as given: t bounds it) the number of triangles it
        passes through -- the triangles the reference's intersectRayWithTriangle accepts on a fresh copy of the ray.  (n,) uint32."""
        r = _as_ray_array(rays)
        return self._slots_count("crossings", (_ptr(r), len(r)))

    def list_crossings(self, rays, offsets=None, want_counts: bool = True):
        """Every crossing of every ray, in order (by t, equal t by prim_id): cgrt_count_crossings, the exclusive prefix sums, then
        cgrt_list_crossings.  Returns (offsets, records): offsets (n + 1,) int64, ray i's crossings are records[offsets[i]:offsets[i + 1]]
        (CROSSING_DTYPE {t, prim_id}).
        With offsets ((n + 1,) slot boundaries chosen by the caller) one cgrt_list_crossings call: ray i receives its first crossings in
        order in records [offsets[i], offsets[i + 1]), {+inf, NO_PRIM} in what remains.  Returns (records (offsets[-1],), counts: the full
        numbers of crossings -- or None with want_counts=False, which lets the search of a ray stop at the largest t its full slot keeps)."""
        r = _as_ray_array(rays)
        return self._slots_list("crossings", (_ptr(r), len(r)), offsets, want_counts)

    def list_crossings_brute(self, rays, offsets=None, k: int = 0):
        """cgrt_list_crossings_brute: the list by testing every triangle in turn (validation; the same bytes).  With neither offsets nor
        k the full list, as list_crossings returns it: (offsets, records); with offsets ((n + 1,) slot boundaries) or k (k records per
        ray): (records, counts)."""
        r = _as_ray_array(rays)
        return self._slots_brute("crossings", (_ptr(r), len(r)), offsets, k)

    def first_crossings(self, rays, k: int, want_counts: bool = True):
        """The first k crossings of every ray: ((n, k) CROSSING_DTYPE records, unused entries {+inf, NO_PRIM}; (n,) uint32 counts -- the
        full numbers of crossings; None with want_counts=False, as list_crossings with offsets)."""
        r = _as_ray_array(rays)
        return self._slots_first("crossings", (_ptr(r), len(r)), k, want_counts)

    def debug_crossing_work(self, rays):
        """cgrt_debug_crossing_work: (node steps, triangles evaluated) of count_crossings' search, summed over the rays (a separate
        counting launch)."""
        r = _as_ray_array(rays)
        w = np.zeros(2, np.uint64)
        _check(lib().cgrt_debug_crossing_work(self._h, _ptr(r), len(r), _ptr(w)))
        return int(w[0]), int(w[1])

    def count_crossings_device(self, d_rays_ptr: int, n: int, d_counts_ptr: int, stream: int = 0) -> None:
        """cgrt_count_crossings_device: n rays (28 bytes each) at d_rays_ptr -> n uint32 counts at d_counts_ptr, enqueued on the
        hipStream_t `stream`.  Raw integers."""
        _check(lib().cgrt_count_crossings_device(self._h, _vp(d_rays_ptr), int(n), _vp(d_counts_ptr), _vp(stream)))

    def list_crossings_device(self, d_rays_ptr: int, n: int, d_out_ptr: int, capacity: int, d_offsets_ptr: int = 0, k: int = 0,
                              d_counts_ptr: int = 0, stream: int = 0) -> None:
        """cgrt_list_crossings_device: slots from the n + 1 uint64 offsets at d_offsets_ptr, or of k records each; `capacity` records of
        8 bytes at d_out_ptr, nothing beyond them is written whatever the offsets hold; d_counts_ptr (optional) receives the full counts.
        Enqueued on `stream`.  Raw integers."""
        _check(lib().cgrt_list_crossings_device(self._h, _vp(d_rays_ptr), int(n), _vp(d_offsets_ptr), int(k), _vp(d_out_ptr), int(capacity),
                                                _vp(d_counts_ptr), _vp(stream)))

    def first_crossings_device(self, d_rays_ptr: int, n: int, k: int, d_out_ptr: int, d_counts_ptr: int = 0, stream: int = 0) -> None:
        """list_crossings_device with k records per ray: n * k records at d_out_ptr."""
        self.list_crossings_device(d_rays_ptr, n, d_out_ptr, int(n) * int(k), k=k, d_counts_ptr=d_counts_ptr, stream=stream)

    def _crossing_rays_tensor(self, rays):
        import torch

        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 7:
            raise ValueError("rays must be a torch tensor of shape (n, 7)")
        self._device_tensor(rays, "rays", (torch.float32,))
        return rays.shape[0]

    def _points_tensor(self, points, shape_first: bool = False):
        """The checks of a point list's tensor: (n, 3) float32, contiguous, on the scene's device (ValueError).  Returns n.  The host-only
        scene is reported first, or with shape_first (sdf_tensor, winding_numbers_tensor) behind the shape."""
        import torch

        if self.device < 0 and not shape_first:
            raise ValueError("the scene has no device (created host-only)")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must be a torch tensor of shape (n, 3)")
        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        self._device_tensor(points, "points", (torch.float32,))
        return points.shape[0]

    def count_crossings_tensor(self, rays, out=None, stream=None):
        """count_crossings on torch tensors: rays (n, 7) float32 on cuda:<device> -> (n,) torch.int32, into `out` or a new tensor,
        enqueued on `stream` (default: torch.cuda.current_stream())."""
        import torch

        n = self._crossing_rays_tensor(rays)
        if out is not None:
            self._device_tensor(out, "out", (torch.int32,), (n,))
        return self._tensor_call(out, (n,), torch.int32, stream, lambda o, s: self.count_crossings_device(rays.data_ptr(), n, o.data_ptr(), stream=s))

    def list_crossings_tensor(self, rays, stream=None):
        """list_crossings on torch tensors: rays (n, 7) float32 on cuda:<device> -> (offsets (n + 1,) torch.int64, records (m, 2) float32
        with the prim_id BITS in column 1: records.view(torch.int32)[:, 1]).  Count, a torch cumsum and the list are enqueued on `stream`;
        the total m is read back in between (one synchronisation of that stream)."""
        n = self._crossing_rays_tensor(rays)
        return self._slots_full_tensor(n, stream, lambda s: self.count_crossings_tensor(rays, stream=s),
                                       lambda o, m, off, s: self.list_crossings_device(rays.data_ptr(), n, o, m, d_offsets_ptr=off, stream=s))

    def first_crossings_tensor(self, rays, k: int, out=None, stream=None):
        """first_crossings on torch tensors: rays (n, 7) float32 on cuda:<device> -> (records (n, k, 2) float32 -- `out`, or a new tensor;
        the prim_id bits in [..., 1], unused entries {+inf, NO_PRIM} --, counts (n,) torch.int32: the full numbers of crossings)."""
        n = self._crossing_rays_tensor(rays)
        return self._slots_first_tensor(n, k, True, out, stream,
                                        lambda o, c, s: self.first_crossings_device(rays.data_ptr(), n, k, o, d_counts_ptr=c, stream=s))

    # ---- neighbour queries (include/cgrt.h cgrt_count_neighbors*, cgrt_list_neighbors*) ----
    @staticmethod
    def _neighbor_points(points, radius2):
        p = _f32(points, (-1, 3))
        r = None if radius2 is None else _f32(radius2, (-1,))
        if r is not None and len(r) != len(p):
            raise ValueError("radius2 must hold one squared radius per point")
        return p, r

    def count_neighbors(self, points, radius2=None, max_dist2: float = float("inf")) -> np.ndarray:
        """cgrt_count_neighbors: for every query point ((n, 3) float32) the number of triangles whose closest_points dist2 is <= its
        squared radius -- radius2[i] ((n,) float32; NaN or negative: no neighbours), or max_dist2 for every query.  (n,) uint32."""
        p, r = self._neighbor_points(points, radius2)
        return self._slots_count("neighbors", (_ptr(p), len(p), _ptr(r), float(max_dist2)))

    def list_neighbors(self, points, radius2=None, max_dist2: float = float("inf"), offsets=None, want_counts: bool = True):
        """Every neighbour of every query point, in order (by dist2, equal dist2 by prim_id): cgrt_count_neighbors, the exclusive prefix
        sums, then cgrt_list_neighbors.  Returns (offsets, records): offsets (n + 1,) int64, query i's neighbours are
        records[offsets[i]:offsets[i + 1]] (NEIGHBOR_DTYPE {dist2, prim_id}).
        With offsets ((n + 1,) slot boundaries chosen by the caller) one cgrt_list_neighbors call: query i receives its first neighbours
        in order in records [offsets[i], offsets[i + 1]), {+inf, NO_PRIM} in what remains.  Returns (records (offsets[-1],), counts: the
        full numbers of neighbours -- or None with want_counts=False, which lets a query's search shrink to the largest dist2 its full
        slot keeps)."""
        p, r = self._neighbor_points(points, radius2)
        return self._slots_list("neighbors", (_ptr(p), len(p), _ptr(r), float(max_dist2)), offsets, want_counts)

    def list_neighbors_brute(self, points, radius2=None, max_dist2: float = float("inf"), offsets=None, k: int = 0):
        """cgrt_list_neighbors_brute: the list by testing every triangle in turn (validation; the same bytes).  With neither offsets nor
        k the full list, as list_neighbors returns it: (offsets, records); with offsets ((n + 1,) slot boundaries) or k (k records per
        query): (records, counts)."""
        p, r = self._neighbor_points(points, radius2)
        return self._slots_brute("neighbors", (_ptr(p), len(p), _ptr(r), float(max_dist2)), offsets, k)

    def nearest_triangles(self, points, k: int, radius2=None, max_dist2: float = float("inf"), want_counts: bool = False):
        """The k nearest triangles of every query point within its squared radius: (n, k) NEIGHBOR_DTYPE records in order, unused entries
        {+inf, NO_PRIM}.  With want_counts=True returns (records, counts): counts (n,) uint32, the full numbers of neighbours (the
        search then cannot shrink its bound to the slot)."""
        p, r = self._neighbor_points(points, radius2)
        out, counts = self._slots_first("neighbors", (_ptr(p), len(p), _ptr(r), float(max_dist2)), k, want_counts)
        return (out, counts) if want_counts else out

    def debug_neighbor_work(self, points, radius2=None, max_dist2: float = float("inf"), k: int = 0):
        """cgrt_debug_neighbor_work: (node steps, triangles evaluated), summed over the queries (a separate counting launch), of
        count_neighbors' search (k = 0) or of nearest_triangles' (k > 0: the shrinking bound)."""
        p, r = self._neighbor_points(points, radius2)
        w = np.zeros(2, np.uint64)
        _check(lib().cgrt_debug_neighbor_work(self._h, _ptr(p), len(p), _ptr(r), float(max_dist2), int(k), _ptr(w)))
        return int(w[0]), int(w[1])

    def count_neighbors_device(self, d_points_ptr: int, n: int, d_counts_ptr: int, d_radius2_ptr: int = 0, max_dist2: float = float("inf"),
                               stream: int = 0) -> None:
        """cgrt_count_neighbors_device: n points (3 floats each) at d_points_ptr (and n squared radii at d_radius2_ptr, or 0) -> n uint32
        counts at d_counts_ptr, enqueued on the hipStream_t `stream`.  Raw integers."""
        _check(lib().cgrt_count_neighbors_device(self._h, _vp(d_points_ptr), int(n), _vp(d_radius2_ptr), float(max_dist2), _vp(d_counts_ptr),
                                                 _vp(stream)))

    def list_neighbors_device(self, d_points_ptr: int, n: int, d_out_ptr: int, capacity: int, d_offsets_ptr: int = 0, k: int = 0,
                              d_counts_ptr: int = 0, d_radius2_ptr: int = 0, max_dist2: float = float("inf"), stream: int = 0) -> None:
        """cgrt_list_neighbors_device: slots from the n + 1 uint64 offsets at d_offsets_ptr, or of k records each; `capacity` records of
        8 bytes at d_out_ptr, nothing beyond them is written whatever the offsets hold; d_counts_ptr (optional) receives the full counts.
        Enqueued on `stream`.  Raw integers."""
        _check(lib().cgrt_list_neighbors_device(self._h, _vp(d_points_ptr), int(n), _vp(d_radius2_ptr), float(max_dist2), _vp(d_offsets_ptr),
                                                int(k), _vp(d_out_ptr), int(capacity), _vp(d_counts_ptr), _vp(stream)))

    def _neighbor_tensors(self, points, radius2, max_dist2):
        """(n, the radii's address or 0, the scalar bound) of a *_tensor call: radius2 a float (it replaces max_dist2) or an (n,) tensor."""
        import torch

        n = self._points_tensor(points)
        if radius2 is None:
            return n, 0, float(max_dist2)
        if isinstance(radius2, torch.Tensor):
            self._device_tensor(radius2, "radius2", (torch.float32,), (n,))
            return n, (radius2.data_ptr() if n else 0), float(max_dist2)
        return n, 0, float(radius2)

    def count_neighbors_tensor(self, points, radius2=None, max_dist2: float = float("inf"), out=None, stream=None):
        """count_neighbors on torch tensors: points (n, 3) float32 on cuda:<device>, radius2 None, a float (one squared radius for every
        query) or an (n,) float32 tensor -> (n,) torch.int32, into `out` or a new tensor, enqueued on `stream` (default:
        torch.cuda.current_stream())."""
        import torch

        n, rad, md = self._neighbor_tensors(points, radius2, max_dist2)
        if out is not None:
            self._device_tensor(out, "out", (torch.int32,), (n,))
        return self._tensor_call(out, (n,), torch.int32, stream,
                                 lambda o, s: self.count_neighbors_device(points.data_ptr(), n, o.data_ptr(), d_radius2_ptr=rad, max_dist2=md, stream=s))

    def list_neighbors_tensor(self, points, radius2=None, max_dist2: float = float("inf"), stream=None):
        """list_neighbors on torch tensors -> (offsets (n + 1,) torch.int64, records (m, 2) float32 with the prim_id BITS in column 1:
        records.view(torch.int32)[:, 1]).  Count, a torch cumsum and the list are enqueued on `stream`; the total m is read back in
        between (one synchronisation of that stream)."""
        n, rad, md = self._neighbor_tensors(points, radius2, max_dist2)
        return self._slots_full_tensor(n, stream, lambda s: self.count_neighbors_tensor(points, radius2, max_dist2, stream=s),
                                       lambda o, m, off, s: self.list_neighbors_device(points.data_ptr(), n, o, m, d_offsets_ptr=off,
                                                                                       d_radius2_ptr=rad, max_dist2=md, stream=s))

    def nearest_triangles_tensor(self, points, k: int, radius2=None, max_dist2: float = float("inf"), want_counts: bool = False, out=None,
                                 stream=None):
        """nearest_triangles on torch tensors -> records (n, k, 2) float32 (`out`, or a new tensor; the prim_id bits in [..., 1], unused
        entries {+inf, NO_PRIM}); with want_counts=True (records, counts (n,) torch.int32: the full numbers of neighbours)."""
        n, rad, md = self._neighbor_tensors(points, radius2, max_dist2)
        rec, counts = self._slots_first_tensor(n, k, want_counts, out, stream,
                                               lambda o, c, s: self.list_neighbors_device(points.data_ptr(), n, o, n * k, k=k, d_counts_ptr=c,
                                                                                          d_radius2_ptr=rad, max_dist2=md, stream=s))
        return (rec, counts) if want_counts else rec

    def inside_tensor(self, points, directions=None, stream=None):
        """Inside / outside for points (n, 3) float32 on cuda:<device>, meaningful for WATERTIGHT meshes: the majority vote, over an odd
        number of fixed directions (default: the three of INSIDE_DIRECTIONS), of the parity of count_crossings along the unbounded ray from
        the point.  One ray's parity fails where the ray passes exactly through a shared edge or a vertex (both triangles are crossed);
        the vote absorbs one such failure in three.  A composition in Python: no kernel of its own (sdf_tensor(want=("inside",)) is the
        native entry with the same bytes).  Returns (n,) torch.bool."""
        import torch

        self._points_tensor(points)
        dirs = np.asarray(INSIDE_DIRECTIONS if directions is None else directions, np.float32).reshape(-1, 3)
        if len(dirs) % 2 == 0:
            raise ValueError("an odd number of directions is needed for a majority")
        n = points.shape[0]
        dev, stream = self._torch_stream(stream)
        with torch.cuda.stream(stream):
            votes = torch.zeros((n,), dtype=torch.int32, device=dev)
            for d in dirs:
                rays = torch.empty((n, 7), dtype=torch.float32, device=dev)
                rays[:, 0:3] = points
                rays[:, 3:6] = torch.tensor(d, dtype=torch.float32, device=dev)
                rays[:, 6] = float("inf")
                votes += self.count_crossings_tensor(rays, stream=stream) & 1
            return votes > len(dirs) // 2

    def signed_distance_tensor(self, points, stream=None):
        """Signed distance for points (n, 3) float32 on cuda:<device>, meaningful for watertight meshes: sqrt(closest_points' dist2),
        negated where inside_tensor says inside.  A composition in Python (sdf_tensor is the native entry with the same bytes).  Returns
        (n,) float32."""
        import torch

        inside = self.inside_tensor(points, stream=stream)
        _, stream = self._torch_stream(stream)
        d2 = self.closest_points_tensor(points, stream=stream)["dist2"]
        with torch.cuda.stream(stream):
            dist = torch.sqrt(d2)
            return torch.where(inside, -dist, dist)

    # ---- signed distance and occupancy (include/cgrt.h cgrt_signed_distance*) ----
    @staticmethod
    def _field_want(want, value: str):
        """`want` of the signed-distance (value "sdf") and winding (value "w") entries as a tuple of names."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(w not in (value, "inside") for w in want) or len(set(want)) != len(want):
            raise ValueError(f'want must name "{value}", "inside" or both')
        return want

    def _field_host(self, f, value: str, want, params, points=None, grid=None):
        """The host form of a signed-distance or winding entry f on a point list (points) or a grid (grid = (origin, spacing, dims)):
        the arrays named by `want` ((n,), or (nz, ny, nx) for a grid), as _sdf_result returns them.  params() makes the parameter
        structure, after the points have been looked at."""
        want = self._field_want(want, value)
        if grid is None:
            p = _f32(points, (-1, 3))
            lead, shape, m = (_ptr(p), len(p)), (len(p),), len(p)
        else:
            g = _sdf_grid_struct(*grid)
            lead, shape = (C.byref(g),), (g.dims[2], g.dims[1], g.dims[0])
            m = shape[0] * shape[1] * shape[2] if max(shape) <= 1 << 24 and shape[0] * shape[1] * shape[2] <= 0x7FFFFFFF else 0  # (else: the library says why)
        prm = params()
        res = {value: np.zeros(m, np.float32) if value in want else None, "inside": np.zeros(m, np.uint8) if "inside" in want else None}
        _check(f(self._h, *lead, C.byref(prm), _ptr(res[value]), _ptr(res["inside"])))
        return self._sdf_result({k: (None if v is None else v.reshape(shape)) for k, v in res.items()}, want)

    def sdf(self, points, max_dist2: float = float("inf"), directions=None, want=("sdf", "inside")):
        """cgrt_signed_distance: for every point ((n, 3) float32) sqrt(closest_points' dist2), negative where the majority of the parity
        walks along `directions` (None: INSIDE_DIRECTIONS; an odd number, at most 7) says inside -- one fused kernel, the bytes of
        signed_distance_tensor / inside_tensor.  Beyond max_dist2 the value is +-inf; a non-finite point gets (+inf, False).  Returns the
        arrays named by `want`, in that order ((n,) float32 / (n,) bool); a single name returns the array itself."""
        return self._field_host(lib().cgrt_signed_distance, "sdf", want, lambda: _sdf_params(max_dist2, directions), points=points)

    @staticmethod
    def _sdf_result(res, want):
        if res["inside"] is not None and res["inside"].dtype == np.uint8:
            res["inside"] = res["inside"].view(np.bool_)
        out = tuple(res[w] for w in want)
        return out[0] if len(out) == 1 else out

    def sdf_device(self, d_points_ptr: int, n: int, d_sdf_ptr: int, d_inside_ptr: int, max_dist2: float = float("inf"), directions=None,
                   stream: int = 0) -> None:
        """cgrt_signed_distance_device: n points (3 floats each) at d_points_ptr -> n float32 at d_sdf_ptr and / or n bytes (0 / 1) at
        d_inside_ptr (0: not wanted; without d_sdf_ptr the closest-point search is not run), enqueued on the hipStream_t `stream`.  Raw
        integers."""
        prm = _sdf_params(max_dist2, directions)
        _check(lib().cgrt_signed_distance_device(self._h, _vp(d_points_ptr), int(n), C.byref(prm), _vp(d_sdf_ptr), _vp(d_inside_ptr), _vp(stream)))

    def _sdf_tensors(self, shape, want, out, stream, call, value="sdf"):
        """The *_tensor conventions for the two outputs (`value`: the name of the float32 one): `out` None, or a dict / tuple (in want's
        order) of tensors to write into."""
        import torch

        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        if out is not None and not isinstance(out, dict):
            out = (out,) if isinstance(out, torch.Tensor) else tuple(out)
            if len(out) != len(want):
                raise ValueError("out must hold one tensor per name in want")
            out = dict(zip(want, out))
        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        res = {}
        for w, dtypes in ((value, (torch.float32,)), ("inside", (torch.bool, torch.uint8))):
            if w not in want:
                continue
            t = None if out is None else out.get(w)
            if t is None:
                with torch.cuda.stream(stream):  # (allocated on the stream the answers are written on)
                    t = torch.empty(shape, dtype=dtypes[0], device=dev)
            else:
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype not in dtypes:
                    raise ValueError(f"out[{w!r}] must be a torch tensor of shape {tuple(shape)} and one of {dtypes}")
                if t.device.type != "cuda" or t.device.index != self.device or not t.is_contiguous() or (w == value and t.data_ptr() % 4):
                    raise ValueError(f"out[{w!r}] must be contiguous ({value}: 4-byte aligned) on cuda:{self.device}")
            res[w] = t
        if int(np.prod(shape)):  # (an empty tensor has no address to pass: the call would touch nothing anyway)
            call(res[value].data_ptr() if value in res else 0, res["inside"].data_ptr() if "inside" in res else 0, stream.cuda_stream)
        got = tuple(res[w] for w in want)
        return got[0] if len(got) == 1 else got

    def sdf_tensor(self, points, max_dist2: float = float("inf"), directions=None, want=("sdf", "inside"), out=None, stream=None):
        """sdf on torch tensors: points (n, 3) float32 on cuda:<device> -> the tensors named by `want`, in that order ((n,) float32 /
        (n,) torch.bool; a single name returns the tensor itself), written into `out` (one tensor, a tuple in want's order or a dict by
        name; inside may also be torch.uint8) or new ones, enqueued on `stream` (default: torch.cuda.current_stream())."""
        want = self._field_want(want, "sdf")
        n = self._points_tensor(points, shape_first=True)
        return self._sdf_tensors((n,), want, out, stream,
                                 lambda ds, di, s: self.sdf_device(points.data_ptr(), n, ds, di, max_dist2=max_dist2, directions=directions, stream=s))

    def sdf_grid(self, origin, spacing, dims, max_dist2: float = float("inf"), directions=None, want=("sdf", "inside")):
        """cgrt_signed_distance_grid: sdf on the regular grid of sdf_grid_points(origin, spacing, dims), dims = (nx, ny, nz); the lanes
        make their own points.  Returns the arrays named by `want` shaped (nz, ny, nx) (x fastest), as sdf returns them."""
        return self._field_host(lib().cgrt_signed_distance_grid, "sdf", want, lambda: _sdf_params(max_dist2, directions),
                                grid=(origin, spacing, dims))

    def sdf_grid_device(self, origin, spacing, dims, d_sdf_ptr: int, d_inside_ptr: int, max_dist2: float = float("inf"), directions=None,
                        stream: int = 0) -> None:
        """cgrt_signed_distance_grid_device: nx * ny * nz float32 at d_sdf_ptr and / or bytes at d_inside_ptr (0: not wanted), in
        (nz, ny, nx) order, enqueued on the hipStream_t `stream`.  Raw integers."""
        g, prm = _sdf_grid_struct(origin, spacing, dims), _sdf_params(max_dist2, directions)
        _check(lib().cgrt_signed_distance_grid_device(self._h, C.byref(g), C.byref(prm), _vp(d_sdf_ptr), _vp(d_inside_ptr), _vp(stream)))

    def sdf_grid_tensor(self, origin, spacing, dims, max_dist2: float = float("inf"), directions=None, want=("sdf", "inside"), out=None,
                        stream=None):
        """sdf_grid on torch tensors: the tensors named by `want`, shaped (nz, ny, nx), as sdf_tensor returns them."""
        want = self._field_want(want, "sdf")
        nx, ny, nz = (int(x) for x in dims)
        return self._sdf_tensors((nz, ny, nx), want, out, stream,
                                 lambda ds, di, s: self.sdf_grid_device(origin, spacing, dims, ds, di, max_dist2=max_dist2, directions=directions,
                                                                        stream=s))

    def debug_sdf_work(self, points, max_dist2: float = float("inf"), directions=None, want_sdf: bool = True):
        """cgrt_debug_sdf_work: (closest node steps, closest triangles evaluated, crossing node steps, crossing triangles evaluated,
        direction walks run) of sdf's search, summed over the points (a separate counting launch)."""
        p = _f32(points, (-1, 3))
        prm = _sdf_params(max_dist2, directions)
        w = np.zeros(5, np.uint64)
        _check(lib().cgrt_debug_sdf_work(self._h, _ptr(p), len(p), C.byref(prm), 1 if want_sdf else 0, _ptr(w)))
        return tuple(int(x) for x in w)

    # ---- winding numbers (include/cgrt.h cgrt_winding_numbers*) ----
    def winding_numbers(self, points, beta: float = 2.0, threshold: float = 0.5, want=("w", "inside")):
        """cgrt_winding_numbers: for every point ((n, 3) float32) the generalised winding number of the scene's triangles -- +-1 inside a
        closed mesh, 0 outside, smooth near holes: a sign that also means something on OPEN meshes -- by the cluster tree (far clusters,
        from `beta` cluster radii on, are replaced by their dipole; beta = inf: every triangle, the bytes of winding_numbers_brute), and
        inside = |w| > threshold.  A non-finite point gets (0, False).  Returns the arrays named by `want`, in that order ((n,) float32 /
        (n,) bool); a single name returns the array itself."""
        return self._field_host(lib().cgrt_winding_numbers, "w", want, lambda: _winding_params(beta, threshold), points=points)

    def winding_numbers_brute(self, points, threshold: float = 0.5, want=("w", "inside")):
        """cgrt_winding_numbers_brute: the sum over every triangle in record order (validation; what winding_numbers returns with
        beta = inf, byte for byte)."""
        return self._field_host(lib().cgrt_winding_numbers_brute, "w", want, lambda: _winding_params(0.0, threshold), points=points)

    def winding_numbers_device(self, d_points_ptr: int, n: int, d_w_ptr: int, d_inside_ptr: int, beta: float = 2.0, threshold: float = 0.5,
                               stream: int = 0) -> None:
        """cgrt_winding_numbers_device: n points (3 floats each) at d_points_ptr -> n float32 at d_w_ptr and / or n bytes (0 / 1) at
        d_inside_ptr (0: not wanted), enqueued on the hipStream_t `stream`.  Raw integers."""
        prm = _winding_params(beta, threshold)
        _check(lib().cgrt_winding_numbers_device(self._h, _vp(d_points_ptr), int(n), C.byref(prm), _vp(d_w_ptr), _vp(d_inside_ptr), _vp(stream)))

    def winding_numbers_tensor(self, points, beta: float = 2.0, threshold: float = 0.5, want=("w", "inside"), out=None, stream=None):
        """winding_numbers on torch tensors: points (n, 3) float32 on cuda:<device> -> the tensors named by `want`, in that order ((n,)
        float32 / (n,) torch.bool; a single name returns the tensor itself), written into `out` (one tensor, a tuple in want's order or
        a dict by name; inside may also be torch.uint8) or new ones, enqueued on `stream` (default: torch.cuda.current_stream())."""
        want = self._field_want(want, "w")
        n = self._points_tensor(points, shape_first=True)
        return self._sdf_tensors((n,), want, out, stream,
                                 lambda dw, di, s: self.winding_numbers_device(points.data_ptr(), n, dw, di, beta=beta, threshold=threshold, stream=s),
                                 value="w")

    def winding_grid(self, origin, spacing, dims, beta: float = 2.0, threshold: float = 0.5, want=("w", "inside")):
        """cgrt_winding_numbers_grid: winding_numbers on the regular grid of sdf_grid_points(origin, spacing, dims), dims = (nx, ny, nz);
        the lanes make their own points.  Returns the arrays named by `want` shaped (nz, ny, nx) (x fastest)."""
        return self._field_host(lib().cgrt_winding_numbers_grid, "w", want, lambda: _winding_params(beta, threshold),
                                grid=(origin, spacing, dims))

    def winding_grid_device(self, origin, spacing, dims, d_w_ptr: int, d_inside_ptr: int, beta: float = 2.0, threshold: float = 0.5,
                            stream: int = 0) -> None:
        """cgrt_winding_numbers_grid_device: nx * ny * nz float32 at d_w_ptr and / or bytes at d_inside_ptr (0: not wanted), in
        (nz, ny, nx) order, enqueued on the hipStream_t `stream`.  Raw integers."""
        g, prm = _sdf_grid_struct(origin, spacing, dims), _winding_params(beta, threshold)
        _check(lib().cgrt_winding_numbers_grid_device(self._h, C.byref(g), C.byref(prm), _vp(d_w_ptr), _vp(d_inside_ptr), _vp(stream)))

    def winding_grid_tensor(self, origin, spacing, dims, beta: float = 2.0, threshold: float = 0.5, want=("w", "inside"), out=None, stream=None):
        """winding_grid on torch tensors: the tensors named by `want`, shaped (nz, ny, nx), as winding_numbers_tensor returns them."""
        want = self._field_want(want, "w")
        nx, ny, nz = (int(x) for x in dims)
        return self._sdf_tensors((nz, ny, nx), want, out, stream,
                                 lambda dw, di, s: self.winding_grid_device(origin, spacing, dims, dw, di, beta=beta, threshold=threshold, stream=s),
                                 value="w")

    def debug_winding_work(self, points, beta: float = 2.0):
        """cgrt_debug_winding_work: (clusters tested, dipoles taken, triangles evaluated) of winding_numbers' walk, summed over the points
        (a separate counting launch)."""
        p = _f32(points, (-1, 3))
        prm = _winding_params(beta)
        w = np.zeros(3, np.uint64)
        _check(lib().cgrt_debug_winding_work(self._h, _ptr(p), len(p), C.byref(prm), _ptr(w)))
        return tuple(int(x) for x in w)

    def debug_winding_tree(self):
        """cgrt_debug_get_winding_tree (works host-only): {'clusters': (m, 8) float32 rows {c.xyz, r2, n.xyz, 0}, 'level_offsets':
        (nlevels + 1,) int64 -- level L is rows [level_offsets[L], level_offsets[L + 1]), level 0 first --, 'record_prims': (ntris,)
        uint32, the prim_id of every triangle record in record order: level 0's cluster i covers records [8 i, 8 i + 8)}."""
        nlev = C.c_uint32(0)
        off = np.zeros(10, np.uint32)
        _check(lib().cgrt_debug_get_winding_tree(self._h, None, _ptr(off), C.byref(nlev), None))
        off = off[: nlev.value + 1]
        clusters = np.zeros((int(off[-1]), 8), np.float32)
        prims = np.zeros(int(np.asarray(self.sd.tri).size // 3), np.uint32)
        _check(lib().cgrt_debug_get_winding_tree(self._h, _ptr(clusters), None, C.byref(nlev), _ptr(prims)))
        return {"clusters": clusters, "level_offsets": off.astype(np.int64), "record_prims": prims}

    def inside_winding_tensor(self, points, beta: float = 2.0, threshold: float = 0.5, stream=None):
        """Inside / outside by the winding number, meaningful for open meshes too: |winding_numbers_tensor| > threshold.  (n,) torch.bool."""
        return self.winding_numbers_tensor(points, beta=beta, threshold=threshold, want=("inside",), stream=stream)

    def signed_distance_winding_tensor(self, points, max_dist2: float = float("inf"), beta: float = 2.0, stream=None):
        """Signed distance with the winding number's sign: sqrt(closest_points' dist2), negated where |w| > 0.5.  On a closed mesh away
        from the surface these are sdf_tensor's bytes; on an open mesh the sign still means something.  A composition in Python (the
        signed-distance kernel is left as it is).  Returns (n,) float32."""
        import torch

        inside = self.inside_winding_tensor(points, beta=beta, stream=stream)
        _, stream = self._torch_stream(stream)
        d2 = self.closest_points_tensor(points, max_dist2=max_dist2, stream=stream)["dist2"]
        with torch.cuda.stream(stream):
            dist = torch.sqrt(d2)
            return torch.where(inside, -dist, dist)

    # ---- surface sampling (include/cgrt.h cgrt_sample_surface*) ----
    def triangle_areas(self):
        """cgrt_triangle_areas (works host-only): ((ntris,) float32 areas in prim_id order -- the reference's area function, 0 where it is
        NaN, infinite or not > 0 --, their float64 sum added in that order)."""
        areas = np.zeros(int(np.asarray(self.sd.tri).size // 3), np.float32)
        total = C.c_double(0.0)
        _check(lib().cgrt_triangle_areas(self._h, _ptr(areas) if len(areas) else None, C.byref(total)))
        return areas, float(total.value)

    def debug_sample_table(self):
        """cgrt_debug_get_sample_table (works host-only): {'thresholds': (ntris,) uint32, 'last': the largest prim_id with an area, or
        NO_PRIM when the scene is empty for sampling}."""
        thr = np.zeros(int(np.asarray(self.sd.tri).size // 3), np.uint32)
        last = C.c_uint32(0)
        _check(lib().cgrt_debug_get_sample_table(self._h, _ptr(thr) if len(thr) else None, C.byref(last)))
        return {"thresholds": thr, "last": int(last.value)}

    def sample_surface(self, n: int, seed: int = 0, first: int = 0, strata: int = 0, attr=None):
        """cgrt_sample_surface: samples first .. first + n - 1 of the stream `seed` -- area-weighted points on the scene's triangles, each
        a function of (scene, seed, index, strata) alone; strata = N > 0 puts sample j into stratum j of N equal strata of the area.
        Returns a SURFACE_SAMPLE_DTYPE array {point, mesh_id, prim_id, bary}; with attr ((nverts, C) float32) also the (n, C) rows
        (bary0 * attr[i0] + bary1 * attr[i1]) + bary2 * attr[i2].  A scene without a triangle of positive area gives
        {0, 0xffffffff, NO_PRIM, 0} records and zero rows."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        prm = _sample_params(seed, first, strata)
        out = np.zeros(n, SURFACE_SAMPLE_DTYPE)
        if attr is None:
            _check(lib().cgrt_sample_surface(self._h, n, C.byref(prm), _ptr(out) if n else None, None, 0, None))
            return out
        a = self._attr_array(attr)
        rows = np.zeros((n, a.shape[1]), np.float32)
        _check(lib().cgrt_sample_surface(self._h, n, C.byref(prm), _ptr(out) if n else None, _ptr(a), a.shape[1], _ptr(rows)))
        return out, rows

    def sample_surface_device(self, n: int, d_out_ptr: int, seed: int = 0, first: int = 0, strata: int = 0, d_attr_ptr: int = 0,
                              channels: int = 0, d_out_attr_ptr: int = 0, stream: int = 0) -> None:
        """cgrt_sample_surface_device: n SURFACE_SAMPLE_DTYPE records (32 bytes each) to d_out_ptr and, with a table (d_attr_ptr:
        (nverts, channels) float32), n x channels floats to d_out_attr_ptr; enqueued on the hipStream_t `stream`.  Raw integers."""
        prm = _sample_params(seed, first, strata)
        _check(lib().cgrt_sample_surface_device(self._h, int(n), C.byref(prm), _vp(d_out_ptr), _vp(d_attr_ptr), int(channels),
                                                _vp(d_out_attr_ptr), _vp(stream)))

    def sample_surface_tensor(self, n: int, seed: int = 0, first: int = 0, strata: int = 0, attr=None, out=None, out_attr=None, stream=None):
        """sample_surface on torch tensors: an (n, 8) float32 tensor of SURFACE_SAMPLE_DTYPE records (`out`, or a new one) on
        cuda:<device>, enqueued on `stream` (default: torch.cuda.current_stream()).  Returns a dict of views of it: 'point' (n, 3),
        'mesh_id' and 'prim_id' (n,) int32 (-1 = NO_PRIM), 'bary' (n, 3), 'out' itself, and with attr ((nverts, C) float32 on the device)
        'attr': the (n, C) rows (`out_attr`, or a new tensor)."""
        import torch

        n = int(n)
        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        if n < 0:
            raise ValueError("n must be >= 0")
        if out is not None:
            self._device_tensor(out, "out", (torch.float32,), (n, 8))
        if attr is None:
            if out_attr is not None:
                raise ValueError("out_attr needs attr")
            o = self._tensor_call(out, (n, 8), torch.float32, stream,
                                  lambda t, s: self.sample_surface_device(n, t.data_ptr(), seed=seed, first=first, strata=strata, stream=s))
            rows = None
        else:
            attr = self._attr_tensor(attr)
            ch = attr.shape[1]
            if out_attr is not None:
                self._device_tensor(out_attr, "out_attr", (torch.float32,), (n, ch))
            _, stream = self._torch_stream(stream)
            rows = self._tensor_call(out_attr, (n, ch), torch.float32, stream, lambda t, s: None)  # (out_attr, or new on the stream)
            o = self._tensor_call(out, (n, 8), torch.float32, stream,
                                  lambda t, s: self.sample_surface_device(n, t.data_ptr(), seed=seed, first=first, strata=strata,
                                                                          d_attr_ptr=attr.data_ptr(), channels=ch,
                                                                          d_out_attr_ptr=rows.data_ptr(), stream=s))
        res = {"point": o[:, 0:3], "mesh_id": o.view(torch.int32)[:, 3], "prim_id": o.view(torch.int32)[:, 4], "bary": o[:, 5:8], "out": o}
        if rows is not None:
            res["attr"] = rows
        return res

    # ---- Poisson-disk sets (include/cgrt.h cgrt_poisson_disk*) ----
    @staticmethod
    def _priority_array(priority, n: int):
        if priority is None:
            return None
        a = np.asarray(priority)
        if a.shape != (n,) or a.dtype.kind not in "iu" or (a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF)):
            raise ValueError(f"priority must be ({n},) integers in 0 .. 2^32 - 1")
        return np.ascontiguousarray(a, np.uint32)

    def _poisson_host(self, f, points, min_dist2: float, seed: int, priority) -> np.ndarray:
        p = _f32(points, (-1, 3))
        pr = self._priority_array(priority, len(p))
        prm = _poisson_params(min_dist2, seed, pr.ctypes.data if pr is not None and len(pr) else 0)
        keep = np.zeros(len(p), np.uint8)
        kept = C.c_uint64(0)
        _check(f(self._h, _ptr(p) if len(p) else None, len(p), C.byref(prm), _ptr(keep) if len(p) else None, C.byref(kept)))
        mask = keep.view(np.bool_)
        if int(kept.value) != int(mask.sum()):
            raise RuntimeError(f"the library reports {int(kept.value)} kept points, its flags hold {int(mask.sum())}")
        return mask

    def poisson_disk(self, points, min_dist2: float, seed: int = 0, priority=None) -> np.ndarray:
        """cgrt_poisson_disk: of the points ((n, 3) float32), the (n,) bool mask of the lexicographically first maximal subset in which no
        two points have a squared distance below min_dist2.  Point i goes before j iff (P_i, i) < (P_j, j), P the caller's priority
        ((n,) uint32) or Philox word 3 of index i under `seed`.  A non-finite point is never kept; min_dist2 NaN or <= 0 keeps every
        finite point.  Defined to the last bit (include/cgrt.h); blocks."""
        return self._poisson_host(lib().cgrt_poisson_disk, points, min_dist2, seed, priority)

    def poisson_disk_brute(self, points, min_dist2: float, seed: int = 0, priority=None) -> np.ndarray:
        """cgrt_poisson_disk_brute: poisson_disk without the grid, every pair tested in every round (validation; the same bytes)."""
        return self._poisson_host(lib().cgrt_poisson_disk_brute, points, min_dist2, seed, priority)

    def debug_poisson_work(self, points, min_dist2: float, seed: int = 0, priority=None) -> dict:
        """cgrt_debug_poisson_work (a counted run): {'rounds', 'pair_tests', 'buckets_used', 'buckets', 'build_ns', 'rounds_ns'}."""
        p = _f32(points, (-1, 3))
        pr = self._priority_array(priority, len(p))
        prm = _poisson_params(min_dist2, seed, pr.ctypes.data if pr is not None and len(pr) else 0)
        w = np.zeros(6, np.uint64)
        _check(lib().cgrt_debug_poisson_work(self._h, _ptr(p) if len(p) else None, len(p), C.byref(prm), _ptr(w)))
        return dict(zip(("rounds", "pair_tests", "buckets_used", "buckets", "build_ns", "rounds_ns"), (int(x) for x in w)))

    def poisson_disk_workspace(self, n: int) -> int:
        """cgrt_poisson_disk_workspace: the bytes of device memory a poisson_disk_device call with n points needs."""
        b = C.c_uint64(0)
        _check(lib().cgrt_poisson_disk_workspace(self._h, int(n), C.byref(b)))
        return int(b.value)

    def poisson_disk_device(self, d_points_ptr: int, n: int, min_dist2: float, d_keep_ptr: int, d_workspace_ptr: int, workspace_bytes: int,
                            seed: int = 0, d_priority_ptr: int = 0, stream: int = 0) -> int:
        """cgrt_poisson_disk_device: n points (3 floats each) at d_points_ptr -> n flag bytes at d_keep_ptr, with the caller's workspace
        (poisson_disk_workspace(n) bytes of device memory, 8-byte aligned, this call's alone).  Ordered on the hipStream_t `stream`;
        returns the number of kept points once the flags are complete.  Raw integers."""
        prm = _poisson_params(min_dist2, seed, d_priority_ptr)
        kept = C.c_uint64(0)
        _check(lib().cgrt_poisson_disk_device(self._h, _vp(d_points_ptr), int(n), C.byref(prm), _vp(d_keep_ptr), C.byref(kept),
                                              _vp(d_workspace_ptr), int(workspace_bytes), _vp(stream)))
        return int(kept.value)

    def poisson_disk_tensor(self, points, min_dist2: float, seed: int = 0, priority=None, out=None, workspace=None, stream=None):
        """poisson_disk on torch tensors: points (n, 3) float32 on cuda:<device> -> an (n,) torch.bool mask (`out`, which may also be
        torch.uint8, or a new tensor).  priority: None, or an (n,) torch.int32 / torch.uint32 tensor whose words are read as unsigned.
        workspace: None (allocated here on the call's stream), or a torch.uint8 tensor of at least poisson_disk_workspace(n) bytes,
        8-byte aligned.  Ordered on `stream` (default: torch.cuda.current_stream()); returns when the mask is complete."""
        import torch

        n = self._points_tensor(points)
        if out is not None:
            self._device_tensor(out, "out", (torch.bool, torch.uint8), (n,))
        if priority is not None:
            self._device_tensor(priority, "priority", (torch.int32, getattr(torch, "uint32", torch.int32)), (n,))
        nbytes = self.poisson_disk_workspace(n)
        if workspace is not None:
            self._device_tensor(workspace, "workspace", (torch.uint8,))
            if workspace.numel() < nbytes or workspace.data_ptr() % 8:
                raise ValueError(f"workspace must hold {nbytes} bytes and be 8-byte aligned")
        _, stream = self._torch_stream(stream)
        if workspace is None and n:
            with torch.cuda.stream(stream):
                workspace = torch.empty((nbytes,), dtype=torch.uint8, device=stream.device)
        return self._tensor_call(out, (n,), torch.bool, stream,
                                 lambda o, s: self.poisson_disk_device(points.data_ptr(), n, min_dist2, o.data_ptr(), workspace.data_ptr(),
                                                                       workspace.numel(), seed=seed,
                                                                       d_priority_ptr=priority.data_ptr() if priority is not None else 0,
                                                                       stream=s))

    def sample_surface_poisson_tensor(self, candidates: int, min_dist2: float, seed: int = 0, strata: bool = True, attr=None):
        """Blue-noise surface samples: sample_surface_tensor(candidates, seed, strata = candidates or 0), its points filtered by
        poisson_disk_tensor under the same seed.  Returns sample_surface_tensor's keys restricted to the kept rows, in ascending
        candidate index, plus 'index' ((kept,) int64, the candidate indices): a function of (scene, candidates, min_dist2, seed,
        strata) alone."""
        import torch

        candidates = int(candidates)
        res = self.sample_surface_tensor(candidates, seed=seed, strata=candidates if strata else 0, attr=attr)
        _, stream = self._torch_stream(None)
        with torch.cuda.stream(stream):
            mask = self.poisson_disk_tensor(res["point"].contiguous(), min_dist2, seed=seed, stream=stream)
            index = torch.nonzero(mask).reshape(-1)
            out = {k: v[index] for k, v in res.items()}
        out["index"] = index
        return out

    # ---- point-set neighbours (include/cgrt.h cgrt_point_grid_*, cgrt_count_point_neighbors*, cgrt_list_point_neighbors*) ----
    @staticmethod
    def _point_cloud_args(data, points, radius2, max_dist2, skip_same_index):
        """(data (m, 3), points (n, 3), the radii or None -- kept alive by the caller --, the CgrtPointQuery)."""
        d, p = _f32(data, (-1, 3)), _f32(points, (-1, 3))
        r = None if radius2 is None else _f32(radius2, (-1,))
        if r is not None and len(r) != len(p):
            raise ValueError("radius2 must hold one squared radius per point")
        return d, p, r, _point_query(r.ctypes.data if r is not None and len(r) else 0, max_dist2, skip_same_index)

    def _point_list_host(self, d, cell, p, q, offsets, k: int, want_counts: bool = True, brute: bool = False):
        """One cgrt_list_point_neighbors(_brute) call into slots from `offsets` or of k records each: (records, counts or None)."""
        n = len(p)
        cap = int(offsets[-1]) if offsets is not None else n * k
        out = np.zeros(cap, POINT_NEIGHBOR_DTYPE)
        counts = np.zeros(n, np.uint32) if want_counts else None
        tail = (_ptr(p), n, C.byref(q), _ptr(offsets), int(k), _ptr(out), cap, _ptr(counts))
        if brute:
            _check(lib().cgrt_list_point_neighbors_brute(self._h, _ptr(d), len(d), *tail))
        else:
            _check(lib().cgrt_list_point_neighbors(self._h, _ptr(d), len(d), float(cell), *tail))
        return out, counts

    def _point_list_full(self, d, cell, p, q, counts, brute: bool = False):
        off = np.zeros(len(p) + 1, np.uint64)
        np.cumsum(counts, dtype=np.uint64, out=off[1:])
        out, _ = self._point_list_host(d, cell, p, q, off, 0, want_counts=False, brute=brute)
        return off.astype(np.int64), out

    def count_point_neighbors(self, data, cell: float, points, radius2=None, max_dist2: float = float("inf"),
                              skip_same_index: bool = False) -> np.ndarray:
        """cgrt_count_point_neighbors: for every query point ((n, 3) float32) the number of points of `data` ((m, 3) float32) whose d2 is
        <= its squared radius -- radius2[i] ((n,) float32; NaN or negative: no neighbours), or max_dist2 for every query.  cell: the
        wanted cell edge of the call's own grid (about the radius; no result depends on it).  skip_same_index: data point i is not a
        neighbour of query i.  (n,) uint32."""
        d, p, r, q = self._point_cloud_args(data, points, radius2, max_dist2, skip_same_index)
        counts = np.zeros(len(p), np.uint32)
        _check(lib().cgrt_count_point_neighbors(self._h, _ptr(d), len(d), float(cell), _ptr(p), len(p), C.byref(q), _ptr(counts)))
        return counts

    def list_point_neighbors(self, data, cell: float, points, radius2=None, max_dist2: float = float("inf"), skip_same_index: bool = False,
                             offsets=None, want_counts: bool = True):
        """Every neighbour of every query point among `data`, in order (by d2, equal d2 by index): cgrt_count_point_neighbors, the
        exclusive prefix sums, then cgrt_list_point_neighbors.  Returns (offsets, records): offsets (n + 1,) int64, query i's neighbours
        are records[offsets[i]:offsets[i + 1]] (POINT_NEIGHBOR_DTYPE {dist2, index}).
        With offsets ((n + 1,) slot boundaries chosen by the caller) one cgrt_list_point_neighbors call: (records (offsets[-1],),
        counts: the full numbers of neighbours -- or None with want_counts=False), as list_neighbors."""
        d, p, r, q = self._point_cloud_args(data, points, radius2, max_dist2, skip_same_index)
        if offsets is not None:
            return self._point_list_host(d, cell, p, q, np.ascontiguousarray(offsets, np.uint64), 0, want_counts)
        counts = np.zeros(len(p), np.uint32)
        _check(lib().cgrt_count_point_neighbors(self._h, _ptr(d), len(d), float(cell), _ptr(p), len(p), C.byref(q), _ptr(counts)))
        return self._point_list_full(d, cell, p, q, counts)

    def nearest_points(self, data, cell: float, points, k: int, radius2=None, max_dist2: float = float("inf"), skip_same_index: bool = False,
                       want_counts: bool = False):
        """The k nearest points of `data` of every query point within its squared radius: (n, k) POINT_NEIGHBOR_DTYPE records in order,
        unused entries {+inf, NO_PRIM}.  With want_counts=True returns (records, counts): counts (n,) uint32, the full numbers of
        neighbours."""
        if k < 1:
            raise ValueError("k must be at least 1")
        d, p, r, q = self._point_cloud_args(data, points, radius2, max_dist2, skip_same_index)
        out, counts = self._point_list_host(d, cell, p, q, None, k, want_counts)
        out = out.reshape(len(p), k)
        return (out, counts) if want_counts else out

    def list_point_neighbors_brute(self, data, points, radius2=None, max_dist2: float = float("inf"), skip_same_index: bool = False,
                                   offsets=None, k: int = 0):
        """cgrt_list_point_neighbors_brute: the list by testing every data point in turn, no grid (validation; the same bytes).  With
        neither offsets nor k the full list, as list_point_neighbors returns it: (offsets, records); with offsets ((n + 1,) slot
        boundaries) or k (k records per query): (records, counts)."""
        d, p, r, q = self._point_cloud_args(data, points, radius2, max_dist2, skip_same_index)
        if offsets is None and not k:
            _, c = self._point_list_host(d, 0.0, p, q, None, 1, brute=True)  # k = 1 only to obtain the counts
            return self._point_list_full(d, 0.0, p, q, c, brute=True)
        off = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
        out, counts = self._point_list_host(d, 0.0, p, q, off, k, brute=True)
        return (out.reshape(len(p), k) if off is None else out), counts

    def debug_point_neighbor_work(self, data, cell: float, points, radius2=None, max_dist2: float = float("inf"), skip_same_index: bool = False,
                                  k: int = 0) -> dict:
        """cgrt_debug_point_neighbor_work (a counted launch): {'cells', 'entries', 'foreign', 'd2_evals', 'linear', 'buckets_used'}, summed
        over the queries, of count_point_neighbors' search (k = 0) or of nearest_points' (k > 0: k records per query, no counts)."""
        d, p, r, q = self._point_cloud_args(data, points, radius2, max_dist2, skip_same_index)
        w = np.zeros(6, np.uint64)
        _check(lib().cgrt_debug_point_neighbor_work(self._h, _ptr(d), len(d), float(cell), _ptr(p), len(p), C.byref(q), int(k), _ptr(w)))
        return dict(zip(("cells", "entries", "foreign", "d2_evals", "linear", "buckets_used"), (int(x) for x in w)))

    def point_grid_workspace(self, m: int) -> int:
        """cgrt_point_grid_workspace: the bytes of device memory a grid over m points needs."""
        b = C.c_uint64(0)
        _check(lib().cgrt_point_grid_workspace(self._h, int(m), C.byref(b)))
        return int(b.value)

    def point_grid_build_device(self, d_data_ptr: int, m: int, cell: float, d_grid_ptr: int, grid_bytes: int, stream: int = 0) -> None:
        """cgrt_point_grid_build_device: enqueues the build of the grid over m points (3 floats each) at d_data_ptr into the caller's
        memory at d_grid_ptr (point_grid_workspace(m) bytes, 8-byte aligned) on the hipStream_t `stream`.  Raw integers."""
        _check(lib().cgrt_point_grid_build_device(self._h, _vp(d_data_ptr), int(m), float(cell), _vp(d_grid_ptr), int(grid_bytes), _vp(stream)))

    def count_point_neighbors_device(self, d_grid_ptr: int, grid_bytes: int, d_points_ptr: int, n: int, d_counts_ptr: int, d_radius2_ptr: int = 0,
                                     max_dist2: float = float("inf"), skip_same_index: bool = False, stream: int = 0) -> None:
        """cgrt_count_point_neighbors_device: n points (3 floats each) at d_points_ptr (and n squared radii at d_radius2_ptr, or 0) against
        the built grid at d_grid_ptr -> n uint32 counts at d_counts_ptr, enqueued on the hipStream_t `stream`.  Raw integers."""
        q = _point_query(d_radius2_ptr, max_dist2, skip_same_index)
        _check(lib().cgrt_count_point_neighbors_device(self._h, _vp(d_grid_ptr), int(grid_bytes), _vp(d_points_ptr), int(n), C.byref(q),
                                                       _vp(d_counts_ptr), _vp(stream)))

    def list_point_neighbors_device(self, d_grid_ptr: int, grid_bytes: int, d_points_ptr: int, n: int, d_out_ptr: int, capacity: int,
                                    d_offsets_ptr: int = 0, k: int = 0, d_counts_ptr: int = 0, d_radius2_ptr: int = 0,
                                    max_dist2: float = float("inf"), skip_same_index: bool = False, stream: int = 0) -> None:
        """cgrt_list_point_neighbors_device: slots from the n + 1 uint64 offsets at d_offsets_ptr, or of k records each; `capacity` records
        of 8 bytes at d_out_ptr, nothing beyond them is written whatever the offsets hold; d_counts_ptr (optional) receives the full
        counts.  Enqueued on `stream`.  Raw integers."""
        q = _point_query(d_radius2_ptr, max_dist2, skip_same_index)
        _check(lib().cgrt_list_point_neighbors_device(self._h, _vp(d_grid_ptr), int(grid_bytes), _vp(d_points_ptr), int(n), C.byref(q),
                                                      _vp(d_offsets_ptr), int(k), _vp(d_out_ptr), int(capacity), _vp(d_counts_ptr), _vp(stream)))

    def point_grid_tensor(self, data, cell: float, stream=None) -> "PointGrid":
        """The grid over data ((m, 3) float32 on cuda:<device>) with the wanted cell edge `cell` (about the query radius), built on
        `stream` (default: torch.cuda.current_stream()) into a tensor the returned PointGrid owns.  Only enqueues.  The grid holds the
        coordinates: `data` may be freed once the build has run."""
        import torch

        m = self._points_tensor(data)
        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        nbytes = self.point_grid_workspace(m)
        with torch.cuda.stream(stream):
            grid = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        self.point_grid_build_device(data.data_ptr() if m else 0, m, cell, grid.data_ptr(), nbytes, stream=stream.cuda_stream)
        return PointGrid(self, grid, m, float(cell))

    # ---- point-set frames (include/cgrt.h cgrt_point_frames*) ----
    def _point_frames_host(self, data, cell, points, k, radius2, max_dist2, skip_same_index, orient, want_neighbors, brute):
        if k < 1:
            raise ValueError("k must be at least 1")
        d, p, r, q = self._point_cloud_args(data, points, radius2, max_dist2, skip_same_index)
        o = None if orient is None else _f32(orient, (-1, 3))
        if o is not None and len(o) != len(p):
            raise ValueError("orient must hold one vector per point")
        n = len(p)
        frames = np.zeros(n, POINT_FRAME_DTYPE)
        nb = np.zeros((n, k), POINT_NEIGHBOR_DTYPE) if want_neighbors else None
        tail = (_ptr(p), n, C.byref(q), int(k), _ptr(o), _ptr(nb), _ptr(frames))
        if brute:
            _check(lib().cgrt_point_frames_brute(self._h, _ptr(d), len(d), *tail))
        else:
            _check(lib().cgrt_point_frames(self._h, _ptr(d), len(d), float(cell), *tail))
        return (frames, nb) if want_neighbors else frames

    def point_frames(self, data, cell: float, points, k: int, radius2=None, max_dist2: float = float("inf"), skip_same_index: bool = False,
                     orient=None, want_neighbors: bool = False):
        """cgrt_point_frames: for every query point ((n, 3) float32) the local PCA of its k nearest points of `data` ((m, 3) float32) within
        its squared radius -- (n,) POINT_FRAME_DTYPE records {centroid, used, normal, lambda0, tangent_u, lambda1, tangent_v, lambda2},
        defined to the last bit by include/cgrt.h "Point-set frames".  cell: the wanted cell edge of the call's own grid (no result
        depends on it).  orient ((n, 3) float32, optional): the normal is turned to the side of orient[i].  With want_neighbors=True
        returns (frames, neighbors (n, k) POINT_NEIGHBOR_DTYPE): the records nearest_points gives."""
        return self._point_frames_host(data, cell, points, k, radius2, max_dist2, skip_same_index, orient, want_neighbors, False)

    def point_frames_brute(self, data, points, k: int, radius2=None, max_dist2: float = float("inf"), skip_same_index: bool = False,
                           orient=None, want_neighbors: bool = False):
        """cgrt_point_frames_brute: point_frames by testing every data point in turn, no grid (validation; the same bytes)."""
        return self._point_frames_host(data, 0.0, points, k, radius2, max_dist2, skip_same_index, orient, want_neighbors, True)

    def point_frames_device(self, d_grid_ptr: int, grid_bytes: int, d_data_ptr: int, m: int, d_points_ptr: int, n: int, k: int,
                            d_neighbors_ptr: int, d_frames_ptr: int, d_orient_ptr: int = 0, d_radius2_ptr: int = 0,
                            max_dist2: float = float("inf"), skip_same_index: bool = False, stream: int = 0) -> None:
        """cgrt_point_frames_device: n points at d_points_ptr against the built grid at d_grid_ptr and the m points at d_data_ptr it was
        built on -> n * k neighbour records of 8 bytes at d_neighbors_ptr and n frame records of 64 bytes at d_frames_ptr (16-byte
        aligned), enqueued on the hipStream_t `stream`.  Raw integers."""
        q = _point_query(d_radius2_ptr, max_dist2, skip_same_index)
        _check(lib().cgrt_point_frames_device(self._h, _vp(d_grid_ptr), int(grid_bytes), _vp(d_data_ptr), int(m), _vp(d_points_ptr), int(n),
                                              C.byref(q), int(k), _vp(d_orient_ptr), _vp(d_neighbors_ptr), _vp(d_frames_ptr), _vp(stream)))

    # ---- iso-surfaces (include/cgrt.h cgrt_isosurface*) ----
    def isosurface(self, values, origin, spacing, iso: float = 0.0, inside_above: bool = False):
        """cgrt_isosurface: the triangle mesh of the level `iso` of values ((nz, ny, nx) float32 on the grid origin + i * spacing), by
        marching tetrahedra, in the order include/cgrt.h defines.  Returns (verts (nv, 3) float32, tris (nt, 3) uint32).  Inside is
        value < iso (inside_above: value > iso); normals point from inside to outside."""
        v = np.ascontiguousarray(np.asarray(values, np.float32))
        if v.ndim != 3:
            raise ValueError("values must be shaped (nz, ny, nx)")
        g, prm = _sdf_grid_struct(origin, spacing, v.shape[::-1]), _iso_params(iso, inside_above)
        counts = np.zeros(2, np.uint64)
        _check(lib().cgrt_isosurface(self._h, C.byref(g), _ptr(v), C.byref(prm), None, 0, None, 0, _ptr(counts)))
        verts, tris = np.zeros((int(counts[0]), 3), np.float32), np.zeros((int(counts[1]), 3), np.uint32)
        if len(verts) or len(tris):
            _check(lib().cgrt_isosurface(self._h, C.byref(g), _ptr(v), C.byref(prm), _ptr(verts) if len(verts) else None, len(verts),
                                         _ptr(tris) if len(tris) else None, len(tris), _ptr(counts)))
        return verts, tris

    def debug_isosurface_work(self, values, origin, spacing, iso: float = 0.0, inside_above: bool = False):
        """cgrt_debug_isosurface_work: (cells that emit a triangle, tetrahedra that emit one, vertices, triangles) of isosurface (a
        counted run)."""
        v = np.ascontiguousarray(np.asarray(values, np.float32))
        if v.ndim != 3:
            raise ValueError("values must be shaped (nz, ny, nx)")
        g, prm = _sdf_grid_struct(origin, spacing, v.shape[::-1]), _iso_params(iso, inside_above)
        w = np.zeros(4, np.uint64)
        _check(lib().cgrt_debug_isosurface_work(self._h, C.byref(g), _ptr(v), C.byref(prm), _ptr(w)))
        return tuple(int(x) for x in w)

    def isosurface_workspace(self, dims) -> int:
        """cgrt_isosurface_workspace: the bytes of device memory an isosurface call on a grid of dims = (nx, ny, nz) needs."""
        g = _sdf_grid_struct((0, 0, 0), (1, 1, 1), dims)
        b = C.c_uint64(0)
        _check(lib().cgrt_isosurface_workspace(self._h, C.byref(g), C.byref(b)))
        return int(b.value)

    def isosurface_count_device(self, origin, spacing, dims, d_values_ptr: int, d_counts2_ptr: int, d_workspace_ptr: int, workspace_bytes: int,
                                iso: float = 0.0, inside_above: bool = False, stream: int = 0) -> None:
        """cgrt_isosurface_count_device: nx * ny * nz float32 at d_values_ptr -> {vertices, triangles} as two uint64 at d_counts2_ptr
        (8-byte aligned), with the caller's workspace; enqueued on the hipStream_t `stream`.  Raw integers."""
        g, prm = _sdf_grid_struct(origin, spacing, dims), _iso_params(iso, inside_above)
        _check(lib().cgrt_isosurface_count_device(self._h, C.byref(g), _vp(d_values_ptr), C.byref(prm), _vp(d_counts2_ptr), _vp(d_workspace_ptr),
                                                  int(workspace_bytes), _vp(stream)))

    def isosurface_device(self, origin, spacing, dims, d_values_ptr: int, d_verts_ptr: int, vert_capacity: int, d_tris_ptr: int,
                          tri_capacity: int, d_counts2_ptr: int, d_workspace_ptr: int, workspace_bytes: int, iso: float = 0.0,
                          inside_above: bool = False, stream: int = 0) -> None:
        """cgrt_isosurface_device: the vertices below vert_capacity (3 floats each) to d_verts_ptr, the triangles below tri_capacity (3
        uint32 each) to d_tris_ptr, the full counts to d_counts2_ptr; nothing beyond the capacities is written.  Enqueued on `stream`.
        Raw integers."""
        g, prm = _sdf_grid_struct(origin, spacing, dims), _iso_params(iso, inside_above)
        _check(lib().cgrt_isosurface_device(self._h, C.byref(g), _vp(d_values_ptr), C.byref(prm), _vp(d_verts_ptr), int(vert_capacity),
                                            _vp(d_tris_ptr), int(tri_capacity), _vp(d_counts2_ptr), _vp(d_workspace_ptr), int(workspace_bytes),
                                            _vp(stream)))

    def isosurface_tensor(self, values, origin, spacing, iso: float = 0.0, inside_above: bool = False, capacity=None, workspace=None,
                          stream=None):
        """isosurface on torch tensors: values (nz, ny, nx) float32 on cuda:<device> -> {'verts': (nv, 3) float32, 'tris': (nt, 3) int32
        (the uint32 indices, viewed), 'counts': (2,) int64 {vertices, triangles}, the full counts}.  capacity None: counts, reads the two
        counts (this blocks), allocates exactly and lists.  capacity = (v, t): lists in one pass into tensors of that size and returns
        them cut to the counts (the cut reads the counts: it blocks too; records beyond a capacity are dropped, the counts say so).
        workspace: None (allocated here), or a torch.uint8 tensor of at least isosurface_workspace(dims) bytes, 8-byte aligned.  Ordered
        on `stream` (default: torch.cuda.current_stream())."""
        import torch

        self._device_tensor(values, "values", (torch.float32,))
        if values.dim() != 3:
            raise ValueError("values must be shaped (nz, ny, nx)")
        nz, ny, nx = (int(x) for x in values.shape)
        dims = (nx, ny, nz)
        nbytes = self.isosurface_workspace(dims)
        if workspace is not None:
            self._device_tensor(workspace, "workspace", (torch.uint8,))
            if workspace.numel() < nbytes or workspace.data_ptr() % 8:
                raise ValueError(f"workspace must hold {nbytes} bytes and be 8-byte aligned")
        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        with torch.cuda.stream(stream):
            if workspace is None:
                workspace = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            counts = torch.empty((2,), dtype=torch.int64, device=dev)
            if capacity is None:
                self.isosurface_count_device(origin, spacing, dims, values.data_ptr(), counts.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                             iso=iso, inside_above=inside_above, stream=stream.cuda_stream)
                capacity = tuple(int(x) for x in counts.cpu())
            vcap, tcap = (int(x) for x in capacity)
            verts = torch.empty((vcap, 3), dtype=torch.float32, device=dev)
            tris = torch.empty((tcap, 3), dtype=torch.int32, device=dev)
            self.isosurface_device(origin, spacing, dims, values.data_ptr(), verts.data_ptr() if vcap else 0, vcap, tris.data_ptr() if tcap else 0,
                                   tcap, counts.data_ptr(), workspace.data_ptr(), workspace.numel(), iso=iso, inside_above=inside_above,
                                   stream=stream.cuda_stream)
            nv, nt = (int(x) for x in counts.cpu())
            return {"verts": verts[: min(nv, vcap)], "tris": tris[: min(nt, tcap)], "counts": counts}

    def sdf_isosurface_tensor(self, origin, spacing, dims, offset: float = 0.0, **sdf_kw):
        """The offset surface of the scene: sdf_grid_tensor(origin, spacing, dims, **sdf_kw)'s signed distances, extracted at
        iso = offset (isosurface_tensor's result plus 'values', the (nz, ny, nx) grid)."""
        values = self.sdf_grid_tensor(origin, spacing, dims, want="sdf", **sdf_kw)
        res = self.isosurface_tensor(values, origin, spacing, iso=offset, stream=sdf_kw.get("stream"))
        res["values"] = values
        return res

    def winding_isosurface_tensor(self, origin, spacing, dims, level: float = 0.5, beta: float = 2.0):
        """A watertight stand-in for an open mesh: the `level` surface of |w|, w the winding numbers of winding_grid_tensor, inside where
        |w| > level (isosurface_tensor's result plus 'values', the (nz, ny, nx) grid of |w|).  Closed as long as no cell on the grid's
        boundary is crossed: choose a margin over which |w| has fallen below the level."""
        values = self.winding_grid_tensor(origin, spacing, dims, beta=beta, want="w").abs()
        res = self.isosurface_tensor(values, origin, spacing, iso=level, inside_above=True)
        res["values"] = values
        return res

    # ---- grid fields (include/cgrt.h "Grid fields") ----
    _GRID_WANT = ("value", "gradient", "inside")

    def _grid_want(self, want):
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or len(set(want)) != len(want) or any(w not in self._GRID_WANT for w in want):
            raise ValueError(f"want must name some of {self._GRID_WANT}, each once")
        return want

    @staticmethod
    def _grid_values(values):
        v = np.ascontiguousarray(np.asarray(values, np.float32))
        if v.ndim != 3:
            raise ValueError("values must be shaped (nz, ny, nx)")
        return v

    def sample_grid(self, values, origin, spacing, points, outside=float("nan"), clamp: bool = False, want=("value", "gradient", "inside")):
        """cgrt_sample_grid: the trilinear sample of values ((nz, ny, nx) float32 on the grid origin + i * spacing) at every point ((n, 3)
        float32), as include/cgrt.h defines it to the last bit.  Returns a dict of the arrays named by `want`: 'value' (n,) float32,
        'gradient' (n, 3) float32 (the derivative of the trilinear polynomial), 'inside' (n,) bool.  A point outside the grid gets
        (`outside`, 0, False); clamp: the nearest point of the grid's box is sampled instead."""
        want = self._grid_want(want)
        v, p = self._grid_values(values), _f32(points, (-1, 3))
        g, prm = _sdf_grid_struct(origin, spacing, v.shape[::-1]), _field_params(outside, clamp)
        res = {"value": np.zeros(len(p), np.float32), "gradient": np.zeros((len(p), 3), np.float32), "inside": np.zeros(len(p), np.uint8)}
        res = {w: res[w] for w in want}
        _check(lib().cgrt_sample_grid(self._h, C.byref(g), _ptr(v), _ptr(p), len(p), C.byref(prm), _ptr(res.get("value")),
                                      _ptr(res.get("gradient")), _ptr(res.get("inside"))))
        if "inside" in res:
            res["inside"] = res["inside"].view(np.bool_)
        return res

    def sample_grid_device(self, origin, spacing, dims, d_values_ptr: int, d_points_ptr: int, n: int, d_value_ptr: int, d_gradient_ptr: int,
                           d_inside_ptr: int, outside=float("nan"), clamp: bool = False, stream: int = 0) -> None:
        """cgrt_sample_grid_device: nx * ny * nz float32 at d_values_ptr and n points (3 floats each) at d_points_ptr -> n float32 at
        d_value_ptr, 3 n float32 at d_gradient_ptr, n bytes at d_inside_ptr (0: not wanted), enqueued on the hipStream_t `stream`.  Raw
        integers."""
        g, prm = _sdf_grid_struct(origin, spacing, dims), _field_params(outside, clamp)
        _check(lib().cgrt_sample_grid_device(self._h, C.byref(g), _vp(d_values_ptr), _vp(d_points_ptr), int(n), C.byref(prm), _vp(d_value_ptr),
                                             _vp(d_gradient_ptr), _vp(d_inside_ptr), _vp(stream)))

    def _grid_values_tensor(self, values):
        import torch

        self._device_tensor(values, "values", (torch.float32,))
        if values.dim() != 3:
            raise ValueError("values must be shaped (nz, ny, nx)")
        nz, ny, nx = (int(x) for x in values.shape)
        return (nx, ny, nz)

    def sample_grid_tensor(self, values, origin, spacing, points, outside=float("nan"), clamp: bool = False,
                           want=("value", "gradient", "inside"), out=None, stream=None, reproducible: bool = False):
        """sample_grid on torch tensors: values (nz, ny, nx) and points (n, 3), contiguous float32 on cuda:<device> -> a dict of the
        tensors named by `want` ('value' (n,) float32, 'gradient' (n, 3) float32, 'inside' (n,) torch.bool), written into `out` (a dict
        by name; inside may also be torch.uint8) or new ones, enqueued on `stream` (default: torch.cuda.current_stream()).
        When values or points requires grad (and grad mode is on) the call is recorded for autograd (out= is then refused): 'value' and
        'gradient' are differentiable with respect to values, through one sample_grid_grad_tensor call on the current stream of the
        backward; 'value' is differentiable with respect to points, as grad_value[:, None] * gradient (the sampler's own gradient
        output, computed internally when it is not in want); the 'gradient' OUTPUT is treated as constant in the points (no second
        derivatives); 'inside' is not differentiable.  The backward runs once (no double backward) and, since the adds into the volume
        are float atomics, raises under torch.use_deterministic_algorithms(True) (warns in warn-only mode) when values needs a gradient
        -- unless reproducible: then the recorded backward is the bitwise-reproducible entry (sample_grid_grad_tensor(...,
        reproducible=True); include/cgrt.h cgrt_sample_grid_grad_repro*), which runs in deterministic mode and gives the same bytes in
        every run.  With nothing requiring grad the call and its bytes are the plain ones, whatever the keyword."""
        import torch

        want = self._grid_want(want)
        dims = self._grid_values_tensor(values)
        self._device_tensor(points, "points", (torch.float32,))
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must be shaped (n, 3)")
        if (values.requires_grad or points.requires_grad) and torch.is_grad_enabled():  # recorded: the outputs carry a grad_fn
            if out is not None:
                raise ValueError("out= cannot be combined with values or points that require grad")
            inner = want if "gradient" in want else want + ("gradient",)
            res = _grid_function().apply(
                values, points,
                lambda v, p: self.sample_grid_tensor(v, origin, spacing, p, outside=outside, clamp=clamp, want=inner, stream=stream),
                lambda p, gv, gg: self.sample_grid_grad_tensor(origin, spacing, dims, p, gv, gg, clamp=clamp, reproducible=bool(reproducible)),
                want, bool(reproducible))
            return dict(zip(want, res))
        n = int(points.shape[0])
        shapes = {"value": ((n,), (torch.float32,)), "gradient": ((n, 3), (torch.float32,)), "inside": ((n,), (torch.bool, torch.uint8))}
        if out is not None and (not isinstance(out, dict) or set(out) - set(want)):
            raise ValueError("out must be a dict of tensors by the names in want")
        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        res = {}
        with torch.cuda.stream(stream):
            for w in want:
                shape, dtypes = shapes[w]
                if out is not None and w in out:
                    t = out[w]
                    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype not in dtypes:
                        raise ValueError(f"out[{w!r}] must be a torch tensor of shape {shape} and one of {dtypes}")
                    if t.device.type != "cuda" or t.device.index != self.device or not t.is_contiguous() or (w != "inside" and t.data_ptr() % 4):
                        raise ValueError(f"out[{w!r}] must be contiguous (4-byte aligned) on cuda:{self.device}")
                else:
                    t = torch.empty(shape, dtype=dtypes[0], device=dev)
                res[w] = t
        if n:  # (an empty tensor has no address to pass: the call would touch nothing anyway)
            ptr = {w: (res[w].data_ptr() if w in res else 0) for w in self._GRID_WANT}
            self.sample_grid_device(origin, spacing, dims, values.data_ptr(), points.data_ptr(), n, ptr["value"], ptr["gradient"], ptr["inside"],
                                    outside=outside, clamp=clamp, stream=stream.cuda_stream)
        return res

    # ---- grid fields, the sampler's adjoint (include/cgrt.h cgrt_sample_grid_grad*) ----
    def sample_grid_grad_repro_workspace(self, origin, spacing, dims) -> int:
        """cgrt_sample_grid_grad_repro_workspace: the bytes of device memory a reproducible adjoint call on this grid needs
        (12 * nx * ny * nz)."""
        b = C.c_uint64(0)
        g = _sdf_grid_struct(origin, spacing, dims)
        _check(lib().cgrt_sample_grid_grad_repro_workspace(self._h, C.byref(g), C.byref(b)))
        return int(b.value)

    def sample_grid_grad(self, origin, spacing, dims, points, grad_value=None, grad_gradient=None, grad_values=None,
                         clamp: bool = False, reproducible: bool = False) -> np.ndarray:
        """cgrt_sample_grid_grad, the adjoint of sample_grid with respect to values: grad_value ((n,) float32) and grad_gradient ((n, 3)
        float32) are the gradients with respect to sample_grid's value and gradient at points ((n, 3) float32); either may be None, not
        both.  Every inside point's eight contributions are ADDED into grad_values -- a writeable C-contiguous (nz, ny, nx) float32 array
        that is accumulated into in place, or None for a new zero array -- which is returned.  dims = (nx, ny, nz).  The order of the
        additions into one element is unspecified (last bits may differ from run to run); each contribution is defined to the last bit
        (include/cgrt.h).  With grad_value alone this is the trilinear splat of the weights grad_value.  reproducible: then
        cgrt_sample_grid_grad_repro, whose result is defined to the last bit (include/cgrt.h)."""
        p = _f32(points, (-1, 3))
        gv = None if grad_value is None else _f32(grad_value, (-1,))
        gg = None if grad_gradient is None else _f32(grad_gradient, (-1, 3))
        if (gv is not None and len(gv) != len(p)) or (gg is not None and len(gg) != len(p)):
            raise ValueError(f"grad_value and grad_gradient must have one row per point: {len(p)}")
        nx, ny, nz = (int(x) for x in dims)
        if grad_values is None:
            grad_values = np.zeros((nz, ny, nx), np.float32)
        elif not (isinstance(grad_values, np.ndarray) and grad_values.dtype == np.float32 and grad_values.flags.c_contiguous
                  and grad_values.flags.writeable and grad_values.shape == (nz, ny, nx)):
            raise ValueError(f"grad_values must be a writeable C-contiguous float32 array of shape ({nz}, {ny}, {nx})")
        g, prm = _sdf_grid_struct(origin, spacing, (nx, ny, nz)), _field_params(clamp=clamp)
        f = lib().cgrt_sample_grid_grad_repro if reproducible else lib().cgrt_sample_grid_grad
        _check(f(self._h, C.byref(g), _ptr(p), len(p), C.byref(prm), _ptr(gv), _ptr(gg), _ptr(grad_values)))
        return grad_values

    def sample_grid_grad_device(self, origin, spacing, dims, d_points_ptr: int, n: int, d_grad_value_ptr: int, d_grad_gradient_ptr: int,
                                d_grad_values_ptr: int, clamp: bool = False, stream: int = 0, reproducible: bool = False,
                                d_workspace_ptr: int = 0, workspace_bytes: int = 0) -> None:
        """cgrt_sample_grid_grad_device: n points (3 floats each) at d_points_ptr, n float32 at d_grad_value_ptr and 3 n float32 at
        d_grad_gradient_ptr (0: not given; not both) are added, weighted, into the nx * ny * nz float32 at d_grad_values_ptr; enqueued on
        the hipStream_t `stream`.  Raw integers.  reproducible: cgrt_sample_grid_grad_repro_device with the caller's workspace
        (sample_grid_grad_repro_workspace(origin, spacing, dims) bytes of device memory, 8-byte aligned, this call's alone)."""
        g, prm = _sdf_grid_struct(origin, spacing, dims), _field_params(clamp=clamp)
        if reproducible:
            _check(lib().cgrt_sample_grid_grad_repro_device(self._h, C.byref(g), _vp(d_points_ptr), int(n), C.byref(prm),
                                                            _vp(d_grad_value_ptr), _vp(d_grad_gradient_ptr), _vp(d_grad_values_ptr),
                                                            _vp(d_workspace_ptr), int(workspace_bytes), _vp(stream)))
            return
        _check(lib().cgrt_sample_grid_grad_device(self._h, C.byref(g), _vp(d_points_ptr), int(n), C.byref(prm), _vp(d_grad_value_ptr),
                                                  _vp(d_grad_gradient_ptr), _vp(d_grad_values_ptr), _vp(stream)))

    def sample_grid_grad_tensor(self, origin, spacing, dims, points, grad_value=None, grad_gradient=None, out=None, clamp: bool = False,
                                stream=None, reproducible: bool = False):
        """sample_grid_grad on torch tensors: points (n, 3), grad_value (n,) and grad_gradient (n, 3) (either may be None, not both),
        contiguous float32 on cuda:<device>; added into `out` ((nz, ny, nx) float32 on the device, or None for a new zero tensor), which
        is returned.  dims = (nx, ny, nz).  Enqueued on `stream` (default: torch.cuda.current_stream()).  sample_grid_tensor calls this in
        its backward when values requires grad.  reproducible: the bitwise-reproducible entry, its workspace (12 bytes per grid element)
        allocated here on the call's stream."""
        import torch

        self._device_tensor(points, "points", (torch.float32,))
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must be shaped (n, 3)")
        n = int(points.shape[0])
        if grad_value is None and grad_gradient is None:
            raise ValueError("one of grad_value and grad_gradient must be given")
        if grad_value is not None:
            self._device_tensor(grad_value, "grad_value", (torch.float32,), (n,))
        if grad_gradient is not None:
            self._device_tensor(grad_gradient, "grad_gradient", (torch.float32,), (n, 3))
        nx, ny, nz = (int(x) for x in dims)
        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev)
        else:
            self._device_tensor(out, "out", (torch.float32,), (nz, ny, nx))
        if n:  # (an empty tensor has no address to pass: the call would touch nothing anyway)
            ws, kw = self._repro_workspace_tensor(
                self.sample_grid_grad_repro_workspace(origin, spacing, (nx, ny, nz)) if reproducible else None, stream)
            self.sample_grid_grad_device(origin, spacing, (nx, ny, nz), points.data_ptr(), n,
                                         0 if grad_value is None else grad_value.data_ptr(),
                                         0 if grad_gradient is None else grad_gradient.data_ptr(), out.data_ptr(), clamp=clamp,
                                         stream=stream.cuda_stream, **kw)
            del ws  # (held until the passes were enqueued: the allocator hands the block only to later work of the same stream)
        return out

    def splat_grid_tensor(self, points, weights, origin, spacing, dims, out=None, clamp: bool = False, stream=None,
                          reproducible: bool = False):
        """Points -> volume: the trilinear splat of weights ((n,) float32) at points ((n, 3) float32) into the grid origin + i * spacing
        of dims = (nx, ny, nz) -- sample_grid_grad_tensor with grad_value = weights and no grad_gradient.  Added into `out` ((nz, ny, nx)
        float32, or None for a new zero tensor), which is returned: a density estimate or a particle-to-grid deposit that
        isosurface_tensor, sample_grid_tensor and march_grid_tensor read as it is.  Points outside the grid deposit nothing (clamp: they
        deposit at the nearest point of its box).  reproducible: the bitwise-reproducible entry, a density defined to the last bit."""
        if weights is None:
            raise ValueError("weights must be a torch tensor of shape (n,)")
        return self.sample_grid_grad_tensor(origin, spacing, dims, points, grad_value=weights, out=out, clamp=clamp, stream=stream,
                                            reproducible=reproducible)

    def march_grid(self, values, origin, spacing, rays, iso: float = 0.0, relax: float = 1.0, min_step: float = 1e-4, hit_eps: float = 1e-4,
                   max_steps: int = 256, refine: int = 0, inside_above: bool = False) -> np.ndarray:
        """cgrt_march_grid: every ray (a RAY_DTYPE array or (n, 7) float32; the direction as given) marched through values ((nz, ny, nx)
        float32 on the grid origin + i * spacing) to its first sample with value - iso <= hit_eps (inside_above: iso - value), as
        include/cgrt.h defines it to the last bit.  relax = 1: sphere tracing of a signed distance field; relax = 0: steps of min_step;
        refine: bisection steps of a hit.  Returns an (n,) GRID_HIT_DTYPE array {t, value, steps, status (MARCH_*), gradient}."""
        v, r = self._grid_values(values), _as_ray_array(rays)
        g, prm = _sdf_grid_struct(origin, spacing, v.shape[::-1]), _march_params(iso, relax, min_step, hit_eps, max_steps, refine, inside_above)
        hits = np.zeros(len(r), GRID_HIT_DTYPE)
        _check(lib().cgrt_march_grid(self._h, C.byref(g), _ptr(v), _ptr(r), len(r), C.byref(prm), _ptr(hits)))
        return hits

    def march_grid_device(self, origin, spacing, dims, d_values_ptr: int, d_rays_ptr: int, n: int, d_hits_ptr: int, iso: float = 0.0,
                          relax: float = 1.0, min_step: float = 1e-4, hit_eps: float = 1e-4, max_steps: int = 256, refine: int = 0,
                          inside_above: bool = False, stream: int = 0) -> None:
        """cgrt_march_grid_device: nx * ny * nz float32 at d_values_ptr and n rays (7 floats each) at d_rays_ptr -> n records of 32
        bytes (CgrtGridHit) at d_hits_ptr, enqueued on the hipStream_t `stream`.  Raw integers."""
        g, prm = _sdf_grid_struct(origin, spacing, dims), _march_params(iso, relax, min_step, hit_eps, max_steps, refine, inside_above)
        _check(lib().cgrt_march_grid_device(self._h, C.byref(g), _vp(d_values_ptr), _vp(d_rays_ptr), int(n), C.byref(prm), _vp(d_hits_ptr),
                                            _vp(stream)))

    def march_grid_tensor(self, values, origin, spacing, rays, out=None, stream=None, **march):
        """march_grid on torch tensors: values (nz, ny, nx) and rays (n, 7), contiguous float32 on cuda:<device>; `march`: march_grid's
        parameters.  Returns views over ONE (n, 8) float32 tensor of records (`out`, or a new one; also returned as 'records'): 't' (n,)
        float32, 'value' (n,) float32, 'steps' (n,) int32, 'status' (n,) int32, 'gradient' (n, 3) float32.  Enqueued on `stream`
        (default: torch.cuda.current_stream())."""
        import torch

        dims = self._grid_values_tensor(values)
        self._device_tensor(rays, "rays", (torch.float32,))
        if rays.dim() != 2 or rays.shape[1] != 7:
            raise ValueError("rays must be shaped (n, 7)")
        n = int(rays.shape[0])
        if out is not None:
            self._device_tensor(out, "out", (torch.float32,), (n, 8))
        rec = self._tensor_call(out, (n, 8), torch.float32, stream,
                                lambda o, s: self.march_grid_device(origin, spacing, dims, values.data_ptr(), rays.data_ptr(), n, o.data_ptr(),
                                                                    stream=s, **march))
        words = rec.view(torch.int32)
        return {"records": rec, "t": rec[:, 0], "value": rec[:, 1], "steps": words[:, 2], "status": words[:, 3], "gradient": rec[:, 4:7]}

    def debug_march_work(self, values, origin, spacing, rays, iso: float = 0.0, relax: float = 1.0, min_step: float = 1e-4,
                         hit_eps: float = 1e-4, max_steps: int = 256, refine: int = 0, inside_above: bool = False):
        """cgrt_debug_march_work: (rays that entered the grid's box, main-loop samples, refinement samples) of march_grid, summed over
        the rays (a separate counting launch)."""
        v, r = self._grid_values(values), _as_ray_array(rays)
        g, prm = _sdf_grid_struct(origin, spacing, v.shape[::-1]), _march_params(iso, relax, min_step, hit_eps, max_steps, refine, inside_above)
        w = np.zeros(3, np.uint64)
        _check(lib().cgrt_debug_march_work(self._h, C.byref(g), _ptr(v), _ptr(r), len(r), C.byref(prm), _ptr(w)))
        return tuple(int(x) for x in w)

    def _surface_frames_tensor(self, raycams, cams, W, H, depth, prim_id, attr, want_bary, chw, out, stream, reproducible=False):
        import torch

        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        if raycams:
            a = raycam_array(cams)
        else:
            if isinstance(cams, Camera):
                cams = [cams]
            elif isinstance(cams, np.ndarray) and cams.ndim == 1:
                cams = cams.reshape(1, -1)
            a = camera_array(cams)
        B = len(a)
        if attr is None and not want_bary:
            raise ValueError("nothing requested: pass attr, or want_bary=True")
        if not isinstance(depth, torch.Tensor) or tuple(depth.shape) not in ((B, H, W),) + (((H, W),) if B == 1 else ()):
            raise ValueError(f"depth must be a torch tensor of shape {(B, H, W)}" + (f" or {(H, W)}" if B == 1 else ""))
        lead = tuple(depth.shape[:-2])
        self._device_tensor(depth, "depth", (torch.float32,))
        self._device_tensor(prim_id, "prim_id", (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ()), depth.shape)
        out = {} if out is None else out
        if not isinstance(out, dict) or any(k not in ("bary", "attr") for k in out):
            raise ValueError("out must be a dict with the keys 'bary' and / or 'attr'")
        want = {}
        if want_bary:
            want["bary"] = lead + ((3, H, W) if chw else (H, W, 3))
        if attr is not None:
            attr = self._attr_tensor(attr)
            want["attr"] = lead + ((attr.shape[1], H, W) if chw else (H, W, attr.shape[1]))
        for k, t in out.items():
            if k not in want:
                raise ValueError(f"out[{k!r}] given, but that output is not requested")
            self._device_tensor(t, f"out[{k!r}]", (torch.float32,), want[k])
        if attr is not None and attr.requires_grad and torch.is_grad_enabled():  # recorded: 'attr' carries a grad_fn (_surface_frames_grad_tensor)
            if "attr" in out:
                raise ValueError("out['attr'] cannot be combined with an attr that requires grad")
            keys = list(want)

            def forward(table):
                res = self._surface_frames_tensor(raycams, cams, W, H, depth, prim_id, table, want_bary, chw, out, stream)
                return tuple(res[k] for k in keys)

            got = _surface_function().apply(
                attr, forward, lambda g: self._surface_frames_grad_tensor(raycams, cams, W, H, depth, prim_id, g, chw, None, None, reproducible),
                keys.index("attr"), bool(reproducible))
            return dict(zip(keys, got))
        dev, stream = self._torch_stream(stream)
        _check_one_hip_runtime()
        with torch.cuda.stream(stream):
            res = {k: out[k] if k in out else torch.empty(shape, dtype=torch.float32, device=dev) for k, shape in want.items()}
        self.surface_views_device(a, W, H, depth.data_ptr(), prim_id.data_ptr(), d_bary_ptr=res["bary"].data_ptr() if "bary" in res else 0,
                                  d_attr_ptr=0 if attr is None else attr.data_ptr(), channels=0 if attr is None else attr.shape[1],
                                  d_out_ptr=res["attr"].data_ptr() if "attr" in res else 0, chw=chw, stream=stream.cuda_stream, raycams=raycams)
        return res

    def _surface_frames_grad_tensor(self, raycams, cams, W, H, depth, prim_id, grad_out, chw, grad_attr, stream, reproducible=False):
        import torch

        if self.device < 0:
            raise ValueError("the scene has no device (created host-only)")
        if raycams:
            a = raycam_array(cams)
        else:
            if isinstance(cams, Camera):
                cams = [cams]
            elif isinstance(cams, np.ndarray) and cams.ndim == 1:
                cams = cams.reshape(1, -1)
            a = camera_array(cams)
        B = len(a)
        if not isinstance(depth, torch.Tensor) or tuple(depth.shape) not in ((B, H, W),) + (((H, W),) if B == 1 else ()):
            raise ValueError(f"depth must be a torch tensor of shape {(B, H, W)}" + (f" or {(H, W)}" if B == 1 else ""))
        lead = tuple(depth.shape[:-2])
        self._device_tensor(depth, "depth", (torch.float32,))
        self._device_tensor(prim_id, "prim_id", (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ()), depth.shape)
        if not isinstance(grad_out, torch.Tensor) or grad_out.dim() != len(lead) + 3:
            raise ValueError("grad_out must be a torch tensor in the layout of the forward's 'attr' output")
        ch = grad_out.shape[-3] if chw else grad_out.shape[-1]
        if not 1 <= ch <= 256:
            raise ValueError("grad_out must have 1..256 channels")
        self._device_tensor(grad_out, "grad_out", (torch.float32,), lead + ((ch, H, W) if chw else (H, W, ch)))
        grad_attr, stream = self._grad_attr_tensor(grad_attr, ch, stream)
        ws, kw = self._repro_workspace_tensor(self.surface_grad_repro_workspace(ch) if reproducible else None, stream)
        self.surface_views_grad_device(a, W, H, depth.data_ptr(), prim_id.data_ptr(), grad_out.data_ptr(), ch, grad_attr.data_ptr(), chw=chw,
                                       stream=stream.cuda_stream, raycams=raycams, **kw)
        del ws  # (held until here: the passes are enqueued)
        return grad_attr

    def surface_views_grad_tensor(self, cams, W: int, H: int, depth, prim_id, grad_out, chw: bool = False, grad_attr=None, stream=None,
                                  reproducible: bool = False):
        """The adjoint of surface_views_tensor's 'attr' output with respect to the table: cams, W, H, depth and prim_id as the forward
        took them, grad_out (B, H, W, C) float32 -- (B, C, H, W) with chw; (H, W, C) / (C, H, W) for one camera's (H, W) planes.  Added
        into grad_attr ((nverts, C) float32 on the device, or None for a new zero tensor), which is returned: a running gradient over
        several frames is one tensor passed again and again.  Enqueued on `stream` (default: torch.cuda.current_stream()).  The order of
        the additions into one element is unspecified, unless reproducible: then the bitwise-reproducible entry (include/cgrt.h), its
        workspace allocated here on the call's stream.  surface_views_tensor calls this in its backward when attr requires grad."""
        return self._surface_frames_grad_tensor(False, cams, W, H, depth, prim_id, grad_out, chw, grad_attr, stream, reproducible)

    def surface_raycams_grad_tensor(self, cams, W: int, H: int, depth, prim_id, grad_out, chw: bool = False, grad_attr=None, stream=None,
                                    reproducible: bool = False):
        """surface_views_grad_tensor for ray cameras."""
        return self._surface_frames_grad_tensor(True, cams, W, H, depth, prim_id, grad_out, chw, grad_attr, stream, reproducible)

    def surface_views_tensor(self, cams, W: int, H: int, depth, prim_id, attr=None, want_bary: bool = True, chw: bool = False, out=None,
                             stream=None, reproducible: bool = False):
        """The surface attributes of whole frames from their geometry planes: cams (B Trackball cameras, or one) and the `depth` (float32)
        and `prim_id` (int32) planes of render_views_aov_tensor / render_aov_tensor, (B, H, W) -- or (H, W) for one camera; for the planes
        of an aa frame pass 2W, 2H.  Returns a dict: 'bary' (B, H, W, 3) when want_bary, 'attr' (B, H, W, C) when attr ((nverts, C)
        float32 on the device) is given; (B, 3, H, W) / (B, C, H, W) with chw.  out: dict of caller's tensors for some or all of them.
        Enqueued on `stream` (default: torch.cuda.current_stream()); nothing is traced.  reproducible: when attr requires grad, the
        recorded backward is the bitwise-reproducible entry (it runs under torch.use_deterministic_algorithms(True))."""
        return self._surface_frames_tensor(False, cams, W, H, depth, prim_id, attr, want_bary, chw, out, stream, reproducible)

    def surface_raycams_tensor(self, cams, W: int, H: int, depth, prim_id, attr=None, want_bary: bool = True, chw: bool = False, out=None,
                               stream=None, reproducible: bool = False):
        """surface_views_tensor for ray cameras (the planes of render_raycams_tensor(aovs=...))."""
        return self._surface_frames_tensor(True, cams, W, H, depth, prim_id, attr, want_bary, chw, out, stream, reproducible)

    def generate_rays(self, cam, W: int, H: int, rect=None) -> np.ndarray:
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
        rays = np.zeros((x1 - x0) * (y1 - y0), RAY_DTYPE)
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(lib().cgrt_generate_rays(self._h, C.byref(c), W, H, x0, y0, x1, y1, _ptr(rays)))
        return rays

    def count_primary(self, cam, W, H, rect=None, rank=0, nranks=1) -> dict:
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        out = Counters()
        _check(lib().cgrt_count_primary(self._h, C.byref(c), W, H, x0, y0, x1, y1, rank, nranks, C.byref(out)))
        return out.as_dict()

    def debug_wave_times(self, cam, W, H) -> np.ndarray:
        """(ntiles, 16) u64 per wave, see cgrt_debug_wave_times in include/cgrt.h (diagnostic launch)."""
        nst = ((W + 63) // 64) * ((H + 63) // 64)
        nt = 4 * 16 * 8 * ((nst + 7) // 8)
        out = np.zeros((nt, 16), np.uint64)
        c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
        _check(lib().cgrt_debug_wave_times(self._h, C.byref(c), W, H, _ptr(out), nt))
        return out

    def debug_trace_shadow(self, rays, dist, how: int = 0, dmul: int = 1, capacity: int = 0, expected: int = 0, mirror_rays=None,
                           mirror_capacity: int = 0, mirror_expected: int = 0):
        """cgrt_debug_trace_shadow: the frame's shadow-list launchers on caller rays (see include/cgrt.h for `how`).  The ray is in
        shadow iff `hit && !(t + 0.001f >= dist)`.  Returns hits (n entries for how 0, else max(n, capacity): entries the kernel did
        not write hold the 0xA5 fill), and for how 2 also (mirror hits, mirror normals), max(nmirror, mirror_capacity) entries each."""
        r = _as_ray_array(rays)
        d = np.ascontiguousarray(dist, np.float32).reshape(-1)
        if len(d) != len(r):
            raise ValueError("dist needs one entry per ray")
        n = len(r)
        hits = np.zeros(n if how == 0 else max(n, capacity), HIT_DTYPE)
        m = _as_ray_array(mirror_rays if mirror_rays is not None else np.zeros((0, 7), np.float32))
        mcap = max(len(m), mirror_capacity) if how == 2 else 0
        mh = np.zeros(mcap, HIT_DTYPE)
        mn = np.zeros((mcap, 3), np.float32)
        _check(lib().cgrt_debug_trace_shadow(self._h, _ptr(r), _ptr(d), n, how, dmul, capacity, expected, _ptr(m), len(m), mirror_capacity,
                                             mirror_expected, _ptr(mh), _ptr(mn), _ptr(hits)))
        return (hits, mh, mn) if how == 2 else hits

    def debug_soft_lit(self, item_rays, item_hits, item_pixels, spherical, units, samples: int, seed: int = 0, level: int = 0,
                       anyhit: bool = True) -> np.ndarray:
        """cgrt_debug_soft_lit: the frame's soft-shadow launcher on caller items (ray + hit + pixel).  Returns lit[nitems, nspherical]
        (uint32): the samples of each spherical light that reach each item's hit point."""
        r = _as_ray_array(item_rays)
        h = np.ascontiguousarray(item_hits, HIT_DTYPE)
        px = np.ascontiguousarray(item_pixels, np.int32)
        if len(h) != len(r) or len(px) != len(r):
            raise ValueError("item_rays, item_hits and item_pixels need the same length")
        q, keep = self._soft_arg(spherical, units, samples, seed)  # noqa: F841
        lit = np.zeros((len(r), len(keep[0]) if keep else 0), np.uint32)
        _check(lib().cgrt_debug_soft_lit(self._h, _ptr(r), _ptr(h), _ptr(px), len(r), q, level, 1 if anyhit else 0, _ptr(lit)))
        return lit

    def count_batch(self, rays: np.ndarray) -> dict:
        rays = _as_ray_array(rays)
        out = Counters()
        _check(lib().cgrt_count_batch(self._h, _ptr(rays), len(rays), C.byref(out)))
        return out.as_dict()


class PointGrid:
    """A built point-set neighbour grid on the device (Scene.point_grid_tensor; include/cgrt.h "Point-set neighbours"): it owns the grid's
    tensor and answers queries on torch tensors -- points (n, 3) float32 on the scene's device, radius2 None, a float (one squared
    radius for every query) or an (n,) float32 tensor, skip_same_index: data point i is not a neighbour of query i.  Every call only
    enqueues on `stream` (default: torch.cuda.current_stream()), except where it says it blocks; the caller orders a query on another
    stream behind the build.  Records are (…, 2) float32 with the data index BITS in column 1: records.view(torch.int32)[..., 1]."""

    #: bounded passes of knn (the radius doubles in each) before the unbounded one
    KNN_PASSES = 8

    def __init__(self, scene: "Scene", grid, m: int, cell: float):
        self.scene, self.grid, self.m, self.cell = scene, grid, int(m), float(cell)

    def _args(self, points, radius2, max_dist2):
        n, rad, md = self.scene._neighbor_tensors(points, radius2, max_dist2)
        return n, rad, md, self.grid.data_ptr(), self.grid.numel()

    def count(self, points, radius2=None, max_dist2: float = float("inf"), skip_same_index: bool = False, out=None, stream=None):
        """The number of data points within each query's squared radius: (n,) torch.int32, into `out` or a new tensor."""
        import torch

        n, rad, md, g, gb = self._args(points, radius2, max_dist2)
        if out is not None:
            self.scene._device_tensor(out, "out", (torch.int32,), (n,))
        return self.scene._tensor_call(out, (n,), torch.int32, stream, lambda o, s: self.scene.count_point_neighbors_device(
            g, gb, points.data_ptr(), n, o.data_ptr(), d_radius2_ptr=rad, max_dist2=md, skip_same_index=skip_same_index, stream=s))

    def list(self, points, radius2=None, max_dist2: float = float("inf"), skip_same_index: bool = False, stream=None):
        """Every neighbour of every query, CSR style: (offsets (n + 1,) torch.int64, records (total, 2) float32), query i's neighbours
        are records[offsets[i]:offsets[i + 1]] in (d2, index) order.  A count call, a torch cumsum and the list call are enqueued on
        `stream`; the total is read back in between (one synchronisation of that stream)."""
        n, rad, md, g, gb = self._args(points, radius2, max_dist2)
        return self.scene._slots_full_tensor(
            n, stream, lambda s: self.count(points, radius2, max_dist2, skip_same_index, stream=s),
            lambda o, cap, off, s: self.scene.list_point_neighbors_device(g, gb, points.data_ptr(), n, o, cap, d_offsets_ptr=off, d_radius2_ptr=rad,
                                                                          max_dist2=md, skip_same_index=skip_same_index, stream=s))

    def nearest(self, points, k: int, radius2=None, max_dist2: float = float("inf"), skip_same_index: bool = False, want_counts: bool = False,
                out=None, stream=None):
        """The k nearest data points of every query within its squared radius: records (n, k, 2) float32 (`out`, or a new tensor), unused
        entries {+inf, NO_PRIM}; with want_counts=True (records, counts (n,) torch.int32: the full numbers of neighbours)."""
        n, rad, md, g, gb = self._args(points, radius2, max_dist2)
        rec, counts = self.scene._slots_first_tensor(
            n, k, want_counts, out, stream,
            lambda o, c, s: self.scene.list_point_neighbors_device(g, gb, points.data_ptr(), n, o, n * k, k=k, d_counts_ptr=c, d_radius2_ptr=rad,
                                                                   max_dist2=md, skip_same_index=skip_same_index, stream=s))
        return (rec, counts) if want_counts else rec

    def knn(self, points, k: int, skip_same_index: bool = False, stream=None):
        """The k nearest data points of every query, no radius from the caller: records (n, k, 2) float32, byte for byte what the brute
        form gives for r2 = +inf and k records per query (fewer than k data points: the rest {+inf, NO_PRIM}).  A composition, not a C
        entry: `nearest` with counts at r2 = cell^2; a query whose count reaches k holds its exact k nearest (whatever lies outside the
        radius is farther than everything inside); the others are asked again with 4 r2 -- in place, under a per-query radius that is
        negative for the finished ones, so that every query keeps its index and skip_same_index its meaning -- up to KNN_PASSES times,
        and what is still short then takes one pass with r2 = +inf, the linear walk over the grid's entries.  BLOCKS: the number of
        unfinished queries is read back after every pass."""
        import torch

        n = self.scene._points_tensor(points)
        if k < 1:
            raise ValueError("k must be at least 1")
        dev, stream = self.scene._torch_stream(stream)
        with torch.cuda.stream(stream):
            out = torch.empty((n, k, 2), dtype=torch.float32, device=dev)
            if n == 0:
                return out
            c2 = float(np.float32(self.cell) * np.float32(self.cell))
            r2 = torch.full((n,), c2, dtype=torch.float32, device=dev)
            done = torch.zeros((n,), dtype=torch.bool, device=dev)
            for p in range(self.KNN_PASSES + 1):
                if p == self.KNN_PASSES:
                    r2 = torch.where(done, torch.full_like(r2, -1.0), torch.full_like(r2, float("inf")))
                rec, cnt = self.nearest(points, k, radius2=r2, skip_same_index=skip_same_index, want_counts=True, stream=stream)
                if p:  # (as integers: an index's bits may spell a NaN)
                    rec = torch.where(done[:, None, None], out.view(torch.int32), rec.view(torch.int32)).view(torch.float32)
                out = rec
                done = done | (cnt >= k)
                if p == self.KNN_PASSES or bool(done.all().item()):
                    break
                r2 = torch.where(done, torch.full_like(r2, -1.0), r2 * 4.0)
        return out

    @staticmethod
    def _frame_views(buf, neighbors) -> dict:
        """The fields of (n, 16) float32 frame records as views of that one tensor (include/cgrt.h CgrtPointFrame)."""
        import torch

        return dict(centroid=buf[:, 0:3], used=buf.view(torch.int32)[:, 3], normal=buf[:, 4:7], tangent_u=buf[:, 8:11], tangent_v=buf[:, 12:15],
                    eigenvalues=buf[:, 7::4], neighbors=neighbors, records=buf)

    def _frames_call(self, points, data, k: int, radius2, max_dist2, skip_same_index, orient, stream):
        """(frames (n, 16) float32, neighbors (n, k, 2) float32), enqueued on `stream`."""
        import torch

        if k < 1:
            raise ValueError("k must be at least 1")
        n, rad, md, g, gb = self._args(points, radius2, max_dist2)
        m = self.scene._points_tensor(data)
        if m != self.m:
            raise ValueError("data must be the (m, 3) tensor the grid was built on")
        if orient is not None:
            self.scene._device_tensor(orient, "orient", (torch.float32,), (n, 3))
        dev, stream = self.scene._torch_stream(stream)
        _check_one_hip_runtime()
        with torch.cuda.stream(stream):
            buf = torch.empty((n, 16), dtype=torch.float32, device=dev)
            nb = torch.empty((n, k, 2), dtype=torch.float32, device=dev)
        if n:
            self.scene.point_frames_device(g, gb, data.data_ptr() if m else 0, m, points.data_ptr(), n, k, nb.data_ptr(), buf.data_ptr(),
                                           d_orient_ptr=orient.data_ptr() if orient is not None else 0, d_radius2_ptr=rad, max_dist2=md,
                                           skip_same_index=skip_same_index, stream=stream.cuda_stream)
        return buf, nb

    def frames(self, points, data, k: int, radius2=None, max_dist2: float = float("inf"), skip_same_index: bool = False, orient=None,
               stream=None) -> dict:
        """The local PCA of every query's k nearest data points within its squared radius (include/cgrt.h "Point-set frames"): search
        and solve in one kernel, only enqueued.  data: the (m, 3) tensor the grid was built on, alive and unchanged until the call has
        run (the frames read coordinates by index).  orient ((n, 3) float32, optional): normals are turned to the side of orient[i].
        A dict of views over ONE (n, 16) float32 tensor ('records'): 'centroid', 'normal', 'tangent_u', 'tangent_v' (n, 3), 'eigenvalues'
        (n, 3) ascending, 'used' (n,) int32 -- and 'neighbors' (n, k, 2), the records `nearest` gives.  used == 0: a record of zeros."""
        return self._frame_views(*self._frames_call(points, data, k, radius2, max_dist2, skip_same_index, orient, stream))

    def knn_frames(self, points, data, k: int, skip_same_index: bool = False, orient=None, stream=None) -> dict:
        """`frames` over the k nearest data points with no radius from the caller: byte for byte what the brute form gives for r2 = +inf.
        The composition of `knn`: `frames` at r2 = cell^2; a query whose used reaches k is finished; the others are asked again in place
        with 4 r2 (a negative radius for the finished ones) up to KNN_PASSES times, and what is still short takes one unbounded pass.
        BLOCKS: the number of unfinished queries is read back after every pass."""
        import torch

        n = self.scene._points_tensor(points)
        dev, stream = self.scene._torch_stream(stream)
        with torch.cuda.stream(stream):
            if n == 0:
                return self._frame_views(*self._frames_call(points, data, k, None, float("inf"), skip_same_index, orient, stream))
            c2 = float(np.float32(self.cell) * np.float32(self.cell))
            r2 = torch.full((n,), c2, dtype=torch.float32, device=dev)
            done = torch.zeros((n,), dtype=torch.bool, device=dev)
            buf = nb = None
            for p in range(self.KNN_PASSES + 1):
                if p == self.KNN_PASSES:
                    r2 = torch.where(done, torch.full_like(r2, -1.0), torch.full_like(r2, float("inf")))
                b, r = self._frames_call(points, data, k, r2, float("inf"), skip_same_index, orient, stream)
                if p:  # (as integers: an index's bits may spell a NaN)
                    b = torch.where(done[:, None], buf.view(torch.int32), b.view(torch.int32)).view(torch.float32)
                    r = torch.where(done[:, None, None], nb.view(torch.int32), r.view(torch.int32)).view(torch.float32)
                buf, nb = b, r
                done = done | (buf.view(torch.int32)[:, 3] >= k)
                if p == self.KNN_PASSES or bool(done.all().item()):
                    break
                r2 = torch.where(done, torch.full_like(r2, -1.0), r2 * 4.0)
        return self._frame_views(buf, nb)


# ---- one caller, N devices, one framebuffer ----
def trace_primary_multi(scenes, cam, W: int, H: int, want_normals: bool = False):
    """cgrt_trace_primary_multi over replicas `scenes` (one Scene per device / rank). Returns (hits, normals or None, stats dict)."""
    arr = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    hits = np.zeros(W * H, HIT_DTYPE)
    normals = np.zeros((W * H, 3), np.float32) if want_normals else None
    st = MultiStats()
    c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
    _check(lib().cgrt_trace_primary_multi(arr, len(scenes), C.byref(c), W, H, _ptr(hits), _ptr(normals), C.byref(st)))
    return hits, normals, dict(replicas=st.replicas, kernel_ms_max=st.kernel_ms_max, download_ms_max=st.download_ms_max, wall_ms=st.wall_ms,
                               rays=[int(st.rays[i]) for i in range(len(scenes))])


def render_multi(scenes, cam, W: int, H: int, lights=None, max_level: int = 2, spherical=None, units=None, samples: int = 200, seed: int = 0):
    """cgrt_render_multi over replicas `scenes`. Returns (rgb[W*H,3], stats dict)."""
    arr = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    lights = _f32(scenes[0].sd.point_lights if lights is None else lights, (-1, 6))
    rgb = np.zeros((W * H, 3), np.float32)
    st = RenderStats()
    q = None
    if spherical is not None:
        spherical, units = _f32(spherical, (-1, 7)), _f32(units, (-1, 3))
        q = C.byref(SoftShadows(spherical.ctypes.data, units.ctypes.data, len(spherical), samples, len(units), seed, 0))
    c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
    _check(lib().cgrt_render_multi(arr, len(scenes), C.byref(c), W, H, _ptr(lights), len(lights), q, max_level, _ptr(rgb), C.byref(st)))
    return rgb, {k: getattr(st, k) for k, _ in st._fields_}


def render_multi_aa(scenes, cam, W: int, H: int, lights=None, max_level: int = 2, spherical=None, units=None, samples: int = 200,
                    seed: int = 0):
    """cgrt_render_multi_aa over replicas `scenes`: the anti-aliased frame (Scene.render_aa), every replica downloading only its own
    resolved pixels. Returns (rgb[W*H,3], stats dict)."""
    arr = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    lights = _f32(scenes[0].sd.point_lights if lights is None else lights, (-1, 6))
    rgb = np.zeros((W * H, 3), np.float32)
    st = RenderStats()
    q = None
    if spherical is not None:
        spherical, units = _f32(spherical, (-1, 7)), _f32(units, (-1, 3))
        q = C.byref(SoftShadows(spherical.ctypes.data, units.ctypes.data, len(spherical), samples, len(units), seed, 0))
    c = cam if isinstance(cam, Camera) else Camera.from_array(cam)
    _check(lib().cgrt_render_multi_aa(arr, len(scenes), C.byref(c), W, H, _ptr(lights), len(lights), q, max_level, _ptr(rgb), C.byref(st)))
    return rgb, {k: getattr(st, k) for k, _ in st._fields_}


def debug_export_frame(rgb, W: int, H: int, format="rgb", row_bytes: int = 0, out: Optional[np.ndarray] = None, device: int = 0) -> np.ndarray:
    """cgrt_debug_export_frame: the export kernel of render_device on the given float frame ((W*H, 3)).  `out` (uint8, at least the bytes
    the format and row_bytes span; zeros by default) is uploaded, exported into and returned: bytes the export does not write keep their
    values.  Returns the raw bytes."""
    fmt = _frame_format(format)
    rgb = _f32(rgb, (W * H, 3))
    row = W * (12 if fmt == 0 else 4)
    pitch = row_bytes or row
    n = pitch * ((3 * H if fmt == 1 else H) - 1) + row
    out = np.zeros(n, np.uint8) if out is None else out
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < n:
        raise ValueError(f"out must be a contiguous uint8 array of at least {n} bytes")
    _check(lib().cgrt_debug_export_frame(device, _ptr(rgb), W, H, fmt, int(row_bytes), _ptr(out)))
    return out


def resolve_aa(sub: np.ndarray, W: int, H: int) -> np.ndarray:
    """The resolve of the reference's antiAliasing branch (main.cpp:663-687) in numpy float32, for checking: `sub` is a 2W x 2H frame
    ((2W*2H, 3), index yc*2W + xc); pixel (x, y) = (((0 + s[2y][2x]) + s[2y][2x+1]) + s[2y+1][2x]) + s[2y+1][2x+1]) / 5.0f."""
    s = np.asarray(sub, np.float32).reshape(2 * H, 2 * W, 3)
    acc = np.zeros((H, W, 3), np.float32)
    for dy in (0, 1):
        for dx in (0, 1):
            acc = acc + s[dy::2, dx::2]
    return (acc / (np.float32(2.0) * np.float32(2.5))).reshape(W * H, 3)


# ---- element-wise primitives (src/ray_tracing.h:10-20) ----
def ray_triangle(tri18, rays, device=0):
    tri18 = _f32(tri18, (-1, 18))
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    n = len(rays)
    t, hit, nrm = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)
    _check(lib().cgrt_ray_triangle_batch(device, _ptr(tri18), _ptr(rays), n, _ptr(t), _ptr(hit), _ptr(nrm)))
    return t, hit, nrm


def ray_plane(plane4, rays, device=0):
    plane4 = _f32(plane4, (-1, 4))
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    n = len(rays)
    t, hit = np.zeros(n, np.float32), np.zeros(n, np.uint8)
    _check(lib().cgrt_ray_plane_batch(device, _ptr(plane4), _ptr(rays), n, _ptr(t), _ptr(hit)))
    return t, hit


def ray_box(box6, rays, device=0):
    box6 = _f32(box6, (-1, 6))
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    n = len(rays)
    t, hit, inside = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    _check(lib().cgrt_ray_box_batch(device, _ptr(box6), _ptr(rays), n, _ptr(t), _ptr(hit), _ptr(inside)))
    return t, hit, inside


def ray_sphere(sph4, rays, device=0):
    sph4 = _f32(sph4, (-1, 4))
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    n = len(rays)
    t, hit, nrm = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)
    _check(lib().cgrt_ray_sphere_batch(device, _ptr(sph4), _ptr(rays), n, _ptr(t), _ptr(hit), _ptr(nrm)))
    return t, hit, nrm


def fastdiv_check(a, d, device=0):
    """(mismatch count, first_bad[a, d, got, expected]) of the kernels' exact fast division vs IEEE a / d."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    d = np.ascontiguousarray(d, np.float32).reshape(-1)
    mm = np.zeros(1, np.uint64)
    bad = np.zeros(4, np.float32)
    _check(lib().cgrt_debug_fastdiv_check(device, _ptr(a), _ptr(d), len(a), _ptr(mm), _ptr(bad)))
    return int(mm[0]), bad


def triangle_plane(tri9, device=0):
    tri9 = _f32(tri9, (-1, 9))
    out = np.zeros((len(tri9), 4), np.float32)
    _check(lib().cgrt_triangle_plane_batch(device, _ptr(tri9), len(tri9), _ptr(out)))
    return out


def point_in_triangle(in15, device=0):
    in15 = _f32(in15, (-1, 15))
    out = np.zeros(len(in15), np.uint8)
    _check(lib().cgrt_point_in_triangle_batch(device, _ptr(in15), len(in15), _ptr(out)))
    return out


# ---- C++ host mirror (cg-raytracer_amd/host): render driver, OBJ loader, BMP writer ----
_host = None


def host_lib() -> C.CDLL:
    global _host
    if _host is None:
        lib()  # libcgrt.so first (dependency)
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError(f"{HOST_LIB_PATH} is missing: run __graft_entry__.build()")
        H = C.CDLL(HOST_LIB_PATH)
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
        H.cgrt_host_last_error.restype = C.c_char_p
        H.cgrt_host_render.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, i32, i32, i32, vp, vp]
        H.cgrt_host_time_screen_render.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, i32, i32, i32, i32, vp]
        H.cgrt_host_render_per_ray.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, i32, i32, i32, i32, vp, vp]
        H.cgrt_host_render_soft.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, u32, u32, vp, i32, i32, i32, vp, vp, i32]
        H.cgrt_host_load_obj.argtypes = [C.c_char_p, i32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), vp, vp, vp, vp]
        H.cgrt_host_write_bmp.argtypes = [C.c_char_p, vp, i32, i32]
        H.cgrt_host_selftest.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, C.POINTER(i32)]
        H.cgrt_host_threads_test.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, i32, vp]
        H.cgrt_host_render_bmp.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, i32, i32, i32, i32, C.c_char_p, vp]
        H.cgrt_host_render_aa.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, i32, i32, i32, i32, i32, C.c_char_p, vp, vp]
        H.cgrt_host_shade_rays.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, u32, u32, vp, C.c_uint64, i32, i32, i32, vp, vp]
        H.cgrt_host_occluded.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, C.c_uint64, vp]
        H.cgrt_host_in_shadow.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, C.c_uint64, vp]
        H.cgrt_host_soft_lit.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, u32, u32, u32, vp, C.c_uint64, vp]
        _host = H
    return _host


def host_render(sd: SceneData, cam, W: int, H: int, max_level: int = 2):
    """renderRayTracing of the C++ host mirror (wavefront over the GPU path). Returns (rgb[H*W,3], stats dict)."""
    Hl = host_lib()
    pn, tri = _f32(sd.pos_nrm, (-1, 6)), np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
    tm, mats = np.ascontiguousarray(sd.tri_mesh, np.uint32), _f32(sd.materials, (-1, 8))
    lights, camv = _f32(sd.point_lights, (-1, 6)), _f32(cam, (9,))
    rgb = np.zeros((W * H, 3), np.float32)
    st = np.zeros(5, np.float64)
    rc = Hl.cgrt_host_render(_ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats), _ptr(lights), len(lights),
                             _ptr(camv), W, H, max_level, _ptr(rgb), _ptr(st))
    if rc:
        raise RuntimeError("cgrt_host_render: " + Hl.cgrt_host_last_error().decode())
    return rgb, dict(primary=int(st[0]), shadow=int(st[1]), reflection=int(st[2]), seconds_device=float(st[3]), seconds_total=float(st[4]))


def host_time_screen_render(sd: SceneData, cam, W: int, H: int, max_level: int = 2, reps: int = 5) -> dict:
    """Whole-call milliseconds of the mirror's Screen-filling drivers (BVH built once): renderRayTracingOnDevice, renderRayTracing."""
    Hl = host_lib()
    pn, tri = _f32(sd.pos_nrm, (-1, 6)), np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
    tm, mats = np.ascontiguousarray(sd.tri_mesh, np.uint32), _f32(sd.materials, (-1, 8))
    lights, camv = _f32(sd.point_lights, (-1, 6)), _f32(cam, (9,))
    ms = np.zeros(3, np.float64)
    rc = Hl.cgrt_host_time_screen_render(_ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats), _ptr(lights), len(lights),
                                         _ptr(camv), W, H, max_level, reps, _ptr(ms))
    if rc:
        raise RuntimeError("cgrt_host_time_screen_render: " + Hl.cgrt_host_last_error().decode())
    return dict(on_device_ms=float(ms[0]), host_wavefront_ms=float(ms[1]), on_device_device_share_ms=float(ms[2]))


def host_render_per_ray(sd: SceneData, cam, W: int, H: int, max_level: int = 2, threads: int = 0):
    """The reference's driver taken literally through the C++ mirror (renderToBufferPerRay): omp parallel for over rows, per-pixel
    recursion, one BoundingVolumeHierarchy::intersect call per ray from `threads` threads. Returns (rgb[H*W,3], stats dict)."""
    Hl = host_lib()
    pn, tri = _f32(sd.pos_nrm, (-1, 6)), np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
    tm, mats = np.ascontiguousarray(sd.tri_mesh, np.uint32), _f32(sd.materials, (-1, 8))
    lights, camv = _f32(sd.point_lights, (-1, 6)), _f32(cam, (9,))
    rgb = np.zeros((W * H, 3), np.float32)
    st = np.zeros(5, np.float64)
    rc = Hl.cgrt_host_render_per_ray(_ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats), _ptr(lights), len(lights),
                                     _ptr(camv), W, H, max_level, threads, _ptr(rgb), _ptr(st))
    if rc:
        raise RuntimeError("cgrt_host_render_per_ray: " + Hl.cgrt_host_last_error().decode())
    return rgb, dict(primary=int(st[0]), shadow=int(st[1]), reflection=int(st[2]), seconds_device=float(st[3]), seconds_total=float(st[4]))


def host_render_soft(sd: SceneData, cam, W: int, H: int, spherical, units=None, samples: int = 200, seed: int = 0, lights=None,
                     max_level: int = 2, on_device: bool = False):
    """renderRayTracing of the C++ host mirror for a scene with spherical lights (soft shadows, main.cpp:168-218).
    units=None uses the mirror's own gaussian table (SoftShadowSampler::gaussian); on_device=True runs the C++ mirror's
    renderToBufferOnDevice (the whole driver on the GPU) instead of its host-driven wavefront."""
    Hl = host_lib()
    pn, tri = _f32(sd.pos_nrm, (-1, 6)), np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
    tm, mats = np.ascontiguousarray(sd.tri_mesh, np.uint32), _f32(sd.materials, (-1, 8))
    lights, camv = _f32(sd.point_lights if lights is None else lights, (-1, 6)), _f32(cam, (9,))
    spherical = _f32(spherical, (-1, 7))
    units = np.zeros((0, 3), np.float32) if units is None else _f32(units, (-1, 3))
    rgb = np.zeros((W * H, 3), np.float32)
    st = np.zeros(6, np.float64)
    rc = Hl.cgrt_host_render_soft(_ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats), _ptr(lights), len(lights),
                                  _ptr(spherical), len(spherical), _ptr(units), len(units), samples, seed, _ptr(camv), W, H, max_level,
                                  _ptr(rgb), _ptr(st), int(on_device))
    if rc:
        raise RuntimeError("cgrt_host_render_soft: " + Hl.cgrt_host_last_error().decode())
    return rgb, dict(primary=int(st[0]), shadow=int(st[1]), reflection=int(st[2]), soft_shadow=int(st[3]), seconds_device=float(st[4]),
                     seconds_total=float(st[5]))


def host_load_obj(path: str, normalize: bool = False) -> SceneData:
    """loadMesh of the C++ host mirror, as flat arrays."""
    Hl = host_lib()
    nv, nt, nm = C.c_uint32(), C.c_uint32(), C.c_uint32()
    if Hl.cgrt_host_load_obj(path.encode(), int(normalize), C.byref(nv), C.byref(nt), C.byref(nm), None, None, None, None):
        raise RuntimeError("cgrt_host_load_obj: " + Hl.cgrt_host_last_error().decode())
    pn = np.zeros((nv.value, 6), np.float32)
    tri = np.zeros((nt.value, 3), np.uint32)
    tm = np.zeros(nt.value, np.uint32)
    mats = np.zeros((nm.value, 8), np.float32)
    Hl.cgrt_host_load_obj(path.encode(), int(normalize), C.byref(nv), C.byref(nt), C.byref(nm), _ptr(pn), _ptr(tri), _ptr(tm), _ptr(mats))
    return SceneData(pos_nrm=pn, tri=tri, tri_mesh=tm, materials=mats)


def host_selftest(sd: SceneData, rays7) -> Tuple[int, int]:
    """Runs the C++ mirror's per-ray API (BoundingVolumeHierarchy::intersect, free functions, copy-assign) against its
    batched API on the given rays. Returns (disagreements, numLevels)."""
    Hl = host_lib()
    pn, tri = _f32(sd.pos_nrm, (-1, 6)), np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
    tm, mats = np.ascontiguousarray(sd.tri_mesh, np.uint32), _f32(sd.materials, (-1, 8))
    r = _f32(rays7, (-1, 7))
    lv = C.c_int(0)
    bad = Hl.cgrt_host_selftest(_ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats), _ptr(r), len(r), C.byref(lv))
    if bad < 0:
        raise RuntimeError("cgrt_host_selftest: " + Hl.cgrt_host_last_error().decode())
    return int(bad), int(lv.value)


def host_threads_test(sd: SceneData, rays7, nthreads: int = 8):
    """nthreads std::threads call BoundingVolumeHierarchy::intersect per ray on ONE BVH object (as main.cpp:653-656 does);
    returns (disagreements with intersectBatch, timing dict)."""
    Hl = host_lib()
    pn, tri = _f32(sd.pos_nrm, (-1, 6)), np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
    tm, mats = np.ascontiguousarray(sd.tri_mesh, np.uint32), _f32(sd.materials, (-1, 8))
    r = _f32(rays7, (-1, 7))
    tim = np.zeros(8, np.float64)
    bad = Hl.cgrt_host_threads_test(_ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats), _ptr(r), len(r), nthreads, _ptr(tim))
    if bad < 0:
        raise RuntimeError("cgrt_host_threads_test: " + Hl.cgrt_host_last_error().decode())
    return int(bad), dict(us_per_call_one_thread=float(tim[0]), us_per_call_per_thread=float(tim[1]), calls_per_second=float(tim[2]),
                          combined_generations=int(tim[3]), combined_rays=int(tim[4]), largest_generation=int(tim[5]),
                          leader_gpu_us_per_generation=float(tim[6]) / 1e3 / max(1.0, float(tim[3])),
                          leader_launch_us_per_generation=float(tim[7]) / 1e3 / max(1.0, float(tim[3])))


def host_render_bmp(sd: SceneData, cam, W: int, H: int, path: str, max_level: int = 2, nreplicas: int = 1):
    """Scene -> device render (nreplicas BVH replicas sharing the frame) -> Screen -> BMP file; returns the float frame (W*H, 3)."""
    Hl = host_lib()
    pn, tri = _f32(sd.pos_nrm, (-1, 6)), np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
    tm, mats = np.ascontiguousarray(sd.tri_mesh, np.uint32), _f32(sd.materials, (-1, 8))
    lights, camv = _f32(sd.point_lights, (-1, 6)), _f32(cam, (9,))
    rgb = np.zeros((W * H, 3), np.float32)
    rc = Hl.cgrt_host_render_bmp(_ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats), _ptr(lights), len(lights), _ptr(camv),
                                 W, H, max_level, nreplicas, path.encode(), _ptr(rgb))
    if rc:
        raise RuntimeError("cgrt_host_render_bmp: " + Hl.cgrt_host_last_error().decode())
    return rgb


def host_render_aa(sd: SceneData, cam, W: int, H: int, max_level: int = 2, driver: str = "device", nreplicas: int = 1,
                   path: Optional[str] = None):
    """The anti-aliased frame (antiAliasing = true, main.cpp:663-687) through a driver of the C++ mirror: "device"
    (renderToBufferOnDevices over nreplicas replicas; with `path` also Screen -> writeBitmapToFile, as `render --aa` does),
    "wavefront" (renderToBuffer, resolved on the host) or "per_ray" (the reference's loop literally). Returns (rgb[W*H,3], stats dict)."""
    Hl = host_lib()
    pn, tri = _f32(sd.pos_nrm, (-1, 6)), np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
    tm, mats = np.ascontiguousarray(sd.tri_mesh, np.uint32), _f32(sd.materials, (-1, 8))
    lights, camv = _f32(sd.point_lights, (-1, 6)), _f32(cam, (9,))
    rgb = np.zeros((W * H, 3), np.float32)
    st = np.zeros(5, np.float64)
    d = {"device": 0, "wavefront": 1, "per_ray": 2}[driver]
    rc = Hl.cgrt_host_render_aa(_ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats), _ptr(lights), len(lights), _ptr(camv),
                                W, H, max_level, d, nreplicas, None if path is None else path.encode(), _ptr(rgb), _ptr(st))
    if rc:
        raise RuntimeError("cgrt_host_render_aa: " + Hl.cgrt_host_last_error().decode())
    return rgb, dict(primary=int(st[0]), shadow=int(st[1]), reflection=int(st[2]), seconds_device=float(st[3]), seconds_total=float(st[4]))


def host_shade_rays(sd: SceneData, rays, max_level: int = 2, driver: str = "device", spherical=None, units=None, samples: int = 200,
                    seed: int = 0, lights=None, threads: int = 0):
    """getFinalColor of the caller's rays through the C++ mirror: "device" (getFinalColorsOnDevice -> cgrt_shade_rays) or "per_ray"
    (getFinalColorsPerRay: the reference's recursion, one intersect per ray).  Returns (rgb[n,3], stats dict)."""
    Hl = host_lib()
    pn, tri = _f32(sd.pos_nrm, (-1, 6)), np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
    tm, mats = np.ascontiguousarray(sd.tri_mesh, np.uint32), _f32(sd.materials, (-1, 8))
    lights = _f32(sd.point_lights if lights is None else lights, (-1, 6))
    r = _as_ray_array(rays)
    sph = _f32(np.zeros((0, 7)) if spherical is None else spherical, (-1, 7))
    un = _f32(np.zeros((0, 3)) if units is None else units, (-1, 3))
    rgb = np.zeros((len(r), 3), np.float32)
    st = np.zeros(6, np.float64)
    rc = Hl.cgrt_host_shade_rays(_ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats), _ptr(lights), len(lights),
                                 _ptr(sph), len(sph), _ptr(un), len(un), samples, seed, _ptr(r), len(r), max_level,
                                 {"device": 0, "per_ray": 1}[driver], threads, _ptr(rgb), _ptr(st))
    if rc:
        raise RuntimeError("cgrt_host_shade_rays: " + Hl.cgrt_host_last_error().decode())
    return rgb, dict(primary=int(st[0]), shadow=int(st[1]), reflection=int(st[2]), soft_shadow=int(st[3]), seconds_device=float(st[4]),
                     seconds_total=float(st[5]))


def _host_scene_args(sd: SceneData):
    pn, tri = _f32(sd.pos_nrm, (-1, 6)), np.ascontiguousarray(sd.tri, np.uint32).reshape(-1, 3)
    tm, mats = np.ascontiguousarray(sd.tri_mesh, np.uint32), _f32(sd.materials, (-1, 8))
    return (pn, tri, tm, mats), (_ptr(pn), len(pn), _ptr(tri), _ptr(tm), len(tri), _ptr(mats), len(mats))


def host_occluded(sd: SceneData, rays) -> np.ndarray:
    """BoundingVolumeHierarchy::intersectsBatch of the C++ mirror (cgrt_occluded).  Meshes only (the mirror's test scenes carry no
    spheres).  Returns an (n,) bool array."""
    keep, a = _host_scene_args(sd)  # noqa: F841
    r = _as_ray_array(rays)
    out = np.zeros(len(r), np.uint8)
    if host_lib().cgrt_host_occluded(*a, _ptr(r), len(r), _ptr(out)):
        raise RuntimeError("cgrt_host_occluded: " + host_lib().cgrt_host_last_error().decode())
    return out.view(np.bool_)


def host_in_shadow(sd: SceneData, points, lights=None) -> np.ndarray:
    """pointsInShadowOnDevice of the C++ mirror (cgrt_in_shadow) with the scene's point lights.  Returns (n, nlights) bool."""
    keep, a = _host_scene_args(sd)  # noqa: F841
    p = _f32(points, (-1, 3))
    lights = _f32(sd.point_lights if lights is None else lights, (-1, 6))
    out = np.zeros((len(p), len(lights)), np.uint8)
    if host_lib().cgrt_host_in_shadow(*a, _ptr(lights), len(lights), _ptr(p), len(p), _ptr(out)):
        raise RuntimeError("cgrt_host_in_shadow: " + host_lib().cgrt_host_last_error().decode())
    return out.view(np.bool_)


def host_soft_lit(sd: SceneData, points, spherical, units, samples: int = 200, seed: int = 0) -> np.ndarray:
    """softShadowCountsOnDevice of the C++ mirror (cgrt_soft_lit).  Returns (n, nspherical) uint32."""
    keep, a = _host_scene_args(sd)  # noqa: F841
    p = _f32(points, (-1, 3))
    sph, un = _f32(spherical, (-1, 7)), _f32(units, (-1, 3))
    lit = np.zeros((len(p), len(sph)), np.uint32)
    if host_lib().cgrt_host_soft_lit(*a, _ptr(sph), len(sph), _ptr(un), len(un), samples, seed, _ptr(p), len(p), _ptr(lit)):
        raise RuntimeError("cgrt_host_soft_lit: " + host_lib().cgrt_host_last_error().decode())
    return lit


def host_write_bmp(path: str, rgb, W: int, H: int) -> None:
    rgb = _f32(rgb, (W * H, 3))
    if host_lib().cgrt_host_write_bmp(path.encode(), _ptr(rgb), W, H):
        raise RuntimeError("cgrt_host_write_bmp: " + host_lib().cgrt_host_last_error().decode())
