"""The ray of a CgrtRayCamera (include/cgrt.h) restated in numpy float32, one rounded operation per step, and the cameras the ray-camera
tests share.  Not a test module."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def rays_of(cam, W, H, x0=0, y0=0, w=None, h=None):
    """(w*h, 7) float32 rays {origin, direction, t} of pixels (x0 .. x0+w) x (y0 .. y0+h), row-major, of the camera's W x H frame (W and
    H only name the default region: they do not enter the formula).  cam: a RayCamera (ctypes) or its 20 float32 words."""
    a = np.frombuffer(bytes(cam), np.float32) if not isinstance(cam, np.ndarray) else np.ascontiguousarray(cam, np.float32).reshape(20)
    off = a[18:20].view(np.int32)
    w = W - x0 if w is None else w
    h = H - y0 if h is None else h
    ys, xs = np.meshgrid(np.arange(y0, y0 + h, dtype=np.int32), np.arange(x0, x0 + w, dtype=np.int32), indexing="ij")
    fx = (xs.reshape(-1) + off[0]).astype(np.int32).astype(F32)  # 32-bit integer add, then convert
    fy = (ys.reshape(-1) + off[1]).astype(np.int32).astype(F32)
    out = np.empty((w * h, 7), F32)

    def affine(base, dx, dy):  # (base + fx * dx) + fy * dy, each operation rounded to f32
        cols = []
        for c in range(3):
            px = (fx * F32(dx[c])).astype(F32)
            py = (fy * F32(dy[c])).astype(F32)
            cols.append(((F32(base[c]) + px).astype(F32) + py).astype(F32))
        return cols

    with np.errstate(all="ignore"):
        o = affine(a[0:3], a[3:6], a[6:9])
        v = affine(a[9:12], a[12:15], a[15:18])
        sq = [(c * c).astype(F32) for c in v]
        dot = ((sq[0] + sq[1]).astype(F32) + sq[2]).astype(F32)
        inv = (F32(1.0) / np.sqrt(dot, dtype=F32)).astype(F32)
        for c in range(3):
            out[:, c] = o[c]
            out[:, 3 + c] = (v[c] * inv).astype(F32)
    out[:, 6] = FLT_MAX
    return out


def look_at_pose(eye, target, up=(0.0, 1.0, 0.0)):
    """4x4 camera-to-world pose, OpenCV axes (x right, y down, z forward), of a camera at `eye` looking at `target`."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P


def _place(p, at, scale):
    return np.asarray(at, np.float64) + scale * np.asarray(p, np.float64)


def pinhole(pkg, W, H, eye=(1.1, 1.3, -2.6), target=(0.05, -0.05, 0.0), f=1.1, skew=0.0, centre=(0.42, 0.57), fy_scale=1.0, at=(0, 0, 0), scale=1.0):
    """A perspective pinhole with an off-centre principal point (centre: fractions of W and H), f in units of H.  at, scale: the scene's
    centre and size (eye and target are given for a unit scene at the origin)."""
    K = np.array([[f * H, skew, centre[0] * W], [0.0, f * H * fy_scale, centre[1] * H], [0.0, 0.0, 1.0]])
    return pkg.RayCamera.from_pinhole(K, look_at_pose(_place(eye, at, scale), _place(target, at, scale)))


def ortho(pkg, W, H, width=2.4, eye=(1.0, 1.2, -2.6), target=(0.0, 0.0, 0.0), at=(0, 0, 0), scale=1.0):
    """An orthographic camera `width` units wide looking at `target` from `eye`."""
    P = look_at_pose(_place(eye, at, scale), _place(target, at, scale))
    s = width * scale / W
    corner = P[:3, 3] - 0.5 * W * s * P[:3, 0] - 0.5 * H * s * P[:3, 1]
    return pkg.RayCamera.orthographic(corner, P[:3, 0], P[:3, 1], P[:3, 2], s)


def mixed(pkg, W, H, at=(0, 0, 0), scale=1.0):
    """Non-zero origin_d* and dir_d* together: a pinhole whose origin slides across the frame (pushbroom-like)."""
    kw = dict(eye=(-0.9, 1.0, -2.7), centre=(0.5, 0.5), f=1.4, skew=3.0, fy_scale=0.9, at=at, scale=scale)
    c = pinhole(pkg, W, H, **kw)
    P = look_at_pose(_place(kw["eye"], at, scale), _place((0.05, -0.05, 0.0), at, scale))
    return pkg.RayCamera.from_fields(c.origin[:], 0.6 * scale / W * P[:3, 0], 0.3 * scale / H * P[:3, 1], c.dir[:], c.dir_dx[:], c.dir_dy[:])


def camera_set(pkg, W, H, **where):
    """name -> camera: the kinds every GPU check covers.  where: at=, scale= (the scene's centre and size)."""
    return {"pinhole": pinhole(pkg, W, H, **where), "ortho": ortho(pkg, W, H, **where), "mixed": mixed(pkg, W, H, **where)}


def mixed_batch(pkg, W, H, **where):
    """A batch that mixes the kinds, with different x_off / y_off."""
    return [pinhole(pkg, W, H, **where).tile(3, -2), ortho(pkg, W, H, **where), mixed(pkg, W, H, **where).tile(-5, 7),
            pinhole(pkg, W, H, eye=(-1.2, 0.8, -2.4), **where).tile(0, 11), ortho(pkg, W, H, width=1.7, **where).tile(9, 4)]


WHERE = {"spheres": dict(at=(0.0, 0.0, 6.0), scale=3.0)}  # scene name -> where its cameras go (default: a unit scene at the origin)
