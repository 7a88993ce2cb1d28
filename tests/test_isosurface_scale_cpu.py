"""No GPU: the helpers of the iso-surface tests across scale and at size (tests/test_isosurface_scale_gpu.py) held to the restatement
(tests/isosurface_ref.py).

* isosurface_ref.compose_slabs equals the whole-grid restatement on 16 x 16 x 300 with two spheres, origin (-2, -2, 0), spacing 0.25: the
  mesh is closed; a grid whose coordinates are not exact in float32 is refused.
* scale_ref.in_iso_envelope is never wrong on sphere and noise at 17 x 9 x 5, values and iso times 2^kv for kv in KV, origin and spacing
  times 2^kp for kp in KP: an edge it puts inside carries, at that scale, the vertex of scale 1 (unchanged under kv, ldexp(., kp) under
  kp), bit for bit.  Every edge is inside at +-100 and +-20.
* The cases are reachable: at kp = 127 the restatement's vertices hold NaN (inf - inf on an axis the edge does not move along) and inf
  coordinates; the sphere's vertex bytes under kv = -126 and -140 differ from scale 1 with the same triangles."""
import numpy as np
import pytest

import isosurface_ref as iref
import scale_ref as sref
from conftest import same_bits

F32 = np.float32
KV = (-140, -126, -100, -20, 20, 100, 126, 127)
KP = (-140, -126, -100, 100, 126, 127)
DIMS = (17, 9, 5)
ISO = 0.0625


def ld(x, k):
    with np.errstate(all="ignore"):
        return np.ldexp(np.asarray(x, F32), int(k)).astype(F32)


def two_spheres(dims, origin, spacing, centres, radius, z0=0, nz=None):
    """min(1, |p - c| - radius over the centres) on the layers [z0, z0 + nz) of the grid: +1 away from the spheres"""
    nx, ny, _ = dims
    nz = dims[2] - z0 if nz is None else nz
    ax = [float(origin[c]) + np.arange(n, dtype=np.float64) * float(spacing[c]) for c, n in enumerate((nx, ny, z0 + nz))]
    X, Y, Z = ax[0][None, None, :], ax[1][None, :, None], ax[2][z0:, None, None]
    val = np.ones((nz, ny, nx))
    for c in centres:
        val = np.minimum(val, np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - radius)
    return np.ascontiguousarray(val.astype(F32))


def test_compose_slabs_equals_the_whole_grid():
    dims, o, sp = (16, 16, 300), np.float32([-2, -2, 0]), np.float32([0.25, 0.25, 0.25])
    centres, r = ((0.0, -0.125, 2.0), (-0.125, 0.0, 72.0)), 1.2
    whole = two_spheres(dims, o, sp, centres, r)
    assert (whole[20:280] == 1).all() and (whole[:20] < 0).any() and (whole[280:] < 0).any()
    for above in (False, True):
        val = -whole if above else whole
        verts, tris = iref.isosurface(val, o, sp, inside_above=above)
        slabs = [two_spheres(dims, o, sp, centres, r, 0, 20), two_spheres(dims, o, sp, centres, r, 280, 20)]
        assert np.array_equal(slabs[0], whole[:20]) and np.array_equal(slabs[1], whole[280:])
        cv, ct = iref.compose_slabs([-s for s in slabs] if above else slabs, (0, 280), o, sp, inside_above=above)
        assert cv.dtype == F32 and ct.dtype == np.uint32
        assert cv.tobytes() == verts.tobytes() and ct.tobytes() == tris.tobytes()
        first = len(iref.isosurface(val[:20], o, sp, inside_above=above)[0])
        assert 0 < first < len(verts) and (tris >= first).any(), "the second slab's indices are shifted"
        assert len(tris) > 1000 and iref.is_closed(tris) and iref.unreferenced(len(verts), tris) == 0
    with pytest.raises(AssertionError):
        iref.compose_slabs(slabs, (0, 280), o, np.float32([0.25, 0.25, 0.1]))
    with pytest.raises(AssertionError):
        iref.compose_slabs([whole[:5], whole[280:]], (0, 280), o, sp)  # (layer 4 cuts the first sphere)


_cases = {}


def case(name):
    """(values, origin, spacing, verts, tris, owner * 7 + etype) at scale 1, computed once"""
    if name not in _cases:
        val, o, sp = iref.field(name, DIMS, seed=1)
        verts, tris = iref.isosurface(val, o, sp, iso=ISO)
        owner, etype = iref.carrying_edges(val, ISO)
        _cases[name] = (val, o, sp, verts, tris, owner * 7 + etype)
    return _cases[name]


def _edges_agree(key0, v0, keyk, vk):
    """per edge of scale 1: it carries a vertex at the other scale too, with the bits v0"""
    pos = np.searchsorted(keyk, key0)
    found = (pos < len(keyk)) & (keyk[np.minimum(pos, len(keyk) - 1)] == key0) if len(keyk) else np.zeros(len(key0), bool)
    ok = found.copy()
    ok[found] = same_bits(v0[found], vk[pos[found]]).all(1)
    return ok


@pytest.mark.parametrize("name", ["sphere", "noise"])
def test_iso_envelope_is_never_wrong(name):
    val, o, sp, verts, tris, key = case(name)
    assert len(verts) > 100
    for kv in KV:
        inside = sref.in_iso_envelope(val, ISO, o, sp, DIMS, kv, 0)
        vk, tk = iref.isosurface(ld(val, kv), o, sp, iso=float(ld(ISO, kv)))
        ow, et = iref.carrying_edges(ld(val, kv), ld(ISO, kv))
        agree = _edges_agree(key, verts, ow * 7 + et, vk)
        print(f"{name} kv = {kv}: {int(inside.sum())} of {len(key)} inside, {int(agree.sum())} agree")
        assert agree[inside].all(), kv
        if abs(kv) in (20, 100):
            assert inside.all() and vk.tobytes() == verts.tobytes() and tk.tobytes() == tris.tobytes(), kv
        if name == "sphere" and kv in (-126, -140):
            assert tk.tobytes() == tris.tobytes() and vk.shape == verts.shape and vk.tobytes() != verts.tobytes(), kv
    for kp in KP:
        inside = sref.in_iso_envelope(val, ISO, o, sp, DIMS, 0, kp)
        vk, tk = iref.isosurface(val, ld(o, kp), ld(sp, kp), iso=ISO)
        assert tk.tobytes() == tris.tobytes(), "the triangles do not depend on origin or spacing"
        agree = same_bits(ld(verts, kp), vk).all(1)
        print(f"{name} kp = {kp}: {int(inside.sum())} of {len(key)} inside, {int(agree.sum())} agree")
        assert agree[inside].all(), kp
        if abs(kp) == 100:
            assert inside.all(), kp
        if kp == 127:
            assert np.isnan(vk).sum() > 10 and np.isinf(vk).sum() > 10 and not inside.all(), "inf - inf is reached"
        if kp == -140:
            assert not agree.all(), "subnormal positions lose bits"
    assert not sref.in_iso_envelope(val, ISO, o * F32(np.inf), sp, DIMS, 0, 0).any()
