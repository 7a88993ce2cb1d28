"""GPU: iso-surfaces across scale and past 2^18 blocks (include/cgrt.h "Iso-surfaces", its "Envelope" paragraph).  The
helpers are held by tests/test_isosurface_scale_cpu.py.  Vertices are compared through conftest.same_bits (a NaN equals a NaN: inf - inf
has the bits ffc00000 in numpy on x86 and 7fc00000 on the device), triangles by bytes.

* Sphere and noise on (17, 9, 5) and (65, 33, 4), both flags; values and iso times 2^kv, kv in KV, and origin and spacing times 2^kp, kp
  in KP, inside the envelope or not (subnormal and +-inf differences vB - vA, overflowing grid_coord): the count form, the device form at
  full capacity and one below, the host form and debug_isosurface_work all equal the restatement.  The triangles and both counts are
  those of scale 1 at every kp; for every edge scale_ref.in_iso_envelope puts inside the vertex is ldexp(vertex at 1, kp), and unchanged
  under kv.  NaN and inf coordinates at kp = 127 are asserted to be there.  Noise times 2^128 and times 2^130, where most points are
  non-finite: the forms still equal the restatement.
* (64, 64, 16 448): 67 371 008 points, 263 168 blocks, 257 scan tiles of 1 024 -- the second pass of the shared scan's carry loop.  +1
  everywhere but two spheres, the second in tile 257; values built on the device; the expected mesh is isosurface_ref.compose_slabs over
  the layers [0, 48) and [16 384, 16 448).  Count form, device form at full capacity by bytes, closedness, guards compared on the device.
* End to end: sdf_isosurface_tensor on the cube and its grid at 2^k, k in (-20, 30), the level scaled alike: the triangles of scale 1,
  vertices ldexp(vertices at 1, k)."""
import numpy as np
import pytest

import isosurface_ref as iref
import scale_ref as sref
from conftest import same_bits
from test_isosurface_gpu import PAD, SENTINEL, Guarded, _count, _device, _fixture_grid, sc  # noqa: F401  (sc: fixture)
from test_isosurface_scale_cpu import ISO, KP, KV, ld, two_spheres

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
DIMS = ((17, 9, 5), (65, 33, 4))


def _rows(got, want, what, floats):
    """got: the bytes of a guarded array of some capacity; want: the restatement's full array"""
    rows = len(got) // 12
    k = min(rows, len(want))
    g = got[: 12 * k].view(np.uint32).reshape(-1, 3)
    w = np.ascontiguousarray(want[:k]).view(np.uint32).reshape(-1, 3)
    ok = same_bits(g.view(F32), w.view(F32)) if floats else g == w
    if not ok.all():
        bad = np.flatnonzero(~ok.all(1))
        raise AssertionError(f"{what}: {len(bad)} of {k} rows differ, first at {bad[0]}: {g[bad[0]]} != {w[bad[0]]}")
    assert (got[12 * k :] == SENTINEL).all(), f"{what}: a row beyond the count was written"


def _check(sc, val, o, sp, iso, above, ref, what):
    """The count form, the device form at full capacity and one below, the host form and the work counters against the restatement's
    (verts, tris, work); NaN-aware."""
    verts, tris, work = ref
    nv, nt = len(verts), len(tris)
    tv = torch.from_numpy(np.ascontiguousarray(val).copy()).cuda()
    assert _count(sc, val, o, sp, iso, above, tv) == (nv, nt), (what, "count form")
    for vcap, tcap in {(nv, nt), (max(nv - 1, 0), max(nt - 1, 0))}:
        gv, gt, counts = _device(sc, val, o, sp, iso, above, vcap, tcap, tv=tv)
        assert counts == (nv, nt), (what, vcap, tcap)
        _rows(gv, verts, (what, "verts", vcap), True)
        _rows(gt, tris, (what, "tris", tcap), False)
    hv, ht = sc.isosurface(val, o, sp, iso=iso, inside_above=above)
    assert hv.shape == verts.shape and ht.shape == tris.shape and same_bits(hv, verts).all() and ht.tobytes() == tris.tobytes(), (what, "host form")
    assert sc.debug_isosurface_work(val, o, sp, iso=iso, inside_above=above) == work, (what, "work")


# ---- across scale ----
@pytest.mark.parametrize("above", [False, True])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", ["sphere", "noise"])
def test_every_form_at_every_scale(sc, name, dims, above):
    val, o, sp = iref.field(name, dims, seed=1)
    iso = float(F32(ISO))
    verts, tris, work = iref.isosurface(val, o, sp, iso=iso, inside_above=above, want_work=True)
    assert len(verts) > 100 and len(tris) > 100
    _check(sc, val, o, sp, iso, above, (verts, tris, work), "scale 1")
    owner, etype = iref.carrying_edges(val, iso, above)
    key = owner * 7 + etype
    for kv in KV:
        vk, ik = ld(val, kv), float(ld(iso, kv))
        ref = iref.isosurface(vk, o, sp, iso=ik, inside_above=above, want_work=True)
        _check(sc, vk, o, sp, ik, above, ref, f"values * 2^{kv}")
        inside = sref.in_iso_envelope(val, iso, o, sp, dims, kv, 0, inside_above=above)
        ow, et = iref.carrying_edges(vk, ik, above)
        kk = ow * 7 + et
        pos = np.searchsorted(kk, key[inside])
        assert (pos < len(kk)).all() and (kk[pos] == key[inside]).all(), (kv, "an edge inside the envelope lost its vertex")
        assert same_bits(ref[0][pos], verts[inside]).all(), (kv, "the vertex bytes are unchanged under a scale of the values")
        if abs(kv) in (20, 100):  # (on the finer grid a few differences iso - vA of 2^-28 leave the range at 2^-100)
            assert inside.all() if dims == DIMS[0] else inside.mean() > 0.99
    for kp in KP:
        ok_, sk = ld(o, kp), ld(sp, kp)
        ref = iref.isosurface(val, ok_, sk, iso=iso, inside_above=above, want_work=True)
        _check(sc, val, ok_, sk, iso, above, ref, f"positions * 2^{kp}")
        assert ref[1].tobytes() == tris.tobytes() and ref[2] == work, (kp, "triangles and counts do not depend on origin or spacing")
        inside = sref.in_iso_envelope(val, iso, o, sp, dims, 0, kp, inside_above=above)
        assert same_bits(ld(verts, kp), ref[0])[inside].all(), (kp, "vertices are the power-of-two image inside the envelope")
        if abs(kp) == 100:  # (on the finer grid a few coordinates next to 0 are rounding residues of 2^-27)
            assert inside.all() if dims == DIMS[0] else inside.mean() > 0.99
        if kp == 127:
            assert np.isnan(ref[0]).sum() > 10 and np.isinf(ref[0]).sum() > 10, "inf - inf on an axis the edge does not move along"


@pytest.mark.parametrize("kv", [128, 130])
def test_values_scaled_out_of_range(sc, kv):
    dims = (65, 33, 4)
    val, o, sp = iref.field("noise", dims, seed=1)
    vk, ik = ld(val, kv), float(ld(F32(ISO), kv))
    bad = ~np.isfinite(vk)
    print(f"noise * 2^{kv}: {bad.mean():.1%} of the points are non-finite")
    if kv == 130:
        assert bad.mean() > 0.5 and np.isposinf(vk).any() and np.isneginf(vk).any(), "most points are non-finite"
    assert np.isfinite(ik)
    for above in (False, True):
        ref = iref.isosurface(vk, o, sp, iso=ik, inside_above=above, want_work=True)
        assert len(ref[0]) > 0
        with np.errstate(all="ignore"):
            flat = vk.reshape(-1)
            assert np.isinf(flat[1:] - flat[:-1]).any(), "vB - vA overflows"
        _check(sc, vk, o, sp, ik, above, ref, f"values * 2^{kv}")


# ---- past 2^18 blocks ----
BIG = (64, 64, 16448)


def test_past_2_18_blocks(sc):
    o, sp = np.float32([-8, -8, 0]), np.float32([0.25, 0.25, 0.25])
    nx, ny, nz = BIG
    N = nx * ny * nz
    assert N == 67_371_008 and N % (256 * 1024) == 0 and N // (256 * 1024) == 257, "257 scan tiles exactly"
    z0s, depth = (0, 16384), (48, 64)
    centres, r = ((0.0, -0.125, 5.0), (-0.125, 0.0, 16416 * 0.25)), 3.0
    slabs = [two_spheres(BIG, o, sp, centres, r, z0, d) for z0, d in zip(z0s, depth)]
    assert z0s[1] * nx * ny // 256 >= 256 * 1024, "the second slab's blocks lie in tile 257: their starts are the carry"
    for s in slabs:
        assert (s < 0).any() and (s[0] == 1).all() and (s[-1] == 1).all()
    verts, tris = iref.compose_slabs(slabs, z0s, o, sp)
    nv1 = len(iref.isosurface(slabs[0], o, sp)[0])
    nv, nt = len(verts), len(tris)
    assert 0 < nv1 < nv and nt > 2 * nv1 and iref.is_closed(tris)
    tv = torch.full((nz, ny, nx), 1.0, dtype=torch.float32, device="cuda")
    for s, z0 in zip(slabs, z0s):
        tv[z0 : z0 + len(s)] = torch.from_numpy(s).cuda()
    nbytes = sc.isosurface_workspace(BIG)
    ws = torch.full((nbytes + 2 * PAD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    lo = PAD + 8
    assert ws.data_ptr() % 16 == 0

    def ws_intact():
        return bool((ws[:lo] == SENTINEL).all().item()) and bool((ws[lo + nbytes :] == SENTINEL).all().item())

    counts = Guarded(16)
    sc.isosurface_count_device(o, sp, BIG, tv.data_ptr(), counts.ptr(), ws.data_ptr() + lo, nbytes)
    assert tuple(int(x) for x in counts.bytes().view(np.uint64)) == (nv, nt), "count form"
    assert counts.intact() and ws_intact()
    gv, gt, counts = Guarded(12 * nv), Guarded(12 * nt), Guarded(16)
    sc.isosurface_device(o, sp, BIG, tv.data_ptr(), gv.ptr(), nv, gt.ptr(), nt, counts.ptr(), ws.data_ptr() + lo, nbytes)
    assert tuple(int(x) for x in counts.bytes().view(np.uint64)) == (nv, nt), "device form's counts"
    _rows(gv.bytes(), verts, "verts", False)
    _rows(gt.bytes(), tris, "tris", False)
    assert iref.is_closed(gt.bytes().view(np.uint32).reshape(-1, 3))
    assert gv.intact() and gt.intact() and counts.intact() and ws_intact(), "guards"


# ---- end to end ----
@pytest.mark.parametrize("k", [-20, 30])
def test_cube_offset_surface_across_scale(pkg, scene_data, k):
    sd = scene_data("cube")
    n = 24
    origin, spacing, ext = _fixture_grid(sd, n, 0.5)
    offset = F32(0.1 * ext)
    out = []
    for kk in (0, k):
        src = pkg.Scene(sref.scaled(sd, kk), device=0)
        try:
            res = src.sdf_isosurface_tensor(ld(origin, kk), ld(spacing, kk), (n, n, n), offset=float(ld(offset, kk)))
            out.append((res["verts"].cpu().numpy(), res["tris"].cpu().numpy().view(np.uint32), res["values"].cpu().numpy()))
        finally:
            src.close()
    (v0, t0, val0), (vk, tk, valk) = out
    assert len(t0) > 100 and iref.is_closed(t0)
    assert same_bits(ld(val0, k), valk).all(), "the signed distances are the power-of-two image"
    assert tk.tobytes() == t0.tobytes(), "the same triangles"
    assert vk.shape == v0.shape and same_bits(ld(v0, k), vk).all(), "vertices == ldexp(vertices at 1, k)"
