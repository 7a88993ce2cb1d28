"""No GPU: point-set frames (cgrt_point_frames*; include/cgrt.h "Point-set frames").

* The three entries are exported and bound; CgrtPointFrame is 64 bytes with the stated offsets.
* Every argument check, in the documented order, on a host-only scene, ending in CGRT_E_NO_DEVICE.
* The host side of csrc/sym3_eigen.h, compiled as the stand-alone program tools/sym3_eigen_check.cpp, gives the bits of the numpy
  restatement (tests/point_frames_ref.py, which the GPU tests compare bytes with) for steps 4 to 7 -- on the covariances of the clouds and
  on zero, huge, subnormal, NaN and inf matrices.
* The restatement against the truth, numpy.linalg.eigh in float64 on the float64 covariance of the same neighbours (an independent
  computation), on the clouds of point_frames_ref.cloud with k = 3, 8, 32.  With u = 2^-24, T the trace, P the largest coordinate
  magnitude of the neighbourhood, the LARGEST VALUES MEASURED on these clouds are
      eigenvalues   |lambda - lambda64| <= c1 u T + c2 u^2 P^2,  c1 = 3.36 (the clouds at unit scale, where the second term is
                    below 1e-3 of the first), c2 = 1.03 (the cloud at offset 100 with spread 0.01, with c1 as measured)
      unit length   | |v|^2 - 1 | <= 13.2 u
      normal        angle(normal, float64 eigenvector) x (lambda1 - lambda0) / T <= 1.50 (u + u^2 P^2 / T) over the queries whose
                    relative gap exceeds 1e-2 (taken from the norm of the cross product)
      sweeps        every off-diagonal exactly zero after at most 5 sweeps
  and the tests hold four times each (the sweeps: the definition's 8): the clouds are a sample of inputs, not a worst case, so the margin
  covers inputs, not the code.
* Scale: the restatement at 2^s, s in {-40, -8, 8, 40}, against itself at scale 1 (point_frames_ref.scale_case: a base cloud per s, so
  that both scales lie inside the envelope): centroid x 2^s and eigenvalues x 2^2s exactly, vectors and used unchanged, for every query
  inside the envelope -- at least half of them at every s, or the case would show nothing (measured: 205, 284, 300, 221 of 300; the
  queries outside it gave equal bytes as well, which is printed and not claimed).
* Exact cases: points of the plane z = 0.5; k = 1; duplicates of one point; a diagonal covariance; orientation; NaN canonical."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import point_frames_ref as fref

E_ARG, E_NO_DEVICE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0**-24
# the largest values measured (the module's docstring); the tests hold FACTOR times each
MEASURED = dict(c1=3.36, c2=1.03, unit=13.2, angle=1.50, sweeps=5)
FACTOR = 4.0
CLOUDS = ("shell", "patch", "offset", "cube", "holes")
KS = (3, 8, 32)


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ("cgrt_point_frames", "cgrt_point_frames_device", "cgrt_point_frames_brute"):
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    for name in ("point_frames", "point_frames_brute", "point_frames_device"):
        assert callable(getattr(pkg.Scene, name, None)), name
    for name in ("frames", "knn_frames"):
        assert callable(getattr(pkg.PointGrid, name, None)), name
    names = ("centroid", "used", "normal", "lambda0", "tangent_u", "lambda1", "tangent_v", "lambda2")
    offsets = [0, 12, 16, 28, 32, 44, 48, 60]
    assert C.sizeof(pkg.PointFrame) == 64 and [getattr(pkg.PointFrame, k).offset for k in names] == offsets
    assert pkg.POINT_FRAME_DTYPE.itemsize == 64 and [pkg.POINT_FRAME_DTYPE.fields[k][1] for k in names] == offsets
    assert fref.FRAME == pkg.POINT_FRAME_DTYPE


# ---- the argument checks, on a host-only scene ----
@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


N = M = 16
_BUF = {k: np.zeros(4096, np.uint8) for k in ("pts", "data", "rad", "orient", "nb", "frames", "grid")}


def _p(name, off):
    if off is None:
        return None
    base = (-_BUF[name].ctypes.data) % 16
    return C.c_void_p(_BUF[name].ctypes.data + base + off)


def _call(pkg, sc, form, handle="ok", n=N, m=M, cell=0.5, query="ok", md=1.0, rad=None, flags=0, points=0, data=0, grid=0, grid_bytes=None,
          k=4, orient=None, nb=0, frames=0):
    """form: host / brute / device.  points / data / rad / orient / nb / frames / grid: a byte offset from a 16-byte boundary of the
    module's buffers, or None for NULL."""
    L = pkg.lib()
    h = sc._h if handle == "ok" else None
    q = None
    if query is not None:
        qs = pkg.PointQuery()
        qs.radius2, qs.max_dist2, qs.flags = (None if rad is None else _p("rad", rad).value), md, flags
        q = C.byref(qs)
    tail = (_p("pts", points), n, q, k, _p("orient", orient), _p("nb", nb), _p("frames", frames))
    if form == "device":
        need = C.c_uint64(0)
        assert L.cgrt_point_grid_workspace(sc._h, 0, C.byref(need)) == 0
        return L.cgrt_point_frames_device(h, _p("grid", grid), need.value if grid_bytes is None else grid_bytes, _p("data", data), m, *tail, None)
    if form == "host":
        return L.cgrt_point_frames(h, _p("data", data), m, cell, *tail)
    assert form == "brute"
    return L.cgrt_point_frames_brute(h, _p("data", data), m, *tail)


@pytest.mark.parametrize("form", ["host", "brute", "device"])
def test_argument_checks_and_their_order(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    err = lambda: pkg.lib().cgrt_last_error().decode()  # noqa: E731
    inf, nan = float("inf"), float("nan")
    device = form == "device"
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    for md in (0.0, inf, 3e38):
        assert c(md=md) == E_NO_DEVICE, md
    assert c(rad=0) == E_NO_DEVICE and c(flags=1) == E_NO_DEVICE and c(orient=0) == E_NO_DEVICE and c(k=1) == E_NO_DEVICE
    assert c(n=0, points=None, data=None, nb=None, frames=None, grid=None) == E_NO_DEVICE, "n == 0 needs no array"
    assert c(m=0, data=None) == E_NO_DEVICE, "no data point needs no data"
    if not device:
        assert c(nb=None) == E_NO_DEVICE, "the host forms' neighbors may be NULL"
    # every check with every later one failing too: the earlier one is reported
    later = dict(n=1 << 31, m=1 << 31, cell=nan, md=nan, flags=2, k=0, frames=4)
    assert c(handle=None, points=None, **later) == E_ARG and "scene or query" in err()
    assert c(query=None, points=None, **later) == E_ARG and "scene or query" in err()
    for null in ("points", "frames", "data") + (("nb", "grid") if device else ()):
        kw = dict(later)
        kw.pop("frames")
        kw[null] = None
        assert c(**kw) == E_ARG and "NULL" in err(), null
    del later["n"]
    assert c(n=1 << 31, **later) == E_ARG and "n exceeds" in err()
    del later["m"]
    assert c(m=1 << 31, **later) == E_ARG and "m exceeds" in err()
    del later["cell"]
    if form == "host":
        for cell in (nan, 0.0, -1.0, inf):
            assert c(cell=cell, **later) == E_ARG and "cell" in err(), cell
    else:
        assert c(cell=nan) == E_NO_DEVICE, "no cell in this form"
    del later["md"]
    for md in (nan, -1.0, -inf):
        assert c(md=md, **later) == E_ARG and "max_dist2" in err(), md
    del later["flags"]
    assert c(flags=2, **later) == E_ARG and "flags" in err()
    del later["k"]
    assert c(k=0, **later) == E_ARG and "k must be" in err()
    assert c(n=1 << 30, k=129, **later) == E_ARG and "2^37" in err()
    assert c(n=1 << 30, k=128, **later) == (E_ARG if device else E_NO_DEVICE), "n * k == 2^37 records is allowed"
    if device:
        assert "d_frames" in err()
        for name in ("points", "data", "orient", "nb", "rad"):
            assert c(**{name: 2}, **later) == E_ARG and "aligned to their elements" in err(), name
        assert c(grid=4, **later) == E_ARG and "aligned to their elements" in err()
        for off in (4, 8):
            assert c(frames=off) == E_ARG and "d_frames must be 16-byte aligned" in err(), off
        assert c(grid_bytes=0) == E_ARG and "grid_bytes" in err()
        assert c(frames=4, grid_bytes=0) == E_ARG and "d_frames" in err()
        assert c(n=0, grid_bytes=0, points=None, frames=None, nb=None) == E_NO_DEVICE, "n == 0: grid_bytes is not looked at"
    else:
        assert c(frames=4) == E_NO_DEVICE, "a host form's arrays need no alignment"


# ---- the restatement ----
_cache = {}


def _case(name, k, own):
    """(data, queries, frames, slots, detail, truth) of a cloud queried by its own first 200 points or by the separate list; computed once."""
    key = (name, k, own)
    if key not in _cache:
        data, pts = fref.cloud(name, m=1500, n=200)
        q = data[:200] if own else pts
        fr, sl, det = fref.frames(q, data, k, skip_same_index=False, detail=True)
        for a in (data, q, fr, sl):
            a.setflags(write=False)
        _cache[key] = (data, q, fr, sl, det, fref.truth(sl, data))
    return _cache[key]


def _all_cases():
    return [(name, k, own) for name in CLOUDS for k in KS for own in (False, True)]


def _lams(fr):
    return np.stack([fr["lambda0"], fr["lambda1"], fr["lambda2"]], 1)


def test_restatement_against_float64():
    worst = dict(c1=0.0, c2=0.0, unit=0.0, angle=0.0, sweeps=0)
    bad = []
    for name, k, own in _all_cases():
        data, q, fr, sl, det, (lam, vec, tr, p) = _case(name, k, own)
        on = fr["used"] > 0
        assert on.sum() >= 150
        p2 = p  # (max |p|^2 over the neighbourhood)
        err = np.abs(_lams(fr).astype(np.float64) - lam).max(1)[on]
        T, P2 = tr[on], p2[on]
        if name == "offset":
            c2 = ((err - MEASURED["c1"] * U * T) / (U * U * P2)).max()
            worst["c2"] = max(worst["c2"], c2)
        else:  # (unit scale: the second term is below 1e-3 of the first)
            worst["c1"] = max(worst["c1"], (err / (U * T + U * U * P2)).max())
        if not (err <= FACTOR * (MEASURED["c1"] * U * T + MEASURED["c2"] * U * U * P2)).all():
            bad.append((name, k, own, "eigenvalues"))
        unit = max(np.abs((fr[f][on].astype(np.float64) ** 2).sum(1) - 1.0).max() for f in ("normal", "tangent_u", "tangent_v")) / U
        worst["unit"] = max(worst["unit"], unit)
        gap = (lam[:, 1] - lam[:, 0]) / np.where(tr > 0, tr, 1.0)
        g = on & (gap > 1e-2)
        if g.any():
            nn, v0 = fr["normal"][g].astype(np.float64), vec[g][:, :, 0]
            ang = np.arcsin(np.minimum(1.0, np.linalg.norm(np.cross(nn, v0), axis=1) / np.linalg.norm(nn, axis=1)))
            worst["angle"] = max(worst["angle"], (ang * gap[g] / (U + U * U * p2[g] / tr[g])).max())
        worst["sweeps"] = max(worst["sweeps"], int(det["sweeps"].max()))
        assert (det["off"][on] == 0).all(), (name, k, own, "an off-diagonal is not zero at the loop's end")
    print("largest values measured:", {k: round(float(v), 3) for k, v in worst.items()})
    assert not bad, bad
    assert worst["unit"] <= FACTOR * MEASURED["unit"] and worst["angle"] <= FACTOR * MEASURED["angle"]
    assert worst["c1"] <= FACTOR * MEASURED["c1"] and worst["c2"] <= FACTOR * MEASURED["c2"]
    assert worst["sweeps"] <= fref.SWEEPS


def test_vectors_match_float64_up_to_sign():
    """Where the three eigenvalues are well apart, each vector is the float64 one up to sign, and the frame is right-handed."""
    data, q, fr, sl, det, (lam, vec, tr, p2) = _case("cube", 8, False)
    sep = np.minimum(lam[:, 1] - lam[:, 0], lam[:, 2] - lam[:, 1]) / tr > 0.05
    assert sep.sum() > 50
    for c, f in enumerate(("normal", "tangent_u", "tangent_v")):
        d = np.abs((fr[f][sep].astype(np.float64) * vec[sep][:, :, c]).sum(1))
        assert (d > 1.0 - 1e-4).all(), f
    F = np.stack([fr["normal"], fr["tangent_u"], fr["tangent_v"]], 1).astype(np.float64)
    assert (np.linalg.det(F[fr["used"] >= 3]) > 0.99).all()


@pytest.mark.parametrize("s", [-40, -8, 8, 40])
def test_restatement_scales_exactly(s):
    base, q0 = fref.scale_case(s)
    fr0, sl0, det0 = fref.frames(q0, base, 8, skip_same_index=True, detail=True)
    frs, sls, _ = fref.frames(np.ldexp(q0, s), np.ldexp(base, s), 8, skip_same_index=True, detail=True)
    ok = fref.in_frame_envelope(det0, s)
    same = (frs["normal"].view(np.uint32) == fr0["normal"].view(np.uint32)).all(1)
    print(f"s = {s}: {ok.sum()} of {len(ok)} queries inside the envelope; outside it {same[~ok].sum()} of {(~ok).sum()} normals are equal too")
    assert ok.mean() >= 0.5, "the envelope leaves too few queries for the case to show anything"
    assert np.array_equal(sls["index"], sl0["index"]) and np.array_equal(sls["dist2"], np.ldexp(sl0["dist2"], 2 * s))
    assert np.array_equal(frs["used"], fr0["used"])
    for f in ("normal", "tangent_u", "tangent_v"):
        assert np.array_equal(frs[f][ok].view(np.uint32), fr0[f][ok].view(np.uint32)), f
    assert np.array_equal(frs["centroid"][ok].view(np.uint32), np.ldexp(fr0["centroid"][ok], s).view(np.uint32))
    assert np.array_equal(_lams(frs)[ok].view(np.uint32), np.ldexp(_lams(fr0)[ok], 2 * s).view(np.uint32))


# ---- the header's host side against the restatement ----
@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx, "a C++ compiler is needed for the stand-alone program"
    exe = str(tmp_path_factory.mktemp("sym3") / "sym3_eigen_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "cg-raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tools", "sym3_eigen_check.cpp"), "-o", exe], check=True)
    return exe


def test_header_gives_the_restatements_bits(solver, tmp_path):
    covs, orients = [], []
    for name in CLOUDS:
        data, q, fr, sl, det, _ = _case(name, 8, False)
        covs.append(det["cov"][fr["used"] > 0])
    cov = np.concatenate(covs)
    rng = np.random.default_rng(3)
    odd = np.array([0.0, -0.0, 1.0, -1.0, 3e38, -3e38, 1e-45, 1e-39, np.inf, -np.inf, np.nan], np.float32)
    cov = np.concatenate([cov, cov[:200] * np.float32(2.0**100), cov[:200] * np.float32(2.0**-100), odd[rng.integers(0, len(odd), (600, 6))],
                          np.zeros((1, 6), np.float32), np.diag([3.0, 1.0, 2.0])[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]][None].astype(np.float32)])
    n = len(cov)
    orient = rng.normal(size=(n, 3)).astype(np.float32)
    orient[::7, 1] = np.nan
    has = (np.arange(n) % 3 != 0).astype(np.float32)
    rec = np.concatenate([cov, has[:, None], orient], 1).astype(np.float32)
    (tmp_path / "in.bin").write_bytes(rec.tobytes())
    subprocess.run([solver, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.float32).reshape(n, 13)
    want = np.zeros((n, 13), np.float32)
    for sel, o in ((has != 0, orient), (has == 0, None)):  # (orientation vectors only where the record says so)
        lam, nrm, tu, tv, sweeps, _ = fref.solve(cov[sel], None if o is None else o[sel])
        want[sel] = np.concatenate([fref._canonical(x) for x in (lam, nrm, tu, tv)] + [sweeps[:, None].astype(np.float32)], 1)
    diff = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
    assert len(diff) == 0, (len(diff), n, rec[diff[0]], got[diff[0]], want[diff[0]])


# ---- exact cases of the restatement ----
def test_plane_points_give_the_plane_normal():
    data, q, fr, sl, det, _ = _case("patch", 8, False)
    assert (fr["used"] == 8).all()
    assert (fr["lambda0"] == 0).all() and (fr["centroid"][:, 2] == 0.5).all()
    assert np.array_equal(fr["normal"], np.tile(np.float32([0, 0, 1]), (len(fr), 1)))
    assert (fr["tangent_v"][:, 2] == 0).all() and (fr["tangent_u"][:, 2] == 0).all()


def test_one_neighbour_and_duplicates():
    data, pts = fref.cloud("cube", m=300, n=40)
    fr, sl = fref.frames(pts, data, 1)
    assert (fr["used"] == 1).all() and np.array_equal(fr["centroid"], data[sl["index"][:, 0]])
    assert (_lams(fr) == 0).all()
    for c, f in enumerate(("normal", "tangent_u", "tangent_v")):
        assert np.array_equal(fr[f], np.tile(np.eye(3, dtype=np.float32)[c], (len(fr), 1))), f
    dup = np.tile(np.float32([0.3, -1.7, 2.5e3]), (9, 1))
    fr, sl = fref.frames(dup[:2], dup, 5)
    assert (fr["used"] == 5).all() and np.array_equal(sl["index"], np.tile(np.arange(5, dtype=np.uint32), (2, 1)))
    assert np.array_equal(fr["centroid"], dup[:2]) and (_lams(fr) == 0).all() and (fr["normal"] == np.float32([1, 0, 0])).all()


def test_diagonal_covariance_is_returned_unrotated():
    lam, nrm, tu, tv, sweeps, off = fref.solve(np.float32([[3, 0, 0, 1, 0, 2], [0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 0, 1]]))
    assert np.array_equal(lam, np.float32([[1, 2, 3], [0, 0, 0], [1, 1, 1]])) and (sweeps == 1).all()
    assert np.array_equal(nrm[0], np.float32([0, 1, 0])) and np.array_equal(tu[0], np.float32([0, 0, 1]))
    assert np.array_equal(tv[0], np.float32([1, 0, 0])), "y x z = x: right-handed as it stands"
    for r in (1, 2):  # ties keep column order
        assert np.array_equal(np.stack([nrm[r], tu[r], tv[r]]), np.eye(3, dtype=np.float32))


def test_orientation_and_canonical_nan():
    data, q, fr, sl, det, _ = _case("shell", 8, False)
    o = -q.copy()  # (towards the centre of the shell)
    o[::5, 0] = np.nan
    fro, _ = fref.frames(q, data, 8, orient=o, slots=sl)
    dots = (fr["normal"].astype(np.float64) * o).sum(1)
    flip = np.isfinite(o).all(1) & (fref._dot(fr["normal"], o) < 0)
    assert flip.sum() > 50 and (~flip).sum() > 50 and (flip == (np.nan_to_num(dots) < 0))[np.abs(np.nan_to_num(dots)) > 1e-3].all()
    assert np.array_equal(fro["normal"][flip], -fr["normal"][flip]) and np.array_equal(fro["normal"][~flip], fr["normal"][~flip])
    assert np.array_equal(fro["tangent_u"], fr["tangent_u"]) and np.array_equal(fro["tangent_v"][flip], -fr["tangent_v"][flip])
    big = np.ldexp(np.random.default_rng(2).random((50, 3)).astype(np.float32), 100)  # e e overflows: inf, then NaN
    frb, _ = fref.frames(big[:10], big, 6)
    words = frb.view(np.uint32).reshape(-1, 16)
    nan = np.isnan(words.view(np.float32))
    nan[:, 3] = False
    assert nan.any() and (words[nan] == fref.CANONICAL_NAN).all()
    empty, _ = fref.frames(np.float32([[np.nan, 0, 0], [0, 0, 0]]), big, 4, radius2=np.float32([1.0, -1.0]))
    assert not empty.view(np.uint8).any()
