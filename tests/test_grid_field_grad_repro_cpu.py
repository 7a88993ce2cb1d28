"""No GPU: the bitwise-reproducible form of the sampler's adjoint (cgrt_sample_grid_grad_repro*; include/cgrt.h "Grid fields, the
bitwise-reproducible form of the sampler's adjoint").

* The three entries are exported, the Python methods exist and carry the keyword; the workspace is 12 nx ny nz bytes.
* The argument checks come in the documented order on a host-only scene, for both forms: the float twin's, then the workspace's
  (device form; skipped with n == 0), ending in CGRT_E_NO_DEVICE.
* The restatement alone (tests/grid_field_grad_repro_ref.py, which the GPU tests compare with): S at its thresholds; a permutation of the
  points gives the same bytes; the float form's bound gamma(m + 1) S_abs + (m + 1) 2^-126 for every element, none excluded; on the exact
  family the result is the sequential f32 sum; zero contributions leave a -0 and a NaN payload in place; the non-finite rules; a term more
  than 24 + S binades below E truncates to 0 and its element is still touched; the 2^k scaling of the grads.
* The stand-alone checker (tools/grid_field_grad_repro_check.cpp), compiled here from the kernels' own headers by a C++ compiler that is
  not hipcc, gives the restatement's bytes and passes its self-test."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import grid_field_grad_ref as aref
import grid_field_grad_repro_ref as rref

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_sample_grid_grad_repro_workspace", "cgrt_sample_grid_grad_repro", "cgrt_sample_grid_grad_repro_device")
KEYWORD = ("sample_grid_grad", "sample_grid_grad_device", "sample_grid_grad_tensor", "splat_grid_tensor", "sample_grid_tensor")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
COMBOS = {"value": (True, False), "gradient": (False, True), "both": (True, True)}
SNAN, QNAN, NEG0, SENTINEL = 0x7FA00001, 0x7FC00000, 0x80000000, 0xA5A5A5A5
ids = lambda d: "x".join(map(str, d))  # noqa: E731


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    assert callable(getattr(pkg.Scene, "sample_grid_grad_repro_workspace", None))
    for name in KEYWORD:
        sig = inspect.signature(getattr(pkg.Scene, name))
        assert sig.parameters["reproducible"].default is False, name
    sig = inspect.signature(pkg.Scene.sample_grid_grad_device)
    assert sig.parameters["d_workspace_ptr"].default == 0 and sig.parameters["workspace_bytes"].default == 0


# ---- the workspace and the argument checks, on a host-only scene ----
@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


def test_workspace_is_twelve_bytes_per_element(pkg, host_scene):
    for dims in ((2, 2, 2), (3, 2, 2), (17, 9, 5), (256, 256, 256), (1 << 11, 1 << 10, (1 << 10) - 1)):
        assert host_scene.sample_grid_grad_repro_workspace((0, 0, 0), (1.0, -0.5, 2.0), dims) == 12 * dims[0] * dims[1] * dims[2], dims
    L = pkg.lib()
    b = C.c_uint64(7)
    g = pkg.Grid()
    g.origin[:], g.spacing[:], g.dims[:] = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (4, 3, 2)
    assert L.cgrt_sample_grid_grad_repro_workspace(None, C.byref(g), C.byref(b)) == E_ARG
    assert L.cgrt_sample_grid_grad_repro_workspace(host_scene._h, None, C.byref(b)) == E_ARG
    assert L.cgrt_sample_grid_grad_repro_workspace(host_scene._h, C.byref(g), None) == E_ARG
    for bad in (dict(dims=(1, 5, 5)), dict(dims=(1 << 11, 1 << 10, 1 << 10)), dict(spacing=(1.0, 0.0, 1.0)), dict(origin=(0.0, float("nan"), 0.0))):
        h = pkg.Grid()
        h.origin[:], h.spacing[:], h.dims[:] = bad.get("origin", (0.0, 0.0, 0.0)), bad.get("spacing", (1.0, 1.0, 1.0)), bad.get("dims", (4, 3, 2))
        assert L.cgrt_sample_grid_grad_repro_workspace(host_scene._h, C.byref(h), C.byref(b)) == E_ARG and "grid" in L.cgrt_last_error().decode(), bad
    assert b.value == 7, "a refused call reports nothing"


_BUF = np.zeros(256, np.uint64)  # (never touched: the scene is host-only); 8-byte aligned
NEED = 12 * 4 * 3 * 2


def _p(off):
    return None if off is None else C.c_void_p(_BUF.ctypes.data + off)


def _call(pkg, sc, form, handle="ok", grid="ok", dims=(4, 3, 2), origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), params="ok", flags=0,
          points=0, n=2, gv=0, gg=0, out=0, ws=512, ws_bytes=NEED):
    """form: host / device.  points / gv / gg / out / ws: byte offsets into _BUF, None for NULL."""
    L = pkg.lib()
    h = sc._h if handle == "ok" else None
    g = None
    if grid is not None:
        gs = pkg.Grid()
        gs.origin[:], gs.spacing[:], gs.dims[:] = origin, spacing, dims
        g = C.byref(gs)
    q = None
    if params is not None:
        prm = pkg.FieldParams()
        prm.outside, prm.flags = 0.0, flags
        q = C.byref(prm)
    a = (h, g, _p(points), n, q, _p(gv), _p(gg), _p(out))
    return L.cgrt_sample_grid_grad_repro(*a) if form == "host" else L.cgrt_sample_grid_grad_repro_device(*a, _p(ws), ws_bytes, None)


FORMS = ["host", "device"]
# every later step is broken in each call: the step under test is the one that is reported
BROKEN = {
    1: dict(flags=2, points=None, gv=None, gg=None, out=None, n=1 << 40, ws=None),
    2: dict(flags=2, points=None, gv=None, gg=None, out=None, n=1 << 40, ws=None),
    3: dict(points=None, gv=None, gg=None, out=None, n=1 << 40, ws=None),
    4: dict(gv=None, gg=None, out=None, n=1 << 40, ws=None),
    5: dict(out=None, n=1 << 40, ws=None),
    6: dict(n=1 << 40, ws=None),
    7: dict(ws=None),
    8: dict(ws=None),
}


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


@pytest.mark.parametrize("form", FORMS)
def test_valid_calls_end_in_no_device(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(flags=1) == E_NO_DEVICE and c(params=None) == E_NO_DEVICE, "NULL parameters mean flags 0"
    assert c(spacing=(1.0, -0.5, 2.0)) == E_NO_DEVICE and c(dims=(2, 2, 2)) == E_NO_DEVICE
    assert c(gv=None) == E_NO_DEVICE and c(gg=None) == E_NO_DEVICE, "one of the two grads is enough"
    assert c(n=0, points=None) == E_NO_DEVICE, "n == 0 passes every argument check"
    assert c(n=0, points=None, ws=None, ws_bytes=0) == E_NO_DEVICE and c(n=0, ws=513, ws_bytes=1) == E_NO_DEVICE, "n == 0 skips the workspace's"
    assert c(n=(1 << 31) - 1) == E_NO_DEVICE
    assert c(ws_bytes=NEED + 1000) == E_NO_DEVICE, "a larger workspace is fine"


@pytest.mark.parametrize("form", FORMS)
def test_checks_of_the_float_twin_come_first_and_in_its_order(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    assert c(handle=None, dims=(0, 1, 1), **BROKEN[1]) == E_ARG and "NULL" in _err(pkg)
    assert c(grid=None, **BROKEN[1]) == E_ARG and "NULL" in _err(pkg)
    for kw in (dict(dims=(1, 5, 5)), dict(dims=((1 << 24) + 1, 2, 2)), dict(dims=(1 << 11, 1 << 10, 1 << 10)), dict(origin=(0.0, float("nan"), 0.0)),
               dict(spacing=(1.0, 1.0, float("inf"))), dict(spacing=(1.0, 0.0, 1.0))):
        assert c(**kw, **BROKEN[2]) == E_ARG and "grid" in _err(pkg), kw
    assert c(flags=2, **BROKEN[3]) == E_ARG and "flags" in _err(pkg)
    assert c(points=None, **BROKEN[4]) == E_ARG and "points" in _err(pkg)
    assert c(gv=None, gg=None, **BROKEN[5]) == E_ARG and "grad_value" in _err(pkg) and "grad_values" not in _err(pkg)
    assert c(gv=None, gg=None, n=0, points=None) == E_ARG, "also with n == 0"
    assert c(out=None, **BROKEN[6]) == E_ARG and "grad_values" in _err(pkg)
    assert c(n=1 << 31, points=1 if form == "device" else 0, **BROKEN[7]) == E_ARG and "0x7fffffff" in _err(pkg)
    for kw in (dict(points=1), dict(gv=2), dict(gg=3), dict(out=2)):
        assert c(**kw, **BROKEN[8]) == (E_ARG if form == "device" else E_NO_DEVICE), kw
        assert form == "host" or ("aligned" in _err(pkg) and "workspace" not in _err(pkg))


def test_then_the_workspace_then_the_host_only_scene(pkg, host_scene):
    c = lambda **kw: _call(pkg, host_scene, "device", **kw)  # noqa: E731
    assert c(ws=None) == E_ARG and "workspace" in _err(pkg), "NULL"
    assert c(ws=516) == E_ARG and "8-byte" in _err(pkg), "4-byte aligned is not enough"
    assert c(ws=513) == E_ARG and "8-byte" in _err(pkg)
    assert c(ws_bytes=NEED - 1) == E_ARG and "workspace_bytes" in _err(pkg), "one byte short"
    assert c(ws_bytes=0) == E_ARG
    assert c(ws=None, ws_bytes=0, dims=(17, 9, 5)) == E_ARG
    assert c(dims=(17, 9, 5)) == E_ARG and "workspace_bytes" in _err(pkg), "the size follows the grid"
    assert c(ws_bytes=NEED) == E_NO_DEVICE
    assert not _BUF.any()


# ---- the restatement alone ----
def test_shift_at_its_thresholds():
    assert [rref.shift(n) for n in (1, 16383, 16384, 0x7FFFFFFF)] == [24, 24, 23, 7]
    assert rref.shift(70000) == 21 and rref.shift(20000) == 23 and rref.shift(4099) == 24


def _noise_case(dims, n=4099):
    o, sp = aref.noise_grid(dims)
    p = aref.mixed_points(dims, o, sp, n)
    gv, gg = aref.noise_grads(n)
    return o, sp, p, gv, gg


def test_a_permutation_of_the_points_gives_the_same_bytes():
    dims = (17, 9, 5)
    o, sp, p, gv, gg = _noise_case(dims)
    prev = aref.noise_previous(dims)
    want = rref.adjoint(o, sp, dims, p, gv, gg, previous=prev)
    assert want.tobytes() != prev.tobytes()
    rng = np.random.default_rng(11)
    for _ in range(3):
        order = rng.permutation(len(p))
        assert rref.adjoint(o, sp, dims, p[order], gv[order], gg[order], previous=prev).tobytes() == want.tobytes()
    o, sp, dims, p, gv, gg, prev = rref.pile_up(20000)
    want = rref.adjoint(o, sp, dims, p, gv, gg, previous=prev)
    order = rng.permutation(len(p))
    assert rref.adjoint(o, sp, dims, p[order], gv[order], gg[order], previous=prev).tobytes() == want.tobytes()
    assert want.tobytes() != aref.adjoint(o, sp, dims, p, gv, gg, previous=prev)["sequential"].tobytes(), "where the sequential f32 sum rounds otherwise"


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 2, 2), (17, 9, 5)], ids=ids)
def test_the_float_forms_bound_holds_for_every_element(dims, combo):
    """gamma(m + 1) S_abs + (m + 1) 2^-126 against the float64 sum of the float32 contributions, every element, none excluded
    (grid_field_grad_ref.check also holds elements with m = 0 to their previous bits)."""
    use_v, use_g = COMBOS[combo]
    prev = aref.noise_previous(dims)
    worst = 0.0
    for n in (65, 4099):
        o, sp, p, gv, gg = _noise_case(dims, n)  # (the y spacing is negative)
        a, b = (gv if use_v else None), (gg if use_g else None)
        for clamp in (False, True):
            res = aref.adjoint(o, sp, dims, p, a, b, clamp=clamp, previous=prev)
            got = rref.adjoint(o, sp, dims, p, a, b, clamp=clamp, previous=prev)
            worst = max(worst, aref.check(got, res, prev, what=(dims, combo, n, clamp)))
    print(f"largest error / bound, {dims} {combo}: {worst:.4f}")
    o, sp, dims2, p, gv, gg, prev = rref.pile_up(20000)
    if dims == dims2:  # the pile-up too: m = 20 000 per element, S = 23
        a, b = (gv if use_v else None), (gg if use_g else None)
        ratio = aref.check(rref.adjoint(o, sp, dims, p, a, b, previous=prev), aref.adjoint(o, sp, dims, p, a, b, previous=prev), prev)
        print(f"largest error / bound, pile-up {combo}: {ratio:.6f}")


@pytest.mark.parametrize("k", [-1, 0, 1])
@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 2, 2), (17, 9, 5)], ids=ids)
def test_exact_family_equals_the_sequential_sum(dims, k):
    o, sp, p, gv, gg, prev = aref.exact_family(dims, k)
    for use_v, use_g in COMBOS.values():
        a, b = (gv if use_v else None), (gg if use_g else None)
        res = aref.adjoint(o, sp, dims, p, a, b, previous=prev)
        assert res["S"].max() < 2.0 ** 12
        assert rref.adjoint(o, sp, dims, p, a, b, previous=prev).tobytes() == res["sequential"].tobytes(), (dims, k, use_v, use_g)


def _grid_points_case():
    dims = (5, 4, 3)
    o, sp = np.asarray([-1.0, 1.0, 0.0], F), np.asarray([0.5, -0.25, 2.0], F)
    ix, iy, iz = np.meshgrid(np.arange(0, 5, 2), np.arange(0, 4, 3), np.arange(3), indexing="ij")
    grid_pts = np.stack([ix, iy, iz], axis=-1).reshape(-1, 3)
    p = (o + grid_pts.astype(F) * sp).astype(F)
    return dims, o, sp, grid_pts, p


def test_zero_contributions_leave_minus_zero_and_a_nan_payload_in_place():
    dims, o, sp, grid_pts, p = _grid_points_case()
    gv = (np.arange(len(p)) + 1).astype(F)
    for pattern in (NEG0, SNAN, SENTINEL):
        prev = np.full(dims[::-1], pattern, np.uint32).view(F)
        got = rref.adjoint(o, sp, dims, p, gv, None, previous=prev).view(np.uint32)
        touched = np.zeros(dims[::-1], bool)
        touched[grid_pts[:, 2], grid_pts[:, 1], grid_pts[:, 0]] = True
        assert touched.sum() == len(p), "a point on a grid point with grad_value alone touches one element"
        assert (got[~touched] == pattern).all(), hex(pattern)
        assert (got[touched] != pattern).all()
        # zero grads contribute zeros, which are not contributions: nothing is touched
        got = rref.adjoint(o, sp, dims, p, np.zeros(len(p), F), np.zeros((len(p), 3), F), previous=prev).view(np.uint32)
        assert (got == pattern).all()
    prev = np.full(dims[::-1], NEG0, np.uint32).view(F)
    got = rref.adjoint(o, sp, dims, p, gv, None, previous=prev)
    assert np.array_equal(got[grid_pts[:, 2], grid_pts[:, 1], grid_pts[:, 0]], gv)


def test_non_finite_rules():
    o, sp, dims = np.zeros(3, F), np.ones(3, F), (4, 3, 2)
    mid = np.asarray([[0.5, 0.5, 0.5]], F)  # all eight weights are 1/8
    inf, nan = np.inf, np.nan
    cell = (slice(0, 2), slice(0, 2), slice(0, 2))
    prev = np.full(dims[::-1], 2.0, F)
    for grads, want in (([inf], inf), ([-inf], -inf), ([inf, -inf], nan), ([nan], nan), ([inf, nan], nan), ([inf, 1.0, -3.0], inf)):
        p = np.repeat(mid, len(grads), axis=0)
        got = rref.adjoint(o, sp, dims, p, np.asarray(grads, F), None, previous=prev)
        if np.isnan(want):
            assert (got[cell].view(np.uint32) == QNAN).all(), grads
        else:
            assert (got[cell] == want).all(), grads
        untouched = np.ones(dims[::-1], bool)
        untouched[cell] = False
        assert (got[untouched] == 2.0).all()
    # the previous content takes part: +inf stored, -inf arriving
    got = rref.adjoint(o, sp, dims, mid, np.asarray([-inf], F), None, previous=np.full(dims[::-1], inf, F))
    assert (got[cell].view(np.uint32) == QNAN).all()
    # a signalling NaN stored and a finite contribution: the one quiet NaN
    got = rref.adjoint(o, sp, dims, mid, np.asarray([1.0], F), None, previous=np.full(dims[::-1], SNAN, np.uint32).view(F))
    assert (got[cell].view(np.uint32) == QNAN).all() and (got.view(np.uint32)[:, :, 2:] == SNAN).all()
    # a NaN grad on an outside point stays out
    p = np.asarray([[0.5, 0.5, 0.5], [9.0, 0.5, 0.5]], F)
    got = rref.adjoint(o, sp, dims, p, np.asarray([8.0, nan], F), np.asarray([[0, 0, 0], [nan, inf, 0]], F), previous=prev)
    assert not np.isnan(got).any() and (got[cell] == 3.0).all()


def test_a_term_far_below_the_largest_truncates_to_zero_and_cancelled_elements_are_still_touched():
    o, sp, dims = np.zeros(3, F), np.ones(3, F), (4, 3, 2)
    at = np.asarray([[1.0, 1.0, 1.0]], F)  # a grid point: one element
    tiny = F(2.0 ** -60)
    assert rref.shift(2) == 24
    big = terms_of([1.0, tiny])
    assert big.tolist() == [1 << 47, 0], "d = 60 >= 24 + S: the shift reaches 24"
    prev = np.full(dims[::-1], NEG0, np.uint32).view(F)
    got = rref.adjoint(o, sp, dims, np.repeat(at, 2, axis=0), np.asarray([1.0, tiny], F), None, previous=prev)
    assert got[1, 1, 1] == 1.0 and (np.delete(got.view(np.uint32).reshape(-1), (1 * 3 + 1) * 4 + 1) == NEG0).all()
    alone = rref.adjoint(o, sp, dims, at, np.asarray([tiny], F), None, previous=prev)
    assert alone[1, 1, 1] == tiny, "alone it is the largest and exact"
    # d = 24 + S - 1 still leaves the top bit; one binade more and nothing is left
    assert terms_of([1.0, 2.0 ** -47]).tolist() == [1 << 47, 1] and terms_of([1.0, 2.0 ** -48]).tolist() == [1 << 47, 0]
    assert terms_of([1.0, -1.5 * 2.0 ** -47]).tolist() == [1 << 47, -1], "the magnitude is truncated, towards zero"
    # +x and -x: I = 0, and the element is still touched: a stored -0 becomes fl32(fl64(-0) + 0) = +0
    got = rref.adjoint(o, sp, dims, np.repeat(at, 2, axis=0), np.asarray([3.0, -3.0], F), None, previous=prev)
    assert got.view(np.uint32)[1, 1, 1] == 0 and (got.view(np.uint32) == NEG0).sum() == 23


def terms_of(x, S=24):
    x = np.asarray(x, F)
    ef = (x.view(np.uint32).astype(np.int64) >> 23) & 0xFF
    return rref.terms(x, np.full(len(x), np.maximum(ef, 1).max()), S)


@pytest.mark.parametrize("k", [-8, 8])
def test_scaling_the_grads_scales_the_result(k):
    dims = (17, 9, 5)
    o, sp, p, gv, gg = _noise_case(dims)
    s = F(2.0 ** k)
    for use_v, use_g in COMBOS.values():
        one = rref.adjoint(o, sp, dims, p, gv if use_v else None, gg if use_g else None)
        big = rref.adjoint(o, sp, dims, p, gv * s if use_v else None, gg * s if use_g else None)
        assert np.abs(one[one != 0]).min() * min(s, 1) > 2.0 ** -126, "inside the normal range"
        assert (one * s).tobytes() == big.tobytes(), (k, use_v, use_g)


# ---- the stand-alone checker ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("grid_field_grad_repro_check") / "grid_field_grad_repro_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "cg-raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tools", "grid_field_grad_repro_check.cpp"), "-o", exe], check=True)
    return exe


def _write_grid(path, values, origin, spacing):
    nz, ny, nx = values.shape
    with open(path, "wb") as f:
        f.write(np.asarray([nx, ny, nz], np.uint32).tobytes())
        f.write(np.asarray(origin, F).tobytes() + np.asarray(spacing, F).tobytes())
        f.write(np.ascontiguousarray(values, F).tobytes())


def _run_checker(checker, tmp_path, o, sp, p, gv, gg, prev, clamp):
    _write_grid(tmp_path / "grid.bin", prev, o, sp)
    p.tofile(tmp_path / "points.bin")
    if gv is not None:
        gv.tofile(tmp_path / "gv.bin")
    if gg is not None:
        gg.tofile(tmp_path / "gg.bin")
    subprocess.run([checker, "adjoint", str(tmp_path / "grid.bin"), str(tmp_path / "points.bin"), str(tmp_path / "gv.bin") if gv is not None else "-",
                    str(tmp_path / "gg.bin") if gg is not None else "-", str(tmp_path / "out.bin"), str(int(clamp))], check=True)
    return np.fromfile(tmp_path / "out.bin", F).reshape(prev.shape)


def test_checker_self_test(checker):
    r = subprocess.run([checker, "--self-test"], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


def test_checker_writes_the_restatements_bytes(checker, tmp_path):
    dims = (17, 9, 5)
    o, sp, p, gv, gg = _noise_case(dims)  # n = 4099
    gv, gg = gv.copy(), gg.copy()
    gv[5::97], gg[7::89, 1] = np.nan, np.inf  # (at inside and at outside points)
    prev = aref.noise_previous(dims)
    for use_v, use_g in COMBOS.values():
        a, b = (gv if use_v else None), (gg if use_g else None)
        for clamp in (False, True):
            got = _run_checker(checker, tmp_path, o, sp, p, a, b, prev, clamp)
            assert got.tobytes() == rref.adjoint(o, sp, dims, p, a, b, clamp=clamp, previous=prev).tobytes(), (use_v, use_g, clamp)
    o, sp, dims, p, gv, gg, prev = rref.pile_up(20000)  # one cell of 2 x 2 x 2: S = 23, m = 20 000
    assert rref.shift(len(p)) == 23
    for use_v, use_g in COMBOS.values():
        a, b = (gv if use_v else None), (gg if use_g else None)
        got = _run_checker(checker, tmp_path, o, sp, p, a, b, prev, False)
        assert got.tobytes() == rref.adjoint(o, sp, dims, p, a, b, previous=prev).tobytes(), ("pile-up", use_v, use_g)
