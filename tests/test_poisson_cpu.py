"""No GPU: Poisson-disk sets (cgrt_poisson_disk*; include/cgrt.h "Poisson-disk sets").

* The five entries are exported, the Python methods exist, CgrtPoissonParams is 24 bytes.
* The argument checks come in the documented order on a host-only scene, ending in CGRT_E_NO_DEVICE.
* Philox word 3 (the order word) against the header's known answer, 9b00dbd8 for the zero counter and key.
* The restatement (tests/poisson_ref.py, which the GPU tests compare bytes with): its synchronous-round form equals its sequential form,
  and both give independent, maximal sets, on seeded clouds, with and without a priority, with non-finite points mixed in.
* Two fixed cases: 512 points on a line at spacing 0.6, min_dist2 = 1, priority = index -- the 256 even indices, 512 synchronous rounds;
  an 8^3 lattice of spacing 0.25 -- nothing conflicts at min_dist2 = 0.0625 (strictly less), every interior point has 6 conflicts at the
  next float above."""
import ctypes as C

import numpy as np
import pytest

import poisson_ref as pref
import sampling_ref as sref

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_poisson_disk", "cgrt_poisson_disk_device", "cgrt_poisson_disk_workspace", "cgrt_poisson_disk_brute", "cgrt_debug_poisson_work")
METHODS = ("poisson_disk", "poisson_disk_device", "poisson_disk_tensor", "poisson_disk_brute", "debug_poisson_work", "poisson_disk_workspace",
           "sample_surface_poisson_tensor")


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    for name in METHODS:
        assert callable(getattr(pkg.Scene, name, None)), name
    assert C.sizeof(pkg.PoissonParams) == 24
    assert [getattr(pkg.PoissonParams, k).offset for k in ("min_dist2", "seed", "priority")] == [0, 8, 16]


# ---- the argument checks, on a host-only scene ----
@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


N = 16
_PTS = np.zeros(N * 3 + 4, np.float32)
_KEEP = np.zeros(N + 8, np.uint8)
_PRIO = np.zeros(N + 4, np.uint32)
_WS = np.zeros(1 << 16, np.uint8)  # (more than the workspace of 16 points; never touched: the scene is host-only)


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


def _call(pkg, sc, device, handle="ok", n=N, params="ok", m=1.0, points=0, keep=0, prio=None, ws=0, ws_bytes=None, entry=None):
    """points / keep / prio / ws: a byte offset into the module's arrays, or None for NULL."""
    p = lambda a, off: None if off is None else C.c_void_p(a.ctypes.data + off)  # noqa: E731
    prm = None
    if params is not None:
        prm = pkg.PoissonParams()
        prm.min_dist2, prm.seed, prm.priority = m, 3, (None if prio is None else _PRIO.ctypes.data + prio)
        prm = C.byref(prm)
    kept = C.c_uint64(77)
    args = [sc._h if handle == "ok" else None, p(_PTS, points), n, prm, p(_KEEP, keep), C.byref(kept)]
    L = pkg.lib()
    if device:
        base = (-_WS.ctypes.data) % 8  # the array's first 8-byte boundary
        need = C.c_uint64(0)
        assert L.cgrt_poisson_disk_workspace(sc._h, min(n, 0x7FFFFFFF), C.byref(need)) == 0
        rc = L.cgrt_poisson_disk_device(*args, p(_WS, None if ws is None else base + ws), need.value if ws_bytes is None else ws_bytes, None)
    else:
        rc = getattr(L, entry or "cgrt_poisson_disk")(*args)
    return rc, kept.value


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_argument_checks_and_their_order(pkg, host_scene, device):
    c = lambda **kw: _call(pkg, host_scene, device, **kw)[0]  # noqa: E731
    inf, nan = float("inf"), float("nan")
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    for m in (0.0, -1.0, nan, -inf, 3e38):
        assert c(m=m) == E_NO_DEVICE, m
    assert c(n=0, points=None, keep=None, ws=None) == E_NO_DEVICE and c(prio=0) == E_NO_DEVICE and c(n=0x7FFFFFFF, ws_bytes=1 << 62) == E_NO_DEVICE
    # 1 .. 6, each with every later check failing too
    assert c(handle=None, points=None, n=1 << 31, m=inf, ws=None) == E_ARG and "scene" in _err(pkg)
    assert c(params=None, points=None, n=1 << 31, ws=None) == E_ARG and "params" in _err(pkg)
    assert c(points=None, n=1 << 31, m=inf, prio=2, ws=None) == E_ARG and "NULL" in _err(pkg)
    assert c(keep=None, n=1 << 31, m=inf, prio=2, ws=None) == E_ARG and "NULL" in _err(pkg)
    assert c(n=1 << 31, m=inf, prio=2, ws=None) == E_ARG and "too many" in _err(pkg)
    assert c(m=inf, prio=2, points=2, ws=None) == E_ARG and "+inf" in _err(pkg)
    if device:
        assert c(points=2, ws=None) == E_ARG and "4-byte" in _err(pkg)
        assert c(prio=2, ws=None) == E_ARG and "4-byte" in _err(pkg)
        assert c(ws=None, ws_bytes=0) == E_ARG and "NULL" in _err(pkg)
        assert c(ws=4, ws_bytes=0) == E_ARG and "8-byte" in _err(pkg)
        need = C.c_uint64(0)
        assert pkg.lib().cgrt_poisson_disk_workspace(host_scene._h, N, C.byref(need)) == 0 and need.value % 8 == 0
        assert c(ws_bytes=need.value - 1) == E_ARG and "workspace_bytes" in _err(pkg)
        assert c(keep=1) == E_NO_DEVICE, "the flags are bytes: no alignment"
    else:
        assert c(points=2, prio=2) == E_NO_DEVICE, "host pointers need no alignment"
        for entry in ("cgrt_poisson_disk_brute",):
            assert c(entry=entry) == E_NO_DEVICE and c(entry=entry, m=inf) == E_ARG
    w = np.zeros(6, np.uint64)
    prm = pkg.PoissonParams()
    prm.min_dist2 = 1.0
    assert pkg.lib().cgrt_debug_poisson_work(host_scene._h, C.c_void_p(_PTS.ctypes.data), N, C.byref(prm), C.c_void_p(w.ctypes.data)) == E_NO_DEVICE
    assert pkg.lib().cgrt_debug_poisson_work(host_scene._h, C.c_void_p(_PTS.ctypes.data), N, C.byref(prm), None) == E_ARG
    assert _call(pkg, host_scene, device)[1] == 77, "*kept is not written by a call that fails"


def test_workspace_size(pkg, host_scene):
    L = pkg.lib()
    b = C.c_uint64(0)
    assert L.cgrt_poisson_disk_workspace(None, 1, C.byref(b)) == E_ARG and L.cgrt_poisson_disk_workspace(host_scene._h, 1, None) == E_ARG
    assert L.cgrt_poisson_disk_workspace(host_scene._h, 1 << 31, C.byref(b)) == E_ARG
    sizes = [host_scene.poisson_disk_workspace(n) for n in (0, 1, 1000, 1 << 20, 0x7FFFFFFF)]
    assert sizes == sorted(sizes) and all(s % 8 == 0 for s in sizes)
    assert 40 * (1 << 20) <= sizes[3] <= 48 * (1 << 20), "about 41 bytes per point"


def test_order_word_is_philox_word_3():
    assert int(pref.order_words(1, seed=0)[0]) == 0x9B00DBD8
    for seed, i in ((0, 5), (1, 0), ((1 << 63) + 5, 4096), (0xDEADBEEF12345678, 77)):
        want = sref.philox_python([i, 0, 0, 0], [seed & 0xFFFFFFFF, seed >> 32])[3]
        assert int(pref.order_words(i + 1, seed=seed)[i]) == want
    k = pref.keys(3, priority=[7, 7, 0])
    assert [int(x) for x in k] == [7 << 32, (7 << 32) | 1, 2]


def _cloud(rng, n, bad=0):
    p = rng.random((n, 3)).astype(np.float32)
    if bad:
        idx = rng.choice(n, bad, replace=False)
        p[idx, rng.integers(0, 3, bad)] = rng.choice(np.asarray([np.nan, np.inf, -np.inf], np.float32), bad)
    return p


@pytest.mark.parametrize("n, k", [(1, 1), (2, 1), (65, 10), (700, 1), (700, 10), (700, 100)])
def test_round_form_equals_the_sequential_form_and_the_set_is_maximal(n, k):
    rng = np.random.default_rng(1000 * n + k)
    p = _cloud(rng, n, bad=n // 20)
    m = np.float32((k / n / (4.0 / 3.0 * np.pi)) ** (2.0 / 3.0))  # a ball of this radius holds k of n uniform points
    d2 = pref.d2_matrix(p)
    assert np.array_equal(d2, d2.T, equal_nan=True), "d2 is symmetric"
    for seed, prio in ((0, None), (5, None), (0, rng.integers(0, 4, n).astype(np.uint32)), (0, np.zeros(n, np.uint32))):
        seq = pref.greedy(p, m, seed, prio, d2)
        par, count = pref.rounds(p, m, seed, prio, d2)
        assert np.array_equal(seq, par), (seed, prio is None)
        pref.check_set(p, m, seq, seed, prio, d2)
        assert 1 <= count <= n
    for none in (0.0, -1.0, np.nan):
        assert np.array_equal(pref.greedy(p, none, d2=d2), pref.finite(p))


def test_line_case():
    p, m, prio = pref.line_case()
    seq = pref.greedy(p, m, priority=prio)
    par, count = pref.rounds(p, m, priority=prio)
    assert np.array_equal(seq, par) and count == 512
    assert np.array_equal(np.flatnonzero(seq), np.arange(0, 512, 2)) and seq.sum() == 256


def test_lattice_case():
    p = pref.lattice_case()
    assert len(p) == 512
    m = np.float32(0.0625)
    assert not pref.conflicts(p, m).any(), "strictly less: a neighbour at exactly the radius does not conflict"
    assert pref.greedy(p, m).all() and pref.rounds(p, m)[0].all()
    up = np.nextafter(m, np.float32(1))
    c = pref.conflicts(p, up)
    interior = ((p > 0) & (p < 1.75)).all(1)
    assert interior.sum() == 216 and (c.sum(1)[interior] == 6).all() and c.sum() == 2 * 3 * 7 * 64
    keep = pref.greedy(p, up, seed=3)
    pref.check_set(p, up, keep, seed=3)
    assert np.array_equal(keep, pref.rounds(p, up, seed=3)[0])
