"""No GPU: surface sampling (cgrt_sample_surface*; include/cgrt.h "Surface sampling").

* The four entries are exported, CgrtSurfaceSample is 32 bytes with point / prim_id / bary at CgrtClosest's offsets, and the argument
  checks come in the documented order on a host-only scene, ending in CGRT_E_NO_DEVICE.
* The restatement's Philox (tests/sampling_ref.py) gives the three known-answer vectors, and agrees with a Python-integer version.
* cgrt_triangle_areas and cgrt_debug_get_sample_table (host work: they run on a host-only scene) equal the restatement bit for bit on
  cube, cornell, monkey, dodge and a hand-made 8-triangle scene with zero-area triangles first, in the middle and last, a NaN vertex and
  a triangle of about 2^-40 of the total; scenes without a triangle of positive area, or without meshes, have last == NO_PRIM; scaling
  cube and monkey by 2^-20 and 2^+20 leaves thresholds and last unchanged.
* Statistics of the restatement alone (the GPU tests are byte comparisons against it), conditions fixed in advance:
    - independent samples, 2^20, seeds 1..3: chi-square z = (X^2 - dof) / sqrt(2 dof) <= 4 with triangles of expectation < 5 pooled into
      one bin; the mean of each barycentric within 5 standard errors of 1/3 (a uniform point's weight has variance 1/18);
    - stratified, strata = n = 2^20: |count_i - n area_i / A| < 2 for every triangle;
    - every point lies on its triangle: |point - p64|_inf <= 4 * 2^-24 * S against the float64 mix of the same integer weights, S the
      triangle's largest |coordinate| (three product roundings of together at most 2^-24 S, two sum roundings of at most 2^-24 S each,
      one unit for second-order terms)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import sampling_ref as sref

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_sample_surface", "cgrt_sample_surface_device", "cgrt_triangle_areas", "cgrt_debug_get_sample_table")
METHODS = ("triangle_areas", "debug_sample_table", "sample_surface", "sample_surface_device", "sample_surface_tensor")
FIXTURES = ("cube", "cornell", "monkey", "dodge")
NSTAT = 1 << 20


def test_entries_are_exported_and_the_record_is_32_bytes(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    for name in METHODS:
        assert callable(getattr(pkg.Scene, name, None)), name
    d, c = pkg.SURFACE_SAMPLE_DTYPE, pkg.CLOSEST_DTYPE
    assert d.itemsize == 32 and C.sizeof(pkg.SampleParams) == 24
    assert [d.fields[k][1] for k in ("point", "mesh_id", "prim_id", "bary")] == [0, 12, 16, 20]
    for k in ("point", "prim_id", "bary"):
        assert d.fields[k][1] == c.fields[k][1], k
    assert d == sref.SAMPLE_DTYPE


# ---- the argument checks, on a host-only scene ----
@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


N = 16
_OUT = np.zeros(N * 8 + 4, np.float32)
_ATTR = np.zeros(8 * 256 + 4, np.float32)  # (the cube has 8 vertices)
_ROWS = np.zeros(N * 256 + 4, np.float32)


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


def _call(pkg, sc, device, handle="ok", n=N, params="default", out=0, attr=None, channels=3, rows=None):
    """out / attr / rows: a byte offset into the module's arrays, or None for NULL; params: (seed, first, strata), or None for NULL."""
    p = lambda a, off: None if off is None else C.c_void_p(a.ctypes.data + off)  # noqa: E731
    prm = None
    if params is not None:
        prm = pkg.SampleParams()
        prm.seed, prm.first, prm.strata = (0, 0, 0) if isinstance(params, str) else params
        prm = C.byref(prm)
    args = [sc._h if handle == "ok" else None, n, prm, p(_OUT, out), p(_ATTR, attr), channels, p(_ROWS, rows)]
    return pkg.lib().cgrt_sample_surface_device(*args, None) if device else pkg.lib().cgrt_sample_surface(*args)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_argument_checks_and_their_order(pkg, host_scene, device):
    c = lambda **kw: _call(pkg, host_scene, device, **kw)  # noqa: E731
    M = 0xFFFFFFFF
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(params=None) == E_NO_DEVICE, "NULL params: zeros"
    assert c(n=0x7FFFFFFF) == E_NO_DEVICE and c(n=0, out=None) == E_NO_DEVICE
    assert c(attr=0, rows=0) == E_NO_DEVICE and c(attr=0, rows=0, channels=256) == E_NO_DEVICE and c(channels=0) == E_NO_DEVICE, "channels unread without a table"
    assert c(params=(5, 0, M), n=N) == E_NO_DEVICE and c(params=(5, M - N, M)) == E_NO_DEVICE and c(params=(1 << 63, (1 << 64) - N - 1, 0)) == E_NO_DEVICE
    # 1 .. 8, each with every later check failing too where that is possible
    assert c(handle=None, out=None, attr=0) == E_ARG and "scene" in _err(pkg)
    assert c(out=None, attr=0) == E_ARG and "NULL" in _err(pkg)
    assert c(attr=0, n=1 << 31) == E_ARG and "together" in _err(pkg)
    assert c(rows=0, n=1 << 31) == E_ARG and "together" in _err(pkg)
    assert c(n=1 << 31, attr=0, rows=0, channels=0) == E_ARG and "too many" in _err(pkg)
    for ch in (0, 257):
        assert c(attr=0, rows=0, channels=ch, params=(0, 0, 1 << 32)) == E_ARG and "channels" in _err(pkg)
    assert c(n=0x7FFFFFFF, attr=0, rows=0, channels=256, params=(0, 0, 1 << 32)) == E_ARG and "2^40" in _err(pkg)
    assert c(params=(0, 5, 1 << 32)) == E_ARG and "strata exceeds" in _err(pkg)
    assert c(params=(0, M - N + 1, M)) == E_ARG and "first + n" in _err(pkg) and "strata" in _err(pkg)
    assert c(params=(0, (1 << 64) - 1, 7)) == E_ARG and "strata" in _err(pkg), "7 before 8"
    for first in ((1 << 64) - N, (1 << 64) - 1):
        assert c(params=(0, first, 0), out=2) == E_ARG and "overflows" in _err(pkg)
    # 9
    if device:
        for kw in (dict(out=2), dict(attr=2, rows=0), dict(attr=0, rows=2)):
            assert c(**kw) == E_ARG and "aligned" in _err(pkg), kw
    else:
        assert c(out=2) == E_NO_DEVICE


def test_known_answer_vectors_of_philox():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert tuple(int(w[0]) for w in sref.philox4x32_10(ctr, key)) == want
        assert tuple(sref.philox_python(ctr, key)) == want
    g = np.random.default_rng(5)
    ctr = g.integers(0, 1 << 32, (4, 64), dtype=np.uint64)
    key = [int(x) for x in g.integers(0, 1 << 32, 2, dtype=np.uint64)]
    w = sref.philox4x32_10(list(ctr), key)
    for i in range(64):
        assert [int(x[i]) for x in w] == sref.philox_python(ctr[:, i], key)
    # the sampler's use of it: counter {lo(j), hi(j), 0, 0}, key {lo(seed), hi(seed)}
    x, w1, w2 = sref.position_words(3, seed=(7 << 32) | 9, first=(1 << 32) - 1)
    for i, j in enumerate(((1 << 32) - 1, 1 << 32, (1 << 32) + 1)):
        assert [int(x[i]), int(w1[i]), int(w2[i])] == sref.philox_python((j & 0xFFFFFFFF, j >> 32, 0, 0), (9, 7))[:3]


def _scaled(sd, k):
    pn = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6).copy()
    pn[:, 0:3] *= np.float32(2.0 ** k)
    return dataclasses.replace(sd, pos_nrm=pn, name=f"{sd.name}*2^{k}")


def _library_table(pkg, sd):
    sc = pkg.Scene(sd, device=-1)
    try:
        areas, total = sc.triangle_areas()
        tab = sc.debug_sample_table()
        again = sc.debug_sample_table()
    finally:
        sc.close()
    assert np.array_equal(tab["thresholds"], again["thresholds"]) and tab["last"] == again["last"]
    return areas, total, tab["thresholds"], tab["last"]


def _same_table(lib, ref):
    assert np.array_equal(lib[0].view(np.uint32), ref[0].view(np.uint32)), "areas"
    assert np.float64(lib[1]).tobytes() == np.float64(ref[1]).tobytes(), "total"
    assert lib[2].dtype == np.uint32 and np.array_equal(lib[2], ref[2]), "thresholds"
    assert lib[3] == ref[3], "last"


@pytest.mark.parametrize("name", FIXTURES)
def test_areas_and_thresholds_equal_the_restatement(pkg, scene_data, name):
    sd = scene_data(name)
    lib, ref = _library_table(pkg, sd), sref.table(sd)
    _same_table(lib, ref)
    assert (np.diff(lib[2].astype(np.int64)) >= 0).all() and lib[2][lib[3]] == 0xFFFFFFFF and lib[3] < sd.ntris


def test_the_degenerate_scene(pkg):
    sd = sref.degenerate_scene(pkg)
    areas, total, T, last = lib = _library_table(pkg, sd)
    _same_table(lib, sref.table(sd))
    assert [bool(a > 0) for a in areas] == [False, True, True, False, False, True, True, False], "collinear, point and NaN triangles count as 0"
    assert (areas[[0, 3, 4, 7]].view(np.uint32) == 0).all()
    assert last == 6
    assert T[0] == 0 and T[3] == T[2] and T[4] == T[2] and T[7] == T[6] == 0xFFFFFFFF, "a zero-area triangle repeats its predecessor's threshold"
    assert 0 < areas[5] / total < 2.0 ** -39 and T[5] == T[4], "smaller than 2^-32 of the total: its threshold repeats too"
    rec, _ = sref.sample(sd, 1 << 16, seed=3)
    assert set(np.unique(rec["prim_id"])) == {1, 2, 6}
    assert np.array_equal(rec["mesh_id"], np.where(rec["prim_id"] == 6, 1, 0))


def test_scenes_that_are_empty_for_sampling(pkg, scene_data):
    sd = sref.degenerate_scene(pkg)
    tri = np.asarray(sd.tri).reshape(-1, 3)
    flat = dataclasses.replace(sd, tri=tri[[0, 3, 4, 7]].copy(), tri_mesh=np.zeros(4, np.uint32), name="flat")
    for empty in (flat, scene_data("spheres")):
        areas, total, T, last = lib = _library_table(pkg, empty)
        _same_table(lib, sref.table(empty))
        assert last == pkg.NO_PRIM and total == 0.0 and not T.any() and len(T) == empty.ntris
        rec, rows = sref.sample(empty, 5, attr=np.ones((len(empty.pos_nrm), 2), np.float32))
        assert (rec["prim_id"] == pkg.NO_PRIM).all() and (rec["mesh_id"] == 0xFFFFFFFF).all() and not rec["point"].any() and not rows.any()


@pytest.mark.parametrize("name", ["cube", "monkey"])
def test_thresholds_do_not_move_under_a_power_of_two_scale(pkg, scene_data, name):
    sd = scene_data(name)
    base = _library_table(pkg, sd)
    for k in (-20, 20):
        s = _library_table(pkg, _scaled(sd, k))
        assert np.array_equal(s[2], base[2]) and s[3] == base[3], k
        assert np.array_equal(s[0], base[0] * np.float32(4.0 ** k)), "the areas scale exactly"
        r0, _ = sref.sample(sd, 4096, seed=2)
        r1, _ = sref.sample(_scaled(sd, k), 4096, seed=2)
        assert np.array_equal(r0["prim_id"], r1["prim_id"]) and np.array_equal(r0["bary"].view(np.uint32), r1["bary"].view(np.uint32))
        assert np.array_equal((r0["point"] * np.float32(2.0 ** k)).view(np.uint32), r1["point"].view(np.uint32))


# ---- statistics of the restatement ----
@pytest.fixture(scope="module")
def tables(scene_data):
    return {name: sref.table(scene_data(name)) for name in FIXTURES}


@pytest.mark.parametrize("name", FIXTURES)
def test_independent_samples_follow_the_areas(scene_data, tables, name):
    sd, tab = scene_data(name), tables[name]
    a, total = tab[0].astype(np.float64), tab[1]
    expect = NSTAT * a / total
    small = expect < 5
    for seed in (1, 2, 3):
        rec, _ = sref.sample(sd, NSTAT, seed=seed, tab=tab)
        count = np.bincount(rec["prim_id"], minlength=sd.ntris).astype(np.float64)
        assert not count[a == 0].any(), "a zero-area triangle is never chosen"
        obs, exp = list(count[~small]), list(expect[~small])
        if expect[small].sum() > 0:
            obs.append(count[small].sum())
            exp.append(expect[small].sum())
        obs, exp = np.asarray(obs), np.asarray(exp)
        dof = len(obs) - 1
        z = (((obs - exp) ** 2 / exp).sum() - dof) / np.sqrt(2 * dof)
        mean = rec["bary"].astype(np.float64).mean(0)
        se = np.sqrt(1.0 / 18.0 / NSTAT)
        print(f"{name} seed {seed}: chi-square z = {z:+.2f} (dof {dof}), bary means - 1/3 = {(mean - 1 / 3) / se} standard errors")
        assert z <= 4
        assert (np.abs(mean - 1 / 3) <= 5 * se).all()
        b = rec["bary"]
        assert (b >= 0).all() and np.array_equal((b[:, 0] + b[:, 1]) + b[:, 2], np.ones(NSTAT, np.float32))


@pytest.mark.parametrize("name", FIXTURES)
def test_stratified_samples_hit_every_triangle_within_two_of_its_share(scene_data, tables, name):
    sd, tab = scene_data(name), tables[name]
    rec, _ = sref.sample(sd, NSTAT, seed=1, strata=NSTAT, tab=tab)
    count = np.bincount(rec["prim_id"], minlength=sd.ntris).astype(np.float64)
    dev = np.abs(count - NSTAT * tab[0].astype(np.float64) / tab[1])
    print(f"{name}: largest |count - n area / A| = {dev.max():.3f}")
    assert (dev < 2).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_every_point_lies_on_its_triangle(scene_data, tables, name):
    sd = scene_data(name)
    for strata in (0, 1 << 16):
        rec, _ = sref.sample(sd, 1 << 16, seed=2, strata=strata, tab=tables[name])
        p64, S = sref.points64(sd, rec)
        err = np.abs(rec["point"].astype(np.float64) - p64).max(1)
        print(f"{name} strata {strata}: largest error / (2^-24 S) = {(err / (2.0 ** -24 * S)).max():.3f}")
        assert (err <= 4 * 2.0 ** -24 * S).all()
