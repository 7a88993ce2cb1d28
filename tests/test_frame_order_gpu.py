"""GPU tests of the primary frames' ORDER TABLE (cgrt_layout.h FrameDev::order, walk_exact.h tile_pixel_of, trace_kernels.hip
k_build_frame_order, capi_primary.cpp attach_order, include/cgrt.h cgrt_set_frame_order).  Only the order in which a launch
hands out its super-tiles changes, so a frame launched with any valid table, a profile frame and every frame of the policy must equal
the plain launch byte for byte; the device builder must make the table frame_order_ref.py states; tables that are not residue-keeping
permutations of the right length are refused."""
import numpy as np
import pytest

import frame_order_ref as ref

pytestmark = pytest.mark.gpu

W, H = 256, 192


@pytest.fixture
def order(pkg):
    """Frames this small are hinted by default; the order table is for frames the hint policy leaves alone."""
    pkg.set_frame_hints(0)
    yield pkg.set_frame_order
    pkg.set_frame_order(-1)
    pkg.set_frame_hints(-1)


@pytest.fixture(scope="module")
def dragon(pkg):
    return pkg.scenes.make_dragon(20_000)


def _plain(pkg, sc, cam, w, h, **kw):
    pkg.set_frame_order(0)
    return sc.trace_primary(cam, w, h, want_normals=True, **kw)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _tables(nst):
    return (("identity", np.arange(ref.padded(nst), dtype=np.uint16)), ("reversal", ref.reversal(nst)), ("random", ref.random_valid(nst, 11)))


# ---- the builder ----
def test_device_builder_equals_the_reference(pkg):
    rng = np.random.default_rng(7)
    cases = []
    for n in (510, 13, 8, 2043):  # 13 and 2043: not a multiple of 8 before padding
        cases.append(rng.integers(0, 12000, n))
        cases.append(rng.integers(0, 3, n) * 450 + rng.integers(0, 2, n) * 100)  # many ties, on both sides of the threshold
        cases.append(np.zeros(n))
        cases.append(np.full(n, 900))
        cases.append(np.where(np.arange(n) == n // 2, 700, 0))  # one live position
        cases.append(np.where(np.arange(n) % 8 == 3, 0xffffffff - np.arange(n), 499))  # one lane live, the largest values
    cases.append(rng.integers(0, 12000, 16379))  # close to the longest table: 2048 positions per lane
    for t in cases:
        t = np.asarray(t, np.uint32)
        got = pkg.debug_build_frame_order(t)
        assert np.array_equal(got, ref.build_order(t)), len(t)
        assert ref.is_valid_order(got, len(t))


# ---- installed tables ----
def test_frames_with_a_table_equal_the_plain_frame(pkg, order, dragon):
    cam = pkg.scenes.default_camera(W, H)
    sc = pkg.Scene(dragon)
    p0 = _plain(pkg, sc, cam, W, H)
    assert p0[0]["hit"].sum() > 1000
    for name, tab in _tables(ref.super_tiles(W, H)):
        order(1)
        sc.debug_set_frame_order(W, H, tab)
        for k in range(2):
            assert _same(sc.trace_primary(cam, W, H, want_normals=True), p0), (name, k)
        got, state, _ = sc.debug_get_frame_order()
        assert state == 2 and np.array_equal(got, tab), name
        assert sc.trace_primary(cam, W, H)[0].tobytes() == p0[0].tobytes(), name  # hits alone


@pytest.mark.parametrize("shape", ["200x136", "rectangle", "ranks"])
def test_tables_on_partial_tiles_rectangles_and_ranks(pkg, order, dragon, shape):
    sc = pkg.Scene(dragon)
    if shape == "ranks":
        cam = pkg.scenes.default_camera(W, H)
        whole = _plain(pkg, sc, cam, W, H)
        for name, _ in _tables(1):
            merged_h, merged_n = None, None
            for r in range(3):
                p0 = _plain(pkg, sc, cam, W, H, rank=r, nranks=3)
                tab = dict(_tables(ref.super_tiles(W, H, rank=r, nranks=3)))[name]
                order(1)
                sc.debug_set_frame_order(W, H, tab, rank=r, nranks=3)
                got = sc.trace_primary(cam, W, H, want_normals=True, rank=r, nranks=3)
                assert _same(got, p0), (name, r)
                own = ~np.isnan(got[0]["t"])  # (pixels of other ranks keep the caller's mark)
                if merged_h is None:
                    merged_h, merged_n = got[0].copy(), got[1].copy()
                else:
                    assert not (own & ~np.isnan(merged_h["t"])).any()
                    merged_h[own], merged_n[own] = got[0][own], got[1][own]
            assert _same((merged_h, merged_n), whole), name
        return
    w, h, rect = (200, 136, None) if shape == "200x136" else (W, H, (37, 11, W - 60, H - 9))
    cam = pkg.scenes.default_camera(w, h)
    p0 = _plain(pkg, sc, cam, w, h, rect=rect)
    for name, tab in _tables(ref.super_tiles(w, h, rect=rect)):
        order(1)
        sc.debug_set_frame_order(w, h, tab, rect=rect)
        assert _same(sc.trace_primary(cam, w, h, want_normals=True, rect=rect), p0), name


def test_tables_on_a_thin_leaf_scene(pkg, order, scene_data):
    """Cornell: rays that leave the certified walk for the exact one all the time."""
    sd = scene_data("cornell")
    cam = pkg.scenes.default_camera(W, H)
    sc = pkg.Scene(sd)
    p0 = _plain(pkg, sc, cam, W, H)
    for name, tab in _tables(ref.super_tiles(W, H)):
        order(1)
        sc.debug_set_frame_order(W, H, tab)
        assert _same(sc.trace_primary(cam, W, H, want_normals=True), p0), name
    sc.debug_set_frame_order(W, H, None)
    for k in range(6):  # ... and under the policy
        assert _same(sc.trace_primary(cam, W, H, want_normals=True), p0), k


def test_invalid_tables_are_refused(pkg, order, dragon):
    sc = pkg.Scene(dragon)
    nst = ref.super_tiles(W, H)  # 12, padded to 16
    ident = np.arange(ref.padded(nst), dtype=np.uint16)
    dup = ident.copy()
    dup[8] = 0
    res = ident.copy()
    res[[0, 1]] = [1, 0]
    pad = ident.copy()
    pad[[4, 12]] = [12, 4]
    for name, tab in (("duplicate", dup), ("residue", res), ("padded position moved", pad), ("short", ident[:8]), ("long", np.arange(24, dtype=np.uint16))):
        with pytest.raises(pkg.CgrtError) as err:
            sc.debug_set_frame_order(W, H, tab)
        assert err.value.code == -1, name  # CGRT_E_ARG
    sc.debug_set_frame_order(W, H, ident)  # (and the valid one is taken)


# ---- the policy ----
def test_policy_end_to_end(pkg, order, dragon):
    cam = pkg.scenes.default_camera(W, H)
    sc = pkg.Scene(dragon)
    p0 = _plain(pkg, sc, cam, W, H)
    order(1)
    nst = ref.super_tiles(W, H)
    tables = []
    for k in range(40):
        assert _same(sc.trace_primary(cam, W, H, want_normals=True), p0), k
        tab, state, since = sc.debug_get_frame_order()
        # launches 0 and 1 plain, 2 the profile frame (a STAMP frame: equal to the plain one above), 3 .. 33 read the table, 34 profiles again
        if k < 2:
            assert tab is None and state == 0, k
        elif k in (2, 34):
            assert state == 1 and since == 0, k
        else:
            assert state == 2 and since == (k - 2 if k < 34 else k - 34), k
        if tab is not None:
            assert ref.is_valid_order(tab, nst), k
            tables.append(tab)
    assert any((t != np.arange(len(t))).any() for t in tables), "the stand-in's frame has super-tiles with long waves: some table moves them"
    order(0)
    assert _same(sc.trace_primary(cam, W, H, want_normals=True), p0)


def test_a_camera_turned_away_gives_the_identity(pkg, order, dragon):
    cam = pkg.scenes.default_camera(W, H).copy()
    cam[0:3] = [50.0, 0.0, 0.0]
    sc = pkg.Scene(dragon)
    p0 = _plain(pkg, sc, cam, W, H)
    assert p0[0]["hit"].sum() == 0
    order(1)
    for k in range(6):
        assert _same(sc.trace_primary(cam, W, H, want_normals=True), p0), k
    tab, state, _ = sc.debug_get_frame_order()
    assert state == 2 and np.array_equal(tab, np.arange(ref.padded(ref.super_tiles(W, H))))


def test_two_shapes_taking_turns(pkg, order, dragon):
    sc = pkg.Scene(dragon)
    shapes = [(W, H), (200, 136)]
    cams = [pkg.scenes.default_camera(w, h) for w, h in shapes]
    refs = [_plain(pkg, sc, c, w, h) for c, (w, h) in zip(cams, shapes)]
    order(1)
    for k in range(14):
        i = k & 1
        assert _same(sc.trace_primary(cams[i], *shapes[i], want_normals=True), refs[i]), k
        tab, state, _ = sc.debug_get_frame_order()
        assert tab is None and state == 0, k
    for k in range(6):  # one shape again: the third launch in a row profiles it, then it has its table
        assert _same(sc.trace_primary(cams[0], *shapes[0], want_normals=True), refs[0]), k
    assert sc.debug_get_frame_order()[1] == 2
    for k in range(9):  # the other shape: the table is dropped, eight launches run without one
        assert _same(sc.trace_primary(cams[1], *shapes[1], want_normals=True), refs[1]), k
        tab, state, _ = sc.debug_get_frame_order()
        assert (tab is None and state == 0) if k < 7 else (tab is not None and state == (1 if k == 7 else 2)), k


def test_two_streams_taking_turns(pkg, order, dragon):
    import ctypes as C

    hip = C.CDLL(pkg.LIB_PATH)  # the HIP runtime libcgrt.so is linked against (test_frame_hints_gpu.py says why)

    def ok(rc):
        assert rc == 0, rc

    cam = pkg.scenes.default_camera(W, H)
    sc = pkg.Scene(dragon)
    h0 = _plain(pkg, sc, cam, W, H)[0]
    order(1)
    nbytes = W * H * 16
    streams, bufs = [], []
    for _ in range(2):
        st, buf = C.c_void_p(), C.c_void_p()
        ok(hip.hipStreamCreateWithFlags(C.byref(st), 1))  # hipStreamNonBlocking
        ok(hip.hipMalloc(C.byref(buf), C.c_size_t(nbytes)))
        streams.append(st)
        bufs.append(buf)

    def frame_of(i):
        out = np.empty(W * H, pkg.HIT_DTYPE)
        ok(hip.hipDeviceSynchronize())
        ok(hip.hipMemcpy(C.c_void_p(out.ctypes.data), bufs[i], C.c_size_t(nbytes), 2))  # device to host
        return out

    def launch(i):
        sc.trace_primary_device(cam, W, H, bufs[i].value, stream=streams[i].value)

    # with a host synchronisation after every launch
    for k, i in enumerate([0, 1] * 6):
        ok(hip.hipMemset(bufs[i], 0, C.c_size_t(nbytes)))
        ok(hip.hipDeviceSynchronize())
        launch(i)
        assert frame_of(i).tobytes() == h0.tobytes(), (k, i)
        assert sc.debug_get_frame_order()[:2] == (None, 0), k
    # one stream for a while: its table comes (eight launches after the change, then the profile frame), the frames stay equal
    for k in range(14):
        ok(hip.hipMemset(bufs[0], 0, C.c_size_t(nbytes)))
        launch(0)
        assert frame_of(0).tobytes() == h0.tobytes(), k
    assert sc.debug_get_frame_order()[1] == 2
    # back-to-back launches without a host synchronisation: one stream, then the two taking turns
    for k in range(40):
        launch(0)
    assert frame_of(0).tobytes() == h0.tobytes()
    for i in range(2):
        ok(hip.hipMemset(bufs[i], 0, C.c_size_t(nbytes)))
    for k in range(16):
        launch(k & 1)
    assert frame_of(0).tobytes() == h0.tobytes() and frame_of(1).tobytes() == h0.tobytes()
    assert sc.debug_get_frame_order()[:2] == (None, 0)
    for st, buf in zip(streams, bufs):
        ok(hip.hipStreamDestroy(st))
        ok(hip.hipFree(buf))


def test_a_profile_frame_equals_the_plain_frame(pkg, order, dragon):
    """The third launch of a shape runs the STAMP instantiation; at 640x360 too (more than one super-tile per lane)."""
    for w, h in ((W, H), (640, 360)):
        cam = pkg.scenes.default_camera(w, h)
        sc = pkg.Scene(dragon)
        p0 = _plain(pkg, sc, cam, w, h)
        order(1)
        for k in range(3):
            got = sc.trace_primary(cam, w, h, want_normals=True)
        assert sc.debug_get_frame_order()[1:] == (1, 0), "the last launch was the profile frame"
        assert _same(got, p0)
        tab = sc.debug_get_frame_order()[0]
        assert ref.is_valid_order(tab, ref.super_tiles(w, h))
