"""GPU tests of light sets (include/cgrt.h cgrt_render_light_sets, cgrt_render_light_sets_device; Scene.render_light_sets /
render_light_sets_device / render_light_sets_tensor).

Frame b of a batch must be, bit for bit, the single frame of the camera under set b's lights: RGB of render / render_soft, and of
render_tensor in every format, with sentinel bytes around every device output.  The dedupe of shadow rays (distinct point-light positions,
by bit pattern) and of soft-shadow counts (distinct position, radius and in-set index) shows in the stats and never in the bytes.  A batch
leaves the scene's single-frame state alone (prediction record, frame hints), orders its export behind the caller's stream and agrees with
the CPU oracle."""
import time

import numpy as np
import pytest

from conftest import same_bits as _same_bits_elementwise

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FORMATS = ("rgb", "chw", "rgba8")
EXACT, PREDICTED = 0, 1
SENTINEL = 0xA5
STAT_KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays")


def same_bits(a, b):
    """Every element bit-identical (NaN payloads aside: conftest.same_bits)."""
    return np.shape(a) == np.shape(b) and bool(_same_bits_elementwise(a, b).all())


def _lights(sd):
    return np.ascontiguousarray(np.asarray(sd.point_lights, np.float32).reshape(-1, 6))


def _variants(sd):
    """Three sets from the scene's own lights: as they are, recoloured with one extra light, and moved."""
    L = _lights(sd)
    a = L.copy()
    b = np.concatenate([L * np.float32([1, 1, 1, 0.5, 0.25, 1.5]), np.float32([[0.3, 0.9, 1.7, 0.2, 0.4, 0.6]])])
    c = L.copy()
    c[:, 0:3] += np.float32([0.25, 0.1, -0.2])
    return [a, np.ascontiguousarray(b, np.float32), c]


def _single(sc, cam, W, H, L, S=None, soft=None, max_level=2):
    if S is not None and len(S):
        return sc.render_soft(cam, W, H, S, soft["units"], samples=soft["samples"], seed=soft["seed"], lights=L, max_level=max_level)
    return sc.render(cam, W, H, lights=L, max_level=max_level)


def _single_tensor(sc, cam, W, H, fmt, L, S=None, soft=None, max_level=2):
    kw = dict(spherical=S, units=soft["units"], samples=soft["samples"], seed=soft["seed"]) if S is not None and len(S) else {}
    t, _ = sc.render_tensor(cam, W, H, format=fmt, lights=L, max_level=max_level, **kw)
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _guarded(nbytes, pad=256):
    buf = torch.full((nbytes + 2 * pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    inner = buf[pad : pad + nbytes]

    def intact():
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        return bool((b[:pad] == SENTINEL).all() and (b[pad + nbytes :] == SENTINEL).all())

    return inner, intact


_FRAME_BYTES = {"rgb": lambda W, H: W * H * 12, "chw": lambda W, H: W * H * 12, "rgba8": lambda W, H: W * H * 4}


def _export_sets(sc, cam, W, H, fmt, sets, **kw):
    """render_light_sets_device into a sentinel-guarded buffer: (per-set byte arrays, stats)."""
    B = len(sets)
    fb = _FRAME_BYTES[fmt](W, H)
    inner, intact = _guarded(B * fb)
    st = sc.render_light_sets_device(cam, W, H, inner.data_ptr(), sets, format=fmt, **kw)
    assert intact(), "bytes outside the batch's frames were written"
    return inner.cpu().numpy().reshape(B, fb), st


def _check_batch(sc, cam, W, H, sets, sph=None, soft=None, max_level=2, formats=FORMATS):
    kw = dict(spherical_sets=sph, units=soft["units"], samples=soft["samples"], seed=soft["seed"]) if sph is not None else {}
    got, st = sc.render_light_sets(cam, W, H, sets, max_level=max_level, **kw)
    assert got.shape == (len(sets), W * H, 3)
    for b in range(len(sets)):
        want, _ = _single(sc, cam, W, H, sets[b], None if sph is None else sph[b], soft, max_level)
        assert same_bits(got[b], want), ("host", b, max_level)
    for fmt in formats:
        out, st2 = _export_sets(sc, cam, W, H, fmt, sets, max_level=max_level, **kw)
        for k in STAT_KEYS + ("levels",):
            assert st2[k] == st[k], (fmt, k)
        for b in range(len(sets)):
            want = _single_tensor(sc, cam, W, H, fmt, sets[b], None if sph is None else sph[b], soft, max_level)
            assert out[b].tobytes() == want.tobytes(), (fmt, b, max_level)
    return got, st


@pytest.mark.parametrize("name", ["cube", "monkey", "spheres", "cornell"])
def test_sets_equal_single_frames(pkg, scene_data, name):
    sd = scene_data(name)
    sc = pkg.Scene(sd)
    W, H = 72, 40
    cam = pkg.scenes.default_camera(W, H)
    sets = _variants(sd)
    for depth in (0, 1, 2, 4):
        got, st = _check_batch(sc, cam, W, H, sets, max_level=depth)
        if depth == 0:
            assert not got.any() and st["primary_rays"] == 0
        elif name in ("cube", "cornell"):
            assert got.any(), "the batch sees the scene"
    sc.close()


def test_ragged_and_edge_sets(pkg, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 40, 24
    cam = pkg.scenes.default_camera(W, H)
    L = _lights(sd)
    extra = np.float32([[0.2, 0.8, 1.5, 0.3, 0.3, 0.9], [-0.3, 0.5, 1.0, 0.6, 0.2, 0.1], [0.0, 0.1, 2.0, 0.5, 0.5, 0.5]])
    empty = np.zeros((0, 6), np.float32)
    soft = dict(units=pkg.unit_vector_table(512, 3), samples=5, seed=11)
    S = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
    E7 = np.zeros((0, 7), np.float32)
    # 0, 1 and 3 point lights; a set with only spherical lights; an all-empty set
    sets = [empty, L[:1], extra, empty, empty]
    sph = [E7, E7, E7, S, E7]
    for depth in (1, 2, 4):
        _check_batch(sc, cam, W, H, sets, sph, soft, max_level=depth)
    got, _ = sc.render_light_sets(cam, W, H, [empty], max_level=2)
    assert not got.any(), "no lights: black"
    # B = 1 and B = 64 on a small frame
    _check_batch(sc, cam, W, H, [extra], max_level=2)
    rng = np.random.default_rng(5)
    many = []
    for b in range(64):
        x = extra[: 1 + b % 3].copy()
        x[:, 3:6] = rng.uniform(0.0, 1.0, (len(x), 3)).astype(np.float32)
        many.append(x)
    t, st = sc.render_light_sets_tensor(cam, 32, 32, many, format="rgb", max_level=2)
    torch.cuda.synchronize()
    a = t.cpu().numpy().reshape(64, -1, 3)
    for b in range(64):
        assert same_bits(a[b], sc.render(cam, 32, 32, lights=many[b], max_level=2)[0]), b
    # a camera facing away: black frames, zero shadow rays
    away = cam.copy()
    away[0:3] = np.float32([50.0, 60.0, 70.0])
    for fmt in FORMATS:
        out, st = _export_sets(sc, away, W, H, fmt, sets[:3], max_level=2)
        for b in range(3):
            assert out[b].tobytes() == _single_tensor(sc, away, W, H, fmt, sets[b], max_level=2).tobytes(), (fmt, b)
        assert st["shadow_rays"] == 0 and st["reflection_rays"] == 0 and st["primary_rays"] == W * H
    # nsets = 1025 is refused; the next batch and the next single frame are still right
    with pytest.raises(RuntimeError):
        sc.render_light_sets(cam, W, H, [L] * 1025, max_level=2)
    _check_batch(sc, cam, W, H, sets[:3], max_level=2, formats=("rgb",))
    ref, _ = sc.render(cam, W, H, lights=L, max_level=2)
    assert same_bits(ref, _single(sc, cam, W, H, L)[0])
    sc.close()


def test_dedupe_shows_in_counts_not_bytes(pkg, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 64, 48
    cam = pkg.scenes.default_camera(W, H)
    L = _lights(sd)
    one, st1 = sc.render(cam, W, H, lights=L, max_level=4)
    # a colour sweep: the batch traces one frame's rays
    sweep = []
    for b in range(8):
        x = L.copy()
        x[:, 3:6] *= np.float32(0.25 + 0.25 * b)
        sweep.append(x)
    got, st = _check_batch(sc, cam, W, H, sweep, max_level=4, formats=())
    for k in ("primary_rays", "shadow_rays", "reflection_rays", "levels"):
        assert st[k] == st1[k], k
    # 8 distinct single-light positions: 8 times one single-light frame's shadow rays
    pos = []
    for b in range(8):
        x = L[:1].copy()
        x[0, 0:3] += np.float32([0.05 * b, -0.03 * b, 0.02 * b])
        pos.append(x)
    _, s1 = sc.render(cam, W, H, lights=pos[0], max_level=4)
    got, st = _check_batch(sc, cam, W, H, pos, max_level=4, formats=())
    assert st["shadow_rays"] == 8 * s1["shadow_rays"] and st["reflection_rays"] == s1["reflection_rays"]
    hits = s1["shadow_rays"]  # (one light: one shadow ray per hit)
    # duplicates within a set, +0.0 / -0.0 positions: bytes of the single frames, counts by bit pattern
    p = np.float32([[0.0, 0.8, 0.0, 0.7, 0.7, 0.7]])
    m = p.copy()
    m[0, 0] = np.float32(-0.0)
    m[0, 2] = np.float32(-0.0)
    dup = [np.concatenate([p, p, m]), np.concatenate([m, p * np.float32([1, 1, 1, 0.5, 0.5, 0.5])]), p]
    got, st = _check_batch(sc, cam, W, H, dup, max_level=4, formats=("rgb",))
    assert st["shadow_rays"] == 2 * hits, "+0.0 and -0.0 are two positions, duplicates one"
    sc.close()


def test_soft_shadows_draw_with_the_in_set_index(pkg, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 48, 40
    cam = pkg.scenes.default_camera(W, H)
    L = _lights(sd)
    soft = dict(units=pkg.unit_vector_table(1000, 9), samples=7, seed=77)
    A = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
    Bl = A.copy()
    Bl[0, 0:3] += np.float32([0.2, -0.05, 0.1])
    Bl[0, 3] = np.float32(0.05)
    A2 = A.copy()
    A2[0, 3] = np.float32(0.2)  # another radius
    A3 = A.copy()
    A3[0, 4:7] = np.float32([0.2, 0.9, 0.4])  # another colour: the same key as A at index 0
    sph = [A, np.concatenate([Bl, A]), np.concatenate([A2, Bl]), A3]
    sets = [L, L[:0], L, L * np.float32([1, 1, 1, 0.5, 0.5, 0.5])]
    for depth in (2, 4):
        got, st = _check_batch(sc, cam, W, H, sets, sph, soft, max_level=depth, formats=FORMATS if depth == 2 else ("rgb",))
        # keys: (A, 0), (Bl, 0), (A, 1), (A2, 0), (Bl, 1) -- A3 at index 0 is (A, 0) again
        _, s1 = sc.render_soft(cam, W, H, A, soft["units"], samples=soft["samples"], seed=soft["seed"], lights=L, max_level=depth)
        hits = s1["soft_shadow_rays"] // soft["samples"]
        assert st["soft_shadow_rays"] == hits * 5 * soft["samples"]
        assert st["shadow_rays"] == s1["shadow_rays"], "two point-light sets at the same positions: one set of shadow rays"
    sc.close()


def test_batch_leaves_the_prediction_record_alone(pkg, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 96, 64
    cam = pkg.scenes.default_camera(W, H)
    first, _ = sc.render(cam, W, H, max_level=2)
    assert sc.last_render_path() == EXACT
    for _ in range(2):
        rgb, _ = sc.render(cam, W, H, max_level=2)
        assert sc.last_render_path() == PREDICTED and rgb.tobytes() == first.tobytes()
    sets = _variants(sd)
    sc.render_light_sets(cam, W, H, sets, max_level=2)
    sc.render_light_sets(cam, 33, 17, sets[:2], max_level=4)
    sc.render_light_sets_tensor(cam, W, H, sets, format="chw", max_level=2)
    rgb, _ = sc.render(cam, W, H, max_level=2)
    assert sc.last_render_path() == PREDICTED, "a batch must not touch the scene's prediction record"
    assert rgb.tobytes() == first.tobytes()
    sc.close()


def test_batch_leaves_frame_hints_alone(pkg):
    pkg.debug_set_hint_thresholds(100, 60)
    pkg.set_frame_hints(1)
    try:
        sd = pkg.scenes.make_dragon(60_000)
        sc = pkg.Scene(sd)
        W, H = 320, 200
        cam = pkg.scenes.default_camera(W, H)
        h0 = torch.full((W * H * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        for _ in range(4):  # hinted frames
            sc.trace_primary_device(cam, W, H, h0.data_ptr())
        torch.cuda.synchronize()
        counts = sc.hint_counts()
        sc.render_light_sets(cam, W, H, _variants(sd), max_level=2)
        assert sc.hint_counts() == counts, "a batch must not touch the frame hints"
        sc.close()
    finally:
        pkg.set_frame_hints(-1)
        pkg.debug_set_hint_thresholds(0, 0)


def test_export_is_ordered_behind_the_callers_stream(pkg, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 256, 160
    cam = pkg.scenes.default_camera(W, H)
    sets = _variants(sd) + [_lights(sd)[:0]]
    B = len(sets)
    ref, _ = sc.render_light_sets(cam, W, H, sets, max_level=2)
    s = torch.cuda.Stream()
    out = torch.empty((B, H, W, 3), dtype=torch.float32, device="cuda")
    with torch.cuda.stream(s):
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            big = big @ big  # keeps the stream busy
        out.fill_(-7.0)  # enqueued BEFORE the call: the export must land after it
    sc.render_light_sets_tensor(cam, W, H, sets, format="rgb", out=out, stream=s, max_level=2)
    with torch.cuda.stream(s):
        copy = out.clone()  # enqueued AFTER the call: sees the frames
    torch.cuda.synchronize()
    assert same_bits(copy.cpu().numpy().reshape(B, -1, 3), ref)
    assert same_bits(out.cpu().numpy().reshape(B, -1, 3), ref)
    sc.close()


def test_light_sets_match_the_oracle(pkg, orc, scene_data):
    """3 sets over 48x32 of Cornell, depth 2, point and spherical lights: every set within 1e-5 of the oracle's shading of the frame's
    row-major rays under that set (ray i = pixel i: the same soft-shadow key)."""
    sd = scene_data("cornell")
    o = orc.OracleScene(sd)
    sc = pkg.Scene(sd)
    W, H = 48, 32
    cam = pkg.scenes.default_camera(W, H)
    L = _lights(sd)
    A = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
    Bl = A.copy()
    Bl[0, 0:3] += np.float32([0.15, 0.0, -0.1])
    sets = [L, L * np.float32([1, 1, 1, 0.3, 0.6, 0.9]), np.concatenate([L, np.float32([[0.2, 0.7, 1.2, 0.4, 0.4, 0.4]])])]
    sph = [A, np.concatenate([Bl, A]), np.zeros((0, 7), np.float32)]
    units, samples, seed = pkg.unit_vector_table(1000, 5), 6, 123
    got, _ = sc.render_light_sets(cam, W, H, sets, spherical_sets=sph, units=units, samples=samples, seed=seed, max_level=2)
    rays = orc.generate_rays(cam, W, H)
    for b in range(3):
        kw = dict(spherical=sph[b], units=units, samples=samples, seed=seed) if len(sph[b]) else {}
        want, _ = o.shade_rays(rays, sets[b], max_level=2, threads=16, **kw)
        assert np.array_equal(np.isnan(got[b]), np.isnan(want)), b
        eq = _same_bits_elementwise(got[b], want)
        with np.errstate(invalid="ignore"):
            err = np.where(eq, 0.0, np.abs(got[b].astype(np.float64) - want))
        assert not np.isnan(err).any() and float(err.max(initial=0.0)) <= 1e-5, (b, float(np.nanmax(err, initial=0.0)))
    sc.close()
    o.close()


def test_certified_walk_on_shadow_lists(pkg):
    sd = pkg.scenes.make_dragon(200_000)
    sc = pkg.Scene(sd)
    assert sc.walk() == 1, "the stand-in has a fast tree (certified walk)"
    W, H = 320, 200
    cam = pkg.scenes.default_camera(W, H)
    L = _lights(sd)
    sets = [L, L * np.float32([1, 1, 1, 0.2, 0.5, 0.8]), np.concatenate([L, L + np.float32([0.3, 0.2, 0.1, 0, 0, 0])]),
            L + np.float32([-0.2, 0.1, 0.3, 0, 0, 0])]
    _check_batch(sc, cam, W, H, sets, max_level=2, formats=("rgba8",))
    sc.close()


def test_seeded_random_batches(pkg, scene_data):
    """Random counts, positions with forced duplicates and colours over three scenes, compared bit for bit with single frames; stops
    after about 60 s."""
    rng = np.random.default_rng(20261016)
    deadline = time.time() + 60.0
    units = pkg.unit_vector_table(777, 1)
    runs = 0
    for name in ("cornell", "monkey", "spheres") * 4:
        if time.time() > deadline:
            break
        sd = scene_data(name)
        sc = pkg.Scene(sd)
        W, H = int(rng.integers(8, 70)), int(rng.integers(8, 50))
        cam = pkg.scenes.default_camera(W, H)
        base = _lights(sd)
        pool = np.concatenate([base[:, 0:3], rng.uniform(-1.0, 2.0, (4, 3)).astype(np.float32)])
        B = int(rng.integers(1, 9))
        sets, sph = [], []
        for _ in range(B):
            n = int(rng.integers(0, 5))
            x = np.zeros((n, 6), np.float32)
            x[:, 0:3] = pool[rng.integers(0, len(pool), n)]  # positions drawn from a small pool: duplicates across and within sets
            x[:, 3:6] = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
            sets.append(x)
            k = int(rng.integers(0, 3))
            y = np.zeros((k, 7), np.float32)
            y[:, 0:3] = pool[rng.integers(0, len(pool), k)]
            y[:, 3] = rng.choice(np.float32([0.05, 0.1]), k)
            y[:, 4:7] = rng.uniform(0.0, 1.0, (k, 3)).astype(np.float32)
            sph.append(y)
        depth = int(rng.choice([1, 2, 3]))
        soft = dict(units=units, samples=int(rng.integers(1, 6)), seed=int(rng.integers(0, 1000)))
        _check_batch(sc, cam, W, H, sets, sph, soft, max_level=depth, formats=("rgb",))
        sc.close()
        runs += 1
    assert runs >= 3
