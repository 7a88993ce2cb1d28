"""GPU tests of multi-view light sets (include/cgrt.h cgrt_render_views_light_sets, cgrt_render_views_light_sets_device;
Scene.render_views_light_sets / render_views_light_sets_device / render_views_light_sets_tensor).

Frame (v, s) of a batch must be, bit for bit, the single frame of cams[v] under set s's lights: RGB of render / render_soft, and of
render_tensor in every format, with sentinel bytes around every device output and NaN (or zero alpha) in every byte of the output before
the call, so that a pixel of sets 1..S-1 left unwritten shows.  With one view the batch is cgrt_render_light_sets (bytes and stats); one set
of the batch is cgrt_render_views.  Soft-shadow samples draw with the in-view pixel and the in-set index together.  The stats are the sums
over the views of the light-set batches.  A batch leaves the scene's single-frame state alone, orders its export behind the caller's stream
and agrees with the CPU oracle."""
import numpy as np
import pytest

from conftest import same_bits as _same_bits_elementwise

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FORMATS = ("rgb", "chw", "rgba8")
EXACT, PREDICTED = 0, 1
SENTINEL = 0xA5
STAT_KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays")
_FRAME_BYTES = {"rgb": lambda W, H: W * H * 12, "chw": lambda W, H: W * H * 12, "rgba8": lambda W, H: W * H * 4}
_FILL = {"rgb": 0xFF, "chw": 0xFF, "rgba8": 0x00}  # NaN floats; zero alpha (every written pixel has alpha 255)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and bool(_same_bits_elementwise(a, b).all())


def _lights(sd):
    return np.ascontiguousarray(np.asarray(sd.point_lights, np.float32).reshape(-1, 6))


def _cams(pkg, V, W, H, name="cornell"):
    """V cameras that differ in euler, distance, fovy and aspect (the spheres preset from its own viewpoint, as tests/test_views_gpu.py)."""
    if name == "spheres":
        base = np.asarray([0, 0, 6, 0, 0, 0, 8.0, np.radians(50.0), np.float32(W) / np.float32(H)], np.float32)
    else:
        base = pkg.scenes.default_camera(W, H).astype(np.float32)
    a = np.repeat(base[None, :], V, axis=0)
    k = np.arange(V, dtype=np.float32)
    a[:, 3] += np.float32(0.04) * k
    a[:, 4] += np.float32(-0.09) * k
    a[:, 6] *= np.float32(1.0) + np.float32(0.07) * k
    a[:, 7] *= np.float32(1.0) - np.float32(0.03) * k
    return np.ascontiguousarray(a, np.float32)


def _variants(sd):
    """Three sets from the scene's own lights: as they are, recoloured with one extra light, and moved."""
    L = _lights(sd)
    b = np.concatenate([L * np.float32([1, 1, 1, 0.5, 0.25, 1.5]), np.float32([[0.3, 0.9, 1.7, 0.2, 0.4, 0.6]])])
    c = L.copy()
    c[:, 0:3] += np.float32([0.25, 0.1, -0.2])
    return [L.copy(), np.ascontiguousarray(b, np.float32), c]


def _mixed(pkg, scene_data):
    """Cornell with two spheres in the box: meshes and spheres in one scene."""
    sd = scene_data("cornell")
    sp = np.asarray([[0.25, -0.35, 0.1, 0.2, 0], [-0.3, -0.4, -0.2, 0.15, -1]], np.float32)
    return pkg.scenes.SceneData(pos_nrm=sd.pos_nrm, tri=sd.tri, tri_mesh=sd.tri_mesh, materials=sd.materials, spheres=sp,
                                point_lights=sd.point_lights, name="cornell+spheres")


def _soft_kw(sph, soft):
    return dict(spherical_sets=sph, units=soft["units"], samples=soft["samples"], seed=soft["seed"]) if sph is not None else {}


def _single(sc, cam, W, H, L, S=None, soft=None, max_level=2):
    if S is not None and len(S):
        return sc.render_soft(cam, W, H, S, soft["units"], samples=soft["samples"], seed=soft["seed"], lights=L, max_level=max_level)
    return sc.render(cam, W, H, lights=L, max_level=max_level)


def _single_tensor(sc, cam, W, H, fmt, L, S=None, soft=None, max_level=2):
    kw = dict(spherical=S, units=soft["units"], samples=soft["samples"], seed=soft["seed"]) if S is not None and len(S) else {}
    t, _ = sc.render_tensor(cam, W, H, format=fmt, lights=L, max_level=max_level, **kw)
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _export(sc, cams, W, H, fmt, sets, pad=256, **kw):
    """render_views_light_sets_device into a sentinel-guarded buffer pre-filled with _FILL: ((V, S, frame bytes) array, stats)."""
    V, S = len(cams), len(sets)
    fb = _FRAME_BYTES[fmt](W, H)
    n = V * S * fb
    buf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf[pad : pad + n].fill_(_FILL[fmt])
    st = sc.render_views_light_sets_device(cams, W, H, buf.data_ptr() + pad, sets, format=fmt, **kw)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[:pad] == SENTINEL).all() and (b[pad + n :] == SENTINEL).all(), "bytes outside the batch's frames were written"
    return b[pad : pad + n].reshape(V, S, fb), st


class _Singles:
    """The single frames of cams[v] under set s, computed once and shared by every sub-batch."""

    def __init__(self, sc, cams, W, H, sets, sph=None, soft=None, max_level=2):
        self.a = (sc, cams, W, H, sets, sph, soft, max_level)
        self.cache = {}

    def get(self, v, s, fmt=None):
        if (v, s, fmt) not in self.cache:
            sc, cams, W, H, sets, sph, soft, ml = self.a
            S = None if sph is None else sph[s]
            if fmt is None:
                self.cache[(v, s, fmt)] = _single(sc, cams[v], W, H, sets[s], S, soft, ml)
            else:
                self.cache[(v, s, fmt)] = _single_tensor(sc, cams[v], W, H, fmt, sets[s], S, soft, ml)
        return self.cache[(v, s, fmt)]


def _check_batch(sc, cams, W, H, sets, sph=None, soft=None, max_level=2, formats=FORMATS, singles=None, vi=None, si=None):
    """Batch (cams[vi], sets[si]) against the single frames, host form and every device format; returns (host rgb, stats)."""
    singles = singles or _Singles(sc, cams, W, H, sets, sph, soft, max_level)
    vi = list(range(len(cams))) if vi is None else vi
    si = list(range(len(sets))) if si is None else si
    bc, bs = cams[vi], [sets[s] for s in si]
    bsph = None if sph is None else [sph[s] for s in si]
    kw = _soft_kw(bsph, soft)
    got, st = sc.render_views_light_sets(bc, W, H, bs, max_level=max_level, **kw)
    assert got.shape == (len(vi), len(si), W * H, 3)
    for a, v in enumerate(vi):
        for b, s in enumerate(si):
            assert same_bits(got[a, b], singles.get(v, s)[0]), ("host", v, s, max_level)
    for fmt in formats:
        out, st2 = _export(sc, bc, W, H, fmt, bs, max_level=max_level, **kw)
        for k in STAT_KEYS + ("levels",):
            assert st2[k] == st[k], (fmt, k)
        for a, v in enumerate(vi):
            for b, s in enumerate(si):
                assert out[a, b].tobytes() == singles.get(v, s, fmt).tobytes(), (fmt, v, s, max_level)
    return got, st


def _grid(sc, cams, W, H, sets, depths, sph=None, soft=None, formats_at=(2,)):
    """V in {1, 3} x S in {1, 3} for every depth; the three formats at the depths in formats_at, the host form and rgb elsewhere."""
    for depth in depths:
        singles = _Singles(sc, cams, W, H, sets, sph, soft, depth)
        for vi in ([0], [0, 1, 2]):
            for si in ([1], [0, 1, 2]):
                fm = FORMATS if depth in formats_at and len(vi) == 3 and len(si) == 3 else ("rgb",)
                got, st = _check_batch(sc, cams, W, H, sets, sph, soft, depth, fm, singles, vi, si)
                if depth == 0:
                    assert not got.any() and st["primary_rays"] == 0


@pytest.mark.parametrize("name", ["cube", "cornell", "monkey", "cornell+spheres"])
def test_frames_equal_single_frames(pkg, scene_data, name):
    sd = _mixed(pkg, scene_data) if name == "cornell+spheres" else scene_data(name)
    sc = pkg.Scene(sd)
    W, H = 40, 24
    cams = _cams(pkg, 3, W, H)
    _grid(sc, cams, W, H, _variants(sd), (0, 1, 2, 4, 16))
    sc.close()


@pytest.mark.parametrize("certified", [True, False])
def test_certified_and_exact_walk(pkg, certified):
    sd = pkg.scenes.make_dragon(20_000)
    sc = pkg.Scene(sd)
    assert sc.walk() == 1, "the stand-in has a fast tree (certified walk)"
    sc.set_walk(certified)
    W, H = 64, 40
    cams = _cams(pkg, 3, W, H)
    L = _lights(sd)
    sets = [L, L * np.float32([1, 1, 1, 0.2, 0.5, 0.8]), np.concatenate([L, L + np.float32([0.3, 0.2, 0.1, 0, 0, 0])])]
    _grid(sc, cams, W, H, sets, (2, 4), formats_at=(4,))
    sc.close()


def test_one_view_is_light_sets_and_one_set_is_views(pkg, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 56, 40
    cams = _cams(pkg, 3, W, H)
    sets = _variants(sd)
    soft = dict(units=pkg.unit_vector_table(800, 2), samples=3, seed=5)
    sph = [pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy(), np.zeros((0, 7), np.float32), pkg.scenes.CORNELL_SPHERICAL_LIGHTS * np.float32(1.0)]
    for depth in (1, 2, 4):
        one, st1 = sc.render_views_light_sets(cams[:1], W, H, sets, max_level=depth, **_soft_kw(sph, soft))
        ls, st_ls = sc.render_light_sets(cams[0], W, H, sets, max_level=depth, **_soft_kw(sph, soft))
        assert same_bits(one[0], ls), depth
        assert st1 == {**st_ls, "device_ms": st1["device_ms"]}, depth
        for fmt in ("rgb", "rgba8"):
            t, _ = sc.render_views_light_sets_tensor(cams, W, H, sets, format=fmt, max_level=depth)
            for s in range(3):
                v, _ = sc.render_views_tensor(cams, W, H, format=fmt, lights=sets[s], max_level=depth)
                torch.cuda.synchronize()
                assert t[:, s].cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), (fmt, s, depth)
    sc.close()


@pytest.mark.parametrize("samples", [1, 16])
def test_soft_shadows_draw_with_view_pixel_and_in_set_index(pkg, scene_data, samples):
    """Three views that differ and three sets whose two spherical lights sit at different in-set indices: every frame is its single frame's
    bytes.  A batch that drew with the frame-wide pixel (the VIEWS rule lost) or with the key's position in the batch (the SETS rule lost)
    would give other bytes in views 1 and 2 or in sets 1 and 2."""
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 48, 32
    cams = _cams(pkg, 3, W, H)
    L = _lights(sd)
    A = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
    Bl = A.copy()
    Bl[0, 0:3] += np.float32([0.2, -0.05, 0.1])
    Bl[0, 3] = np.float32(0.05)
    sph = [np.concatenate([A, Bl]), np.concatenate([Bl, A]), np.concatenate([A * np.float32([1, 1, 1, 1, 0.3, 0.6, 0.9]), Bl])]
    sets = [L, L[:0], L * np.float32([1, 1, 1, 0.5, 0.5, 0.5])]
    soft = dict(units=pkg.unit_vector_table(1000, 9), samples=samples, seed=77)
    for depth in (2, 4):
        got, st = _check_batch(sc, cams, W, H, sets, sph, soft, depth, FORMATS if depth == 2 else ("rgb",))
        # the draws differ between views and between in-set indices: the frames are not copies of each other
        assert not same_bits(got[1, 0], got[0, 0]) and not same_bits(got[0, 1], got[0, 0])
        # keys (A, 0), (Bl, 1), (Bl, 0), (A, 1): the third set's lights are keys of the first (colour is not part of a key)
        _, s1 = sc.render_views(cams, W, H, spherical=A, units=soft["units"], samples=samples, seed=soft["seed"], lights=L, max_level=depth)
        hits = s1["soft_shadow_rays"] // samples
        assert st["soft_shadow_rays"] == hits * 4 * samples
    sc.close()


def test_edge_batches(pkg, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 40, 24
    cams = _cams(pkg, 3, W, H)
    away = cams[1].copy()
    away[0:3] = np.float32([50.0, 60.0, 70.0])  # a view that sees nothing, beside full ones
    cams[1] = away
    L = _lights(sd)
    empty = np.zeros((0, 6), np.float32)
    extra = np.float32([[0.2, 0.8, 1.5, 0.3, 0.3, 0.9], [-0.3, 0.5, 1.0, 0.6, 0.2, 0.1], [0.0, 0.1, 2.0, 0.5, 0.5, 0.5]])
    p = np.float32([[0.0, 0.8, 0.0, 0.7, 0.7, 0.7]])
    m = p.copy()
    m[0, 0] = np.float32(-0.0)
    m[0, 2] = np.float32(-0.0)
    soft = dict(units=pkg.unit_vector_table(512, 3), samples=5, seed=11)
    E7 = np.zeros((0, 7), np.float32)
    S = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
    # ragged: no lights, one, three; a set with only a spherical light; duplicates within and across sets; +0.0 against -0.0
    sets = [empty, L[:1], extra, empty, np.concatenate([p, p, m]), np.concatenate([m, p * np.float32([1, 1, 1, 0.5, 0.5, 0.5])])]
    sph = [E7, E7, E7, S, E7, E7]
    for depth in (1, 2, 4):
        got, st = _check_batch(sc, cams, W, H, sets, sph, soft, depth, FORMATS if depth == 2 else ("rgb",))
        assert not got[1].any(), "the view that sees nothing is black under every set"
        assert not got[:, 0].any(), "a set without lights is black"
        assert got[0, 2].any() and got[2, 2].any()
    # the dedupe shows in the counts: positions L[0], extra x 3, p, m (+0.0 and -0.0 are two positions, duplicates one)
    _, sv = sc.render_views(cams, W, H, lights=L[:1], max_level=4)
    hits = sv["shadow_rays"]
    assert st["shadow_rays"] == hits * (1 + 3 + 2)
    # the same batch after a full batch in the workspace: every pixel of sets 1..S-1 is written again
    sc.render_views_light_sets(_cams(pkg, 3, W, H), W, H, [extra] * 6, max_level=2)
    _check_batch(sc, cams, W, H, sets, sph, soft, 2, ("rgb",))
    # a refused batch leaves the scene usable
    with pytest.raises(RuntimeError):
        sc.render_views_light_sets(cams, W, H, [L] * 1025, max_level=2)
    _check_batch(sc, cams, W, H, sets[:3], max_level=2, formats=("rgb",))
    sc.close()


def test_stats(pkg, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 64, 48
    cams = _cams(pkg, 3, W, H)
    cams[2, 0:3] = np.float32([50.0, 60.0, 70.0])  # (a view without hits)
    L = _lights(sd)
    moved = L.copy()
    moved[:, 0:3] += np.float32([0.1, 0.0, -0.1])
    sets = [L, L * np.float32([1, 1, 1, 0.5, 0.5, 0.5]), moved, np.concatenate([L, moved])]
    A = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
    sph = [A, np.zeros((0, 7), np.float32), np.concatenate([A, A]), A]
    soft = dict(units=pkg.unit_vector_table(700, 4), samples=3, seed=8)
    for depth in (0, 1, 2, 4, 16):
        _, st = sc.render_views_light_sets(cams, W, H, sets, max_level=depth, **_soft_kw(sph, soft))
        per = [sc.render_light_sets(cams[v], W, H, sets, max_level=depth, **_soft_kw(sph, soft))[1] for v in range(3)]
        _, sv = sc.render_views(cams, W, H, lights=L[:1], max_level=depth)
        assert st["primary_rays"] == (3 * W * H if depth >= 1 else 0)
        assert st["reflection_rays"] == sv["reflection_rays"] and st["levels"] == sv["levels"], depth
        for k in STAT_KEYS:
            assert st[k] == sum(p[k] for p in per), (depth, k)
        assert st["levels"] == max(p["levels"] for p in per)
        hits = sv["shadow_rays"]  # (one light: one shadow ray per hit, over all views and levels)
        assert st["shadow_rays"] == hits * 2, "two distinct positions"
        assert st["soft_shadow_rays"] == hits * 2 * soft["samples"], "keys (A, 0), (A, 1)"
        assert st["device_ms"] >= 0.0
    sc.close()


def test_batch_leaves_the_prediction_record_and_hints_alone(pkg, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 96, 64
    cam = pkg.scenes.default_camera(W, H)
    first, _ = sc.render(cam, W, H, max_level=2)
    assert sc.last_render_path() == EXACT
    rgb, _ = sc.render(cam, W, H, max_level=2)
    assert sc.last_render_path() == PREDICTED and rgb.tobytes() == first.tobytes()
    cams = _cams(pkg, 2, W, H)
    sets = _variants(sd)
    sc.render_views_light_sets(cams, W, H, sets, max_level=2)
    sc.render_views_light_sets(cams, 33, 17, sets[:2], max_level=4)
    sc.render_views_light_sets_tensor(cams, W, H, sets, format="chw", max_level=2)
    torch.cuda.synchronize()
    rgb, _ = sc.render(cam, W, H, max_level=2)
    assert sc.last_render_path() == PREDICTED, "a batch must not touch the scene's prediction record"
    assert rgb.tobytes() == first.tobytes()
    sc.close()
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
        sc.render_views_light_sets(_cams(pkg, 2, W, H), W, H, [_lights(sd), _lights(sd) * np.float32(0.5)], max_level=2)
        assert sc.hint_counts() == counts, "a batch must not touch the frame hints"
        sc.close()
    finally:
        pkg.set_frame_hints(-1)
        pkg.debug_set_hint_thresholds(0, 0)


def test_export_is_ordered_behind_the_callers_stream(pkg, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd)
    W, H = 192, 128
    cams = _cams(pkg, 2, W, H)
    sets = _variants(sd) + [_lights(sd)[:0]]
    V, S = 2, len(sets)
    ref, _ = sc.render_views_light_sets(cams, W, H, sets, max_level=2)
    s = torch.cuda.Stream()
    out = torch.empty((V, S, H, W, 3), dtype=torch.float32, device="cuda")
    with torch.cuda.stream(s):
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            big = big @ big  # keeps the stream busy
        out.fill_(-7.0)  # enqueued BEFORE the call: the export must land after it
    sc.render_views_light_sets_tensor(cams, W, H, sets, format="rgb", out=out, stream=s, max_level=2)
    with torch.cuda.stream(s):
        copy = out.clone()  # enqueued AFTER the call: sees the frames
    torch.cuda.synchronize()
    assert same_bits(copy.cpu().numpy().reshape(V, S, -1, 3), ref)
    assert same_bits(out.cpu().numpy().reshape(V, S, -1, 3), ref)
    sc.close()


def test_views_light_sets_match_the_oracle(pkg, orc, scene_data):
    """2 views x 3 sets over 40x28 of Cornell, depth 2, point and spherical lights: every frame within 1e-5 of the oracle's shading of its
    camera's row-major rays under its set (ray i = in-view pixel i: the same soft-shadow key)."""
    sd = scene_data("cornell")
    o = orc.OracleScene(sd)
    sc = pkg.Scene(sd)
    W, H = 40, 28
    cams = _cams(pkg, 2, W, H)
    L = _lights(sd)
    A = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
    Bl = A.copy()
    Bl[0, 0:3] += np.float32([0.15, 0.0, -0.1])
    sets = [L, L * np.float32([1, 1, 1, 0.3, 0.6, 0.9]), np.concatenate([L, np.float32([[0.2, 0.7, 1.2, 0.4, 0.4, 0.4]])])]
    sph = [A, np.concatenate([Bl, A]), np.zeros((0, 7), np.float32)]
    units, samples, seed = pkg.unit_vector_table(1000, 5), 6, 123
    got, _ = sc.render_views_light_sets(cams, W, H, sets, spherical_sets=sph, units=units, samples=samples, seed=seed, max_level=2)
    for v in range(2):
        rays = orc.generate_rays(cams[v], W, H)
        for s in range(3):
            kw = dict(spherical=sph[s], units=units, samples=samples, seed=seed) if len(sph[s]) else {}
            want, _ = o.shade_rays(rays, sets[s], max_level=2, threads=16, **kw)
            assert np.array_equal(np.isnan(got[v, s]), np.isnan(want)), (v, s)
            eq = _same_bits_elementwise(got[v, s], want)
            with np.errstate(invalid="ignore"):
                err = np.where(eq, 0.0, np.abs(got[v, s].astype(np.float64) - want))
            assert not np.isnan(err).any() and float(err.max(initial=0.0)) <= 1e-5, (v, s, float(np.nanmax(err, initial=0.0)))
    sc.close()
    o.close()
