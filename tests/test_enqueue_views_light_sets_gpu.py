"""GPU: the enqueued batch of views under light sets (cgrt_enqueue_render_views_light_sets_device; Scene.enqueue_render_views_light_sets_tensor).

* Enqueued bytes equal the blocking bytes over whole buffers with sentinels: the three formats, depths 0, 2, 4 and 16, spherical lights
  and the exact walk; with one view it is the enqueued light-set batch.
* The call returns while a torch.cuda._sleep queued ahead on its stream is still running, and the batch runs behind it.
* A ticket's stats equal the blocking stats.
* Batches interleave on two streams with enqueued and blocking single frames, and every output stays correct.
* A child process with CGRT_STRIDED_WAVES=64 (tests/test_enqueue_capped_gpu.py's pattern) runs batches whose lists stride (checked from
  their stats): V >= 2, S >= 3, depth 4, spherical lights; its bytes equal the blocking bytes."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("rgb", "chw", "rgba8")
STAT_KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays", "levels")
PAD = 4096
CAP = 64


def _cams(pkg, V, W, H):
    base = pkg.scenes.default_camera(W, H).astype(np.float32)
    a = np.repeat(base[None, :], V, axis=0)
    k = np.arange(V, dtype=np.float32)
    a[:, 3] += np.float32(0.04) * k
    a[:, 4] += np.float32(-0.09) * k
    a[:, 6] *= np.float32(1.0) + np.float32(0.07) * k
    return np.ascontiguousarray(a, np.float32)


def _sets(pkg, sd):
    L = np.ascontiguousarray(np.asarray(sd.point_lights, np.float32).reshape(-1, 6))
    moved = L.copy()
    moved[:, 0:3] += np.float32([0.25, 0.1, -0.2])
    A = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
    Bl = A.copy()
    Bl[0, 0:3] += np.float32([0.2, -0.05, 0.1])
    sets = [L, np.concatenate([L * np.float32([1, 1, 1, 0.5, 0.25, 1.5]), moved]), np.zeros((0, 6), np.float32)]
    sph = [A, np.zeros((0, 7), np.float32), np.concatenate([Bl, A])]
    return sets, sph


def _shape(V, S, W, H, fmt):
    return {"rgb": (V, S, H, W, 3), "chw": (V, S, 3, H, W), "rgba8": (V, S, H, W, 4)}[fmt]


def _fenced(torch, shape, fmt):
    dtype = torch.uint8 if fmt == "rgba8" else torch.float32
    nbytes = int(np.prod(shape)) * (1 if fmt == "rgba8" else 4)
    buf = torch.full((PAD + nbytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[PAD : PAD + nbytes].fill_(0xFF if fmt != "rgba8" else 0x00)  # (NaN / zero alpha: an unwritten pixel shows)
    return buf, buf[PAD : PAD + nbytes].view(dtype).view(shape)


def _same_batch(torch, sc, cams, W, H, sets, fmt="rgb", stream=None, **kw):
    """Enqueued and blocking batch into fenced buffers: the whole buffers equal; the ticket's stats equal the blocking stats."""
    shape = _shape(len(cams), len(sets), W, H, fmt)
    b_e, o_e = _fenced(torch, shape, fmt)
    b_b, o_b = _fenced(torch, shape, fmt)
    _, t = sc.enqueue_render_views_light_sets_tensor(cams, W, H, sets, format=fmt, out=o_e, stream=stream, **kw)
    _, st = sc.render_views_light_sets_tensor(cams, W, H, sets, format=fmt, out=o_b, stream=stream, **kw)
    torch.cuda.synchronize()
    assert torch.equal(b_e, b_b), (fmt, sorted(kw))
    est = sc.enqueue_stats(t)
    for k in STAT_KEYS:
        assert est[k] == st[k], (fmt, k, est, st)
    return est, b_b[PAD:-PAD]


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.mark.parametrize("certified", [True, False])
def test_enqueued_bytes_equal_blocking_bytes(pkg, scene_data, torch, certified):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd, device=0)
    sc.set_walk(certified)
    W, H = 72, 48
    cams = _cams(pkg, 3, W, H)
    sets, sph = _sets(pkg, sd)
    soft = dict(spherical_sets=sph, units=pkg.unit_vector_table(900, 4), samples=5, seed=21)
    for depth in (0, 2, 4, 16):
        for fmt in FORMATS:
            est, _ = _same_batch(torch, sc, cams, W, H, sets, fmt, max_level=depth)
            if depth == 0:
                assert est["primary_rays"] == 0 and est["levels"] == 0
        est, _ = _same_batch(torch, sc, cams, W, H, sets, "rgb", max_level=depth, **soft)
        if depth >= 2:
            assert est["soft_shadow_rays"] > 0 and est["reflection_rays"] > 0
    # one view: the enqueued light-set batch, equal to cgrt_render_light_sets
    for depth in (2, 4):
        _, got = _same_batch(torch, sc, cams[:1], W, H, sets, "rgb", max_level=depth, **soft)
        ref, _ = sc.render_light_sets(cams[0], W, H, sets, max_level=depth, **soft)
        assert got.cpu().numpy().tobytes() == ref.tobytes(), depth
    # a view that sees nothing beside full ones, and a set without lights
    away = cams.copy()
    away[1, 0:3] = np.float32([50.0, 60.0, 70.0])
    _same_batch(torch, sc, away, W, H, sets, "rgba8", max_level=4, **soft)
    sc.close()


def _sleep_cycles(seconds):
    return int(seconds * 1e9 * 2.4)  # (~2.4 GHz shader clock; only the order of magnitude matters)


def test_call_does_not_wait_and_batch_waits_for_the_stream(pkg, scene_data, torch):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd, device=0)
    W, H = 128, 96
    cams = _cams(pkg, 3, W, H)
    sets, sph = _sets(pkg, sd)
    kw = dict(spherical_sets=sph, units=pkg.unit_vector_table(900, 4), samples=3, seed=2, max_level=3)
    s = torch.cuda.Stream()
    out = torch.empty((3, 3, H, W, 3), dtype=torch.float32, device="cuda")
    ref = torch.empty_like(out)
    with torch.cuda.stream(s):
        sc.render_views_light_sets_tensor(cams, W, H, sets, out=ref, stream=s, **kw)
        sc.enqueue_render_views_light_sets_tensor(cams, W, H, sets, out=out, stream=s, **kw)  # (warm: the workspace has its size)
    s.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(_sleep_cycles(0.2))
        out.fill_(float("nan"))  # (the batch must overwrite this, so it ran behind it)
        t0 = time.perf_counter()
        _, ticket = sc.enqueue_render_views_light_sets_tensor(cams, W, H, sets, out=out, stream=s, **kw)
        dt = time.perf_counter() - t0
        ev = torch.cuda.Event()
        ev.record(s)
    pending = not ev.query()
    s.synchronize()
    assert dt < 0.05, f"the enqueue call took {dt * 1e3:.1f} ms"
    assert pending, "the stream had finished when the call returned"
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), "the batch did not run behind the fill"
    _, st = sc.render_views_light_sets(cams, W, H, sets, **kw)
    est = sc.enqueue_stats(ticket)
    for k in STAT_KEYS:
        assert est[k] == st[k], (k, est, st)
    sc.close()


def test_batches_interleave_with_single_frames_on_two_streams(pkg, scene_data, torch):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd, device=0)
    W, H = 80, 56
    cams = _cams(pkg, 2, W, H)
    sets, sph = _sets(pkg, sd)
    kw = dict(spherical_sets=sph, units=pkg.unit_vector_table(900, 4), samples=2, seed=9)
    refs = [sc.render_views_light_sets_tensor(cams, W, H, sets, max_level=d, **kw)[0].clone() for d in (2, 4)]
    cam = pkg.scenes.default_camera(W, H)
    fref = [sc.render_tensor(cam, W, H, max_level=d)[0].clone() for d in (2, 4)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for i in range(12):
        s = streams[i % 2]
        d = i % 2
        with torch.cuda.stream(s):
            b = torch.empty_like(refs[d])
            f = torch.empty_like(fref[d])
            sc.enqueue_render_views_light_sets_tensor(cams, W, H, sets, out=b, stream=s, max_level=(2, 4)[d], **kw)
            if i % 3 == 0:
                sc.render_tensor(cam, W, H, out=f, stream=s, max_level=(2, 4)[d])
            else:
                sc.enqueue_render_tensor(cam, W, H, out=f, stream=s, max_level=(2, 4)[d])
            if i % 4 == 1:
                sc.render_views_light_sets_tensor(cams, W, H, sets, out=b, stream=s, max_level=(2, 4)[d], **kw)
            outs.append((d, b, f))
    torch.cuda.synchronize()
    for i, (d, b, f) in enumerate(outs):
        assert torch.equal(b.view(torch.int32), refs[d].view(torch.int32)), ("batch", i)
        assert torch.equal(f.view(torch.int32), fref[d].view(torch.int32)), ("frame", i)
    sc.close()


def test_enqueued_batch_with_the_smallest_cap(torch):
    env = dict(os.environ, CGRT_STRIDED_WAVES=str(CAP))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "capped batches ok" in r.stdout, r.stdout[-2000:]


# ---- the child process ----
def _child():
    sys.path.insert(0, ROOT)
    import torch  # (first: torch's HIP runtime is the one libcgrt.so binds to)

    import __graft_entry__ as entry

    pkg = entry.load_package()
    assert pkg.lib().cgrt_debug_strided_waves() == CAP, "the cap was not taken from CGRT_STRIDED_WAVES"
    sd = pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz"))
    sc = pkg.Scene(sd, device=0)
    W, H = 256, 160
    cams = _cams(pkg, 3, W, H)
    sets, sph = _sets(pkg, sd)
    sets = sets + [sets[0] * np.float32([1, 1, 1, 0.3, 0.3, 0.3])]
    sph = sph + [sph[2]]
    units = pkg.unit_vector_table(2048, 6)
    # a shading launch covers CAP * 64 = 4096 threads a pass, a trace launch 64 workgroups: lists above a few thousand entries stride
    est, _ = _same_batch(torch, sc, cams, W, H, sets, "rgb", max_level=4, spherical_sets=sph, units=units, samples=4, seed=3)
    print("capped batch:", est)
    # (two distinct positions: shadow_rays / 2 hits over the levels, most of them level 0's; four samples of each of three keys per hit)
    assert est["primary_rays"] == 3 * W * H > CAP * 64
    assert est["shadow_rays"] // 2 > 2 * CAP * 64 and est["soft_shadow_rays"] > 8 * CAP * 64 and est["levels"] >= 2, est
    for fmt in ("chw", "rgba8"):
        _same_batch(torch, sc, cams[:2], W, H, sets, fmt, max_level=4, spherical_sets=sph, units=units, samples=2, seed=1)
    sc.set_walk(False)
    _same_batch(torch, sc, cams, W, H, sets, "rgb", max_level=4, spherical_sets=sph, units=units, samples=2, seed=4)
    sc.close()
    print("capped batches ok")


if __name__ == "__main__":
    _child()
