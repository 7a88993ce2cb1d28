"""GPU: the sampler's adjoint (cgrt_sample_grid_grad*; include/cgrt.h "Grid fields, the adjoint of the sampler") against
the numpy restatement tests/grid_field_grad_ref.py.

* Bound family: dims (2,2,2) (one cell: every point contends), (3,2,2), (17,9,5), (65,33,4), y spacing negative; n in {1, 63, 64, 65,
  4 099} mixed points (grid points, faces, inside, outside, NaN, inf); both flags; grad_value only, grad_gradient only, both; noise grads
  on non-zero noise.  Every element within gamma(m + 1) S + (m + 1) 2^-126 of the float64 sum of the float32 contributions; elements
  with m = 0 keep their bits.  Guard bytes (0xA5) around every buffer, all of them 4 bytes off a 16-byte boundary.
* Exact family (every sum exact in every order): bit for bit equal to the restatement for the device form, the host form, a side stream
  and four host threads; two calls into one tensor equal one call on the concatenated points.
* The zero-contribution rule on a grid of -0.0; n == 0; refusals before any work; no frame state moves; splat_grid_tensor.
* Autograd through sample_grid_tensor, and five descent steps on a least-squares fit."""
import threading

import numpy as np
import pytest

import grid_field_grad_ref as aref
import grid_field_ref as gref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
SENTINEL = 0xA5
PAD = 256
DIMS = ((2, 2, 2), (3, 2, 2), (17, 9, 5), (65, 33, 4))
COUNTS = (1, 63, 64, 65, 4099)
COMBOS = {"value": (True, False), "gradient": (False, True), "both": (True, True)}
KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays", "levels")
ids = lambda d: "x".join(map(str, d))  # noqa: E731


@pytest.fixture(scope="module")
def sc(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=0)
    yield s
    s.close()


class Guarded:
    """nbytes of device memory between two guards, all of it 0xA5 before the call; `shift` moves it off 16-byte alignment."""

    def __init__(self, nbytes, shift=0):
        self.n, self.lo = int(nbytes), PAD + shift
        self.buf = torch.full((self.n + 2 * PAD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def bytes(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()[self.lo : self.lo + self.n]

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        return bool((b[: self.lo] == SENTINEL).all() and (b[self.lo + self.n :] == SENTINEL).all())


def _misaligned(a):
    """A device copy of a float32 array that starts 4 bytes off a 16-byte boundary."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    g = Guarded(len(raw), shift=4)
    g.buf[g.lo : g.lo + g.n] = torch.from_numpy(raw.copy()).cuda()
    assert g.ptr() % 16 == 4
    return g


def _device_call(sc, o, sp, dims, p, gv, gg, prev, clamp=False, stream=0):
    """One device-form call on guarded, misaligned buffers -> the (nz, ny, nx) float32 result; the guards and the inputs are checked."""
    tp, tout = _misaligned(p), _misaligned(prev)
    tgv = None if gv is None else _misaligned(gv)
    tgg = None if gg is None else _misaligned(gg)
    torch.cuda.synchronize()
    sc.sample_grid_grad_device(o, sp, dims, tp.ptr(), len(p), tgv.ptr() if tgv else 0, tgg.ptr() if tgg else 0, tout.ptr(), clamp=clamp, stream=stream)
    torch.cuda.synchronize()
    assert tout.intact(), "guards of grad_values"
    for t, a in ((tp, p), (tgv, gv), (tgg, gg)):
        if t is not None:
            assert t.intact() and t.bytes().tobytes() == np.ascontiguousarray(a).tobytes(), "an input moved"
    return tout.bytes().view(F).reshape(dims[::-1]).copy()


# ---- the bound family ----
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_bound_family(sc, dims, combo):
    use_v, use_g = COMBOS[combo]
    o, sp = aref.noise_grid(dims)
    prev = aref.noise_previous(dims)
    worst = 0.0
    for n in COUNTS:
        p = aref.mixed_points(dims, o, sp, n)
        gv, gg = aref.noise_grads(n)
        gv, gg = (gv if use_v else None), (gg if use_g else None)
        for clamp in (False, True):
            res = aref.adjoint(o, sp, dims, p, gv, gg, clamp=clamp, previous=prev)
            got = _device_call(sc, o, sp, dims, p, gv, gg, prev, clamp=clamp)
            worst = max(worst, aref.check(got, res, prev, what=(dims, combo, n, clamp)))
            if n == 4099 and dims == (2, 2, 2):
                assert res["m"].max() > 2000, "one cell: every inside point contends"
    print(f"largest error / bound, {dims} {combo}: {worst:.4f}")


def test_bound_family_host_form(sc):
    dims = (17, 9, 5)
    o, sp = aref.noise_grid(dims)
    prev = aref.noise_previous(dims)
    p = aref.mixed_points(dims, o, sp, 4099)
    gv, gg = aref.noise_grads(4099)
    for use_v, use_g in COMBOS.values():
        a, b = (gv if use_v else None), (gg if use_g else None)
        mine = prev.copy()
        back = sc.sample_grid_grad(o, sp, dims, p, a, b, grad_values=mine, clamp=True)
        assert back is mine, "accumulated into in place"
        aref.check(mine, aref.adjoint(o, sp, dims, p, a, b, clamp=True, previous=prev), prev)
    fresh = sc.sample_grid_grad(o, sp, dims, p, gv, None)
    assert fresh.shape == dims[::-1] and fresh.dtype == F
    aref.check(fresh, aref.adjoint(o, sp, dims, p, gv, None))


def test_nan_grads_stay_out_or_arrive(sc):
    dims = (17, 9, 5)
    o, sp = aref.noise_grid(dims)
    p = aref.mixed_points(dims, o, sp, 4099)
    gv, gg = (a.copy() for a in aref.noise_grads(4099))
    inside, _, _ = gref.cell(o, sp, dims, p)
    out_rows, in_rows = np.flatnonzero(~inside), np.flatnonzero(inside)
    gv[out_rows], gg[out_rows] = np.nan, np.nan  # every outside point carries NaNs: none may arrive
    prev = aref.noise_previous(dims)
    got = _device_call(sc, o, sp, dims, p, gv, gg, prev)
    assert not np.isnan(got).any()
    aref.check(got, aref.adjoint(o, sp, dims, p, gv, gg, previous=prev), prev)
    gv[in_rows[17]] = np.nan
    res = aref.adjoint(o, sp, dims, p, gv, gg, previous=prev)
    got = _device_call(sc, o, sp, dims, p, gv, gg, prev)
    assert np.isnan(res["exact"]).sum() == 8
    aref.check(got, res, prev)


# ---- the exact family ----
@pytest.mark.parametrize("k", [-1, 0, 1])
@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_exact_family_device_form(sc, dims, k):
    o, sp, p, gv, gg, prev = aref.exact_family(dims, k)
    for use_v, use_g in COMBOS.values():
        a, b = (gv if use_v else None), (gg if use_g else None)
        res = aref.adjoint(o, sp, dims, p, a, b, previous=prev)
        assert res["S"].max() < 2.0 ** 12 and np.array_equal(res["sequential"].astype(np.float64), res["exact"])
        got = _device_call(sc, o, sp, dims, p, a, b, prev)
        assert got.tobytes() == res["sequential"].tobytes(), (dims, k, use_v, use_g)


def test_exact_family_host_form_side_stream_and_threads(sc):
    dims = (17, 9, 5)
    cases = [aref.exact_family(dims, k, seed) for k, seed in ((-1, 1), (0, 2), (1, 3), (0, 4))]
    refs = [aref.adjoint(o, sp, dims, p, gv, gg, previous=prev)["sequential"] for (o, sp, p, gv, gg, prev) in cases]
    o, sp, p, gv, gg, prev = cases[0]
    mine = prev.copy()
    sc.sample_grid_grad(o, sp, dims, p, gv, gg, grad_values=mine)
    assert mine.tobytes() == refs[0].tobytes(), "host form"
    side = torch.cuda.Stream()
    got = _device_call(sc, o, sp, dims, p, gv, gg, prev, stream=side.cuda_stream)
    assert got.tobytes() == refs[0].tobytes(), "side stream"
    tp, tgv, tgg = (torch.from_numpy(a.copy()).cuda() for a in (p, gv, gg))
    tout = torch.from_numpy(prev.copy()).cuda()
    torch.cuda.synchronize()
    back = sc.sample_grid_grad_tensor(o, sp, dims, tp, tgv, tgg, out=tout, stream=side)
    side.synchronize()
    assert back is tout and tout.cpu().numpy().tobytes() == refs[0].tobytes(), "tensor form on a side stream"
    results, errors = {}, []

    def work(t):
        try:
            for it in range(3):
                j = (t + it) % 4
                o, sp, p, gv, gg, prev = cases[j]
                grid = prev.copy()  # this thread's own
                sc.sample_grid_grad(o, sp, dims, p, gv, gg, grad_values=grid)
                results[(t, it)] = (j, grid)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert len(results) == 12
    for (t, it), (j, grid) in results.items():
        assert grid.tobytes() == refs[j].tobytes(), ("host form, threaded", t, it)


def test_two_calls_accumulate_like_one(sc):
    dims = (17, 9, 5)
    o, sp, p, gv, gg, prev = aref.exact_family(dims, 0)
    half = len(p) // 2 + 1
    tp, tgv, tgg = (torch.from_numpy(a.copy()).cuda() for a in (p, gv, gg))
    one = sc.sample_grid_grad_tensor(o, sp, dims, tp, tgv, tgg, out=torch.from_numpy(prev.copy()).cuda())
    two = torch.from_numpy(prev.copy()).cuda()
    sc.sample_grid_grad_tensor(o, sp, dims, tp[:half].contiguous(), tgv[:half].contiguous(), tgg[:half].contiguous(), out=two)
    sc.sample_grid_grad_tensor(o, sp, dims, tp[half:].contiguous(), tgv[half:].contiguous(), tgg[half:].contiguous(), out=two)
    want = aref.adjoint(o, sp, dims, p, gv, gg, previous=prev)["sequential"]
    assert one.cpu().numpy().tobytes() == want.tobytes() and two.cpu().numpy().tobytes() == want.tobytes()


# ---- zeros, empty calls, refusals ----
def test_zero_contributions_keep_the_bits(sc):
    dims = (5, 4, 3)
    o, sp = np.asarray([-1.0, 1.0, 0.0], F), np.asarray([0.5, -0.25, 2.0], F)
    ix, iy, iz = np.meshgrid(np.arange(0, 5, 2), np.arange(0, 4, 3), np.arange(3), indexing="ij")
    grid_pts = np.stack([ix, iy, iz], axis=-1).reshape(-1, 3)
    p = (o + grid_pts.astype(F) * sp).astype(F)
    gv = (np.arange(len(p)) + 1).astype(F)
    prev = np.full(dims[::-1], -0.0, F)
    res = aref.adjoint(o, sp, dims, p, gv, None, previous=prev)
    assert res["m"].sum() == len(p) and res["m"].max() == 1
    got = _device_call(sc, o, sp, dims, p, gv, None, prev)
    assert got.tobytes() == res["sequential"].tobytes()
    assert (got.view(np.uint32)[res["m"] == 0] == 0x80000000).all(), "an untouched element keeps its -0"
    host = prev.copy()
    sc.sample_grid_grad(o, sp, dims, p, gv, None, grad_values=host)
    assert host.tobytes() == res["sequential"].tobytes()
    # zero grads contribute zeros, which are not added either
    got = _device_call(sc, o, sp, dims, p, np.zeros(len(p), F), np.zeros((len(p), 3), F), prev)
    assert (got.view(np.uint32) == 0x80000000).all()


def test_empty_call_and_refusals_touch_nothing(pkg, sc):
    dims = (17, 9, 5)
    o, sp = aref.noise_grid(dims)
    p = aref.mixed_points(dims, o, sp, 65)
    gv, gg = aref.noise_grads(65)
    prev = aref.noise_previous(dims)
    tp, tgv, tgg, tout = _misaligned(p), _misaligned(gv), _misaligned(gg), _misaligned(prev)
    torch.cuda.synchronize()
    sc.sample_grid_grad_device(o, sp, dims, 0, 0, tgv.ptr(), tgg.ptr(), tout.ptr())  # n == 0 succeeds
    assert tout.bytes().tobytes() == prev.tobytes() and tout.intact()
    host = np.zeros(prev.nbytes + 16, np.uint8)
    for kw in (dict(d_grad_values_ptr=tout.ptr() + 2), dict(d_grad_values_ptr=host.ctypes.data + (-host.ctypes.data) % 4),
               dict(d_grad_values_ptr=tout.ptr(), d_grad_value_ptr=0, d_grad_gradient_ptr=0),
               dict(d_grad_values_ptr=tout.ptr(), d_grad_value_ptr=tgv.ptr() + 1)):
        args = dict(dict(d_points_ptr=tp.ptr(), n=65, d_grad_value_ptr=tgv.ptr(), d_grad_gradient_ptr=tgg.ptr()), **kw)
        with pytest.raises(pkg.CgrtError) as e:
            sc.sample_grid_grad_device(o, sp, dims, **args)
        assert e.value.code == -1, kw
    assert tout.bytes().tobytes() == prev.tobytes() and tout.intact() and not host.any()
    assert sc.sample_grid_grad(o, sp, dims, p[:0], gv[:0], None).tobytes() == np.zeros(dims[::-1], F).tobytes()
    tz = sc.sample_grid_grad_tensor(o, sp, dims, torch.zeros((0, 3), device="cuda"), torch.zeros((0,), device="cuda"))
    assert tz.shape == dims[::-1] and not tz.any()
    with pytest.raises(ValueError):
        sc.sample_grid_grad_tensor(o, sp, dims, torch.zeros((4, 3), device="cuda"))
    with pytest.raises(ValueError):
        sc.sample_grid_grad_tensor(o, sp, dims, torch.zeros((4, 3), device="cuda"), torch.zeros((5,), device="cuda"))


def test_nothing_else_moves(pkg, scene_data):
    sd = scene_data("cornell")
    a, b = pkg.Scene(sd, device=0), pkg.Scene(sd, device=0)
    try:
        assert a.device_bytes() == b.device_bytes() and a.layout_hash() == b.layout_hash()
        W, H = 64, 48
        cam = pkg.scenes.default_camera(W, H)
        for _ in range(3):
            before = a.render(cam, W, H)
        path = a.last_render_path()
        base = a.device_bytes()
        dims = (17, 9, 5)
        o, sp = aref.noise_grid(dims)
        p = aref.mixed_points(dims, o, sp, 65)
        gv, gg = aref.noise_grads(65)
        a.sample_grid_grad(o, sp, dims, p, gv, gg)
        tp, tgv, tgg = (torch.from_numpy(x.copy()).cuda() for x in (p, gv, gg))
        a.sample_grid_grad_tensor(o, sp, dims, tp, tgv, tgg)
        a.splat_grid_tensor(tp, tgv, o, sp, dims)
        tv = torch.zeros(dims[::-1], device="cuda", requires_grad=True)
        a.sample_grid_tensor(tv, o, sp, tp, outside=0.0)["value"].sum().backward()
        torch.cuda.synchronize()
        assert a.device_bytes() == base, "no table is made or uploaded"
        for _ in range(3):
            ref_b = b.render(cam, W, H)
        after, after_b = a.render(cam, W, H), b.render(cam, W, H)
        assert after[0].tobytes() == before[0].tobytes() == after_b[0].tobytes() == ref_b[0].tobytes()
        assert a.last_render_path() == b.last_render_path() and path == 1, (path, a.last_render_path(), b.last_render_path())
        assert all(after[1][k] == before[1][k] == after_b[1][k] for k in KEYS)
        assert a.layout_hash() == b.layout_hash() and a.device_bytes() == b.device_bytes()
    finally:
        a.close()
        b.close()


def test_splat_is_the_adjoint_with_weights(sc):
    dims = (17, 9, 5)
    o, sp, p, gv, _, prev = aref.exact_family(dims, 1)
    tp, tw = torch.from_numpy(p.copy()).cuda(), torch.from_numpy(gv.copy()).cuda()
    a = sc.splat_grid_tensor(tp, tw, o, sp, dims)
    b = sc.sample_grid_grad_tensor(o, sp, dims, tp, grad_value=tw)
    want = aref.adjoint(o, sp, dims, p, gv, None)["sequential"]
    assert a.shape == dims[::-1] and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == want.tobytes()
    mine = torch.from_numpy(prev.copy()).cuda()
    assert sc.splat_grid_tensor(tp, tw, o, sp, dims, out=mine, clamp=True) is mine
    assert mine.cpu().numpy().tobytes() == aref.adjoint(o, sp, dims, p, gv, None, clamp=True, previous=prev)["sequential"].tobytes()
    # mass is conserved: the weights of a point sum to one (exactly, in this family)
    assert float(a.double().sum()) == float(gv.astype(np.float64).sum())


# ---- autograd ----
def _autograd_case():
    dims = (17, 9, 5)
    o, sp = aref.noise_grid(dims)
    p = aref.mixed_points(dims, o, sp, 4099)
    a, B = aref.noise_grads(4099, seed=21)
    values = np.random.default_rng(33).uniform(-1, 1, dims[::-1]).astype(F)
    return dims, o, sp, p, a, B, values


def test_autograd(sc):
    dims, o, sp, p, a, B, values = _autograd_case()
    tv = torch.from_numpy(values.copy()).cuda().requires_grad_(True)
    tp = torch.from_numpy(p.copy()).cuda().requires_grad_(True)
    ta, tB = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(B.copy()).cuda()
    res = sc.sample_grid_tensor(tv, o, sp, tp, outside=0.0)
    assert res["value"].requires_grad and res["gradient"].requires_grad and not res["inside"].requires_grad
    assert res["inside"].dtype == torch.bool
    vw, gw, ins = gref.sample(values, o, sp, p, outside=0.0)
    assert res["value"].detach().cpu().numpy().tobytes() == vw.tobytes() and res["gradient"].detach().cpu().numpy().tobytes() == gw.tobytes()
    assert res["inside"].cpu().numpy().view(np.uint8).tobytes() == ins.tobytes()
    loss = (res["value"] * ta).sum() + (res["gradient"] * tB).sum()
    g_values, g_points = torch.autograd.grad(loss, [tv, tp])
    aref.check(g_values.cpu().numpy(), aref.adjoint(o, sp, dims, p, a, B), what="d loss / d values")
    want_points = (a[:, None] * gw.view(F)).astype(F)
    assert g_points.cpu().numpy().tobytes() == want_points.tobytes(), "d loss / d points = a[:, None] * gradient, bit for bit"
    # value alone (the gradient is computed internally), and the gradient output alone
    tv2 = torch.from_numpy(values.copy()).cuda().requires_grad_(True)
    res = sc.sample_grid_tensor(tv2, o, sp, tp, outside=0.0, want="value")
    assert set(res) == {"value"}
    g_values, g_points = torch.autograd.grad((res["value"] * ta).sum(), [tv2, tp])
    aref.check(g_values.cpu().numpy(), aref.adjoint(o, sp, dims, p, a, None), what="value only")
    assert g_points.cpu().numpy().tobytes() == want_points.tobytes()
    res = sc.sample_grid_tensor(tv2, o, sp, tp.detach(), outside=0.0, want=("gradient", "inside"))
    (g_values,) = torch.autograd.grad((res["gradient"] * tB).sum(), [tv2])
    aref.check(g_values.cpu().numpy(), aref.adjoint(o, sp, dims, p, None, B), what="gradient only")
    with pytest.raises(ValueError):
        sc.sample_grid_tensor(tv2, o, sp, tp, out={"value": torch.zeros(4099, device="cuda")})


def test_autograd_off_is_the_plain_call(sc):
    dims, o, sp, p, a, B, values = _autograd_case()
    vw, gw, ins = gref.sample(values, o, sp, p, outside=0.0)
    tv, tp = torch.from_numpy(values.copy()).cuda(), torch.from_numpy(p.copy()).cuda()
    res = sc.sample_grid_tensor(tv, o, sp, tp, outside=0.0)
    assert all(res[k].grad_fn is None and not res[k].requires_grad for k in res)
    assert res["value"].cpu().numpy().tobytes() == vw.tobytes() and res["gradient"].cpu().numpy().tobytes() == gw.tobytes()
    assert res["inside"].cpu().numpy().view(np.uint8).tobytes() == ins.tobytes()
    with torch.no_grad():  # grad mode off: a tensor that requires grad takes the plain path as well, out= included
        mine = torch.zeros(4099, device="cuda")
        res = sc.sample_grid_tensor(tv.clone().requires_grad_(True), o, sp, tp, outside=0.0, want="value", out={"value": mine})
    assert res["value"] is mine and mine.cpu().numpy().tobytes() == vw.tobytes()


def test_autograd_in_deterministic_mode(sc):
    dims, o, sp, p, a, B, values = _autograd_case()
    tp = torch.from_numpy(p.copy()).cuda()
    try:
        torch.use_deterministic_algorithms(True)
        tv = torch.from_numpy(values.copy()).cuda().requires_grad_(True)
        loss = sc.sample_grid_tensor(tv, o, sp, tp, outside=0.0, want="value")["value"].sum()
        with pytest.raises(RuntimeError, match="float atomics"):
            loss.backward()
        torch.use_deterministic_algorithms(True, warn_only=True)
        tv = torch.from_numpy(values.copy()).cuda().requires_grad_(True)
        loss = sc.sample_grid_tensor(tv, o, sp, tp, outside=0.0, want="value")["value"].sum()
        with pytest.warns(UserWarning, match="float atomics"):
            loss.backward()
        aref.check(tv.grad.cpu().numpy(), aref.adjoint(o, sp, dims, p, np.ones(len(p), F), None))
    finally:
        torch.use_deterministic_algorithms(False)


def test_descent_on_a_least_squares_fit(sc):
    """Five plain gradient steps on 1/2 sum (value - y)^2 from a zero grid.  value = A v with A the (n, N) matrix of trilinear weights:
    non-negative, rows summing to 1, so |A|_inf = 1 and |A|_2^2 <= |A|_1 |A|_inf = the largest column sum.  The step 1 / (largest column
    sum) is therefore at most 1 / lambda_max(A^T A) and every step lowers the loss strictly while the gradient is not zero."""
    dims = (17, 9, 5)
    o, sp = aref.noise_grid(dims)
    rng = np.random.default_rng(12)
    p = rng.uniform(-1.19, 1.19, (4099, 3)).astype(F)
    y = (np.linalg.norm(p.astype(np.float64), axis=1) - 0.8).astype(F)
    tp, ty = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
    columns = sc.splat_grid_tensor(tp, torch.ones(len(p), device="cuda"), o, sp, dims)
    step = 1.0 / float(columns.max())
    v = torch.zeros(dims[::-1], device="cuda", requires_grad=True)
    losses = []
    for _ in range(6):
        res = sc.sample_grid_tensor(v, o, sp, tp, want=("value", "inside"))
        assert bool(res["inside"].all())
        r = res["value"] - ty
        losses.append(float(0.5 * (r.detach().double() ** 2).sum()))
        (g,) = torch.autograd.grad(0.5 * (r * r).sum(), [v])
        with torch.no_grad():
            v -= step * g
    print("losses:", losses)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
