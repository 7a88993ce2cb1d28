"""GPU: the bitwise-reproducible form of the sampler's adjoint (cgrt_sample_grid_grad_repro*; include/cgrt.h "Grid fields, the
bitwise-reproducible form of the sampler's adjoint") against the numpy restatement tests/grid_field_grad_repro_ref.py,
byte for byte.

* dims (2,2,2) (one cell: every point contends), (3,2,2), (17,9,5), (65,33,4), y spacing negative; n in {1, 63, 64, 65, 4 099} mixed
  points; both flags; the three input combinations; non-zero previous content.  Guard bytes (0xA5) around grad_values, the inputs and the
  workspace, the float buffers 4 bytes and the workspace 8 bytes off a 16-byte boundary; the workspace arrives full of 0xA5.
* The pile-up: 70 000 points (S = 21) into the one cell of 2 x 2 x 2, grads over 40 binades and both signs: the restatement's bytes,
  from three permutations, a second run, a side stream and four host threads with a workspace each.
* The workspace: 0xFF or zeros beforehand, the same bytes; too small, misaligned or NULL: CGRT_E_ARG and nothing written.
* The host form; untouched elements (-0, 0xA5A5A5A5, a signalling NaN); non-finite grads; the exact family against the float entry;
  no frame state moves; splat_grid_tensor, and autograd under torch.use_deterministic_algorithms(True)."""
import threading
import warnings

import numpy as np
import pytest

import grid_field_grad_ref as aref
import grid_field_grad_repro_ref as rref
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
SNAN, QNAN, NEG0 = 0x7FA00001, 0x7FC00000, 0x80000000
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

    def fill(self, byte):
        self.buf[self.lo : self.lo + self.n] = byte

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


def _workspace(dims, fill=None):
    """A guarded workspace of 12 bytes per element, 8 bytes off a 16-byte boundary, full of 0xA5 (or `fill`)."""
    g = Guarded(12 * dims[0] * dims[1] * dims[2], shift=8)
    assert g.ptr() % 16 == 8
    if fill is not None:
        g.fill(fill)
    return g


def _device_call(sc, o, sp, dims, p, gv, gg, prev, clamp=False, stream=0, fill=None):
    """One device-form call on guarded, misaligned buffers -> the (nz, ny, nx) float32 result; the guards and the inputs are checked."""
    tp, tout, ws = _misaligned(p), _misaligned(prev), _workspace(dims, fill)
    tgv = None if gv is None else _misaligned(gv)
    tgg = None if gg is None else _misaligned(gg)
    torch.cuda.synchronize()
    sc.sample_grid_grad_device(o, sp, dims, tp.ptr(), len(p), tgv.ptr() if tgv else 0, tgg.ptr() if tgg else 0, tout.ptr(), clamp=clamp, stream=stream,
                               reproducible=True, d_workspace_ptr=ws.ptr(), workspace_bytes=ws.n)
    torch.cuda.synchronize()
    assert tout.intact(), "guards of grad_values"
    assert ws.intact(), "guards of the workspace"
    for t, a in ((tp, p), (tgv, gv), (tgg, gg)):
        if t is not None:
            assert t.intact() and t.bytes().tobytes() == np.ascontiguousarray(a).tobytes(), "an input moved"
    return tout.bytes().view(F).reshape(dims[::-1]).copy()


# ---- bytes equal the restatement ----
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_bytes_equal_the_restatement(sc, dims, combo):
    use_v, use_g = COMBOS[combo]
    o, sp = aref.noise_grid(dims)  # (the y spacing is negative)
    prev = aref.noise_previous(dims)
    for n in COUNTS:
        p = aref.mixed_points(dims, o, sp, n)
        gv, gg = aref.noise_grads(n)
        gv, gg = (gv if use_v else None), (gg if use_g else None)
        for clamp in (False, True):
            want = rref.adjoint(o, sp, dims, p, gv, gg, clamp=clamp, previous=prev)
            got = _device_call(sc, o, sp, dims, p, gv, gg, prev, clamp=clamp)
            assert got.tobytes() == want.tobytes(), (dims, combo, n, clamp, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            if n == 4099:
                aref.check(got, aref.adjoint(o, sp, dims, p, gv, gg, clamp=clamp, previous=prev), prev, what=(dims, combo, clamp))


# ---- the pile-up ----
def test_pile_up_is_the_restatement_in_every_order_run_stream_and_thread(sc):
    o, sp, dims, p, gv, gg, prev = rref.pile_up(70000)
    assert rref.shift(len(p)) == 21
    want = rref.adjoint(o, sp, dims, p, gv, gg, previous=prev)
    inside, _, c = aref.contributions(o, sp, dims, p, gv, gg)
    assert inside.all() and np.count_nonzero(c) > 8 * 69000, "every point adds to all eight elements"
    mags = np.abs(c[c != 0])
    assert np.log2(mags.max() / mags.min()) > 40, "the contributions span more than 40 binades"
    assert (c > 0).any() and (c < 0).any()
    got = _device_call(sc, o, sp, dims, p, gv, gg, prev)
    assert got.tobytes() == want.tobytes(), "the restatement's bytes"
    assert _device_call(sc, o, sp, dims, p, gv, gg, prev).tobytes() == want.tobytes(), "a second run"
    rng = np.random.default_rng(2)
    for _ in range(3):
        order = rng.permutation(len(p))
        assert _device_call(sc, o, sp, dims, p[order], gv[order], gg[order], prev).tobytes() == want.tobytes(), "a permutation of the points"
    side = torch.cuda.Stream()
    assert _device_call(sc, o, sp, dims, p, gv, gg, prev, stream=side.cuda_stream).tobytes() == want.tobytes(), "a side stream"
    # four host threads, each with its own stream, output and workspace
    tp, tgv, tgg = _misaligned(p), _misaligned(gv), _misaligned(gg)
    outs, wss, streams = [_misaligned(prev) for _ in range(4)], [_workspace(dims) for _ in range(4)], [torch.cuda.Stream() for _ in range(4)]
    torch.cuda.synchronize()
    errors = []

    def work(t):
        try:
            sc.sample_grid_grad_device(o, sp, dims, tp.ptr(), len(p), tgv.ptr(), tgg.ptr(), outs[t].ptr(), stream=streams[t].cuda_stream,
                                       reproducible=True, d_workspace_ptr=wss[t].ptr(), workspace_bytes=wss[t].n)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for t in range(4):
        assert outs[t].bytes().tobytes() == want.tobytes() and outs[t].intact() and wss[t].intact(), ("thread", t)


# ---- the workspace ----
def test_workspace_contents_do_not_matter(sc):
    dims = (17, 9, 5)
    o, sp = aref.noise_grid(dims)
    p = aref.mixed_points(dims, o, sp, 4099)
    gv, gg = aref.noise_grads(4099)
    prev = aref.noise_previous(dims)
    want = rref.adjoint(o, sp, dims, p, gv, gg, previous=prev)
    assert _device_call(sc, o, sp, dims, p, gv, gg, prev, fill=0xFF).tobytes() == want.tobytes(), "a workspace full of 0xFF"
    assert _device_call(sc, o, sp, dims, p, gv, gg, prev, fill=0x00).tobytes() == want.tobytes(), "a zeroed workspace"
    assert sc.sample_grid_grad_repro_workspace(o, sp, dims) == 12 * 17 * 9 * 5


def test_bad_workspaces_are_refused_and_nothing_is_written(pkg, sc):
    dims = (17, 9, 5)
    o, sp = aref.noise_grid(dims)
    p = aref.mixed_points(dims, o, sp, 65)
    gv, gg = aref.noise_grads(65)
    prev = aref.noise_previous(dims)
    tp, tgv, tgg, tout, ws = _misaligned(p), _misaligned(gv), _misaligned(gg), _misaligned(prev), _workspace(dims)
    torch.cuda.synchronize()
    host = np.zeros(ws.n + 16, np.uint8)
    for kw in (dict(workspace_bytes=ws.n - 1), dict(workspace_bytes=0), dict(d_workspace_ptr=ws.ptr() + 4), dict(d_workspace_ptr=ws.ptr() + 1),
               dict(d_workspace_ptr=0), dict(d_workspace_ptr=0, workspace_bytes=0),
               dict(d_workspace_ptr=host.ctypes.data + (-host.ctypes.data) % 8)):  # (8-byte aligned host memory: not device memory)
        args = dict(dict(d_workspace_ptr=ws.ptr(), workspace_bytes=ws.n), **kw)
        with pytest.raises(pkg.CgrtError) as e:
            sc.sample_grid_grad_device(o, sp, dims, tp.ptr(), 65, tgv.ptr(), tgg.ptr(), tout.ptr(), reproducible=True, **args)
        assert e.value.code == -1, kw
    assert tout.bytes().tobytes() == prev.tobytes() and tout.intact(), "grad_values was written"
    assert (ws.bytes() == SENTINEL).all() and ws.intact() and not host.any(), "the workspace was written"
    # n == 0 skips the workspace's checks and touches nothing
    sc.sample_grid_grad_device(o, sp, dims, 0, 0, tgv.ptr(), tgg.ptr(), tout.ptr(), reproducible=True, d_workspace_ptr=0, workspace_bytes=0)
    assert tout.bytes().tobytes() == prev.tobytes() and (ws.bytes() == SENTINEL).all()


# ---- the host form ----
def test_host_form_gives_the_device_forms_bytes(sc):
    dims = (17, 9, 5)
    o, sp = aref.noise_grid(dims)
    prev = aref.noise_previous(dims)
    p = aref.mixed_points(dims, o, sp, 4099)
    gv, gg = aref.noise_grads(4099)
    for use_v, use_g in COMBOS.values():
        a, b = (gv if use_v else None), (gg if use_g else None)
        mine = prev.copy()
        back = sc.sample_grid_grad(o, sp, dims, p, a, b, grad_values=mine, clamp=True, reproducible=True)
        assert back is mine, "accumulated into in place"
        dev = _device_call(sc, o, sp, dims, p, a, b, prev, clamp=True)
        assert mine.tobytes() == dev.tobytes() == rref.adjoint(o, sp, dims, p, a, b, clamp=True, previous=prev).tobytes()
    fresh = sc.sample_grid_grad(o, sp, dims, p, gv, None, reproducible=True)
    assert fresh.shape == dims[::-1] and fresh.tobytes() == rref.adjoint(o, sp, dims, p, gv, None).tobytes()
    assert sc.sample_grid_grad(o, sp, dims, p[:0], gv[:0], None, reproducible=True).tobytes() == np.zeros(dims[::-1], F).tobytes()
    o, sp, dims, p, gv, gg, prev = rref.pile_up(70000)
    mine = prev.copy()
    sc.sample_grid_grad(o, sp, dims, p, gv, gg, grad_values=mine, reproducible=True)
    assert mine.tobytes() == rref.adjoint(o, sp, dims, p, gv, gg, previous=prev).tobytes(), "the pile-up through the host form"


# ---- untouched elements ----
@pytest.mark.parametrize("pattern", [NEG0, 0xA5A5A5A5, SNAN], ids=["minus-zero", "sentinel", "signalling-nan"])
def test_untouched_elements_keep_their_bytes(sc, pattern):
    dims = (5, 4, 3)
    o, sp = np.asarray([-1.0, 1.0, 0.0], F), np.asarray([0.5, -0.25, 2.0], F)
    ix, iy, iz = np.meshgrid(np.arange(0, 5, 2), np.arange(0, 4, 3), np.arange(3), indexing="ij")
    grid_pts = np.stack([ix, iy, iz], axis=-1).reshape(-1, 3)
    p = (o + grid_pts.astype(F) * sp).astype(F)
    gv = (np.arange(len(p)) + 1).astype(F)
    prev = np.full(dims[::-1], pattern, np.uint32).view(F)
    want = rref.adjoint(o, sp, dims, p, gv, None, previous=prev)
    got = _device_call(sc, o, sp, dims, p, gv, None, prev)
    assert got.tobytes() == want.tobytes()
    touched = np.zeros(dims[::-1], bool)
    touched[grid_pts[:, 2], grid_pts[:, 1], grid_pts[:, 0]] = True
    words = got.view(np.uint32)
    assert touched.sum() == len(p) and (words[~touched] == pattern).all() and (words[touched] != pattern).all(), "one element per grid point"
    # zero grads contribute zeros, which are not contributions: every element keeps its bytes
    got = _device_call(sc, o, sp, dims, p, np.zeros(len(p), F), np.zeros((len(p), 3), F), prev)
    assert (got.view(np.uint32) == pattern).all()
    # +x and -x into one element: the integer sum is 0 and the element is still touched
    two = np.repeat(p[:1], 2, axis=0)
    got = _device_call(sc, o, sp, dims, two, np.asarray([3.0, -3.0], F), None, prev)
    assert got.tobytes() == rref.adjoint(o, sp, dims, two, np.asarray([3.0, -3.0], F), None, previous=prev).tobytes()
    assert (got.view(np.uint32).reshape(-1)[1:] == pattern).all(), "the point sits on element 0 and touches it alone"
    if pattern != 0xA5A5A5A5:  # fl32(fl64(a) + 0): +0 for -0, the quiet NaN for the signalling one (the sentinel is a number and stays)
        assert got.view(np.uint32)[0, 0, 0] == (0 if pattern == NEG0 else QNAN)


# ---- non-finite inputs ----
def test_non_finite_grads(sc):
    dims = (17, 9, 5)
    o, sp = aref.noise_grid(dims)
    p = aref.mixed_points(dims, o, sp, 4099)
    gv, gg = (a.copy() for a in aref.noise_grads(4099))
    inside, index, _ = aref.contributions(o, sp, dims, p, gv, gg)
    out_rows, in_rows = np.flatnonzero(~inside), np.flatnonzero(inside)
    gv[out_rows], gg[out_rows] = np.nan, np.nan  # every outside point carries NaNs: none may arrive
    prev = aref.noise_previous(dims)
    got = _device_call(sc, o, sp, dims, p, gv, gg, prev)
    assert not np.isnan(got).any() and got.tobytes() == rref.adjoint(o, sp, dims, p, gv, gg, previous=prev).tobytes()
    # a NaN, a +inf, and a +inf with a -inf on inside points whose eight weights are all non-zero and whose cells do not meet
    _, _, weights = aref.contributions(o, sp, dims, p, np.ones(len(p), F), None)
    chosen, used = [], set()
    for r in in_rows:
        cells = set(index[r].tolist())
        if (weights[r] != 0).all() and not (cells & used):
            chosen.append(r), used.update(cells)
        if len(chosen) == 3:
            break
    r_nan, r_inf, r_pos = chosen
    gv[r_nan], gv[r_inf] = np.nan, np.inf
    p2, gv2, gg2 = np.vstack([p, p[r_pos][None]]), np.append(gv, F(-np.inf)), np.vstack([gg, gg[r_pos][None]])
    gv2[r_pos] = np.inf  # the last point repeats r_pos with the other infinity
    want = rref.adjoint(o, sp, dims, p2, gv2, gg2, previous=prev)
    got = _device_call(sc, o, sp, dims, p2, gv2, gg2, prev)
    assert got.tobytes() == want.tobytes()
    flat = got.reshape(-1)
    assert (flat[index[r_nan]].view(np.uint32) == QNAN).all() and (flat[index[r_pos]].view(np.uint32) == QNAN).all()
    assert (flat[index[r_inf]] == np.inf).all()
    assert np.isnan(flat).sum() == 16 and np.isinf(flat).sum() == 8


# ---- the exact family ----
@pytest.mark.parametrize("k", [-1, 0, 1])
@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_exact_family_equals_the_float_entry(sc, dims, k):
    o, sp, p, gv, gg, prev = aref.exact_family(dims, k)
    tp, tgv, tgg = (torch.from_numpy(a.copy()).cuda() for a in (p, gv, gg))
    for use_v, use_g in COMBOS.values():
        a, b = (gv if use_v else None), (gg if use_g else None)
        seq = aref.adjoint(o, sp, dims, p, a, b, previous=prev)["sequential"]
        got = _device_call(sc, o, sp, dims, p, a, b, prev)
        flt = sc.sample_grid_grad_tensor(o, sp, dims, tp, tgv if use_v else None, tgg if use_g else None, out=torch.from_numpy(prev.copy()).cuda())
        assert got.tobytes() == flt.cpu().numpy().tobytes() == seq.tobytes(), (dims, k, use_v, use_g)


# ---- nothing else moves ----
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
        a.sample_grid_grad(o, sp, dims, p, gv, gg, reproducible=True)
        tp, tgv, tgg = (torch.from_numpy(x.copy()).cuda() for x in (p, gv, gg))
        a.sample_grid_grad_tensor(o, sp, dims, tp, tgv, tgg, reproducible=True)
        a.splat_grid_tensor(tp, tgv, o, sp, dims, reproducible=True)
        tv = torch.zeros(dims[::-1], device="cuda", requires_grad=True)
        a.sample_grid_tensor(tv, o, sp, tp, outside=0.0, reproducible=True)["value"].sum().backward()
        torch.cuda.synchronize()
        assert a.device_bytes() == base, "no table is made or uploaded"
        for _ in range(3):
            ref_b = b.render(cam, W, H)
        after, after_b = a.render(cam, W, H), b.render(cam, W, H)
        assert after[0].tobytes() == before[0].tobytes() == after_b[0].tobytes() == ref_b[0].tobytes()
        assert a.last_render_path() == b.last_render_path() and path == 1, (path, a.last_render_path(), b.last_render_path())
        assert set(after[1]) == set(before[1]) == set(after_b[1]), "the stats keys"
        assert all(after[1][k] == before[1][k] == after_b[1][k] for k in KEYS)
        assert a.layout_hash() == b.layout_hash() and a.device_bytes() == b.device_bytes()
    finally:
        a.close()
        b.close()


# ---- Python ----
def _autograd_case():
    dims = (17, 9, 5)
    o, sp = aref.noise_grid(dims)
    p = aref.mixed_points(dims, o, sp, 4099)
    a, B = aref.noise_grads(4099, seed=21)
    values = np.random.default_rng(33).uniform(-1, 1, dims[::-1]).astype(F)
    return dims, o, sp, p, a, B, values


def test_splat_is_the_reproducible_adjoint_with_weights(sc):
    o, sp, dims, p, w, _, prev = rref.pile_up(70000)
    tp, tw = torch.from_numpy(p.copy()).cuda(), torch.from_numpy(w.copy()).cuda()
    a = sc.splat_grid_tensor(tp, tw, o, sp, dims, reproducible=True)
    b = sc.sample_grid_grad_tensor(o, sp, dims, tp, grad_value=tw, reproducible=True)
    assert a.shape == dims[::-1] and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == rref.adjoint(o, sp, dims, p, w, None).tobytes()
    mine = torch.from_numpy(prev.copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert sc.splat_grid_tensor(tp, tw, o, sp, dims, out=mine, clamp=True, stream=side, reproducible=True) is mine
    side.synchronize()
    assert mine.cpu().numpy().tobytes() == rref.adjoint(o, sp, dims, p, w, None, clamp=True, previous=prev).tobytes()
    tz = sc.sample_grid_grad_tensor(o, sp, dims, torch.zeros((0, 3), device="cuda"), torch.zeros((0,), device="cuda"), reproducible=True)
    assert tz.shape == dims[::-1] and not tz.any()


def test_autograd_in_deterministic_mode_with_the_keyword(sc):
    dims, o, sp, p, a, B, values = _autograd_case()
    tp, ta, tB = (torch.from_numpy(x.copy()).cuda() for x in (p, a, B))
    direct = sc.sample_grid_grad_tensor(o, sp, dims, tp, ta, tB, reproducible=True).cpu().numpy()
    assert direct.tobytes() == rref.adjoint(o, sp, dims, p, a, B).tobytes()
    grads = []
    try:
        torch.use_deterministic_algorithms(True)
        for _ in range(2):
            tv = torch.from_numpy(values.copy()).cuda().requires_grad_()
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                res = sc.sample_grid_tensor(tv, o, sp, tp, outside=0.0, reproducible=True)
                ((res["value"] * ta).sum() + (res["gradient"] * tB).sum()).backward()
                torch.cuda.synchronize()
            assert not seen, [str(w.message) for w in seen]
            grads.append(tv.grad.cpu().numpy())
        # without the keyword the recorded backward still raises
        tv = torch.from_numpy(values.copy()).cuda().requires_grad_()
        loss = sc.sample_grid_tensor(tv, o, sp, tp, outside=0.0, want="value")["value"].sum()
        with pytest.raises(RuntimeError, match="float atomics"):
            loss.backward()
    finally:
        torch.use_deterministic_algorithms(False)
    assert grads[0].tobytes() == grads[1].tobytes() == direct.tobytes(), "values.grad has the bytes of the direct call, in both runs"


def test_keyword_changes_no_byte_of_a_plain_forward(sc):
    dims, o, sp, p, a, B, values = _autograd_case()
    vw, gw, ins = gref.sample(values, o, sp, p, outside=0.0)
    tv, tp = torch.from_numpy(values.copy()).cuda(), torch.from_numpy(p.copy()).cuda()
    for flag in (False, True):
        res = sc.sample_grid_tensor(tv, o, sp, tp, outside=0.0, reproducible=flag)
        assert all(res[k].grad_fn is None and not res[k].requires_grad for k in res)
        assert res["value"].cpu().numpy().tobytes() == vw.tobytes() and res["gradient"].cpu().numpy().tobytes() == gw.tobytes()
        assert res["inside"].cpu().numpy().view(np.uint8).tobytes() == ins.tobytes()
    # recorded, the forward's bytes are the same with and without the keyword
    for flag in (False, True):
        res = sc.sample_grid_tensor(tv.clone().requires_grad_(), o, sp, tp, outside=0.0, reproducible=flag)
        assert res["value"].requires_grad and res["value"].detach().cpu().numpy().tobytes() == vw.tobytes()
        assert res["gradient"].detach().cpu().numpy().tobytes() == gw.tobytes()
