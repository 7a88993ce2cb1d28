"""Host-side tests of the TRANSPOSED 4-wide nodes (cgrt_layout.h SubNode): 128 bytes as eight 16-byte quarters,
q0 = lo.x of children 0..3, q1 = hi.x, q2 = lo.y, q3 = hi.y, q4 = lo.z, q5 = hi.z, q6 = the four child references, q7 = word 0 the
leaf index of an accelerator root, the rest zero.  No GPU: host-only scenes."""
import numpy as np
import pytest

REF_NONE = 0xFFFFFFFF
REF_LEAF = 0x80000000
INF = np.float32(np.inf)


def _scenes(pkg, scene_data):
    return {"dragon5000": pkg.scenes.make_dragon(5000), "dragon87000": pkg.scenes.make_dragon(87_000),
            "irregular20000": pkg.scenes.make_dragon_irregular(20_000), "cornell": scene_data("cornell")}


@pytest.fixture(scope="module")
def built(pkg, scene_data):
    """name -> (Scene built host-only with a fast tree, its node table)."""
    pkg.set_fast_tree(1)
    try:
        out = {}
        for name, sd in _scenes(pkg, scene_data).items():
            sc = pkg.Scene(sd, device=-1)
            out[name] = (sc, sc.subnodes())
    finally:
        pkg.set_fast_tree(-1)
    return out


def test_pack_places_every_word_where_the_layout_says(pkg):
    boxes = np.arange(24, dtype=np.float32).reshape(4, 6) + np.float32(0.5)  # child c: lo = 6c + {0,1,2} + .5, hi = 6c + {3,4,5} + .5
    boxes[3] = [INF, INF, INF, -INF, -INF, -INF]                             # an absent child: the builder's empty box
    refs = np.array([10, REF_LEAF | (1 << 26) | 77, 12, REF_NONE], np.uint32)
    w = pkg.node_pack(boxes, refs, leaf_index=4242)
    f = w.view(np.float32)
    for a in range(3):
        assert np.array_equal(f[8 * a : 8 * a + 4], boxes[:, a]), f"quarter {2 * a}: lower {'xyz'[a]} of children 0..3"
        assert np.array_equal(f[8 * a + 4 : 8 * a + 8], boxes[:, 3 + a]), f"quarter {2 * a + 1}: upper {'xyz'[a]} of children 0..3"
    assert np.array_equal(w[24:28], refs) and w[28] == 4242 and not w[29:].any()
    b2, r2, li = pkg.node_unpack(w)
    assert np.array_equal(b2.view(np.uint32), boxes.view(np.uint32)) and np.array_equal(r2, refs) and li == 4242
    # every one of the 32 words belongs to exactly one field: a distinct value per word survives the round trip
    w = np.arange(100, 132, dtype=np.uint32)
    w[29:] = 0
    b2, r2, li = pkg.node_unpack(w)
    assert np.array_equal(pkg.node_pack(b2, r2, li), w)


@pytest.mark.parametrize("name", ["dragon5000", "dragon87000", "irregular20000", "cornell"])
def test_layout_check_passes(built, name):
    sc, t = built[name]
    sc.check_layout()
    assert sc.num_subnodes() > 0 and sc.num_subnodes() == 2 * len(t["words"]) and t["fast_root"] != REF_NONE


@pytest.mark.parametrize("name", ["dragon5000", "irregular20000"])
def test_layout_hash_does_not_depend_on_the_thread_count(pkg, scene_data, name):
    sd = _scenes(pkg, scene_data)[name]
    hashes = []
    try:
        for threads in (1, 3, 16):
            pkg.set_build_threads(threads)
            sc = pkg.Scene(sd, device=-1)
            hashes.append((sc.layout_hash(), sc.num_subnodes()))
    finally:
        pkg.set_build_threads(0)
    assert len(set(hashes)) == 1, hashes


@pytest.mark.parametrize("name", ["dragon5000", "dragon87000", "irregular20000", "cornell"])
def test_nodes_read_back_the_boxes_the_builder_stored(pkg, built, name):
    """The builder bounds every child of an accelerator node by the exact min / max over its triangles, so the box it stores for a
    child that is itself a node equals the union of that node's own child boxes, bit for bit: read back through the load helper, a
    parent's slot and its child's four slots must agree.  Absent children read back as the empty box with no reference, an
    accelerator root carries its leaf's index and every other node zero."""
    sc, t = built[name]
    words, base = t["words"], t["sub_base"]
    n = len(words)
    boxes = np.empty((n, 4, 6), np.float32)
    refs = np.empty((n, 4), np.uint32)
    leaf = np.empty(n, np.uint32)
    for i in range(n):
        boxes[i], refs[i], leaf[i] = pkg.node_unpack(words[i])
    # the same through the documented slot arithmetic, all nodes at once
    f = words.view(np.float32)
    for a in range(3):
        assert np.array_equal(f[:, 8 * a : 8 * a + 4].view(np.uint32), boxes[:, :, a].view(np.uint32))
        assert np.array_equal(f[:, 8 * a + 4 : 8 * a + 8].view(np.uint32), boxes[:, :, 3 + a].view(np.uint32))
    assert np.array_equal(words[:, 24:28], refs) and np.array_equal(words[:, 28], leaf) and not words[:, 29:].any()
    absent = refs == REF_NONE
    assert absent.any(), "some node has fewer than four children"
    assert (boxes[absent][:, :3] == INF).all() and (boxes[absent][:, 3:] == -INF).all()
    assert not absent[:, 0].any() and not absent[:, 1].any(), "a node has at least two children"
    # accelerator roots <-> leaf indices
    roots = t["leaf_roots"]
    has = roots != REF_NONE
    assert has.any() == (name != "cornell"), "the thin-leaf scene's leaves are runs (no accelerator): its nodes are the fast tree's alone"
    idx = (roots[has] - base) // 2
    assert ((roots[has] - base) % 2 == 0).all() and np.array_equal(leaf[idx], np.flatnonzero(has).astype(np.uint32))
    others = np.ones(n, bool)
    others[idx] = False
    assert not leaf[others].any()
    # parent slot == union of the child's slots, inside the in-leaf accelerators (reached from the leaves' roots)
    todo = list(idx)
    seen = 0
    while todo:
        i = todo.pop()
        for c in range(4):
            r = int(refs[i, c])
            if r == REF_NONE or (r & REF_LEAF):
                continue
            k = (r - base) // 2
            live = refs[k] != REF_NONE
            lo, hi = boxes[k][live][:, :3].min(axis=0), boxes[k][live][:, 3:].max(axis=0)
            assert np.array_equal(boxes[i, c, :3], lo) and np.array_equal(boxes[i, c, 3:], hi), (name, i, c)
            seen += 1
            todo.append(k)
    if name == "dragon87000":  # >= 42 triangles per reference leaf (at most 2^11 leaves) against 4 runs of 2 under one node
        assert seen > 0, "some accelerator is more than one node deep"
