"""CPU tests of the OBJ/MTL loader of the C++ host mirror (cg-raytracer_amd/host/src/mesh.cpp, replaces src/mesh.cpp:58-166
without assimp) on small files committed under tests/golden/obj/ (written for these tests, so they exist everywhere -- the
reference's data/ directory does not travel).  Loader parity with assimp itself is unpinned (assimp 5.0.1 is absent from the
image); what is pinned here: the documented semantics (per-face-corner vertices, one mesh per object and material
run, objects in reverse file order, fan triangulation, flat normals when a face has none, relative indices, MTL fields), the
agreement of the C++ loader with the Python loader that made the committed scene fixtures, and the failure behaviour:
an index that is 0, out of range, or not a number makes loadMesh print upstream's message and throw (mesh.cpp:66-71)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

OBJ = os.path.join(GOLDEN, "obj")


def test_small_obj_semantics(pkg):
    sd = pkg.host_load_obj(os.path.join(OBJ, "small.obj"))
    # objects in reverse file order; inside an object one mesh per material run
    assert sd.nmesh == 4 and sd.ntris == 5
    assert sd.tri_mesh.tolist() == [0, 1, 2, 2, 3]
    # mesh 0: `second`, default material (no usemtl yet in that object -> the run keeps the previous material name "mirror")
    mirror = [0.1, 0.1, 0.1, 0.9, 0.9, 0.9, 200.0, 1.0]
    red = [0.8, 0.1, 0.1, 0.2, 0.2, 0.2, 12.0, 1.0]
    assert np.allclose(sd.materials[0], mirror) and np.allclose(sd.materials[1], red)
    assert np.allclose(sd.materials[2], red) and np.allclose(sd.materials[3], mirror)
    # per-face-corner vertices: 3 + 3 + 4 + 3
    assert len(sd.pos_nrm) == 13
    # the face given with negative indices is the triangle (0,0,2) (1,0,2) (0,1,2), normals generated: flat +z
    assert np.array_equal(sd.pos_nrm[0:3, 0:3], np.float32([[0, 0, 2], [1, 0, 2], [0, 1, 2]]))
    assert np.allclose(sd.pos_nrm[0:3, 3:6], [0, 0, 1])
    # the quad is fan-triangulated from its first corner
    quad = sd.tri[sd.tri_mesh == 2]
    assert (quad - quad.min()).tolist() == [[0, 1, 2], [0, 2, 3]]
    # `f 1 2 3` has no normals: generated flat normal
    assert np.allclose(sd.pos_nrm[sd.tri[4], 3:6], [0, 0, 1])


def test_cpp_loader_equals_python_loader(pkg):
    for normalize in (False, True):
        a = pkg.host_load_obj(os.path.join(OBJ, "small.obj"), normalize=normalize)
        b = pkg.scenes.load_obj(os.path.join(OBJ, "small.obj"), normalize=normalize)
        assert np.array_equal(a.tri, b.tri) and np.array_equal(a.tri_mesh, b.tri_mesh)
        assert a.pos_nrm.tobytes() == b.pos_nrm.tobytes() and a.materials.tobytes() == b.materials.tobytes()
    n = pkg.host_load_obj(os.path.join(OBJ, "small.obj"), normalize=True)
    assert np.abs(np.linalg.norm(n.pos_nrm[:, 0:3], axis=1).max() - 1.0) < 1e-6  # centred, farthest vertex at distance 1 (mesh.cpp:143-166)


def test_exported_token_forms(pkg):
    """forms.obj: vt lines and v/vt pairs (normals generated), v/vt/vn triplets whose normal is the THIRD index (the given
    normals differ from the flat ones, and reading the vt index as the normal would pick another normal or run past the list),
    relative triplets, g groups (objects in reverse file order), s lines (ignored), two usemtl runs in one group, and a
    material that stays current across groups.  The C++ and the Python loader must agree bit for bit."""
    path = os.path.join(OBJ, "forms.obj")
    sd = pkg.host_load_obj(path)
    py = pkg.scenes.load_obj(path)
    assert sd.tri.tobytes() == py.tri.tobytes() and sd.tri_mesh.tobytes() == py.tri_mesh.tobytes()
    assert sd.pos_nrm.tobytes() == py.pos_nrm.tobytes() and sd.materials.tobytes() == py.materials.tobytes()
    # groups reversed: `last` (mirror, kept from `side`), `side` (red run, mirror run), then the faces before any group (default)
    assert sd.nmesh == 4 and sd.ntris == 4 and sd.tri_mesh.tolist() == [0, 1, 2, 3]
    mirror = [0.1, 0.1, 0.1, 0.9, 0.9, 0.9, 200.0, 1.0]
    red = [0.8, 0.1, 0.1, 0.2, 0.2, 0.2, 12.0, 1.0]
    default = [0.6, 0.6, 0.6, 0.0, 0.0, 0.0, 0.0, 1.0]
    assert np.array_equal(sd.materials, np.float32([mirror, red, mirror, default]))
    P = np.float32([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 3]])
    corners = {0: ([0, 1, 2], [1, 0, 0]),   # f -4/-3/-1 -3/-2/-1 -2/-1/-1: vertices 1 2 3, normal 2
               1: ([0, 1, 3], [1, 0, 0]),   # f 1/1/2 2/2/2 4/3/2 (its flat normal would be (0, -1, 0))
               2: ([1, 2, 3], [0, 0, -1]),  # f 2/1/1 3/2/1 4/3/1
               3: ([0, 2, 1], [0, 0, -1])}  # f 1/1 3/3 2/2: no normals, flat normal of (0,2,0) x (2,0,0)
    for m, (vi, nrm) in corners.items():
        rows = sd.pos_nrm[sd.tri[sd.tri_mesh == m][0]]
        assert np.array_equal(rows[:, 0:3], P[vi]), m
        assert np.array_equal(rows[:, 3:6], np.float32([nrm] * 3)), m


@pytest.mark.parametrize("name", ["bad_out_of_range", "bad_zero_index", "bad_negative", "bad_token", "bad_normal_index", "does_not_exist"])
def test_invalid_files_throw_like_upstream(pkg, name, capfd):
    """Malformed faces are REJECTED with upstream's message and a bare exception (mesh.cpp:60-71).  PARITY UNPINNED: which malformed
    faces assimp 5.0.1 refuses rather than repairs or skips is recorded nowhere in the reference and assimp is not importable
    here; the bad_*.obj fixtures are this repo's own expectation (an index that cannot be resolved must not become a triangle),
    not a statement about upstream's rejected set."""
    with pytest.raises(RuntimeError):
        pkg.host_load_obj(os.path.join(OBJ, name + ".obj"))
    err = capfd.readouterr().err
    assert ("does not exist" in err) if name == "does_not_exist" else ("Assimp failed to load mesh file" in err)
