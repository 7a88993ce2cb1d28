"""How many point-light shadow verdicts of a frame reach its pixels (CPU, oracle only).

k_shade adds dif + spec of an unoccluded light (main.cpp:219-232): both are zero when the light is behind the surface (dot(toLight, n)
<= 0 and dot(refl, toLight) <= 0) or the material / light is black, and a level's colour reaches the pixel only through the ks of
every level above it (main.cpp:262).  A verdict whose flip leaves (dif + spec) * (product of the parents' ks) at zero cannot change
the pixel: a frame comparison is blind to it.  This walks the reference's recursion (camera rays, then mirror rays where ks.z > 0.01,
main.cpp:246) level by level on the oracle and counts, over every shadow ray the frame casts, the share whose flip would change the
pixel.
Usage: python tools/measure_shadow_masking.py [W] [H]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as e  # noqa: E402
import occlfam  # noqa: E402

pkg = e.load_package()
orc = e.load_oracle()


def masking(sd, cam, W, H, max_level, lights):
    o = orc.OracleScene(sd)
    rays = orc.generate_rays(cam, W, H)
    weight = np.ones((len(rays), 3), np.float32)  # product of the parents' ks
    mats = np.asarray(sd.materials, np.float32).reshape(-1, 8)
    total = visible = shadowed = 0
    for level in range(max_level):
        if len(rays) == 0:
            break
        ref = o.intersect(rays)
        m = ref["hit"] == 1
        rays, weight, ref = rays[m], weight[m], ref[m]
        d = rays[:, 3:6]
        pts = (rays[:, 0:3] + d * ref["t"][:, None]).astype(np.float32)
        nrm = ref["normal"].astype(np.float32)
        mid = ref["material"]
        kd = np.where(mid[:, None] >= 0, mats[np.maximum(mid, 0), 0:3], 0).astype(np.float32)
        ks = np.where(mid[:, None] >= 0, mats[np.maximum(mid, 0), 3:6], 0).astype(np.float32)
        shin = np.where(mid >= 0, mats[np.maximum(mid, 0), 6], 1).astype(np.float32)
        dn = (nrm * d).sum(1, dtype=np.float32)
        refl = occlfam.normalize(d - nrm * (dn * np.float32(2.0))[:, None])
        for lp in lights:
            to = occlfam.normalize(lp[None, 0:3] - pts)
            dc = (to * nrm).sum(1, dtype=np.float32)
            dif = np.where(dc[:, None] > 0, lp[None, 3:6] * kd * dc[:, None], 0)
            sc = (refl * to).sum(1, dtype=np.float32)
            with np.errstate(invalid="ignore", over="ignore"):
                spec = np.where(sc[:, None] > 0, lp[None, 3:6] * ks * np.power(np.maximum(sc, 0), shin)[:, None], 0)
                term = ((dif + spec) * weight).astype(np.float32)
            sr, sdist = occlfam.spawn(pts, lp[None, 0:3])
            v, _ = occlfam.reference(o, sr, sdist)
            total += len(pts)
            visible += int((term != 0).any(1).sum())
            shadowed += int(v.sum())
        if level + 1 >= max_level:
            break
        keep = ks[:, 2] > np.float32(0.01)
        nr = np.empty((int(keep.sum()), 7), np.float32)
        nr[:, 3:6] = refl[keep]
        nr[:, 0:3] = pts[keep] + np.float32(0.001) * refl[keep]
        nr[:, 6] = occlfam.length(d[keep])  # main.cpp:254
        rays, weight = nr, (weight[keep] * ks[keep]).astype(np.float32)
    return total, visible, shadowed


def main():
    W = int(sys.argv[1]) if len(sys.argv) > 1 else 160
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 120
    cornell = pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz"))
    dragon = pkg.scenes.make_dragon(40_000)
    dl = np.asarray(dragon.point_lights, np.float32).reshape(-1, 6)
    if len(dl) == 0:
        dl = np.float32([[0.0, 2.0, -2.0, 1, 1, 1]])
    for name, sd, depth, lights in (("cornell", cornell, 4, np.asarray(cornell.point_lights, np.float32).reshape(-1, 6)),
                                    ("dragon 40K", dragon, 2, dl)):
        total, visible, shadowed = masking(sd, pkg.scenes.default_camera(W, H), W, H, depth, lights)
        print(f"{name} {W}x{H} depth {depth}: {total} shadow verdicts, {visible} ({100.0 * visible / max(total, 1):.1f} %) would change the "
              f"pixel if flipped, {shadowed} in shadow")


if __name__ == "__main__":
    main()
