"""Random triangle soups for the octree builders — TEST INFRASTRUCTURE (a helper, no tests in it)."""
import os

import numpy as np

SOUP_SEEDS = range(16)


def write_soup(directory, seed):
    """Random meshes the shipped ones do not resemble: triangle soups of 1 .. 3000 triangles — tiny, huge and sliver triangles,
    zero-area ones, vertices shared by most of the mesh (the valence stop rule), all triangles in one corner of the box, flat
    meshes (a root box of zero thickness).  Writes <directory>/Models/soup<seed>.obj and returns its path."""
    rng = np.random.default_rng(4242 + seed)
    n_v = int(rng.choice([3, 8, 50, 400, 1500]))
    n_t = int(rng.choice([1, 5, 60, 700, 3000]))
    scale = rng.choice([1e-3, 1.0, 1.0, 50.0])
    verts = rng.normal(size=(n_v, 3)) * scale
    mode = seed % 4
    if mode == 1:
        verts[:, 2] = 0.25                                   # a flat mesh
    if mode == 2:
        verts[: n_v // 2] = verts[0] + rng.normal(size=(n_v // 2, 3)) * 1e-4 * scale      # half of the vertices in one spot
    tris = rng.integers(0, n_v, size=(n_t, 3))
    if mode == 3:
        tris[:, 0] = 0                                        # one vertex in every triangle
    degenerate = rng.random(n_t) < 0.05
    tris[degenerate, 2] = tris[degenerate, 1]               # a few zero-area triangles
    os.makedirs(os.path.join(str(directory), "Models"), exist_ok=True)
    path = os.path.join(str(directory), "Models", f"soup{seed}.obj")
    with open(path, "w") as f:
        for v in verts:
            f.write(f"v {v[0]:.6f} {v[1]:.6f} {v[2]:.6f}\n")
        for t in tris:
            f.write(f"f {t[0] + 1} {t[1] + 1} {t[2] + 1}\n")
    return path
