"""Scenes of the bake tests (tests/test_bake_model.py, tests/test_bake.py): host.SceneBuilder scenes with UV-mapped meshes."""
import numpy as np

QUAD_UV = [(0, 0), (1, 0), (1, 1), (0, 1)]
QUAD_IDX = [0, 1, 2, 0, 2, 3]


def _builder(pkg):
    b = pkg.host.SceneBuilder()
    b.film.update(xres=8, yres=8); b.spp = 1
    b.look_at((0, 0, 5), (0, 0, 0), (0, 1, 0)); b.camera(fov=30.0)
    b.world_begin()
    return b


def floor(b, half=2.0, z=0.0, uv=QUAD_UV, N=None):
    return b.trianglemesh([(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)], QUAD_IDX, UV=uv, N=N)


def open_floor(pkg):
    """A UV-mapped floor and nothing else: shape 0."""
    b = _builder(pkg)
    floor(b)
    return b.world_end()[0]


def uv_mesh(pkg, uvs, indices, second=None):
    """One flat mesh (z = 0, P = (u, v, 0) scaled) with the given vertex UVs: shape 0. `second` = (uvs, indices): another mesh, shape 1."""
    b = _builder(pkg)
    for part in ([(uvs, indices)] + ([second] if second is not None else [])):
        uv = np.asarray(part[0], np.float32).reshape(-1, 2)
        P = np.concatenate([uv * 3.0 - 1.0, np.zeros((len(uv), 1), np.float32)], axis=1)
        b.trianglemesh(P, part[1], UV=uv)
    return b.world_end()[0]


def small_triangles(n_side=13):
    """(uvs, indices) of a grid of 2 * n_side^2 triangles (n_side = 13: 338 >= 300) over [0.03, 0.97]^2, jittered so that no edge follows the texel grid."""
    rng = np.random.RandomState(7)
    g = np.linspace(0.03, 0.97, n_side + 1)
    uv = np.stack(np.meshgrid(g, g, indexing="xy"), axis=-1).reshape(-1, 2) + rng.uniform(-0.01, 0.01, ((n_side + 1) ** 2, 2))
    idx = []
    for j in range(n_side):
        for i in range(n_side):
            a = j * (n_side + 1) + i
            idx += [a, a + 1, a + n_side + 2, a, a + n_side + 2, a + n_side + 1]
    return uv.astype(np.float32), idx


def shaded(pkg, normals=False, reverse=False, mirror=False):
    """A tilted, curved-looking patch of 2 x 2 quads with UVs over [0.1, 0.9]^2: with per-vertex N or without, under ReverseOrientation, under a mirroring transform."""
    b = _builder(pkg)
    if mirror:
        b.scale(-1.0, 1.0, 1.0)
    b.rotate(25.0, 1, 0.3, 0)
    if reverse:
        b.toggle_reverse_orientation()
    g = np.linspace(0.0, 1.0, 3)
    uv = np.stack(np.meshgrid(g, g, indexing="xy"), axis=-1).reshape(-1, 2)
    P = np.stack([uv[:, 0] * 2 - 1, uv[:, 1] * 2 - 1, 0.3 * np.sin(2.0 * uv[:, 0]) + 0.2 * uv[:, 1] ** 2], axis=1)
    N = None
    if normals:
        N = np.stack([-0.6 * np.cos(2.0 * uv[:, 0]), -0.4 * uv[:, 1], np.ones(len(uv))], axis=1)
    idx = []
    for j in range(2):
        for i in range(2):
            a = j * 3 + i
            idx += [a, a + 1, a + 4, a, a + 4, a + 3]
    b.trianglemesh(P, idx, UV=uv * 0.8 + 0.1, N=N)
    return b.world_end()[0]


def occluded_floor(pkg):
    """A UV-mapped floor (shape 0) under a box, a sphere (high above: out of reach of a short max_distance), an instanced quad and a fully alpha-masked triangle."""
    b = _builder(pkg)
    floor(b)
    lo, hi = np.array([-1.2, -0.9, 0.3]), np.array([-0.2, 0.1, 0.8])
    c = np.array([[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])])
    b.trianglemesh(c, [0, 1, 3, 0, 3, 2, 4, 7, 5, 4, 6, 7, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3])
    b.attribute_begin(); b.translate(1.0, 1.0, 3.0); b.sphere(radius=0.6); b.attribute_end()
    b.object_begin("leaf")
    b.trianglemesh([(-0.4, -0.4, 0), (0.4, -0.4, 0), (0.4, 0.4, 0), (-0.4, 0.4, 0)], QUAD_IDX)
    b.trianglemesh([(-0.4, 0, -0.3), (0.4, 0, -0.3), (0.4, 0, 0.3)], [0, 1, 2])
    b.object_end()
    b.attribute_begin(); b.translate(1.0, -1.0, 0.5); b.rotate(20.0, 1, 0, 0); b.object_instance("leaf"); b.attribute_end()
    b.attribute_begin(); b.translate(-1.0, 1.2, 0.6); b.object_instance("leaf"); b.attribute_end()
    b.trianglemesh([(-2, 0.2, 0.4), (2, 0.2, 0.4), (0, 2, 0.4)], [0, 1, 2], alpha=0.0)
    return b.world_end()[0]
