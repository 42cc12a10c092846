"""Scenes of the transfer-bake tests (tests/test_bake_transfer_model.py, tests/test_bake_transfer.py): UV-mapped targets (the low-polygon side) and sources without
UVs (the detailed side), host.SceneBuilder scenes."""
import numpy as np
import bake_scenes as S

QUAD_P = [(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)]


def quad_target(pkg, smooth=False):
    """A two-triangle quad over [-1, 1]^2 at z = 0, normal +z, UVs over [0.05, 0.95]^2: shape 0. `smooth`: per-vertex N leaning outward, so the cage fans out."""
    b = S._builder(pkg)
    uv = [(0.05, 0.05), (0.95, 0.05), (0.95, 0.95), (0.05, 0.95)]
    N = [(-0.25, -0.2, 1), (0.3, -0.15, 1), (0.2, 0.25, 1), (-0.3, 0.2, 1)] if smooth else None
    b.trianglemesh(QUAD_P, S.QUAD_IDX, UV=uv, N=N)
    return b.world_end()[0]


def mirrored_target(pkg):
    """Two quads side by side (x < 0: primitives 0 and 1, x > 0: 2 and 3) in one mesh, shape 0: the left island's v runs with y, the right island's against it (a
    mirrored island: dpdv points the other way, the UV frame is left-handed)."""
    b = S._builder(pkg)
    P = [(-1, -1, 0), (0, -1, 0), (0, 1, 0), (-1, 1, 0), (0, -1, 0), (1, -1, 0), (1, 1, 0), (0, 1, 0)]
    uv = [(0.04, 0.06), (0.46, 0.06), (0.46, 0.94), (0.04, 0.94), (0.54, 0.94), (0.96, 0.94), (0.96, 0.06), (0.54, 0.06)]
    b.trianglemesh(P, S.QUAD_IDX + [i + 4 for i in S.QUAD_IDX], UV=uv)
    return b.world_end()[0]


def degenerate_uv_target(pkg):
    """One triangle, shape 0, that is a sliver in UV space: its determinant there, 2^-25 * 0.2 = 6e-9, is not zero -- it owns the texel whose centre is its vertex
    (0.5, 0.5): the middle of a 5 x 5 atlas -- but below the 1e-8 under which Triangle::intersect takes its partials from coordinate_system of the geometric normal."""
    b = S._builder(pkg)
    a = np.float32(0.5) - np.float32(2.0 ** -25)
    b.trianglemesh([(-1, -1, 0), (1, 0, 0), (-1, 1, 0)], [0, 1, 2], UV=[(a, 0.4), (0.5, 0.5), (a, 0.6)])
    return b.world_end()[0]


def plane_source(pkg, z=0.25, tilt=0.0, half=3.0):
    """A quad without UVs at height z over the origin, facing down the projection rays' way (normal +z), rotated by `tilt` degrees about the x axis."""
    b = S._builder(pkg)
    b.translate(0, 0, z)
    if tilt:
        b.rotate(tilt, 1, 0, 0)
    b.trianglemesh([(-half, -half, 0), (half, -half, 0), (half, half, 0), (-half, half, 0)], S.QUAD_IDX)
    return b.world_end()[0]


def bump(x, y):
    return 0.1 * np.sin(4.0 * x + 0.5) * np.cos(3.0 * y)


def _bump_grid(b, normals, n=12, half=0.85):
    g = np.linspace(-half, half, n + 1)
    xy = np.stack(np.meshgrid(g, g, indexing="xy"), axis=-1).reshape(-1, 2)
    P = np.concatenate([xy, bump(xy[:, 0], xy[:, 1])[:, None]], axis=1)
    N = None
    if normals:   # the surface normal of z = bump(x, y): (-dz/dx, -dz/dy, 1)
        N = np.stack([-0.4 * np.cos(4.0 * xy[:, 0] + 0.5) * np.cos(3.0 * xy[:, 1]), 0.3 * np.sin(4.0 * xy[:, 0] + 0.5) * np.sin(3.0 * xy[:, 1]), np.ones(len(xy))], axis=1)
    idx = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            idx += [a, a + 1, a + n + 2, a, a + n + 2, a + n + 1]
    b.trianglemesh(P, idx, N=N)


def bump_source(pkg, normals=False):
    """A 12 x 12 grid (288 triangles, no UVs) over [-0.85, 0.85]^2 with a sine bump of amplitude 0.1: narrower than the targets, so some owned texels miss."""
    b = S._builder(pkg)
    _bump_grid(b, normals)
    return b.world_end()[0]


def mixed_source(pkg):
    """The bump grid with a sphere poking through it and an instanced quad hovering over a corner: hits that are no detail hits."""
    b = S._builder(pkg)
    _bump_grid(b, True)
    b.attribute_begin(); b.translate(0.3, 0.25, 0.0); b.sphere(radius=0.25); b.attribute_end()
    b.object_begin("card")
    b.trianglemesh([(-0.2, -0.2, 0), (0.2, -0.2, 0), (0.2, 0.2, 0), (-0.2, 0.2, 0)], S.QUAD_IDX)
    b.object_end()
    b.attribute_begin(); b.translate(-0.5, -0.45, 0.2); b.rotate(10.0, 0, 1, 0); b.object_instance("card"); b.attribute_end()
    return b.world_end()[0]
