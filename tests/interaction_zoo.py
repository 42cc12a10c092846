"""Test infrastructure of tests/test_interaction_zoo.py (CPU) and tests/test_interaction_probe.py (GPU): three small scenes in which every primitive sits in a grid
cell of its own, rays aimed at the edges of those primitives, and a float64 model of the scenes' geometry that trusts neither the oracle nor the device.

Scenes (SceneBuilder, 8x8 film): tri_zoo (fifteen two-triangle quads, one per branch of Triangle::intersect's interaction), quadric_zoo (five spheres, six disks),
instanced_zoo (a multi-primitive object, a one-triangle object and a one-sphere object, each under the identity, Scale 2 2 2, a rotation with a non-uniform scale and a mirror).
Queries are built in float64 and cast to float32: `random` (4096 per scene, aimed from all sides at points inside each primitive's bounds) and `structured`
(vertices, edges, poles, seams, rims, tangents, clipped roots, parallel rays, t_max at the hit: the lists in structured_triangle / _sphere / _disk).

The float64 model (truth): every float32 ray is intersected with every primitive in float64 -- a quadric in its object space through the float64 inverse of its
float32 object-to-world matrix (composed with the instance's), a triangle in world space. A ray is CLEAR when every boundary of every primitive it could meet
(edge, tangent, pole, centre, rim, phi seam of a partial shape, phi_max, z_min, z_max, t = 0, t = t_max) is missed or cleared by MARGIN = 1e-3 of that primitive's
size, and when it meets triangles and disks at a cosine of at least MIN_COS: a distance of 1e-3 of the size from an edge shrinks to 1e-3 * size * cos in the
plane perpendicular to the ray, where the watertight test evaluates its edge functions with an absolute rounding error of a few 2^-23 of coordinates up to 20
(about 1e-5); at cos = 1e-2 the margin (2e-5 for these quads) is still above it, at the structured cosines 1e-3 and 1e-6 it is not, so those rays are compared
bit for bit but not against float64. Two quirks of the reference are kept by oracle and device; the rays they change are named by their geometry and left out of
the float64 hit / miss check:
  * Disk::intersect divides by the WORLD ray's d.z (disk.rs:66, ref_sphere.cpp disk_hit): every ray at a disk whose object-space d.z differs from the d.z of the
    ray the shape is handed (`quirk_closest`);
  * Sphere::intersect_p, and Sphere::intersect for its second root, take `phi += 2 * phi` for a negative phi (sphere.rs:108-110 / 243-261, ref_sphere.cpp
    sphere_hit): phi stays negative and is never clipped by phi_max -- every ray at a sphere with phi_max < 2 pi whose examined root lies at y < 0
    (`quirk_any`: any examined root; `quirk_closest`: the second root)."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
TOP_INSTANCE = 0x80000000
MARGIN = 1e-3
MIN_COS = 1e-2
EPS20 = 2.0 ** -20
FAR_ORIGIN = 30.0
N_RANDOM = 4096


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------------
def _base(pkg):
    b = pkg.host.SceneBuilder()
    b.film.update(xres=8, yres=8); b.spp = 1
    b.look_at((8.0, 8.0, 40.0), (8.0, 8.0, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=40.0)
    b.world_begin()
    b.light_source("infinite", L=(1.0, 1.0, 1.0))
    return b


def _unit_rows(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


QUAD_P = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F)   # exact coordinates in cells at integer offsets: a ray along -z at an edge midpoint has e == 0 and b0 == b1 exactly
QUAD_I = np.array([0, 1, 2, 0, 2, 3], np.uint32)
N_UP = _unit_rows([[0.1, 0.0, 1.0], [-0.1, 0.1, 1.0], [0.0, -0.1, 1.0], [0.05, 0.05, 1.0]])
N_ZERO0 = N_UP.copy(); N_ZERO0[0] = 0.0
_V = _unit_rows([[0.3, 0.1, 0.9]])[0]
N_CANCEL = np.array([_V, -_V, N_UP[2], N_UP[3]], F)          # n0 == -n1: the interpolated normal is zero at b0 == b1, b2 == 0 (the midpoint of edge 0-1 of the first triangle)
UV_UNIT = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F)
UV_TINY = (UV_UNIT * F(5e-5)).astype(F)                        # determinant 2.5e-9 < 1e-8
Z4 = np.array([[0, 0, 1]] * 4, F)
TRI_KINDS = [
    ("plain", dict()),
    ("n_agrees", dict(N=N_UP)),
    ("n_opposes", dict(N=-N_UP)),
    ("n_one_zero", dict(N=N_ZERO0)),
    ("n_cancels", dict(N=N_CANCEL)),
    ("s_given", dict(S=np.array([[1, 0.2, 0], [1, -0.1, 0.1], [0.9, 0.1, -0.1], [1, 0, 0]], F))),
    ("s_parallel_n", dict(N=Z4, S=Z4)),                        # cross(ss, ns) == 0: coordinate_system
    ("uv_equal", dict(UV=np.array([[0.5, 0.5]] * 4, F))),
    ("uv_collinear", dict(UV=np.array([[0, 0], [0.5, 0.5], [1, 1], [0.25, 0.25]], F))),
    ("uv_tiny_n_varied", dict(UV=UV_TINY, N=N_UP)),           # |det| < 1e-8, cross(n2 - n0, n1 - n0) != 0
    ("uv_tiny_n_equal", dict(UV=UV_TINY, N=Z4)),              # |det| < 1e-8, cross == 0: dndu / dndv stay zero
    ("reversed", dict(UV=UV_UNIT, N=N_UP, reverse=True)),
    ("mirrored", dict(UV=UV_UNIT, N=N_UP, mirror=True)),       # Scale -1 1 1 swaps handedness
    ("reversed_mirrored", dict(UV=UV_UNIT, N=N_UP, reverse=True, mirror=True)),
    ("alpha_mask", dict(UV=UV_UNIT, alpha="holes")),
]
SPACING = 4.0


def _cell(k, columns=4, spacing=SPACING):
    return spacing * (k % columns), spacing * (k // columns)


def tri_zoo(pkg):
    b = _base(pkg)
    b.texture("holes", "float", "checkerboard", uscale=3.0, vscale=3.0, tex1=1.0, tex2=0.0)
    names = []
    for k, (name, kw) in enumerate(TRI_KINDS):
        kw = dict(kw)
        b.attribute_begin()
        b.material("matte", Kd=(0.1 + 0.05 * k, 0.5, 0.4))
        b.translate(*_cell(k), 0.0)
        if kw.pop("mirror", False): b.scale(-1.0, 1.0, 1.0)
        if kw.pop("reverse", False): b.toggle_reverse_orientation()
        b.trianglemesh(QUAD_P, QUAD_I, **kw)
        b.attribute_end()
        names += [name + "/0", name + "/1"]
    return b, names


def quadric_zoo(pkg):
    b = _base(pkg)
    shapes = [
        ("sphere_full", lambda: None, lambda: b.sphere(radius=1.0)),
        ("sphere_partial", lambda: None, lambda: b.sphere(radius=1.0, zmin=-0.6, zmax=0.7, phimax=200.0)),
        ("sphere_rotated_scaled", lambda: (b.rotate(30.0, 1.0, 1.0, 0.5), b.scale(1.0, 0.7, 1.2)), lambda: b.sphere(radius=1.0, zmin=-0.8, zmax=0.9, phimax=300.0)),
        ("sphere_mirrored", lambda: b.scale(-1.0, 1.0, 1.0), lambda: b.sphere(radius=0.9, zmax=0.7, phimax=250.0)),
        ("sphere_reversed", lambda: b.toggle_reverse_orientation(), lambda: b.sphere(radius=1.0)),
        ("disk_full", lambda: None, lambda: b.disk(radius=1.0)),
        ("disk_annulus", lambda: None, lambda: b.disk(radius=1.0, innerradius=0.4)),
        ("disk_partial", lambda: None, lambda: b.disk(radius=1.0, phimax=200.0)),
        ("disk_height", lambda: None, lambda: b.disk(height=0.3, radius=0.9)),
        ("disk_rotated", lambda: b.rotate(40.0, 1.0, 0.0, 0.0), lambda: b.disk(radius=1.0, innerradius=0.2)),   # the world ray's d.z and the object ray's differ
        ("disk_mirrored", lambda: b.scale(-1.0, 1.0, 1.0), lambda: b.disk(radius=1.0, phimax=250.0)),
    ]
    names = []
    for k, (name, xf, shape) in enumerate(shapes):
        b.attribute_begin()
        b.material("matte", Kd=(0.1 + 0.05 * k, 0.4, 0.5))
        b.translate(*_cell(k), 0.0)
        xf(); shape()
        b.attribute_end()
        names.append(name)
    return b, names


INSTANCE_XF = [
    ("identity", None),
    ("scale2", lambda b: b.scale(2.0, 2.0, 2.0)),
    ("rotated_scaled", lambda b: (b.rotate(35.0, 0.3, 1.0, 0.2), b.scale(1.3, 0.8, 1.1))),
    ("mirrored", lambda b: b.scale(-1.0, 1.0, 1.0)),
]


def instanced_zoo(pkg):
    """Objects are defined around (0, 0, 0), (6, 0, 0) and (12, 0, 0), where their identity instances stand; row r > 0 holds the instances under transform r."""
    b = _base(pkg)
    centres = {"multi": (0.0, 0.0, 0.0), "tri1": (6.0, 0.0, 0.0), "sph1": (12.0, 0.0, 0.0)}
    b.object_begin("multi")
    b.material("matte", Kd=(0.3, 0.5, 0.2))
    b.attribute_begin(); b.translate(-0.6, 0.0, 0.0); b.scale(0.5, 0.5, 0.5); b.trianglemesh(QUAD_P, QUAD_I, N=N_UP, UV=UV_UNIT); b.attribute_end()
    b.material("matte", Kd=(0.5, 0.3, 0.2))
    b.attribute_begin(); b.translate(0.6, 0.0, 0.0); b.sphere(radius=0.5, zmin=-0.3, zmax=0.35, phimax=200.0); b.attribute_end()
    b.object_end()
    b.object_begin("tri1")
    b.material("matte", Kd=(0.2, 0.3, 0.6))
    b.attribute_begin(); b.translate(6.0, 0.0, 0.0); b.trianglemesh(QUAD_P[:3], QUAD_I[:3], N=N_UP[:3]); b.attribute_end()
    b.object_end()
    b.object_begin("sph1")
    b.material("matte", Kd=(0.6, 0.3, 0.6))
    b.attribute_begin(); b.translate(12.0, 0.0, 0.0); b.sphere(radius=0.8); b.attribute_end()
    b.object_end()
    names = []
    for r, (xname, xf) in enumerate(INSTANCE_XF):
        for oname, c in centres.items():
            b.attribute_begin()
            if xf is not None:
                b.translate(c[0], 6.0 * r, 0.0); xf(b); b.translate(-c[0], -c[1], -c[2])
            b.object_instance(oname)
            b.attribute_end()
            names.append(f"{oname}@{xname}")
    return b, names


SCENES = {"tri_zoo": tri_zoo, "quadric_zoo": quadric_zoo, "instanced_zoo": instanced_zoo}


# ---- targets: every (primitive, instance) pair of a scene, with what the float64 model needs ------------------------------------------------------------
def _m4(a):
    return np.array(list(a), np.float64).reshape(4, 4)


def targets(pkg, sd):
    A = pkg._abi
    out = []

    def add(prim, inst, M):
        ref = int(sd.prim_shape[prim]); k = ref & 0x3FFFFFFF
        t = dict(prim=prim, inst=inst, outer=M, outer_inv=np.linalg.inv(M))
        if (ref >> 30) == A.PT_SHAPE_SPHERE:
            S = sd.spheres[k]
            t.update(kind="disk" if S.kind == A.PT_QUADRIC_DISK else "sphere", M=M @ _m4(S.object_to_world), r=float(S.radius), ri=float(S.inner_radius),
                     zmin=float(S.z_min), zmax=float(S.z_max), phimax=float(S.phi_max), rigid=False)
            t["Minv"] = np.linalg.inv(t["M"]); t["size"] = t["r"]
            L = t["M"][:3, :3]
            t["rigid"] = bool(np.allclose(L.T @ L, np.eye(3), atol=1e-6) and np.linalg.det(L) > 0)
            t["partial_phi"] = t["phimax"] < 2.0 * np.pi - 1e-6
        else:
            v = sd.P[sd.idx[k]].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
            t.update(kind="tri", v=v, size=float(max(np.linalg.norm(v[1] - v[0]), np.linalg.norm(v[2] - v[1]), np.linalg.norm(v[0] - v[2]))),
                     alpha=bool(sd.tri_alpha is not None and sd.tri_alpha[k] >= 0))
        out.append(t)

    if sd.top_refs is None:
        for prim in range(len(sd.prim_shape)): add(prim, NONE, np.eye(4))
    else:
        for ref in sd.top_refs:
            ref = int(ref)
            if ref & TOP_INSTANCE:
                I = sd.instances[ref & ~TOP_INSTANCE]; O = sd.objects[I.object]
                for prim in range(O.first_prim, O.first_prim + O.n_prims): add(prim, ref & ~TOP_INSTANCE, _m4(I.instance_to_world))
            else:
                add(ref, NONE, np.eye(4))
    return out


# ---- queries ----------------------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _sphere_dirs(rng, n):
    z = 1.0 - 2.0 * rng.random(n); ph = 2.0 * np.pi * rng.random(n); r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([r * np.cos(ph), r * np.sin(ph), z], axis=1)


def _to_world(M, p, d):
    return M[:3, :3] @ p + M[:3, 3], M[:3, :3] @ d


def _aim_points(rng, t, n):
    """World points inside the primitive's bounds."""
    if t["kind"] == "tri":
        u = rng.random((n, 2)); s = np.sqrt(u[:, 0])
        bb = np.stack([1.0 - s, s * (1.0 - u[:, 1]), s * u[:, 1]], axis=1)   # uniform on the triangle
        return bb @ t["v"]
    r = t["r"]
    p = np.stack([r * (2.0 * rng.random(n) - 1.0), r * (2.0 * rng.random(n) - 1.0), t["zmin"] + (t["zmax"] - t["zmin"]) * rng.random(n)], axis=1)
    return p @ t["M"][:3, :3].T + t["M"][:3, 3]


def random_queries(tg, seed):
    """N_RANDOM rays, an equal share per primitive: a uniform direction through a point inside the primitive's bounds, from 0.5 to 4 sizes away (from all sides)."""
    rng = np.random.default_rng(seed)
    per = [N_RANDOM // len(tg) + (1 if k < N_RANDOM % len(tg) else 0) for k in range(len(tg))]
    o, d, which = [], [], []
    for k, (t, n) in enumerate(zip(tg, per)):
        p = _aim_points(rng, t, n); w = _sphere_dirs(rng, n)
        size = t["size"] * (np.abs(np.linalg.det(t["M"][:3, :3])) ** (1.0 / 3.0) if t["kind"] != "tri" else 1.0)
        dist = size * (0.5 + 3.5 * rng.random((n, 1)))
        scale = np.where(rng.random((n, 1)) < 0.5, 1.0, 3.0)   # d normalised, or of length 3
        o.append(p - w * dist); d.append(w * scale); which += [k] * n
    o = np.concatenate(o).astype(F); d = np.concatenate(d).astype(F)
    return dict(o=o, d=d, tmax=np.full(len(o), np.inf, F), target=np.array(which), tag=["random"] * len(o))


def structured_triangle(t, full=True):
    """Every vertex, every edge midpoint (the zero-normal point of n_cancels is the midpoint of edge 0-1) and the centroid; from the front and from the back; at cosines
    1, 1e-3 and 1e-6 to the plane; d normalised and of length 3 (`full` False: the cosines 1 and 1e-3 at length 1 only, for the triangles inside instances)."""
    v = t["v"]; n = _unit(np.cross(v[1] - v[0], v[2] - v[0]))
    tang = _unit((v[1] - v[0]) * 0.8 + (v[2] - v[0]) * 0.3)
    pts = [("vertex", v[0]), ("vertex", v[1]), ("vertex", v[2]), ("edge", 0.5 * (v[0] + v[1])), ("edge", 0.5 * (v[1] + v[2])), ("edge", 0.5 * (v[2] + v[0])),
           ("centroid", (v[0] + v[1] + v[2]) / 3.0)]
    out = []
    for what, p in pts:
        for side in (1.0, -1.0):
            for c in ((1.0, 1e-3, 1e-6) if full else (1.0, 1e-3)):
                w = -(side * c * n + np.sqrt(1.0 - c * c) * tang)
                for length in ((1.0, 3.0) if full else (1.0,)):
                    out.append((p - w * 2.0, w * length, np.inf, f"{what} side {side:+.0f} cos {c:g} |d| {length:g}"))
    return out


def _on_sphere(r, theta, phi):
    return r * np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])


def structured_sphere(t, rng):
    """Object-space rays (origin, direction, t_max, tag) of one sphere; see the tags."""
    r, zmin, zmax, phimax = t["r"], t["zmin"], t["zmax"], t["phimax"]
    out = []
    both = lambda p, tag: out.extend([(3.0 * p, -p, np.inf, tag + " from outside"), (np.zeros(3), p, np.inf, tag + " from the centre")])
    for s in (1.0, -1.0):   # along +-z of the object through both poles (zradius == 0: the ph.x = 1e-5 * radius nudge)
        out.append((np.array([0.0, 0.0, 3.0 * r * s]), np.array([0.0, 0.0, -s]), np.inf, "pole, through both"))
        out.append((np.zeros(3), np.array([0.0, 0.0, s]), np.inf, "pole, from the centre"))
    theta_mid = np.arccos(np.clip(0.5 * (zmin + zmax) / r + 0.1, -1.0, 1.0))
    for ph in (1e-6, -1e-6, 2.0 ** -30, -2.0 ** -30): both(_on_sphere(r, theta_mid, ph), f"phi seam {ph:+.1e}")
    for s in (1.0, -1.0): both(_on_sphere(r, theta_mid, phimax * (1.0 + s * EPS20)), f"phi_max * (1 {s:+.0f} 2^-20)")
    for name, z in (("z_min", zmin), ("z_max", zmax)):
        for s in (1.0, -1.0):
            both(_on_sphere(r, np.arccos(np.clip(z * (1.0 + s * EPS20) / r, -1.0, 1.0)), 1.0), f"{name} * (1 {s:+.0f} 2^-20)")
    # first root clipped away (for the partial spheres) and the second kept; both clipped; the second root at y < 0 (the `phi += 2 * phi` form of Sphere::intersect)
    p = _on_sphere(r, 1.3, np.radians(280.0)); out.append((3.0 * p, -p, np.inf, "first root in the phi gap, second kept"))
    a, b = _on_sphere(r, 1.4, np.radians(230.0)), _on_sphere(r, 1.4, np.radians(330.0)); out.append((a - (b - a), b - a, np.inf, "chord through the phi gap: both roots clipped"))
    out.append((np.array([0.15 * r, 0.1 * r, 3.0 * r]), np.array([0.0, 0.0, -1.0]), np.inf, "along z beside the axis: both caps"))
    a, b = np.array([0.05 * r, 0.3 * r, 2.0 * r]), _on_sphere(r, 1.6, np.radians(300.0)); out.append((a, b - a, np.inf, "first root on the cap, second at y < 0"))
    for k in (1, 8, 64):   # tangents at distance r * (1 +- k * 2^-23); the tangent point lies at theta = 60 degrees, phi = 90 degrees
        for s in (1.0, -1.0):
            dist = r * (1.0 + s * k * 2.0 ** -23)
            out.append((np.array([-3.0 * r, dist * np.cos(0.5), dist * np.sin(0.5)]), np.array([1.0, 0.0, 0.0]), np.inf, f"tangent at r * (1 {s * k:+.0f} * 2^-23)"))
    generic = [_on_sphere(r, th, ph) for th, ph in ((0.9, 0.7), (1.2, 2.0), (1.5, 3.0), (1.7, 1.3), (2.0, 0.4), (1.1, 4.5), (1.4, 5.5), (0.6, 2.6))]
    for j, p in enumerate(generic):
        out.append((np.zeros(3), p, np.inf, "origin at the centre"))
        out.append((p * 10.0, -p * 3.0, np.inf, "origin 10 r away"))
        if j < 4: out.append((p * 1e4, -p * 1e4, np.inf, "origin 1e4 r away"))
        if j < 3: out.append((p, -p, np.inf, "origin on the surface, inwards")); out.append((p, p + np.array([0.1, 0.0, 0.0]), np.inf, "origin on the surface, outwards"))
        for s in ((1.0, -1.0) if j < 2 else ()):   # (from 3 p along -p the first root lies at t = 2 / 3)
            out.append((3.0 * p, -3.0 * p, (2.0 / 3.0) * (1.0 + s * EPS20), f"t_max = t * (1 {s:+.0f} 2^-20)"))
            out.append((np.zeros(3), p, 1.0 * (1.0 + s * EPS20), f"t_max = t * (1 {s:+.0f} 2^-20), from the centre"))
    for _ in range(56):   # lines through interior points, from outside
        q = r * 0.55 * (2.0 * rng.random(3) - 1.0); w = _sphere_dirs(rng, 1)[0]
        out.append((q - w * 3.0 * r, w * (1.0 if rng.random() < 0.5 else 3.0), np.inf, "through an interior point"))
    return out


def structured_disk(t, rng):
    """Object-space rays of one disk (the rays with WORLD d.z == 0 are added by structured_queries, which knows the world)."""
    R, ri, h, phimax = t["r"], t["ri"], t["zmin"], t["phimax"]
    at = lambda rho, phi: np.array([rho * np.cos(phi), rho * np.sin(phi), h])
    pts = [("centre", at(0.0, 0.0))]
    for s in (1.0, -1.0):
        pts.append((f"rim * (1 {s:+.0f} 2^-20)", at(R * (1.0 + s * EPS20), 1.0)))
        if ri > 0.0: pts.append((f"inner rim * (1 {s:+.0f} 2^-20)", at(ri * (1.0 + s * EPS20), 1.0)))
        pts.append((f"phi seam {s:+.0f}e-6", at(0.7 * R, s * 1e-6)))
        pts.append((f"phi_max * (1 {s:+.0f} 2^-20)", at(0.7 * R, phimax * (1.0 + s * EPS20))))
    out = []
    for tag, p in pts:
        for s in (1.0, -1.0):   # from above and from below, straight and slanted
            out.append((p + np.array([0.0, 0.0, 2.0 * s]), np.array([0.0, 0.0, -s]), np.inf, tag + (" from above" if s > 0 else " from below")))
            w = _unit((0.3, -0.2, -s)); out.append((p - 2.0 * w, w * 3.0, np.inf, tag + (" from above" if s > 0 else " from below") + ", slanted"))
    for z in (h, h + 0.1 * R):   # object d.z == 0: in the disk's plane and beside it
        out.append((np.array([-2.0 * R, 0.1 * R, z]), np.array([1.0, 0.2, 0.0]), np.inf, "object d.z == 0"))
    for _ in range(48):
        rho = R * np.sqrt(rng.random()); phi = 2.0 * np.pi * rng.random(); w = _sphere_dirs(rng, 1)[0]
        if abs(w[2]) < 0.2: w[2] = 0.5
        p = at(rho, phi)
        out.append((p - 2.0 * w, w, np.inf, "through a point of the plane"))
    for s in (1.0, -1.0):   # t_max at the hit: from 2 above the point (0.5 R, 1 rad) straight down, t = 2
        p = at(0.5 * R, 1.0)
        out.append((p + np.array([0.0, 0.0, 2.0]), np.array([0.0, 0.0, -1.0]), 2.0 * (1.0 + s * EPS20), f"t_max = t * (1 {s:+.0f} 2^-20)"))
    return out


def structured_queries(tg, seed):
    rng = np.random.default_rng(seed)
    o, d, tmax, which, tags = [], [], [], [], []

    def put(k, ow, dw, tm, tag):
        o.append(ow); d.append(dw); tmax.append(tm); which.append(k); tags.append(tag)

    for k, t in enumerate(tg):
        if t["kind"] == "tri":
            for ow, dw, tm, tag in structured_triangle(t, full=t["inst"] == NONE): put(k, ow, dw, tm, tag)
            continue
        rays = structured_sphere(t, rng) if t["kind"] == "sphere" else structured_disk(t, rng)
        for oo, dd, tm, tag in rays:
            ow, dw = _to_world(t["M"], np.asarray(oo, np.float64), np.asarray(dd, np.float64)); put(k, ow, dw, tm, tag)
        if t["kind"] == "disk":   # d.z == 0 for the ray the shape is handed (the world ray; for the rotated disk the object ray's d.z is not 0): disk.rs:66 divides by it
            for tag, dw in (("world d.z == 0", np.array([1.0, 0.3, 0.0])), ("world d.z == 0, -x", np.array([-1.0, 0.2, 0.0]))):
                pw, _ = _to_world(t["M"], np.array([0.3 * t["r"], 0.2 * t["r"], t["zmin"]]), np.zeros(3))
                dw = t["outer"][:3, :3] @ dw
                put(k, pw - 2.0 * dw, dw, np.inf, tag)
    return dict(o=np.array(o, np.float64).astype(F), d=np.array(d, np.float64).astype(F), tmax=np.array(tmax, np.float64).astype(F), target=np.array(which), tag=tags)


# ---- the float64 model -------------------------------------------------------------------------------------------------------------------------------------
def _half_plane_distance(x, y, alpha):
    """Distance in the xy-plane from (x, y) to the half line at angle alpha from the origin."""
    along = x * np.cos(alpha) + y * np.sin(alpha)
    return np.where(along >= 0.0, np.abs(-x * np.sin(alpha) + y * np.cos(alpha)), np.hypot(x, y))


def _t_clear(t, tmax, speed, margin):
    return (np.abs(t) * speed > margin) & (np.abs(t - tmax) * speed > margin)   # (t_max == inf: the second is true)


def _truth_tri(t, o, d, tmax):
    v0, v1, v2 = t["v"]; e1, e2 = v1 - v0, v2 - v0
    n = np.cross(e1, e2); nn = n / np.linalg.norm(n)
    speed = np.linalg.norm(d, axis=1)
    cos = np.abs(d @ nn) / speed
    pv = np.cross(d, e2); det = pv @ e1
    safe = np.where(det == 0.0, 1.0, det)
    tv = o - v0
    b1 = np.einsum("ij,ij->i", tv, pv) / safe
    qv = np.cross(tv, e1)
    b2 = np.einsum("ij,ij->i", d, qv) / safe
    tt = (qv @ e2) / safe
    bmin = np.minimum(np.minimum(b1, b2), 1.0 - b1 - b2)
    margin = MARGIN * t["size"]
    inside = bmin >= 0.0
    hit = inside & (tt > 0.0) & (tt < tmax) & (det != 0.0)
    outside_clear = bmin < -MARGIN
    # a grazing ray (cos < MIN_COS) is unclear only where its line, projected into the triangle's plane, passes over the triangle or within the margin of it
    dp = d - np.outer(d @ nn, nn); dpn = np.linalg.norm(dp, axis=1, keepdims=True)
    side = np.cross(nn, dp / np.where(dpn == 0.0, 1.0, dpn))
    s = np.stack([np.einsum("ij,ij->i", v - o, side) for v in (v0, v1, v2)], axis=1)
    over = (s.min(axis=1) < margin) & (s.max(axis=1) > -margin)
    clear = np.where(cos >= MIN_COS, outside_clear | ((bmin > MARGIN) & _t_clear(tt, tmax, speed, margin)), ~over)
    if t["alpha"]:   # the mask is no part of this model: a ray that reaches the masked quad at all is not classed
        clear = clear & outside_clear
    z = np.zeros(len(o), bool)
    return hit, np.where(hit, tt, np.inf), clear, z, z


def _truth_quadric(t, o, d, tmax):
    Mi = t["Minv"]
    oo = o @ Mi[:3, :3].T + Mi[:3, 3]; dd = d @ Mi[:3, :3].T
    speed = np.linalg.norm(dd, axis=1)
    r = t["r"]; margin = MARGIN * r
    n = len(o); false = np.zeros(n, bool)
    if t["kind"] == "disk":
        h, ri, phimax = t["zmin"], t["ri"], t["phimax"]
        d_handed = d @ t["outer_inv"][:3, :3].T   # the ray Disk::intersect is handed (the world ray; inside an instance the instance's)
        differs = np.abs(d_handed[:, 2] - dd[:, 2]) > 1e-6 * np.maximum(np.abs(dd[:, 2]), 1e-30)
        cos = np.abs(dd[:, 2]) / speed
        parallel = cos < 1e-9
        safe = np.where(dd[:, 2] == 0.0, 1.0, dd[:, 2])
        tt = (h - oo[:, 2]) / safe
        ph = oo + dd * tt[:, None]
        rho = np.hypot(ph[:, 0], ph[:, 1]); phi = np.arctan2(ph[:, 1], ph[:, 0]); phi = np.where(phi < 0.0, phi + 2.0 * np.pi, phi)
        inside = (rho <= r) & (rho >= ri) & ((phi <= phimax) if t["partial_phi"] else True)
        hit = ~parallel & inside & (tt > 0.0) & (tt < tmax)
        edge = np.minimum(np.abs(rho - r), rho)   # the rim and the centre (r_hit == 0 divides dpdv)
        if ri > 0.0: edge = np.minimum(edge, np.abs(rho - ri))
        if t["partial_phi"]: edge = np.minimum(edge, np.minimum(_half_plane_distance(ph[:, 0], ph[:, 1], 0.0), _half_plane_distance(ph[:, 0], ph[:, 1], phimax)))
        outside_clear = ~inside & (edge > margin)
        # a grazing or parallel ray is unclear only where its line, projected into the disk's plane, passes over the disk or within the margin of it
        planar = np.hypot(dd[:, 0], dd[:, 1])
        over = np.abs(oo[:, 0] * dd[:, 1] - oo[:, 1] * dd[:, 0]) / np.where(planar == 0.0, 1.0, planar) < r + margin
        clear = np.where(cos >= MIN_COS, outside_clear | ((edge > margin) & _t_clear(tt, tmax, speed, margin)), ~over | (parallel & (np.abs(oo[:, 2] - h) > margin)))
        # the quirk's own point: t from the handed ray's d.z. It matters for a ray that reaches the disk in either form
        tq = (h - oo[:, 2]) / np.where(d_handed[:, 2] == 0.0, 1e-300, d_handed[:, 2])
        rho_q = np.hypot(oo[:, 0] + dd[:, 0] * tq, oo[:, 1] + dd[:, 1] * tq)
        quirk = differs & (~outside_clear | ~(rho_q > r + margin))
        return hit, np.where(hit, tt, np.inf), clear, quirk, false
    zmin, zmax, phimax = t["zmin"], t["zmax"], t["phimax"]
    a = speed ** 2; b = 2.0 * np.einsum("ij,ij->i", oo, dd); c = np.einsum("ij,ij->i", oo, oo) - r * r
    dist = np.linalg.norm(np.cross(oo, dd), axis=1) / speed
    reach = dist < r
    root = np.sqrt(np.maximum(b * b - 4.0 * a * c, 0.0))
    q = np.where(b < 0.0, -0.5 * (b - root), -0.5 * (b + root)); qs = np.where(q == 0.0, 1.0, q)
    ta, tb = q / a, c / qs
    t0, t1 = np.minimum(ta, tb), np.maximum(ta, tb)

    def at(tt):
        ph = oo + dd * tt[:, None]
        rho = np.hypot(ph[:, 0], ph[:, 1]); phi = np.arctan2(ph[:, 1], ph[:, 0]); phi = np.where(phi < 0.0, phi + 2.0 * np.pi, phi)
        clipped = np.zeros(n, bool); edge = rho.copy()   # the pole (zradius == 0)
        if zmin > -r: clipped |= ph[:, 2] < zmin; edge = np.minimum(edge, np.abs(ph[:, 2] - zmin))
        if zmax < r: clipped |= ph[:, 2] > zmax; edge = np.minimum(edge, np.abs(ph[:, 2] - zmax))
        if t["partial_phi"]:
            clipped |= phi > phimax
            edge = np.minimum(edge, np.minimum(_half_plane_distance(ph[:, 0], ph[:, 1], 0.0), _half_plane_distance(ph[:, 0], ph[:, 1], phimax)))
        ok = (tt > 0.0) & (tt < tmax) & ~clipped
        clear = (edge > margin) & _t_clear(tt, tmax, speed, margin)
        return ok, clear, ph[:, 1] < 0.0

    ok0, clear0, neg0 = at(t0); ok1, clear1, neg1 = at(t1)
    # Sphere::intersect (sphere.rs:59-152): the first root unless it lies behind the origin; the second only where the first was clipped or lies behind
    hit = reach & (ok0 | ((t0 < tmax) & ok1))
    tt = np.where(ok0, t0, t1)
    second = ~ok0 & (t0 < tmax)   # the second root is examined
    # (an origin beyond FAR_ORIGIN radii: the reference's running error bound on c = |o|^2 - r^2, about 2^-20 |o|^2, passes the margin 1e-3 r^2 at |o| = 32 r, and
    #  its conservative `t1.low <= 0` exit then misses spheres the ray goes through -- ref_sphere.cpp sphere_hit, sphere.rs:80-84; such rays are not classed)
    clear = (np.abs(dist - r) > margin) & (~reach | (clear0 & (ok0 | ~second | clear1))) & (~reach | (np.linalg.norm(oo, axis=1) <= FAR_ORIGIN * r))
    quirk_closest = reach & t["partial_phi"] & second & neg1
    quirk_any = reach & t["partial_phi"] & (neg0 | (second & neg1))
    return hit, np.where(hit, tt, np.inf), clear, quirk_closest, quirk_any


def truth(tg, q):
    """The float64 geometry of the float32 rays `q`: dict(hit, t, target (index into tg of the closest hit, -1), clear, quirk_closest, quirk_any). A ray is clear when it is
    clear of every primitive; a quirk of any primitive it reaches takes it out of the hit / miss check."""
    o, d, tmax = (q[k].astype(np.float64) for k in ("o", "d", "tmax"))
    n = len(o)
    best = np.full(n, np.inf); which = np.full(n, -1); clear = np.ones(n, bool); qc = np.zeros(n, bool); qa = np.zeros(n, bool)
    for k, t in enumerate(tg):
        hit, tt, c, quirk_c, quirk_a = (_truth_tri if t["kind"] == "tri" else _truth_quadric)(t, o, d, tmax)
        closer = hit & (tt < best)
        best = np.where(closer, tt, best); which = np.where(closer, k, which)
        clear &= c; qc |= quirk_c; qa |= quirk_a
    return dict(hit=which >= 0, t=best, target=which, clear=clear, quirk_closest=qc, quirk_any=qa)


# ---- checks that do not trust the oracle: on the words of orc_intersect or of the probe ------------------------------------------------------------------------
def field(words, fields, name):
    first, count, is_float = fields[name]
    a = np.ascontiguousarray(words[:, first:first + count])
    a = a.view(F) if is_float else a
    return a[:, 0] if count == 1 else a


def surface_excess(tg, words, fields, rows):
    """Per row of `rows` (hits): how far the box p +- p_error, carried to the object space of the primitive the record names, is from containing a point of the true
    surface, in units of the primitive's size: 0 when the surface passes through the box (its corners lie on both sides), else the nearest corner's distance."""
    lookup = {(t["prim"], t["inst"]): t for t in tg}
    p = field(words, fields, "p").astype(np.float64); e = field(words, fields, "p_error").astype(np.float64)
    prim, inst = field(words, fields, "prim"), field(words, fields, "inst")
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    out = np.zeros(len(rows))
    for j, i in enumerate(rows):
        t = lookup[(int(prim[i]), int(inst[i]))]
        c = p[i] + corners * e[i]
        if t["kind"] == "tri":
            v = t["v"]; n = _unit(np.cross(v[1] - v[0], v[2] - v[0])); f = (c - v[0]) @ n
        else:
            c = c @ t["Minv"][:3, :3].T + t["Minv"][:3, 3]
            f = np.linalg.norm(c, axis=1) - t["r"] if t["kind"] == "sphere" else c[:, 2] - t["zmin"]
        out[j] = max(0.0, f.min(), -f.max()) / t["size"]
    return out


def parallel_excess(words, fields, rows):
    """|cross(normalize(cross(dpdu, dpdv)), n)|: 0 when cross(dpdu, dpdv) is parallel to +-n."""
    du, dv, n = (field(words, fields, k).astype(np.float64)[rows] for k in ("dpdu", "dpdv", "n"))
    c = np.cross(du, dv); c = c / np.linalg.norm(c, axis=1, keepdims=True)
    return np.linalg.norm(np.cross(c, n), axis=1)


def unit_excess(words, fields, rows):
    n, s = (field(words, fields, k).astype(np.float64)[rows] for k in ("n", "sh_n"))
    return np.maximum(np.abs(np.linalg.norm(n, axis=1) - 1.0), np.abs(np.linalg.norm(s, axis=1) - 1.0))


def sphere_normal_excess(tg, q, words, fields, rows):
    """For the rows that hit a sphere under a rigid transform: (|dot(n, normalize(p - centre)) - 1|, the KAT's bound 1e-5 * max(1, |dot|)) (tests/shapes.rs:490-535)."""
    lookup = {(t["prim"], t["inst"]): t for t in tg}
    p, n = field(words, fields, "p").astype(np.float64), field(words, fields, "n").astype(np.float64)
    prim, inst = field(words, fields, "prim"), field(words, fields, "inst")
    err, bound = [], []
    for i in rows:
        t = lookup[(int(prim[i]), int(inst[i]))]
        if t["kind"] != "sphere" or not t["rigid"]: continue
        dot = float(n[i] @ _unit(p[i] - t["M"][:3, 3]))
        err.append(abs(dot - 1.0)); bound.append(1e-5 * max(1.0, abs(dot)))
    return np.array(err), np.array(bound)


# Tolerances of the float64 checks. The box and parallelism tolerances are 4 x the worst value the ORACLE's own output shows over the three scenes' clear rays
# (tests/test_interaction_zoo.py measures them again on every run and asserts they still hold): see the measured values beside each.
BOX_TOL = 4 * 0.0                 # measured worst surface_excess: 0.0 in all six query sets -- the surface passes through every box p +- p_error
PARALLEL_TOL = 4 * 2.12e-7        # measured worst parallel_excess: 2.119e-07 (quadric_zoo random; 1.655e-07 structured, instanced_zoo 1.657e-07 / 1.377e-07, tri_zoo 0)
# n and sh_n come out of a float32 normalize (a dot product of three squares, a square root, three divisions: under 3 ulp of 1) and, for instances and quadrics, a second
# one after the transform: 8 * 2^-24 covers both
UNIT_TOL = 8 * 2.0 ** -24


def check_against_float64(name, tg, q, tr, words, fields, hit_any=None):
    """The checks of the module docstring on the clear rays of one query set; `words`: orc_intersect's or the probe's. Returns the figures for the printed line."""
    hit = field(words, fields, "hit") != 0
    clear = tr["clear"]
    hm = clear & ~tr["quirk_closest"]
    bad = np.flatnonzero(hm & (hit != tr["hit"]))
    assert len(bad) == 0, f"{name}: hit / miss differs from the float64 geometry for {len(bad)} clear rays; first: ray {bad[0]} ({q['tag'][bad[0]]}), float64 hit {tr['hit'][bad[0]]}"
    if hit_any is not None:
        ha = clear & ~tr["quirk_any"] & ~tr["quirk_closest"]
        bad = np.flatnonzero(ha & ((hit_any != 0) != tr["hit"]))
        assert len(bad) == 0, f"{name}: any-hit differs from the float64 geometry for {len(bad)} clear rays; first: ray {bad[0]} ({q['tag'][bad[0]]})"
    rows = np.flatnonzero(hm & hit & tr["hit"])
    prim, inst = field(words, fields, "prim"), field(words, fields, "inst")
    want = np.array([(tg[k]["prim"], tg[k]["inst"]) for k in tr["target"][rows]], np.int64).reshape(-1, 2)
    same = (prim[rows] == want[:, 0]) & (inst[rows] == want[:, 1])
    assert same.all(), f"{name}: {int((~same).sum())} clear rays hit another primitive than the float64 geometry's closest; first: ray {rows[np.flatnonzero(~same)[0]]}"
    box = surface_excess(tg, words, fields, rows); par = parallel_excess(words, fields, rows); unit = unit_excess(words, fields, rows)
    uv = field(words, fields, "uv")[rows]
    fig = dict(clear=int(clear.sum()), checked=len(rows), box=float(box.max(initial=0.0)), parallel=float(par.max(initial=0.0)), unit=float(unit.max(initial=0.0)))
    assert box.max(initial=0.0) <= BOX_TOL, f"{name}: p +- p_error misses the true surface by {box.max():.3e} sizes at ray {rows[box.argmax()]} ({q['tag'][rows[box.argmax()]]})"
    assert par.max(initial=0.0) <= PARALLEL_TOL, f"{name}: cross(dpdu, dpdv) not parallel to n: {par.max():.3e} at ray {rows[par.argmax()]} ({q['tag'][rows[par.argmax()]]})"
    assert unit.max(initial=0.0) <= UNIT_TOL, f"{name}: |n| or |sh_n| off 1 by {unit.max():.3e} at ray {rows[unit.argmax()]}"
    assert ((uv >= 0.0) & (uv <= 1.0)).all(), f"{name}: uv outside [0, 1]^2 at ray {rows[np.flatnonzero(~((uv >= 0.0) & (uv <= 1.0)).all(axis=1))[0]]}"
    err, bound = sphere_normal_excess(tg, q, words, fields, rows)
    assert (err <= bound).all(), f"{name}: a rigid sphere's n is off the radius by {err.max():.3e}"
    fig["sphere_normals"] = len(err)
    return fig


# ---- one scene with its queries and the oracle's answers, computed once per session ---------------------------------------------------------------------------
_CASES = {}
HIT_SHARE_FLOOR = 0.5       # of a scene's random rays
CLEAR_SHARE_FLOOR = 0.6     # of a scene's structured quadric rays


def case(pkg, oracle, name):
    if name in _CASES:
        return _CASES[name]
    from oracle.oracle_binding import INTERSECT_FIELDS
    b, names = SCENES[name](pkg)
    sd, rp = b.world_end()
    tg = targets(pkg, sd)
    sets = {"random": random_queries(tg, seed=11 + len(tg)), "structured": structured_queries(tg, seed=5 + len(tg))}
    orc = oracle.scene(sd)
    ref = {}
    for part, q in sets.items():
        words = orc.intersect(q["o"], q["d"], q["tmax"]); counters = orc.counters()
        closest = orc.trace_closest(q["o"], q["d"], q["tmax"]); closest_counters = orc.counters()
        t = field(words, INTERSECT_FIELDS, "t").astype(np.float64); hit = field(words, INTERSECT_FIELDS, "hit") != 0
        lo = np.where(hit, t * (1.0 - 2.0 ** -16), np.inf).astype(F); hi = np.where(hit, t * (1.0 + 2.0 ** -16), np.inf).astype(F)
        inf = np.full(len(t), np.inf, F)
        anys = {}
        for key, tm in (("lo", lo), ("hi", hi), ("inf", inf)):
            anys[key] = (tm, orc.trace_any(q["o"], q["d"], tm), orc.counters())
        ref[part] = dict(words=words, counters=counters, closest=closest, closest_counters=closest_counters, any=anys, truth=truth(tg, q))
    orc.close()
    _CASES[name] = dict(sd=sd, rp=rp, targets=tg, names=names, sets=sets, ref=ref, fields=INTERSECT_FIELDS)
    return _CASES[name]


def check_conditions(name, c):
    """A test must not pass by comparing nothing: the floors of the module docstring, on the oracle's answers alone. Returns the figures for the printed line."""
    tg, fields = c["targets"], c["fields"]
    fig = {}
    for part in ("random", "structured"):
        w = c["ref"][part]["words"]
        hit = field(w, fields, "hit") != 0
        got = set(zip(field(w, fields, "prim")[hit].tolist(), field(w, fields, "inst")[hit].tolist()))
        missing = [(t["prim"], t["inst"]) for t in tg if (t["prim"], t["inst"]) not in got]
        assert not missing, f"{name}: no {part} ray hits (prim, inst) {missing}"
        fig[part] = (len(hit), int(hit.sum()))
    share = fig["random"][1] / fig["random"][0]
    assert share >= HIT_SHARE_FLOOR, f"{name}: only {share:.3f} of the random rays hit"
    q, tr = c["sets"]["structured"], c["ref"]["structured"]["truth"]
    quadric = np.array([tg[k]["kind"] != "tri" for k in q["target"]])
    if quadric.any():
        cs = float(tr["clear"][quadric].mean())
        assert cs >= CLEAR_SHARE_FLOOR, f"{name}: only {cs:.3f} of the structured quadric rays class as clear"
        fig["clear_share"] = cs
    return fig
