"""Scenes of the lightmap tests (tests/test_bake_light_model.py, tests/test_bake_light.py): the geometries of tests/bake_scenes.py under lights. The lights come
first, so the shapes some of them are (quad, sphere, disk) take the first shape ordinals: scene() returns the ordinal of the bake target with the scene data."""
import numpy as np
import bake_scenes as S


def point(b, at=(0.3, 0.2, 1.5), I=(3.0, 2.0, 1.0)):
    b.attribute_begin(); b.translate(*at); b.light_source("point", I=I); b.attribute_end()   # (the position through the CTM: "from" has the reference's x, y, x quirk)
    return 0


def spot(b):
    b.light_source("spot", from_=(0.0, 0.0, 2.0), to=(0.5, 0.0, 0.0), I=(4.0, 4.0, 3.0), coneangle=25.0, conedeltaangle=8.0)   # a pool of ~0.9 radius: most of the floor is outside
    return 0


def distant(b, frm=(0.3, 0.5, 1.0), L=(1.0, 0.9, 0.8)):
    b.light_source("distant", from_=frm, to=(0.0, 0.0, 0.0), L=L)
    return 0


def quad(b, twosided=False, z=1.8, at=(-0.5, 0.4), half=0.35, L=(5.0, 4.0, 3.0), up=False):
    """A two-triangle quad light facing down (its normal is -z; `up`: +z, so a one-sided one sends nothing to the floor)."""
    x, y = at
    P = [(x - half, y - half, z), (x - half, y + half, z), (x + half, y + half, z), (x + half, y - half, z)]
    if up:
        P = P[::-1]
    b.attribute_begin(); b.area_light_source(L=L, twosided=twosided); b.trianglemesh(P, S.QUAD_IDX); b.attribute_end()
    return 1


def yardstick(b):
    """A small emissive triangle: the lights whose far end the model cannot restate are held against the exact rays of this one (tests/lightmap_reference.py)."""
    b.attribute_begin(); b.area_light_source(L=(2.0, 2.0, 2.0), twosided=True)
    b.trianglemesh([(1.2, 1.1, 1.4), (1.5, 1.2, 1.5), (1.3, 1.5, 1.3)], [0, 1, 2]); b.attribute_end()
    return 1


def sphere(b):
    b.attribute_begin(); b.translate(-0.8, 0.5, 1.6); b.area_light_source(L=(6.0, 5.0, 4.0), twosided=True); b.sphere(radius=0.3); b.attribute_end()
    return 1


def disk(b):
    b.attribute_begin(); b.translate(0.7, -0.6, 1.7); b.rotate(180.0, 1, 0, 0); b.area_light_source(L=(3.0, 5.0, 4.0)); b.disk(radius=0.4); b.attribute_end()   # turned to face the floor
    return 1


def infinite(b):
    b.light_source("infinite", L=(0.5, 0.6, 0.7))
    return 0


def envmap(b):
    tex = np.random.RandomState(5).uniform(0.1, 2.0, (8, 16, 3)).astype(np.float32)
    b.attribute_begin(); b.rotate(35.0, 0.2, 1, 0.1); b.light_source("infinite", texels=tex); b.attribute_end()
    return 0


LIGHTS = {
    "point": [point],
    "spot": [spot],
    "distant": [distant, yardstick],
    "quad": [quad],
    "quad_twosided": [lambda b: quad(b, twosided=True)],
    "sphere": [sphere, yardstick],
    "disk": [disk, yardstick],
    "infinite": [infinite, yardstick],
    "envmap": [envmap, yardstick],
    "all": [point, spot, distant, quad, sphere, disk, envmap],      # 8 lights: the quad is two
    "point_quad": [point, lambda b: quad(b, twosided=True)],       # 3 lights
}
GEOMETRY = {
    "open_floor": S.open_floor,
    "occluded_floor": S.occluded_floor,
    "shaded_normals": lambda pkg: S.shaded(pkg, normals=True),
    "shaded_mirror": lambda pkg: S.shaded(pkg, mirror=True),
}


def scene(pkg, geometry, lights):
    """(scene data, the bake target's shape ordinal) of GEOMETRY[geometry] under LIGHTS[lights] (or a list of light functions)."""
    adders = LIGHTS[lights] if isinstance(lights, str) else lights
    shapes = []
    builder = S._builder

    def lit(p):
        b = builder(p)
        shapes.append(sum(add(b) for add in adders))
        return b
    S._builder = lit   # (the geometries make their own builder: hand them one that holds the lights already)
    try:
        sd = GEOMETRY[geometry](pkg)
    finally:
        S._builder = builder
    return sd, shapes[0]


def emissive_floor(pkg):
    """A floor that is itself an area light (its two triangles are lights 0 and 1) under a point light (light 2): shape 0."""
    b = S._builder(pkg)
    b.attribute_begin(); b.area_light_source(L=(1.0, 2.0, 3.0), twosided=True); S.floor(b); b.attribute_end()
    point(b)
    return b.world_end()[0], 0
