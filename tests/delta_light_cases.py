"""Scenes and float64 restatements shared by test_delta_lights.py and test_delta_lights_host.py.

The restatements are written from the rules in include/pupil_pt.h (PUPIL_EMITTER_POINT), not from
the kernels: a point light of intensity I at L lights a diffuse surface point P with normal n by
albedo / pi * max(0, n . wi) * I / d^2, wi = (L - P) / d; a spot multiplies that by mitsuba's
falloff of the angle between -wi and its axis; a directional light of irradiance E travelling
along dir gives albedo / pi * max(0, n . -dir) * E."""
import numpy as np

from pupiloptixlab_amd import abi
from pupiloptixlab_amd import world as W

ALBEDO = np.array([0.5, 0.6, 0.7])
POINT_POS = np.array([0.3, 1.5, -0.2])
POINT_I = np.array([10.0, 8.0, 6.0])
DIR_D = np.array([0.3, -1.0, 0.2]) / np.linalg.norm([0.3, -1.0, 0.2])
DIR_E = np.array([3.0, 2.0, 1.0])
SPOT_AXIS = np.array([np.sin(np.deg2rad(10.0)), -np.cos(np.deg2rad(10.0)), 0.0])  # (0, -1, 0) tilted 10 deg to +x
SPOT_CUTOFF, SPOT_BEAM = 35.0, 20.0
OCC_Y, OCC_HALF = 0.75, 0.5  # the 1 x 1 occluder under the point light
FLOOR_N = np.array([0.0, 1.0, 0.0])

# 8 x 8 floor points within |x|, |z| <= 1.4
GRID = np.linspace(-1.4, 1.4, 8)
POINTS = np.array([(x, 0.0, z) for z in GRID for x in GRID])

# Tolerance of a closed-form comparison, relative.  From the hit record to the radiance the chain is
# the barycentric position (5 ops per axis), its transform (7), L - P (1), the dot (5), 1 / sqrt, the
# scale of wi, n . wi (5), d = sqrt (1), d * d, 1 / d^2, color * that, albedo / pi, the product of T,
# radiance, f, NoL and mis (5) and the division by pdf_l: under 50 float32 operations, each within
# 2^-24 relative (sqrt and division are correctly rounded, nothing is contracted), so at most
# 50 * 2^-24 = 3e-6 if every error pointed the same way.  1e-5 leaves a factor of three.
RTOL = 1e-5
assert 50 * 2.0 ** -24 < RTOL / 3


def floor_world(max_depth=2, occluder=None, film=(8, 8), cam_height=4.0):
    """The common scene: a 4 x 4 rectangle at y = 0 facing +Y, two-sided diffuse ALBEDO; no env, no
    area light.  occluder: the centre (x, z) of a 1 x 1 rectangle at y = OCC_Y."""
    wd = W.World()
    wd.set_film(film[0], film[1], max_depth)
    rect = wd.add_builtin("rectangle")
    mat = wd.add_material(W.twosided(W.diffuse(tuple(ALBEDO))))
    wd.add_instance(rect, mat, W.transform(scale=(2, 2, 1), rotate=((1, 0, 0), -90)))
    if occluder is not None:
        wd.add_instance(rect, mat, W.transform(scale=(OCC_HALF, OCC_HALF, 1), rotate=((1, 0, 0), -90),
                                               translate=(occluder[0], OCC_Y, occluder[1])))
    wd.set_sensor(60.0, W.look_at_mitsuba((0.0, cam_height, 0.0), (0.0, 0.0, 0.0), (0, 0, 1)), fov_axis="y")
    return wd


def box_world(max_depth=4, lamp=False, film=(16, 16)):
    """A 4 x 4 x 4 box of five rectangles (floor, ceiling, three walls; the camera looks in through
    the open side) with a point light inside, and with lamp=True a small emissive rectangle under
    the ceiling as well."""
    wd = W.World()
    wd.set_film(film[0], film[1], max_depth)
    rect = wd.add_builtin("rectangle")
    mat = wd.add_material(W.twosided(W.diffuse(tuple(ALBEDO))))
    for rot, tr in ((((1, 0, 0), -90), (0, 0, 0)), (((1, 0, 0), 90), (0, 4, 0)), (None, (0, 2, -2)),
                    (((0, 1, 0), 90), (-2, 2, 0)), (((0, 1, 0), -90), (2, 2, 0))):
        wd.add_instance(rect, mat, W.transform(scale=(2, 2, 1), rotate=rot, translate=tr))
    if lamp:
        wd.lamp = wd.add_instance(rect, mat, W.transform(scale=(0.4, 0.4, 1), rotate=((1, 0, 0), 90),
                                                         translate=(0.3, 3.9, 0.1)), emitter_radiance=(12.0, 11.0, 9.0))
    wd.add_point_light((-0.6, 2.5, 0.4), (6.0, 7.0, 8.0))
    wd.set_sensor(60.0, W.look_at_mitsuba((0.0, 2.0, 5.5), (0.0, 2.0, 0.0), (0, 1, 0)), fov_axis="y")
    return wd


def rays_down(points=POINTS, height=2.0):
    """(n, 8) float32 rays from `height` above each point straight down."""
    r = np.zeros((len(points), 8), np.float32)
    r[:, 0], r[:, 1], r[:, 2] = points[:, 0], height, points[:, 2]
    r[:, 4] = -1.0
    r[:, 7] = 1e16
    return r


# ------------------------------------------------------------------ float64 restatements
def point_sample(pos, intensity, p):
    """wi, distance, radiance of the point light from shading points p (n, 3)."""
    d = pos[None, :] - p
    dist = np.linalg.norm(d, axis=1)
    return d / dist[:, None], dist, intensity[None, :] / (dist ** 2)[:, None]


def spot_angle(pos, axis, p):
    wi, _, _ = point_sample(pos, np.ones(3), p)
    return np.arccos(np.clip((-wi) @ axis, -1.0, 1.0))


def spot_falloff(a, cutoff, beam):
    """1 for a <= beam, 0 for a >= cutoff, linear in the angle between (radians)."""
    out = np.where(a <= beam, 1.0, 0.0)
    mid = (a > beam) & (a < cutoff)
    if cutoff > beam:
        out = np.where(mid, (cutoff - a) / (cutoff - beam), out)
    return out


def lit(wi, radiance, n=FLOOR_N, albedo=ALBEDO):
    """The direct term of a diffuse surface: albedo / pi * max(0, n . wi) * radiance."""
    cos = np.maximum(0.0, wi @ n)
    return albedo[None, :] / np.pi * cos[:, None] * radiance


def point_expect(p=POINTS, pos=POINT_POS, intensity=POINT_I):
    wi, _, rad = point_sample(pos, intensity, p)
    return lit(wi, rad)


def dir_expect(p=POINTS, d=DIR_D, e=DIR_E):
    wi = np.repeat((-d)[None, :], len(p), axis=0)
    return lit(wi, np.repeat(e[None, :], len(p), axis=0))


def shadow_classes(cross, centre):
    """Where the segments to the light cross the occluder's plane (n, 2: x, z) against the 1 x 1
    occluder centred at `centre`: (shadowed, lit, left out) masks -- at least 0.05 inside its edge,
    at least 0.05 outside, nearer the edge than that."""
    dx, dz = np.abs(cross[:, 0] - centre[0]), np.abs(cross[:, 1] - centre[1])
    eps = 1e-9  # a grid point that lies on a margin to within rounding is 0.05 from the edge
    inside = (dx <= OCC_HALF - 0.05 + eps) & (dz <= OCC_HALF - 0.05 + eps)
    outside = (dx >= OCC_HALF + 0.05 - eps) | (dz >= OCC_HALF + 0.05 - eps)
    return inside, outside, ~(inside | outside)


def select_scan(select_probability, p, has_env):
    """SelectOneEmiiter (render/emitter.h:110-135) in float32 over the table as read back: the
    first i with p <= sum_p + select_probability[i], else -1 for the env, else the last entry."""
    sp = np.asarray(select_probability, np.float32)
    out = np.empty(len(p), np.int32)
    for k, x in enumerate(np.asarray(p, np.float32)):
        sum_p = np.float32(0.0)
        pick = -1 if has_env else len(sp) - 1
        for i in range(len(sp)):
            if x <= np.float32(sum_p + sp[i]):
                pick = i
                break
            sum_p = np.float32(sum_p + sp[i])
        out[k] = pick
    return out


def compute_probability(weights, num_delta, has_env):
    """EmitterHelper::ComputeProbability (world/emitter.cpp:321-337) in float32: `weights` of the
    true area emitters in table order, then num_delta delta lights of weight 1, and the env."""
    f = np.float32
    w = [f(x) for x in weights]
    s = f(0.0)
    for x in w:
        s = f(s + x)
    areas = [f(f(x / s) * f(len(w))) for x in w]
    emitter_num = f(len(w) + num_delta + (1 if has_env else 0))
    areas = [f(x / emitter_num) for x in areas]
    delta = [f(f(1.0) / emitter_num)] * num_delta
    return np.array(areas + delta, np.float32), f(f(1.0) / emitter_num)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def emitter_fields(e):
    """The fields of an abi.Emitter a delta light uses, as numpy."""
    return {"type": int(e.type), "weight": np.float32(e.weight), "select_probability": np.float32(e.select_probability),
            "area": np.float32(e.area), "center": np.array(list(e.center), np.float32),
            "color": np.array(list(e.color), np.float32), "axis": np.array(list(e.nrm[0]), np.float32),
            "cutoff": np.float32(e.pos[0][0]), "beam": np.float32(e.pos[0][1])}


DELTA_TYPES = (abi.EMITTER_POINT, abi.EMITTER_SPOT, abi.EMITTER_DIRECTIONAL)
