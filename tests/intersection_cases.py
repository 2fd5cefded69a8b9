"""Degenerate-ray cases and float64 references shared by test_intersection_degenerate.py (the
oracle against numpy, CPU) and test_gpu_intersection_degenerate.py (the traversal kernels against
the oracle, bit for bit, and against the same references, on the very same rays).

The parity tests use generic random rays in the window [0.001, 1e16].  The families here are the
cases a ray tracer usually gets wrong: direction components of +-0 (the 1e-30 clamp of ray_pre,
idir = +-1e30), rays lying in a box face plane, rays through shared edges and vertices (the
U == 0 double-precision fallback of the watertight test), equal-t ties, and tmin / tmax windows
that sit between hits (what every shadow ray uses).

Every mesh vertex, ray origin and ray direction is a float32 value before it is widened, so the
references see the inputs of the code under test.  The lattice scene's coordinates are dyadic
(multiples of 1/8 of magnitude <= 2): differences, products and sums of them are exact in
float32, so for rays with two zero direction components the float32 test, the float64 reference
and the exact answer coincide -- hits, ties and distances (the doubled triangle area is 1/16, a
power of two, so the reciprocal is exact too).

References: a float64 Moller-Trumbore over every triangle (the tied set: hit inside the window
with barycentrics >= -1e-5; the strict set: barycentrics >= +1e-5) and the analytic roots of
|M^-1 (o + t d)| = 1 for the builtin spheres.  Test infrastructure only; pure numpy.
"""
import numpy as np

from pupiloptixlab_amd import World
from pupiloptixlab_amd import world as W

F32, F64 = np.float32, np.float64
MISS = 0xFFFFFFFF
TMIN, TMAX = 0.001, 1e16            # the path tracer's window
T_RTOL, T_ATOL, B_ATOL = 3e-5, 1e-6, 1e-4  # float32 against float64 (test_intersection_restatement.py)
BARY_EPS = 1e-5                     # tied set >= -BARY_EPS, strict set >= +BARY_EPS

FAMILIES = ["axis", "exact_edge", "no_leak", "window", "sphere", "instanced", "single"]


class Case:
    """world / desc of a family, its rays (n, 8) = o, d, tmin, tmax, a tag per ray, the world-space
    triangles in primitive-id order (float64 (m, 3, 3)) and the spheres [(primitive id, float64
    3 x 4 instance matrix)].
    exact[i]: ray i's float32 arithmetic is exact (lattice scene, two zero direction components).
    ref_rays / alt_rays: the windows the references are taken under.  They are the rays' own except
    for rays tagged "equal" (tmax = fl(t1): either outcome is right for that one hit), which get
    tmax a relative 1e-4 above t1 in ref_rays and as much below it in alt_rays; the answer must
    match one of the two."""

    def __init__(self, name, world, rays, tags, tris, spheres=(), exact=None, ref_rays=None, alt_rays=None):
        self.name, self.world, self.desc = name, world, world.desc()
        self.rays = np.ascontiguousarray(rays, F32)
        assert self.rays.shape[1] == 8 and np.isfinite(self.rays).all()
        self.tags = np.asarray(tags)
        assert len(self.tags) == len(self.rays)
        self.tris = np.asarray(tris, F64).reshape(-1, 3, 3)
        self.spheres = list(spheres)
        self.exact = np.zeros(len(self.rays), bool) if exact is None else np.asarray(exact, bool)
        self.ref_rays = self.rays if ref_rays is None else np.ascontiguousarray(ref_rays, F32)
        self.alt_rays = None if alt_rays is None else np.ascontiguousarray(alt_rays, F32)

    @property
    def n(self):
        return len(self.rays)


def _rays8(o, d, tmin=TMIN, tmax=TMAX):
    o = np.asarray(o, F32).reshape(-1, 3)
    d = np.asarray(d, F32).reshape(-1, 3)
    n = max(len(o), len(d))
    o, d = np.broadcast_to(o, (n, 3)), np.broadcast_to(d, (n, 3))
    w = np.empty((n, 2), F32)
    w[:, 0], w[:, 1] = tmin, tmax
    return np.concatenate([o, d, w], 1)


def _unit32(v):
    v = np.asarray(v, F64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


# ------------------------------------------------------------------ scenes
LATTICE_Z = (0.5, 1.0, 1.5)
HALF = np.arange(-8, 9) / 8.0   # the half lattice on [-1, 1]: vertices, edge midpoints, cell centres


def lattice_mesh():
    """Three 9 x 9-vertex sheets over [-1, 1]^2 at z = 0.5, 1, 1.5, two triangles per cell of 1/4:
    (243, 3) float32 positions, (384, 3) uint32 indices.  The outer bounding planes are
    |x| = 1, |y| = 1, z = 0.5 and z = 1.5."""
    g = np.arange(9) / 4.0 - 1.0
    pos, idx = [], []
    for k, z in enumerate(LATTICE_Z):
        yy, xx = np.meshgrid(g, g, indexing="ij")
        pos.append(np.stack([xx, yy, np.full_like(xx, z)], -1).reshape(-1, 3))
        for j in range(8):
            for i in range(8):
                v00 = 81 * k + 9 * j + i
                v10, v01, v11 = v00 + 1, v00 + 9, v00 + 10
                idx += [(v00, v10, v11), (v00, v11, v01)]
    return np.concatenate(pos).astype(F32), np.asarray(idx, np.uint32)


def icosphere(subdiv=2):
    """A closed unit icosphere: 20 * 4^subdiv faces (320), float32 vertices."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, F64) / np.linalg.norm(x) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v).astype(F32), np.asarray(f, np.uint32)


def _world(film=8):
    w = World()
    w.set_film(film, film, 2)
    w.set_sensor(40.0, W.look_at_mitsuba((0, 0, -6), (0, 0, 0), (0, 1, 0)))
    return w


def _mesh_world(pos, idx, transforms=(None,)):
    """One mesh under the given instance matrices (4 x 4 or None); the world-space triangles by id."""
    w = _world()
    mesh = w.add_mesh(pos, idx)
    mat = w.add_material(W.diffuse(0.5))
    tris = []
    for m in transforms:
        w.add_instance(mesh, mat, m)
        m4 = np.eye(4) if m is None else np.asarray(m, F32).astype(F64)
        # fl32(M v): exact for the matrices used here (entries 0, +-1, 2, 0.5; dyadic translations)
        wp = (pos.astype(F64) @ m4[:3, :3].T + m4[:3, 3]).astype(F32).astype(F64)
        assert np.array_equal(wp, pos.astype(F64) @ m4[:3, :3].T + m4[:3, 3]), "instance matrix is not exact"
        tris.append(wp[idx.astype(np.int64)])
    return w, np.concatenate(tris)


# ------------------------------------------------------------------ ray sets
def _zero_signs():
    return [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)]


def axis_rays():
    """Rays of the lattice scene with one or two direction components of +-0: (rays, tags, exact)."""
    rays, tags, exact = [], [], []

    def add(r, tag, ex):
        rays.append(r)
        tags.extend([tag] * len(r))
        exact.extend([ex] * len(r))

    yy, xx = np.meshgrid(HALF, HALF, indexing="ij")
    xy = np.stack([xx.ravel(), yy.ravel()], 1)  # 289 points: on vertices, edge midpoints, cell centres, |x| = 1, |y| = 1
    # +-z from outside the slab, every sign combination of the two zero components
    for dz, oz in ((1.0, 0.0), (-1.0, 2.0)):
        for sx, sy in _zero_signs():
            o = np.concatenate([xy, np.full((len(xy), 1), oz)], 1)
            add(_rays8(o, [(sx, sy, dz)]), "z_outside", True)
    # +-z from between two sheets and from a sheet itself (t = 0 lies below tmin)
    for oz, tag, (sx, sy) in ((0.75, "z_between", (0.0, -0.0)), (1.0, "z_on_sheet", (-0.0, 0.0))):
        for dz in (1.0, -1.0):
            o = np.concatenate([xy, np.full((len(xy), 1), oz)], 1)
            add(_rays8(o, [(sx, sy, dz)]), tag, True)
    # +-x and +-y in a sheet's plane (edge-on: a miss in every implementation), in the outer bounding
    # planes z = 0.5 and z = 1.5 (edge-on as well) and in a plane between the sheets
    for axis in (0, 1):
        for z in (0.5, 1.0, 1.5, 0.75):
            for sgn, start in ((1.0, -2.0), (-1.0, 2.0)):
                for s1, s2 in _zero_signs():
                    o = np.zeros((len(HALF), 3))
                    o[:, axis], o[:, 1 - axis], o[:, 2] = start, HALF, z
                    d = np.zeros(3)
                    d[axis], d[1 - axis], d[2] = sgn, s1, s2
                    add(_rays8(o, [d]), "in_plane", True)
    # one zero component: (0, +-0.6, +-0.8) and (+-0.6, 0, +-0.8) from the half lattice on the other axis,
    # the outer planes |x| = 1 and |y| = 1 included
    for axis in (0, 1):
        for z0 in (-0.0, 0.0):
            for s1 in (0.6, -0.6):
                for dz, oz in ((0.8, 0.0), (-0.8, 2.0)):
                    for c in (-0.5, 0.125):
                        o = np.zeros((len(HALF), 3))
                        o[:, axis], o[:, 1 - axis], o[:, 2] = HALF, c, oz
                        d = np.zeros(3)
                        d[axis], d[1 - axis], d[2] = z0, s1, dz
                        add(_rays8(o, [d]), "one_zero", False)
    return np.concatenate(rays), tags, np.asarray(exact)


def axis_case():
    pos, idx = lattice_mesh()
    w, tris = _mesh_world(pos, idx)
    rays, tags, exact = axis_rays()
    return Case("axis", w, rays, tags, tris, exact=exact)


def exact_edge_case():
    """Non-axis rays through lattice vertices, edge midpoints and along cell diagonals.  Directions
    with components of equal magnitude ((+-1, 0, +-1) / sqrt 2, (+-1, +-1, +-1) / sqrt 3, ...) make the
    shear Sx, Sy of the watertight test exactly 0 or +-1, so from lattice origins U, V or W is exactly 0
    on every shared edge and vertex the ray crosses.  The second half aims float32-normalised
    directions at interior vertices and edge midpoints from generic origins (the ray passes within
    a few 1e-8 of them)."""
    pos, idx = lattice_mesh()
    w, tris = _mesh_world(pos, idx)
    rays, tags = [], []
    dirs = [(sx, 0, sz) for sx in (1, -1) for sz in (1, -1)] + [(0, sy, sz) for sy in (1, -1) for sz in (1, -1)] + \
           [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    g = np.arange(-8, 9, 2) / 8.0
    for d in dirs:
        d32 = _unit32(d)
        assert all(abs(c) in (0.0, abs(d32[np.flatnonzero(d32)[0]])) for c in d32)
        oz = 0.0 if d[2] > 0 else 2.0
        # lattice origins (vertex and vertical / horizontal edge hits) and origins shifted by 1/8 on both
        # axes (hits on the cells' diagonal edges for (1, 1, 1)-like directions)
        for shift, tag in ((0.0, "vertex"), (0.125, "edge")):
            yy, xx = np.meshgrid(g[:-1] + shift, g[:-1] + shift, indexing="ij")
            o = np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, oz)], 1)
            rays.append(_rays8(o, [d32]))
            tags += [tag] * len(o)
    v = pos.astype(F64)
    inner = (np.abs(v[:, 0]) < 1) & (np.abs(v[:, 1]) < 1)
    e_mid = np.concatenate([0.5 * (v[idx[:, a]] + v[idx[:, b]]) for a, b in ((0, 1), (1, 2), (2, 0))])
    e_mid = e_mid[(np.abs(e_mid[:, 0]) < 1) & (np.abs(e_mid[:, 1]) < 1)]
    targets = np.unique(np.concatenate([v[inner], e_mid]), axis=0)
    for o in ((0.3, -0.2, -0.7), (-0.55, 0.35, 2.6)):
        o32 = np.asarray(o, F32)
        rays.append(_rays8([o32], _unit32(targets - o32.astype(F64))))
        tags += ["near_edge"] * len(targets)
    return Case("exact_edge", w, np.concatenate(rays), tags, tris)


def no_leak_case():
    """A closed icosphere from 3 interior origins towards every vertex, every edge midpoint and the
    +-1 ulp neighbours of those directions: every ray must hit."""
    pos, idx = icosphere(2)
    w, tris = _mesh_world(pos, idx)
    v = pos.astype(F64)
    edges = np.unique(np.sort(np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]]), 1), axis=0)
    targets = np.concatenate([v, 0.5 * (v[edges[:, 0]] + v[edges[:, 1]])])
    assert len(idx) == 320 and len(v) == 162 and len(edges) == 480
    rays, tags = [], []
    for o in ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1), (-0.5, 0.4, 0.45)):
        o32 = np.asarray(o, F32)
        d = _unit32(targets - o32.astype(F64))
        for dd, tag in ((d, "aimed"), (np.nextafter(d, F32(np.inf)), "ulp_up"), (np.nextafter(d, F32(-np.inf)), "ulp_down")):
            rays.append(_rays8([o32], dd))
            tags += [tag] * len(dd)
    return Case("no_leak", w, np.concatenate(rays), tags, tris)


def _ulps(x, k):
    x = np.asarray(x, F32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def window_case():
    """tmin / tmax windows around the three hits t1 < t2 < t3 of rays through the lattice scene.
    Axis rays: exact arithmetic, so the window edges sit 4 ulps from fl(t1) = t1.  Oblique rays: the
    edges sit a relative 1e-4 away, beyond the t tolerance (3e-5), so the reference's answer holds for
    any float32 result inside the tolerance."""
    pos, idx = lattice_mesh()
    w, tris = _mesh_world(pos, idx)
    g = np.arange(8) / 4.0 - 1.0
    yy, xx = np.meshgrid(g + 0.125, g + 0.0625, indexing="ij")  # strictly inside the lower triangle of each cell
    xy = np.stack([xx.ravel(), yy.ravel()], 1)
    base = []  # (o, d, exact)
    for dz, oz in ((1.0, 0.0), (-1.0, 2.0)):
        for p in xy:
            base.append(((p[0], p[1], oz), (0.0, -0.0, dz), True))
    rng = np.random.default_rng(41)
    for _ in range(64):
        o = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -0.25])
        tgt = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), 1.5])
        base.append((o, _unit32(tgt - o), False))
    rays, ref, alt, tags, exact = [], [], [], [], []
    for o, d, ex in base:
        o32, d32 = np.asarray(o, F32), np.asarray(d, F32)
        t, _, _, _ = mt_reference(o32[None], d32[None], np.array([[0.0, 1e16]]), tris)
        ts = np.sort(t[0][np.isfinite(t[0])])
        assert len(ts) == 3 and ts[0] > 0.1, (o, d, ts)
        t1, t2, t3 = ts
        f1 = F32(t1)
        lo, hi = (_ulps(f1, -4), _ulps(f1, 4)) if ex else (F32(t1 * (1 - 1e-4)), F32(t1 * (1 + 1e-4)))
        m12, m23 = F32(0.5 * (t1 + t2)), F32(0.5 * (t2 + t3))
        windows = [("tmax_below", TMIN, lo), ("equal", TMIN, f1), ("tmax_above", TMIN, hi),
                   ("tmin_between", m12, TMAX), ("tmin_tmax_between", m12, m23), ("empty", hi, F32(t2 * (1 - 1e-4))),
                   ("tmin_below", lo, TMAX), ("tmin_above", hi, TMAX), ("past_all", F32(t3 * (1 + 1e-4)), TMAX)]
        for tag, a, b in windows:
            rays.append(_rays8([o32], [d32], a, b))
            ref.append(_rays8([o32], [d32], a, F32(t1 * (1 + 1e-4)) if tag == "equal" else b))
            alt.append(_rays8([o32], [d32], a, F32(t1 * (1 - 1e-4)) if tag == "equal" else b))
            tags.append(tag)
            exact.append(ex)
    return Case("window", w, np.concatenate(rays), tags, tris, exact=exact, ref_rays=np.concatenate(ref),
                alt_rays=np.concatenate(alt))


SPHERE_XFORMS = [W.transform(scale=(1.5, 0.5, 0.75), rotate=((1, 2, 3), 40), translate=(0.5, -0.25, 1.0)),
                 W.transform(translate=(-3.0, 0.5, 0.25))]


def sphere_case():
    """Two builtin spheres: non-uniform scale with rotation, and a pure translation.  Origins at the
    centre, inside, on the surface (outward and inward), a few radii and 10^4 radii away; grazing rays
    offset by +-1e-3 radii from tangency (exactly tangent rays are left out); zero direction components."""
    w = _world()
    sph = w.add_builtin("sphere")
    mat = w.add_material(W.diffuse(0.5))
    for m in SPHERE_XFORMS:
        w.add_instance(sph, mat, m)
    desc = w.desc()
    mats = [np.asarray(list(desc.instances[i].to_world), F32).astype(F64).reshape(3, 4) for i in range(2)]
    rng = np.random.default_rng(43)
    rays, tags = [], []

    def add(o, d, tag):
        r = _rays8(o, d)
        rays.append(r)
        tags.extend([f"{tag}:{pid}"] * len(r))  # pid: the sphere (primitive id) the ray is aimed at

    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (-0.0, 1, -0.0), (0, 0.6, -0.8),
                     (-0.8, -0.0, 0.6), (0.6, 0.8, 0)], F64)
    for pid, m in enumerate(mats):
        A, c = m[:, :3], m[:, 3]
        u = rng.normal(size=(40, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        dirs = rng.normal(size=(40, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        add([c], _unit32(dirs), "centre")
        add([c], axes, "centre_axis")
        add(c + (0.6 * u) @ A.T, _unit32(dirs), "inside")
        add(c + (0.6 * u[:10]) @ A.T, axes, "inside_axis")
        # on the surface: along the outward normal (A^-T u) a miss, against it a hit of the far side
        nrm = u @ np.linalg.inv(A)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        add(c + u @ A.T, _unit32(nrm), "surface_out")
        add(c + u @ A.T, _unit32(-nrm), "surface_in")
        # from 4 and from 10^4 object-space radii away, aimed at points within 0.9 radii of the centre
        for dist, tag in ((4.0, "near"), (1e4, "far")):
            o = c + (dist * u) @ A.T
            tgt = c + (0.9 * rng.uniform(-1, 1, (40, 1)) * np.roll(u, 7, 0)) @ A.T
            add(o, _unit32(tgt - o.astype(F32).astype(F64)), tag)
        # grazing: in object space from p = 4 u towards the point (1 +- 1e-3) w, w a unit vector
        # perpendicular to u, offset so the ray through it is tangent to the sphere of that radius
        wv = np.cross(u, np.roll(u, 3, 0))
        wv /= np.linalg.norm(wv, axis=1, keepdims=True)
        for rad, tag in ((1.0 - 1e-3, "graze_hit"), (1.0 + 1e-3, "graze_miss")):
            # tangent point from distance 4 on the sphere of radius rad, in the plane of u and wv
            ca = rad / 4.0
            tp = rad * (ca * u + np.sqrt(1 - ca * ca) * wv)
            o = c + (4.0 * u) @ A.T
            tgt = c + tp @ A.T
            add(o, _unit32(tgt - o.astype(F32).astype(F64)), tag)
        add([c - np.array([6.0, 0.0, 0.0])], [(1.0, 0.0, -0.0)], "axis_through")
    tris = np.zeros((0, 3, 3))
    return Case("sphere", w, np.concatenate(rays), tags, tris, spheres=[(0, mats[0]), (1, mats[1])])


INSTANCE_XFORMS = [None,
                   # an exact 90 degree rotation about y, then a translation
                   np.array([[0, 0, 1, 4.0], [0, 1, 0, 0.5], [-1, 0, 0, 0.25], [0, 0, 0, 1]], F32),
                   # a non-uniform scale (2, 0.5, 1), then a translation
                   np.array([[2, 0, 0, -5.0], [0, 0.5, 0, -0.25], [0, 0, 1, 0.5], [0, 0, 0, 1]], F32)]


def instanced_case():
    """The lattice mesh instanced 3 times (identity; an exact 90 degree rotation about y with a
    translation; the scale (2, 0.5, 1) with a translation) and the axis family's rays carried into world
    space by each instance's matrix (axis rays stay axis rays; directions are renormalised exactly)."""
    pos, idx = lattice_mesh()
    w, tris = _mesh_world(pos, idx, INSTANCE_XFORMS)
    rays0, tags0, exact0 = axis_rays()
    rays, tags, exact = [], [], []
    for k, m in enumerate(INSTANCE_XFORMS):
        m4 = np.eye(4) if m is None else m.astype(F64)
        sel = slice(k, None, 3)  # a third of the set for each copy
        r = rays0[sel].astype(F64)
        o = r[:, :3] @ m4[:3, :3].T + m4[:3, 3]
        d = r[:, 3:6] @ m4[:3, :3].T
        two_zero = (r[:, 3:6] == 0).sum(1) == 2
        nrm = np.linalg.norm(d, axis=1, keepdims=True)
        d = np.where(two_zero[:, None], d / nrm, _unit32(d).astype(F64))  # +-1 and +-0 stay exact
        rays.append(_rays8(o, d))
        tags += [f"inst{k}:{t}" for t in np.asarray(tags0)[sel]]
        exact += list(exact0[sel])
    return Case("instanced", w, np.concatenate(rays), tags, tris, exact=exact)


def single_case():
    """n = 1: one ray through a lattice vertex shared by six triangles."""
    pos, idx = lattice_mesh()
    w, tris = _mesh_world(pos, idx)
    return Case("single", w, _rays8([(-0.5, 0.25, 0.0)], [_unit32((1, 1, 1))]), ["vertex"], tris)


_BUILDERS = {"axis": axis_case, "exact_edge": exact_edge_case, "no_leak": no_leak_case, "window": window_case,
             "sphere": sphere_case, "instanced": instanced_case, "single": single_case}
_CACHE = {}


def case(name):
    """The family's Case, built once per process and left unchanged."""
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name]()
    return _CACHE[name]


# ------------------------------------------------------------------ float64 references
def mt_reference(o, d, win, tris, chunk=512):
    """float64 Moller-Trumbore of rays o, d (n, 3), windows win (n, 2), against every triangle
    (m, 3, 3): t (n, m) with inf outside the tied set (|det| > 0, barycentrics >= -BARY_EPS,
    tmin <= t <= tmax), the weights u, v of vertices 1 and 2, and the strict-set mask."""
    n, m = len(o), len(tris)
    T = np.full((n, m), np.inf)
    U, V, S = np.zeros((n, m)), np.zeros((n, m)), np.zeros((n, m), bool)
    if m == 0:
        return T, U, V, S
    v0 = tris[:, 0]
    e1, e2 = tris[:, 1] - v0, tris[:, 2] - v0
    for a in range(0, n, chunk):
        oo, dd, ww = o[a:a + chunk, None, :], d[a:a + chunk, None, :], win[a:a + chunk]
        p = np.cross(dd, e2[None])
        det = (e1[None] * p).sum(-1)
        ok = np.abs(det) > 1e-14
        inv = 1.0 / np.where(ok, det, 1.0)
        s = oo - v0[None]
        u = (s * p).sum(-1) * inv
        q = np.cross(s, e1[None])
        v = (q * dd).sum(-1) * inv
        t = (q * e2[None]).sum(-1) * inv
        b = np.minimum(np.minimum(u, v), 1.0 - u - v)
        inwin = ok & (t >= ww[:, :1]) & (t <= ww[:, 1:])
        T[a:a + chunk] = np.where(inwin & (b >= -BARY_EPS), t, np.inf)
        U[a:a + chunk], V[a:a + chunk] = u, v
        S[a:a + chunk] = inwin & (b >= BARY_EPS)
    return T, U, V, S


def sphere_reference(o, d, win, m34):
    """The nearest root inside the window of |M^-1 (o + t d)| = 1, float64 (inf: none)."""
    m4 = np.eye(4)
    m4[:3] = m34
    inv = np.linalg.inv(m4)
    f = o @ inv[:3, :3].T + inv[:3, 3]
    od = d @ inv[:3, :3].T
    a = (od * od).sum(1)
    b = (f * od).sum(1)
    c = (f * f).sum(1) - 1.0
    disc = b * b - a * c
    real = disc >= 0
    sq = np.sqrt(np.where(real, disc, 0.0))
    q = -(b + np.where(b >= 0, 1.0, -1.0) * sq)
    with np.errstate(divide="ignore", invalid="ignore"):
        r0, r1 = q / a, np.where(q != 0, c / q, np.inf)
    roots = np.stack([np.minimum(r0, r1), np.maximum(r0, r1)], 1)
    ok = real[:, None] & (roots >= win[:, :1]) & (roots <= win[:, 1:])
    return np.where(ok, roots, np.inf).min(1)


class Reference:
    """Per ray and primitive id: the float64 hit distance (inf outside the tied set), the
    barycentrics and the strict-set mask."""

    def __init__(self, cs, rays):
        r = rays.astype(F64)
        o, d, win = r[:, :3], r[:, 3:6], r[:, 6:8]
        nprim = len(cs.tris) + len(cs.spheres)
        self.T = np.full((len(r), nprim), np.inf)
        self.U, self.V = np.zeros_like(self.T), np.zeros_like(self.T)
        self.S = np.zeros(self.T.shape, bool)
        sph = {pid for pid, _ in cs.spheres}
        tri_ids = np.array([i for i in range(nprim) if i not in sph], np.int64)
        assert len(tri_ids) == len(cs.tris)
        if len(tri_ids):
            self.T[:, tri_ids], self.U[:, tri_ids], self.V[:, tri_ids], self.S[:, tri_ids] = mt_reference(o, d, win, cs.tris)
        for pid, m34 in cs.spheres:
            self.T[:, pid] = sphere_reference(o, d, win, m34)
            self.S[:, pid] = np.isfinite(self.T[:, pid])
        self.hit = np.isfinite(self.T).any(1)
        self.tmin = self.T.min(1)


_REFS = {}


def reference(name, alt=False):
    key = (name, alt)
    if key not in _REFS:
        cs = case(name)
        _REFS[key] = Reference(cs, cs.alt_rays if alt else cs.ref_rays)
    return _REFS[key]


def _ok_closest(cs, ref, got):
    """Per ray: does the closest-hit answer `got` (n, 4) satisfy the float64 reference?  Also a
    reason code per ray (0 = fine)."""
    n = len(got)
    ids = got[:, 3].view(np.uint32).astype(np.int64)
    got_hit = ids != MISS
    why = np.zeros(n, np.int32)
    why[got_hit != ref.hit] = 1                                    # hit / miss
    why[(why == 0) & ~got_hit & (got[:, 0] != -1.0)] = 2           # a miss reports t = -1
    h = np.flatnonzero((why == 0) & got_hit)
    if len(h) == 0:
        return why == 0, why
    bad_id = ids[h] >= ref.T.shape[1]
    why[h[bad_id]] = 3
    h = h[~bad_id]
    p = ids[h]
    t, tref = got[h, 0].astype(F64), ref.tmin[h]
    tol = T_ATOL + T_RTOL * np.abs(tref)
    why[h[np.abs(t - tref) > tol]] = 4                             # the distance of the closest hit
    tp = ref.T[h, p]
    why[h[(why[h] == 0) & ~(np.abs(tp - tref) <= tol)]] = 5        # the primitive is in the tied set, at that distance
    bad_b = (np.abs(got[h, 1] - ref.U[h, p]) > B_ATOL) | (np.abs(got[h, 2] - ref.V[h, p]) > B_ATOL)
    why[h[(why[h] == 0) & bad_b]] = 6                              # its barycentrics
    cand = np.abs(ref.T[h] - tref[:, None]) <= tol[:, None]
    strict = cand & ref.S[h]
    one = strict.sum(1) == 1
    why[h[(why[h] == 0) & one & (strict.argmax(1) != p)]] = 7      # a single strict member is the answer
    # exact arithmetic: float64 ties are float32 ties, and the lowest id of the tie wins
    ex = cs.exact[h]
    low = (ref.T[h] == tref[:, None]).argmax(1)
    why[h[(why[h] == 0) & ex & ((low != p) | (t != tref))]] = 8
    return why == 0, why


WHY = {1: "hit / miss", 2: "t of a miss", 3: "primitive id out of range", 4: "t", 5: "primitive outside the tied set",
       6: "barycentrics", 7: "primitive (single strict member)", 8: "exact ray: lowest id of the tie, exact t"}


def check_closest(name, got):
    """Assert the closest-hit answers of family `name` against float64; returns the number of rays
    that took the documented alternative of an "equal" window."""
    cs = case(name)
    got = np.ascontiguousarray(got, F32)
    ok, why = _ok_closest(cs, reference(name), got)
    took_alt = 0
    if cs.alt_rays is not None:
        eq = cs.tags == "equal"
        ok2, _ = _ok_closest(cs, reference(name, alt=True), got)
        took_alt = int((~ok & ok2 & eq).sum())
        ok = ok | (ok2 & eq)
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, (f"{name}: {len(bad)} of {cs.n} rays differ from float64: " +
                           "; ".join(f"ray {i} [{cs.tags[i]}] {WHY[int(why[i])]} got {got[i, :3]} id {got[i, 3:].view(np.uint32)[0]}"
                                     f" ref t {reference(name).tmin[i]}" for i in bad[:6]) +
                           f" | by reason {dict(zip(*np.unique(why[bad], return_counts=True)))}")
    return took_alt


def check_any(name, occ):
    """Assert the any-hit answers (column 0: 1 / -1) of family `name` against float64."""
    cs = case(name)
    got = np.asarray(occ)[:, 0] > 0
    ok = got == reference(name).hit
    if cs.alt_rays is not None:
        ok = ok | ((got == reference(name, alt=True).hit) & (cs.tags == "equal"))
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, f"{name}: any-hit of {len(bad)} rays differs from float64, e.g. ray {bad[0]} [{cs.tags[bad[0]]}]"
