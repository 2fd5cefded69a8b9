"""Engine-owned area-emitter table, host side (no GPU): the new entry points exist and refuse a
null engine, the shared GetWeight gives world.cpp the weights it always had, and a float32 numpy
restatement of the rebuild's five stages (pt_emitters.hip) reproduces the host's table bit for bit
from the desc's vertices, indices and instance matrices -- the specification the device kernels
are held to by tests/test_device_emitters.py, pinned here without a GPU.

Also the worlds the GPU tests share."""
import ctypes as C
import functools
import os
import re

import numpy as np

from pupiloptixlab_amd import World, abi
from pupiloptixlab_amd import world as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pupil_pt_enable_device_emitters", "pupil_pt_refresh_emitters", "pupil_pt_device_emitters_info",
       "pupil_debug_read_emitters", "pupil_debug_read_emitter_guide")
f32 = np.float32


# ------------------------------------------------------------------ meshes
@functools.lru_cache(maxsize=None)
def grid_mesh(nx=7, ny=9):
    """nx x ny vertices over [-1, 1]^2 with a gentle relief: (positions, normals, uvs, indices);
    2 (nx - 1) (ny - 1) triangles"""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, nx), np.linspace(0.0, 1.0, ny), indexing="ij")
    x, y = 2.0 * u - 1.0, 2.0 * v - 1.0
    z = 0.15 * np.cos(2.3 * x + 0.4) * np.sin(1.7 * y - 0.2)
    pos = np.stack([x, y, z], -1).reshape(-1, 3).astype(f32)
    uv = np.stack([u, v], -1).reshape(-1, 2).astype(f32)
    vid = lambda i, j: i * ny + j
    idx = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            idx += [[vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)], [vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)]]
    idx = np.asarray(idx, np.uint32)
    return pos, vertex_normals(pos, idx), uv, idx


def vertex_normals(p, idx):
    n = np.zeros_like(p, dtype=np.float64)
    f = np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]]).astype(np.float64)
    for k in range(3):
        np.add.at(n, idx[:, k], f)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.maximum(ln, 1e-30), [[0.0, 0.0, 1.0]]).astype(f32)


def bulge(p):
    q = p.copy()
    q[:, 2] = (p[:, 2] + 0.6 * np.sin(2.5 * p[:, 0]) * np.cos(1.5 * p[:, 1])).astype(f32)
    return q


def squeeze(p):
    return (p * np.array([0.7, 1.2, -0.5], f32)).astype(f32)


# ------------------------------------------------------------------ worlds
XF_A = {0: dict(scale=(1.3, 0.7, 1.0), rotate=((1, 2, 0), 25), translate=(-1.4, 0.3, 0.2)),
        1: dict(scale=(0.35, 0.35, 0.35), translate=(0.2, 1.3, -0.5)),
        2: dict(scale=(0.5, 1.6, 0.8), rotate=((0, 1, 1), -40), translate=(1.5, 0.1, 0.6)),
        3: dict(scale=(0.4, 0.3, 1.0), rotate=((1, 0, 0), 90), translate=(0.0, 2.2, 0.0))}
# case 4's rigid move of one grid instance and the sphere
XF_MOVED = {0: dict(scale=(1.1, 0.9, 1.2), rotate=((0, 1, 3), -35), translate=(-1.1, 0.6, -0.3)),
            1: dict(scale=(0.5, 0.5, 0.5), translate=(0.4, 1.0, 0.1))}


def _finish(w, env=True, film=(64, 48, 4)):
    if env:
        w.add_const_env((0.8, 0.9, 1.0))
    w.set_film(*film)
    w.set_sensor(45.0, W.look_at_mitsuba((0.5, 1.5, -7.0), (0.0, 0.2, 0.0), (0, 1, 0)))
    return w


def _floor(w, rect):
    m = w.add_material(W.twosided(W.diffuse((0.6, 0.6, 0.55))))
    w.add_instance(rect, m, W.transform(scale=(6, 6, 1), rotate=((1, 0, 0), -90), translate=(0.0, -2.2, 0.0)))


def world_a(pos=None, nrm=None, xf=None, rect_emissive=True):
    """World A, 195 area emitters: instance 0 the grid (shape 0, 96 emitters), 1 a sphere (1),
    2 the grid again (96), 3 a rectangle (2), 4 the floor; a constant env.  The emitter ranges
    start at 0, 96, 97 and 193: no boundary on a multiple of 64."""
    p0, n0, uv, idx = grid_mesh()
    pos = p0 if pos is None else pos
    nrm = n0 if nrm is None else nrm
    t = dict(XF_A)
    t.update(xf or {})
    w = World()
    grid = w.add_mesh(pos, idx, nrm, uv)
    sphere, rect = w.add_builtin("sphere"), w.add_builtin("rectangle")
    m = w.add_material(W.twosided(W.diffuse((0.7, 0.4, 0.3))))
    w.add_instance(grid, m, W.transform(**t[0]), emitter_radiance=(12.0, 9.0, 6.0))
    w.add_instance(sphere, m, W.transform(**t[1]), emitter_radiance=(3.0, 3.0, 2.5))
    w.add_instance(grid, m, W.transform(**t[2]), emitter_radiance=(0.9, 0.7, 0.4))
    w.add_instance(rect, m, W.transform(**t[3]), emitter_radiance=(6.0, 6.0, 6.0) if rect_emissive else None)
    _floor(w, rect)
    return _finish(w)


def one_emitter_world(pos=None):
    """exactly one emitter (no env): one emissive triangle (shape 0, with normals) over the floor"""
    pos = ONE_TRI if pos is None else pos
    w = World()
    s = w.add_mesh(pos, np.array([[0, 1, 2]], np.uint32), np.tile(np.array([[0, 0, 1]], f32), (3, 1)))
    m = w.add_material(W.twosided(W.diffuse((0.7, 0.4, 0.3))))
    w.add_instance(s, m, W.transform(rotate=((1, 0, 0), 30), translate=(0.0, 0.5, 0.0)), emitter_radiance=(5.0, 4.0, 3.0))
    _floor(w, w.add_builtin("rectangle"))
    return _finish(w, env=False)


ONE_TRI = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0.2]], f32)


def big_world(pos=None, nrm=None):
    """4,098 emitters: a 65 x 33 grid (4,096 triangles) and the rectangle"""
    p0, n0, uv, idx = grid_mesh(65, 33)
    w = World()
    s = w.add_mesh(p0 if pos is None else pos, idx, n0 if nrm is None else nrm, uv)
    rect = w.add_builtin("rectangle")
    m = w.add_material(W.twosided(W.diffuse((0.7, 0.4, 0.3))))
    w.add_instance(s, m, W.transform(**XF_A[0]), emitter_radiance=(2.0, 3.0, 1.0))
    w.add_instance(rect, m, W.transform(**XF_A[3]), emitter_radiance=(6.0, 6.0, 6.0))
    _floor(w, rect)
    return _finish(w)


def no_normals_world(pos=None):
    """the 7 x 9 grid without normals or uvs, emissive, and an emissive sphere"""
    p0, _, _, idx = grid_mesh()
    w = World()
    s = w.add_mesh(p0 if pos is None else pos, idx)
    m = w.add_material(W.twosided(W.diffuse((0.7, 0.4, 0.3))))
    w.add_instance(s, m, W.transform(**XF_A[2]), emitter_radiance=(4.0, 1.0, 2.0))
    w.add_instance(w.add_builtin("sphere"), m, W.transform(**XF_A[1]), emitter_radiance=(3.0, 3.0, 2.5))
    _floor(w, w.add_builtin("rectangle"))
    return _finish(w)


# ------------------------------------------------------------------ the desc as numpy
def desc_table(desc):
    """the host's table: select_probability, area, weight (n,), pos, nrm (n, 3, 3)"""
    n = desc.num_area_emitters
    e = [desc.area_emitters[i] for i in range(n)]
    g = lambda name: np.array([getattr(x, name) for x in e], f32)
    return {"select_probability": g("select_probability"), "area": g("area"), "weight": g("weight"),
            "type": np.array([x.type for x in e], np.uint32), "center": np.array([list(x.center) for x in e], f32),
            "radius": g("radius"),
            "pos": np.array([[list(r) for r in x.pos] for x in e], f32).reshape(n, 3, 3),
            "nrm": np.array([[list(r) for r in x.nrm] for x in e], f32).reshape(n, 3, 3)}


def host_cdf_and_guide(sp, binary=False):
    """host/emitter_tables.h emitter_tables: the sequential CDF, guide_bits and the guide's linear walk"""
    cdf = np.zeros(len(sp), f32)
    s = f32(0.0)
    for i, p in enumerate(sp):
        s = f32(s + p)
        cdf[i] = s
    bits = 0
    while (1 << bits) < len(sp) and bits < 20:
        bits += 1
    guide = None
    if len(sp) > 1 and not binary:
        m = 1 << bits
        guide = np.zeros(m + 1, np.uint32)
        i = 0
        for k in range(m + 1):
            t = f32(k) / f32(m)
            while i < len(cdf) and cdf[i] < t:
                i += 1
            guide[k] = i
    return cdf, bits, guide


def select_weight(t):
    """GetWeight (world/emitter.cpp:73-101) of an abi.Texture in float32, the bitmap walk bug for bug"""
    mx = lambda c: f32(max(f32(c[0]), f32(c[1]), f32(c[2])))
    if t.type == abi.TEX_RGB:
        return mx(t.c0)
    if t.type == abi.TEX_CHECKERBOARD:
        return f32(f32(mx(t.c0) + mx(t.c1)) * f32(0.5))
    texels = np.ctypeslib.as_array(t.rgba, (t.width * t.height * 4,))
    w = f32(0.0)
    for i in range(t.width):
        for j in range(t.height):
            k = (i * t.width + j) * 4
            if k + 2 < texels.size:
                w = f32(w + mx(texels[k:k + 3]))
    return f32(w / f32(f32(f32(1.0) * f32(t.width)) * f32(t.height)))


# ------------------------------------------------------------------ the five stages in float32
def _point(m, p):
    """TransformPoint by a 3x4 whose fourth row is 0 0 0 1, w computed and divided by"""
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    x = m[0] * px + m[1] * py + m[2] * pz + m[3]
    y = m[4] * px + m[5] * py + m[6] * pz + m[7]
    z = m[8] * px + m[9] * py + m[10] * pz + m[11]
    w = f32(0) * px + f32(0) * py + f32(0) * pz + f32(1)
    return np.stack([x / w, y / w, z / w], -1)


def _normal(o, n):
    """TransformNormal by the transpose of to_object's 3x3"""
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    x = o[0] * nx + o[4] * ny + o[8] * nz
    y = o[1] * nx + o[5] * ny + o[9] * nz
    z = o[2] * nx + o[6] * ny + o[10] * nz
    ln = np.sqrt(x * x + y * y + z * z)
    return np.stack([x / ln, y / ln, z / ln], -1)


def restate(desc, reduce="chain"):
    """The rebuild from what the engine holds: per emissive instance its shape's vertices, indices
    and normals, to_world / to_object and the select weight of its radiance.  reduce = 'tree' sums
    the weights pairwise instead of in order (the sensitivity check)."""
    n = desc.num_area_emitters
    out = {"pos": np.zeros((n, 3, 3), f32), "nrm": np.zeros((n, 3, 3), f32), "area": np.zeros(n, f32),
           "center": np.zeros((n, 3), f32), "radius": np.zeros(n, f32)}
    weight = np.zeros(n, f32)
    for i in range(desc.num_instances):
        ins = desc.instances[i]
        if ins.emitter_offset < 0:
            continue
        e0 = ins.emitter_offset
        sw = select_weight(desc.area_emitters[e0].radiance)
        tw, to = np.array(list(ins.to_world), f32), np.array(list(ins.to_object), f32)
        sh = desc.shapes[ins.shape]
        if sh.kind == abi.SHAPE_SPHERE:
            o = _point(tw, np.zeros((1, 3), f32))[0]
            p = _point(tw, np.array([[1, 0, 0]], f32))[0]
            d = o - p
            r = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            out["center"][e0], out["radius"][e0] = o, r
            out["area"][e0] = f32(4.0) * f32(3.14159265358979323846) * r * r
            weight[e0] = sw * out["area"][e0]
            continue
        nf = sh.num_faces
        pos = np.ctypeslib.as_array(sh.positions, (sh.num_vertices, 3))
        idx = np.ctypeslib.as_array(sh.indices, (nf, 3))
        nrm = (np.ctypeslib.as_array(sh.normals, (sh.num_vertices, 3)) if sh.normals
               else np.tile(np.array([[0, 0, 1]], f32), (sh.num_vertices, 1)))
        p = np.stack([_point(tw, pos[idx[:, v]]) for v in range(3)], 1)
        out["pos"][e0:e0 + nf] = p
        out["nrm"][e0:e0 + nf] = np.stack([_normal(to, nrm[idx[:, v]]) for v in range(3)], 1)
        v1, v2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        cx = v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1]
        cy = v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2]
        cz = v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]
        area = np.sqrt(cx * cx + cy * cy + cz * cz) * f32(0.5)
        out["area"][e0:e0 + nf] = area
        weight[e0:e0 + nf] = sw * area
    assert weight.dtype == f32 and out["pos"].dtype == f32
    if reduce == "chain":
        total = np.cumsum(weight, dtype=f32)[-1]
    else:
        t = weight.copy()
        while len(t) > 1:
            if len(t) & 1:
                t = np.append(t, f32(0))
            t = t[0::2] + t[1::2]
        total = t[0]
    emitter_num = n + (1 if desc.env else 0)
    sp = weight / total * f32(n)
    sp = sp / f32(emitter_num)
    out["weight"], out["select_probability"] = weight, sp
    out["cdf"] = np.cumsum(sp, dtype=f32)
    bits = 0
    while (1 << bits) < n and bits < 20:
        bits += 1
    m = 1 << bits
    out["guide_bits"] = bits
    out["guide"] = np.searchsorted(out["cdf"], np.arange(m + 1, dtype=f32) / f32(m), side="left").astype(np.uint32)
    return out


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------ tests
def test_new_entries_are_exported_declared_bound_and_refuse_a_null_engine():
    lib = abi.load_library()
    header = open(os.path.join(ROOT, "include", "pupil_pt.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    w = world_a()
    desc = w.desc()
    out = np.zeros(24, f32)
    cnt = C.c_uint32(0)
    assert lib.pupil_pt_enable_device_emitters(None, C.byref(desc)) == abi.ERR_INVALID
    assert lib.pupil_pt_enable_device_emitters(None, None) == abi.ERR_INVALID
    assert lib.pupil_pt_refresh_emitters(None) == abi.ERR_INVALID
    assert lib.pupil_pt_device_emitters_info(None, None, None, None) == abi.ERR_INVALID
    assert lib.pupil_debug_read_emitters(None, 0, 1, out.ctypes.data_as(abi.f32p)) == abi.ERR_INVALID
    assert lib.pupil_debug_read_emitter_guide(None, None, None, C.byref(cnt)) == abi.ERR_INVALID
    assert lib.pupil_abi_version() == 7  # no ABI bump: the feature is detected by symbol


def test_world_a_is_the_world_the_issue_describes():
    desc = world_a().desc()
    assert desc.num_area_emitters == 195
    assert [desc.instances[i].emitter_offset for i in range(desc.num_instances)] == [0, 96, 97, 193, -1]
    w = desc_table(desc)["weight"]
    assert w.min() > 0 and w.max() / w.min() > 10.0  # the weights span more than a decade


def test_shared_get_weight_gives_every_emitter_its_weight():
    """weight = select_weight * area bit for bit, select_weight recomputed here from the texture:
    RGB, checkerboard and a 3 x 2 bitmap (whose walk visits texels 0, 1, 3, 4 and skips two)."""
    texels = np.ascontiguousarray(np.random.default_rng(5).uniform(0.1, 4.0, (2, 3, 4)), f32)
    bitmap = abi.Texture()
    bitmap.type = abi.TEX_BITMAP
    bitmap.width, bitmap.height = 3, 2
    bitmap.transform[:] = W.identity4().reshape(-1)
    bitmap.rgba = texels.ctypes.data_as(abi.f32p)
    for rad in (W.rgb(0.3, 2.5, 1.1), W.checkerboard((0.2, 0.9, 0.4), (3.0, 1.0, 2.0), (4.0, 4.0)), bitmap):
        w = World()
        m = w.add_material(W.diffuse((0.5, 0.5, 0.5)))
        w.add_instance(w.add_builtin("rectangle"), m, W.transform(**XF_A[0]), emitter_radiance=rad)
        w.add_instance(w.add_builtin("sphere"), m, W.transform(**XF_A[1]), emitter_radiance=rad)
        desc = _finish(w).desc()
        assert desc.num_area_emitters == 3
        sw = select_weight(desc.area_emitters[0].radiance)
        assert sw > 0 and sw == select_weight(rad)
        t = desc_table(desc)
        assert np.array_equal(_bits(t["weight"]), _bits(sw * t["area"])), rad.type


def test_float32_restatement_of_the_five_stages_reproduces_the_host_table():
    desc = world_a(bulge(grid_mesh()[0])).desc()
    host, got = desc_table(desc), restate(desc)
    for k in ("pos", "nrm", "area", "weight", "select_probability", "center", "radius"):
        assert np.array_equal(_bits(got[k]), _bits(host[k])), k
    cdf, bits, guide = host_cdf_and_guide(host["select_probability"])
    assert bits == got["guide_bits"] == 8 and len(guide) == 257
    assert np.array_equal(_bits(got["cdf"]), _bits(cdf))
    assert np.all(np.diff(cdf) >= 0)  # the precondition of the lower-bound search
    assert np.array_equal(got["guide"], guide)  # lower bound per k == the host's linear walk
    # the comparison is sensitive to the order of the weight sum: a pairwise (tree) sum of the
    # same weights changes select_probability bits on this world
    tree = restate(desc, reduce="tree")
    assert np.array_equal(_bits(tree["weight"]), _bits(host["weight"]))
    assert not np.array_equal(_bits(tree["select_probability"]), _bits(host["select_probability"]))


def test_restatement_on_the_edge_worlds():
    """one emitter, 4,098 emitters, no normals: the same restatement holds"""
    for w in (one_emitter_world(), big_world(), no_normals_world(bulge(grid_mesh()[0]))):
        desc = w.desc()
        host, got = desc_table(desc), restate(desc)
        for k in ("pos", "nrm", "area", "select_probability"):
            assert np.array_equal(_bits(got[k]), _bits(host[k])), (desc.num_area_emitters, k)
        cdf, _, guide = host_cdf_and_guide(host["select_probability"])
        assert np.array_equal(_bits(got["cdf"]), _bits(cdf))
        if guide is not None:
            assert np.array_equal(got["guide"], guide)
