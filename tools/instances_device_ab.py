#!/usr/bin/env python3
"""Cost of moving many instances whose transforms live on the device: the device entry against
the host path it spares.

  python tools/instances_device_ab.py [--instances 4096] [--reps 20] [--warmup 3] [--config5 1]

Scene A: --instances instances of one small mesh (a 13 x 13 grid, 288 triangles) over a floor, in
the two-level world mode (PUPIL_ACCEL=two_level), every instance moved every step by a new random
rigid transform with a non-uniform scale, produced as a float32 tensor on the device.
Scene B (--config5): the 40-instance config 5 field (250k triangles per instance), the same way.
Per scene the two paths alternate in one process after --warmup rounds; every figure is the host's
clock around calls that return once the structure is updated, in ms, median and min - max:
  device       PTPass.update_instances_device(tensor): the engine inverts and refits on the device
  host         the same move as a caller had to make it before: tensor.cpu(), the world's own
               inversion (World.set_instance_transform + desc), PTPass.update_instances
  host_call    of that, the engine's pupil_pt_update_instances_masked alone
Both paths' kernel launches and synchronisations per call come from the engine's own counters
(pupil_debug_update_counts).  After the last round the two paths' instance tables are compared.
One JSON line per scene after the tables."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def grid(nx, ny):
    import numpy as np

    u, v = np.meshgrid(np.linspace(-1.0, 1.0, nx), np.linspace(-1.0, 1.0, ny), indexing="ij")
    pos = np.stack([u, v, 0.2 * np.cos(2.0 * u) * np.sin(1.5 * v)], -1).reshape(-1, 3).astype(np.float32)
    idx = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            a = i * ny + j
            idx += [[a, a + ny, a + ny + 1], [a, a + ny + 1, a + 1]]
    return pos, np.asarray(idx, np.uint32)


def random_transforms(rng, n, spread):
    """(n, 4, 4) float32: scale, rotation about a random axis, translation"""
    import numpy as np

    from pupiloptixlab_amd import world as W

    out = np.zeros((n, 4, 4), np.float32)
    for k in range(n):
        out[k] = W.transform(scale=tuple(rng.uniform(0.05, 0.15, 3)), rotate=(tuple(rng.normal(size=3)),
                             float(rng.uniform(0.0, 360.0))), translate=tuple(rng.uniform(-spread, spread, 3)))
    return out


def counts(pt):
    la, sy = C.c_uint32(0), C.c_uint32(0)
    pt._lib.pupil_debug_update_counts(pt._pt, C.byref(la), C.byref(sy))
    return la.value, sy.value


def run(name, world, movers, sets, reps, warmup):
    import numpy as np
    import torch

    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(world)
    pt.render(1)
    torch.cuda.synchronize()
    ids = torch.arange(len(movers), dtype=torch.int32, device=pt.device) + int(movers[0])
    dev = [torch.from_numpy(np.ascontiguousarray(s.reshape(-1, 16)[:, :12])).to(pt.device) for s in sets]
    dev16 = [torch.from_numpy(s).to(pt.device) for s in sets]
    torch.cuda.synchronize()
    rows = {"device": [], "host": [], "host_call": []}
    got = {}
    tables = {}
    for k in range(warmup + reps):
        tw, full = dev[k % 2], dev16[k % 2]
        # the device entry
        t0 = time.perf_counter()
        pt.update_instances_device(tw, ids)
        a = (time.perf_counter() - t0) * 1e3
        got["device"] = counts(pt)
        tables["device"] = pt.instance_transforms()
        # the host path: the tensor comes to the host, the world inverts, the host entry uploads
        real = pt._lib.pupil_pt_update_instances_masked
        inner = []

        def timed(*args):
            t = time.perf_counter()
            rc = real(*args)
            inner.append((time.perf_counter() - t) * 1e3)
            return rc

        t0 = time.perf_counter()
        m = full.cpu().numpy()
        for i, x in zip(movers, m):
            world.set_instance_transform(int(i), x)
        pt._lib.pupil_pt_update_instances_masked = timed
        try:
            pt.update_instances(world, movers)
        finally:
            pt._lib.pupil_pt_update_instances_masked = real
        b = (time.perf_counter() - t0) * 1e3
        got["host"] = counts(pt)
        tables["host"] = pt.instance_transforms()
        if k >= warmup:
            rows["device"].append(a)
            rows["host"].append(b)
            rows["host_call"].append(inner[0])
    same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(tables["device"], tables["host"]))
    pt.close_engine()
    print(f"# {name}: {len(movers)} instances moved per call, {reps} alternated rounds after {warmup} warm-up rounds, ms")
    print(f"{'':12s}{'median':>10s}{'min':>10s}{'max':>10s}{'launches':>10s}{'syncs':>8s}")
    for key, v in rows.items():
        c = got["device" if key == "device" else "host"]
        print(f"{key:12s}{statistics.median(v):10.3f}{min(v):10.3f}{max(v):10.3f}{c[0]:10d}{c[1]:8d}")
    ratio = statistics.median(rows["host"]) / statistics.median(rows["device"])
    print(f"host / device, medians: {ratio:.2f}; instance tables of the two paths bit-identical: {same}")
    print(json.dumps({"scene": name, "moved": len(movers), "reps": reps, "host_over_device": ratio, "tables_identical": same,
                      "launches": {k: v[0] for k, v in got.items()}, "syncs": {k: v[1] for k, v in got.items()},
                      **{k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
                         for k, v in rows.items()}}))
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config5", type=int, default=1)
    args = ap.parse_args()
    os.environ.setdefault("PUPIL_ACCEL", "two_level")

    import numpy as np

    from pupiloptixlab_amd import World, scenes
    from pupiloptixlab_amd import world as W

    rng = np.random.default_rng(5)
    n = args.instances
    w = World()
    pos, idx = grid(13, 13)
    mesh = w.add_mesh(pos, idx)
    rect = w.add_builtin("rectangle")
    mat = w.add_material(W.twosided(W.diffuse((0.6, 0.6, 0.6))))
    sets = [random_transforms(rng, n, 4.0) for _ in range(3)]
    for k in range(n):
        w.add_instance(mesh, mat, sets[2][k])
    w.add_instance(rect, mat, W.transform(scale=(8, 8, 1), rotate=((1, 0, 0), -90), translate=(0.0, -4.5, 0.0)))
    w.add_const_env((0.8, 0.9, 1.0))
    w.set_film(64, 48, 4)
    w.set_sensor(45.0, W.look_at_mitsuba((0.0, 1.0, -14.0), (0.0, 0.0, 0.0), (0, 1, 0)))
    ok = run(f"{n} x 288 triangles", w, list(range(n)), sets[:2], args.reps, args.warmup)
    if args.config5:
        field = scenes.instanced_field(40, 64, 48, 6, seed=2)
        d = field.desc()
        base = np.array([list(d.instances[i].to_world) + [0, 0, 0, 1] for i in range(40)], np.float32).reshape(40, 4, 4)
        moved = base.copy()
        moved[:, :3, 3] += rng.uniform(-0.5, 0.5, (40, 3)).astype(np.float32)
        ok = run("config 5, 40 x 250k triangles", field, list(range(40)), [moved, base], max(5, args.reps // 2),
                 args.warmup) and ok
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
