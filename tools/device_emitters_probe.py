#!/usr/bin/env python3
"""Cost of keeping the area-emitter table current under a deforming emissive mesh.

  python tools/device_emitters_probe.py [--n 257] [--reps 20]

Scene: an n x n-vertex grid (n = 257: 131,072 triangles) made emissive over a floor, a constant
env, 960 x 540.  Every timed call moves every vertex (the grid alternates between two reliefs).
Three rows, each warm, the median of --reps, the host's clock around the call (the calls are
synchronous: the time is what a caller waits for):
  (a) host      World.set_mesh_vertices + PTPass.update_shape with the mode off: the host derives
                the emitters (pupil_world_get_desc) and the engine uploads them
                (pupil_pt_update_emitters), after the refit
  (b) device    PTPass.update_shape_device with device_emitters on: refit + rebuild on the device
  (c) rebuild   pupil_pt_refresh_emitters alone (its own last_ms)
and, for (a) and (b), the part that is the refit (build_ms, the vertex update's own clock).
One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=257)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    from pupiloptixlab_amd import World
    from pupiloptixlab_amd import world as W
    from pupiloptixlab_amd.pt_pass import PTPass

    n = args.n
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n), np.linspace(0.0, 1.0, n), indexing="ij")
    x, y = 2.0 * u - 1.0, 2.0 * v - 1.0
    relief = [0.15 * np.cos(2.3 * x + 0.4) * np.sin(1.7 * y - 0.2), 0.4 * np.sin(2.5 * x) * np.cos(1.5 * y)]
    pos = [np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32) for z in relief]
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
    idx = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3).astype(np.uint32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (n * n, 1))
    w = World()
    grid = w.add_mesh(pos[0], idx, nrm, np.stack([u, v], -1).reshape(-1, 2).astype(np.float32))
    m = w.add_material(W.twosided(W.diffuse((0.7, 0.4, 0.3))))
    w.add_instance(grid, m, W.transform(scale=(2.0, 1.5, 1.0), rotate=((1, 0, 0), -60), translate=(0.0, 0.3, 0.0)),
                   emitter_radiance=(4.0, 3.0, 2.0))
    w.add_instance(w.add_builtin("rectangle"), w.add_material(W.twosided(W.diffuse((0.6, 0.6, 0.55)))),
                   W.transform(scale=(6, 6, 1), rotate=((1, 0, 0), -90), translate=(0.0, -2.2, 0.0)))
    w.add_const_env((0.8, 0.9, 1.0))
    w.set_film(960, 540, 4)
    w.set_sensor(45.0, W.look_at_mitsuba((0.5, 1.5, -7.0), (0.0, 0.2, 0.0), (0, 1, 0)))
    pt = PTPass(device=0)
    pt.set_scene(w)
    dev = [torch.from_numpy(p).to(pt.device) for p in pos]
    torch.cuda.synchronize()
    out = {"grid": n, "emitters": int(idx.shape[0]), "reps": args.reps, "two_level": pt.stats()["two_level"]}

    def timed(fn):
        ms = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            extra = fn(k + 1)
            ms.append(((time.perf_counter() - t0) * 1e3, extra))
        ms = ms[args.warmup:]
        return ms

    def row(name, ms):
        out[name + "_ms_median"] = statistics.median(t for t, _ in ms)
        out[name + "_ms_min"], out[name + "_ms_max"] = min(t for t, _ in ms), max(t for t, _ in ms)

    def host(k):
        w.set_mesh_vertices(grid, pos[k & 1])
        pt.update_shape(w, grid)
        return pt.stats()["build_ms"]

    ms = timed(host)
    row("host", ms)
    out["host_refit_ms_median"] = statistics.median(e for _, e in ms)

    pt.device_emitters = True
    out["enable_rebuild_ms"] = pt.device_emitters_info()["last_ms"]

    def device(k):
        pt.update_shape_device(grid, dev[k & 1])
        return pt.stats()["build_ms"], pt.device_emitters_info()["last_ms"]

    ms = timed(device)
    row("device", ms)
    out["device_refit_ms_median"] = statistics.median(e[0] for _, e in ms)
    out["device_rebuild_ms_median"] = statistics.median(e[1] for _, e in ms)

    def refresh(_):
        pt.refresh_emitters()
        return pt.device_emitters_info()["last_ms"]

    ms = timed(refresh)
    row("refresh_call", ms)
    out["refresh_last_ms_median"] = statistics.median(e for _, e in ms)
    out["refresh_last_ms_min"], out["refresh_last_ms_max"] = min(e for _, e in ms), max(e for _, e in ms)
    pt.close_engine()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
