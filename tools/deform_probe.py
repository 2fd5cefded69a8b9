#!/usr/bin/env python3
"""Cost and trace quality of a vertex update (pupil_pt_update_shape_vertices) on the bench scenes.

  python tools/deform_probe.py --config 4 --what refit      # median of N refits, ms
  python tools/deform_probe.py --config 4 --what rebuild    # the same with PUPIL_VERTS_REBUILD
  python tools/deform_probe.py --config 4 --what quality    # node visits per ray: refit vs rebuild

config 4: the 1 M triangle sphere field, flattened BVH; its mesh data are 8 shapes of 126 k
triangles, so one call deforms ONE of them and refits the whole tree.  config 5: 40 instances of
a 250 k triangle BLAS, two-level world mode (bench.py's defaults).  The largest mesh shape is
deformed from device tensors (update_shape_device), alternating between the bulge
z' = zc + (z - zc) (1 + 0.8 sin(3 (x - xc) / xr)) and the original vertices, so every timed call
moves every vertex of that shape.  The call is synchronous (it returns once the structure is
updated) and part of its work is the host's (reading back the world-mode TLAS entries, the
object-mode TLAS build, launches and the final synchronisation), which device events on the
engine's stream would leave out: the time is the host's around the call, the number a caller
waits for, with the engine's own build_ms counter beside it.
One JSON line per run."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4, choices=(4, 5))
    ap.add_argument("--what", default="refit", choices=("refit", "rebuild", "quality"))
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    args = ap.parse_args()
    if args.config == 5:
        os.environ.setdefault("PUPIL_ACCEL", "two_level")

    import numpy as np
    import torch

    from pupiloptixlab_amd import scenes
    from pupiloptixlab_amd.pt_pass import PTPass

    depth = 4 if args.config == 4 else 6
    if args.config == 5:
        world = scenes.instanced_field(40, args.width, args.height, depth, seed=2, spheres_per_blas=125)
    else:
        world = scenes.sphere_field(500, args.width, args.height, depth, seed=1)
    desc = world.desc()
    shape = max((s for s in range(desc.num_shapes) if desc.shapes[s].kind == 0),
                key=lambda s: desc.shapes[s].num_vertices)
    nv, nf = desc.shapes[shape].num_vertices, desc.shapes[shape].num_faces
    p0 = np.ctypeslib.as_array(desc.shapes[shape].positions, (nv, 3)).copy()
    xc, zc = 0.5 * (p0[:, 0].max() + p0[:, 0].min()), 0.5 * (p0[:, 2].max() + p0[:, 2].min())
    xr = max(1e-6, 0.5 * (p0[:, 0].max() - p0[:, 0].min()))
    p1 = p0.copy()
    p1[:, 2] = zc + (p0[:, 2] - zc) * (1.0 + 0.8 * np.sin(3.0 * (p0[:, 0] - xc) / xr))
    pt = PTPass(device=0)
    pt.set_scene(world)
    dev = [torch.from_numpy(p0).to(pt.device), torch.from_numpy(p1.astype(np.float32)).to(pt.device)]
    torch.cuda.synchronize()
    out = {"config": args.config, "what": args.what, "shape_vertices": nv, "shape_faces": nf,
           "two_level": pt.stats()["two_level"], "create_build_ms": pt.stats()["build_ms"]}

    def update(k, rebuild):
        t0 = time.perf_counter()
        pt.update_shape_device(shape, dev[k & 1], rebuild=rebuild)
        return (time.perf_counter() - t0) * 1e3, pt.stats()["build_ms"]

    if args.what in ("refit", "rebuild"):
        rebuild = args.what == "rebuild"
        for k in range(args.warmup):
            update(k + 1, rebuild)
        ms = [update(k + 1 + args.warmup, rebuild) for k in range(args.n)]
        out["call_ms_median"] = statistics.median(m[0] for m in ms)
        out["call_ms_min"], out["call_ms_max"] = min(m[0] for m in ms), max(m[0] for m in ms)
        out["build_ms_median"] = statistics.median(m[1] for m in ms)
    else:
        def visits():
            pt.mark_dirty()
            pt.render(1, collect_stats=1)
            torch.cuda.synchronize()
            c = pt.stats()
            rays = c["primary_rays"] + c["extension_rays"] + c["shadow_rays"]
            return c["node_visits"] / max(1, rays), c["prim_tests"] / max(1, rays), rays

        out["undeformed"] = visits()
        update(1, False)
        out["bulge_refit"] = visits()
        update(1, True)
        out["bulge_rebuild"] = visits()
        out["fields"] = "node visits per ray, primitive tests per ray, rays"
    pt.close_engine()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
