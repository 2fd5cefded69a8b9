#!/usr/bin/env python3
"""Cost of replacing a mesh by one of new topology in place, against the only alternative there
was before: destroying the engine and creating a new one on the updated world.

  python tools/replace_mesh_timing.py [--spheres 500] [--rounds 3] [--accel flat]

Scene: the benchmark's config-4 field (scenes.sphere_field: 500 spheres of 2,000 triangles merged
into 8 meshes, the room, the lamp; 1 M triangles), film 64 x 48.  Shape 0 is first made a
100 k-face mesh (50 of its spheres), then replaced by a 120 k-face one (60 of them); per round,
after an untimed replacement back to 100 k faces, in this order:
  host      PTPass.replace_shape(numpy arrays)
  device    PTPass.replace_shape_device(tensors already on the device)
  recreate  close_engine + set_scene on the world that holds the 120 k-face mesh
Every figure is the host's clock around a call that returns once the structure is published, in
ms; build_ms is the engine's own counter after it (a replacement: the call's time; a create: the
builder's).  After the last round the three engines' renders are compared bit for bit.  One JSON
line after the table."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sub_mesh(num_spheres, centers, radii):
    import numpy as np

    from pupiloptixlab_amd import scenes

    v, nrm, uv, idx = scenes.uv_sphere()
    pos = np.concatenate([v * r + c for c, r in zip(centers[:num_spheres], radii[:num_spheres])]).astype(np.float32)
    nn = np.concatenate([nrm] * num_spheres).astype(np.float32)
    tt = np.concatenate([uv] * num_spheres).astype(np.float32)
    ii = np.concatenate([idx + k * len(v) for k in range(num_spheres)]).astype(np.uint32)
    return pos, ii, nn, tt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spheres", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--accel", default="flat", choices=("flat", "two_level"))
    args = ap.parse_args()
    os.environ["PUPIL_ACCEL"] = args.accel

    import numpy as np
    import torch

    from pupiloptixlab_amd import scenes
    from pupiloptixlab_amd.pt_pass import PTPass

    world = scenes.sphere_field(args.spheres, 64, 48, 4, seed=1)
    centers, radii, _ = scenes._field_geometry(args.spheres, 1)
    sel = np.nonzero(np.arange(args.spheres) % 8 == 0)[0]  # the spheres of shape 0
    small = sub_mesh(50, centers[sel], radii[sel])
    large = sub_mesh(60, centers[sel], radii[sel])
    faces = {"small": len(small[1]), "large": len(large[1])}

    def image(pt):
        pt.mark_dirty()
        pt.render(1)
        torch.cuda.synchronize()
        return pt.buffers.get("pt accum buffer").cpu().numpy().view(np.uint32)

    pt = PTPass(device=0)
    pt.set_scene(world)
    image(pt)
    dev = [torch.from_numpy(a.astype(np.int32) if a.dtype == np.uint32 else a).to(pt.device) for a in large]
    torch.cuda.synchronize()
    rows = {"host": [], "device": [], "recreate": []}
    build = {"host": [], "device": [], "recreate": []}
    images = {}

    def to_small():
        world.set_mesh(0, *small)
        pt.replace_shape(0, small[0], small[1], small[2], small[3])

    for _ in range(args.rounds):
        to_small()
        t0 = time.perf_counter()
        pt.replace_shape(0, large[0], large[1], large[2], large[3])
        rows["host"].append((time.perf_counter() - t0) * 1e3)
        build["host"].append(pt.stats()["build_ms"])
        images["host"] = image(pt)

        to_small()
        t0 = time.perf_counter()
        pt.replace_shape_device(0, dev[0], dev[1], dev[2], dev[3])
        rows["device"].append((time.perf_counter() - t0) * 1e3)
        build["device"].append(pt.stats()["build_ms"])
        images["device"] = image(pt)

        world.set_mesh(0, *large)
        world.desc()  # the world's own rebuild of its description is not the engine's cost
        t0 = time.perf_counter()
        pt.close_engine()
        pt.set_scene(world)
        rows["recreate"].append((time.perf_counter() - t0) * 1e3)
        build["recreate"].append(pt.stats()["build_ms"])
        images["recreate"] = image(pt)
    prims = pt.stats()["bvh_prims"]
    pt.close_engine()
    same = all(np.array_equal(images[k], images["recreate"]) for k in ("host", "device"))
    print(f"# config-4 field, {prims} primitives, {args.accel}: shape 0 from {faces['small']} to {faces['large']} faces, "
          f"{args.rounds} alternated rounds, ms (host clock around the call; build_ms: the engine's counter)")
    print(f"{'':10s}" + "".join(f"{'round ' + str(k + 1):>12s}" for k in range(args.rounds)) + f"{'build_ms':>12s}")
    for key, v in rows.items():
        print(f"{key:10s}" + "".join(f"{x:12.2f}" for x in v) + f"{min(build[key]):12.2f}")
    print(f"renders of the three engines bit-identical: {same}")
    print(json.dumps({"accel": args.accel, "prims": int(prims), "faces": faces, "rounds": args.rounds,
                      "images_identical": bool(same), "ms": rows, "build_ms": build}))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
