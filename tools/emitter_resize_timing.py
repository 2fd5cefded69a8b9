#!/usr/bin/env python3
"""Cost of resizing the engine-owned emitter table in place (device_emitters on), against the only
route there was before: destroying the engine and creating a new one on the world's description of
the same scene.

  python tools/emitter_resize_timing.py [--spheres 500] [--rounds 5] [--accel flat|two_level]

Scene: the benchmark's config-4 field (scenes.sphere_field: 500 spheres of 2,000 triangles merged
into 8 meshes, the room; 1 M triangles), film 64 x 48, its lamp given a mesh of its own: a flat
grid of 224 x 224 quads, 100,352 emissive faces.  Per round, after one untimed warm-up round:
  (a) replace   the lamp's mesh replaced by 245 x 245 quads (120,050 faces):
        device    PTPass.replace_shape_device(tensors already on the device)
        recreate  close_engine + set_scene on the world that holds the larger mesh
      (before each, untimed: back to the 100 k-face mesh)
  (b) add       a second emissive instance of the 100 k-face mesh:
        entry     pupil_pt_set_instances_emitters alone (bindings and description prepared before)
        pass      PTPass.set_instances: the entry, the bindings and the world's description,
                  which derives 200 k emitter records on the host that the entry does not read
        recreate  close_engine + set_scene on the world with the second lamp
      (before each, untimed: back to one lamp)
Every figure is the host's clock around a call that returns once the structure is published, in
ms; the median of the timed rounds is reported.  The world's own rebuild of its description is
left out of `recreate`, as in tools/replace_mesh_timing.py.  After the last round the in-place
engines' renders are compared bit for bit with the recreated ones.  One JSON line after the table."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def grid(n):
    """n x n quads over [-1, 1]^2 in the plane z = 0, like the builtin rectangle: 2 n^2 faces"""
    import numpy as np

    x, y = np.meshgrid(np.linspace(-1.0, 1.0, n + 1), np.linspace(-1.0, 1.0, n + 1), indexing="xy")
    p = np.stack([x, y, np.zeros_like(x)], -1).reshape(-1, 3).astype(np.float32)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(p), 1))
    t = np.stack([(x + 1.0) / 2.0, (y + 1.0) / 2.0], -1).reshape(-1, 2).astype(np.float32)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + n + 2], 1), np.stack([i, i + n + 2, i + n + 1], 1)]).astype(np.uint32)
    return p, f, nrm, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spheres", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--accel", default="flat", choices=("flat", "two_level"))
    args = ap.parse_args()
    os.environ["PUPIL_ACCEL"] = args.accel
    if args.accel == "two_level":
        os.environ["PUPIL_TL_MODE"] = "world"

    import numpy as np
    import torch

    from pupiloptixlab_amd import abi, scenes
    from pupiloptixlab_amd import world as W
    from pupiloptixlab_amd.pt_pass import PTPass

    small, large = grid(224), grid(245)
    faces = {"small": len(small[1]), "large": len(large[1])}
    lamp_xf = W.transform(scale=(3, 3, 1), rotate=((1, 0, 0), 90), translate=(0, 13.9, 0))
    second_xf = W.transform(scale=(1, 1, 1), rotate=((1, 0, 0), 90), translate=(4.0, 13.8, 4.0))

    def make_world(mesh, second):
        """config 4's scene; the lamp (its last instance) shows a mesh shape of its own"""
        w = scenes.sphere_field(args.spheres, 64, 48, 4, seed=1)
        last = w.desc().num_instances - 1
        assert w.desc().instances[last].emitter_offset == 0
        w.remove_instance(last)
        shape = w.add_mesh(*mesh)
        mat = w.add_material(W.twosided(W.diffuse((0.0, 0.0, 0.0))))
        w.add_instance(shape, mat, lamp_xf, emitter_radiance=(40.0, 38.0, 34.0))
        if second:
            w.add_instance(shape, mat, second_xf, emitter_radiance=(20.0, 19.0, 17.0))
        return w, shape

    world, lamp = make_world(small, False)  # follows the replacements
    world_two, _ = make_world(small, True)
    world_one, _ = make_world(small, False)

    def image(pt):
        pt.mark_dirty()
        pt.render(1)
        torch.cuda.synchronize()
        return pt.buffers.get("pt accum buffer").cpu().numpy().view(np.uint32)

    def set_mesh(mesh):
        world.set_mesh(lamp, *mesh, allow_emissive=True)

    pt = PTPass(device=0)
    pt.set_scene(world)
    pt.device_emitters = True
    image(pt)
    dev = [torch.from_numpy(a.astype(np.int32) if a.dtype == np.uint32 else a).to(pt.device) for a in large]
    torch.cuda.synchronize()
    rows = {"replace.device": [], "replace.recreate": [], "add.entry": [], "add.pass": [], "add.recreate": []}
    images = {}

    def to_small():
        set_mesh(small)
        pt.replace_shape(lamp, *small)

    def to_one():
        pt.set_instances(world_one)

    def recreate(w):
        w.desc()  # the world's own rebuild of its description is not the engine's cost
        t0 = time.perf_counter()
        pt.close_engine()
        pt.set_scene(w)
        ms = (time.perf_counter() - t0) * 1e3
        return ms

    for _ in range(args.rounds + 1):  # the first round warms up and is dropped
        # ---- (a)
        to_small()
        t0 = time.perf_counter()
        pt.replace_shape_device(lamp, dev[0], dev[1], dev[2], dev[3])
        rows["replace.device"].append((time.perf_counter() - t0) * 1e3)
        images["replace.device"] = image(pt)
        set_mesh(large)
        rows["replace.recreate"].append(recreate(world))
        images["replace.recreate"] = image(pt)
        pt.device_emitters = True
        # ---- (b)
        to_small()
        to_one()
        n, arr, vis = pt._bindings(world_two)
        src = world_two.desc()
        desc = abi.SceneDesc()
        C.memmove(C.byref(desc), C.byref(src), C.sizeof(abi.SceneDesc))
        desc.instances = C.cast(arr, C.POINTER(abi.Instance))
        t0 = time.perf_counter()
        abi.check(pt._lib.pupil_pt_set_instances_emitters(pt._pt, C.byref(desc), vis.ctypes.data_as(abi.u32p), None, 0, None))
        rows["add.entry"].append((time.perf_counter() - t0) * 1e3)
        pt._after_set_instances(world_two)
        images["add.entry"] = image(pt)
        to_one()
        t0 = time.perf_counter()
        pt.set_instances(world_two)
        rows["add.pass"].append((time.perf_counter() - t0) * 1e3)
        images["add.pass"] = image(pt)
        rows["add.recreate"].append(recreate(world_two))
        images["add.recreate"] = image(pt)
        # back on the world that follows the replacements, for the next round
        pt.close_engine()
        pt.set_scene(world)
        pt.device_emitters = True
    info = pt.emitter_resize_info()
    prims = pt.stats()["bvh_prims"]
    pt.close_engine()
    same = np.array_equal(images["replace.device"], images["replace.recreate"]) and \
        all(np.array_equal(images[k], images["add.recreate"]) for k in ("add.entry", "add.pass"))
    timed = {k: v[1:] for k, v in rows.items()}
    med = {k: statistics.median(v) for k, v in timed.items()}
    print(f"# config-4 field with a {faces['small']}-face emissive lamp mesh, {prims} primitives, {args.accel}: "
          f"(a) lamp mesh to {faces['large']} faces, (b) a second instance of the lamp; {args.rounds} rounds after one "
          "warm-up, ms (host clock around the call)")
    print(f"{'':18s}" + "".join(f"{'round ' + str(k + 1):>10s}" for k in range(args.rounds)) + f"{'median':>10s}")
    for key, v in timed.items():
        print(f"{key:18s}" + "".join(f"{x:10.2f}" for x in v) + f"{med[key]:10.2f}")
    print(f"renders of the in-place and the recreated engines bit-identical: {same}")
    print(json.dumps({"accel": args.accel, "prims": int(prims), "faces": faces, "rounds": args.rounds,
                      "images_identical": bool(same), "median_ms": med, "ms": timed,
                      "last_true_areas": info["last_true_areas"]}))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
