#!/usr/bin/env python3
"""Cost of adding and removing one instance in place (pupil_pt_set_instances), against the only
alternative there was before: destroying the engine and creating a new one on the edited world.

  python tools/instance_set_probe.py [--rounds 5] [--out profiles/instance_set_timing.txt]

Scenes: the benchmark's config-5 field (scenes.instanced_field: 40 instances of one 250 k-triangle
mesh, the room, the lamp) in two-level world and object mode, and its config-4 field
(scenes.sphere_field: 1 M triangles in 8 meshes) on the flattened BVH; film 64 x 48.  Per round,
in this order, all in one process:
  host add / remove      PTPass.set_instances after World.add_instance of a used shape / after
                         World.remove_instance of it again
  device add / remove    PTPass.set_instances_device, transforms already on the device
  recreate               close_engine + set_scene on the world with the extra instance
Every figure is the host's clock around a call that returns once the structure is published, in
ms; the table gives the median and the range over the rounds.  One JSON line after the table."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(name, env, make_world, rounds):
    import numpy as np
    import torch

    from pupiloptixlab_amd import world as W
    from pupiloptixlab_amd.pt_pass import PTPass

    for k in ("PUPIL_ACCEL", "PUPIL_TL_MODE"):
        os.environ.pop(k, None)
    os.environ.update(env)
    world = make_world()
    material = 0
    xf = W.transform(scale=(0.9, 0.9, 0.9), rotate=((0, 1, 0), 40.0), translate=(1.0, 6.0, 0.5))
    pt = PTPass(device=0)
    pt.set_scene(world)
    n0 = world.desc().num_instances
    times = {k: [] for k in ("host add", "host remove", "device add", "device remove", "recreate")}
    info = {}

    def clock(key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times[key].append(1e3 * (time.perf_counter() - t0))

    def tensor():
        d = world.desc()
        a = np.array([list(d.instances[i].to_world) for i in range(d.num_instances)], np.float32)
        t = torch.from_numpy(a).to(pt.device)
        torch.cuda.synchronize()
        return t

    for r in range(rounds + 1):  # round 0 warms every path up and is dropped
        world.add_instance(0, material, xf)
        clock("host add", lambda: pt.set_instances(world))
        info["add"] = pt.set_instances_info()
        world.remove_instance(n0)
        clock("host remove", lambda: pt.set_instances(world))
        world.add_instance(0, material, xf)
        t = tensor()
        clock("device add", lambda: pt.set_instances_device(world, t))
        world.remove_instance(n0)
        t = tensor()
        clock("device remove", lambda: pt.set_instances_device(world, t))
        world.add_instance(0, material, xf)

        def recreate():
            pt.close_engine()
            pt.set_scene(world)

        clock("recreate", recreate)
        world.remove_instance(n0)
        pt.set_instances(world)  # untimed: back to the scene every round starts from
        if r == 0:
            for v in times.values():
                v.clear()
    pt.close_engine()
    row = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
    return {"scene": name, "instances": n0, "rounds": rounds, "last_blas_builds": info["add"]["last_blas_builds"],
            "last_whole_rebuild": info["add"]["last_whole_rebuild"], "ms": row}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from pupiloptixlab_amd import scenes

    field5 = lambda: scenes.instanced_field(40, 64, 48, 6, seed=2)
    field4 = lambda: scenes.sphere_field(500, 64, 48, 4, seed=1)
    runs = [("config 5, two-level world", {"PUPIL_ACCEL": "two_level", "PUPIL_TL_MODE": "world"}, field5),
            ("config 5, two-level object", {"PUPIL_ACCEL": "two_level", "PUPIL_TL_MODE": "object"}, field5),
            ("config 4, flattened", {"PUPIL_ACCEL": "flat"}, field4)]
    results = [measure(name, env, make, args.rounds) for name, env, make in runs]
    lines = ["pupil_pt_set_instances: one instance of a used shape added, then removed; ms, median (min - max) of "
             f"{args.rounds} rounds, one process, alternated", ""]
    keys = ("host add", "host remove", "device add", "device remove", "recreate")
    lines.append(f"{'scene':30s}" + "".join(f"{k:>26s}" for k in keys) + "   blas builds / whole rebuild")
    for r in results:
        cells = "".join(f"{r['ms'][k]['median']:10.2f} ({r['ms'][k]['min']:.1f} - {r['ms'][k]['max']:.1f})".rjust(26)
                        for k in keys)
        lines.append(f"{r['scene']:30s}{cells}   {r['last_blas_builds']} / {r['last_whole_rebuild']}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"instance_set_probe": results}))


if __name__ == "__main__":
    main()
