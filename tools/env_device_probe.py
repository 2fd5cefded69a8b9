#!/usr/bin/env python3
"""Cost of replacing the env map's texels, from the host against from device memory.

  python tools/env_device_probe.py [--width 2048] [--height 1024] [--reps 20]

Scene: one rectangle under a width x height env map, film 64 x 64.  The two paths alternate in one
process, after --warmup rounds; every figure is the host's clock around a call that synchronises
before it returns, in ms, as median and min - max over --reps:
  (a) host     pupil_pt_update_emitters with a desc whose env texels changed: the serial table
               build on the host, texels and tables uploaded into new allocations
  (b) device   pupil_pt_update_env_device with the same texels resident on the device: a
               device-to-device copy and the two table stages of pt_envmap.hip
  (b) engine   pupil_pt_env_info's last_ms of the same calls (the engine's own clock)
  params       pupil_pt_update_env_params (scale and rotation only)
  (d2h)        the device texels copied to the host, what path (a) costs on top when the texels
               are produced on the GPU (not part of (a))
After each round the tables of (a) and (b), built from the same texels, are compared bit for bit.
One JSON line after the table."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    from pupiloptixlab_amd import World, abi, scenes
    from pupiloptixlab_amd.pt_pass import PTPass

    w, h = args.width, args.height
    rng = np.random.default_rng(1)
    tex = [np.ascontiguousarray(np.concatenate([rng.uniform(0.08, 1.0, (h, w, 3)), np.ones((h, w, 1))], -1), np.float32)
           for _ in range(2)]
    with tempfile.TemporaryDirectory() as tmp:  # the loader reads the files once
        scenes._write_pfm(os.path.join(tmp, "env.pfm"), tex[0][..., :3])
        xml = os.path.join(tmp, "env.xml")
        with open(xml, "w") as f:
            f.write('<scene version="3.0.0"><integrator type="path"><integer name="max_depth" value="2"/></integrator>'
                    '<sensor type="perspective"><float name="fov" value="45"/><transform name="to_world">'
                    '<lookat origin="0, 2, 6" target="0, 0, 0" up="0, 1, 0"/></transform><film type="hdrfilm">'
                    '<integer name="width" value="64"/><integer name="height" value="64"/></film></sensor>'
                    '<emitter type="envmap"><string name="filename" value="env.pfm"/><float name="scale" value="1.5"/>'
                    '<transform name="to_world"><rotate y="1" angle="30"/></transform></emitter>'
                    '<shape type="rectangle"><transform name="to_world"><rotate x="1" angle="-90"/></transform>'
                    '<bsdf type="diffuse"><rgb name="reflectance" value="0.5, 0.5, 0.5"/></bsdf></shape></scene>')
        world = World().load_scene(xml)
    desc = world.desc()
    pt = PTPass(device=0)
    pt.set_scene(world)
    lib = pt._lib
    pt.render(1)
    torch.cuda.synchronize()
    dev = [torch.from_numpy(t).to(pt.device) for t in tex]
    torch.cuda.synchronize()
    env = desc.env.contents
    to_world = np.array(list(env.to_world), np.float32)

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def host(k):
        env.radiance.rgba = tex[k % 2].ctypes.data_as(abi.f32p)
        abi.check(lib.pupil_pt_update_emitters(pt._pt, C.byref(desc)))

    rows = {"host": [], "device": [], "device_engine": [], "params": [], "d2h": []}
    identical = True
    for k in range(args.warmup + args.reps):
        a = clock(lambda: host(k))
        ta = pt.env_tables()
        b = clock(lambda: pt.update_env_device(dev[k % 2]))
        be = pt.env_info()["last_ms"]
        tb = pt.env_tables()
        identical = identical and all(np.array_equal(np.asarray(ta[n]).view(np.uint32), np.asarray(tb[n]).view(np.uint32))
                                      for n in ("col_cdf", "row_cdf", "row_weight", "normalization"))
        p = clock(lambda: pt.update_env_params(1.0 + 0.25 * (k % 2), to_world))
        c = clock(lambda: dev[k % 2].cpu())
        if k >= args.warmup:
            for name, v in zip(rows, (a, b, be, p, c)):
                rows[name].append(v)
    print(f"# env map {w} x {h} ({w * h * 16 / 1e6:.1f} MB of texels), {args.reps} alternated rounds after "
          f"{args.warmup} warm-up rounds, ms")
    print(f"{'':16s}{'median':>10s}{'min':>10s}{'max':>10s}")
    for name, v in rows.items():
        print(f"{name:16s}{statistics.median(v):10.3f}{min(v):10.3f}{max(v):10.3f}")
    ratio = statistics.median(rows["host"]) / statistics.median(rows["device"])
    print(f"(a) host / (b) device, medians: {ratio:.1f}; tables of the two paths bit-identical in every round: {identical}")
    print(json.dumps({"width": w, "height": h, "reps": args.reps, "tables_identical": identical, "host_over_device": ratio,
                      **{k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in rows.items()}}))
    if not identical:
        sys.exit(1)


if __name__ == "__main__":
    main()
