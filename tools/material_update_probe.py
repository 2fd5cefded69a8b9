#!/usr/bin/env python3
"""Cost of changing a material in place, against re-creating the engine.

  python tools/material_update_probe.py [--size 1024] [--reps 20]

Scene: the Cornell box of scenes.py (256 x 256, depth 4) whose first material is a diffuse with one
size x size bitmap.  Every row is warm, the median of --reps, in ms; "call" is the host's clock
around the pass's method (what a caller waits for: the calls are synchronous), "engine" the
engine's own clock around its entry (pupil_pt_material_info):
  (a) edit       a diffuse colour: World.set_material + PTPass.update_material
  (b) host tex   the bitmap replaced from host texels: the same two calls (the world copies the
                 texels, the engine uploads them into the allocation it keeps)
  (c) device     PTPass.update_texture_device on the diffuse's slot: a device-to-device copy
  (d) plastic    the same on the diffuse slot of a plastic: copy + the averaging kernel
                 (pt_materials.hip).  The kernel's share is (d) - (c) of the engine's clock: both
                 run the same copy on the engine's stream and wait for it.
  (e) host sum   what the kernel replaces: the texels copied to the host and summed there in the
                 host's order (np.cumsum, a sequential float32 chain per channel)
  (f) re-create  pupil_pt_destroy + pupil_pt_create of the same scene, the only way to change a
                 material without these entries
One JSON line after the table."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    from pupiloptixlab_amd import World, scenes
    from pupiloptixlab_amd import world as W
    from pupiloptixlab_amd.pt_pass import PTPass

    n = args.size
    rng = np.random.default_rng(1)
    tex = [rng.uniform(0.05, 0.95, (n, n, 4)).astype(np.float32) for _ in range(2)]
    with tempfile.TemporaryDirectory() as tmp:  # the loader reads the file once
        w = World().load_scene(scenes.cornell_xml(os.path.join(tmp, "cornell.xml"), 256, 256, 4))
    w.set_material(0, W.twosided(W.diffuse(W.bitmap(tex[0]))))
    pt = PTPass(device=0)
    pt.set_scene(w)
    pt.render(1)
    torch.cuda.synchronize()
    dev = [torch.from_numpy(t).to(pt.device) for t in tex]
    torch.cuda.synchronize()

    def timed(fn):
        call, engine = [], []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            fn(k)
            ms = (time.perf_counter() - t0) * 1e3
            if k >= args.warmup:
                call.append(ms)
                engine.append(pt.material_info()["last_ms"])
        return statistics.median(call), statistics.median(engine)

    def edit(k):
        w.set_material(1, W.diffuse((0.2 + 0.1 * (k % 2), 0.5, 0.4)))
        pt.update_material(w, 1)

    def host_tex(k):
        w.set_material(0, W.twosided(W.diffuse(W.bitmap(tex[k % 2]))))
        pt.update_material(w, 0)

    def device_tex(k):
        pt.update_texture_device(0, 0, dev[k % 2])

    def host_sum(k):
        a = dev[k % 2].cpu().numpy().reshape(-1, 4)
        return [np.cumsum(a[:, c], dtype=np.float32)[-1] for c in range(3)]

    def recreate(k):
        pt.set_scene(w)

    rows = {"edit": timed(edit), "host_tex": timed(host_tex), "device": timed(device_tex)}
    w.set_material(0, W.plastic(W.bitmap(tex[0]), 0.9))
    pt.update_material(w, 0)
    rows["plastic"] = timed(device_tex)
    weight = pt.read_material(0)["specular_sampling_weight"]
    rows["host_sum"] = (timed(host_sum)[0], 0.0)
    rows["recreate"] = (timed(recreate)[0], 0.0)
    kernel = rows["plastic"][1] - rows["device"][1]
    print(f"# material updates, Cornell 256 x 256, one {n} x {n} bitmap ({n * n * 16 / 1e6:.1f} MB), median of {args.reps}, ms")
    print(f"{'':14s}{'call':>10s}{'engine':>10s}")
    for name, (c, e) in rows.items():
        print(f"{name:14s}{c:10.3f}" + (f"{e:10.3f}" if e else f"{'-':>10s}"))
    print(f"averaging kernel (plastic - device, engine clock): {kernel:.3f} ms; host copy + sum: {rows['host_sum'][0]:.3f} ms")
    print(json.dumps({"size": n, "reps": args.reps, "kernel_ms": kernel, "weight": float(weight),
                      **{k: {"call_ms": c, "engine_ms": e} for k, (c, e) in rows.items()}}))


if __name__ == "__main__":
    main()
