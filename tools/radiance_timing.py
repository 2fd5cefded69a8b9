#!/usr/bin/env python3
"""What PTPass.radiance costs next to the render it restates, and whether it costs the render anything.

  python tools/radiance_timing.py --only radiance|render --reps 6       (one case, under a kernel trace:
        rocprofv3 --kernel-trace -d DIR -o NAME -- python tools/radiance_timing.py --only ...)
  python tools/radiance_timing.py --parent-lib PATH [--trace-radiance DB --trace-render DB --trace-calls 6]
        [--out profiles/radiance_rays_timing.txt]

Workload: config 4 (sphere_field 500, seed 1) at 1920 x 1080, the seed-0 camera rays (film jitter of
rng_init(pixel, 0), restated here in numpy float32 in camera_path's order) through radiance() at
spp 8, depth 4.  Baseline: pupil_pt_render of the same frame (seed 0, spp 8, no PUPIL_HINT_CONTINUE)
by the library built from the parent commit (--parent-lib), its own engine on the same scene in the
same process.  The cases -- parent render, this commit's render, radiance, and radiance on an engine
created under PUPIL_RADIANCE_CHUNK=4194304 (--small-chunk) -- are alternated
round by round, their order rotated every round; device events around each call; the median, min, p10 and p90 of --reps samples
after --warmup rounds.  The one condition: this commit's render lies within the parent's p10-p90.

--trace-radiance / --trace-render: the result databases (rocpd SQLite) of the two --only runs of
--trace-calls calls each; their kernel times per stage are appended as a table.

The whole text goes to --out (and stdout): a re-run rewrites all of it.  Recorded, asserted nowhere."""
import argparse
import contextlib
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, SPP, DEPTH = 1920, 1080, 8, 4


def rng_jitter(pixels, seed):
    """rng_init(pixel, seed) and the two film draws (pt_shading.h), vectorised."""
    import numpy as np

    m = np.uint64(0xFFFFFFFF)
    v0, v1, s0 = pixels.astype(np.uint64), np.full(len(pixels), seed, np.uint64), np.uint64(0)
    for _ in range(4):
        s0 = (s0 + np.uint64(0x9E3779B9)) & m
        v0 = (v0 + ((((v1 << np.uint64(4)) + np.uint64(0xA341316C)) & m) ^ ((v1 + s0) & m)
                    ^ (((v1 >> np.uint64(5)) + np.uint64(0xC8013EA4)) & m))) & m
        v1 = (v1 + ((((v0 << np.uint64(4)) + np.uint64(0xAD90777D)) & m) ^ ((v0 + s0) & m)
                    ^ (((v0 >> np.uint64(5)) + np.uint64(0x7E95761E)) & m))) & m
    s = v0
    out = []
    for _ in range(2):
        s = (np.uint64(1664525) * s + np.uint64(1013904223)) & m
        out.append((s & np.uint64(0x00FFFFFF)).astype(np.float32) / np.float32(16777216.0))
    return out


def camera_rays(desc, seed):
    """camera_path (pt_shade.h) for every pixel at `seed`, float32, sums left to right: (n, 8)."""
    import numpy as np

    f = np.float32
    s2c = np.array(list(desc.sample_to_camera), f).reshape(4, 4)
    c2w = np.array(list(desc.camera_to_world), f).reshape(4, 4)
    pix = np.arange(desc.width * desc.height, dtype=np.uint32)
    jx, jy = rng_jitter(pix, seed)
    x, y = (pix % desc.width).astype(f), (pix // desc.width).astype(f)
    film = [(x + jx) / f(desc.width), (y + jy) / f(desc.height), np.zeros_like(jx), np.ones_like(jx)]

    def dot(row, v):
        acc = row[0] * v[0]
        for k in range(1, len(v)):
            acc = acc + row[k] * v[k]
        return acc

    def normalize(v):
        inv = f(1.0) / np.sqrt(dot(v, v))
        return [c * inv for c in v]

    d = [dot(s2c[r], film) for r in range(4)]
    inv_w = f(1.0) / d[3]
    d = normalize([d[0] * inv_w, d[1] * inv_w, d[2] * inv_w, np.zeros_like(jx)])
    d = normalize([dot(c2w[r], d) for r in range(3)])
    n = len(pix)
    o = [np.full(n, c2w[r, 3], f) for r in range(3)]
    return np.ascontiguousarray(np.stack(o + d + [np.full(n, 0.001, f), np.full(n, 1e16, f)], 1), f)


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def device_name(torch):
    """The accelerator by its architecture: torch's marketing name of an MI355X is a generic one."""
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    name = torch.cuda.get_device_name(0)
    return f"MI355X (gfx950; torch names it '{name}')" if arch == "gfx950" else f"{name} ({arch})"


def stage_times(db_path, calls):
    """{kernel: (ms per call, launches per call)} of the wavefront stages in a rocprofv3 database."""
    import sqlite3

    db = sqlite3.connect(db_path)
    out = {}
    for name, count, ns in db.execute("select name, count(*), sum(end - start) from kernels group by name"):
        m = re.search(r"\b(k_(?:generate|trace4|shade|part|accumulate)\w*)(<[^>(]*>)?", name)
        if m:
            key = m.group(1) + (m.group(2) or "")
            a, b = out.get(key, (0.0, 0.0))
            out[key] = (a + ns / 1e6 / calls, b + count / calls)
    return out


@contextlib.contextmanager
def environment(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "radiance_rays_timing.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("radiance", "render"), default=None)
    ap.add_argument("--small-chunk", type=int, default=4194304, help="PUPIL_RADIANCE_CHUNK of the second engine, 0 = none")
    ap.add_argument("--trace-radiance", default=None)
    ap.add_argument("--trace-render", default=None)
    ap.add_argument("--trace-calls", type=int, default=6)
    args = ap.parse_args()

    import torch

    from pupiloptixlab_amd import abi, scenes
    from pupiloptixlab_amd.pt_pass import PTPass

    world = scenes.sphere_field(500, W, H, DEPTH, seed=1)
    desc = world.desc()

    def engine(lib=None):
        pt = PTPass(device=0)
        if lib is not None:
            pt._lib = lib
        pt.set_scene(world)
        return pt

    new = engine()
    rays = torch.from_numpy(camera_rays(desc, 0)).to(new.device)
    n = rays.shape[0]
    out = {"radiance": torch.zeros((n, 4), device=new.device), "albedo": torch.zeros((n, 3), device=new.device),
           "normal": torch.zeros((n, 3), device=new.device)}

    def render(pt, spp=SPP, stats=0):
        pt.dirty = False
        pt.random_seed, pt.sample_cnt = 0, 0
        pt.render(spp, collect_stats=stats)

    def radiance(pt=new, spp=SPP):
        pt.radiance(rays, spp=spp, seed=0, accumulate=True, want=tuple(out), out=out)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    if args.only:
        fn = radiance if args.only == "radiance" else (lambda: render(new))
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        print(f"{args.only}: {args.reps} calls")
        return

    lines = [f"Radiance along rays from device memory (pupil_pt_radiance_rays), one {device_name(torch)}.",
             "", "Timing -- recorded, asserted nowhere but for the one condition below.",
             f"config 4 (sphere_field 500, seed 1, flat BVH), {W}x{H} = {n} rays: the seed-0 camera rays, spp {SPP}, "
             f"depth {DEPTH} = {n * SPP} paths per call.",
             f"Device events around each call, {args.reps} samples after {args.warmup} warm-up rounds, the cases "
             "alternated round by round in one process, their order rotated every round; ms per call.", ""]

    # what the rays are: radiance at spp 1 against the render's pixels
    render(new, 1)
    radiance(new, 1)
    torch.cuda.synchronize()
    same = {k: bool(torch.equal(out[k].view(torch.int32), new.buffers.get(b).view(torch.int32)))
            for k, b in (("radiance", "pt accum buffer"), ("albedo", "albedo"), ("normal", "normal"))}
    lines.append(f"radiance(spp=1, seed=0) == render(1) at seed 0 bit for bit, all {n} pixels: {same}")

    rad = "radiance (this commit)"
    cases = {"render (this commit)": lambda: render(new), rad: radiance}
    parent = small = None
    if args.parent_lib:
        parent = engine(abi.load_library(args.parent_lib))
        cases = {"render (parent lib)": lambda: render(parent), **cases}
    rad_small = f"radiance, chunk {args.small_chunk}"
    if args.small_chunk:
        with environment(PUPIL_RADIANCE_CHUNK=str(args.small_chunk)):
            small = engine()
        cases[rad_small] = lambda: radiance(small)
    ms = {k: [] for k in cases}
    names = list(cases)
    for r in range(args.warmup + args.reps):
        for k in names[r % len(names):] + names[:r % len(names)]:  # no case always follows the same one
            t = timed(cases[k])
            if r >= args.warmup:
                ms[k].append(t)
    lines += ["", f"{'case':<28}{'median':>9}{'min':>9}{'p10':>9}{'p90':>9}  Mpaths/s (median)"]
    for k, v in ms.items():
        med = statistics.median(v)
        lines.append(f"{k:<28}{med:>9.3f}{min(v):>9.3f}{pct(v, 0.1):>9.3f}{pct(v, 0.9):>9.3f}  {n * SPP / med / 1e3:>8.0f}")
    med = {k: statistics.median(v) for k, v in ms.items()}
    base = "render (parent lib)" if parent else "render (this commit)"
    lines.append(f"radiance / {base}: {med[rad] / med[base]:.4f} (the default chunk: the call is "
                 f"{-(-n * SPP // new_chunk())} chunk(s))")
    if small:
        lines.append(f"{rad_small} / {base}: {med[rad_small] / med[base]:.4f} ({-(-n * SPP // args.small_chunk)} chunks: "
                     "every stage drains that many launch tails instead of one)")
    if parent:
        lo, hi = pct(ms[base], 0.1), pct(ms[base], 0.9)
        ok = lo <= med["render (this commit)"] <= hi
        lines.append(f"the one condition: this commit's render, median {med['render (this commit)']:.3f} ms, within the "
                     f"parent's p10-p90 [{lo:.3f}, {hi:.3f}]: {ok}")

    # the render's own stage times (PUPIL_STATS_TIMING: events around every stage launch)
    render(new, SPP, stats=2)
    st = new.stats()
    lines += ["", f"stage times of one render of this commit with PUPIL_STATS_TIMING: extend {st['extend_ms']:.3f} ms, "
              f"bounce traversals {st['trace_ms'] - st['extend_ms']:.3f} ms, shade {st['shade_ms']:.3f} ms, "
              f"whole render {st['last_render_ms']:.3f} ms"]
    info = new.radiance_info()
    lines.append(f"radiance calls {info['calls']}, scratch growths {info['scratch_grows']}, extension rays "
                 f"{info['extension_rays']}, shadow rays {info['shadow_rays']}; last call {info['last_ms']:.3f} ms by "
                 "the engine's own events")

    if args.trace_radiance and args.trace_render:
        a, b = stage_times(args.trace_radiance, args.trace_calls), stage_times(args.trace_render, args.trace_calls)
        lines += ["", f"Stage kernels under a kernel trace, {args.trace_calls} calls of each kind in processes of their own "
                  "(--only), default chunk; ms per call (launches per call).  k_trace4<0..>: the primary extend, "
                  "k_trace4<3..>: a bounce's mixed traversal; k_shade_*<1..>: the first shade, <2..>: a bounce's, "
                  "<0>: shading by material bins; k_part_*: the partitions.",
                  f"{'kernel':<44}{'radiance':>16}{'render':>16}{'difference':>12}"]
        tot = 0.0
        for k in sorted(set(a) | set(b)):
            (am, ac), (bm, bc) = a.get(k, (0.0, 0.0)), b.get(k, (0.0, 0.0))
            tot += am - bm
            lines.append(f"{k:<44}{am:>10.3f} ({ac:>3.0f}){bm:>10.3f} ({bc:>3.0f}){am - bm:>+12.3f}")
        lines.append(f"{'sum of the differences':<44}{'':>32}{tot:>+12.3f}")
        lines.append("Read with pt_radiance.hip's header: the generate stores five 16-B records per path where the "
                     "render's (fresh paths) stores one and reads 32 B of ray; the primary extend reads 4 B of queue "
                     "and the 16-B origin record per path; the first shade reads back throughput, radiance and RNG.")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    for pt in (new, parent, small):
        if pt:
            pt.close_engine()


def new_chunk():
    """The default PUPIL_RADIANCE_CHUNK, or what the environment sets."""
    return int(float(os.environ.get("PUPIL_RADIANCE_CHUNK", 1 << 24)))


if __name__ == "__main__":
    main()
