"""The frame-pipeline schedule (csrc/host/pipe_schedule.h) without a GPU: a stand-alone driver
(pipe_schedule_driver.cpp) walks the schedule as engine.hip render_pipelined does and prints one
line per decision; the checks below hold those lines to the schedule's properties -- complete
frames, consecutive seeds, free slots, ring extents, tags, the steady state of an OnRun sequence,
grouped sequences and their split iterations, resets, the moving camera, the ramp, the OOM shrink
order and the conservation of trace halves.  The driver is built twice, plain and with
-fsanitize=address,undefined; every script runs through both and must print the same lines."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pupiloptixlab_amd", "csrc")
P = 48 * 32  # paths of a 1-spp render: the size of test_pipelined_onrun_sequence


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("pipe_schedule")
    exes = []
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                     "-fno-sanitize-recover=undefined"])):
        exe = d / name
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                            os.path.join(HERE, "pipe_schedule_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        exes.append(str(exe))
    return exes


def knobs(ahead=1, limit=0, budget=1e12, paths=64e6, group_paths=1.0, group_max=64, group_all=0, split=1, ramp=1,
          frame_paths=4e5):
    return f"knobs {ahead} {limit} {budget!r} {paths!r} {float(group_paths)!r} {group_max} {group_all} {split} {ramp} {frame_paths!r}"


def render(seed, spp=1, hint=0, depth=4, paths=None, pixels=P):
    return f"render {spp} {seed} {hint} {depth} {pixels * spp if paths is None else paths} {pixels}"


def sequence(n, seed0=0, **kw):
    spp = kw.get("spp", 1)
    return [render(seed0 + i * spp, **kw) for i in range(n)]


def fields(line):
    return {k: int(v) for k, v in (t.split("=") for t in line.split()[1:] if "=" in t and not t.startswith("groups"))}


def walk(drivers, script):
    """Runs the script through both builds and returns one record per render."""
    outs = []
    for exe in drivers:
        r = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr)
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    renders = []
    for line in outs[0].splitlines():
        kind = line.split()[0]
        if kind == "render":
            renders.append({"render": fields(line), "shrinks": [], "drops": [], "events": [], "oom": False})
        elif kind == "shrink":
            renders[-1]["shrinks"].append(fields(line))
        elif kind == "oom":
            renders[-1]["oom"] = True
        elif kind == "drop":
            d = fields(line)
            renders[-1]["drops"].append((d["off"], d["len"]))
        elif kind == "shortcut":
            renders[-1]["shortcut"] = int(line.split()[1])
        elif kind in ("trace", "shade", "iters", "finish"):
            renders[-1]["events"].append((kind, fields(line)))
        elif kind == "state":
            renders[-1]["state"] = fields(line)
            g = line.split("groups=")[1]
            renders[-1]["groups"] = [tuple(int(x) for x in t.split(":")) for t in g.split(",") if t]
        else:
            renders[-1][kind] = fields(line)
    return renders


def check(renders):
    """The properties every walk must have; returns a summary per render."""
    live, wtag, pending = [], None, False  # groups in flight as the lines imply them
    cap = slot_cap = np_old = 0
    advances = retired = 0  # group-phases traced; groups completed (conservation)
    seq_ok, D_seq = True, None
    out = []

    def extent():
        return max((g["slot"] * slot_cap + g["frames"] * npaths for g in live), default=0)

    for r in renders:
        R, p = r["render"], r["plan"]
        D, npaths, spp = R["depth"], R["paths"], R["spp"]
        assert p["K"] * p["G"] * npaths < 2 ** 31 or p["K"] * p["G"] == 1
        assert p["need"] == (p["K"] * p["G"] * npaths if p["speculate"] else npaths)
        lost = p["need"] > cap  # the ring is reallocated: nothing left to clear
        if r["oom"]:
            live, pending, cap = [], False, 0
            out.append({"oom": True, "shrinks": r["shrinks"]})
            continue
        c = r["commit"]
        K, G = c["K"], c["G"]
        assert K * G * npaths < 2 ** 31 or K * G == 1
        pre = [e for e in r["events"][:1] if e[0] == "shade"]  # the shade half of a split iteration
        if c["reset"]:
            want = [] if lost else sorted((g["slot"] * slot_cap, g["frames"] * np_old) for g in live)
            assert sorted(r["drops"]) == want, (r["drops"], want)
            assert all(off + n <= c["cap"] for off, n in r["drops"])
            assert not pre  # a pending half is dropped, never shaded
            if not p["continues"]:
                advances = retired = 0
                D_seq = D
            live, pending = [], False
        else:
            assert p["continues"] and not r["drops"] and len(pre) == int(pending)
        cap, slot_cap, np_old = c["cap"], G * npaths, npaths
        s = {"oom": False, "reset": c["reset"], "speculate": p["speculate"], "K": K, "G": G, "need": p["need"],
             "shortcut": r["shortcut"], "L": None, "traces": 0, "ahead_groups": 0, "own_frames": None, "pre_shade": len(pre),
             "shrinks": r["shrinks"], "may_pipe": p["may_pipe"]}
        if r["shortcut"]:
            assert not live and not p["speculate"] and not r["events"]
        finished = False
        inject = None
        for kind, e in r["events"]:
            if kind == "iters":
                s["L"] = e["L"]
            elif kind == "trace":
                s["traces"] += 1
                assert e["had"] == int(bool(live))
                if e["had"]:
                    assert e["rtag"] == wtag and e["extent"] == extent()
                    assert e["extent"] <= K * G * npaths and e["extent"] <= cap
                else:
                    assert e["inject"]
                inject = None
                if e["inject"]:
                    assert len(live) < K and e["slot"] < K and e["slot"] not in [g["slot"] for g in live]
                    assert e["seed"] == (live[-1]["seed"] + live[-1]["frames"] * spp if live else R["seed"])
                    assert 1 <= e["frames"] <= G and e["paths"] == e["frames"] * npaths and e["base"] == e["slot"] * slot_cap
                    assert e["samples"] == e["frames"] * spp and e["aov"] == int(bool(live) or e["frames"] > 1)
                    assert e["base"] + e["paths"] <= cap
                    if live:
                        s["ahead_groups"] += 1
                    else:
                        s["own_frames"] = e["frames"]
                    inject = e
                    live.append({"slot": e["slot"], "seed": e["seed"], "frames": e["frames"], "consumed": 0, "T": 0, "S": 0,
                                 "aov": e["aov"]})
                for g in live:
                    assert g["T"] == g["S"] < D  # alternating, trace first
                    g["T"] += 1
                advances += len(live)
                pending = finished  # a trace half after the finish waits for the next render's shade half
            elif kind == "shade":
                for g in live:
                    assert g["T"] == g["S"] + 1
                    g["S"] += 1
                wtag = e["wtag"]
                assert 1 <= wtag <= 63 and e["extent"] == extent() <= min(cap, K * G * npaths)
                assert e["max"] <= e["extent"] and e["clear"] == int(D > 63)
                if kind == "shade" and e is (pre[0][1] if pre else None):
                    pending = False
                else:
                    assert (e["n"], e["aov"]) == ((inject["paths"], inject["aov"]) if inject else (0, 0))
                    if inject:
                        assert e["base"] == inject["base"] and e["seed"] == inject["seed"] and e["idx"] == inject["slot"] * G
                    assert e["list"] == (2 if inject else 1) if len(live) > (1 if inject else 0) else e["list"] == 0
            elif kind == "finish":
                g = live[0]
                # the frame a render accumulates carries its seed and has run D trace and D shade halves
                assert g["seed"] + g["consumed"] * spp == R["seed"] and g["T"] == g["S"] == D
                assert (e["slot"], e["offset"], e["aov"]) == (g["slot"], g["consumed"] * npaths, g["aov"])
                assert e["idx"] == g["slot"] * G + g["consumed"] and (not e["aov"] or (e["idx"] + 1) * 7 * R["paths"] // spp <= c["aov_cap"])
                g["consumed"] += 1
                if g["consumed"] == g["frames"]:
                    live.pop(0)
                    retired += 1
                finished = True
                s["ahead"] = e["ahead"]
        assert len(live) <= K
        st = r["state"]
        assert r["groups"] == [(g["slot"], g["seed"], g["S"], g["frames"], g["consumed"]) for g in live]
        assert st["in_flight"] == sum(g["frames"] - g["consumed"] for g in live) and st["pending"] == int(pending)
        assert st["slots"] == K
        # conservation: group-phases traced = D x groups completed + the phases of the groups in flight
        if not r["shortcut"]:
            assert advances == D * retired + sum(ph + st["pending"] for _, _, ph, _, _ in r["groups"])
        s.update(in_flight=st["in_flight"], slots=st["slots"], pending=st["pending"], groups=r["groups"])
        out.append(s)
    return out


@pytest.mark.parametrize("depth,limit", [(4, 0), (5, 0), (8, 0), (8, 3)])
def test_steady_state_of_a_continued_sequence(drivers, depth, limit):
    """2 K + 1 continuing 1-spp renders, one frame per slot: K slots, K - 1 frames in flight (what
    test_pipelined_onrun_sequence asserts on the GPU), one iteration per render once the ring is full."""
    K = min(depth, limit) if limit else depth
    for ramp in (1, 0):
        s = check(walk(drivers, [knobs(limit=limit, ramp=ramp)] + sequence(2 * K + 1, depth=depth)))
        assert (s[-1]["slots"], s[-1]["in_flight"]) == (K, K - 1)
        full = next(i for i, r in enumerate(s) if r["in_flight"] == K - 1)
        assert full < 2 * K and all(r["in_flight"] == K - 1 and not r["reset"] for r in s[full + 1:])
        if K < depth:  # a ring capped below the depth: each frame still needs `depth` iterations
            continue
        assert all(r["L"] == 1 and r["traces"] == 1 for r in s[full + 1:])
        # Without the ramp limit the first speculating render (the third: two renders must have
        # continued) fills the ring, and every render from render max(K, 4) on runs one iteration;
        # PUPIL_PIPE_RAMP=1 spreads the fill over the renders after it (still within 2 K + 1)
        if ramp == 0:
            assert all(r["L"] == 1 for r in s[max(K, 4) - 1:]), [r["L"] for r in s]


@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("group_max", [1, 2, 4])
@pytest.mark.parametrize("depth", [4, 8])
def test_grouped_sequence(drivers, depth, group_max, split):
    s = check(walk(drivers, [knobs(group_paths=4 * P - 1, group_max=group_max, split=split)] + sequence(6 * depth, depth=depth)))
    assert all(r["G"] == group_max for r in s)
    tail = s[3 * depth:]
    assert any(r["L"] == 0 for r in tail) == (group_max > 1)
    for prev, r in zip(tail, tail[1:]):
        if not split or group_max == 1:
            assert not r["pending"] and not r["pre_shade"]
        if r["L"] == 0:  # an earlier render completed this frame
            assert r["traces"] == r["pending"] == (1 if split and r["groups"] and r["groups"][0][4] == 0 else 0)
        assert r["pre_shade"] == prev["pending"]


@pytest.mark.parametrize("group_all", [0, 1])
@pytest.mark.parametrize("hint", [0, 1])
def test_batched_renders_group_only_when_asked(drivers, hint, group_all):
    """2-spp renders pipeline with the hint only, and batch frames per slot only with group_all."""
    s = check(walk(drivers, [knobs(group_paths=4 * 2 * P - 1, group_max=4, group_all=group_all)] +
                   sequence(12, spp=2, hint=hint, depth=5)))
    assert all(r["may_pipe"] == hint and r["K"] == (5 if hint else 1) for r in s)
    assert all(r["G"] == (4 if hint and group_all else 1) for r in s)
    if hint and group_all:
        assert any(r["L"] == 0 for r in s[4:])


@pytest.mark.parametrize("stop", ["seed", "invalidate", "depth", "key"])
@pytest.mark.parametrize("group_max", [1, 2])
def test_a_change_drops_the_frames_in_flight(drivers, stop, group_max):
    for n in (9, 10, 11, 12):  # the change lands at every point of a group, and between two halves
        script = [knobs(group_paths=4 * P - 1, group_max=group_max)] + sequence(n)
        if stop == "seed":
            after = sequence(4, seed0=100)
        elif stop == "depth":
            after = sequence(4, seed0=n, depth=5)
        else:
            script.append("invalidate" if stop == "invalidate" else "key 1")
            after = sequence(4, seed0=n)
        s = check(walk(drivers, script + after))
        before, r = s[n - 1], s[n]
        assert before["in_flight"] >= 1 and r["reset"] and len(r["groups"]) <= 1
        assert any(x["pending"] for x in s[:n]) == (group_max > 1)
        # speculation is off until a render has been continued again -- except in the resetting
        # render itself when only the depth or the tiling changed: its seed continues the
        # sequence, which is all `speculate` asks (the rule as it stands in the engine)
        same_seed = stop in ("depth", "key")
        assert [x["speculate"] for x in s[n:]] == [same_seed, False, True, True]
        assert all(x["ahead_groups"] == 0 for x in s[n + (1 if same_seed else 0):n + 2])


@pytest.mark.parametrize("frame_paths", [4e5, 0.0])
def test_moving_camera_starts_nothing_ahead(drivers, frame_paths):
    script = [knobs(group_paths=4 * P - 1, frame_paths=frame_paths)]
    for i in range(8):
        script += ["invalidate", render(i, depth=5)]
    s = check(walk(drivers, script))
    for r in s:
        assert r["ahead_groups"] == 0 and r["need"] == P and r["in_flight"] == 0 and not r["speculate"]
        assert r["shortcut"] == int(frame_paths > 0)
        if not r["shortcut"]:
            assert (r["L"], r["own_frames"], r["traces"]) == (5, 1, 5)


@pytest.mark.parametrize("ramp", [0, 1])
def test_ramp_limits_the_first_speculating_render(drivers, ramp):
    s = check(walk(drivers, [knobs(group_paths=4 * P - 1, group_max=4, ramp=ramp)] + sequence(4, depth=8)))
    first = next(r for r in s if r["speculate"])
    if ramp:
        assert first["own_frames"] == 1 and first["ahead_groups"] <= 1
    else:
        assert first["own_frames"] == 4 and first["ahead_groups"] > 1


def test_oom_shrinks_slots_then_frames(drivers):
    kn = knobs(group_paths=4 * P - 1, group_max=4)
    s = check(walk(drivers, [kn, "fail 100", render(0, hint=1, depth=8)]))
    assert s[0]["oom"] and [(x["K"], x["G"]) for x in s[0]["shrinks"]] == [(4, 4), (2, 4), (1, 4), (1, 2), (1, 1)]
    # three failures: the ring ends at one slot of four frames, and the sequence runs on it
    s = check(walk(drivers, [kn, "fail 3", render(0, hint=1, depth=8)]))
    assert (s[0]["K"], s[0]["G"], s[0]["need"]) == (1, 4, 8 * 4 * P) and not s[0]["oom"]
    # a render that does not speculate has nothing to shrink
    s = check(walk(drivers, [kn, "fail 1", render(0, depth=8)]))
    assert s[0]["oom"] and not s[0]["shrinks"]


@pytest.mark.parametrize("depth,pipe_paths", [(8, 64e6), (8, 1e12), (63, 1e12)])
def test_ring_stays_below_2_31_paths(drivers, depth, pipe_paths):
    """133 M paths per frame (config 5): K G paths < 2^31 whatever the budgets allow."""
    n = 133_000_000
    s = check(walk(drivers, [knobs(paths=pipe_paths, budget=1e15)] +
                   [render(i, hint=1, depth=depth, paths=n, pixels=n) for i in range(3)]))
    assert s[0]["K"] == (1 if pipe_paths == 64e6 else min(depth, (2 ** 31 - 1) // n))
