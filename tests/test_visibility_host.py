"""Instance visibility without a GPU: the new C-ABI entries, the counters layout, the world layer's
mask bookkeeping, and the filtered-desc helper of tests/test_visibility.py against the oracle alone."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import oracle
from pupiloptixlab_amd import World, abi, scenes
from test_visibility import filtered_desc, filtered_to_full_ids, prim_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("pupil_pt_update_instances_masked", "pupil_world_set_instance_visibility",
               "pupil_world_get_instance_visibility")


def test_new_entries_are_exported_and_declared():
    lib = abi.load_library()
    header = open(os.path.join(ROOT, "include", "pupil_pt.h")).read()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES and name + "(" in header, name
    assert lib.pupil_abi_version() == 7  # new entries are detected by symbol, not by version


def test_masked_update_rejects_null_arguments():
    lib = abi.load_library()
    ids = (C.c_uint32 * 1)(0)
    mask = (C.c_uint32 * 1)(0)
    assert lib.pupil_pt_update_instances_masked(None, 1, ids, None, None, mask) == abi.ERR_INVALID
    assert lib.pupil_pt_update_instances(None, 1, ids, None, None) == abi.ERR_INVALID


def test_counters_end_with_hidden_instances(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pupil_pt.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(pupil_pt_counters), '
                   'offsetof(pupil_pt_counters, hidden_instances)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off = map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(abi.Counters)
    assert off == abi.Counters.hidden_instances.offset == size - 8  # the last field
    assert "hidden_instances" in abi.Counters().as_dict()


def _cornell(tmp):
    return World().load_scene(scenes.cornell_xml(os.path.join(tmp, "cb_vis.xml"), 32, 32, 3))


def _desc_bytes(desc):
    parts = [bytes(desc)[: abi.SceneDesc.shapes.offset]]
    parts.append(C.string_at(desc.instances, C.sizeof(abi.Instance) * desc.num_instances))
    parts.append(C.string_at(desc.area_emitters, C.sizeof(abi.Emitter) * desc.num_area_emitters))
    return b"".join(parts)


def test_world_remembers_masks_and_desc_does_not_change():
    with tempfile.TemporaryDirectory(prefix="pupil_vis_") as tmp:
        w = _cornell(tmp)
        before = w.desc()
        n = before.num_instances
        raw = _desc_bytes(before)
        assert all(w.instance_visibility(i) == 1 for i in range(n))  # render_object.h:16
        w.set_instance_visibility(n - 1, 0)
        w.set_instance_visibility(1, 0x100)  # only the low 8 bits count for the engine; the world keeps the value
        assert w.instance_visibility(n - 1) == 0 and w.instance_visibility(1) == 0x100
        assert w.instance_visibility(0) == 1
        after = w.desc()
        assert (after.num_instances, after.num_area_emitters) == (n, before.num_area_emitters)
        assert _desc_bytes(after) == raw  # emitters stay, as in the reference
        lib = abi.load_library()
        out = C.c_uint32()
        assert lib.pupil_world_set_instance_visibility(w._h, n, 0) == abi.ERR_INVALID
        assert lib.pupil_world_get_instance_visibility(w._h, n, C.byref(out)) == abi.ERR_INVALID
        assert lib.pupil_world_get_instance_visibility(w._h, 0, None) == abi.ERR_INVALID
        assert lib.pupil_world_set_instance_visibility(None, 0, 0) == abi.ERR_INVALID
        w.set_instance_visibility(n - 1, 255)
        assert w.instance_visibility(n - 1) == 255
        w.load_scene(scenes.cornell_xml(os.path.join(tmp, "cb_vis.xml"), 32, 32, 3))
        assert w.instance_visibility(1) == 1  # a new scene: every instance visible


def test_filtered_desc_against_the_oracle():
    """Hiding a wall of the Cornell scene changes the image; hiding the light's instance leaves a
    non-black image (the emitter table is not filtered)."""
    with tempfile.TemporaryDirectory(prefix="pupil_vis_") as tmp:
        w = _cornell(tmp)
        desc = w.desc()
        n = desc.num_instances
        light = [i for i in range(n) if desc.instances[i].emitter_offset >= 0]
        assert len(light) == 1
        wall = next(i for i in range(n) if i not in light)
        full = oracle.OracleScene(desc).render(spp=2)["accum"]
        f = filtered_desc(desc, (wall,))
        assert f.num_instances == n - 1 and f.num_area_emitters == desc.num_area_emitters
        no_wall = oracle.OracleScene(f).render(spp=2)["accum"]
        assert np.isfinite(no_wall).all() and not np.array_equal(no_wall, full)
        no_light = oracle.OracleScene(filtered_desc(desc, light)).render(spp=2)["accum"]
        assert np.isfinite(no_light).all() and no_light[:, :3].max() > 0.0
        assert not np.array_equal(no_light, full)
        # the id map: dropping an instance shifts the later primitive ids down by its count
        cnt = prim_counts(desc)
        ids = filtered_to_full_ids(desc, (wall,))
        assert len(ids) == cnt.sum() - cnt[wall]
        first = int(np.cumsum(cnt)[wall - 1]) if wall else 0
        assert np.array_equal(ids[:first], np.arange(first))
        assert np.array_equal(ids[first:], np.arange(first + cnt[wall], cnt.sum()))
