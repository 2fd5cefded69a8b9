"""pupil_pt_set_instances without a GPU: the world edits that feed it (World.remove_instance /
add_instance against a world built that way from the start, description field by field), the ABI
symbols, and the record assembly the host mirror and the fill kernel share
(csrc/host/instance_record.h), run by the stand-alone driver instance_set_driver.cpp under
-fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pupiloptixlab_amd import abi

import instance_set_cases as cases
from instance_set_cases import BASE, LAMP_INSTANCE

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pupiloptixlab_amd", "csrc")


def _struct_values(s, skip=()):
    out = {}
    for name, typ in s._fields_:
        if name in skip:
            continue
        if isinstance(typ, type(C.POINTER(C.c_int))) or typ in (C.c_void_p, C.c_char_p):
            continue  # pointers: every world owns its arrays
        v = getattr(s, name)
        if isinstance(v, C.Array):
            out[name] = bytes(v)
        elif isinstance(v, C.Structure):
            out[name] = _struct_values(v, skip)
        else:
            out[name] = v
    return out


def _description(w):
    """every field of the scene description that an instance edit can touch, as plain values"""
    d = w.desc()
    out = {"counts": (d.num_shapes, d.num_materials, d.num_instances, d.num_area_emitters, d.width, d.height, d.max_depth),
           "camera": (bytes(d.sample_to_camera), bytes(d.camera_to_world)), "env": bool(d.env)}
    out["instances"] = [_struct_values(d.instances[i]) for i in range(d.num_instances)]
    out["materials"] = [bytes(d.materials[i]) for i in range(d.num_materials)]
    out["emitters"] = [_struct_values(d.area_emitters[i]) for i in range(d.num_area_emitters)]
    out["shapes"] = [(d.shapes[i].kind, d.shapes[i].num_vertices, d.shapes[i].num_faces) for i in range(d.num_shapes)]
    out["masks"] = [w.instance_visibility(i) for i in range(d.num_instances)]
    return out


def _same_description(a, b):
    da, db = _description(a), _description(b)
    assert da.keys() == db.keys()
    for k in da:
        assert da[k] == db[k], k


def test_abi_exposes_the_symbols():
    lib = abi.load_library()
    for name in ("pupil_pt_set_instances", "pupil_pt_set_instances_info", "pupil_world_remove_instance"):
        assert hasattr(lib, name), name
    assert abi.INSTANCES_DEVICE == 1
    assert lib.pupil_pt_set_instances(None, 0, None, None, None, 0, None) == abi.ERR_INVALID
    assert lib.pupil_pt_set_instances_info(None, None, None, None, None) == abi.ERR_INVALID


@pytest.mark.parametrize("removed", [0, 1, 2, 3, 5])
def test_removed_instance_equals_a_world_built_without_it(removed):
    w = cases.world(BASE)
    w.remove_instance(removed)
    _same_description(w, cases.world(BASE[:removed] + BASE[removed + 1:]))


def test_removing_the_lamp_rebuilds_the_emitters():
    w = cases.world(BASE + (cases.SECOND_LAMP,))
    before = w.desc().num_area_emitters
    w.remove_instance(LAMP_INSTANCE)
    assert 0 < w.desc().num_area_emitters < before
    _same_description(w, cases.world(BASE[:LAMP_INSTANCE] + BASE[LAMP_INSTANCE + 1:] + (cases.SECOND_LAMP,)))


def test_added_instance_equals_a_world_built_with_it():
    w = cases.world(BASE)
    w.desc()  # a description was handed out before the edit
    for extra in (cases.EXTRA_A, cases.HIDDEN_SPHERE, cases.SECOND_LAMP):
        cases.add(w, extra)
    _same_description(w, cases.world(BASE + (cases.EXTRA_A, cases.HIDDEN_SPHERE, cases.SECOND_LAMP)))
    w.remove_instance(len(BASE) + 1)  # the hidden sphere: the mask goes with it
    w.remove_instance(1)
    _same_description(w, cases.world(BASE[:1] + BASE[2:] + (cases.EXTRA_A, cases.SECOND_LAMP)))


def test_remove_out_of_range_is_refused():
    w = cases.world(BASE)
    with pytest.raises(abi.PupilError) as e:
        w.remove_instance(len(BASE))
    assert e.value.code == abi.ERR_INVALID
    _same_description(w, cases.world(BASE))


def test_record_assembly_equals_the_records_of_create(tmp_path):
    exe = tmp_path / "instance_set_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-O1", "-g",
                        "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(HERE, "instance_set_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr)
