"""csrc/host/material_tables.h, the one owner of the engine's materials, without a GPU: the
stand-alone driver material_tables_driver.cpp puts a counting allocator in place of the device and
walks create then drop, a scene without materials, stage then drop, stage then commit then the drop
of the replaced texels, the reuse of a same-size bitmap, bitmap to constant and back, a size change,
an id named twice, an allocation failing at each position of a three-bitmap update, a write failing
between two materials and the refusals.  It is built with -fsanitize=address,undefined, so a leak, a
double free or a use after free fails the run."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pupiloptixlab_amd", "csrc")


def test_materials_have_one_owner_on_every_path(tmp_path):
    exe = tmp_path / "material_tables_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(HERE, "material_tables_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr)
