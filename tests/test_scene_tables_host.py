"""csrc/host/scene_tables.h, the one owner of the engine's instance and primitive tables, without a
GPU: the stand-alone driver scene_tables_driver.cpp puts a counting allocator in place of the device
and walks stage then drop, stage then adopt, two adoptions in a row, an allocation failing at each
of the four positions and the refusals, and compares the staged tables with the definition.  It is
built with -fsanitize=address,undefined, so a leak, a double free or a use after free fails the
run."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pupiloptixlab_amd", "csrc")


def test_tables_have_one_owner_on_every_path(tmp_path):
    exe = tmp_path / "scene_tables_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(HERE, "scene_tables_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr)
