"""csrc/host/prim_tables.h, the host half of pupil_pt_replace_shape_mesh, without a GPU: the
stand-alone driver prim_tables_driver.cpp compares the prefix sums, the guide's geometry and the
per-primitive lookup the fill kernel runs with the tables pupil_pt_create builds from an explicit
prim_inst array.  It is built with -fsanitize=address,undefined and fills exactly sized arrays, so
an index past an end, an overflow or a wrong entry fails the run."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pupiloptixlab_amd", "csrc")


def test_prim_tables_equal_the_tables_of_create(tmp_path):
    exe = tmp_path / "prim_tables_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(HERE, "prim_tables_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr)
