"""csrc/host/scoped_buffer.h, the BVH builder's device-scratch holder, without a GPU: the stand-alone
driver scoped_buffer_driver.cpp swaps hipMalloc / hipFree for a counting allocator and walks the
destructor, move, release and failed-sequence paths, and the same paths of the handle holder beside
it (events, the stream) with a counting destroy.  It is built with
-fsanitize=address,undefined, so a leak, a double free or a use after free fails the run."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pupiloptixlab_amd", "csrc")


def test_holder_frees_every_allocation_once(tmp_path):
    exe = tmp_path / "scoped_buffer_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-self-move", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(HERE, "scoped_buffer_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr)
