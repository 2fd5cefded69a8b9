"""csrc/host/emitter_tables.h, the one owner of the engine's emitter tables, their texels and the
device-side mode's bookkeeping, without a GPU: the stand-alone driver emitter_tables_driver.cpp puts
a counting allocator in place of the device and walks stage then drop, stage then adopt, three
replacing adoptions of a textured lamp and an env map (live allocations and bytes stay), the
in-place writers, an allocation failing at each position of both stagings and every refusal twice
in a row, and compares the staged CDF and guide with their definition.  It is built with
-fsanitize=address,undefined, so a leak, a double free or a use after free fails the run."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pupiloptixlab_amd", "csrc")


def test_emitters_have_one_owner_on_every_path(tmp_path):
    exe = tmp_path / "emitter_tables_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(HERE, "emitter_tables_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {k: v for k, v in os.environ.items() if k != "PUPIL_EMITTER_SELECT"}  # the driver expects the guide
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr)
