"""Fixtures of the reference's own scene files (data/static/*.xml of vymv/PupilOptixLab).

Each XML is loaded by this repo's XML loader (pupiloptixlab_amd.World: the
mitsuba subset of resource/scene.cpp:27-227, shapes of resource/shape.cpp,
emitter tables of world/emitter.cpp:77-337) and the flattened scene is stored
as numbers (pupiloptixlab_amd.scene_io): meshes, material and instance records,
emitter tables, camera matrices.  The XML text itself is not kept.  The GPU
tests render these scenes without the reference tree.

`renders` records what the oracle renders from each freshly loaded XML (the
pixels and film size of tests/test_ref_scenes.py::test_fixture_matches_fresh_xml_load)
in ref_scenes_xml_render.npz, so that test needs no reference tree either.

usage (with a checkout of the reference at REF):
    python tests/golden/make_ref_scenes.py REF/data/static            # scene fixtures + renders
    python tests/golden/make_ref_scenes.py REF/data/static renders    # renders only
"""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import oracle  # noqa: E402
from pupiloptixlab_amd import World, scene_io  # noqa: E402


def main(src, fixtures=True):
    from test_ref_scenes import SMALL, XML_SPP, XML_STRIDE

    out_dir = os.path.join(HERE, "ref_scenes")
    os.makedirs(out_dir, exist_ok=True)
    renders = {}
    for path in sorted(glob.glob(os.path.join(src, "*.xml"))):
        name = os.path.splitext(os.path.basename(path))[0]
        desc = World().load_scene(path).desc()
        if fixtures:
            scene_io.save_desc(desc, os.path.join(out_dir, name + ".npz"))
        xml = scene_io.LoadedScene.__new__(scene_io.LoadedScene)
        xml.desc = desc
        small = scene_io.LoadedScene.resized(xml, *SMALL[name])
        px = np.arange(0, small.width * small.height, XML_STRIDE, dtype=np.uint32)
        renders[name] = oracle.OracleScene(small).render(spp=XML_SPP, pixels=px)["accum"]
        renders[name + "_size"] = np.array(SMALL[name], np.int32)
        print(name, desc.width, desc.height, desc.max_depth, desc.num_instances, desc.num_area_emitters)
    np.savez_compressed(os.path.join(HERE, "ref_scenes_xml_render.npz"), **renders)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], fixtures=sys.argv[2:] != ["renders"])
