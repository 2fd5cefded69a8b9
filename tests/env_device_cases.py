"""Scenes and inputs of test_env_device.py: the 8 x 8 film of sampling_cases.env_scene under an env
map whose texels, rotation and scale the caller chooses.  Every world here writes its own PFM (and
XML) under build/test_scenes, with its own seed, so a "fresh engine" is one created from a World
that loaded the new texels from disk.  Test infrastructure only."""
import os

import numpy as np

import re

from pupiloptixlab_amd import World, abi, scenes
from sampling_cases import ROOT, TMP

# the values a wave of pt_envmap.hip stages per chunk of a chain, read from the kernels' header
ENV_STAGE = int(re.search(r"constexpr uint32_t kEnvStage = (\d+);",
                          open(os.path.join(ROOT, "pupiloptixlab_amd", "csrc", "pt_kernels.h")).read()).group(1))

# (w, h): the smallest map; an odd size; two rows; a power of two; a row that crosses one LDS stage
# of the chain and is no multiple of 4; more rows than a wave has lanes (and than two waves), odd width
SIZES = [(2, 2), (5, 3), (64, 2), (16, 8), (ENV_STAGE + 6, 3), (7, 130)]
RENDER_SIZE = (16, 8)
ROTATION = '<rotate y="1" angle="30"/>'
SCALE = 1.5


def texels(w, h, seed):
    """(h, w, 3) float32 drawn as sampling_cases.env_map_texels draws them -- every channel in
    [0.08, 1), a bright 2 x 2 patch -- from this module's own seed: no row sums to zero."""
    rng = np.random.Generator(np.random.PCG64(77000 + 1000 * seed + 31 * w + h))
    env = rng.uniform(0.08, 1.0, (h, w, 3)).astype(np.float32)
    r0, c0 = min(1, h - 2), w // 2
    env[r0:r0 + 2, c0:c0 + 2] = (30.0, 25.0, 18.0)
    return env


def env_world(rgb, name, rotation=ROTATION, scale=SCALE):
    """World of one rectangle under the env map `rgb` ((h, w, 3) float32), written to
    build/test_scenes/env_device_<name>.pfm; rotation: the XML of the emitter's to_world."""
    os.makedirs(TMP, exist_ok=True)
    env_file = f"env_device_{name}.pfm"
    scenes._write_pfm(os.path.join(TMP, env_file), rgb)
    xml = os.path.join(TMP, f"env_device_{name}.xml")
    with open(xml, "w") as f:
        f.write("\n".join([
            '<scene version="3.0.0">',
            '  <integrator type="path"><integer name="max_depth" value="2"/></integrator>',
            '  <sensor type="perspective"><float name="fov" value="45"/>',
            '    <transform name="to_world"><lookat origin="0, 2, 6" target="0, 0, 0" up="0, 1, 0"/></transform>',
            '    <film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="8"/></film>',
            '  </sensor>',
            f'  <emitter type="envmap"><string name="filename" value="{env_file}"/>'
            f'<float name="scale" value="{scale}"/>',
            f'    <transform name="to_world">{rotation}</transform></emitter>',
            '  <shape type="rectangle"><transform name="to_world"><rotate x="1" angle="-90"/></transform>',
            '    <bsdf type="diffuse"><rgb name="reflectance" value="0.5, 0.5, 0.5"/></bsdf></shape>',
            '</scene>']))
    return World().load_scene(xml)


def desc_texels(desc):
    """(h, w, 4) float32 copy of the env map's texels as the desc holds them: what a fresh engine
    is created from, and so what the device path is given."""
    t = desc.env.contents.radiance
    assert desc.env.contents.type == abi.EMITTER_ENV_MAP and t.type == abi.TEX_BITMAP
    return np.ctypeslib.as_array(t.rgba, shape=(t.height * t.width * 4,)).reshape(t.height, t.width, 4).copy()


def probe_xi(row_cdf):
    """256 xi pairs for SampleDirect: 0 and 1, xi.x above row_cdf[h - 1] (the row index is then h),
    and uniform draws."""
    rng = np.random.Generator(np.random.PCG64(5151))
    xi = rng.uniform(0.0, 1.0, (256, 2)).astype(np.float32)
    last = np.float32(row_cdf[-2])
    above = [np.nextafter(last, np.float32(2.0)), np.float32(0.5) * (last + np.float32(1.0)), np.float32(1.0 - 2.0 ** -24),
             np.float32(1.0)]
    xi[0], xi[1], xi[2] = (0.0, 0.0), (1.0, 1.0), (0.0, 1.0)
    for k, x in enumerate(above):
        xi[3 + 2 * k] = (x, 0.0)
        xi[4 + 2 * k] = (x, 0.61)
    return xi


def probe_dirs():
    """256 unit directions for Eval, both poles and the axes included."""
    rng = np.random.Generator(np.random.PCG64(6161))
    d = rng.normal(size=(256, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    d[:6] = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1]]
    return d
