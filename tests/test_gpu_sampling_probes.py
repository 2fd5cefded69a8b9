"""The device's env-emitter and texture sampling (pupil_debug_env, pupil_debug_tex_sample: one
thread per input through emitter_sample_direct, env_eval and tex_sample of pt_shading.h) against
the CPU oracle's probes, bit for bit, on exactly the inputs test_env_restatement.py and
test_texture_restatement.py pin the oracle with: every texel's CDF cell, row index h (the last
row), the lat-long grid, the poles and axes, the quadrature grid, all three map sizes; the
uv lattice, the general uv and the checkerboard."""
import numpy as np
import pytest

import oracle
import sampling_cases as sc
from pupiloptixlab_amd import abi

pytestmark = pytest.mark.gpu

P = np.float32([0.3, 0.0, 0.2])
N = np.float32([0.0, 1.0, 0.0])


def _engine(desc):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(desc)
    return pt


def gpu_env(pt, inputs, mode, pos=P, nrm=N):
    x = np.zeros((len(inputs), 3), np.float32)
    x[:, :inputs.shape[1]] = inputs
    pn = np.ascontiguousarray(np.concatenate([pos, nrm]), np.float32)
    out = np.zeros((len(x), 8), np.float32)
    abi.check(pt._lib.pupil_debug_env(pt._pt, len(x), x.ctypes.data_as(abi.f32p), pn.ctypes.data_as(abi.f32p), mode,
                                      out.ctypes.data_as(abi.f32p)))
    return out


def gpu_tex(pt, material, uv):
    uv = np.ascontiguousarray(uv, np.float32)
    out = np.zeros((len(uv), 3), np.float32)
    abi.check(pt._lib.pupil_debug_tex_sample(pt._pt, material, 0, len(uv), uv.ctypes.data_as(abi.f32p),
                                             out.ctypes.data_as(abi.f32p)))
    return out


def assert_bits(got, ref, what):
    mism = (got.view(np.uint32) != ref.view(np.uint32)).any(axis=1)
    assert not mism.any(), f"{what}: {int(mism.sum())} of {len(ref)} differ, first at {int(np.argmax(mism))}: " \
                           f"{got[np.argmax(mism)]} != {ref[np.argmax(mism)]}"


@pytest.mark.parametrize("size", sc.ENV_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_env_probes_match_oracle(size):
    desc = sc.env_scene(*size)
    orc, e = oracle.OracleScene(desc), sc.Env64(desc)
    xi = np.concatenate([sc.env_cell_xi(e), sc.env_last_row_xi(e)])
    dirs = np.concatenate([sc.env_eval_dirs(e), sc.env_quadrature_dirs(e)[0]])
    assert len(xi) <= 65536 and len(dirs) <= 65536
    pt = _engine(desc)
    try:
        got_s = gpu_env(pt, xi, 0)
        got_e = gpu_env(pt, dirs, 1, pos=np.zeros(3, np.float32))
    finally:
        pt.close_engine()
    ref_s = np.array([orc.emitter_sample(0, P, N, x) for x in xi], np.float32)
    assert_bits(got_s, ref_s, "SampleDirect")
    last = len(sc.env_cell_xi(e))
    assert (got_s[last:, 3] == 0).all() and np.isfinite(got_s).all()
    assert_bits(got_e[:, :4], orc.env_eval(dirs), "Eval")
    assert np.isfinite(got_e).all()


def test_env_pole_past_one_matches_oracle():
    """to_local = (1 + 2^-20) I takes dir.y of +-Y past 1: finite, and the same bits on both sides."""
    desc = sc.set_pole_overshoot(sc.env_scene(16, 8))
    ref = oracle.OracleScene(desc).env_eval(sc.POLES_AND_AXES)
    pt = _engine(desc)
    try:
        got = gpu_env(pt, sc.POLES_AND_AXES, 1, pos=np.zeros(3, np.float32))
    finally:
        pt.close_engine()
    assert np.isfinite(got).all()
    assert_bits(got[:, :4], ref, "Eval past the pole")


def test_const_env_probes_match_oracle():
    desc = sc.const_env_scene()
    orc = oracle.OracleScene(desc)
    xi = sc.hemisphere_xi()
    pt = _engine(desc)
    try:
        got = [gpu_env(pt, xi, 0, nrm=n) for n in sc.HEMI_FRAMES]
        got_e = gpu_env(pt, sc.POLES_AND_AXES, 1, pos=np.zeros(3, np.float32))
    finally:
        pt.close_engine()
    for n, g in zip(sc.HEMI_FRAMES, got):
        assert_bits(g, np.array([orc.emitter_sample(0, P, n, x) for x in xi], np.float32), f"hemisphere about {n}")
    assert_bits(got_e[:, :4], orc.env_eval(sc.POLES_AND_AXES), "const Eval")


def test_tex_probes_match_oracle():
    desc, mats = sc.texture_scene()
    orc = oracle.OracleScene(desc)
    lattice, general = sc.lattice_uv(), sc.general_uv()
    cases = [("lattice_point", lattice), ("lattice_bilinear", lattice), ("general_point", general),
             ("general_bilinear", general), ("checker", lattice)]
    pt = _engine(desc)
    try:
        got = []
        for name, uv in cases:
            out = np.concatenate([gpu_tex(pt, mats[name], uv[k:k + 65536]) for k in range(0, len(uv), 65536)])
            got.append(out)
        lib = pt._lib
        bad = np.zeros(3, np.float32)
        assert lib.pupil_debug_tex_sample(pt._pt, desc.num_materials, 0, 1, bad.ctypes.data_as(abi.f32p),
                                          bad.ctypes.data_as(abi.f32p)) == abi.ERR_INVALID
        assert lib.pupil_debug_env(pt._pt, 1, np.float32([1.5, 0, 0]).ctypes.data_as(abi.f32p),
                                   np.zeros(6, np.float32).ctypes.data_as(abi.f32p), 0,
                                   np.zeros(8, np.float32).ctypes.data_as(abi.f32p)) == abi.ERR_INVALID
    finally:
        pt.close_engine()
    for (name, uv), g in zip(cases, got):
        assert_bits(g, orc.tex_sample(mats[name], 0, uv), name)
