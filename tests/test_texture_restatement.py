"""cuda::Texture::Sample of the oracle (cuda/texture.h:33-57; bitmaps read with normalized
coordinates, wrap addressing and tex2D's 8-bit bilinear weights, cuda/texture.cpp:82-88) pinned
by a float64 restatement (sampling_cases.tex_sample64), one material per texture under test.

The engine is bit-identical to the oracle on these very inputs (test_gpu_sampling_probes.py).
  * Exact lattice: 8 x 4 bitmaps, point and bilinear, identity to_uv, uv = m / 2048.  Every
    float32 step (t * W - 0.5, the weight floor(frac * 256 + 0.5) / 256) is exact there, so the
    texel choice and the weights cannot differ; only the float32 lerps round: rtol 1e-6.
  * General: a 5 x 3 bitmap, to_uv scale 3 and an offset, 20 000 uniform uv in [-1, 2]^2 at rtol
    1e-5, skipping only samples whose rounded quantity lies within 4e-3 of an integer, where
    float32 may take the neighbouring weight or texel.  The restatement's own skip rate for this
    seed: 1.650 % (point), 1.685 % (bilinear).
  * Checkerboard with to_uv scale 4 on the lattice: the exact colour.
Test infrastructure only; CPU.
"""
import numpy as np
import pytest

import oracle
import sampling_cases as sc


@pytest.fixture(scope="module")
def setup():
    desc, mats = sc.texture_scene()
    return oracle.OracleScene(desc), desc, mats


@pytest.mark.parametrize("name", ["lattice_point", "lattice_bilinear"])
def test_bitmap_exact_lattice(setup, name):
    orc, desc, mats = setup
    uv = sc.lattice_uv()
    tex = sc.material_tex64(desc, mats[name])
    assert (tex.w, tex.h) == (8, 4) and np.array_equal(tex.r0, [1, 0, 0, 0]) and np.array_equal(tex.r1, [0, 1, 0, 0])
    # the lattice holds what it is meant to: negative uv, 0 and 1 exactly, texel centres
    # ((k + 0.5) / W) and edges (k / W) on both axes, and more than one wrap either side
    for axis, size in ((0, 8), (1, 4)):
        vals = set(uv[:, axis].tolist())
        assert {-2.0, -1.0, 0.0, 1.0, 3.0, 1.5 / size, 3.0 / size, -0.5 / size} <= vals
    ref = sc.tex_sample64(tex, uv)
    got = orc.tex_sample(mats[name], 0, uv)
    assert np.allclose(got, ref, rtol=1e-6, atol=0)
    if name == "lattice_point":
        assert np.array_equal(got, ref.astype(np.float32))  # a fetched texel, untouched


@pytest.mark.parametrize("name", ["general_point", "general_bilinear"])
def test_bitmap_general(setup, name):
    orc, desc, mats = setup
    uv = sc.general_uv()
    tex = sc.material_tex64(desc, mats[name])
    assert (tex.w, tex.h) == (5, 3) and tex.r0[0] == 3 and tex.r1[1] == 3 and tex.r0[3] != 0 and tex.r1[3] != 0
    ref, margin = sc.tex_sample64(tex, uv, want_margin=True)
    skip = margin < 4e-3
    print(f"{name}: {100.0 * skip.mean():.3f} % of {len(uv)} samples skipped")
    assert skip.mean() <= 0.05
    got = orc.tex_sample(mats[name], 0, uv)
    assert np.allclose(got[~skip], ref[~skip], rtol=1e-5, atol=0)


def test_checkerboard_exact_colour(setup):
    orc, desc, mats = setup
    uv = sc.lattice_uv()
    tex = sc.material_tex64(desc, mats["checker"])
    assert tex.r0[0] == 4 and tex.r1[1] == 4
    t = 4.0 * uv.astype(np.float64)
    frac = t - np.trunc(t)
    # tx == 0.5 (strict >), integers (fraction 0) and negatives (truncated, then + 1) all occur
    assert (frac[:, 0] == 0.5).any() and (frac[:, 1] == 0.5).any() and (frac == 0).any() and (frac < 0).any()
    ref = sc.tex_sample64(tex, uv)
    got = orc.tex_sample(mats["checker"], 0, uv)
    assert np.array_equal(got, ref.astype(np.float32))
    c0, c1 = (np.float32(c) for c in sc.CHECKER_COLORS)
    first = (got == c0).all(axis=1)
    assert (first | (got == c1).all(axis=1)).all() and 0.4 < first.mean() < 0.6
    # spot values written out: fractions (0.5, 0.75) -> not > 0.5, > 0.5 -> colour1; (0.75, 0.75) -> colour0
    spot = orc.tex_sample(mats["checker"], 0, np.float32([[0.125, 0.1875], [0.1875, 0.1875], [-0.0625, 0.0], [0.0, 0.0]]))
    assert np.array_equal(spot, np.float32([c1, c0, c1, c0]))
