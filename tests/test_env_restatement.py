"""Env-emitter sampling of the oracle pinned by float64 restatements (render/emitter/env.h:23-64
and 70-84, world/emitter.cpp:107-149; sampling_cases.py holds them).

The engine is bit-identical to the oracle on these very inputs (test_gpu_sampling_probes.py);
this file pins the oracle, on maps of 16 x 8, 5 x 3 and 64 x 2 texels:
  * SampleDirect at the middle of every texel's CDF cell, the bottom row included;
  * row index h (every xi.x past row_cdf[h - 1]): pdf exactly 0, the same in every process --
    the column walk and the row weight of that row read the table block's defined tail;
  * Eval on a lat-long grid, the poles and the axes;
  * the Eval pdf's integral over the sphere against the restatement's own;
  * the constant env's hemisphere sampling.

Integral of the restatement's Eval pdf by midpoint quadrature on a grid 8 x finer than the map
(printed by the test): 16 x 8: 1.59978, 5 x 3: 1.07787, 64 x 2: 1.50000 -- not 1.  The pdf takes
the luminance of radiance * scale (1.5 here) while `normalization` is built from the unscaled
texels (emitter.cpp:107-149), the row weights are lerped between row centres and extrapolated
below the last one (negative there), and the radiance is bilinear: the reference's own
discretisation, restated as it stands.
Test infrastructure only; CPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import sampling_cases as sc

P = np.float32([0.3, 0.0, 0.2])
N = np.float32([0.0, 1.0, 0.0])


@pytest.fixture(scope="module", params=sc.ENV_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def env(request):
    desc = sc.env_scene(*request.param)
    return oracle.OracleScene(desc), sc.Env64(desc), desc


def oracle_sample(orc, xi):
    return np.array([orc.emitter_sample(0, P, N, x) for x in xi])  # emitter 0 = env: no area emitters


def test_tables_follow_the_texels(env):
    """The restated BuildEnvMapCdfTable on the texels the desc carries: shapes, monotone CDFs
    ending at 1, the floor on the luminance, scale and rotation as the scene states them."""
    _, e, desc = env
    assert desc.num_area_emitters == 0 and e.tex.filter == 1
    assert (e.tex.texels @ sc.LUM).min() >= 0.05
    assert e.col_cdf.shape == (e.h, e.w + 1) and e.row_cdf.shape == (e.h + 1,)
    assert (np.diff(e.col_cdf, axis=1) > 0).all() and (np.diff(e.row_cdf) > 0).all()
    assert (e.col_cdf[:, 0] == 0).all() and (e.col_cdf[:, -1] == 1).all() and e.row_cdf[0] == 0 and e.row_cdf[-1] == 1
    assert e.scale == sc.ENV_SCALE
    c, s = np.cos(np.deg2rad(30)), np.sin(np.deg2rad(30))
    assert np.allclose(e.to_world, [[c, 0, s], [0, 1, 0], [-s, 0, c]], atol=1e-6)
    assert np.allclose(e.to_world @ e.to_local, np.eye(3), atol=1e-6)


def test_sample_direct_every_cell(env):
    orc, e, _ = env
    xi = sc.env_cell_xi(e)
    wi, pdf, rad, rows, cols = sc.env_sample_direct64(e, xi)
    # each xi is clear of the CDF entries either side of it, in the tables its searches walk
    for (x, y), row, col in zip(xi.astype(np.float64), rows, cols):
        assert np.abs(e.row_cdf - x).min() >= 1e-5
        seg = e.block[row * (e.w + 1): row * (e.w + 1) + e.w - 1]
        assert np.abs(seg - y).min() >= 1e-5, (row, col)
    # every row index the search can return for xi.x > 0 is drawn, the last (h) included; the
    # column walk of row index r reads the CDF of texel row r (row_cdf itself for r = h)
    assert set(rows.tolist()) == set(range(1, e.h + 1)) and cols.min() >= 1 and cols.max() == e.w - 1
    got = oracle_sample(orc, xi)
    assert np.isfinite(got).all()
    assert np.allclose(got[:, 0:3], wi, atol=2e-6, rtol=0)
    assert np.allclose(got[:, 3], pdf, rtol=1e-4, atol=0)
    assert np.allclose(got[:, 5:8], rad, rtol=1e-4, atol=0)
    assert (got[rows < e.h, 3] > 0).all() and (got[rows == e.h, 3] == 0).all()
    assert (got[:, 4] == got[0, 4]).all() and got[0, 4] > 1e15  # MAX_DISTANCE


def test_last_row_has_pdf_zero(env):
    orc, e, _ = env
    xi = sc.env_last_row_xi(e)
    assert (xi[:, 0] > e.row_cdf[e.h - 1]).all() and (xi[:, 0] <= 1).all()
    wi, pdf, rad, rows, _ = sc.env_sample_direct64(e, xi)
    assert (rows == e.h).all() and (pdf == 0).all()
    got = oracle_sample(orc, xi)
    assert np.isfinite(got).all()
    assert (got[:, 3] == 0.0).all() and not np.signbit(got[:, 3]).any()
    assert np.allclose(got[:, 0:3], wi, atol=2e-6, rtol=0)
    assert np.allclose(got[:, 5:8], rad, rtol=1e-4, atol=0)
    assert np.array_equal(got, oracle_sample(orc, xi))


DUMP = """
import sys
sys.path[:0] = {paths!r}
import numpy as np, oracle, sampling_cases as sc
out = []
for w, h in sc.ENV_SIZES:
    desc = sc.env_scene(w, h)
    orc, e = oracle.OracleScene(desc), sc.Env64(desc)
    out.append(np.array([orc.emitter_sample(0, {p!r}, {n!r}, x) for x in sc.env_last_row_xi(e)], np.float32))
sys.stdout.write(np.concatenate(out).tobytes().hex())
"""


def test_last_row_is_the_same_in_every_process():
    """What row h reads is defined data, not whatever lies behind an allocation: two fresh
    processes return the same bits as each other and as this one, for all three maps."""
    code = DUMP.format(paths=[sc.ROOT, os.path.join(sc.ROOT, "tests")], p=P.tolist(), n=N.tolist())
    runs = [subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120) for _ in range(2)]
    for r in runs:
        assert r.returncode == 0, r.stderr
    here = []
    for w, h in sc.ENV_SIZES:
        desc = sc.env_scene(w, h)
        here.append(oracle_sample(oracle.OracleScene(desc), sc.env_last_row_xi(sc.Env64(desc))).astype(np.float32))
    here = np.concatenate(here)
    assert (here[:, 3] == 0).all()
    assert runs[0].stdout == runs[1].stdout == here.tobytes().hex()


def test_eval_grid_poles_and_axes(env):
    orc, e, _ = env
    dirs = sc.env_eval_dirs(e)
    rad, pdf, t, pdf_terms = sc.env_eval64(e, dirs, want_row_t=True)
    skip = np.abs(t - np.round(t)) < 1e-4  # the row index may legitimately differ there
    assert not skip[:-6].any(), "the grid is chosen off the texel rows"
    assert skip.sum() <= 0.01 * len(dirs)
    got = orc.env_eval(dirs)
    assert np.isfinite(got).all()
    # Below the centre of the bottom row the reference extrapolates the row weight (row clamped
    # to h - 2, lerp factor past 1) and its Eval pdf goes negative: restated as it stands.
    assert (got[t <= e.h - 1, 3] > 0).all()
    keep = ~skip
    assert np.allclose(got[keep, 0:3], rad[keep], rtol=1e-4, atol=0)
    assert np.allclose(got[keep, 3], pdf[keep], rtol=1e-4, atol=0)
    # The exact poles fall under the skip (tex.y * h = 0 and h).  There the denominator sits at
    # its 1e-4 floor and, at -Y, the extrapolated row weight w0 + f (w1 - w0) cancels (to exactly
    # 0 for 3 rows), so the same 1e-4 is taken relative to the sum's terms |w0| + |f (w1 - w0)|.
    assert skip[-6:-4].all()
    assert (np.abs(got[-6:-4, 3] - pdf[-6:-4]) <= 1e-4 * pdf_terms[-6:-4]).all()
    assert np.allclose(got[-6:-4, 0:3], rad[-6:-4], rtol=1e-4, atol=0)


def test_eval_pdf_quadrature(env):
    """Midpoint quadrature of the Eval pdf over the sphere: the oracle's equals the
    restatement's (a swapped w / h or a missing scale in `normalization` shifts it)."""
    orc, e, _ = env
    dirs, weight = sc.env_quadrature_dirs(e)
    _, pdf = sc.env_eval64(e, dirs)
    ref = float((pdf * weight).sum())
    got = float((orc.env_eval(dirs)[:, 3].astype(np.float64) * weight).sum())
    print(f"env {e.w}x{e.h}: integral of the Eval pdf, restatement {ref:.5f}, oracle {got:.5f}")
    assert np.isclose(got, ref, rtol=1e-4, atol=0)


def test_pole_direction_past_one_stays_finite():
    """to_local = (1 + 2^-20) I: a unit +-Y has |dir.y| > 1 in Eval, where acos is undefined;
    the clamp gives theta = 0 / pi and a finite pdf (the GPU probe returns the same bits)."""
    desc = sc.set_pole_overshoot(sc.env_scene(16, 8))
    got = oracle.OracleScene(desc).env_eval(sc.POLES_AND_AXES[:2])
    assert np.isfinite(got).all()
    e = sc.Env64(desc)
    rad, pdf, _, pdf_terms = sc.env_eval64(e, sc.POLES_AND_AXES[:2], want_row_t=True)
    assert np.allclose(got[:, 0:3], rad, rtol=1e-4, atol=0) and (np.abs(got[:, 3] - pdf) <= 1e-4 * pdf_terms).all()


def test_const_env_hemisphere():
    desc = sc.const_env_scene()
    orc = oracle.OracleScene(desc)
    color = [desc.env.contents.color[k] for k in range(3)]
    xi = sc.hemisphere_xi()
    for n in sc.HEMI_FRAMES:
        wi, pdf = sc.uniform_hemisphere64(xi, n)
        got = np.array([orc.emitter_sample(0, P, n, x) for x in xi])
        assert np.allclose(got[:, 0:3], wi, atol=2e-6, rtol=0)
        assert np.allclose(got[:, 3], pdf, rtol=1e-6, atol=0)
        assert np.isclose(pdf.max(), 1.0 / (2.0 * np.pi), rtol=1e-6) and (pdf == 0).sum() == 1  # xi.x = 0.5: z = 0
        assert (np.einsum("ij,j->i", got[:, 0:3].astype(np.float64), n.astype(np.float64)) >= -1e-6).all()
        assert np.allclose(got[:, 5:8], color)
    ev = orc.env_eval(sc.POLES_AND_AXES)
    assert np.allclose(ev[:, 3], 1.0 / (4.0 * np.pi), rtol=1e-6) and np.allclose(ev[:, 0:3], color)
