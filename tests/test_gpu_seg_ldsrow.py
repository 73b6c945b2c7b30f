"""GPU: the scatters whose item row fits LDS (csrc/segsum.hip, the LDS-row apply:
one block per (batch, channel) stages in[b, c, :] in sorted order in LDS and
sums every voxel's segment from there) -- avg_voxelize_fwd and
trilinear_devoxelize_bwd, planned and unplanned.

  * against the oracle with the bar of tests/test_gpu_ops.py (ind / cnt
    bit-exact, float sums rtol 1e-5), and for the smallest shapes against a
    direct fp64 torch index_add;
  * every output element written (the outputs are NaN-filled before each call,
    tests/helpers/seg_ldsrow_cases.py) and two calls bit-equal (asserted by the
    runners there);
  * against the transposing engine (PCFM_SEG_LDSROW=0, a child process: the
    switch is read once) on every shape -- the voxelization to the bit: the
    LDS-row apply adds in that engine's order -- one of them the longest row
    that fits and one a single item longer;
  * the devoxelization backward is the forward's adjoint;
  * grouping backward (key = neighbour index, V = n rows) on both engines: equal
    bits, and every element within the first-order bound of an fp32 sum of its
    terms in any order around a float64 np.add.at.

The runners compute every case once per process; the tests share the results.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import seg_ldsrow_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def new():
    from pcfm import _lib
    _lib.load()
    assert torch.cuda.is_available()
    assert os.environ.get("PCFM_SEG_LDSROW", "1") != "0", "the suite runs the default path"
    return cases.run_all()


@pytest.fixture(scope="module")
def old(tmp_path_factory):
    path = tmp_path_factory.mktemp("seg_ldsrow") / "old.npz"
    env = dict(os.environ, PCFM_SEG_LDSROW="0")
    subprocess.run([sys.executable, os.path.join(HERE, "helpers", "seg_ldsrow_cases.py"),
                    str(path)], check=True, timeout=300, env=env,
                   cwd=os.path.dirname(HERE))
    return np.load(path)


def _vox_fp64(feat, ind, cnt, s):
    """out[b, c, v] = sum of feat[b, c, i] over ind[b, i] == v, / cnt[b, v]."""
    b, c, _ = feat.shape
    out = torch.zeros((b, c, s), dtype=torch.float64)
    f = torch.from_numpy(feat).double()
    for k in range(b):
        out[k].index_add_(1, torch.from_numpy(ind[k]).long(), f[k])
    return (out / torch.from_numpy(cnt).double().clamp(min=1)[:, None, :]).numpy()


def _devox_fp64(gy, inds, wgts, s):
    """gx[b, c, v] = sum over (i, k) with inds[b, k, i] == v of wgts[b, k, i] *
    gy[b, c, i]; a corner outside [0, s) contributes nothing."""
    b, c, _ = gy.shape
    gx = torch.zeros((b, c, s), dtype=torch.float64)
    g = torch.from_numpy(gy).double()
    for k in range(b):
        for t in range(8):
            i = torch.from_numpy(inds[k, t]).long()
            ok = (i >= 0) & (i < s)
            w = torch.from_numpy(wgts[k, t]).double() * ok
            gx[k].index_add_(1, i.clamp(0, max(s - 1, 0)), g[k] * w[None, :])
    return gx.numpy()


@pytest.mark.parametrize("name", list(cases.VOX))
def test_avg_voxelize_fwd(new, name):
    feat, coords, r = cases.vox_inputs(name)
    e_out, e_ind, e_cnt = O.avg_voxelize_fwd(feat, coords, r)
    np.testing.assert_array_equal(new[f"vox.{name}.ind"], e_ind)
    np.testing.assert_array_equal(new[f"vox.{name}.cnt"], e_cnt)
    for k in ("out", "out_planned"):
        got = new[f"vox.{name}.{k}"]
        assert not np.isnan(got).any(), f"{k}: an output element was not written"
        np.testing.assert_allclose(got, e_out, rtol=1e-5, atol=1e-6, err_msg=k)
    np.testing.assert_array_equal(new[f"vox.{name}.out"], new[f"vox.{name}.out_planned"])
    if name in cases.FP64_CASES:
        ref = _vox_fp64(feat, e_ind, e_cnt, r ** 3)
        np.testing.assert_allclose(new[f"vox.{name}.out"], ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", list(cases.DEVOX))
def test_trilinear_devoxelize_bwd(new, name):
    gy, pts, r = cases.devox_inputs(name)
    grid = cases.devox_grid(name)
    e_fwd, e_inds, e_wgts = O.trilinear_devoxelize_fwd(pts, grid, r, True)
    np.testing.assert_array_equal(new[f"devox.{name}.inds"], e_inds)
    np.testing.assert_array_equal(new[f"devox.{name}.wgts"], e_wgts)
    e_gx = O.trilinear_devoxelize_bwd(gy, e_inds, e_wgts, r)
    scale = max(1.0, float(np.abs(e_gx).max())) if e_gx.size else 1.0
    for k in ("gx", "gx_planned"):
        got = new[f"devox.{name}.{k}"]
        assert not np.isnan(got).any(), f"{k}: an output element was not written"
        np.testing.assert_allclose(got, e_gx, rtol=1e-5, atol=1e-6 * scale, err_msg=k)
    np.testing.assert_array_equal(new[f"devox.{name}.gx"], new[f"devox.{name}.gx_planned"])
    if name in cases.FP64_CASES:
        ref = _devox_fp64(gy, e_inds, e_wgts, r ** 3)
        np.testing.assert_allclose(new[f"devox.{name}.gx"], ref, rtol=1e-5, atol=1e-6 * scale)
    # adjoint: <fwd(grid), gy> == <grid, bwd(gy)>
    lhs = float((new[f"devox.{name}.fwd"].astype(np.float64) * gy).sum())
    rhs = float((grid.astype(np.float64) * new[f"devox.{name}.gx"]).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs)), (lhs, rhs)


@pytest.mark.parametrize("name", list(cases.GROUP))
def test_grouping_bwd(new, old, name):
    """Both engines return the same bits (two calls of each too: asserted by the
    runner), every element written, each within k * 2^-24 * sum |term| of the
    float64 sum (k the row's item count; helpers/seg_ldsrow_cases.py)."""
    ref, bound = cases.group_reference(name)
    for tag, got in (("lds-row", new[f"group.{name}.gx"]),
                     ("transposing", old[f"group.{name}.gx"])):
        assert got.shape == ref.shape, tag
        assert not np.isnan(got).any(), f"{tag}: an output element was not written"
        err = np.abs(got.astype(np.float64) - ref)
        print(f"group {name} {tag}: max err / bound = "
              f"{float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0:.3g}")
        assert (err <= bound).all(), (tag, float((err - bound).max()))
    np.testing.assert_array_equal(new[f"group.{name}.gx"], old[f"group.{name}.gx"])


def test_new_path_matches_transposing_engine(new, old):
    """Within 1e-5 on every shape; the voxelization, which the LDS-row apply
    sums piece by piece in the transposing engine's own order, to the bit."""
    for key in old.files:
        a, b = new[key], old[key]
        assert a.shape == b.shape, key
        assert not np.isnan(b).any(), f"{key}: the transposing engine left an element unwritten"
        scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6 * scale, err_msg=key)
        if key.startswith("vox."):
            np.testing.assert_array_equal(a, b, err_msg=key)


def test_fit_threshold(new):
    """The longest row that fits LDS (the LDS-row apply) against the same cloud
    with one more point (the transposing engine): equal wherever the extra point
    does not contribute."""
    feat, coords, r = cases.vox_inputs("fit_above")
    assert feat.shape[2] == cases.LDS_ROW_MAX_ITEMS + 1
    below, above = new["vox.fit_below.out"], new["vox.fit_above.out"]
    v = (coords[:, 0, -1] * r + coords[:, 1, -1]) * r + coords[:, 2, -1]
    keep = np.ones(below.shape, bool)
    for k in range(below.shape[0]):
        keep[k, :, v[k]] = False
    np.testing.assert_allclose(above[keep], below[keep], rtol=1e-5, atol=1e-6)
    gy, pts, r = cases.devox_inputs("fit_above")
    below, above = new["devox.fit_below.gx"], new["devox.fit_above.gx"]
    extra = _devox_fp64(gy[:, :, -1:], new["devox.fit_above.inds"][:, :, -1:],
                        new["devox.fit_above.wgts"][:, :, -1:], r ** 3)
    scale = max(1.0, float(np.abs(below).max()))
    np.testing.assert_allclose(above, below + extra, rtol=1e-5, atol=1e-6 * scale)
