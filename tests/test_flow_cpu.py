"""The Farneback flow and the MESSDdt reduction without a GPU: the NumPy restatement (tests/flow_restatement.py) against the fixture that an
independent scipy.ndimage statement (flows) and the reference's own MESSDdt.update (reduction) wrote (tests/golden/flow_pinned.npz,
tests/golden/make_flow_golden.py), properties that do not hang on any detail of OpenCV, the Python surface, and the ISA of csrc/flow.hip."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import flow_restatement as R                                          # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import flow                                     # noqa: E402
from maggie_amd.utils import metric as dm                             # noqa: E402

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SMALL = [k for k, v in R.FLOW_CASES.items() if v[0] * v[1] < 100000]
_FLOWS = {}


def _flow64(name):
    """The fp64 restatement of a small case, computed once and left unchanged."""
    if name not in _FLOWS:
        h, w, shift, seed = R.FLOW_CASES[name]
        a, b = R.frame_pair(h, w, shift, seed)
        _FLOWS[name] = R.farneback(a, b, np.float64)
    return _FLOWS[name]


@pytest.mark.parametrize('name', SMALL)
def test_restatement_equals_the_scipy_statement(name):
    want = load_golden('flow_pinned.npz')['flow.' + name]
    got = _flow64(name)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize('name', sorted(R.REDUCTION_CASES))
def test_restated_reduction_equals_the_reference(name):
    ret, score, count, average = load_golden('flow_pinned.npz')['messddt.' + name]
    pred, gt, tri, flows = R.reduction_case(name)
    s, c = R.messddt(pred, gt, tri, flows)
    assert c == count
    assert s == pytest.approx(score, rel=1e-6, abs=0)
    if count:
        assert s / (c + 1e-8) == pytest.approx(ret, rel=1e-6) and s / (c + 1e-6) == pytest.approx(average, rel=1e-6)


def test_the_uint8_planes_cover_every_value():
    """(k / 255) * 255 in fp32 is not always k: the conversion is one fp32 multiply, truncated, whatever that gives."""
    k = np.arange(256)
    u8 = R.gt_u8(k.astype(np.float32) / np.float32(255))
    exact = (k.astype(np.float64) / 255 * 255).astype(np.uint8)
    assert u8.dtype == np.uint8 and (np.abs(u8.astype(int) - k) <= 1).all()
    assert np.array_equal(u8, ((k.astype(np.float32) / np.float32(255)) * np.float32(255)).astype(np.uint8))
    assert (u8 != k).any() or np.array_equal(u8, exact)                  # the truncation is visible wherever the product falls short of k
    _, gt, _, _ = R.reduction_case('f3_n2_8x32_all_values')
    assert all(len(np.unique(p)) == 256 for p in gt.reshape(-1, 256))


def test_zero_motion_gives_exactly_zero_flow():
    assert not _flow64('131x150_still').any()
    a, _ = R.frame_pair(40, 36, (0.0, 0.0), 1)
    assert not R.farneback(a, a, np.float32).any()


@pytest.mark.parametrize('name', [k for k in SMALL if any(R.FLOW_CASES[k][2])])
def test_a_pure_shift_is_recovered_and_moves_most_pixels(name):
    """Median flow within 0.1 px of (dx, dy) -- [..., 0] along columns, [..., 1] along rows, next(p + flow) ~ prev(p) -- where the image is
    large enough to have an interior (the 9 x 11 case lies inside the 5-px border weights throughout and is held to the sign only); and at
    least half of the pixels have a non-zero rounded flow, so that the metric's warp is exercised."""
    h, w, (dx, dy), _ = R.FLOW_CASES[name]
    f = _flow64(name)
    if min(h, w) >= 32:
        assert abs(np.median(f[..., 0]) - dx) <= 0.1 and abs(np.median(f[..., 1]) - dy) <= 0.1
    else:
        assert np.sign(np.median(f[..., 0])) == np.sign(dx) and np.sign(np.median(f[..., 1])) == np.sign(dy)
    assert (np.rint(f) != 0).any(-1).mean() >= 0.5


def test_shift_axes_are_told_apart():
    a, b = R.frame_pair(64, 80, (2.2, 0.0), 7)
    f = R.farneback(a, b, np.float64)
    assert abs(np.median(f[..., 0]) - 2.2) <= 0.1 and abs(np.median(f[..., 1])) <= 0.1
    whole = R.frames(64, 80, [(3.0, 0.0)], 7)[0]                         # x is the column axis: a whole-pixel move is a roll of the columns
    assert np.abs(whole.astype(int) - np.roll(a, 3, axis=1).astype(int)).max() <= 1


def test_the_shift_band_is_enforced():
    """Fractional parts in [0.15, 0.35] u [0.65, 0.85]; a component of exactly 0 and the one shift the issue names are the exceptions."""
    for ok in ((1.2, -0.8), (9.3, 6.2), (2.2, 0.0), (-0.85, 4.15), R.ISSUE_SHIFT):
        R.check_shift(ok)
    for bad in ((1.5, 0.2), (1.4, 0.2), (0.2, 2.62), (3.05, 0.2), (0.2, -2.1), (1.0, 0.2), (0.2, 0.9)):
        with pytest.raises(AssertionError):
            R.check_shift(bad)
    shifts = [v[2] for v in R.FLOW_CASES.values()] + list(R.BATCH_SHIFTS)
    assert all(R.check_shift(s) is None for s in shifts if s[0] or s[1])


def test_levels_and_level_sizes():
    for mod in (R, flow):
        assert [mod.levels_of(h, w) for h, w in ((40, 36), (131, 150), (1024, 1031), (63, 500))] == [0, 2, 5, 0]
        assert mod.level_size(150, 150, 2) == (38, 38) and mod.level_size(131, 131, 1) == (66, 66)      # 37.5 -> 38, 65.5 -> 66: half to even
        assert mod.level_size(131, 150, 2) == (33, 38) and mod.level_size(100, 100, 3) == (12, 12)      # 12.5 -> 12
    assert [R.smooth_size(k)[1] for k in range(6)] == [3, 3, 9, 19, 39, 79]


def test_build_metric_builds_messddt_only_when_asked():
    with pytest.raises(NotImplementedError):
        dm.build_metric(['MESSDdt'])
    with pytest.raises(NotImplementedError):
        dm.build_metric(['MESSDdt'], device_conn=True)
    with pytest.raises(NotImplementedError):
        dm.build_metric(['Conn'], device_flow=True)
    names = ['MAD', 'MSE', 'SAD', 'Conn', 'Grad', 'dtSSD', 'MESSDdt']                                  # the test metrics of configs/maggie_video.yaml
    built = dm.build_metric(names, device_conn=True, device_flow=True)
    assert list(built) == names and isinstance(built['MESSDdt'], dm.MESSDdt)
    m = built['MESSDdt']
    assert (m.score, m.count) == (0, 0) and all(hasattr(m, a) for a in ('update', 'average', 'reset', 'gather_metric'))
    if not torch.cuda.is_available():
        x = torch.zeros(2, 1, 8, 8)
        with pytest.raises(hip.MaggieHipError):
            m.update(x, x)
        with pytest.raises(hip.MaggieHipError):
            flow.farneback(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8))


def test_farneback_argument_errors():
    with pytest.raises(TypeError):
        flow.farneback(np.zeros((8, 8), np.float32), np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError):
        flow.farneback(np.zeros((8, 8), np.uint8), np.zeros((8, 9), np.uint8))
    with pytest.raises(hip.MaggieHipError):
        flow.check_shape(1, 40000, 8)


@pytest.mark.skipif(not os.path.isfile(HIPCC) or shutil.which('c++filt') is None, reason='hipcc / c++filt not available')
def test_no_flow_kernel_uses_scratch_memory():
    import isa_load_chains as ilc
    with tempfile.NamedTemporaryFile(suffix='.s') as f:
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', os.path.join(ROOT, 'maggie_amd', 'csrc', 'flow.hip'),
                        '-o', f.name], check=True, stderr=subprocess.DEVNULL, timeout=600)
        asm = open(f.name).read()
    table = {name: scratch for name, _, _, _, scratch in ilc.kernels(asm)}
    for key in ('level_rows_kernel', 'level_cols_kernel', 'polyexp_kernel', 'matrices_kernel', 'update_kernel', 'messddt_partial_kernel'):
        assert any(key in name for name in table), (key, sorted(table))
    assert all(v == 0 for v in table.values()), table
