"""Farneback flow and MESSDdt on the device (csrc/flow.hip, maggie_amd.utils.flow, maggie_amd.utils.metric.MESSDdt) against the NumPy
restatement (tests/flow_restatement.py, which tests/test_flow_cpu.py holds against an independent scipy statement and the reference's own
reduction) and the fixture the reference's MESSDdt.update wrote (tests/golden/flow_pinned.npz).

The flow's bar: max-abs distance to the fp64 restatement <= 10 x the fp32 restatement's own distance to it on that case (computed here, on the
CPU, from the restatement alone; 10 covers fused multiply-adds and another summation order over the 7-, 11- and up-to-79-tap sums), and at
most 1e-3 of the pixels with another rounded flow. Each test prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flow_restatement as R                                          # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.hip import c_int, c_long                              # noqa: E402
from maggie_amd.utils import flow                                     # noqa: E402
from maggie_amd.utils import metric as dm                             # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _pair_ref(key, a, b):
    """(fp64 flow, the fp32 restatement's max-abs distance to it) of a plane pair, computed once and left unchanged."""
    if key not in _REF:
        f64 = R.farneback(a, b, np.float64)
        _REF[key] = (f64, float(np.abs(R.farneback(a, b, np.float32) - f64).max()))
    return _REF[key]


def _held(name, got, f64, yard):
    dist = float(np.abs(got.astype(np.float64) - f64).max())
    flips = float((np.rint(got) != np.rint(f64)).any(-1).mean())
    print('%s: device-fp64 %.3g, fp32-fp64 %.3g, ratio %.2f, flips %.3g' % (name, dist, yard, dist / yard if yard else 0.0, flips))
    assert dist <= 10 * yard, (name, dist, yard)
    assert flips <= 1e-3, (name, flips)


@pytest.mark.parametrize('name', sorted(R.FLOW_CASES))
def test_flow_equals_the_restatement(name):
    dev = _dev()
    h, w, shift, seed = R.FLOW_CASES[name]
    a, b = R.frame_pair(h, w, shift, seed)
    f64, yard = _pair_ref(name, a, b)
    got = flow.farneback(a, torch.from_numpy(b).to(dev))                 # one plane from the host, one from the device
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (1, h, w, 2)
    got = got[0].cpu().numpy()
    assert np.isfinite(got).all()
    if not (shift[0] or shift[1]):
        assert not got.any() and not f64.any()                           # zero motion: exactly zero
    else:
        assert (np.rint(f64) != 0).any(-1).mean() >= 0.5
    _held(name, got, f64, yard)


def test_a_batch_equals_its_planes_bit_for_bit():
    """5 pairs of 70 x 90 with different shifts in one call: each plane is the result of its own P = 1 call, and within the bar."""
    dev = _dev()
    prev, nxt = R.batch_pairs()
    got = flow.farneback(prev, nxt, device=dev)
    assert tuple(got.shape) == (5, 70, 90, 2)
    again = flow.farneback(torch.from_numpy(prev).to(dev).reshape(5, 1, 70, 90), torch.from_numpy(nxt).to(dev).reshape(5, 1, 70, 90))
    assert torch.equal(got, again)
    for p in range(5):
        alone = flow.farneback(prev[p], nxt[p], device=dev)
        assert torch.equal(alone[0], got[p]), p
        f64, yard = _pair_ref(('batch', p), prev[p], nxt[p])
        _held('batch[%d]' % p, got[p].cpu().numpy(), f64, yard)
    assert not got[2].any()                                              # the still pair of the batch


def test_other_parameters_and_bad_shapes_are_rejected():
    dev = _dev()
    a = torch.zeros((1, 40, 36), dtype=torch.uint8, device=dev)
    for kw in (dict(pyr_scale=0.8), dict(levels=3), dict(winsize=15), dict(iterations=3), dict(poly_n=5), dict(poly_sigma=1.1), dict(flags=0)):
        with pytest.raises(hip.MaggieHipError):
            flow.farneback(a, a, **kw)
    n = hip.ctypes.c_long(0)
    lib = hip.lib()
    assert lib.mg_flow_scratch_bytes(c_long(40000), c_int(8), c_int(8), hip.ctypes.byref(n)) == -3
    assert lib.mg_flow_scratch_bytes(c_long(1), c_int(0), c_int(8), hip.ctypes.byref(n)) == -2
    assert lib.mg_flow_scratch_bytes(c_long(2), c_int(8), c_int(8), hip.ctypes.byref(n)) == 0 and n.value == 26 * 2 * 64 * 4
    assert [lib.mg_flow_levels(c_int(h), c_int(w)) for h, w in ((40, 36), (131, 150), (1024, 1031), (63, 500))] == [0, 2, 5, 0]
    assert tuple(flow.farneback(np.zeros((0, 8, 8), np.uint8), np.zeros((0, 8, 8), np.uint8), device=dev).shape) == (0, 8, 8, 2)
    torch.cuda.synchronize()


# ---- the reduction alone -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.REDUCTION_CASES))
def test_reduction_equals_the_reference(name):
    """mg_metric_messddt fed the fixture's integer flows (MESSDdt.update(..., flow=)) against the reference's own update()."""
    dev = _dev()
    ret, score, count, average = load_golden('flow_pinned.npz')['messddt.' + name]
    pred, gt, tri, flows = R.reduction_case(name)
    T = lambda x: None if x is None else torch.from_numpy(x).to(dev)      # noqa: E731
    m = dm.build_metric(['MESSDdt'], device_flow=True)['MESSDdt']
    r = m.update(T(pred), T(gt), T(tri), flow=T(flows.astype(np.float32)))
    print(name, 'device', m.score, m.count, 'reference', score, count)
    assert m.count == count
    assert m.score == pytest.approx(score, rel=2e-5, abs=0)
    assert r == pytest.approx(ret, rel=2e-5, abs=0) and m.average() == pytest.approx(average, rel=2e-5, abs=0)
    if count:                                                             # the leading 1 of metric.py:504-506
        m5 = dm.MESSDdt()
        m5.update(T(pred)[None], T(gt)[None], None if tri is None else T(tri)[None], flow=T(flows.astype(np.float32)))
        assert m5.score == m.score and m5.count == m.count


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 2, 131, 150, False), (2, 1, 64, 200, True)], ids=['f3_n2_131x150', 'f2_n1_64x200_trimap'])
def test_messddt_end_to_end(shape):
    """The metric's own flow path (uint8 conversion, the prev / next planes of F x N_i, the scratch carving, `flow_out`): its flow is, bit for
    bit, `flow.farneback` of the planes NumPy converts; at most 1e-3 of each instance's pixels round to another flow than the fp64
    restatement's; and |score - restated| <= sum over instances of 10000 n_disagree / sum num + 2e-5 |score|: a pixel whose rounded flow
    differs from the restatement's moves its instance's sum |error_map| by at most 1."""
    dev = _dev()
    F, N, h, w, trimap = shape
    pred, gt, tri = R.matte_clip(F, N, h, w, 31, trimap)
    assert len(np.unique(R.gt_u8(gt))) == 256                             # every uint8 value goes through the device's conversion
    want, count, flows = R.messddt_restated(pred, gt, tri, np.float64)
    assert count == N and (flows != 0).any(-1).mean() >= 0.5
    T = lambda x: None if x is None else torch.from_numpy(x).to(dev)      # noqa: E731
    m = dm.build_metric(['MESSDdt'], device_flow=True)['MESSDdt']
    r = m.update(T(pred), T(gt), T(tri), keep_flow=True)
    u8 = R.gt_u8(gt)
    alone = flow.farneback(u8[:-1], u8[1:], device=dev).reshape(F - 1, N, h, w, 2)
    assert tuple(m.last_flow.shape) == (F - 1, N, h, w, 2) and torch.equal(m.last_flow, alone)
    got_flows = np.rint(m.last_flow.cpu().numpy()).astype(np.int64)
    mask = np.ones_like(gt) if tri is None else (tri == 1).astype(np.float32)
    slack = 0.0
    for n in range(N):
        disagree = int((got_flows[:, n] != flows[:, n]).any(-1).sum())
        print('instance', n, 'pixels whose rounded flow differs', disagree, 'of', (F - 1) * h * w)
        assert disagree <= 1e-3 * (F - 1) * h * w, (n, disagree)
        slack += 10000.0 * disagree / float(mask[:-1, n].sum() + (F - 1))
    print(shape, 'device', m.score, 'restated', want, 'slack from disagreeing pixels', slack)
    assert abs(m.score - want) <= slack + 2e-5 * abs(want)
    assert m.count == N and r == pytest.approx(m.score / (N + 1e-8))
    first = m.score
    m.update(T(pred), T(gt), T(tri))
    assert m.count == 2 * N and m.score == pytest.approx(2 * first, rel=1e-12)       # the same launches: the same bits
    assert m.average() == pytest.approx(m.score / (2 * N + 1e-6))
    m.reset()
    assert (m.score, m.count) == (0, 0)
    assert m.update(T(pred)[:1], T(gt)[:1], None) == 0.0 and (m.score, m.count) == (0, 0)        # F < 2 adds nothing


def test_the_uint8_conversion_truncates_every_value():
    """The planes the metric's flow runs on are (uint8)(gt * 255.0f): gt = k / 255 for all 256 k (where the fp32 product can fall short of k) and
    gt = (k + 0.6) / 255 (where rounding would give k + 1). The metric's flow equals, bit for bit, the flow of the planes NumPy converts, and
    not the flow of the rounded planes."""
    dev = _dev()
    rng = np.random.default_rng(41)
    k = np.stack([rng.permutation(256) for _ in range(4)]).reshape(2, 2, 8, 32).astype(np.float32)
    for gt in (k / np.float32(255), (k + np.float32(0.6)) / np.float32(255)):
        u8 = R.gt_u8(gt)
        rounded = np.clip(np.rint(gt * np.float32(255)), 0, 255).astype(np.uint8)
        assert len(np.unique(u8)) == 256
        g = torch.from_numpy(gt).to(dev)
        m = dm.MESSDdt()
        m.update(g, g, None, keep_flow=True)
        assert torch.equal(m.last_flow, flow.farneback(u8[:-1], u8[1:], device=dev).reshape(1, 2, 8, 32, 2))
        if (rounded != u8).any():
            assert not torch.equal(m.last_flow, flow.farneback(rounded[:-1], rounded[1:], device=dev).reshape(1, 2, 8, 32, 2))
    assert (rounded != u8).any()                                          # the second set tells truncation from rounding


def test_the_video_metric_list_is_built_without_a_host_metric():
    dev = _dev()
    names = ['MAD', 'MSE', 'SAD', 'Conn', 'Grad', 'dtSSD', 'MESSDdt']
    built = dm.build_metric(names, device_conn=True, device_flow=True)
    pred, gt, tri = (torch.from_numpy(x).to(dev) for x in R.matte_clip(3, 2, 40, 36, 5, True))
    for k in names:
        assert np.isfinite(built[k].update(pred, gt, tri))
        assert built[k].count > 0
