"""Connected components on the device (csrc/ccl.hip): maggie_amd.utils.connected.label against scipy.ndimage.label (skimage's numbering),
the device Conn metric against the reference's own values (conn_pinned.npz) and the fp64 restatement (tests/conn_restatement.py), and
postprocessing.postprocess bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _serpentine(H, W):
    m = np.zeros((H, W), np.uint8)
    m[::2] = 1
    for y in range(1, H, 2):
        m[y, W - 1 if y % 4 == 1 else 0] = 1
    return m


def _label_planes():
    """{name: (P, H, W) uint8 planes}: every plane of one entry has the same shape (one batched call per entry)."""
    rs = np.random.RandomState(5)
    out = {}
    for d in (0.3, 0.59, 0.8):
        out['random%.2f' % d] = (rs.rand(3, 200, 300) < d).astype(np.uint8)
    out['serpentine'] = np.stack([_serpentine(193, 300), _serpentine(193, 300)[::-1].copy()])
    yy, xx = np.mgrid[:131, :150]
    out['checker'] = ((yy + xx) % 2).astype(np.uint8)[None]
    out['empty_full'] = np.stack([np.zeros((70, 130), np.uint8), np.ones((70, 130), np.uint8)])
    out['1x1'] = np.array([[[0]], [[1]]], np.uint8)
    out['1x1029'] = (rs.rand(2, 1, 1029) < 0.59).astype(np.uint8)
    out['777x1'] = (rs.rand(2, 777, 1) < 0.59).astype(np.uint8)
    out['67x1029'] = (rs.rand(2, 67, 1029) < 0.59).astype(np.uint8)
    out['1080x1920'] = (rs.rand(1, 1080, 1920) < 0.59).astype(np.uint8)
    return out


@pytest.mark.parametrize('connectivity', [1, 2])
def test_label_matches_scipy(connectivity):
    """Labels and counts array_equal to scipy.ndimage.label (= skimage.measure.label's numbering: raster order of first pixels)."""
    pytest.importorskip('scipy.ndimage')
    import conn_restatement as R
    from maggie_amd.utils import connected
    dev = _dev()
    for name, planes in _label_planes().items():
        lab, num = connected.label(_T(planes, dev), connectivity=connectivity, return_num=True)
        assert lab.dtype == torch.int32 and num.dtype == torch.int32 and tuple(num.shape) == planes.shape[:1]
        lab, num = lab.cpu().numpy(), num.cpu().numpy()
        for p in range(planes.shape[0]):
            ref, n = R.label(planes[p], connectivity)
            assert num[p] == n, (name, p, num[p], n)
            assert np.array_equal(lab[p], ref), (name, p, int((lab[p] != ref).sum()))
    if connectivity == 2:                                          # checkerboard: one component at 8-, all singletons at 4-connectivity
        assert int(connected.label(_T(_label_planes()['checker'], dev), 2).max()) == 1
    else:
        assert int(connected.label(_T(_label_planes()['checker'], dev), 1).max()) == 131 * 150 // 2


def test_label_batched_bool_and_default_connectivity():
    pytest.importorskip('scipy.ndimage')
    import conn_restatement as R
    from maggie_amd.utils import connected
    dev = _dev()
    rs = np.random.RandomState(6)
    m = rs.rand(2, 3, 90, 140) < 0.5
    lab, num = connected.label(_T(m, dev), return_num=True)
    assert tuple(lab.shape) == m.shape and tuple(num.shape) == (2, 3)
    lab, num = lab.cpu().numpy(), num.cpu().numpy()
    for b in range(2):
        for n in range(3):
            ref, k = R.label(m[b, n], 2)
            assert num[b, n] == k and np.array_equal(lab[b, n], ref)
    assert np.array_equal(connected.label(_T(m, dev)).cpu().numpy(), lab)


def test_conn_matches_reference_fixture():
    """Device Conn == the reference's own Conn (conn_pinned.npz; the reference sums pairwise in fp32: rtol 1e-5); the image config's metric
    list builds with device_conn=True, accumulates over two updates and resets."""
    import conn_restatement as R
    from helpers import load_golden
    from maggie_amd.utils import metric as dm
    dev = _dev()
    gold = load_golden('conn_pinned.npz')
    for key in R.CONN_CASES:
        pred, gt, tri = R.conn_inputs(key)
        ms = dm.build_metric(['MAD', 'MSE', 'SAD', 'Grad', 'Conn'], device_conn=True)
        for name, m in ms.items():
            r = m.update(_T(pred, dev), _T(gt, dev), _T(tri, dev))
            if name != 'Conn':
                continue
            ref = gold['conn.' + key]                              # [update() return, score, count, average()]
            assert m.count == ref[2], key
            assert abs(m.score - ref[1]) <= 1e-5 * abs(ref[1]), (key, m.score, ref[1])
            assert abs(r - ref[0]) <= 1e-5 * abs(ref[0]) and abs(m.average() - ref[3]) <= 1e-5 * abs(ref[3])
            s1 = m.score
            m.update(_T(pred, dev), _T(gt, dev), _T(tri, dev))
            assert m.count == 2 * ref[2] and m.score == 2 * s1
        for m in ms.values():
            m.reset()
            assert m.score == 0 and m.count == 0


def _conn_score(pred, gt, tri, dev):
    from maggie_amd.utils import metric as dm
    m = dm.build_metric(['Conn'], device_conn=True)['Conn']
    m.update(_T(pred, dev), _T(gt, dev), _T(tri, dev))
    return m.score, m.count


def test_conn_matches_restatement():
    """Device Conn == the fp64-summing restatement at rtol 1e-10: every fixture case, (4, 2, 512, 512) and (4, 1080, 1920) smooth fields,
    with and without trimap."""
    pytest.importorskip('scipy.ndimage')
    import conn_restatement as R
    dev = _dev()
    cases = [R.conn_inputs(k) for k in R.CONN_CASES]
    p, g, t = R.conn_inputs('smooth_tri', shape=(4, 2, 512, 512), seed=47)
    cases += [(p, g, t), (p, g, None)]
    p, g, t = R.conn_inputs('smooth_tri', shape=(4, 1080, 1920), seed=48)
    cases += [(p, g, t), (p, g, None)]
    for i, (pred, gt, tri) in enumerate(cases):
        score, count = _conn_score(pred, gt, tri, dev)
        ref = R.conn_diff(pred, gt, tri).sum() * 0.001
        assert count == pred.reshape(-1, *pred.shape[-2:]).shape[0]
        assert abs(score - ref) <= 1e-10 * abs(ref), (i, pred.shape, score, ref)


def test_conn_planted_threshold_values():
    """Pixels at exactly float32(t_i), their float32 neighbours, k/255, and large regions at float32(0.7000000000000001) /
    float32(0.9): the device follows the float32 (numpy < 2) comparison, and the float64-comparison variant scores differently here."""
    pytest.importorskip('scipy.ndimage')
    import conn_restatement as R
    dev = _dev()
    rs = np.random.RandomState(12)
    vals = [np.float32(v) for v in R.THRESH32[1:]]
    vals += [np.nextafter(v, np.float32(2)) for v in R.THRESH32[1:]] + [np.nextafter(v, np.float32(-1)) for v in R.THRESH32[1:]]
    vals += [np.float32(k / 255.0) for k in range(256)]
    vals = np.asarray(vals, np.float32)
    P, H, W = 3, 160, 200
    pred = vals[rs.randint(0, len(vals), size=(P, H, W))]
    gt = vals[rs.randint(0, len(vals), size=(P, H, W))]
    pred[:, 10:90, 10:100] = R.SPLIT_VALUES[0]                     # passes level 7 in float32, not in float64
    gt[:, 10:90, 10:100] = np.float32(0.95)
    pred[:, 10:90, 100:190] = R.SPLIT_VALUES[1]                    # passes level 9 in float32, not in float64
    gt[:, 10:90, 100:190] = np.float32(1.0)
    gt[1, 100:150, 20:120] = R.SPLIT_VALUES[0]
    pred[1, 100:150, 20:120] = np.float32(0.85)
    tri = rs.randint(0, 3, size=(P, H, W)).astype(np.float32)
    for t in (tri, None):
        score, _ = _conn_score(pred, gt, t, dev)
        ref32 = R.conn_diff(pred, gt, t).sum() * 0.001
        ref64 = R.conn_diff(pred, gt, t, float64_thresholds=True).sum() * 0.001
        assert abs(score - ref32) <= 1e-10 * abs(ref32), (score, ref32)
        assert abs(ref64 - ref32) > 1e-3 * abs(ref32), (ref64, ref32)      # the test can see the semantics


def test_conn_tie_goes_to_the_raster_first_component():
    """Two equal-size largest components at levels 1..5: the one whose first pixel comes first in raster order sets round_down."""
    pytest.importorskip('scipy.ndimage')
    import conn_restatement as R
    dev = _dev()
    H, W = 100, 140
    gt = np.zeros((1, H, W), np.float32)
    pred = np.zeros((1, H, W), np.float32)
    gt[0, 10:30, 80:120], pred[0, 10:30, 80:120] = 0.5, 0.9        # A: first pixel (10, 80)
    gt[0, 60:80, 5:45], pred[0, 60:80, 5:45] = 0.5, 0.55           # B: same size, first pixel (60, 5)
    score, _ = _conn_score(pred, gt, None, dev)
    ref = R.conn_diff(pred, gt).sum() * 0.001
    assert abs(score - ref) <= 1e-10 * abs(ref)
    a_wins = (800 * 0.4 + 800 * 0.05) * 0.001                       # A keeps round_down 0.5; B drops to 0
    b_wins = (800 * 0.4 + 0.0) * 0.001
    assert abs(score - a_wins) < 1e-4 and abs(score - b_wins) > 1e-2


def test_postprocess_matches_reference_fixture_bitwise():
    import conn_restatement as R
    from helpers import load_golden
    from maggie_amd.utils.postprocessing import postprocess
    dev = _dev()
    alpha = R.postprocess_inputs()
    ref = load_golden('conn_pinned.npz')['postprocess']
    out = postprocess(_T(alpha, dev))
    assert out.dtype == torch.float32 and tuple(out.shape) == alpha.shape
    out = out.cpu().numpy()
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), int((out.view(np.uint32) != ref.view(np.uint32)).sum())
    assert np.array_equal(np.signbit(out), np.signbit(ref))
    assert np.array_equal(out[0, 0].view(np.uint32), alpha[0, 0].view(np.uint32))                  # no foreground: unchanged
    assert (out[0, 1][10:15, 60:75] == alpha[0, 1][10:15, 60:75]).all() and not out[0, 1][40:55, 50:55].any()     # the tie


def test_postprocess_fullsize_matches_restatement_and_replays_in_a_graph():
    pytest.importorskip('scipy.ndimage')
    import conn_restatement as R
    from maggie_amd.utils.postprocessing import postprocess
    dev = _dev()
    rs = np.random.RandomState(13)
    alpha = (R.smooth_field(rs, (4, 1080, 1920), cell=40) * 1.1 - 0.05).astype(np.float32)
    ref = R.postprocess(alpha)
    x = _T(alpha, dev)
    out = postprocess(x).cpu().numpy()
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), int((out != ref).sum())
    static = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        postprocess(static)                                        # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = postprocess(static)
    static.copy_(x)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    alpha2 = R.postprocess_inputs((2, 2, 1080, 1920), 49).reshape(4, 1080, 1920)
    static.copy_(_T(alpha2, dev))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy().view(np.uint32), R.postprocess(alpha2).view(np.uint32))
    del g


def test_connected_components_are_deterministic():
    import conn_restatement as R
    from maggie_amd.utils import connected
    from maggie_amd.utils.postprocessing import postprocess
    dev = _dev()
    rs = np.random.RandomState(14)
    m = _T(rs.rand(4, 300, 500) < 0.59, dev)
    a, na = connected.label(m, 1, return_num=True)
    b, nb = connected.label(m, 1, return_num=True)
    assert torch.equal(a, b) and torch.equal(na, nb)
    pred, gt, tri = R.conn_inputs('smooth_tri', shape=(3, 2, 256, 320), seed=50)
    s1 = _conn_score(pred, gt, tri, dev)
    s2 = _conn_score(pred, gt, tri, dev)
    assert s1 == s2
    x = _T(R.postprocess_inputs((1, 3, 256, 320), 51), dev)
    assert torch.equal(postprocess(x).view(torch.int32), postprocess(x).view(torch.int32))
