"""Connected components, host side: the test restatement against the reference's own Conn / postprocess (conn_pinned.npz), and the
build_metric contract for the device Conn."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_restatement_matches_reference_fixture():
    pytest.importorskip('scipy.ndimage')
    import conn_restatement as R
    from helpers import load_golden
    gold = load_golden('conn_pinned.npz')
    for key in R.CONN_CASES:
        pred, gt, tri = R.conn_inputs(key)
        r, score, count = R.conn_update(pred, gt, tri)
        ref = gold['conn.' + key]                                  # [update() return, score, count, average()]; the reference sums in fp32
        assert count == ref[2], key
        assert abs(score - ref[1]) <= 1e-5 * abs(ref[1]), (key, score, ref[1])
        assert abs(r - ref[0]) <= 1e-5 * abs(ref[0]), key
    alpha = R.postprocess_inputs()
    out = R.postprocess(alpha)
    ref = gold['postprocess']
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(out[0, 0].view(np.uint32), alpha[0, 0].view(np.uint32))      # no foreground: unchanged, -0.0 included
    assert (out[0, 1][10:15, 60:75] == alpha[0, 1][10:15, 60:75]).all() and (out[0, 1][40:55, 50:55] <= 0).all()     # the tie


def test_fixture_inputs_avoid_the_split_threshold_values():
    import conn_restatement as R
    for key in R.CONN_CASES:
        pred, gt, _ = R.conn_inputs(key)
        for v in R.SPLIT_VALUES:
            assert not (pred == v).any() and not (gt == v).any()
    assert R.SPLIT_VALUES[0] < R.THRESH64[7] and R.SPLIT_VALUES[1] < R.THRESH64[9]


def test_build_metric_device_conn():
    from maggie_amd.utils import metric as dm
    ms = dm.build_metric(['MAD', 'MSE', 'SAD', 'Grad', 'Conn'], device_conn=True)
    assert list(ms) == ['MAD', 'MSE', 'SAD', 'Grad', 'Conn']
    assert isinstance(ms['Conn'], dm.Conn) and isinstance(ms['Conn'], dm.Metric)
    assert ms['Conn'].score == 0 and ms['Conn'].count == 0


def test_build_metric_host_only_metrics_still_raise():
    from maggie_amd.utils import metric as dm
    with pytest.raises(NotImplementedError):
        dm.build_metric(['Conn'])
    with pytest.raises(NotImplementedError):
        dm.build_metric(['MESSDdt'], device_conn=True)
    with pytest.raises(NotImplementedError):
        dm.build_metric(['SAD', 'Conn', 'MESSDdt'], device_conn=True)
