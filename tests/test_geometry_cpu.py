"""Host side of the device input geometry (maggie_amd.utils.geometry): `plan()` against hand-computed sizes, the fixture against the restatement,
the restated OpenCV operators against independent formulations, the argument errors. No GPU needed."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import geometry_restatement as R                                      # noqa: E402
import groundtruth_restatement as G                                   # noqa: E402
import maskgen_restatement as M                                       # noqa: E402
from helpers import load_golden, unpack_bits                         # noqa: E402
from maggie_amd.hip import MaggieHipError                             # noqa: E402
from maggie_amd.utils import geometry                                 # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor            # noqa: E402

# (h, w, short, divisor) -> ratio, resized (h, w), pad (h, w), worked by hand from transforms.py:117-120,149-151
HAND = {
    (37, 53, 24, 64): (24 / 37, (24, 34), (40, 30)),            # 53 * 24 / 37 = 34.38 -> 34
    (45, 61, 96, 64): (96 / 45, (96, 130), (32, 62)),           # 61 * 96 / 45 = 130.13 -> 130
    (50, 70, 25, 64): (0.5, (25, 35), (39, 29)),
    (130, 90, 23, 64): (23 / 90, (33, 23), (31, 41)),           # 130 * 23 / 90 = 33.2 -> 33
    (64, 128, 64, 64): (1.0, (64, 128), (0, 0)),
    (48, 80, 48, 64): (1.0, (48, 80), (16, 48)),
    (97, 139, 75, 16): (75 / 97, (75, 107), (5, 5)),            # 139 * 75 / 97 = 107.47 -> 107
    (40, 56, 30, 64): (0.75, (30, 42), (34, 22)),
}
FLOAT_SHAPES = [((37, 53), (34, 24)), ((45, 61), (130, 96)), ((50, 70), (35, 25)), ((130, 90), (23, 33)), ((97, 139), (107, 75)),
                ((40, 56), (42, 30)), ((64, 64), (200, 9))]


def test_plan_sizes_pads_and_transform_info_by_hand():
    assert {(c['h'], c['w'], c['short'], c['divisor']) for c in R.GOLDEN.values()} == set(HAND)
    for (h, w, short, divisor), (ratio, (rh, rw), (ph, pw)) in HAND.items():
        p = geometry.plan(h, w, short, divisor)
        assert p.ratio == short * 1.0 / min(h, w) and abs(p.ratio - ratio) < 1e-12
        assert (p.rh, p.rw, p.pad_h, p.pad_w, p.out_h, p.out_w) == (rh, rw, ph, pw, rh + ph, rw + pw)
        assert p.out_h % divisor == 0 and p.out_w % divisor == 0
        assert p.transform_info == [{'name': 'resize', 'ori_size': (h, w), 'ratio': p.ratio}, {'name': 'padding', 'pad_size': (ph, pw)}]
        assert list(p.transform_info[0]) == ['name', 'ori_size', 'ratio'] and list(p.transform_info[1]) == ['name', 'pad_size']
        assert p.resized == (ratio != 1.0)
        assert R.plan(h, w, short, divisor) == (p.ratio, (rh, rw), (ph, pw))


def test_plan_tables_match_the_restated_axes_and_pick_the_regime():
    for (h, w, short, divisor) in HAND:
        p = geometry.plan(h, w, short, divisor)
        t = p.tables
        for axis, src, dst in (('x', w, p.rw), ('y', h, p.rh)):
            ofs, c0, c1 = M.resize_axis(src, dst, 1.0 / (dst / src))
            assert np.array_equal(t[axis][0], ofs) and np.array_equal(t[axis][1], c0) and np.array_equal(t[axis][2], c1)
        assert np.array_equal(t['nx'], R.nearest_axis(w, p.rw)) and np.array_equal(t['ny'], R.nearest_axis(h, p.rh))
        assert t['linear'].dtype == np.int32 and t['linear'].shape == (3 * (p.rw + p.rh),)
        assert t['nearest'].dtype == np.int32 and t['nearest'].shape == (p.rw + p.rh,)
    # the regime follows the worst tile's source rows: under 2x shared, the 130 -> 33 rows of the fourth case direct
    assert geometry.plan(37, 53, 24).tables['regime'] == geometry.SHARED_ROWS
    assert geometry.plan(50, 70, 25).tables['regime'] == geometry.SHARED_ROWS
    assert geometry.plan(130, 90, 23).tables['regime'] == geometry.DIRECT
    assert geometry.plan(3000, 4000, 768).tables['regime'] == geometry.DIRECT
    assert geometry.plan(1365, 2048, 768).tables['regime'] == geometry.SHARED_ROWS
    assert geometry.plan(130, 90, 23).tables['rows_read'] > geometry.MAX_ROWS >= geometry.plan(1365, 2048, 768).tables['rows_read']
    with pytest.raises(ValueError):
        geometry._regime(geometry.plan(130, 90, 23).tables, 'shared')


def test_mask_index_map_is_resize_then_pad_then_eighth():
    for (h, w, short, divisor) in HAND:
        p = geometry.plan(h, w, short, divisor)
        mh, mw, vh, vw, tab = p.mask8()
        m = np.arange(h * w, dtype=np.int64).reshape(h, w) + 1                         # every source pixel its own value; 0 is the padding
        full = np.zeros((p.out_h, p.out_w), np.int64)
        full[:p.rh, :p.rw] = m[p.tables['ny'][:, None], p.tables['nx'][None, :]]
        ys = np.minimum(np.floor(np.arange(mh, dtype=np.float32) * (np.float32(p.out_h) / np.float32(mh))).astype(np.int64), p.out_h - 1)
        xs = np.minimum(np.floor(np.arange(mw, dtype=np.float32) * (np.float32(p.out_w) / np.float32(mw))).astype(np.int64), p.out_w - 1)
        want = full[ys[:, None], xs[None, :]]
        got = np.zeros((mh, mw), np.int64)
        got[:vh, :vw] = m[tab[vw:][:, None], tab[:vw][None, :]]
        assert (mh, mw) == (p.out_h // 8, p.out_w // 8) and np.array_equal(got, want)


def test_python_constants_match_the_library():
    from maggie_amd import hip
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert hip.lib().mg_resize_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    assert (a.value, b.value, c.value) == (geometry.TILE_ROWS, geometry.TILE_COLS, geometry.MAX_ROWS)
    assert hip.lib().mg_resize_limits(None, None, None) == -2


def test_c_entry_rejects_bad_arguments_before_any_launch():
    from maggie_amd import hip
    fn = hip.lib().mg_resize_u8
    fn.restype = ctypes.c_int
    I, L = ctypes.c_int, ctypes.c_long

    def call(images=1, C=1, H=4, W=4, dh=2, dw=2, Ho=2, Wo=2, interp=0, epi=0, regime=0, n_in=1, n_slots=1, mean=None):
        return fn(None, None, None, None, None, L(images), I(n_in), I(n_slots), I(C), I(H), I(W), I(dh), I(dw), I(Ho), I(Wo), I(interp), I(epi),
                  I(regime), mean, mean, I(0), None)
    assert call() == -2                                                    # null pointers
    assert call(images=0) == 0
    for bad in (dict(C=2), dict(H=0), dict(dw=0), dict(Ho=1), dict(interp=2), dict(epi=3), dict(regime=2), dict(images=-1),
                dict(epi=1), dict(epi=1, C=3), dict(epi=2, C=3), dict(epi=2, n_slots=2), dict(epi=2, n_in=0)):
        assert call(**bad) == -2, bad


def test_fixture_equals_the_restatement():
    d = load_golden('geometry_pinned.npz')
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'geometry_pinned.npz')) < 64 * 1024
    for name, c in R.GOLDEN.items():
        frames, alphas, masks = R.golden_inputs(name)
        rf, ra, rm, info = R.resize_short_pad(frames, alphas, masks, c['short'], c['divisor'])
        assert np.array_equal(R.unpack_rows(d[name + '.frames']), rf) and np.array_equal(R.unpack_rows(d[name + '.alphas']), ra)
        assert np.array_equal(unpack_bits(d[name + '.masks'], rm.shape) * 255, rm)
        assert np.array_equal(unpack_bits(d[name + '.genmasks'], rm.shape) * 255, M.from_alpha(ra))
        h, w, ratio, ph, pw = d[name + '.info'].tolist()
        assert info == [{'name': 'resize', 'ori_size': (int(h), int(w)), 'ratio': ratio}, {'name': 'padding', 'pad_size': (int(ph), int(pw))}]
        assert info == geometry.plan(c['h'], c['w'], c['short'], c['divisor']).transform_info
        if name == R.FP32_CASE:
            assert np.array_equal(d[name + '.image'], R.normalized(rf))
        if name in R.PREDICT_CASES:
            assert np.array_equal(unpack_bits(d[name + '.predict_masks'], rm.shape) * 255, rm)
        # what the inputs must make visible
        assert ((ra > 0) & (ra < 5)).any() and frames.min() > 0
        if ratio != 1:
            assert not np.array_equal(np.stack([R.resize(m, (rm.shape[2] - int(pw), rm.shape[1] - int(ph))) for m in masks]),
                                      rm[:, :rm.shape[1] - int(ph), :rm.shape[2] - int(pw)])


def test_exact_2x_linear_is_the_area_average():
    rng = np.random.default_rng(5)
    for H, W in ((50, 70), (2, 2), (64, 6)):
        a = rng.integers(0, 256, (H, W), dtype=np.uint8)
        s = a.astype(np.int32)
        area = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
        assert np.array_equal(R.resize(a, (W // 2, H // 2)), area.astype(np.uint8))
    t = geometry.resize_tables(50, 70, 25, 35)
    assert set(t['x'][1].tolist()) == {1024} and set(t['x'][2].tolist()) == {1024} and np.array_equal(t['y'][0], 2 * np.arange(25))


@pytest.mark.parametrize('src,dsize', FLOAT_SHAPES)
def test_fixed_point_linear_against_float64(src, dsize):
    """max |diff| < 1.3 grey levels: 0.5 (final rounding) + 0.5 (the two >> 16) + 0.25 (coefficient rounding, two passes) + 0.01 (>> 4)."""
    H, W = src
    rng = np.random.default_rng(H * 1000 + W)
    for a in (rng.integers(0, 256, (H, W), dtype=np.uint8), G.soft_planes(H + W, 1, H, W)[0]):
        diff = np.abs(R.resize(a, dsize).astype(np.float64) - M.resize_float(a, dsize)).max()
        print('%s -> %s: max |fixed - float64| = %.4f' % (src, dsize, diff))
        assert diff < 1.3


@pytest.mark.parametrize('src,dsize', FLOAT_SHAPES)
def test_nearest_against_floor_indexed_slicing(src, dsize):
    H, W = src
    dw, dh = dsize
    a = np.random.default_rng(W * 1000 + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    ys = np.minimum(np.floor(np.arange(dh) * (H / dh)).astype(np.int64), H - 1)
    xs = np.minimum(np.floor(np.arange(dw) * (W / dw)).astype(np.int64), W - 1)
    assert np.array_equal(R.resize(a, dsize, interpolation=R.INTER_NEAREST), a[ys][:, xs])
    assert np.array_equal(geometry.nearest_axis(H, dh), R.nearest_axis(H, dh)) and np.array_equal(geometry.nearest_axis(W, dw), R.nearest_axis(W, dw))


def test_argument_errors_raise_before_the_device():
    u8 = np.zeros((8, 12), np.uint8)
    f = np.zeros((8, 12, 3), np.uint8)
    with pytest.raises(TypeError):
        geometry.resize(u8.astype(np.float32), (4, 4))
    with pytest.raises(TypeError):
        geometry.resize(u8, (4.0, 4))
    with pytest.raises(ValueError):
        geometry.resize(u8, (0, 4))
    with pytest.raises(ValueError):
        geometry.resize(u8, (4, 4), interpolation='cubic')
    with pytest.raises(ValueError):
        geometry.resize(np.zeros((8,), np.uint8), (4, 4))
    with pytest.raises(ValueError):
        geometry.resize(np.zeros((8, 12, 4), np.uint8), (4, 4), channels=3)
    with pytest.raises(ValueError):
        geometry.resize(u8, (4, 4), regime='lds')
    with pytest.raises(ValueError):
        geometry.plan(8, 12, 0)
    with pytest.raises(TypeError):
        geometry.plan(8, 12, 7.5)
    with pytest.raises(ValueError):
        geometry.plan(0, 12, 8)
    with pytest.raises(ValueError):
        geometry.plan(49, 490, 1)                                              # int(49 * (1 / 49)) is 0: an empty destination
    with pytest.raises(ValueError):
        geometry.resize_short_pad(np.zeros((8, 12, 4), np.uint8), short_size=8)
    with pytest.raises(ValueError):
        geometry.resize_short_pad(f, alphas_u8=np.zeros((2, 8, 13), np.uint8), short_size=8)
    with pytest.raises(TypeError):
        geometry.resize_pad_normalize(f.astype(np.int32), 8)
    with pytest.raises(ValueError):
        geometry.resize_pad_planes(np.zeros((1, 2, 8, 12), np.uint8), 8, down8=True)            # linear cannot be composed
    with pytest.raises(ValueError):
        geometry.resize_pad_planes(np.zeros((2, 8, 12), np.uint8), 8)
    pre = DevicePreprocessor()
    with pytest.raises(ValueError):
        pre.eval_item(np.zeros((1, 8, 12, 1), np.uint8), np.zeros((1, 1, 8, 12), np.uint8))
    with pytest.raises(TypeError):
        pre.eval_item(f[None], np.zeros((1, 1, 8, 12), np.float32))
    with pytest.raises(ValueError):
        pre.eval_item(f[None], np.zeros((1, 1, 8, 13), np.uint8))
    with pytest.raises(ValueError):
        pre.eval_item(f[None], np.zeros((1, 1, 8, 12), np.uint8), short_size=0)
    with pytest.raises(ValueError):
        pre.predict_item(f[None], np.zeros((1, 8, 12), np.uint8))
    with pytest.raises(ValueError):
        pre.predict_item(f, np.zeros((0, 8, 12), np.uint8))


def test_no_gpu_raises_maggie_hip_error():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    u8 = np.zeros((8, 12), np.uint8)
    f = np.zeros((1, 8, 12, 3), np.uint8)
    with pytest.raises(MaggieHipError):
        geometry.resize(u8, (6, 4))
    with pytest.raises(MaggieHipError):
        geometry.resize_short_pad(f, short_size=4)
    with pytest.raises(MaggieHipError):
        geometry.resize_pad_normalize(f, 4)
    with pytest.raises(MaggieHipError):
        DevicePreprocessor().eval_item(f, np.zeros((1, 1, 8, 12), np.uint8), short_size=4)
    with pytest.raises(MaggieHipError):
        DevicePreprocessor().predict_item(f[0], np.zeros((1, 8, 12), np.uint8), short_size=4)


def test_call_signature_is_unchanged():
    sig = inspect.signature(DevicePreprocessor.__call__)
    assert str(sig) == '(self, frames_u8, alphas_u8=None, masks_u8=None, slot_ids=None, *, transition=None, trimap=False, mask_draws=None)'
    assert str(inspect.signature(DevicePreprocessor.__init__)).startswith('(self, max_inst=10, downscale_mask=True, mean=')
