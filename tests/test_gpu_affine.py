"""RandomAffine on the device (csrc/affine.hip, maggie_amd.utils.affine, DevicePreprocessor.train_item_affine): the nearest warp of the
planes, the linear warp of the frames in both regimes with its min / max words, the channel shift with Normalize, against the NumPy restatement
(tests/affine_restatement.py), the pre-existing kernels (DevicePreprocessor.__call__, train_item) and the reference's own class
(tests/golden/affine_pinned.npz). Integer work, a float64 add and clamp, IEEE divisions: every comparison is exact."""
import faulthandler
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import affine_restatement as A                                        # noqa: E402
import crop_restatement as C                                          # noqa: E402
import geometry_restatement as R                                      # noqa: E402
import maskgen_restatement as M                                       # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import affine, crop                             # noqa: E402
from maggie_amd.utils import maskgen as MG                            # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor            # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(A.GOLDEN)
FIRED = [n for n in CASES if n != 'skipped']
WIDTHS = (1, 3, 4, 15, 16, 17, 63, 64, 65)                                  # the packed-store and tile edges
HEIGHTS = (1, 31, 32, 33)
_CACHE = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq(out, ref):
    return torch.equal(out.cpu(), torch.from_numpy(np.ascontiguousarray(ref)))


def _unaligned(t):
    """The same tensor at a base one byte past an allocation: 16-byte (or 4-byte) aligned only by chance."""
    flat = torch.cat([torch.zeros(1, dtype=t.dtype, device=t.device), t.reshape(-1)])[1:]
    assert flat.data_ptr() % 4 != 0
    return flat.view(t.shape)


def _case(name):
    """Inputs and the restated result of a fixture case, computed once and left unchanged."""
    if name not in _CACHE:
        _CACHE[name] = (A.GOLDEN[name],) + tuple(A.golden_inputs(name)) + (A.golden_run(name)[0],)
    return _CACHE[name]


def _composed(theta, shear, form, zx, zy, H, W):
    """The matrix the reference hands to cv2 for these parameters (degrees), composed as it composes them."""
    t, s = np.pi / 180 * theta, np.pi / 180 * shear
    rot = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
    sh = np.array([[1, -np.sin(s), 0], [0, np.cos(s), 0], [0, 0, 1]]) if form == 0 else np.array([[np.cos(s), 0, 0], [np.sin(s), 1, 0], [0, 0, 1]])
    m = A.offset_center(np.dot(np.dot(rot, sh), np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]])), H, W)
    return np.array([[m[1, 1], m[1, 0], m[1, 2]], [m[0, 1], m[0, 0], m[0, 2]]])


def _matrices(H, W):
    cx, cy = (W - 1) / 2, (H - 1) / 2
    out = {'identity': [[1, 0, 0], [0, 1, 0]], 'right': [[1, 0, 3], [0, 1, 0]], 'left': [[1, 0, -3], [0, 1, 0]], 'down': [[1, 0, 0], [0, 1, 2]],
           'up': [[1, 0, 0], [0, 1, -2]], 'half_x': [[1, 0, 0.5], [0, 1, 0]], 'half_y': [[1, 0, 0], [0, 1, 0.5]],
           'half_xy': [[1, 0, -0.5], [0, 1, -0.5]],
           'rot90': [[0, -1, cx + cy], [1, 0, cy - cx]],                      # a quarter turn about the centre
           'zoom2': [[2, 0, -cx], [0, 2, -cy]], 'zoom_half': [[0.5, 0, cx / 2], [0, 0.5, cy / 2]],
           'outside': [[1, 0, 4.0 * W + 7], [0, 1, 0]], 'far_outside': [[1, 0, 1e12], [0, 1, -1e12]],
           'singular': [[1, 2, 3], [2, 4, 5]]}
    for theta in (-10, 10):
        for form in (0, 1):
            for shear, zx, zy in ((5, 0.95, 0.95), (-5, 1.05, 1.05)):
                out['ref_%+d_%d_%+d' % (theta, form, shear)] = _composed(theta, shear, form, zx, zy, H, W)
    return out


def _pixels(seed, T, P, H, W):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 256, (T, H, W, 3), dtype=np.uint8), rng.integers(0, 256, (P, H, W), dtype=np.uint8)


def _restated(frames, planes, matrix, H, W):
    lin, near = A.tables(np.asarray(matrix, np.float64), H, W, A.INTER_LINEAR), A.tables(np.asarray(matrix, np.float64), H, W, A.INTER_NEAREST)
    return np.stack([A.warp_linear(f, lin) for f in frames]), np.stack([A.warp_nearest(p, near) for p in planes])


# ---- the warps -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W', WIDTHS)
def test_warp_of_every_matrix_at_every_size_in_both_regimes(W):
    """Identity, integer translations in the four directions, half-pixel shifts, +-10 degrees with both shear forms at the zoom extremes, a
    quarter turn, zoom 2 and 0.5, everything mapped outside, a singular matrix; T = 1 / 3 and P = 1 / 30 alternate; bases aligned and not."""
    dev = _dev()
    k = 0
    for H in HEIGHTS:
        for name, matrix in _matrices(H, W).items():
            k += 1
            T, P = (1, 30) if k % 2 else (3, 1)
            frames, planes = _pixels(1000 * W + k, T, P, H, W)
            want_f, want_p = _restated(frames, planes, matrix, H, W)
            d = affine.from_matrix(matrix, H, W)
            f, p = _T(frames, dev), _T(planes, dev)
            if k % 3 == 0:
                f, p = _unaligned(f), _unaligned(p)
            got_f, got_p, mm = affine.warp(f, p, d if k % 4 else d.to(dev), regime='direct', return_minmax=True)
            assert got_f.dtype == got_p.dtype == torch.uint8 and _eq(got_f, want_f) and _eq(got_p, want_p), (H, name)
            assert mm.dtype == torch.int32 and _eq(mm, A.minmax(want_f)), (H, name)
            if d.staged_ok:
                staged, _, mm2 = affine.warp(f, None, d, regime='staged', return_minmax=True)
                assert torch.equal(staged, got_f) and torch.equal(mm2, mm), (H, name)
            if name in ('outside', 'far_outside'):
                assert int(got_f.max()) == 0 and int(got_p.max()) == 0 and mm.cpu().tolist() == [[0, 0]] * T
            if name == 'identity':
                assert _eq(got_f, frames) and _eq(got_p, planes)


@pytest.mark.parametrize('offset', [0, 1, 2])
def test_warp_into_unaligned_outputs(offset):
    """The C entries with output bases that are no multiple of 4: the per-element stores give the bytes of the packed ones."""
    dev = _dev()
    H, W, T, P = 33, 64, 2, 3
    frames, planes = _pixels(77, T, P, H, W)
    matrix = _composed(10, 5, 0, 1.05, 0.95, H, W)
    want_f, want_p = _restated(frames, planes, matrix, H, W)
    d = affine.from_matrix(matrix, H, W).to(dev)
    f, p = _T(frames, dev), _T(planes, dev)
    out_f = torch.full((T * H * W * 3 + 8,), 7, dtype=torch.uint8, device=dev)
    out_p = torch.full((P * H * W + 8,), 7, dtype=torch.uint8, device=dev)
    mm = torch.empty((T, 2), dtype=torch.int32, device=dev)
    for regime in (affine.STAGED, affine.DIRECT):
        out_f.fill_(7)
        hip.call('mg_affine_warp_frames', hip.ptr(f), hip.ptr(out_f[offset:]), hip.ptr(d.linear), hip.ptr(mm), hip.c_long(T), hip.c_int(H), hip.c_int(W),
                 hip.c_int(regime), hip.stream())
        assert _eq(out_f[offset:offset + want_f.size], want_f.reshape(-1)) and _eq(mm, A.minmax(want_f))
        assert out_f[:offset].cpu().tolist() == [7] * offset and out_f[offset + want_f.size:].cpu().tolist() == [7] * (8 - offset)
    hip.call('mg_affine_warp_planes', hip.ptr(p), hip.ptr(out_p[offset:]), hip.ptr(d.nearest), hip.c_long(P), hip.c_int(H), hip.c_int(W), hip.stream())
    assert _eq(out_p[offset:offset + want_p.size], want_p.reshape(-1))
    assert out_p[:offset].cpu().tolist() == [7] * offset and out_p[offset + want_p.size:].cpu().tolist() == [7] * (8 - offset)


def test_several_tiles_leading_dimensions_and_the_regimes_on_a_larger_frame():
    """150 x 200: 5 x 4 tiles with ragged edges. The reference's extremes are staged; a quarter turn still fits the box budget, a tenfold reduction does
    not -- the staged kernel reads those tiles' taps from global memory and still gives the direct regime's bits."""
    dev = _dev()
    H, W = 150, 200
    rng = np.random.default_rng(5)
    frames = rng.integers(1, 256, (2, 2, H, W, 3), dtype=np.uint8)
    planes = rng.integers(0, 256, (2, 2, 3, H, W), dtype=np.uint8)
    f, p = _T(frames, dev), _T(planes, dev)
    for name, matrix in (('ref', _composed(-10, 5, 1, 0.95, 1.05, H, W)), ('rot90', [[0, -1, 170], [1, 0, -20]]), ('tenth', [[0.1, 0, 50], [0, 0.1, 40]]),
                         ('zoom3', [[3, 0, -200], [0, 3, -150]])):
        want_f, want_p = _restated(frames.reshape(4, H, W, 3), planes.reshape(12, H, W), matrix, H, W)
        d = affine.from_matrix(matrix, H, W)
        got_f, got_p, mm = affine.warp(f, p, d, regime='direct', return_minmax=True)
        assert tuple(got_f.shape) == (2, 2, H, W, 3) and tuple(got_p.shape) == (2, 2, 3, H, W) and tuple(mm.shape) == (4, 2)
        assert _eq(got_f.reshape(4, H, W, 3), want_f) and _eq(got_p.reshape(12, H, W), want_p) and _eq(mm, A.minmax(want_f)), name
        assert d.staged_ok == (name != 'tenth'), name
        # the staged kernel through the C entry whatever the host would choose: tiles whose box does not fit fall back per tile
        dd = d.to(dev)
        out = torch.empty_like(got_f)
        mm2 = torch.empty_like(mm)
        hip.call('mg_affine_warp_frames', hip.ptr(f), hip.ptr(out), hip.ptr(dd.linear), hip.ptr(mm2), hip.c_long(4), hip.c_int(H), hip.c_int(W),
                 hip.c_int(affine.STAGED), hip.stream())
        assert torch.equal(out, got_f) and torch.equal(mm2, mm), name
        auto_f, _ = affine.warp(f, None, d)
        assert torch.equal(auto_f, got_f)


def test_wrong_tables_give_wrong_pixels_never_an_out_of_bounds_access():
    """Tables that no matrix produces -- not monotone, huge, wrapping sums: every derived index is range-tested, and both regimes still agree
    with the restated reading of the same tables."""
    dev = _dev()
    H, W = 40, 70
    frames, planes = _pixels(9, 2, 3, H, W)
    rng = np.random.default_rng(10)
    n = 2 * (H + W)
    for kind in ('random_small', 'random_huge', 'zigzag'):
        if kind == 'random_small':
            tab = rng.integers(-20 * 1024, (W + 20) * 1024, n)
        elif kind == 'random_huge':
            tab = rng.integers(-2 ** 31, 2 ** 31, n)
        else:
            tab = np.concatenate([(np.arange(W) % 2) * 30 * 1024 + np.arange(W) * 1024, np.zeros(W, np.int64), np.zeros(H, np.int64) + 16,
                                  (np.arange(H)[::-1]) * 1024 + 16])
        tab = np.asarray(tab, np.int64).astype(np.int32)

        def wsum(a, b):
            return (a + b + 2 ** 31) % 2 ** 32 - 2 ** 31                          # int32 wrap-around
        adelta, bdelta, X0, Y0 = (a.astype(np.int64) for a in affine.split(tab, H, W))
        Xs, Ys = wsum(X0[:, None], adelta[None, :]), wsum(Y0[:, None], bdelta[None, :])
        want_p = np.stack([A._taps(p, Ys >> 10, Xs >> 10).astype(np.uint8) for p in planes])

        def lin(src):
            X, Y = Xs >> 5, Ys >> 5
            sx, sy, fx, fy = X >> 5, Y >> 5, (X & 31)[..., None], (Y & 31)[..., None]
            acc = (32 * (32 - fx) * (32 - fy) * A._taps(src, sy, sx) + 32 * fx * (32 - fy) * A._taps(src, sy, sx + 1) +
                   32 * (32 - fx) * fy * A._taps(src, sy + 1, sx) + 32 * fx * fy * A._taps(src, sy + 1, sx + 1))
            return ((acc + 16384) >> 15).astype(np.uint8)
        want_f = np.stack([lin(f) for f in frames])
        d = affine.AffineDraws(True, H, W, None, 0.0, None, tab, tab, np.zeros(1), True).to(dev)
        for regime in ('staged', 'direct'):
            got_f, got_p, mm = affine.warp(_T(frames, dev), _T(planes, dev), d, regime=regime, return_minmax=True)
            assert _eq(got_f, want_f) and _eq(got_p, want_p) and _eq(mm, A.minmax(want_f)), (kind, regime)


def test_minmax_of_a_frame_whose_extreme_is_a_border_blended_pixel():
    """A constant frame of 200 shifted by half a pixel: the first column blends with the border's 0 and holds 100, the only place the minimum
    lives; a frame of 1 with one pixel of 255 whose half-pixel blend (128) is the maximum."""
    dev = _dev()
    H, W = 33, 65
    frames = np.full((2, H, W, 3), 200, np.uint8)
    frames[1] = 1
    frames[1, 20, 40, 1] = 255
    d = affine.from_matrix([[1, 0, 0.5], [0, 1, 0]], H, W)
    want = np.stack([A.warpAffine(f, d.matrix, (W, H)) for f in frames])
    assert want[0].min() == 100 and (want[0] == 100).sum() == 3 * H and want[0, :, 1:].min() == 200
    assert want[1].max() == 128 and (want[1] == 128).sum() == 2 and want[1].min() == 1
    for regime in ('staged', 'direct'):
        got, _, mm = affine.warp(_T(frames, dev), None, d, regime=regime, return_minmax=True)
        assert _eq(got, want) and mm.cpu().tolist() == [[100, 200], [1, 128]] == A.minmax(want).tolist(), regime


# ---- the channel shift ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(1, 1), (5, 7), (8, 16), (33, 65)])
def test_shift_normalize_equals_the_float64_restatement(H, W):
    """Either sign, the clip active at the max (positive) and at the min (negative), a wide-open clip, mn == mx, and min / max words that are
    not the frames' own; H * W a multiple of 4 (16-byte stores) and not."""
    dev = _dev()
    frames = np.random.default_rng(H * W).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    frames[2] = 93                                                            # mn == mx
    f = _T(frames, dev)
    own = A.minmax(frames)
    for intensity in (7.649999, -7.649999, 0.3, -0.0001, 0.0, 2.0 ** -40, -5.5):
        want = A.shift_normalized(frames, intensity)
        for ff in (f, _unaligned(f)):
            got = affine.shift_normalize(ff, own, intensity)
            assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3, H, W) and _eq(got, want), intensity
        assert _eq(affine.shift_normalize(f, _T(own, dev), torch.tensor([intensity], dtype=torch.float64, device=dev)), want)
        if H * W > 1 and intensity > 0.1:
            assert (frames[0].astype(np.float64) + intensity > own[0, 1]).any()                  # the clip is active at the max
        if H * W > 1 and intensity < -0.1:
            assert (frames[0].astype(np.float64) + intensity < own[0, 0]).any()                  # ... and at the min
        for mm in (np.asarray([[0, 255]] * 3, np.int32), np.asarray([[100, 140], [0, 3], [93, 93]], np.int32)):
            assert _eq(affine.shift_normalize(f, mm, intensity), A.shift_normalized(frames, intensity, mm=mm)), (intensity, mm.tolist())
    mean, std = (0.5, 0.25, 0.125), (0.3, 0.2, 0.1)
    assert _eq(affine.shift_normalize(f, own, 3.25, mean, std), A.shift_normalized(frames, 3.25, mean, std))
    # intensity 0 with the frames' own min / max is ToTensor + Normalize of the uint8 frames
    assert _eq(affine.shift_normalize(f, own, 0.0), R.normalized(frames))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_draw_then_apply_equals_the_fixture(name):
    dev = _dev()
    d = load_golden('affine_pinned.npz')
    c, frames, alphas, _, r = _case(name)
    rs = np.random.RandomState(c['rs_seed'])
    draws = affine.draw(rs, c['h'], c['w'], c['p'])
    assert np.array_equal(A.state_digest(rs), d[name + '.state'])              # the generator is where the reference left it
    fix_f, fix_a = R.unpack_rows(d[name + '.frames']), R.unpack_rows(d[name + '.alphas'])
    if name == 'skipped':
        assert not draws.fired and np.array_equal(fix_f, frames) and np.array_equal(fix_a, alphas)
        with pytest.raises(ValueError):
            affine.apply(_T(frames, dev), _T(alphas, dev), draws)
        return
    assert draws.fired and draws.intensity == d[name + '.intensity'][0] and np.array_equal(draws.matrix, d[name + '.matrix'])
    for dd in (draws, draws.to(dev)):
        for regime in ('staged', 'direct', None):
            gf, ga, mm = affine.warp(_T(frames, dev), _T(alphas, dev), dd, regime=regime, return_minmax=True)
            assert _eq(gf, fix_f) and _eq(ga, fix_a) and _eq(mm, d[name + '.minmax']), regime
            image, ga = affine.apply(_T(frames, dev), _T(alphas, dev), dd, regime=regime)
            assert image.dtype == torch.float32 and tuple(image.shape) == (c['T'], 3, c['h'], c['w']) and _eq(ga, fix_a)
            # the reference's float64 frames through ToTensor's .float() and Normalize
            assert _eq(image, A.shift_normalized(fix_f, draws.intensity)), regime
            x = r['frames'].astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255)
            assert _eq(image, (x - np.asarray(affine.IMAGENET_MEAN, np.float32).reshape(1, 3, 1, 1)) /
                       np.asarray(affine.IMAGENET_STD, np.float32).reshape(1, 3, 1, 1))
    image, none = affine.apply(frames, None, draws)                             # host arrays, no alphas
    assert none is None and _eq(image, A.shift_normalized(fix_f, draws.intensity))


@pytest.mark.parametrize('name', ['first_hit', 'mean_vs_any', 'pad_wide_odd'])
def test_train_item_affine_in_both_mask_wirings(name):
    """The crop cases of the training crop, then RandomAffine on the crops: 'alpha', 'mask' and 'transition' against `__call__` on the restated
    arrays, 'image' against the float64 restatement; without draws, or with draws that did not fire, today's train_item bit for bit."""
    dev = _dev()
    c = C.GOLDEN[name]
    frames, alphas, masks = C.golden_inputs(name)
    r = C.golden_run(name)[0]
    T, n = c['T'], c['n']
    oh, ow = r['alphas'].shape[-2:]
    pre = DevicePreprocessor(max_inst=6, device=dev)
    ids = [4, 1][:n]
    cd = crop.draw_on_device(np.random.RandomState(c['rs_seed']), alphas, c['crop'], c['pp'], c['fp']).to(dev)
    ad = affine.draw(np.random.RandomState(7), oh, ow, p=1.0)
    assert ad.fired and ad.matrix is not None
    unfired = affine.draw(np.random.RandomState(5), oh, ow, p=0.1)
    assert not unfired.fired
    md = MG.draw_chain(np.random.RandomState(9), random.Random(9), T * n, oh, ow, from_alpha=T > 1)
    f, a, m = _T(frames, dev), _T(alphas.reshape(T, n, c['h'], c['w']), dev), _T(masks.reshape(T, n, c['h'], c['w']), dev)
    wf, wa = _restated(r['frames'], r['alphas'], ad.matrix, oh, ow)
    assert not np.array_equal(wa, r['alphas'])
    image = A.shift_normalized(wf, ad.intensity)
    wa4, ra4, rm4 = wa.reshape(T, n, oh, ow), r['alphas'].reshape(T, n, oh, ow), r['masks'].reshape(T, n, oh, ow)
    for dd in (ad, ad.to(dev)):
        # the image loader: the alphas are the masks' source, and the chain sees the UNWARPED crop of them
        got = pre.train_item_affine(f, a, a, cd, dd, ids, transition=(3, 2), mask_draws=md)
        want = pre(_T(wf, dev), _T(wa4, dev), _T(ra4, dev), ids, transition=(3, 2), mask_draws=md)
        assert list(got) == list(want) == ['image', 'alpha', 'mask', 'transition']
        assert _eq(got['image'], image) and got['image'].dtype == torch.float32
        for key in ('alpha', 'mask', 'transition'):
            assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
        assert _eq(got['mask'], pre(wf, wa4, M.chain(r['alphas'], md).reshape(T, n, oh, ow), ids)['mask'].cpu().numpy())
        # masks of their own stay unwarped too
        got = pre.train_item_affine(f, a, m, cd, dd, ids)
        want = pre(_T(wf, dev), _T(wa4, dev), _T(rm4, dev), ids)
        assert list(got) == list(want) == ['image', 'alpha', 'mask'] and _eq(got['image'], image)
        assert torch.equal(got['alpha'], want['alpha']) and torch.equal(got['mask'], want['mask'])
        # the video loader: the masks are regenerated from the WARPED alphas
        got = pre.train_item_affine(f, a, a, cd, dd, ids, transition=(3, 2), mask_draws=md, warp_masks=True)
        want = pre(_T(wf, dev), _T(wa4, dev), _T(wa4, dev), ids, transition=(3, 2), mask_draws=md)
        for key in ('alpha', 'mask', 'transition'):
            assert torch.equal(got[key], want[key]), key
        assert _eq(got['image'], image)
        if name == 'first_hit':                                               # the two wirings are visibly different items (one case shows it)
            assert not torch.equal(got['mask'], pre.train_item_affine(f, a, a, cd, dd, ids, mask_draws=md)['mask'])
    # no draws, or draws that did not fire: today's path
    today = pre.train_item(f, a, a, cd, ids, transition=(3, 2), mask_draws=md)
    for dd in (None, unfired):
        for wm in (False, True):
            got = pre.train_item_affine(f, a, a, cd, dd, ids, transition=(3, 2), mask_draws=md, warp_masks=wm)
            assert list(got) == list(today) and all(torch.equal(got[k], today[k]) for k in today)
    # the tone table is applied on the raw crop, before the warp
    lut = np.random.default_rng(17).integers(0, 256, (3, 256), dtype=np.uint8)
    toned = np.stack([lut[ch][r['frames'][..., ch]] for ch in range(3)], -1)
    got = pre.train_item_affine(f, a, m, cd, ad, ids, lut=lut)
    assert _eq(got['image'], A.shift_normalized(_restated(toned, r['alphas'], ad.matrix, oh, ow)[0], ad.intensity))


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_apply_replays_with_new_pixels_and_rewritten_tables():
    dev = _dev()
    c, frames, alphas, _, r = _case('clip')
    H, W, T = c['h'], c['w'], c['T']
    other_f, other_a = R.frames_of(92, T, H, W), R.alphas_of(93, alphas.shape[0], H, W)
    faulthandler.dump_traceback_later(120, exit=True)                      # the test's own time limit: a hung capture or replay ends the process
    try:
        sf, sa = _T(frames, dev), _T(alphas, dev)
        d = affine.from_matrix(r['matrix'], H, W, r['intensity']).to(dev)
        assert d.on_device and d.shift.dtype == torch.float64
        affine.apply(sf, sa, d)                                             # warm-up off the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            image, ga = affine.apply(sf, sa, d)
        for fr, al, matrix, intensity in ((other_f, other_a, _composed(10, -5, 1, 1.05, 0.95, H, W), -6.5), (frames, alphas, r['matrix'], r['intensity']),
                                          (other_f, alphas, [[1, 0, 0.5], [0, 1, -3]], 0.75)):
            new = affine.from_matrix(matrix, H, W, intensity)
            sf.copy_(_T(fr, dev))
            sa.copy_(_T(al, dev))
            d.linear.copy_(torch.from_numpy(new.linear))
            d.nearest.copy_(torch.from_numpy(new.nearest))
            d.shift.copy_(torch.from_numpy(new.shift))
            g.replay()
            torch.cuda.synchronize()
            wf, wa = _restated(fr, al, matrix, H, W)
            assert _eq(image, A.shift_normalized(wf, intensity)) and _eq(ga, wa), intensity
        del g
    finally:
        faulthandler.cancel_dump_traceback_later()
