"""MotionBlur on the device (csrc/motion.hip, maggie_amd.utils.motion, DevicePreprocessor.train_item_motion): the frames' and the planes'
launch, both epilogues, sources smaller than the reach, tile edges, unaligned bases, a rewritten and an out-of-range table, and the training
item's wirings, against the integer NumPy restatement (tests/motion_restatement.py, which tests/test_motion_cpu.py holds against scipy's
fp64 correlation on these very cases) and the fixture scipy wrote (tests/golden/motion_pinned.npz). Integer work and the IEEE divisions of
Normalize: every comparison is exact."""
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
import motion_restatement as M                                        # noqa: E402
import photometric_restatement as P                                   # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.hip import c_int, c_long                              # noqa: E402
from maggie_amd.utils import affine, crop, motion, photometric        # noqa: E402
from maggie_amd.utils import maskgen as MG                            # noqa: E402
from maggie_amd.utils._inputs import float3                           # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor, normalize_frames       # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_motion_golden as G                                        # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = photometric.IMAGENET_MEAN, photometric.IMAGENET_STD
_REF = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq(out, ref):
    return torch.equal(out.cpu(), torch.from_numpy(np.ascontiguousarray(ref)))


def _unaligned(t):
    """The same tensor at a base one byte past an allocation: 4-byte aligned only by chance."""
    flat = torch.cat([torch.zeros(1, dtype=t.dtype, device=t.device), t.reshape(-1)])[1:]
    assert flat.data_ptr() % 4 != 0
    return flat.view(t.shape)


def _case(h, w, kname):
    """The frames and planes of a shape and their restated blur with a kernel, computed once and left unchanged."""
    if (h, w) not in _REF:
        _REF[(h, w)] = (M.case_frames(h, w), M.case_planes(h, w))
    if (h, w, kname) not in _REF:
        f, p = _REF[(h, w)]
        offs = M.offsets(M.KERNELS[kname])
        _REF[(h, w, kname)] = (M.blur_frames(f, offs), M.blur_planes(p, offs))
    return _REF[(h, w)] + _REF[(h, w, kname)]


def _same_as_normalize_frames(norm, raw_u8, dev):
    """The Normalize epilogue against `normalize_frames` of the raw result, where that function is defined (it takes h * w % 4 == 0 only)."""
    h, w = raw_u8.shape[-3:-1]
    return (h * w) % 4 != 0 or torch.equal(norm, normalize_frames(raw_u8, MEAN, STD, dev))


# ---- the two launches ------------------------------------------------------------------------------------------------------------------------------
def test_the_tile_is_the_one_the_shapes_were_chosen_for():
    _dev()
    v = [c_int() for _ in range(6)]
    assert hip.lib().mg_motion_limits(*[hip.ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [49, 49, M.TILE_ROWS, M.TILE_COLS, motion.TABLE, motion.MAX_SIDE]


@pytest.mark.parametrize('shape', M.SHAPES, ids=lambda s: '%dx%d' % s)
def test_blur_equals_the_restatement(shape):
    """3 frames (random, all 255, checkerboard) and 7 planes under every kernel: ties (n = 2, 8), n = 49 in three directions (all 255 fills
    the 16-bit sums), the one-sided halo, n = 1; raw and normalised; host and device tables."""
    dev = _dev()
    h, w = shape
    for k, (kname, K) in enumerate(M.KERNELS.items()):
        f, p, want_f, want_p = _case(h, w, kname)
        d = motion.MotionDraws(K)
        d = d.to(dev) if k % 2 else d
        got_f, got_p = motion.apply(_T(f, dev), p, d)                       # the planes from the host: uploaded by the call
        assert got_f.dtype == got_p.dtype == torch.uint8 and got_f.is_cuda and got_p.is_cuda
        assert _eq(got_f, want_f), kname
        assert _eq(got_p, want_p), kname
        norm, again = motion.apply(f, _T(p.reshape(7, 1, h, w), dev), d, normalize=True, mean=MEAN, std=STD, device=dev)
        assert norm.dtype == torch.float32 and tuple(norm.shape) == (3, 3, h, w) and tuple(again.shape) == (7, 1, h, w)
        assert _eq(norm, P.normalize(want_f, MEAN, STD)) and _same_as_normalize_frames(norm, got_f, dev), kname
        assert _eq(again.reshape(7, h, w), want_p)
        assert _eq(motion.blur_frames(f[1], d), want_f[1]) and _eq(motion.blur_planes(_T(p[:2], dev), d), want_p[:2]), kname
    if (h, w) == M.SHAPES[-1]:
        assert w % 4 and (3 * w) % 4 and w > 2 * M.TILE_COLS
    white = np.full((h, w, 3), 255, np.uint8)
    assert _eq(motion.blur_frames(white, motion.MotionDraws(M.KERNELS['k49_diagonal'])), white)      # 49 * 255 in every 16-bit field


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_unaligned_bases_take_the_per_element_paths(offset):
    """Rows of whole dwords (w = 68) on bases that are not: the source one byte past an allocation, the outputs `offset` bytes in."""
    dev = _dev()
    h, w = 33, 68
    f, p, want_f, want_p = _case(h, w, 'k13')
    table = _T(motion.taps_of(M.KERNELS['k13']), dev)
    d = motion.MotionDraws(taps=table)
    sf, sp = _unaligned(_T(f, dev)), _unaligned(_T(p, dev))
    assert _eq(motion.blur_frames(sf, d), want_f) and _eq(motion.blur_planes(sp, d), want_p)
    assert _eq(motion.blur_frames(sf, d, normalize=True), P.normalize(want_f, MEAN, STD))
    out_f = torch.full((f.size + 8,), 7, dtype=torch.uint8, device=dev)
    out_p = torch.full((p.size + 8,), 7, dtype=torch.uint8, device=dev)
    hip.call('mg_motion_frames', hip.ptr(_T(f, dev)), hip.ctypes.c_void_p(out_f.data_ptr() + offset), hip.ptr(table), c_long(3), c_int(h), c_int(w),
             c_int(motion.RAW), float3(MEAN), float3(STD), hip.stream())
    hip.call('mg_motion_planes', hip.ptr(sp), hip.ctypes.c_void_p(out_p.data_ptr() + offset), hip.ptr(table), c_long(7), c_int(h), c_int(w),
             hip.stream())
    torch.cuda.synchronize()
    for out, want in ((out_f, want_f), (out_p, want_p)):
        assert _eq(out[offset:offset + want.size], want.reshape(-1))
        assert (out[:offset] == 7).all() and (out[offset + want.size:] == 7).all()                   # nothing outside the result was written


def test_zero_frames_and_zero_planes():
    dev = _dev()
    d = motion.MotionDraws(M.KERNELS['k11']).to(dev)
    f, a = motion.apply(np.zeros((0, 5, 7, 3), np.uint8), np.zeros((0, 2, 5, 7), np.uint8), d)
    assert tuple(f.shape) == (0, 5, 7, 3) and tuple(a.shape) == (0, 2, 5, 7) and f.is_cuda and a.is_cuda
    f, a = motion.apply(np.zeros((0, 5, 7, 3), np.uint8), None, d, normalize=True)
    assert tuple(f.shape) == (0, 3, 5, 7) and f.dtype == torch.float32 and a is None
    f3, _, want_f, _ = _case(5, 7, 'k11')
    got_f, got_a = motion.apply(f3, np.zeros((0, 5, 7), np.uint8), d)       # frames without planes
    assert _eq(got_f, want_f) and tuple(got_a.shape) == (0, 5, 7)


def test_argument_errors_of_the_c_abi():
    dev = _dev()
    x, out, table = torch.zeros(3 * 4 * 4, dtype=torch.uint8, device=dev), torch.zeros(3 * 4 * 4 * 4, dtype=torch.uint8, device=dev), \
        _T(motion.taps_of(M.KERNELS['k3_n2']), dev)
    lib = hip.lib()
    m, s, st = float3(MEAN), float3(STD), hip.stream()
    frames = lambda i, o, t, n, h, w, e: lib.mg_motion_frames(hip.ptr(i), hip.ptr(o), hip.ptr(t), c_long(n), c_int(h), c_int(w), c_int(e), m, s, st)   # noqa: E731
    planes = lambda i, o, t, n, h, w: lib.mg_motion_planes(hip.ptr(i), hip.ptr(o), hip.ptr(t), c_long(n), c_int(h), c_int(w), st)   # noqa: E731
    assert frames(x, out, table, 1, 4, 4, 2) == -2 and frames(x, x, table, 1, 4, 4, 0) == -2 and frames(x, out, None, 1, 4, 4, 0) == -2
    assert frames(x, out, table, -1, 4, 4, 0) == -2 and frames(x, out, table, 1, 0, 4, 0) == -2 and frames(x, out, table, 1, 4, 32768, 0) == -2
    assert planes(x, x, table, 1, 4, 4) == -2 and planes(x, None, table, 1, 4, 4) == -2 and planes(x, out, None, 1, 4, 4) == -2
    assert planes(x, out, table, 1 << 40, 4, 4) == -3 and frames(x, out, table, 1 << 40, 4, 4, 0) == -3           # before any launch
    assert frames(None, None, None, 0, 4, 4, 0) == 0 and planes(None, None, None, 0, 4, 4) == 0
    torch.cuda.synchronize()


# ---- tables on the device ----------------------------------------------------------------------------------------------------------------------------
def test_a_table_outside_its_range_is_clamped():
    """A table rewritten on the device may hold anything: n = 60 and offsets of +-30 give the result of n = 49 and +-24. The table sits in a
    larger allocation, so nothing is read that the test does not own whatever the kernel makes of n."""
    dev = _dev()
    h, w = 33, 65
    f, p, _, _ = _case(h, w, 'k3_n2')
    rng = np.random.default_rng(11)
    wild = np.zeros(256, np.int32)
    wild[0], wild[1] = 60, 49
    wild[2:] = rng.integers(-30, 31, 254)
    wild[2], wild[3], wild[4], wild[5] = 30, -30, -2 ** 31, 2 ** 31 - 1
    offs = M.clamped_offsets(wild)
    assert len(offs) == 49 and offs[0] == (24, -24) and offs[1] == (-24, 24)
    store = _T(wild, dev)
    d = motion.MotionDraws(taps=store[:motion.TABLE])
    got_f, got_p = motion.apply(f, p, d, device=dev)
    assert _eq(got_f, M.blur_frames(f, offs)) and _eq(got_p, M.blur_planes(p, offs))
    low = wild.copy()
    low[0] = -5                                                            # n below 1: one tap
    store.copy_(_T(low, dev))
    assert _eq(motion.blur_planes(p, d, device=dev), M.blur_planes(p, M.clamped_offsets(low)))


def test_graph_capture_of_apply_follows_a_table_rewritten_in_place():
    dev = _dev()
    h, w = 33, 65
    faulthandler.dump_traceback_later(120, exit=True)                      # the test's own time limit: a hung capture or replay ends the process
    try:
        f, p, _, _ = _case(h, w, 'k11')
        sf, sp = _T(f, dev), _T(p, dev)
        d = motion.MotionDraws(M.KERNELS['k11']).to(dev)
        assert d.on_device and d.taps.dtype == torch.int32
        motion.apply(sf, sp, d, normalize=True)                            # warm-up off the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            image, alphas = motion.apply(sf, sp, d, normalize=True)
        for kname in ('k49_diagonal', 'k11', 'k49_corner', 'n1', 'k3_n2'):
            d.taps.copy_(_T(motion.taps_of(M.KERNELS[kname]), dev))
            g.replay()
            torch.cuda.synchronize()
            _, _, want_f, want_p = _case(h, w, kname)
            assert _eq(image, P.normalize(want_f, MEAN, STD)) and _eq(alphas, want_p), kname
        del g
    finally:
        faulthandler.cancel_dump_traceback_later()


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(G.CASES))
def test_blur_equals_the_fixture(name):
    dev = _dev()
    g = load_golden('motion_pinned.npz')
    x, K, want = g[name + '.input'], g[name + '.kernel'], g[name + '.output']
    d = motion.MotionDraws(K.astype(np.float32) / K.sum())                  # the normalised kernel, as albumentations hands it over
    got_f, got_p = motion.apply(x, np.moveaxis(x, -1, 0), d, device=dev)
    assert _eq(got_f, want) and _eq(got_p, np.moveaxis(want, -1, 0))
    assert _eq(motion.blur_frames(x, d, normalize=True, device=dev), P.normalize(want[None], MEAN, STD)[0])


# ---- the training item ---------------------------------------------------------------------------------------------------------------------------
def _item_inputs(dev):
    name = 'first_hit'                                                     # a crop of 64 x 64
    c = C.GOLDEN[name]
    frames, alphas, masks = C.golden_inputs(name)
    r = C.golden_run(name)[0]
    T, n = c['T'], c['n']
    oh, ow = r['alphas'].shape[-2:]
    assert (oh, ow) == (64, 64)
    x = dict(T=T, n=n, oh=oh, ow=ow, r=r, ids=[4, 1][:n], pre=DevicePreprocessor(max_inst=6, device=dev))
    x['cd'] = crop.draw_on_device(np.random.RandomState(c['rs_seed']), alphas, c['crop'], c['pp'], c['fp']).to(dev)
    x['md'] = MG.draw_chain(np.random.RandomState(9), random.Random(9), T * n, oh, ow, from_alpha=T > 1)
    x['f'], x['a'], x['m'] = _T(frames, dev), _T(alphas.reshape(T, n, c['h'], c['w']), dev), _T(masks.reshape(T, n, c['h'], c['w']), dev)
    rng = np.random.default_rng(1)
    x['crop_lut'], x['photo_lut'] = rng.integers(0, 256, (3, 256), dtype=np.uint8), rng.integers(0, 256, (3, 256), dtype=np.uint8)
    x['noise'] = rng.integers(-40, 41, (oh, ow, 1)).astype(np.int16)
    x['K'] = M.KERNELS['k11']
    x['offs'] = M.offsets(x['K'])
    x['toned'] = P.apply_lut(r['frames'], x['crop_lut'])                    # Gamma rides on the crop's table, before the blur
    x['alphas_blurred'] = M.blur_planes(r['alphas'], x['offs']).reshape(T, n, oh, ow)
    assert not np.array_equal(x['alphas_blurred'].reshape(r['alphas'].shape), r['alphas'])
    return x


def _assembled(x, alphas_u8, masks_u8, dev):
    """'alpha', 'mask' and 'transition' of restated uint8 planes through the stages their own tests pin (DevicePreprocessor.__call__)."""
    T, n, oh, ow = x['T'], x['n'], x['oh'], x['ow']
    return x['pre'](torch.zeros((T, oh, ow, 3), dtype=torch.uint8, device=dev), _T(alphas_u8.reshape(T, n, oh, ow), dev),
                    _T(masks_u8.reshape(T, n, oh, ow), dev), x['ids'], transition=(3, 2), mask_draws=x['md'])


def _planes_equal(got, want):
    assert list(got) == ['image', 'alpha', 'mask', 'transition']
    return all(torch.equal(got[k], want[k]) for k in ('alpha', 'mask', 'transition'))


def test_train_item_motion_blur_alone():
    """Crop -> curve -> blur -> item: the blur's Normalize epilogue writes 'image'; 'alpha' and 'transition' read the blurred alphas; the
    mask chain reads them when the masks are the alphas or with `warp_masks`, and the UNBLURRED cropped masks when they are separate."""
    dev = _dev()
    x = _item_inputs(dev)
    pre, r = x['pre'], x['r']
    want_image = P.normalize(M.blur_frames(x['toned'], x['offs']), MEAN, STD)
    from_alphas, separate = _assembled(x, x['alphas_blurred'], x['alphas_blurred'], dev), _assembled(x, x['alphas_blurred'], r['masks'], dev)
    assert not torch.equal(from_alphas['mask'], separate['mask'])
    for md in (motion.MotionDraws(x['K']), motion.MotionDraws(x['K']).to(dev)):
        kw = dict(transition=(3, 2), mask_draws=x['md'], lut=x['crop_lut'])
        got = pre.train_item_motion(x['f'], x['a'], x['a'], x['cd'], md, None, None, x['ids'], **kw)
        assert got['image'].dtype == torch.float32 and _eq(got['image'], want_image) and _planes_equal(got, from_alphas)
        got = pre.train_item_motion(x['f'], x['a'], x['m'], x['cd'], md, None, None, x['ids'], **kw)
        assert _eq(got['image'], want_image) and _planes_equal(got, separate)
        got = pre.train_item_motion(x['f'], x['a'], x['m'], x['cd'], md, photometric.PhotoDraws(), None, x['ids'], warp_masks=True, **kw)
        assert _eq(got['image'], want_image) and _planes_equal(got, from_alphas)
    unblurred = pre.train_item(x['f'], x['a'], x['a'], x['cd'], x['ids'], transition=(3, 2), mask_draws=x['md'], lut=x['crop_lut'])
    assert not torch.equal(got['image'], unblurred['image']) and not torch.equal(got['alpha'], unblurred['alpha'])


def test_train_item_motion_with_noise_and_jpeg():
    """Crop -> both curves -> blur -> noise -> JPEG: `photo.lut` joins the crop's table, so it comes BEFORE the blur as GammaContrast does."""
    dev = _dev()
    x = _item_inputs(dev)
    pre = x['pre']
    toned = P.apply_lut(x['toned'], x['photo_lut'])
    want_u8 = P.photometric(M.blur_frames(toned, x['offs']), None, x['noise'], 35)
    wrong_order = P.photometric(M.blur_frames(x['toned'], x['offs']), x['photo_lut'], x['noise'], 35)
    assert not np.array_equal(want_u8, wrong_order)
    want = _assembled(x, x['alphas_blurred'], x['alphas_blurred'], dev)
    photo = photometric.PhotoDraws(x['photo_lut'], x['noise'], 35)
    for md, pd in ((motion.MotionDraws(x['K']), photo), (motion.MotionDraws(x['K']).to(dev), photo.to(dev))):
        got = pre.train_item_motion(x['f'], x['a'], x['a'], x['cd'], md, pd, None, x['ids'], transition=(3, 2), mask_draws=x['md'],
                                    lut=x['crop_lut'])
        assert _eq(got['image'], P.normalize(want_u8, MEAN, STD)) and _planes_equal(got, want)
    # a lone curve in the draws: the blur's own epilogue again
    got = pre.train_item_motion(x['f'], x['a'], x['a'], x['cd'], md, photometric.PhotoDraws(lut=x['photo_lut']), None, x['ids'],
                                transition=(3, 2), mask_draws=x['md'], lut=x['crop_lut'])
    assert _eq(got['image'], P.normalize(M.blur_frames(toned, x['offs']), MEAN, STD)) and _planes_equal(got, want)


def test_train_item_motion_with_affine_and_warped_masks():
    """Crop -> curve -> blur -> RandomAffine: the warp reads the raw blurred frames and alphas; with `warp_masks` the mask chain reads the
    blurred and warped alphas, without it the blurred ones."""
    dev = _dev()
    x = _item_inputs(dev)
    pre, oh, ow = x['pre'], x['oh'], x['ow']
    ad = affine.draw(np.random.RandomState(7), oh, ow, p=1.0)
    assert ad.fired and ad.matrix is not None
    mat = np.asarray(ad.matrix, np.float64)
    lin, near = A.tables(mat, oh, ow, A.INTER_LINEAR), A.tables(mat, oh, ow, A.INTER_NEAREST)
    blurred = M.blur_frames(x['toned'], x['offs'])
    want_image = A.shift_normalized(np.stack([A.warp_linear(fr, lin) for fr in blurred]), ad.intensity)
    warped = np.stack([A.warp_nearest(pl, near) for pl in x['alphas_blurred'].reshape(-1, oh, ow)])
    assert not np.array_equal(warped.reshape(x['alphas_blurred'].shape), x['alphas_blurred'])
    kw = dict(transition=(3, 2), mask_draws=x['md'], lut=x['crop_lut'])
    md = motion.MotionDraws(x['K']).to(dev)
    for masks in (x['a'], x['m']):
        got = pre.train_item_motion(x['f'], x['a'], masks, x['cd'], md, None, ad, x['ids'], warp_masks=True, **kw)
        assert _eq(got['image'], want_image) and _planes_equal(got, _assembled(x, warped, warped, dev))
    got = pre.train_item_motion(x['f'], x['a'], x['a'], x['cd'], md, None, ad, x['ids'], warp_masks=False, **kw)
    assert _eq(got['image'], want_image) and _planes_equal(got, _assembled(x, warped, x['alphas_blurred'], dev))


def test_train_item_motion_not_fired_is_train_item_photo(monkeypatch):
    dev = _dev()
    x = _item_inputs(dev)
    pre = x['pre']
    ad = affine.draw(np.random.RandomState(7), x['oh'], x['ow'], p=1.0)
    photo = photometric.PhotoDraws(x['photo_lut'], x['noise'], 35)
    rs = np.random.RandomState(0)
    unfired = motion.draw(rs, p=0.0)
    assert not unfired.fired
    calls, real = [], DevicePreprocessor.train_item_photo

    def recorded(self, *args, **kwargs):
        calls.append((args, kwargs))
        return real(self, *args, **kwargs)
    for md in (None, unfired, motion.MotionDraws()):
        for pd, dd, masks, wm in ((None, None, x['a'], False), (photo, None, x['m'], False), (photo, ad, x['a'], True)):
            kw = dict(transition=(3, 2), mask_draws=x['md'], lut=x['crop_lut'], warp_masks=wm)
            today = pre.train_item_photo(x['f'], x['a'], masks, x['cd'], pd, dd, x['ids'], **kw)
            with monkeypatch.context() as mp:
                mp.setattr(DevicePreprocessor, 'train_item_photo', recorded)
                got = pre.train_item_motion(x['f'], x['a'], masks, x['cd'], md, pd, dd, x['ids'], **kw)
            assert len(calls) == 1 and calls.pop()[0][4:6] == (pd, dd)                               # a call of it
            assert list(got) == list(today) and all(torch.equal(got[k], today[k]) for k in today)
