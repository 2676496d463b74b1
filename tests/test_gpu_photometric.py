"""The photometric steps on the device (csrc/photometric.hip, maggie_amd.utils.photometric, DevicePreprocessor.train_item_photo): the JPEG
round trip's two launches, the tone curve and the noise on its load, the saturating add alone, both epilogues, against the integer NumPy
restatement (tests/photometric_restatement.py, which tests/test_photometric_cpu.py holds against Pillow on these very cases) and the fixture
Pillow wrote (tests/golden/photometric_pinned.npz). Integer work and IEEE divisions: every comparison is exact."""
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
import photometric_restatement as P                                   # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.hip import c_int, c_long                              # noqa: E402
from maggie_amd.utils import affine, crop, photometric                # noqa: E402
from maggie_amd.utils import maskgen as MG                            # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor, normalize_frames       # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_photometric_golden as G                                   # noqa: E402

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
    """The same tensor at a base one byte past an allocation: 16-byte (or 4-byte) aligned only by chance."""
    flat = torch.cat([torch.zeros(1, dtype=t.dtype, device=t.device), t.reshape(-1)])[1:]
    assert flat.data_ptr() % 4 != 0
    return flat.view(t.shape)


def _case(h, w, q):
    """The three inputs of a shape at a quality and their restated round trips, computed once and left unchanged."""
    if (h, w, q) not in _REF:
        x = np.stack([P.inputs(h, w, kind, P.seed_of(h, w, q, kind)) for kind in P.KINDS])
        _REF[(h, w, q)] = (x, np.stack([P.jpeg_roundtrip(f, q) for f in x]))
    return _REF[(h, w, q)]


def _same_as_normalize_frames(norm, raw_u8, dev):
    """The Normalize epilogue against `normalize_frames` of the raw result, where that function is defined (it takes h * w % 4 == 0 only);
    the callers compare with the restated arithmetic at every size."""
    h, w = raw_u8.shape[-3:-1]
    return (h * w) % 4 != 0 or torch.equal(norm, normalize_frames(raw_u8, MEAN, STD, dev))


def _lut(seed):
    return np.random.default_rng(seed).integers(0, 256, (3, 256), dtype=np.uint8)


def _noise(seed, h, w, nc, extreme=False):
    r = np.random.default_rng(seed)
    n = r.integers(-40, 41, (h, w, nc)).astype(np.int16)
    if extreme:                                                            # +-255 drive both ends of the saturating add
        n[r.random((h, w, nc)) < 0.3] = 255
        n[r.random((h, w, nc)) < 0.3] = -255
        n.flat[0], n.flat[-1] = 255, -255                                  # both ends at every size
    return n


# ---- the round trip --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', P.SHAPES)
def test_round_trip_equals_the_restatement(h, w):
    """Every quality on the three inputs: as one clip of T = 3 and frame by frame (T = 1), from aligned and one-byte-unaligned bases, raw and
    with the Normalize epilogue, which has the bits of `normalize_frames` on the raw result."""
    dev = _dev()
    for k, q in enumerate(P.QUALITIES):
        x, want = _case(h, w, q)
        f = _T(x, dev)
        got = photometric.jpeg_roundtrip(_unaligned(f) if k % 2 else f, q)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3, h, w, 3) and _eq(got, want), q
        norm = photometric.jpeg_roundtrip(f if k % 2 else _unaligned(f), q, normalize=True)
        assert norm.dtype == torch.float32 and tuple(norm.shape) == (3, 3, h, w)
        assert _same_as_normalize_frames(norm, got, dev) and _eq(norm, P.normalize(want, MEAN, STD)), q
        one = photometric.jpeg_roundtrip(f[k % 3:k % 3 + 1], torch.from_numpy(photometric.quant_tables(q)).to(dev))      # T = 1, a device table
        assert _eq(one, want[k % 3:k % 3 + 1]), q
        assert _eq(photometric.jpeg_roundtrip(x[(k + 1) % 3], q, normalize=bool(k % 2), mean=(0.5, 0.25, 0.125), std=(0.3, 0.2, 0.1)),
                   P.normalize(want[(k + 1) % 3][None], (0.5, 0.25, 0.125), (0.3, 0.2, 0.1))[0] if k % 2 else want[(k + 1) % 3]), q


@pytest.mark.parametrize('offset', [0, 1, 4])
def test_round_trip_into_unaligned_outputs(offset):
    """The C entries with output bases that are no multiple of 16 on widths that are: the per-element stores give the bytes of the packed
    ones, and nothing is written outside the output."""
    dev = _dev()
    three = (hip.ctypes.c_float * 3)
    for (h, w), q in (((16, 16), 50), ((32, 64), 21), ((64, 48), 80)):
        x, want = _case(h, w, q)
        f = _T(x, dev)
        qt = _T(photometric.quant_tables(q), dev)
        planes = torch.empty((photometric.plane_bytes(3, h, w),), dtype=torch.uint8, device=dev)
        hip.call('mg_jpeg_ycc', hip.ptr(f), hip.ptr(planes), None, None, c_int(1), hip.ptr(qt), c_long(3), c_int(h), c_int(w), hip.stream())
        want_planes = [np.stack(p) for p in zip(*[P.jpeg_planes(fr, q) for fr in x])]
        at = 0
        for p in want_planes:                                               # Y, then Cb, then Cr, each for all frames
            assert _eq(planes[at:at + p.size], p.astype(np.uint8).reshape(-1))
            at += p.size
        assert at == planes.numel()
        n = 3 * h * w * 3
        raw = torch.full((n + 32,), 7, dtype=torch.uint8, device=dev)
        hip.call('mg_jpeg_rgb', hip.ptr(planes), hip.ctypes.c_void_p(raw.data_ptr() + 16 + offset), c_long(3), c_int(h), c_int(w),
                 c_int(photometric.RAW), three(*MEAN), three(*STD), hip.stream())
        assert _eq(raw[16 + offset:16 + offset + n], want.reshape(-1))
        assert int(raw[:16 + offset].min()) == 7 == int(raw[:16 + offset].max()) and int(raw[16 + offset + n:].min()) == 7 == int(raw[16 + offset + n:].max())
        if offset % 4 == 0:                                                 # floats stay 4-byte aligned
            fl = torch.full((n + 8,), 7.0, dtype=torch.float32, device=dev)
            hip.call('mg_jpeg_rgb', hip.ptr(planes), hip.ctypes.c_void_p(fl.data_ptr() + 16 + offset), c_long(3), c_int(h), c_int(w),
                     c_int(photometric.NORM), three(*MEAN), three(*STD), hip.stream())
            lo = (16 + offset) // 4
            assert _eq(fl[lo:lo + n], P.normalize(want, MEAN, STD).reshape(-1))
            assert float(fl[:lo].min()) == 7.0 == float(fl[:lo].max()) and float(fl[lo + n:].min()) == 7.0 == float(fl[lo + n:].max())


@pytest.mark.parametrize('name', list(G.CASES))
def test_round_trip_equals_the_fixture(name):
    """What Pillow itself wrote, key by key."""
    dev = _dev()
    d = load_golden('photometric_pinned.npz')
    h, w, q = d[name + '.info'].tolist()
    x, y = d[name + '.input'], d[name + '.output']
    assert _eq(photometric.jpeg_roundtrip(x[None], q)[0], y)
    assert _eq(photometric.apply(_T(x[None], dev), photometric.PhotoDraws(quality=q).to(dev), normalize=True), P.normalize(y[None], MEAN, STD))


# ---- the tone curve and the noise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(2, 2), (21, 5), (16, 16), (37, 53), (32, 64), (33, 65)])
def test_curve_and_noise_on_every_path(h, w):
    """With and without `lut`, (h, w, 1) and (h, w, 3) noise including +-255, alone and in front of the round trip, raw and normalised,
    host and device draws."""
    dev = _dev()
    q = 50
    x, _ = _case(h, w, q)
    f = _T(x, dev)
    lut = _lut(h * w)
    k = 0
    for use_lut in (False, True):
        for nc, extreme in ((None, False), (1, False), (3, False), (1, True), (3, True)):
            k += 1
            noise = None if nc is None else _noise(7 * k + h, h, w, nc, extreme)
            curve = lut if use_lut else None
            src = _unaligned(f) if k % 2 else f
            want = P.photometric(x, curve, noise, q)
            got = photometric.jpeg_roundtrip(src, q, lut=curve, noise=noise)
            assert _eq(got, want), (use_lut, nc, extreme)
            d = photometric.PhotoDraws(curve, noise, q)
            for dd in (d, d.to(dev)):
                assert torch.equal(photometric.apply(src, dd), got)
                norm = photometric.apply(src, dd, normalize=True)
                assert _same_as_normalize_frames(norm, got, dev) and _eq(norm, P.normalize(want, MEAN, STD))
            # without the round trip: one pointwise launch, or none at all
            point = P.photometric(x, curve, noise, None)
            d = photometric.PhotoDraws(curve, noise).to(dev)
            got = photometric.apply(src, d)
            assert got.dtype == torch.uint8 and _eq(got, point), (use_lut, nc, extreme)
            assert _eq(photometric.apply(src, d, normalize=True), P.normalize(point, MEAN, STD))
            if noise is not None:
                assert _eq(photometric.add_noise(src, noise), P.add_noise(x, noise))
                assert _eq(photometric.add_noise(x[1], _T(noise, dev)), P.add_noise(x[1], noise))
                if extreme:
                    added = P.add_noise(x, noise)
                    assert added.min() == 0 and added.max() == 255 and not np.array_equal(added, x)
    # nothing set: the frames themselves, or normalize_frames of them
    empty = photometric.PhotoDraws()
    assert torch.equal(photometric.apply(f, empty), f)
    norm = photometric.apply(f, empty, normalize=True)
    assert _same_as_normalize_frames(norm, f, dev) and _eq(norm, P.normalize(x, MEAN, STD))


def test_a_table_outside_its_range_is_clamped():
    """A quantisation table rewritten on the device may hold anything: entries are taken as clip(t, 1, 255)."""
    dev = _dev()
    x, _ = _case(17, 23, 50)
    wild = np.random.default_rng(3).integers(-300, 600, (2, 64)).astype(np.int32)
    wild[0, 0], wild[1, 5] = 0, -2 ** 31
    want = np.stack([P.jpeg_roundtrip(f, np.clip(wild, 1, 255)) for f in x])
    assert _eq(photometric.jpeg_roundtrip(x, wild), want)


# ---- the training item ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['first_hit', 'pad_wide_odd'])
def test_train_item_photo_fired_and_not_with_and_without_affine(name):
    """Crop -> curve -> noise -> JPEG -> (RandomAffine) -> item, against the composition of the three restatements; the planes never see the
    photometric steps; without draws, or with draws that hold neither noise nor quality, today's items bit for bit."""
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
    unfired = affine.draw(np.random.RandomState(5), oh, ow, p=0.1)
    assert ad.fired and ad.matrix is not None and not unfired.fired
    md = MG.draw_chain(np.random.RandomState(9), random.Random(9), T * n, oh, ow, from_alpha=T > 1)
    f, a, m = _T(frames, dev), _T(alphas.reshape(T, n, c['h'], c['w']), dev), _T(masks.reshape(T, n, c['h'], c['w']), dev)
    crop_lut, photo_lut, noise, q = _lut(1), _lut(2), _noise(3, oh, ow, 1, True), 35
    toned = P.apply_lut(r['frames'], crop_lut)
    want_u8 = P.photometric(toned, photo_lut, noise, q)                     # the crop's curve, then the draws' own, the noise, the round trip
    assert not np.array_equal(want_u8, toned)
    lin = A.tables(np.asarray(ad.matrix, np.float64), oh, ow, A.INTER_LINEAR)
    warped = A.shift_normalized(np.stack([A.warp_linear(fr, lin) for fr in want_u8]), ad.intensity)
    photo = photometric.PhotoDraws(photo_lut, noise, q)
    for pd in (photo, photo.to(dev)):
        # no affine: the Normalize epilogue of the round trip writes the image
        for dd in (None, unfired):
            got = pre.train_item_photo(f, a, a, cd, pd, dd, ids, transition=(3, 2), mask_draws=md, lut=crop_lut)
            plain = pre.train_item(f, a, a, cd, ids, transition=(3, 2), mask_draws=md, lut=crop_lut)
            assert list(got) == list(plain) == ['image', 'alpha', 'mask', 'transition']
            assert got['image'].dtype == torch.float32 and _eq(got['image'], P.normalize(want_u8, MEAN, STD))
            assert all(torch.equal(got[key], plain[key]) for key in ('alpha', 'mask', 'transition'))
        # a fired affine reads the raw uint8 result
        for wm in (False, True):
            got = pre.train_item_photo(f, a, m if not wm else a, cd, pd, ad, ids, transition=(3, 2), lut=crop_lut, warp_masks=wm)
            plain = pre.train_item_affine(f, a, m if not wm else a, cd, ad, ids, transition=(3, 2), lut=crop_lut, warp_masks=wm)
            assert _eq(got['image'], warped) and not torch.equal(got['image'], plain['image'])
            assert all(torch.equal(got[key], plain[key]) for key in ('alpha', 'mask', 'transition'))
    # the steps one at a time
    for pd, want in ((photometric.PhotoDraws(noise=noise), P.photometric(toned, None, noise, None)),
                     (photometric.PhotoDraws(quality=q), P.photometric(toned, None, None, q))):
        assert _eq(pre.train_item_photo(f, a, m, cd, pd, None, ids, lut=crop_lut)['image'], P.normalize(want, MEAN, STD))
    # nothing that needs the raw crop: today's items, through today's methods; a lone curve joins the crop's table
    for dd in (None, unfired, ad):
        today = pre.train_item_affine(f, a, a, cd, dd, ids, transition=(3, 2), mask_draws=md, lut=crop_lut)
        for pd in (None, photometric.PhotoDraws()):
            got = pre.train_item_photo(f, a, a, cd, pd, dd, ids, transition=(3, 2), mask_draws=md, lut=crop_lut)
            assert list(got) == list(today) and all(torch.equal(got[k], today[k]) for k in today)
    both = np.stack([photo_lut[ch][crop_lut[ch]] for ch in range(3)])
    for pd in (photometric.PhotoDraws(lut=photo_lut), photometric.PhotoDraws(lut=photo_lut).to(dev)):
        got = pre.train_item_photo(f, a, a, cd, pd, None, ids, lut=crop_lut)
        assert torch.equal(got['image'], pre.train_item(f, a, a, cd, ids, lut=both)['image'])
        assert _eq(got['image'], P.normalize(P.apply_lut(toned, photo_lut), MEAN, STD))
        assert torch.equal(pre.train_item_photo(f, a, a, cd, pd, None, ids)['image'], pre.train_item(f, a, a, cd, ids, lut=photo_lut)['image'])


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_apply_replays_with_new_pixels_and_rewritten_tables():
    dev = _dev()
    h, w = 37, 53
    x, _ = _case(h, w, 50)
    other, _ = _case(h, w, 21)
    faulthandler.dump_traceback_later(120, exit=True)                      # the test's own time limit: a hung capture or replay ends the process
    try:
        sf = _T(x, dev)
        d = photometric.PhotoDraws(_lut(4), _noise(5, h, w, 3), 50).to(dev)
        assert d.on_device and d.qtable.dtype == torch.int32
        photometric.apply(sf, d, normalize=True)                            # warm-up off the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            image = photometric.apply(sf, d, normalize=True)
        for fr, lut, noise, q in ((other, _lut(6), _noise(7, h, w, 3, True), 1), (x, _lut(4), _noise(5, h, w, 3), 50), (other, _lut(8), _noise(9, h, w, 3), 95)):
            sf.copy_(_T(fr, dev))
            d.lut.copy_(_T(lut, dev))
            d.noise.copy_(_T(noise, dev))
            d.qtable.copy_(_T(photometric.quant_tables(q), dev))
            g.replay()
            torch.cuda.synchronize()
            assert _eq(image, P.normalize(P.photometric(fr, lut, noise, q), MEAN, STD)), q
        del g
    finally:
        faulthandler.cancel_dump_traceback_later()
