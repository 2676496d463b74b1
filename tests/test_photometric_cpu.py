"""Host side of the device photometric steps (maggie_amd.utils.photometric): the integer restatement against the fixture Pillow wrote and
against Pillow itself, the quantisation tables against the ones Pillow reports, the kernel's division scheme over the whole range it can meet,
the LDS layout's bank conflicts, the argument errors, the wiring's pass-through. No GPU needed."""
import ctypes
import inspect
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import photometric_restatement as P                                   # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd.hip import MaggieHipError                             # noqa: E402
from maggie_amd.utils import photometric                              # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor            # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_photometric_golden as G                                   # noqa: E402

SHAPES, QUALITIES, KINDS, seed_of = P.SHAPES, P.QUALITIES, P.KINDS, P.seed_of


@pytest.mark.parametrize('name', list(G.CASES))
def test_fixture_equals_the_restatement(name):
    d = load_golden('photometric_pinned.npz')
    h, w, kind, seed, q = G.CASES[name]
    x = P.inputs(h, w, kind, seed)
    assert d[name + '.info'].tolist() == [h, w, q] and np.array_equal(d[name + '.input'], x)
    assert np.array_equal(P.jpeg_roundtrip(x, q), d[name + '.output'])
    assert 'Pillow' in str(d['versions']) and 'jpg' in str(d['versions'])


def test_fixture_is_small_and_lossy():
    d = load_golden('photometric_pinned.npz')
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'photometric_pinned.npz')) < 100 * 1024
    assert max(d[n + '.input'].shape[0] for n in G.CASES) <= 48 and max(d[n + '.input'].shape[1] for n in G.CASES) <= 64
    assert any(not np.array_equal(d[n + '.input'], d[n + '.output']) for n in G.CASES)


@pytest.mark.parametrize('h,w', SHAPES)
def test_restatement_equals_live_pillow(h, w):
    pytest.importorskip('PIL')
    for q in QUALITIES:
        for kind in KINDS:
            x = P.inputs(h, w, kind, seed_of(h, w, q, kind))
            assert np.array_equal(P.jpeg_roundtrip(x, q), G.pil_roundtrip(x, q)), (q, kind)


@pytest.mark.parametrize('q', [1, 20, 21, 49, 50, 51, 80, 81, 100])
def test_quant_tables_equal_the_ones_pillow_reports(q):
    Image = pytest.importorskip('PIL.Image')
    buf = io.BytesIO()
    Image.fromarray(P.inputs(8, 8, 'random', 0)).save(buf, format='JPEG', quality=q)
    buf.seek(0)
    reported = Image.open(buf).quantization
    t = photometric.quant_tables(q)
    assert t.dtype == np.int32 and t.shape == (2, 64) and t.min() >= 1 and t.max() <= 255
    assert sorted(reported) == [0, 1] and np.array_equal(np.asarray(reported[0]), t[0]) and np.array_equal(np.asarray(reported[1]), t[1])
    assert np.array_equal(P.quant_tables(q), t)


def test_quant_table_ends():
    assert np.array_equal(photometric.quant_tables(100), np.ones((2, 64), np.int32))                     # s = 0: everything clips to 1
    assert photometric.quant_tables(1).max() == 255 and photometric.quant_tables(50)[0, 0] == 16
    for bad in (0, 101, -3):
        with pytest.raises(ValueError):
            photometric.quant_tables(bad)
    for bad in (50.0, '50', None, True):
        with pytest.raises(TypeError):
            photometric.quant_tables(bad)


# ---- the division of the quantiser ---------------------------------------------------------------------------------------------------------------
def coefficient_bound():
    """An upper bound of |c| over every coefficient jpeg_fdct_islow can produce from samples in -128..127. Without its roundings a pass is
    linear; its matrix, read off the fixed-point constants by running the restated pass on the unit vectors in exact (float64, all values
    are small dyadic rationals) arithmetic, has rows of L1 norm g. A descale adds at most 1/2. So after the rows |r| <= g1 * 128 + 1/2 and
    after the columns |c| <= g2 * (g1 * 128 + 1/2) + 1/2."""
    saved = P.descale
    P.descale = lambda x, n: x / float(1 << n)
    try:
        eye = np.eye(8, dtype=np.float64)
        g1 = np.abs(P.fdct_1d(eye, True)).sum(0).max()                   # out[k] = sum_i x[i] * M[i][k]: column k of the stacked outputs
        g2 = np.abs(P.fdct_1d(eye, False)).sum(0).max()
    finally:
        P.descale = saved
    return int(np.ceil(g2 * (g1 * 128 + 0.5) + 0.5))


def test_coefficient_bound():
    bound = coefficient_bound()
    assert 8 * 1024 <= bound <= 8 * 1024 + 16                             # the DC term of a block of -128 is exactly -8192
    # the extremes: every coefficient's own worst block (the sign pattern of its basis function) stays inside, and the DC term reaches 8192
    yy, xx = np.mgrid[0:8, 0:8]
    worst = 0
    for u in range(8):
        for v in range(8):
            basis = np.cos((2 * yy + 1) * u * np.pi / 16) * np.cos((2 * xx + 1) * v * np.pi / 16)
            for sign in (1, -1):
                block = np.where(sign * basis >= 0, 127, -128).astype(np.int64)
                worst = max(worst, int(np.abs(P.fdct(block)).max()))
    assert 8192 - 64 <= worst <= bound
    assert int(np.abs(P.fdct(np.full((8, 8), -128, np.int64))).max()) == 8192


def test_division_scheme_is_exact_over_the_whole_range():
    """The kernel's n / qv: m = floor((2^32 - 1) / qv) + 1, (n * m) >> 32 -- against `//` for every divisor 8..2040 (qv = 8 t takes the
    multiples of 8 among them) and every numerator |c| + qv / 2 the forward transform can produce."""
    bound = coefficient_bound()
    n_max = bound + 2040 // 2
    assert n_max * 2040 < 1 << 32                                          # the condition of the proof: n * (m * qv - 2^32) < 2^32
    n = np.arange(n_max + 1, dtype=np.uint64)
    for d0 in range(8, 2041, 64):
        d = np.arange(d0, min(d0 + 64, 2041), dtype=np.uint64)[:, None]
        m = np.uint64(0xFFFFFFFF) // d + np.uint64(1)
        assert int(m.max()) < 1 << 32                                      # the multiplier fits the unsigned word the kernel keeps it in
        assert np.array_equal((n[None, :] * m) >> np.uint64(32), n[None, :] // d), d0


def test_quantiser_restated_with_the_kernels_division():
    """sign(c) * ((|c| + qv / 2) / qv) * t through the multiplier, on the coefficients of real blocks, equals the restatement's quantiser."""
    rng = np.random.RandomState(5)
    c = P.fdct(rng.randint(-128, 128, (200, 8, 8)).astype(np.int64))
    for q in (1, 35, 50, 90, 100):
        t = P.quant_tables(q)[0].reshape(8, 8)
        m = 0xFFFFFFFF // (8 * t) + 1
        k = ((np.abs(c) + 4 * t) * m) >> 32
        assert np.array_equal(np.where(c < 0, -k, k) * t, P.quantise(c, t))


# ---- the LDS layout --------------------------------------------------------------------------------------------------------------------------------
def conflicts(row_pitch, block_pitch, by_column):
    """The worst number of lanes of a 32-lane half that meet in one of the 32 banks, over the eight ds_read_b32 / ds_write_b32 of a pass:
    lane = 8 * block + line reads element k of its row (line * row_pitch + k) or of its column (k * row_pitch + line)."""
    worst = 0
    for half in range(photometric.THREADS // 32):
        lanes = np.arange(32) + 32 * half
        b, l = lanes >> 3, lanes & 7
        for k in range(8):
            addr = b * block_pitch + (k * row_pitch + l if by_column else l * row_pitch + k)
            worst = max(worst, int(np.bincount(addr % 32, minlength=32).max()))
    return worst


def test_lds_layout_is_conflict_free_in_both_passes():
    rp, bp = photometric.ROW_PITCH, photometric.BLOCK_PITCH
    assert (rp, bp) == (9, 72)
    assert conflicts(rp, bp, False) == 1 and conflicts(rp, bp, True) == 1
    assert conflicts(8, 64, True) == 4 and conflicts(8, 64, False) == 8    # the packed block: what the pitches avoid
    assert conflicts(8, 72, True) == 1 and conflicts(8, 72, False) == 8    # the block pitch alone frees the columns only: banks 8 (b + r) + k
    src = open(os.path.join(os.path.dirname(photometric.__file__), os.pardir, 'csrc', 'photometric.hip')).read()
    assert 'constexpr int RP = %d, BP = 8 * RP;' % rp in src


# ---- the small host functions -------------------------------------------------------------------------------------------------------------------
def test_quality_from_compression():
    f = photometric.quality_from_compression
    assert (f(20), f(50), f(80)) == (80, 50, 21)                            # round(80.2), round(50.5) to even, round(20.8)
    assert f(0) == 100 and f(100) == 1 and f(-5) == 100 and f(140) == 1     # the clip ends
    assert all(f(c) == P.quality_from_compression(c) for c in np.linspace(-10, 110, 481))
    assert 'imgaug' in f.__doc__ and 'not' in f.__doc__


def test_draws_record():
    d = photometric.PhotoDraws()
    assert (d.lut, d.noise, d.quality, d.qtable) == (None, None, None, None) and not d.fired
    lut = np.tile(np.arange(256, dtype=np.uint8)[::-1], (3, 1))
    noise = np.zeros((4, 6, 1), np.int16)
    d = photometric.PhotoDraws(lut, noise, 35)
    assert d.fired and d.quality == 35 and np.array_equal(d.qtable, photometric.quant_tables(35)) and not d.on_device
    assert photometric.PhotoDraws(lut=lut).fired is False and photometric.PhotoDraws(quality=1).fired and photometric.PhotoDraws(noise=noise).fired
    for bad in (dict(lut=lut[:2]), dict(lut=lut.astype(np.int32)), dict(noise=noise.astype(np.int32)), dict(noise=noise[..., 0]),
                dict(noise=np.zeros((4, 6, 2), np.int16)), dict(quality=0), dict(quality=101)):
        with pytest.raises(ValueError):
            photometric.PhotoDraws(**bad)
    with pytest.raises(TypeError):
        photometric.PhotoDraws(quality=50.5)


def test_argument_errors_come_before_any_launch():
    f = np.zeros((2, 8, 12, 3), np.uint8)
    noise = np.zeros((8, 12, 3), np.int16)
    with pytest.raises(TypeError):
        photometric.apply(f, None)
    with pytest.raises(TypeError):
        photometric.apply(f.astype(np.float32), photometric.PhotoDraws(quality=50))
    with pytest.raises(TypeError):
        photometric.jpeg_roundtrip(f, 50.0)
    for q in (0, 101):
        with pytest.raises(ValueError):
            photometric.jpeg_roundtrip(f, q)
    with pytest.raises(ValueError):
        photometric.jpeg_roundtrip(f[..., :2], 50)
    with pytest.raises(ValueError):
        photometric.jpeg_roundtrip(f, 50, noise=noise[:7])                  # drawn for another size
    with pytest.raises(ValueError):
        photometric.jpeg_roundtrip(f, 50, noise=noise.astype(np.float32))
    with pytest.raises(ValueError):
        photometric.jpeg_roundtrip(f, 50, lut=np.zeros((3, 255), np.uint8))
    with pytest.raises(ValueError):
        photometric.jpeg_roundtrip(f, np.ones((2, 63), np.int32))
    with pytest.raises(ValueError):
        photometric.add_noise(f, None)
    with pytest.raises(ValueError):
        photometric.add_noise(f, noise[:, :11])
    with pytest.raises(ValueError):
        photometric.apply(f, photometric.PhotoDraws(noise=noise[:, :5]))


def test_no_gpu_raises_maggie_hip_error():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    f = np.zeros((1, 8, 12, 3), np.uint8)
    with pytest.raises(MaggieHipError):
        photometric.jpeg_roundtrip(f, 50)
    with pytest.raises(MaggieHipError):
        photometric.add_noise(f, np.zeros((8, 12, 1), np.int16))
    with pytest.raises(MaggieHipError):
        photometric.apply(f, photometric.PhotoDraws(quality=50))
    with pytest.raises(MaggieHipError):
        photometric.PhotoDraws(quality=50).to()


def test_c_entries_reject_bad_arguments_before_any_launch():
    from maggie_amd import hip
    I, L = ctypes.c_int, ctypes.c_long
    lib = hip.lib()
    for fn in (lib.mg_jpeg_ycc, lib.mg_jpeg_rgb, lib.mg_photo_noise, lib.mg_jpeg_limits):
        fn.restype = ctypes.c_int
    three = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    fake, other, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(4100)      # non-null: never read, the checks come first

    def ycc(n=1, h=4, w=4, src=None, planes=None, noise=None, nc=1, qtab=None):
        return lib.mg_jpeg_ycc(src, planes, None, noise, I(nc), qtab, L(n), I(h), I(w), None)

    def rgb(n=1, h=4, w=4, planes=None, dst=None, epilogue=0, mean=three):
        return lib.mg_jpeg_rgb(planes, dst, L(n), I(h), I(w), I(epilogue), mean, mean, None)

    def point(n=1, h=4, w=4, src=None, dst=None, noise=None, nc=1, epilogue=0, mean=three):
        return lib.mg_photo_noise(src, dst, None, noise, I(nc), L(n), I(h), I(w), I(epilogue), mean, mean, None)
    assert ycc() == rgb() == point() == -2                                   # null pointers
    assert ycc(n=0) == rgb(n=0) == point(n=0) == 0
    for bad in (dict(n=-1), dict(h=0), dict(w=-1), dict(h=photometric.MAX_SIDE + 1), dict(w=photometric.MAX_SIDE + 1)):
        assert ycc(src=fake, planes=other, qtab=fake, **bad) == -2, bad
        assert rgb(planes=fake, dst=other, **bad) == -2, bad
        assert point(src=fake, dst=other, **bad) == -2, bad
    assert ycc(src=fake, planes=other) == -2                                 # no table
    assert ycc(src=fake, planes=fake, qtab=fake) == -2 and rgb(planes=fake, dst=fake) == -2 and point(src=fake, dst=fake) == -2       # in place
    assert ycc(src=fake, planes=odd, qtab=fake) == -2 and rgb(planes=odd, dst=other) == -2                  # the planes are read 16 bytes at a time
    for nc in (0, 2, 4):
        assert ycc(src=fake, planes=other, qtab=fake, noise=fake, nc=nc) == -2 and point(src=fake, dst=other, noise=fake, nc=nc) == -2
    for e in (-1, 2):
        assert rgb(planes=fake, dst=other, epilogue=e) == -2 and point(src=fake, dst=other, epilogue=e) == -2
    assert rgb(planes=fake, dst=other, mean=None) == -2 and point(src=fake, dst=other, mean=None) == -2


def test_python_constants_match_the_library():
    from maggie_amd import hip
    a, b, c, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert hip.lib().mg_jpeg_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)) == 0
    assert (a.value, b.value, c.value, d.value) == (photometric.TILE_ROWS, photometric.TILE_COLS, photometric.THREADS, photometric.MAX_SIDE)
    assert hip.lib().mg_jpeg_limits(None, None, None, None) == -2
    header = open(os.path.join(os.path.dirname(photometric.__file__), os.pardir, os.pardir, 'include', 'maggie_hip.h')).read()
    assert '#define MG_PHOTO_RAW %d\n' % photometric.RAW in header and '#define MG_PHOTO_NORM %d\n' % photometric.NORM in header
    assert np.array_equal(np.asarray(photometric.STD_LUMA), P.STD_LUMA) and np.array_equal(np.asarray(photometric.STD_CHROMA), P.STD_CHROMA)
    assert photometric.plane_bytes(3, 17, 23) == 3 * 32 * 32 * 3 // 2


# ---- the wiring ----------------------------------------------------------------------------------------------------------------------------------
def test_nothing_set_is_literally_the_old_path(monkeypatch):
    """`train_item_photo` with no photo, or with draws that hold neither noise nor quality, IS a call of `train_item_affine` with the same
    arguments; a lone `photo.lut` goes to the crop's `lut`."""
    pre = DevicePreprocessor(max_inst=4)
    seen = []

    def recorder(*args, **kwargs):
        seen.append((args, kwargs))
        return 'old path'
    monkeypatch.setattr(pre, 'train_item_affine', recorder)
    f, a, m, cd, ad, curve = object(), object(), object(), object(), None, np.zeros((3, 256), np.uint8)
    for photo, lut, want in ((None, None, None), (photometric.PhotoDraws(), curve, curve), (photometric.PhotoDraws(lut=curve), None, curve)):
        del seen[:]
        out = pre.train_item_photo(f, a, m, cd, photo, ad, [1, 0], transition=(3, 2), mask_draws='md', lut=lut, warp_masks=True)
        assert out == 'old path' and len(seen) == 1
        args, kwargs = seen[0]
        assert args[:5] == (f, a, m, cd, ad) and args[5] == [1, 0]
        assert kwargs == dict(transition=(3, 2), mask_draws='md', lut=want, warp_masks=True) and kwargs['lut'] is want
    with pytest.raises(TypeError):
        pre.train_item_photo(f, a, m, cd, 'draws')
    with pytest.raises(TypeError):
        pre.train_item_photo(f, a, m, cd, None, 'affine')


def test_signatures():
    """`train_item` and `train_item_affine` keep the signatures the crop and affine suites pin; the photometric wiring is a method of its own."""
    assert str(inspect.signature(DevicePreprocessor.train_item_photo)) == \
        '(self, frames_u8, alphas_u8, masks_u8, crop_draws, photo, affine_draws=None, slot_ids=None, *, transition=None, mask_draws=None, ' \
        'lut=None, warp_masks=False)'
    assert str(inspect.signature(photometric.jpeg_roundtrip)).startswith('(frames_u8, quality, *, lut=None, noise=None, normalize=False, mean=')
    assert str(inspect.signature(photometric.PhotoDraws.__init__)).startswith('(self, lut=None, noise=None, quality=None')
