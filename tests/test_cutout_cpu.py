"""Cut-outs without a GPU: the statement of DESIGN.md section 35 (tests/cutout_restatement.py) held against SciPy's uniform filter, against the two
things an estimator must do (return the image where the matte is opaque; come closer to the true foreground than the image does where it is
not), its colour PNG files read back by Pillow, the host half of `maggie_amd.utils.cutout` and `pngenc.encode_images` (argument checks before
any device is touched, the framing), and the colour entries of csrc/pngenc.hip compiled for the host under the address and undefined-behaviour
sanitizers (tests/csrc/pngenc_colour_host.cpp), byte-equal to the restatement."""
import io
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cutout_restatement as C                              # noqa: E402
import pngenc_restatement as R                              # noqa: E402
from maggie_amd.utils import cutout, pngenc                 # noqa: E402

RADII = (1, 2, 3, 6, 9, 90, 255)


def test_constants_are_the_header_s():
    text = open(os.path.join(ROOT, 'include', 'maggie_hip.h')).read()
    for name, v in (('MAX_RADIUS', cutout.MAX_RADIUS), ('MAX_SIDE', cutout.MAX_SIDE)):
        assert '#define MG_CUTOUT_%s %d' % (name, v) in text, name
    assert cutout.RADII == C.RADII == (90, 6)


@pytest.mark.parametrize('shape', [(13, 17), (1, 1)])
def test_window_sums_are_scipy_s_mirror_filter(shape):
    rng = np.random.RandomState(3)
    p = rng.randint(0, 65026, shape)
    for r in RADII:
        got = C.window_sums(p, r)
        want = ndimage.uniform_filter(p.astype(np.float64), size=r, mode='mirror') * (r * r)
        assert got.dtype == np.int64 and got.shape == shape
        assert np.allclose(got, want, rtol=1e-6, atol=0), (shape, r)


def test_reflection_repeats_as_often_as_needed():
    assert C.reflect(np.arange(-7, 9), 3).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]
    assert C.reflect(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert C.reflect(np.arange(-2, 4), 2).tolist() == [0, 1, 0, 1, 0, 1]


def test_an_opaque_matte_returns_the_image():
    rng = np.random.RandomState(5)
    I = rng.randint(0, 256, (23, 31, 3)).astype(np.uint8)
    a = np.full((23, 31), 255, np.uint8)
    a[5:12, 4:20] = rng.randint(0, 255, (7, 16))
    for radii in (C.RADII, (2, 7), (1, 1)):
        F = C.estimate(I, a, radii)
        assert np.array_equal(F[a == 255], I[a == 255]), radii
    full = np.full((23, 31), 255, np.uint8)
    assert np.array_equal(C.estimate(I, full), I)
    assert np.array_equal(C.cutout(I, full)[..., :3], I) and (C.cutout(I, full)[..., 3] == 255).all()
    assert not C.cutout(I, np.zeros((23, 31), np.uint8)).any()


def test_the_estimate_halves_the_error_of_the_raw_image():
    I, F, B, a = C.scene(240, 320)
    est = C.estimate(I, a)
    mixed = (a > 12) & (a < 243)
    assert mixed.sum() > 2000
    err_est = np.abs(est[mixed].astype(np.float64) - F[mixed]).mean()
    err_raw = np.abs(I[mixed].astype(np.float64) - F[mixed]).mean()
    print('mean absolute error against the true foreground over %d mixed pixels: estimate %.2f, raw image %.2f' % (mixed.sum(), err_est, err_raw))
    assert err_est < 0.5 * err_raw


def test_float_alpha_is_the_unit_byte():
    x = np.array([[np.nan, -0.5, 1.5, 0.5, 1.0, 0.999, 0.0]], np.float32)
    assert C.alpha_byte(x).tolist() == [[0, 0, 255, 127, 255, 254, 0]]
    u = np.array([[3, 250]], np.uint8)
    assert C.alpha_byte(u) is u


@pytest.mark.parametrize('channels', [3, 4])
def test_restated_colour_files_decode_to_the_input(channels):
    rng = np.random.RandomState(channels)
    images = [rng.randint(0, 256, (1, 1, channels)), rng.randint(0, 256, (1, 3, channels)), rng.randint(0, 256, (7, 5, channels)),
              C.disc_image(67, 257, channels), np.full((9, 40, channels), 77), rng.randint(0, 256, (5, 4096, channels))]
    for im in images:
        im = im.astype(np.uint8)
        f, blocks = C.encode_colour(im)
        back = Image.open(io.BytesIO(f))
        assert back.mode == ('RGB' if channels == 3 else 'RGBA')
        assert np.array_equal(np.asarray(back), im), im.shape
        assert zlib.decompress(R.idat(f)) == C.filtered_colour(im).tobytes()
        assert pngenc.frame(im.shape[0], im.shape[1], R.idat(f), channels) == f
        assert len(blocks) == pngenc.blocks_of(im.shape[0], channels * im.shape[1])


def test_grey_framing_is_unchanged():
    p = R.cases()['mixed_130x67']
    f, _ = R.encode(p)
    assert pngenc.frame(130, 67, R.idat(f)) == f == pngenc.frame(130, 67, R.idat(f), 1)


def test_argument_checks_come_before_the_device():
    fr = np.zeros((4, 5, 3), np.uint8)
    a8 = torch.zeros((2, 4, 5), dtype=torch.uint8)
    with pytest.raises(TypeError):
        cutout.estimate_foreground(fr.astype(np.float32), a8)
    with pytest.raises(TypeError):
        cutout.estimate_foreground(fr, np.zeros((2, 4, 5), np.uint8))                 # the alpha is a tensor
    with pytest.raises(TypeError):
        cutout.estimate_foreground(fr, a8.double())
    with pytest.raises(TypeError):
        cutout.estimate_foreground(fr, a8, radii=(90.0, 6))
    with pytest.raises(TypeError):
        cutout.cutout(fr, a8, transform_info=[{'name': 'padding', 'pad_size': (0, 0)}])   # the reverse transform takes float32
    with pytest.raises(ValueError):
        cutout.estimate_foreground(fr, a8[:, :3])
    with pytest.raises(ValueError):
        cutout.estimate_foreground(fr, a8[0, 0])
    with pytest.raises(ValueError):
        cutout.estimate_foreground(np.zeros((2, 2, 4, 5, 3), np.uint8), a8)
    for radii in ((0, 6), (90, 256), (90,), 90, (90, 6, 1)):
        with pytest.raises(ValueError):
            cutout.cutout(fr, a8, radii=radii)
    with pytest.raises(ValueError):
        cutout.save_cutouts(np.zeros((2, 4, 5, 3), np.uint8), '.', 'x')
    with pytest.raises(TypeError):
        pngenc.encode_images(np.zeros((1, 4, 4, 3), np.float32))
    for shape in ((4, 4, 3), (1, 4, 4, 2), (1, 4, 4, 1), (0, 4, 4, 3), (1, 0, 4, 3), (1, 2, 5462, 3), (1, 2, 4097, 4)):
        with pytest.raises(ValueError):
            pngenc.encode_images(np.zeros(shape, np.uint8))
    with pytest.raises(ValueError):
        pngenc.encode_image(np.zeros((1, 4, 4, 3), np.uint8))


# ---- the colour entries of the kernel source on the host, under the sanitizers -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    cxx = next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)
    assert cxx is not None, 'no host C++ compiler (g++, c++, clang++): the sanitizer run of the kernel source is the only bounds evidence, so it does not skip'
    exe = str(tmp_path_factory.mktemp('pngenc_colour_host') / 'pngenc_colour_host')
    subprocess.check_call([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-strict-aliasing', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'pngenc_colour_host.cpp')])
    return exe


def test_colour_entries_on_the_host_equal_the_restatement(host_exe, tmp_path):
    rng = np.random.RandomState(11)
    calls = []
    for ch in (3, 4):
        calls += [rng.randint(0, 256, (1, 1, 1, ch)), rng.randint(0, 256, (2, 1, 3, ch)), rng.randint(0, 256, (1, 7, 5, ch)),
                  rng.randint(0, 256, (1, 5, 4096, ch)), np.stack([C.disc_image(67, 257, ch, s) for s in range(3)]),
                  np.full((1, 33, 700, ch), 200)]
    calls = [np.ascontiguousarray(c, np.uint8) for c in calls]
    body = [struct.pack('<4i', c.shape[1], c.shape[2], c.shape[0], c.shape[3]) + c.tobytes() for c in calls]
    src, dst = str(tmp_path / 'colour.in'), str(tmp_path / 'colour.out')
    with open(src, 'wb') as f:
        f.write(struct.pack('<i', len(calls)) + b''.join(body))
    r = subprocess.run([host_exe, src, dst], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'pngenc_colour_host: ok' in r.stdout and not r.stderr.strip(), (r.stdout + r.stderr)[-3000:]
    buf, p = open(dst, 'rb').read(), 0
    for c in calls:
        N = c.shape[0]
        rc1, rc2, nb, total = struct.unpack_from('<4i', buf, p)
        p += 16
        assert (rc1, rc2) == (0, 0), c.shape
        sizes = np.frombuffer(buf, np.int64, N, p)
        p += 8 * N
        recs = np.frombuffer(buf, np.int32, N * nb * R.REC_WORDS, p).reshape(N, nb, R.REC_WORDS)
        p += recs.nbytes
        blob = buf[p:p + total]
        p += total
        at = 0
        for k in range(N):
            f, blocks = C.encode_colour(c[k])
            stream = R.idat(f)
            assert np.array_equal(recs[k], np.stack([R.record(b) for b in blocks])), (c.shape, k, 'block records')
            assert sizes[k] == len(stream) and blob[at:at + len(stream)] == stream, (c.shape, k, 'stream')
            at += len(stream)
        assert at == len(blob)
    assert p == len(buf)
