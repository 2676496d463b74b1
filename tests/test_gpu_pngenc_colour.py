"""The colour form of the device PNG encoder (`pngenc.encode_images`, the colour entries of csrc/pngenc.hip) against the sequential restatement
(tests/cutout_restatement.py: tests/pngenc_restatement.py on the colour filtered stream), which tests/test_cutout_cpu.py holds readable by
Pillow: block records first, then the stream bytes; then every reader (Pillow, `pngcolor.decode_frames` on the device); the size against
zlib's level-1 Z_RLE configuration; and the grey path, which must not have moved. Every comparison is exact."""
import ctypes
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cutout_restatement as C                                        # noqa: E402
import pngenc_restatement as R                                        # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import pngcolor, pngenc                         # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 3), (7, 5), (5, 4096), (67, 257)]
_REF = {}


def image(kind, h, w, ch):
    rs = np.random.RandomState(17 * h + w + ch)
    if kind == 'noise':
        return rs.randint(0, 256, size=(h, w, ch)).astype(np.uint8)
    if kind == 'constant':
        return np.broadcast_to(np.array([200, 17, 90, 255], np.uint8)[:ch], (h, w, ch)).copy()
    return C.disc_image(h, w, ch, seed=h + w)


def ref(kind, h, w, ch):
    """(image, file, [Block]): computed once, never modified."""
    key = (kind, h, w, ch)
    if key not in _REF:
        im = image(kind, h, w, ch)
        _REF[key] = (im,) + C.encode_colour(im, pngenc.BLOCK_BYTES)
    return _REF[key]


def check(r, want):
    """An `Encoded` of encode_images_stats(guard=...) against [(image, file, [Block])]: records, sizes, bytes, guards (the checks of
    tests/test_gpu_pngenc.py)."""
    assert len(r.files) == len(want) and r.readbacks == 2
    for k, (_, f, blocks) in enumerate(want):
        assert np.array_equal(r.recs[k], np.stack([R.record(b) for b in blocks])), (k, 'block records')
        assert r.sizes[k] == len(R.idat(f)), (k, 'stream size')
        assert r.streams[k] == R.idat(f), (k, 'stream bytes')
        assert r.files[k] == f, (k, 'file')
    assert len(r.guards) == 6 and all(bool((g == 0xA5).all()) for g in r.guards)
    assert r.blob.numel() == int(r.sizes.sum()) and not bool(r.slack.any())


@pytest.mark.parametrize('ch', [3, 4])
@pytest.mark.parametrize('h,w', SIZES)
def test_files_equal_the_restatement_and_every_reader_returns_the_image(h, w, ch):
    want = [ref(kind, h, w, ch) for kind in ('noise', 'constant', 'disc')]
    x = torch.from_numpy(np.stack([im for im, _, _ in want])).cuda()
    r = pngenc.encode_images_stats(x, guard=64)
    check(r, want)
    assert pngenc.encode_images(x) == [f for _, f, _ in want]
    assert pngenc.encode_image(x[2]) == want[2][1] and pngenc.encode_image(want[0][0]) == want[0][1]      # one image; an array is uploaded
    for (im, _, blocks), f in zip(want, r.files):
        back = Image.open(io.BytesIO(f))
        assert back.mode == ('RGB' if ch == 3 else 'RGBA') and np.array_equal(np.asarray(back), im)
        z = zlib.compressobj(1, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
        zl = len(z.compress(C.filtered_colour(im).tobytes()) + z.flush())
        stream = len(R.idat(f))
        print('%d x %d x %d: %d bytes, zlib Z_RLE level 1 %d, %d blocks' % (h, w, ch, stream, zl, len(blocks)))
        assert stream <= 1.02 * zl + 32 * len(blocks), (h, w, ch, stream, zl)
    frames = pngcolor.decode_frames(r.files)
    assert frames.is_cuda and frames.dtype == torch.uint8 and torch.equal(frames, x[..., :3])


def test_block_edges_fall_inside_a_pixel():
    """5 x 4096: a row of 16 385 (RGBA) or 12 289 (RGB) filtered bytes against blocks of 16 384."""
    for ch, nb in ((4, 6), (3, 4)):
        _, f, blocks = ref('noise', 5, 4096, ch)
        assert len(blocks) == nb == pngenc.blocks_of(5, ch * 4096)
        assert any((k * pngenc.BLOCK_BYTES) % (1 + ch * 4096) % ch != 1 for k in range(1, nb))     # an edge that is not at a pixel's first byte


def test_two_calls_give_identical_bytes():
    x = torch.from_numpy(np.stack([ref(kind, 67, 257, 4)[0] for kind in ('noise', 'disc')])).cuda()
    a, b = pngenc.encode_images(x), pngenc.encode_images(x)
    assert a == b and all(isinstance(f, bytes) for f in a)


def test_grey_files_are_unchanged():
    cases = R.cases(pngenc.BLOCK_BYTES)
    for name in ('mixed_130x67', 'stream_Bp1'):
        p = cases[name]
        planes = np.stack([p, np.ascontiguousarray(np.roll(p, 3, axis=1))])
        want = [R.encode(q, pngenc.BLOCK_BYTES) for q in planes]
        r = pngenc.encode_stats(planes, guard=64)
        check(r, [(None,) + w for w in want])
        assert pngenc.encode_planes(torch.from_numpy(planes).cuda()) == [f for f, _ in want]


def test_argument_errors_return_minus_two_before_any_launch():
    L = hip.lib()
    x = torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device='cuda')
    recs = torch.zeros((2 * pngenc.REC_WORDS + 4,), dtype=torch.int32, device='cuda')
    sizes = torch.zeros((4,), dtype=torch.int64, device='cuda')
    out = torch.zeros((256,), dtype=torch.uint8, device='cuda')
    P, I, Lg, V = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    torch.cuda.synchronize()

    def size(im=x.data_ptr(), ch=4, n=2, h=8, w=8, r=recs.data_ptr(), s=sizes.data_ptr()):
        return L.mg_pngenc_size_rgb(P(im), I(ch), Lg(n), I(h), I(w), P(r), P(s), V(None))

    def emit(im=x.data_ptr(), ch=4, n=2, h=8, w=8, r=recs.data_ptr(), s=sizes.data_ptr(), o=out.data_ptr(), nbytes=256):
        return L.mg_pngenc_emit_rgb(P(im), I(ch), Lg(n), I(h), I(w), P(r), P(s), P(o), Lg(nbytes), V(None))

    assert size(im=None) == -2 and size(r=None) == -2 and size(s=None) == -2
    assert size(ch=1) == -2 and size(ch=2) == -2 and size(ch=5) == -2 and size(ch=0) == -2 and size(n=0) == -2 and size(n=pngenc.MAX_PLANES + 1) == -2
    assert size(h=0) == -2 and size(w=0) == -2 and size(h=pngenc.MAX_SIDE + 1) == -2 and size(w=4097) == -2 and size(ch=3, w=5462) == -2
    assert size(r=recs.data_ptr() + 2) == -2 and size(s=sizes.data_ptr() + 4) == -2
    assert emit(im=None) == -2 and emit(r=None) == -2 and emit(s=None) == -2 and emit(o=None) == -2 and emit(ch=6) == -2 and emit(w=4097) == -2
    assert emit(o=out.data_ptr() + 4) == -2 and emit(nbytes=254) == -2 and emit(nbytes=0) == -2
    torch.cuda.synchronize()
    assert not bool(recs.any()) and not bool(sizes.any()) and not bool(out.any())                      # nothing ran
    with pytest.raises(TypeError):
        pngenc.encode_images(x.float())
    with pytest.raises(ValueError):
        pngenc.encode_images(x[0])
    with pytest.raises(ValueError):
        pngenc.encode_images(torch.zeros((1, 2, 4097, 4), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        pngenc.encode_images(torch.zeros((1, 2, 5462, 3), dtype=torch.uint8, device='cuda'))
