"""The device PNG frame decoder (maggie_amd.utils.pngcolor, csrc/pngcolor.hip) against the sequential restatement of
tests/pngcolor_restatement.py, which tests/test_pngcolor_cpu.py holds equal to live Pillow, and against the pinned fixture: the defiltered
bytes first, then the pixels, so that a wrong pixel points at the right kernel. Well-formed streams only; every comparison is exact."""
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pngcolor_restatement as R                                      # noqa: E402
from maggie_amd.utils import pngcolor, pngdec                          # noqa: E402
from maggie_amd.utils.preprocess import normalize_frames              # noqa: E402

pytestmark = pytest.mark.gpu
P = R.P
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pngcolor_pinned.npz')
_CASES, _REF = {}, {}


def cases():
    if not _CASES:
        _CASES.update(R.small_cases())
        _CASES.update(R.clip_cases())
    return _CASES


def ref(name):
    """(file, defiltered bytes, RGB, L) of a case: computed once, never modified. The frames of the 270 x 480 clip come from live Pillow (the
    sequential restatement takes a second a frame; tests/test_pngcolor_cpu.py runs it): the defiltered scanlines of a non-interlaced RGB-8 file
    are its filter type bytes and its pixels."""
    if name not in _REF:
        d = cases()[name]
        if name.startswith('clip'):
            rgb, l = R.pillow(d)
            types = np.frombuffer(zlib.decompress(P.walk(d)[2]), np.uint8).reshape(rgb.shape[0], -1)[:, :1]
            _REF[name] = (d, np.concatenate([types, rgb.reshape(rgb.shape[0], -1)], 1).tobytes(), rgb, l)
        else:
            _REF[name] = (d,) + R.decode(d)
    return _REF[name]


def check(r, names, planes=False):
    """`raw` first, then the pixels, of a `Decoded` against the references of `names`."""
    assert (r.status == 0).all() and r.readbacks == 1 and r.launches == 3
    raw = r.raw.cpu().numpy()
    out = r.out.cpu().numpy()
    for k, n in enumerate(names):
        _, want_raw, rgb, l = ref(n)
        assert r.raw_sizes[k] == len(want_raw) and raw[k, :len(want_raw)].tobytes() == want_raw, (n, 'defiltered bytes')
        want = l if planes else rgb
        assert out[k].shape == want.shape and np.array_equal(out[k], want), (n, 'pixels')


@pytest.mark.parametrize('part', range(4))
def test_decode_is_exact_on_the_list(part):
    for name in [n for n in cases() if not n.startswith('clip')][part::4]:
        d = ref(name)[0]
        check(pngcolor.decode_stats([d]), [name])
        check(pngcolor.decode_stats([d], planes=True), [name], planes=True)


def test_single_file_forms():
    for name in ('pair_c6_d16_i1_17x13', 'grey16_edges_i0_4x2', 'size_c0_d1_i1_1x1', 'band_c2_d8_i1_9x131'):
        d, _, rgb, l = ref(name)
        a, b = pngcolor.decode_frame(d), pngcolor.decode(d)
        assert a.dtype == torch.uint8 and a.is_cuda and a.shape == rgb.shape and np.array_equal(a.cpu().numpy(), rgb), name
        assert b.dtype == torch.uint8 and b.is_cuda and b.shape == l.shape and np.array_equal(b.cpu().numpy(), l), name
        n = pngcolor.decode_frame(d, normalize=True)
        assert n.dtype == torch.float32 and n.shape == (3,) + l.shape


def test_clips_of_mixed_type_depth_and_interlace():
    by_size = {}
    for n, d in cases().items():
        by_size.setdefault(P.walk(d)[0][:2], []).append(n)
    groups = [g for g in by_size.values() if len(g) > 1]
    assert any(len({P.walk(cases()[n])[0][2:4] + P.walk(cases()[n])[0][6:] for n in g}) == 30 for g in groups)     # all 15 pairs x interlace in one launch
    for g in groups:
        check(pngcolor.decode_stats([ref(n)[0] for n in g]), g)
        check(pngcolor.decode_stats([ref(n)[0] for n in g], planes=True), g, planes=True)
    three = ['pair_c3_d2_i1_17x13', 'pair_c6_d16_i0_17x13', 'pair_c0_d16_i1_17x13']
    frames = pngcolor.decode_frames([ref(n)[0] for n in three])
    assert frames.shape == (3, 13, 17, 3) and np.array_equal(frames.cpu().numpy(), np.stack([ref(n)[2] for n in three]))
    planes = pngcolor.decode_planes([ref(n)[0] for n in three])
    assert planes.shape == (3, 13, 17) and np.array_equal(planes.cpu().numpy(), np.stack([ref(n)[3] for n in three]))
    with pytest.raises(ValueError, match='out must be'):
        pngcolor.decode_frames([ref(n)[0] for n in three], out=torch.empty((2, 13, 17, 3), dtype=torch.uint8, device='cuda'))


def test_fixture_key_by_key():
    z = np.load(GOLDEN)
    names = sorted(k[5:] for k in z.files if k.startswith('file_'))
    assert len(names) >= 19
    for name in names:
        d = z['file_' + name].tobytes()
        assert np.array_equal(pngcolor.decode_frame(d).cpu().numpy(), z['rgb_' + name]), name
        assert np.array_equal(pngcolor.decode(d).cpu().numpy(), z['l_' + name]), name


def test_clip_of_four_frames_uint8_and_normalised():
    names = sorted(n for n in cases() if n.startswith('clip'))
    assert len(names) == 4
    files = [ref(n)[0] for n in names]
    r = pngcolor.decode_stats(files)
    check(r, names)
    assert r.out.shape == (4, 270, 480, 3)
    norm = pngcolor.decode_frames(files, normalize=True)
    assert norm.dtype == torch.float32 and norm.shape == (4, 3, 270, 480) and torch.equal(norm, normalize_frames(r.out))
    m, s = (0.5, 0.25, 0.125), (0.3, 0.2, 0.1)
    assert torch.equal(pngcolor.decode_frames(files[:2], normalize=True, mean=m, std=s), normalize_frames(r.out[:2], m, s))
    # the normalised form of a width that is no multiple of 16, of an interlaced palette file
    d, _, rgb, _ = ref('pair_c3_d4_i1_17x13')
    x = rgb.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    want = (x - np.array(pngcolor.IMAGENET_MEAN, np.float32)[:, None, None]) / np.array(pngcolor.IMAGENET_STD, np.float32)[:, None, None]
    assert np.array_equal(pngcolor.decode_frame(d, normalize=True).cpu().numpy().view(np.int32), want.view(np.int32))


def test_out_in_an_odd_offset_slice_between_guards():
    for name, front, mode in (('pair_c2_d8_i1_17x13', 13, pngcolor.OUT_RGB), ('pair_c6_d16_i0_17x13', 1, pngcolor.OUT_RGB),
                              ('lane_c3_d4_i1_33x3', 7, pngcolor.OUT_L), ('band_c2_d8_i1_9x131', 2, pngcolor.OUT_RGB),
                              ('lane_c2_d8_i0_16x3', 3, pngcolor.OUT_RGB), ('lane_c2_d8_i0_16x3', 5, pngcolor.OUT_L)):
        d, want_raw, rgb, l = ref(name)
        want = l if mode == pngcolor.OUT_L else rgb
        plan = pngcolor.parse(d)
        blob = torch.frombuffer(bytearray(b'\xff' * front + plan.stream + b'\xff' * 29), dtype=torch.uint8).cuda()
        rec = pngcolor.record(plan, front)[None]
        # an allocated destination between guards
        r = pngcolor.run(blob, rec, plan.height, plan.width, mode, guard=64)
        check(r, [name], planes=mode == pngcolor.OUT_L)
        assert len(r.guards) == 4 and all(bool((g == 0xA5).all()) for g in r.guards), name
        assert (r.raw.cpu().numpy()[0, len(want_raw):] == 0xA5).all(), name                # nothing behind the file's own bytes either
        # the caller's destination: a slice that starts at an odd byte of a larger buffer
        big = torch.full((want.size + 64,), 0xA5, dtype=torch.uint8, device='cuda')
        at = (16 + front) | 1
        r = pngcolor.run(blob, rec, plan.height, plan.width, mode, out=big[at:at + want.size], guard=64)
        assert r.out.data_ptr() == big.data_ptr() + at and r.readbacks == 1
        host = big.cpu().numpy()
        assert np.array_equal(host[at:at + want.size].reshape(want.shape), want), name
        assert (host[:at] == 0xA5).all() and (host[at + want.size:] == 0xA5).all(), name
        assert all(bool((g == 0xA5).all()) for g in r.guards), name


def _jpeg(x, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def test_load_frames_on_a_png_a_baseline_and_a_progressive_jpeg():
    from PIL import Image
    x = P.content(32, 48, 'smooth', 3, 3)
    png = R.make(x.astype(np.int64), 2, 8, interlace=1, seed=5)
    files = [_jpeg(x, quality=90), png, _jpeg(x, quality=85, progressive=True)]
    want = np.stack([np.asarray(Image.open(io.BytesIO(d)).convert('RGB')) for d in files])
    assert np.array_equal(want[1], x)
    got = pngcolor.load_frames(files)
    assert got.dtype == torch.uint8 and got.shape == (3, 32, 48, 3) and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(pngcolor.load_frames(files, normalize=True), normalize_frames(got))
    assert np.array_equal(pngcolor.load_frames([png]).cpu().numpy(), want[1:2])
    assert np.array_equal(pngcolor.load_frames(files[::2]).cpu().numpy(), want[::2])


def test_load_planes_on_files_of_both_decoders():
    names = ['pair_c0_d8_i1_17x13', 'pair_c0_d8_i0_17x13', 'pair_c4_d16_i0_17x13', 'pair_c3_d4_i0_17x13', 'pair_c2_d16_i1_17x13']
    files = [ref(n)[0] for n in names]
    routed = []
    for d in files:
        try:
            pngdec.parse(d)
            routed.append(0)
        except pngdec.Unsupported:
            routed.append(1)
    assert routed == [1, 0, 1, 0, 1]
    got = pngcolor.load_planes(files)
    assert got.dtype == torch.uint8 and got.shape == (5, 13, 17) and np.array_equal(got.cpu().numpy(), np.stack([ref(n)[3] for n in names]))
    assert np.array_equal(got.cpu().numpy()[[1, 3]], pngdec.decode_planes([files[1], files[3]]).cpu().numpy())
