"""The device JPEG decoder (maggie_amd.utils.jpegdec, csrc/jpegdec.hip) against the sequential restatement of tests/jpegdec_restatement.py, which
tests/test_jpegdec_cpu.py holds against Pillow itself: the coefficients first, then the component planes, then the pixels, so that a wrong
pixel points at the right kernel. Well-formed streams only; every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

import jpegdec_restatement as R                                       # noqa: E402
import make_jpegdec_golden as G                                       # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd.utils import geometry, jpegdec                        # noqa: E402
from maggie_amd.utils._inputs import IMAGENET_MEAN, IMAGENET_STD      # noqa: E402
from maggie_amd.utils.preprocess import normalize_frames              # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(R.CASES)
SPECIAL = [n for n in NAMES if any(k in n for k in ('res', 'opt', 'qta', 'periodic'))] + ['64x48_uniform_0_qua100']
_REF = {}


def ref(name):
    """(stream, coefficients, planes flattened in the device's layout, pixels) of a case: computed once, never modified."""
    if name not in _REF:
        data = R.stream(*(R.LARGE if name == 'large' else R.CASES[name]))
        coef = R.coefficients(data)
        planes = np.concatenate([p.reshape(-1) for p in R.planes_of(data, coef)]).astype(np.uint8)
        _REF[name] = (data, coef, planes, R.pixels(data, coef))
    return _REF[name]


def check(name, sub_bytes=None):
    data, coef, planes, px = ref(name)
    r = jpegdec.decode_stats([data], sub_bytes=sub_bytes)
    assert np.array_equal(r.coef.cpu().numpy().reshape(-1, 64), coef), (name, sub_bytes, 'coefficients')
    assert np.array_equal(r.planes.cpu().numpy(), planes), (name, sub_bytes, 'planes')
    assert r.out.shape == (1,) + px.shape and np.array_equal(r.out[0].cpu().numpy(), px), (name, sub_bytes, 'pixels')
    assert r.rounds <= r.subsequences and r.launches <= -(-r.subsequences // jpegdec.THREADS) + 2
    return r


@pytest.mark.parametrize('part', range(8))
def test_decode_equals_the_restatement_on_the_list(part):
    for name in NAMES[part::8]:
        data, _, _, px = ref(name)
        out = jpegdec.decode(data)
        assert out.dtype == torch.uint8 and out.is_cuda and np.array_equal(out.cpu().numpy(), px), name
        check(name)


@pytest.mark.parametrize('sub_bytes', R.SUB_BYTES)
def test_every_sub_bytes_gives_the_same_coefficients(sub_bytes):
    for name in SPECIAL + NAMES[3::9]:
        check(name, sub_bytes)


def test_the_large_stream_spans_several_workgroups_at_the_default():
    r = check('large')
    assert r.subsequences > 2 * jpegdec.THREADS and r.readbacks >= 1
    check('large', 29)


def test_the_periodic_stream_stays_within_the_round_bound():
    r = check('64x256_periodic_2_qua100', jpegdec.MIN_SUB)
    assert r.subsequences > 8 * jpegdec.THREADS and r.subsequences // 4 < r.rounds <= r.subsequences
    assert 2 < r.launches <= -(-r.subsequences // jpegdec.THREADS) + 2 and r.readbacks == r.launches


@pytest.mark.parametrize('names', [['37x53_uniform_2_qua90_res1', '37x53_uniform_2_optT_qua90', '37x53_flat_2_qua1'],
                                   ['64x48_smooth_0_optT_qua50', '64x48_uniform_0_qua100_res3', '64x48_uniform_0_qua100'],
                                   ['33x65_binary_L_qta1', '33x65_binary_L_qta255', '33x65_uniform_L_qua100'], ['17x23_flat_2_qua90']])
def test_decode_clip_takes_per_frame_tables_and_offsets(names):
    datas = [ref(n)[0] for n in names]
    want = np.stack([ref(n)[3] for n in names])
    for s in R.SUB_BYTES:
        r = jpegdec.decode_stats(datas, sub_bytes=s)
        assert np.array_equal(r.coef.cpu().numpy(), np.stack([ref(n)[1] for n in names])), s
        assert np.array_equal(r.out.cpu().numpy(), want), s
    out = jpegdec.decode_clip(datas)
    assert out.shape == want.shape and np.array_equal(out.cpu().numpy(), want)
    norm = jpegdec.decode_clip(datas, normalize=True)
    assert norm.shape == (len(names), 3) + want.shape[1:3] and np.array_equal(norm.cpu().numpy(), R.P.normalize(want, IMAGENET_MEAN, IMAGENET_STD))


@pytest.mark.parametrize('name', ['16x16_uniform_2_qua50', '16x16_uniform_0_qua50', '16x16_uniform_L_qua50', '37x53_uniform_2_qua90',
                                  '37x53_uniform_0_qua90', '9x4_uniform_L_qua90', '64x48_uniform_0_qua100', '1x1_uniform_2_qua1'])
def test_normalize_epilogue(name):
    data, _, _, px = ref(name)
    mean, std = (0.4, 0.5, 0.6), (0.2, 0.25, 0.3)
    for m, s in ((IMAGENET_MEAN, IMAGENET_STD), (mean, std)):
        out = jpegdec.decode(data, normalize=True, mean=m, std=s)
        assert out.dtype == torch.float32 and out.shape == (3,) + px.shape[:2]
        assert np.array_equal(out.cpu().numpy(), R.P.normalize(px[None], m, s)[0])
        if px.shape[0] * px.shape[1] % 4 == 0:                              # where normalize_frames is defined
            assert torch.equal(out, normalize_frames(jpegdec.decode(data), m, s))


@pytest.mark.parametrize('name', G.PINNED)
def test_fixture_key_by_key(name):
    d = load_golden('jpegdec_pinned.npz')
    out = jpegdec.decode(d[name + '.stream'].tobytes())
    assert np.array_equal(out.cpu().numpy(), d[name + '.pixels'])


@pytest.mark.parametrize('name', ['37x53_uniform_2_qua90_res1', '37x53_uniform_0_optT_qua90', '33x65_uniform_L_qua100'])
def test_odd_offset_inside_a_larger_buffer_and_guarded_outputs(name):
    data, coef, _, px = ref(name)
    plan = jpegdec.parse(data)
    h, w, layout = plan.geometry
    for pad in (1, 3, 7):
        blob = torch.from_numpy(np.frombuffer(b'\xff' * pad + data + b'\xff\x00\xd0' * 11, np.uint8).copy()).cuda()
        for normalize in (False, True):
            n = h * w * 3
            guard = torch.full((n + 64,), 7, dtype=torch.float32 if normalize else torch.uint8, device='cuda')
            r = jpegdec.run(blob, jpegdec.record(plan, pad)[None], h, w, layout, sub_bytes=29, normalize=normalize, out=guard[13:13 + n])
            assert np.array_equal(r.coef.cpu().numpy()[0], coef)
            got = guard.cpu().numpy()
            assert (got[:13] == 7).all() and (got[13 + n:] == 7).all()
            want = R.P.normalize(px[None], IMAGENET_MEAN, IMAGENET_STD)[0] if normalize else px
            assert np.array_equal(got[13:13 + n].reshape(want.shape), want)


def test_decode_feeds_resize_short_pad():
    data, _, _, px = ref('64x48_smooth_2_qua50_res1')
    a = geometry.resize_short_pad(jpegdec.decode(data), short_size=96, divisor=32)
    b = geometry.resize_short_pad(R.pillow(data), short_size=96, divisor=32)
    assert a[0].shape == b[0].shape and torch.equal(a[0], b[0])
