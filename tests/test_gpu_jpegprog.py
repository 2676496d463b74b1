"""The device progressive JPEG decoder (maggie_amd.utils.jpegprog, csrc/jpegprog.hip) against the sequential restatement of
tests/jpegprog_restatement.py, which tests/test_jpegprog_cpu.py holds against Pillow itself: the coefficients first, then the component planes,
then the pixels, so that a wrong pixel points at the right stage. Every comparison is exact. The three corrupt streams at the end are malformed
inputs that the bounded loops reject by status bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

import jpegprog_restatement as J                                      # noqa: E402
import make_jpegprog_golden as G                                      # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd.utils import geometry, jpegdec, jpegprog              # noqa: E402
from maggie_amd.utils._inputs import IMAGENET_MEAN, IMAGENET_STD      # noqa: E402
from maggie_amd.utils.preprocess import normalize_frames              # noqa: E402

pytestmark = pytest.mark.gpu
R = J.R
NAMES = list(J.CASES)
PARTS = 16
_REF = {}


def ref(name):
    """(stream, coefficients, planes flattened in the device's layout, pixels) of a case: computed once, never modified."""
    if name not in _REF:
        data = J.named(name)
        coef = J.coefficients(data)
        planes = np.concatenate([p.reshape(-1) for p in J.planes_of(data, coef)]).astype(np.uint8)
        _REF[name] = (data, coef, planes, J.pixels(data, coef))
    return _REF[name]


def check(name):
    data, coef, planes, px = ref(name)
    r = jpegprog.decode_stats([data])
    assert np.array_equal(r.coef.cpu().numpy().reshape(-1, 64), coef), (name, 'coefficients')
    assert np.array_equal(r.planes.cpu().numpy(), planes), (name, 'planes')
    assert r.out.shape == (1,) + px.shape and np.array_equal(r.out[0].cpu().numpy(), px), (name, 'pixels')
    assert r.readbacks == 1 and r.launches == 3
    return r


@pytest.mark.parametrize('part', range(PARTS))
def test_decode_equals_the_restatement_on_the_list(part):
    for name in NAMES[part::PARTS]:
        data, _, _, px = ref(name)
        out = jpegprog.decode(data)
        assert out.dtype == torch.uint8 and out.is_cuda and np.array_equal(out.cpu().numpy(), px), name
        r = check(name)
        assert r.chains == (2 if '_L_' in name else 4), name              # one DC chain and one AC chain per component


@pytest.mark.parametrize('name', list(J.RESTART))
def test_restart_markers_in_every_scan(name):
    data = ref(name)[0]
    assert data.count(b'\xff\xdd') >= 1 and sum(data.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) > 8
    check(name)


def test_the_large_stream_refills_the_byte_window_many_times():
    plan = jpegprog.parse(ref('large')[0])
    assert max(s.length for s in plan.scans) > 16 * 2048                    # the window in LDS holds 2 048 bytes
    check('large')


def test_the_longest_end_of_band_runs():
    """1472 x 1472 with AC terms in the first block only: the AC-first scans hold run class 14 (the encoder flushes at 32 767) and every
    refinement scan walks 33 855 blocks that read no bit."""
    data = ref('runs')[0]
    assert len(data) < 32 * 1024 and jpegprog.parse(data).geometry == (J.RUNS_SIDE, J.RUNS_SIDE, jpegdec.L444)
    r = check('runs')
    assert r.coef.shape == (1, 3 * 184 * 184, 64)


@pytest.mark.parametrize('names', [['37x53_uniform_2_q1', '37x53_uniform_2_q50', '37x53_uniform_2_q100'],
                                   ['64x48_smooth_0_q100', '64x48_smooth_0_q1', '64x48_smooth_0_q50_rows1'],
                                   ['33x65_binary_L_q90', '33x65_binary_L_q100_blocks1', '33x65_binary_L_q50'], ['17x23_flat_2_q90']])
def test_decode_clip_takes_per_file_scripts_and_tables(names):
    datas = [ref(n)[0] for n in names]
    want = np.stack([ref(n)[3] for n in names])
    assert len({len(d) for d in datas}) == len(datas)                       # other qualities: other tables and scan lengths
    r = jpegprog.decode_stats(datas)
    assert np.array_equal(r.coef.cpu().numpy(), np.stack([ref(n)[1] for n in names]))
    assert np.array_equal(r.out.cpu().numpy(), want) and r.readbacks == 1 and r.launches == 3
    assert r.chains == len(names) * (2 if '_L_' in names[0] else 4)
    out = jpegprog.decode_clip(datas)
    assert out.shape == want.shape and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
    norm = jpegprog.decode_clip(datas, normalize=True)
    assert norm.shape == (len(names), 3) + want.shape[1:3] and np.array_equal(norm.cpu().numpy(), R.P.normalize(want, IMAGENET_MEAN, IMAGENET_STD))


@pytest.mark.parametrize('name', ['16x16_uniform_2_q50', '16x16_uniform_0_q50', '16x16_uniform_L_q50', '37x53_uniform_2_q90',
                                  '37x53_uniform_0_q90', '9x4_uniform_L_q90', '64x48_uniform_0_q100', '1x1_uniform_2_q1'])
def test_normalize_epilogue(name):
    data, _, _, px = ref(name)
    mean, std = (0.4, 0.5, 0.6), (0.2, 0.25, 0.3)
    for m, s in ((IMAGENET_MEAN, IMAGENET_STD), (mean, std)):
        out = jpegprog.decode(data, normalize=True, mean=m, std=s)
        assert out.dtype == torch.float32 and out.shape == (3,) + px.shape[:2]
        assert np.array_equal(out.cpu().numpy(), R.P.normalize(px[None], m, s)[0])
        if px.shape[0] * px.shape[1] % 4 == 0:                              # where normalize_frames is defined
            assert torch.equal(out, normalize_frames(jpegprog.decode(data), m, s))


@pytest.mark.parametrize('name', G.PINNED)
def test_fixture_key_by_key(name):
    d = load_golden('jpegprog_pinned.npz')
    out = jpegprog.decode(d[name + '.stream'].tobytes())
    assert np.array_equal(out.cpu().numpy(), d[name + '.pixels'])


def test_load_clip_of_a_mixed_list_makes_one_launch_set_per_group(monkeypatch):
    case = (64, 48, 'smooth', 2)
    datas = [R.stream(*case, dict(quality=50)), J.stream(*case, dict(quality=90, progressive=True)),
             R.stream(*case, dict(quality=90, restart_marker_blocks=3)), J.stream(*case, dict(quality=50, progressive=True, restart_marker_rows=1))]
    want = np.stack([R.pillow(d) for d in datas])
    calls = {'baseline': 0, 'progressive': 0}
    base_run, prog_run = jpegdec.run, jpegprog.run

    def count(key, fn):
        def wrapped(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return wrapped
    monkeypatch.setattr(jpegdec, 'run', count('baseline', base_run))
    monkeypatch.setattr(jpegprog, 'run', count('progressive', prog_run))
    out = jpegprog.load_clip(datas)
    assert calls == {'baseline': 1, 'progressive': 1}
    assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
    for k, d in enumerate(datas):
        assert np.array_equal(jpegprog.load(d).cpu().numpy(), want[k]), k
    assert np.array_equal(jpegprog.decode(datas[1]).cpu().numpy(), want[1]) and np.array_equal(jpegdec.decode(datas[0]).cpu().numpy(), want[0])
    norm = jpegprog.load_clip(datas, normalize=True)
    assert np.array_equal(norm.cpu().numpy(), R.P.normalize(want, IMAGENET_MEAN, IMAGENET_STD))
    assert np.array_equal(jpegprog.load_clip(datas[::2]).cpu().numpy(), want[::2])       # one kind only: no reordering
    assert np.array_equal(jpegprog.load_clip(datas[1::2]).cpu().numpy(), want[1::2])


@pytest.mark.parametrize('name', ['37x53_uniform_2_q90_blocks1', '37x53_uniform_0_q90', '33x65_uniform_L_q100'])
def test_odd_offset_inside_a_larger_buffer_and_guarded_outputs(name):
    data, coef, _, px = ref(name)
    plan = jpegprog.parse(data)
    h, w, layout = plan.geometry
    for pad in (1, 3, 7):
        blob = torch.from_numpy(np.frombuffer(b'\xff' * pad + data + b'\xff\x00\xd0' * 11, np.uint8).copy()).cuda()
        scans, chains = jpegprog.records(plan, pad, 0, 0)
        for normalize in (False, True):
            n = h * w * 3
            guard = torch.full((n + 64,), 7, dtype=torch.float32 if normalize else torch.uint8, device='cuda')
            r = jpegprog.run(blob, scans, chains, plan.qtables[None], h, w, layout, normalize=normalize, out=guard[13:13 + n])
            assert np.array_equal(r.coef.cpu().numpy()[0], coef)
            got = guard.cpu().numpy()
            assert (got[:13] == 7).all() and (got[13 + n:] == 7).all()
            want = R.P.normalize(px[None], IMAGENET_MEAN, IMAGENET_STD)[0] if normalize else px
            assert np.array_equal(got[13:13 + n].reshape(want.shape), want)


def test_decode_feeds_resize_short_pad():
    data = ref('64x48_smooth_2_q50_rows1')[0]
    a = geometry.resize_short_pad(jpegprog.decode(data), short_size=96, divisor=32)
    b = geometry.resize_short_pad(R.pillow(data), short_size=96, divisor=32)
    assert a[0].shape == b[0].shape and torch.equal(a[0], b[0])


# ---- malformed streams: a status bit, a ValueError, and the call returns -----------------------------------------------------------------------
def truncated(data):
    """The longest scan's segment cut in half."""
    s = max(J.parse(data)['scans'], key=lambda s: s['length'])
    return data[:s['offset'] + s['length'] // 2] + data[s['offset'] + s['length']:]


def exchanged(data):
    """The segments of the last two refinement scans (two components' last bits, or for grey the DC bit and the AC bits) exchanged."""
    a, b = J.parse(data)['scans'][-2:]
    sa, sb = data[a['offset']:a['offset'] + a['length']], data[b['offset']:b['offset'] + b['length']]
    return data[:a['offset']] + sb + data[a['offset'] + a['length']:b['offset']] + sa + data[b['offset'] + b['length']:]


def short_table(data, number):
    """The AC table in front of scan `number` without its last code, which is the longest one: the scan uses every code of its optimised table."""
    s = J.parse(data)['scans'][number]
    at = data.rfind(b'\xff\xc4', 0, s['offset'])
    size = (data[at + 2] << 8) | data[at + 3]
    seg = bytearray(data[at + 4:at + 2 + size])
    assert seg[0] >> 4 == 1 and len(seg) == 17 + sum(seg[1:17])               # one AC table
    longest = max(l for l in range(16) if seg[1 + l])
    seg[1 + longest] -= 1
    del seg[-1]
    return data[:at + 2] + (len(seg) + 2).to_bytes(2, 'big') + bytes(seg) + data[at + 2 + size:]


CORRUPT = {'truncated': truncated, 'exchanged': exchanged, 'short_table': lambda d: short_table(d, 1)}


@pytest.mark.parametrize('kind', list(CORRUPT))
@pytest.mark.parametrize('name', ['64x48_uniform_2_q90', '37x53_uniform_L_q90'])
def test_a_corrupt_stream_raises_and_the_call_returns(kind, name):
    good = ref(name)[0]
    bad = CORRUPT[kind](good)
    assert bad != good and jpegprog.parse(bad).geometry == jpegprog.parse(good).geometry     # the headers still stand
    with pytest.raises(ValueError):
        J.coefficients(bad)                                                 # the restatement refuses it too
    with pytest.raises(ValueError, match='corrupt entropy-coded segment'):
        jpegprog.decode(bad)
    with pytest.raises(ValueError, match=r'file 1\)'):
        jpegprog.decode_clip([good, bad, good])
    assert np.array_equal(jpegprog.decode(good).cpu().numpy(), ref(name)[3])                 # and the next call decodes
