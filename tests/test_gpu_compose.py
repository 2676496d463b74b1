"""Compositing on the device (csrc/compose.hip, maggie_amd.utils.compose) against the NumPy restatement (tests/compose_restatement.py, which
tests/test_compose_cpu.py holds against the live Pillow on these very cases) and the fixture Pillow wrote (tests/golden/compose_pinned.npz).
Integer work and single IEEE operations: every comparison of pixels and planes is exact. The areas of `try_place` are fp64 sums in the
device's own fixed order (strided partials, a tree, then the partials in index order), which is not the restatement's (math.fsum, the exact
sum rounded once): they are compared to 1e-12 relative, the bound of a few thousand fp64 additions of values in 0..1. No Pillow here."""
import faulthandler
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import compose_restatement as R                                       # noqa: E402
import photometric_restatement as P                                   # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd.utils import compose                                  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq(out, ref):
    return torch.equal(out.cpu(), torch.from_numpy(np.ascontiguousarray(ref)))


def _golden():
    if 'golden' not in _REF:
        g = load_golden('compose_pinned.npz')
        _REF['golden'] = {k: g[k] for k in g.files}
    return _REF['golden']


def _resized(channels, name):
    """Pillow's outputs of every RESIZE_CASES entry, from the fixture."""
    key = ('resized', channels, name)
    if key not in _REF:
        _REF[key] = R.resize_unpack(_golden()['resize/%d/%s' % (channels, name)], channels)
    return _REF[key]


def _offset_view(shape, offset, dev):
    """An uninitialised contiguous uint8 view `offset` bytes past an allocation."""
    n = int(np.prod(shape))
    t = torch.full((n + 16,), 7, dtype=torch.uint8, device=dev)[offset:offset + n].view(shape)
    assert t.data_ptr() % 16 == offset
    return t


@pytest.mark.parametrize('name', R.FILTERS)
@pytest.mark.parametrize('channels', (1, 3))
@pytest.mark.parametrize('index', range(len(R.RESIZE_CASES)))
def test_pil_resize_equals_pillow_in_both_forms(index, channels, name):
    dev = _dev()
    (h, w), (oh, ow), crop = R.RESIZE_CASES[index]
    src = R.resize_input(index, channels)
    want = _resized(channels, name)[index]
    assert (R.resize(src, (ow, oh), name, crop) == want).all()               # restatement == fixture
    tables = compose.ResizeTables((w, h) if crop is None else (crop[2] - crop[0], crop[3] - crop[1]), (ow, oh), name)
    forms = [None, 'two_pass'] + (['fused'] if tables.rows <= compose.MAX_ROWS else [])
    if index == 8:
        assert tables.regime == compose.TWO_PASS                            # the case that does not fit LDS
    s = _T(src, dev)
    for regime in forms:
        got = compose.pil_resize(s, (ow, oh), name, crop, regime=regime, channels=channels)
        assert got.shape == want.shape and _eq(got, want), regime
    for offset in (1, 4):                                                    # outputs at bases that are not 16-byte aligned, from both store paths
        for regime in (None, 'two_pass'):
            out = _offset_view(want.shape, offset, dev)
            compose.pil_resize(s, (ow, oh), name, crop, regime=regime, out=out, channels=channels)
            assert _eq(out, want), (offset, regime)


def test_pil_resize_of_a_stack_and_of_a_host_array():
    dev = _dev()
    srcs = np.stack([R.resize_input(0, 3), R.resize_input(0, 3)[::-1].copy()])
    got = compose.pil_resize(srcs, (71, 20), 'bicubic', device=dev)
    assert got.is_cuda and got.shape == (2, 20, 71, 3)
    for k in range(2):
        assert _eq(got[k], R.resize(srcs[k], (71, 20), 'bicubic'))


@pytest.mark.parametrize('channels', (1, 3))
def test_paste_equals_pillow(channels):
    dev = _dev()
    dst, src, mask = R.paste_input(channels)
    assert (mask[0] == 0).all() and (mask[1] == 255).all()
    pinned = _golden()['paste/%d' % channels]
    for k, (xy, _) in enumerate(R.PASTE_CASES):
        for masked in (0, 1):
            want = R.paste(dst, src, xy, mask if masked else None)
            assert (want == pinned[k, masked]).all()
            d = _T(dst, dev)
            assert compose.paste(d, _T(src, dev), xy, _T(mask, dev) if masked else None) is d
            assert _eq(d, want), (xy, masked)
    d = _T(dst, dev)
    compose.paste(d, src, (50, 0), mask)                                     # a box outside the destination pastes nothing
    assert _eq(d, dst)


def _placement(dtype):
    """Three planes with two instances placed, and a third alpha about to be placed past the right edge."""
    key = ('placement', dtype)
    if key not in _REF:
        _, a0 = R.person(30, 26, (1, 1, 24, 28), 0)
        _, a1 = R.person(33, 40, (0, 0, 40, 33), 1)
        fg2, a2 = R.person(28, 60, (0, 0, 60, 28), 2)
        planes = np.zeros((3, 48, 67), dtype)
        _, _, planes = R.commit(None, planes, None, a0, (3, 10), 0)
        _, _, planes = R.commit(None, planes, None, a1, (15, 2), 1)
        _REF[key] = (planes, fg2, a2, (10, 17))
    return _REF[key]


@pytest.mark.parametrize('dtype', (np.float32, np.float64))
def test_try_place_areas(dtype):
    dev = _dev()
    planes, _, a, xy = _placement(dtype)
    want_new, want_old, want_a = R.place_areas(planes, a, xy, 2, dtype)
    p = _T(planes, dev)
    new, old, area = compose.try_place(p, a, xy, 2, torch.from_numpy(planes).dtype)
    assert _eq(p, planes)                                                    # writes nothing
    np.testing.assert_allclose(new, want_new, rtol=1e-12, atol=0)
    np.testing.assert_allclose(old, want_old, rtol=1e-12, atol=0)
    np.testing.assert_allclose(area, want_a, rtol=1e-12, atol=0)
    assert (want_new < want_old).all() and want_a > 0
    new0, old0, _ = compose.try_place(p, a, xy, 0)
    assert new0.size == 0 and old0.size == 0


@pytest.mark.parametrize('dtype', (np.float32, np.float64))
def test_commit_and_planes_u8_bit_for_bit(dtype):
    dev = _dev()
    planes, fg, a, xy = _placement(dtype)
    image = R.background(2, (48, 67))
    want_image, want_canvas, want_planes = R.commit(image, planes, fg, a, xy, 2)
    p, im = _T(planes, dev), _T(image, dev)
    canvas = torch.full((48, 67, 3), 9, dtype=torch.uint8, device=dev)
    compose.commit(im, canvas, p, fg, a, xy, 2)
    assert _eq(im, want_image) and _eq(canvas, want_canvas)
    assert _eq(p.view(torch.int32 if dtype == np.float32 else torch.int64), want_planes.view(np.int32 if dtype == np.float32 else np.int64))
    u8, flags = compose.planes_u8(p)
    want_u8, want_flags = R.planes_u8(want_planes)
    assert _eq(u8, want_u8) and flags.cpu().numpy().astype(bool).tolist() == want_flags.tolist()
    p2 = _T(planes, dev)                                                     # planes only: no image, no canvas, no foreground
    compose.commit(None, None, p2, None, a, xy, 2)
    assert torch.equal(p2, p)
    z, zf = compose.planes_u8(torch.zeros((2, 5, 7), dtype=p.dtype, device=dev))
    assert int(z.max()) == 0 and zf.cpu().tolist() == [0, 0]


def test_alpha_box():
    dev = _dev()
    for box in ((5, 3, 18, 34), (0, 0, 72, 40), (71, 39, 1, 1)):
        _, a = R.person(40, 72, box, 0)
        a[box[1], box[0]] = a[box[1] + box[3] - 1, box[0] + box[2] - 1] = 1      # the corners of the box, at the smallest non-zero value
        assert compose.alpha_box(_T(a, dev)) == R.alpha_box(a) == box
    with pytest.raises(ValueError):
        compose.alpha_box(torch.zeros((9, 11), dtype=torch.uint8, device=dev))


def _history_rows(history):
    rows = []
    for i, tries in enumerate(history):
        rows.extend((i, x, y, int(ok)) for x, y, ok in tries)
        if not tries:
            rows.append((i, -1, -1, 0))
    return np.array(rows, np.int32).reshape(-1, 4)


@pytest.mark.parametrize('run', range(5))
def test_synthesize_image_equals_the_pillow_run(run):
    dev = _dev()
    g = _golden()
    name, seed = str(g['image/%d/name' % run]), int(g['image/%d/seed' % run])
    fgs, alphas, bg = R.image_inputs(name)
    want = R.synthesize_image(seed, fgs, alphas, bg)
    random = np.random.RandomState(seed)
    got = compose.synthesize_image(seed, fgs, alphas, bg, random=random, device=dev)
    assert int(random.randint(0, 2 ** 31 - 1)) == int(g['image/%d/next' % run])   # the state's position after the run
    if bool(g['image/%d/none' % run]):
        assert got is None and want is None
        return
    assert (_history_rows(got['history']) == g['image/%d/history' % run]).all()
    assert got['history'] == want['history']
    for key in ('image', 'alphas', 'fgs'):
        assert _eq(got[key], g['image/%d/%s' % (run, key)]), key
        assert (want[key] == g['image/%d/%s' % (run, key)]).all(), key
    assert _eq(got['bg'], bg)


def test_synthesize_image_seeds_its_own_state_and_jpeg_equals_the_chained_restatement():
    dev = _dev()
    g = _golden()
    seed = int(g['image/0/seed'])
    fgs, alphas, bg = R.image_inputs(str(g['image/0/name']))
    got = compose.synthesize_image(seed, fgs, alphas, bg, jpeg=True, device=dev)
    want = R.synthesize_image(seed, fgs, alphas, bg)
    jpeg = lambda x: np.asarray(P.jpeg_roundtrip(x, 75)).astype(np.uint8)
    assert _eq(got['image'], jpeg(want['image'])) and _eq(got['bg'], jpeg(bg))
    assert _eq(got['fgs'], np.stack([jpeg(f) for f in want['fgs']]))
    assert _eq(got['alphas'], g['image/0/alphas'])


@pytest.mark.parametrize('level', R.VIDEO_LEVELS)
def test_video_frame_equals_the_pillow_frame(level):
    dev = _dev()
    g = _golden()
    fgrs, alphas, bg, boxes = R.video_inputs(level)
    rs = np.random.RandomState(int(g['video/%s/seed' % level]))
    plan = compose.plan_video(rs, level, bg.shape[:2], boxes, n_bg_frames=7)
    assert int(rs.randint(0, 2 ** 31 - 1)) == int(g['video/%s/next' % level])
    assert (np.array(plan['placed'], np.int32) == g['video/%s/placed' % level]).all() and plan['start_bg_frame'] == int(g['video/%s/start' % level])
    frame, planes, most, abort = compose.video_frame(bg, fgrs, alphas, plan, level, device=dev)
    w_frame, w_planes, w_occ, w_most, w_abort = R.video_frame(bg, fgrs, alphas, plan, level)
    assert not abort and not w_abort
    assert _eq(frame, g['video/%s/frame' % level]) and (w_frame == g['video/%s/frame' % level]).all()
    assert _eq(planes.view(torch.int64), w_planes.view(np.int64))            # the fp64 planes bit for bit
    assert (w_planes[:, ::7, ::5] == g['video/%s/planes_f64' % level]).all()
    assert _eq(compose.planes_u8(planes)[0], g['video/%s/planes' % level])
    # most = 1 - new / old: the areas agree to 1e-12 relative (the summation orders differ), and the difference from 1 amplifies that by
    # 1 / most; the fixtures' values are above 0.08 (the generator keeps them above 0.06), so 1e-12 / 0.06 < 2e-11, inside 1e-9
    assert float(g['video/%s/max_occluded' % level]) > 0.06
    np.testing.assert_allclose(most, float(g['video/%s/max_occluded' % level]), rtol=1e-9)
    assert most == pytest.approx(w_most, rel=1e-9)


def test_video_frame_aborts_where_the_tool_drops_the_clip():
    dev = _dev()
    fgrs, alphas, bg, boxes = R.video_inputs('medium')
    plan = {'boxes': boxes, 'placed': [(5, 12, 24, 36), (8, 10, 25, 38), (40, 20, 30, 28)]}     # the second instance covers the first
    _, _, w_occ, w_most, w_abort = R.video_frame(bg, fgrs, alphas, plan, 'medium')
    assert w_abort and w_occ[-1] > 0.31
    frame, planes, most, abort = compose.video_frame(bg, fgrs, alphas, plan, 'medium', device=dev)
    assert abort and frame is None and planes is None and most == pytest.approx(w_most, rel=1e-9)


def test_graph_capture_of_resize_and_commit_follows_new_pixels_and_rewritten_tables():
    dev = _dev()
    faulthandler.dump_traceback_later(120, exit=True)                      # the test's own time limit: a hung capture or replay ends the process
    try:
        (h, w), (oh, ow) = (40, 72), (30, 41)
        fg0, a0 = R.person(h, w, (0, 0, w, h), 0)
        fg1, a1 = R.person(h, w, (4, 2, 60, 36), 3)
        xy = (20, 9)
        image0 = R.background(1)
        sf, sa = _T(fg0, dev), _T(a0, dev)
        image = _T(image0, dev)
        canvas = torch.zeros((48, 64, 3), dtype=torch.uint8, device=dev)
        planes = torch.zeros((2, 48, 64), dtype=torch.float32, device=dev)
        planes0 = np.zeros((2, 48, 64), np.float32)
        planes0[0, 5:30, 10:50] = 0.5
        tables = compose.ResizeTables((w, h), (ow, oh), 'bicubic').to(dev)
        both = {name: compose.ResizeTables((w, h), (ow, oh), name) for name in R.FILTERS}

        def step():
            f = compose.pil_resize(sf, (ow, oh), tables=tables)
            a = compose.pil_resize(sa, (ow, oh), tables=tables)
            compose.commit(image, canvas, planes, f, a, xy, 1)

        planes.copy_(_T(planes0, dev))
        step()                                                              # warm-up off the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        for name, fg, a in (('bilinear', fg1, a1), ('bicubic', fg1, a1), ('bilinear', fg0, a0)):
            # bilinear taps written into the bicubic tables' rows: the launch keeps its shape, the contents are new
            assert both[name].x.shape[1] <= tables.x.shape[1] and both[name].y.shape[1] <= tables.y.shape[1]
            for dst, src in ((tables.x, both[name].x), (tables.y, both[name].y)):
                dst.zero_()
                dst[:, :src.shape[1]].copy_(_T(src, dev))
            sf.copy_(_T(fg, dev)); sa.copy_(_T(a, dev))
            image.copy_(_T(image0, dev)); planes.copy_(_T(planes0, dev))
            g.replay()
            torch.cuda.synchronize()
            rf, ra = R.resize(fg, (ow, oh), name), R.resize(a, (ow, oh), name)
            w_image, w_canvas, w_planes = R.commit(image0, planes0, rf, ra, xy, 1)
            assert _eq(image, w_image) and _eq(canvas, w_canvas) and _eq(planes.view(torch.int32), w_planes.view(np.int32)), name
        del g
    finally:
        faulthandler.cancel_dump_traceback_later()
