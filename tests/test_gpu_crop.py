"""The training crop on the device (csrc/crop.hip, maggie_amd.utils.crop, DevicePreprocessor.train_item): the box, the hit test, the gather with
its flip, both epilogues and the tone table, the pad-and-resize branch, against the NumPy restatement (tests/crop_restatement.py), the
pre-existing kernels (normalize_frames, DevicePreprocessor.__call__) and the reference's own transforms (tests/golden/crop_pinned.npz).
Integer work and IEEE divisions: every comparison is exact."""
import faulthandler
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import crop_restatement as C                                          # noqa: E402
import geometry_restatement as R                                      # noqa: E402
import maskgen_restatement as M                                       # noqa: E402
from helpers import load_golden, unpack_bits                         # noqa: E402
from maggie_amd.utils import crop                                     # noqa: E402
from maggie_amd.utils import maskgen as MG                            # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor, normalize_frames      # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(C.GOLDEN)
CROP_CASES = [n for n in CASES if C.GOLDEN[n]['pp'] < 1.0]
PAD_CASES = [n for n in CASES if C.GOLDEN[n]['pp'] == 1.0]
WIDTHS = (1, 3, 4, 15, 16, 17, 64)
LUT = np.random.default_rng(17).integers(0, 256, (3, 256), dtype=np.uint8)
_CACHE = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq(out, ref):
    return torch.equal(out.cpu(), torch.from_numpy(np.ascontiguousarray(ref)))


def _case(name):
    """Inputs and the restated result of a case, computed once and left unchanged."""
    if name not in _CACHE:
        _CACHE[name] = (C.GOLDEN[name],) + tuple(C.golden_inputs(name)) + (C.golden_run(name)[0],)
    return _CACHE[name]


def _toned(frames):
    return np.stack([LUT[c][frames[..., c]] for c in range(3)], -1)


def _crop_draws(H, W, ch, cw, x0, y0, flip):
    return crop.CropDraws('crop', H, W, (ch, cw), flip, ch, cw, window=np.asarray([x0, y0, int(flip)], np.int32), pairs=1)


# ---- the box and the hit test ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_bbox_and_hits_equal_the_restatement(name):
    dev = _dev()
    c, _, alphas, _, r = _case(name)
    P, H, W = alphas.shape
    ch, cw = c['crop']
    x = _T(alphas, dev)
    assert crop.bbox(x).cpu().tolist() == list(C.bbox(alphas))
    offset = torch.cat([torch.zeros_like(x[:1]), x])[1:]                     # the same planes at a base that is 16-byte aligned only by chance
    assert crop.bbox(offset).cpu().tolist() == list(C.bbox(alphas))
    windows = [r['window'] or (0, 0), (0, 0), (W - cw, H - ch)]
    rs = np.random.RandomState(3)
    windows += [(int(rs.randint(0, W - cw + 1)), int(rs.randint(0, H - ch + 1))) for _ in range(3)]
    for ws in (windows[:3], windows[3:], windows[:1]):
        assert crop.window_hits(x, ws, c['crop']).cpu().tolist() == C.hits(alphas, ws, c['crop']), ws
        assert crop.window_hits(offset, ws, c['crop']).cpu().tolist() == C.hits(alphas, ws, c['crop']), ws
    if r['branch'] == 'crop':
        assert bool(C.hits(alphas, [r['window']], c['crop'])[0]) == bool((r['alphas'] > 127).any())


@pytest.mark.parametrize('P', [1, 30])
@pytest.mark.parametrize('H,W', [(96, 160), (99, 157)])
def test_bbox_of_a_single_pixel_in_each_corner(P, H, W):
    """One qualifying pixel, everything else at exactly 127 (sum == 127 * P: not above). Three corners hold 255 in every plane; the last holds
    127 in all planes but one at 128: the sum is 127 * P + 1."""
    dev = _dev()
    for k, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        a = np.full((P, H, W), 127, np.uint8)
        if k < 3:
            a[:, y, x] = 255
        else:
            a[P // 2, y, x] = 128
        assert C.bbox(a) == (1, x, x, y, y)
        assert crop.bbox(_T(a, dev)).cpu().tolist() == [1, x, x, y, y]
        ws = [(0, 0), (W - 8, H - 8), (W - 8, 0)]
        assert crop.window_hits(_T(a, dev), ws, (8, 8)).cpu().tolist() == C.hits(a, ws, (8, 8))
    a = np.zeros((P, H, W), np.uint8)
    a[0, 5, 7] = 255                                                         # above 127 in one plane: a hit, and for P > 2 not in the box
    assert crop.bbox(_T(a, dev)).cpu().tolist() == list(C.bbox(a)) == ([1, 7, 7, 5, 5] if P == 1 else [0, W, -1, H, -1])
    assert crop.window_hits(_T(a, dev), [(0, 0), (8, 0)], (8, 8)).cpu().tolist() == [1, 0]


# ---- the gather --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cw', WIDTHS)
def test_gather_at_every_x0_and_width(cw):
    """x0 = 0 .. 17 (every alignment of the unaligned 16-byte loads), flipped and not, planes and frames, both epilogues, with and without the
    tone table; the widths cover whole chunks (16, 64), a chunk and a tail (17), tails only, and rows that are no multiple of 4."""
    dev = _dev()
    H, ch, y0, W = 9, 5, 3, cw + 19
    rng = np.random.default_rng(cw)
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    planes = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    f, a, lut = _T(frames, dev), _T(planes, dev), _T(LUT, dev)
    for x0 in range(18):
        for flip in (False, True):
            d = _crop_draws(H, W, ch, cw, x0, y0, flip).to(dev)
            want_f, want_a = C.gather(frames, (x0, y0), (ch, cw), flip), C.gather(planes, (x0, y0), (ch, cw), flip)
            gf, ga, gm = crop.apply(f, a, a, d)
            assert gf.dtype == ga.dtype == torch.uint8 and _eq(gf, want_f) and _eq(ga, want_a) and torch.equal(gm, ga), (x0, flip)
            gt, _, none = crop.apply(f, a, None, d, lut=lut)
            assert none is None and _eq(gt, _toned(want_f)), (x0, flip)
            gn, _, _ = crop.apply(f, None, None, d, normalize=True)
            assert gn.dtype == torch.float32 and _eq(gn, R.normalized(want_f)), (x0, flip)
            gn, _, _ = crop.apply(f, None, None, d, normalize=True, lut=lut)
            assert _eq(gn, R.normalized(_toned(want_f))), (x0, flip)


@pytest.mark.parametrize('name', CROP_CASES)
def test_gather_of_every_case_through_both_epilogues(name):
    dev = _dev()
    c, frames, alphas, masks, r = _case(name)
    ch, cw = c['crop']
    f, a, m = _T(frames, dev), _T(alphas, dev), _T(masks, dev)
    for flip in (False, True):
        d = _crop_draws(c['h'], c['w'], ch, cw, r['window'][0], r['window'][1], flip)
        want = [C.gather(x, r['window'], c['crop'], flip) for x in (frames, alphas, masks)]
        for lut in (None, LUT):
            wf = want[0] if lut is None else _toned(want[0])
            gf, ga, gm = crop.apply(f, a, m, d, lut=lut)
            assert _eq(gf, wf) and _eq(ga, want[1]) and _eq(gm, want[2]), (flip, lut is not None)
            gn, ga, gm = crop.apply(frames, alphas, masks, d, normalize=True, lut=lut)             # host arrays
            assert tuple(gn.shape) == (c['T'], 3, ch, cw) and _eq(ga, want[1]) and _eq(gm, want[2])
            # the normalised epilogue has the bits of the pre-existing kernel on the uint8 crop
            assert torch.equal(gn, normalize_frames(_T(wf, dev))) and _eq(gn, R.normalized(wf)), (flip, lut is not None)
            if (ch * cw) % 4 == 0:
                for fused in (True, False):                                                        # the composed form gives the same bits
                    saved, crop.FUSED_NORMALIZE = crop.FUSED_NORMALIZE, fused
                    try:
                        assert torch.equal(crop.apply(f, None, None, d, normalize=True, lut=lut)[0], gn)
                    finally:
                        crop.FUSED_NORMALIZE = saved
    if r['flip']:
        assert not _eq(crop.apply(f, None, None, _crop_draws(c['h'], c['w'], ch, cw, r['window'][0], r['window'][1], False))[0], r['frames'])


def test_gather_keeps_leading_dimensions_and_clamps_a_wild_window():
    dev = _dev()
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (2, 2, 20, 37, 3), dtype=np.uint8)
    planes = rng.integers(0, 256, (2, 2, 3, 20, 37), dtype=np.uint8)
    d = _crop_draws(20, 37, 8, 16, 1000, -5, True)                             # a device table may hold anything: clamped to (37 - 16, 0)
    gf, ga, _ = crop.apply(frames, planes, None, d)
    assert tuple(gf.shape) == (2, 2, 8, 16, 3) and tuple(ga.shape) == (2, 2, 3, 8, 16)
    assert _eq(gf, C.gather(frames.reshape(4, 20, 37, 3), (21, 0), (8, 16), True).reshape(2, 2, 8, 16, 3))
    assert _eq(ga, C.gather(planes.reshape(12, 20, 37), (21, 0), (8, 16), True).reshape(2, 2, 3, 8, 16))


# ---- the padding branch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', PAD_CASES)
def test_padresize_linear_and_nearest_with_the_flip_folded_in(name):
    dev = _dev()
    c, frames, alphas, masks, r = _case(name)
    ch, cw = c['crop']
    f, a, m = _T(frames, dev), _T(alphas, dev), _T(masks, dev)
    for flip in (False, True):
        pad_h, pad_w, oh, ow, linear, nearest = crop.pad_tables(c['h'], c['w'], c['crop'], flip)
        assert (oh, ow) == (cw, ch) and (pad_h > 0) != (pad_w > 0)
        d = crop.CropDraws('pad', c['h'], c['w'], c['crop'], flip, oh, ow, pad=(pad_h, pad_w), linear=linear, nearest=nearest)
        wf, wa = C.padresize(frames, c['crop'], flip, R.INTER_LINEAR), C.padresize(alphas, c['crop'], flip, R.INTER_LINEAR)
        wm = C.padresize(masks, c['crop'], flip, R.INTER_NEAREST)
        assert not np.array_equal(wm, C.padresize(masks, c['crop'], flip, R.INTER_LINEAR))
        gf, ga, gm = crop.apply(f, a, m, d)
        assert tuple(gf.shape) == (c['T'], oh, ow, 3) and _eq(gf, wf) and _eq(ga, wa) and _eq(gm, wm), flip
        gf, ga, gm = crop.apply(f, a, m, d.to(dev), lut=LUT)
        assert _eq(gf, _toned(wf)) and _eq(ga, wa) and _eq(gm, wm), flip                             # the border's 0 goes through the table too
        gn, _, _ = crop.apply(f, None, None, d, normalize=True)
        assert torch.equal(gn, normalize_frames(_T(wf, dev))) and _eq(gn, R.normalized(wf)), flip
        gn, _, _ = crop.apply(f, None, None, d, normalize=True, lut=LUT)
        assert _eq(gn, R.normalized(_toned(wf))), flip
        if flip == r['flip']:
            assert _eq(gf, _toned(r['frames'])) and _eq(ga, r['alphas']) and _eq(gm, r['masks'])


def test_padresize_with_ragged_rows():
    """An output whose rows are no multiple of 4 (per-element stores) from a source taller than wide by an odd amount."""
    dev = _dev()
    rng = np.random.default_rng(8)
    frames = rng.integers(1, 256, (2, 41, 30, 3), dtype=np.uint8)
    planes = rng.integers(0, 256, (3, 41, 30), dtype=np.uint8)
    for size in ((13, 22), (50, 7)):
        for flip in (False, True):
            pad_h, pad_w, oh, ow, linear, nearest = crop.pad_tables(41, 30, size, flip)
            d = crop.CropDraws('pad', 41, 30, size, flip, oh, ow, pad=(pad_h, pad_w), linear=linear, nearest=nearest)
            gf, ga, gm = crop.apply(frames, planes, planes, d)
            assert _eq(gf, C.padresize(frames, size, flip, R.INTER_LINEAR)) and _eq(ga, C.padresize(planes, size, flip, R.INTER_LINEAR))
            assert _eq(gm, C.padresize(planes, size, flip, R.INTER_NEAREST))
            assert _eq(crop.apply(frames, None, None, d, normalize=True)[0], R.normalized(C.padresize(frames, size, flip, R.INTER_LINEAR)))


# ---- the draws on the device, and the items ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_draw_on_device_then_apply_equals_the_fixture(name):
    dev = _dev()
    d = load_golden('crop_pinned.npz')
    c, frames, alphas, masks, r = _case(name)
    rs = np.random.RandomState(c['rs_seed'])
    draws = crop.draw_on_device(rs, _T(alphas, dev), c['crop'], c['pp'], c['fp'])
    assert np.array_equal(C.state_digest(rs), d[name + '.state'])              # the generator is where the reference left it
    pad, x0, y0, pairs, flip = d[name + '.info'].tolist()[:5]
    assert (draws.branch == 'pad') == bool(pad) and draws.flip == bool(flip) and not draws.on_device
    if not pad:
        assert draws.window.tolist() == [x0, y0, flip] and draws.pairs == pairs and list(draws.box) == d[name + '.info'].tolist()[5:]
    gf, ga, gm = crop.apply(_T(frames, dev), _T(alphas, dev), _T(masks, dev), draws)
    fix_f, fix_a = R.unpack_rows(d[name + '.frames']), R.unpack_rows(d[name + '.alphas'])
    assert _eq(gf, fix_f) and _eq(ga, fix_a) and _eq(gm, unpack_bits(d[name + '.masks'], r['masks'].shape) * np.uint8(255))
    assert _eq(gf, r['frames']) and _eq(ga, r['alphas']) and _eq(gm, r['masks'])
    # host arrays give the same draws
    rs2 = np.random.RandomState(c['rs_seed'])
    again = crop.draw_on_device(rs2, alphas, c['crop'], c['pp'], c['fp'])
    assert np.array_equal(C.state_digest(rs2), d[name + '.state']) and again.branch == draws.branch
    assert pad or again.window.tolist() == draws.window.tolist()


@pytest.mark.parametrize('name', ['first_hit', 'mean_vs_any', 'clamped', 'pad_wide_odd'])
def test_train_item_equals_call_on_the_restated_crops(name):
    dev = _dev()
    c, frames, alphas, masks, r = _case(name)
    T, n = c['T'], c['n']
    oh, ow = r['alphas'].shape[-2:]
    pre = DevicePreprocessor(max_inst=6, device=dev)
    ids = [4, 1][:n]
    rs = np.random.RandomState(c['rs_seed'])
    cd = crop.draw_on_device(rs, alphas, c['crop'], c['pp'], c['fp']).to(dev)
    assert cd.on_device
    md = MG.draw_chain(np.random.RandomState(9), random.Random(9), T * n, oh, ow, from_alpha=T > 1)
    f, a, m = _T(frames, dev), _T(alphas.reshape(T, n, c['h'], c['w']), dev), _T(masks.reshape(T, n, c['h'], c['w']), dev)
    ra, rm = r['alphas'].reshape(T, n, oh, ow), r['masks'].reshape(T, n, oh, ow)
    # image training: the alphas are the masks' source (him.py:103); video: the same with GenMaskFromAlpha folded into the draws
    got = pre.train_item(f, a, a, cd, ids, transition=(3, 2), mask_draws=md)
    want = pre(_T(r['frames'], dev), _T(ra, dev), _T(ra, dev), ids, transition=(3, 2), mask_draws=md)
    assert list(got) == list(want) == ['image', 'alpha', 'mask', 'transition']
    for key in want:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
    assert _eq(got['mask'], pre(r['frames'], ra, M.chain(r['alphas'], md).reshape(T, n, oh, ow), ids)['mask'].cpu().numpy())
    # masks of their own, no chain, no transition, with the tone table
    got = pre.train_item(f, a, m, cd, ids, lut=LUT)
    want = pre(_T(_toned(r['frames']), dev), _T(ra, dev), _T(rm, dev), ids)
    assert list(got) == list(want) == ['image', 'alpha', 'mask']
    for key in want:
        assert torch.equal(got[key], want[key]), key
    assert tuple(got['image'].shape) == (T, 3, oh, ow) and tuple(got['mask'].shape) == (T, 6, oh // 8, ow // 8)


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_apply_replays_with_new_pixels_and_a_rewritten_window():
    dev = _dev()
    c, frames, alphas, masks, r = _case('first_hit')
    ch, cw = c['crop']
    other_f, other_a = R.frames_of(91, c['T'], c['h'], c['w']), C.golden_inputs('second_hit')[1].repeat(2, 0)
    faulthandler.dump_traceback_later(120, exit=True)                      # the test's own time limit: a hung capture or replay ends the process
    try:
        sf, sa = _T(frames, dev), _T(alphas, dev)
        d = _crop_draws(c['h'], c['w'], ch, cw, r['window'][0], r['window'][1], True).to(dev)
        lut = _T(LUT, dev)
        crop.apply(sf, sa, None, d, normalize=True, lut=lut)                # warm-up off the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gn, ga, _ = crop.apply(sf, sa, None, d, normalize=True, lut=lut)
        for fr, al, win in ((other_f, other_a, (7, 30, 0)), (frames, alphas, (96, 0, 1)), (other_f, alphas, (33, 32, 1))):
            sf.copy_(_T(fr, dev))
            sa.copy_(_T(al, dev))
            d.window.copy_(torch.tensor(win, dtype=torch.int32))
            g.replay()
            torch.cuda.synchronize()
            wf = _toned(C.gather(fr, win[:2], (ch, cw), bool(win[2])))
            assert _eq(gn, R.normalized(wf)) and _eq(ga, C.gather(al, win[:2], (ch, cw), bool(win[2]))), win
        del g
    finally:
        faulthandler.cancel_dump_traceback_later()
