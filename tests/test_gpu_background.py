"""The background chain on the device (csrc/background.hip, maggie_amd.utils.background): the window of the blurred background, the histograms,
the tone curves, the composite, the driver, a graph capture and the errors, against the NumPy restatement (tests/background_restatement.py,
which tests/test_background_cpu.py holds against scipy and against the literal np.unique / np.interp and float32 / float64 expressions) and
the fixture (tests/golden/background_pinned.npz). Integer work, IEEE fp64 divisions and uncontracted fp32 / fp64 products and sums: every
comparison is exact."""
import faulthandler
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import background_restatement as R                                    # noqa: E402
import crop_restatement as C                                          # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.hip import c_int, c_long                              # noqa: E402
from maggie_amd.utils import background as B                          # noqa: E402
from maggie_amd.utils import crop                                     # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor            # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_background_golden as G                                    # noqa: E402

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


def _unaligned(t):
    """The same tensor at a base one byte past an allocation."""
    flat = torch.cat([torch.zeros(1, dtype=t.dtype, device=t.device), t.reshape(-1)])[1:]
    assert flat.data_ptr() % 4 != 0
    return flat.view(t.shape)


def _blurred(key, bg, pair):
    """The restated blur of a whole background, computed once and left unchanged."""
    if (key, pair) not in _REF:
        _REF[(key, pair)] = bg if pair is None else R.blur(bg, R.taps(*pair))
    return _REF[(key, pair)]


# ---- the window --------------------------------------------------------------------------------------------------------------------------------------
BG_40 = R.image(40, 45, 1, 'noise')


@pytest.mark.parametrize('pair', R.PAIRS, ids=lambda p: 'ks%d_s%s' % p)
def test_window_of_every_pair_in_every_corner(pair):
    """A 40 x 45 background, windows of 13 x 17 in the four corners (the halo reflects on two sides each) and in the middle."""
    dev = _dev()
    full = _blurred('bg40', BG_40, pair)
    bg = _T(BG_40, dev)
    taps = B.gaussian_taps(*pair)
    for k, (x, y) in enumerate(((0, 0), (45 - 17, 0), (0, 40 - 13), (45 - 17, 40 - 13), (11, 9))):
        d = B.BackgroundDraws(taps, x, y, 13, 17)
        got = B.blur_crop(bg, d.to(dev) if k % 2 else d)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (13, 17, 3)
        assert _eq(got, full[y:y + 13, x:x + 17]), (x, y)


def test_window_of_a_background_smaller_than_the_reach():
    """5 x 7 under ks = 25: every side is reflected more than once."""
    dev = _dev()
    bg = R.image(5, 7, 2, 'noise')
    for pair in ((25, 5.0), (25, 1.0), (15, 3.0)):
        full = R.blur(bg, R.taps(*pair))
        for x, y, h, w in ((0, 0, 5, 7), (2, 1, 3, 4), (6, 4, 1, 1)):
            assert _eq(B.blur_crop(bg, B.BackgroundDraws(B.gaussian_taps(*pair), x, y, h, w), device=dev), full[y:y + h, x:x + w]), (pair, x, y)


def test_window_that_crosses_tiles_both_ways():
    """33 x 65 out of 70 x 131: three tile rows, two tile columns, both with a partial last tile; white fills the 16-bit sums."""
    dev = _dev()
    assert 33 > 2 * B.TILE_ROWS and 65 > B.TILE_COLS
    bg = R.image(70, 131, 3, 'ramp')
    for pair in ((25, 3.0), (5, 1.0)):
        full = _blurred('bg70', bg, pair)
        for x, y in ((66, 37), (0, 0), (33, 18)):
            assert _eq(B.blur_crop(bg, B.BackgroundDraws(B.gaussian_taps(*pair), x, y, 33, 65), device=dev), full[y:y + 33, x:x + 65]), (pair, x, y)
    white = np.full((70, 131, 3), 255, np.uint8)
    assert _eq(B.blur_crop(white, B.BackgroundDraws(B.gaussian_taps(25, 5.0), 10, 10, 33, 65), device=dev), white[:33, :65])


def test_ks1_and_the_plain_copy():
    dev = _dev()
    bg = R.image(40, 44, 4, 'noise')                                        # rows of whole dwords: the wide loads
    for taps in (B.gaussian_taps(1, 1.0), None):
        for x, y, h, w in ((3, 5, 20, 30), (0, 0, 40, 44), (43, 39, 1, 1)):
            assert _eq(B.blur_crop(bg, B.BackgroundDraws(taps, x, y, h, w), device=dev), bg[y:y + h, x:x + w])


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_window_on_unaligned_bases(offset):
    """Rows of whole dwords (bw = 44) on a base that is not one; the output `offset` bytes into an allocation, nothing written around it."""
    dev = _dev()
    bg = R.image(40, 44, 4, 'noise')
    full = _blurred('bg44', bg, (15, 1.5))
    d = B.BackgroundDraws(B.gaussian_taps(15, 1.5), 5, 3, 30, 32)           # 96-byte rows: 16-byte stores when the base allows
    want = full[3:33, 5:37]
    assert _eq(B.blur_crop(_unaligned(_T(bg, dev)), d), want)
    out = torch.full((want.size + 32,), 7, dtype=torch.uint8, device=dev)
    dbg, dwin = _T(bg, dev), _T(d.win, dev)                                 # named: both live until the launch has run
    hip.call('mg_bg_blur_crop', hip.ptr(dbg), c_int(40), c_int(44), hip.ptr(dwin), hip.ctypes.c_void_p(out.data_ptr() + offset),
             c_int(30), c_int(32), hip.stream())
    torch.cuda.synchronize()
    assert _eq(out[offset:offset + want.size], want.reshape(-1))
    assert (out[:offset] == 7).all() and (out[offset + want.size:] == 7).all()


def test_a_window_table_outside_its_range_is_clamped():
    dev = _dev()
    bg = R.image(40, 45, 1, 'noise')
    wild = np.zeros(B.WIN_TABLE, np.int32)
    wild[:4] = 40, 1000, -7, 99
    wild[4:] = np.random.default_rng(3).integers(-5, 12, B.WIN_TABLE - 4)   # taps below zero clamp to 0; the sums stay below 2^16
    assert np.clip(wild[4:29], 0, 256).sum() * 255 < 65536
    d = B.BackgroundDraws(None, 0, 0, 13, 17, win=_T(wild, dev))
    assert _eq(B.blur_crop(bg, d, device=dev), R.clamped_window(bg, wild, 13, 17))


# ---- the histograms ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pixels', [1, 63, 64, 65, 4099])
def test_histograms_equal_bincount(pixels):
    dev = _dev()
    x = np.random.default_rng(pixels).integers(0, 256, (1, pixels, 3), dtype=np.uint8)
    got = B.histograms(_T(x, dev))
    assert tuple(got.shape) == (3, 256) and got.dtype == torch.int32 and got.is_cuda
    assert _eq(got, R.counts_of(x).astype(np.int32))
    assert _eq(B.histograms(_unaligned(_T(x, dev))), R.counts_of(x).astype(np.int32))


def test_histograms_of_a_clip_a_constant_image_and_runs():
    dev = _dev()
    clip = R.clip(3, 37, 41, 6)
    assert _eq(B.histograms(clip, device=dev), R.counts_of(clip).astype(np.int32))
    const = np.empty((2, 64, 67, 3), np.uint8)
    const[...] = (7, 7, 250)                                                # every lane of every wave hits one bin per channel
    assert _eq(B.histograms(const, device=dev), R.counts_of(const).astype(np.int32))
    runs = np.repeat(np.random.default_rng(2).integers(0, 256, (1, 50, 9, 3), dtype=np.uint8), 7, axis=2)    # runs of 7 cross the groups of 16
    assert _eq(B.histograms(runs, device=dev), R.counts_of(runs).astype(np.int32))
    acc = torch.zeros((3, 256), dtype=torch.int32, device=dev)              # the C entry accumulates
    dclip = _T(clip, dev)
    for _ in range(2):
        hip.call('mg_bg_hist', hip.ptr(dclip), c_long(clip.size // 3), hip.ptr(acc), hip.stream())
    assert _eq(acc, 2 * R.counts_of(clip).astype(np.int32))


# ---- the curves --------------------------------------------------------------------------------------------------------------------------------------
def _three_channels(s, t):
    """(1, n, 3) frames whose channels are s, a rotation of s, and s reversed (the three channels are independent)."""
    return np.stack([s, np.roll(s, 5), s[::-1]], axis=-1)[None], np.stack([t, np.roll(t, 3), t[::-1]], axis=-1)[None]


@pytest.mark.parametrize('name', sorted(R.curve_cases()))
def test_curves_equal_the_restatement(name):
    """One value on either side, equal sides (the exact-hit branch), a source wholly brighter and wholly darker (the clamps), disjoint
    ranges; ratios 0.0 and 0.4999 among others; both directions; host and device draws. The whole (2, 3, 256) table is compared."""
    dev = _dev()
    s, t = R.curve_cases()[name]
    fg, bg = _three_channels(s, t)
    dfg, dbg = _T(fg, dev), _T(bg, dev)
    for k, ratio in enumerate((0.0, 0.4999, 0.3141592653589793)):
        for match_bg in (False, True):
            h = B.HistDraws(ratio, match_bg)
            got = B.match_luts(dfg, dbg, h.to(dev) if k % 2 else h)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, 256)
            assert _eq(got, R.luts(fg, bg, (ratio, match_bg))), (ratio, match_bg)


def test_curves_of_frames_and_of_a_tiled_background():
    dev = _dev()
    fg, win = R.clip(3, 17, 19, 3), R.image(17, 19, 5, 'band')
    for hist in ((0.37, False), (0.2, True)):
        want = R.luts(fg, win, hist)
        assert _eq(B.match_luts(fg, win, B.HistDraws(*hist), device=dev), want)
        assert _eq(B.match_luts(fg, np.tile(win, (3, 1, 1, 1)), B.HistDraws(*hist), device=dev), want)      # the reference's tiled background
    ident = B.match_luts(fg, win, None, device=dev)
    assert _eq(ident, R.luts(fg, win, None)) and ident.data_ptr() == B.match_luts(_T(fg, dev), win, None).data_ptr()      # no launch: the shared table


# ---- the composite -----------------------------------------------------------------------------------------------------------------------------------
def test_composite_of_all_triples_in_one_launch():
    """All 256^3 (fg, bg, a) triples as one 4096 x 4096 frame whose three channels hold the same triple: row = a * 16 + fg // 16,
    column = (fg % 16) * 256 + bg. The expected frame comes from the literal float32 / float64 expression, row block by row block."""
    dev = _dev()
    i = torch.arange(4096, device=dev)
    fgv = ((i[:, None] % 16) * 16 + i[None, :] // 256).to(torch.uint8)
    bgv = (i[None, :] % 256).to(torch.uint8).expand(4096, 4096)
    av = (i[:, None] // 16).to(torch.uint8).expand(4096, 4096).contiguous()
    fg = fgv[..., None].expand(4096, 4096, 3).contiguous()
    bg = bgv[..., None].expand(4096, 4096, 3).contiguous()
    got = B.compose(fg, av, bg)
    assert tuple(got.shape) == (4096, 4096, 3)
    assert torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 0], got[..., 2])
    a = (np.arange(4096) // 16).astype(np.uint8)
    f = ((np.arange(4096)[:, None] % 16) * 16 + np.arange(4096)[None, :] // 256).astype(np.uint8)
    b = np.broadcast_to((np.arange(4096) % 256).astype(np.uint8), (4096, 4096))
    want = R.compose_literal(f[..., None], np.broadcast_to(a[:, None], (4096, 4096)), b[..., None])[..., 0]
    assert len(np.unique(f.astype(np.int64) * 65536 + b.astype(np.int64) * 256 + a[:, None])) == 256 ** 3        # every triple is there
    assert _eq(got[..., 0], want)


@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (17, 67)], ids=lambda s: '%dx%d' % s)
def test_composite_shapes_backgrounds_curves_and_outputs(shape):
    dev = _dev()
    h, w = shape
    T = 3
    fg, a = R.clip(T, h, w, 7), R.alphas(T, h, w, 8)
    shared, per_frame = R.image(h, w, 9, 'band'), R.clip(T, h, w, 10, 'noise')
    luts = R.luts(fg, shared, (0.41, False))
    luts[1] = R.luts(fg, shared, (0.3, True))[1]                            # curves on both sides at once
    for bg in (shared, per_frame):
        assert _eq(B.compose(fg, a, bg, device=dev), R.compose_literal(fg, a, bg))
        f2, b2 = R.apply_luts(fg, luts[0]), R.apply_luts(bg, luts[1])
        want = R.compose_literal(f2, a, b2)
        assert _eq(B.compose(_T(fg, dev), _T(a, dev), bg, luts=luts), want)
        out, fo, bo = B.compose(fg, a, _T(bg, dev), luts=_T(luts, dev), return_fg_bg=True, device=dev)
        assert _eq(out, want) and _eq(fo, f2) and _eq(bo, b2) and tuple(bo.shape) == bg.shape
        out, fo, bo = B.compose(_unaligned(_T(fg, dev)), _unaligned(_T(a, dev)), _unaligned(_T(bg, dev)), luts=luts, return_fg_bg=True)
        assert _eq(out, want) and _eq(fo, f2) and _eq(bo, b2)
    one = B.compose(fg[0], a[0], shared, device=dev)                        # a single frame without a leading axis
    assert tuple(one.shape) == (h, w, 3) and _eq(one, R.compose_literal(fg[:1], a[:1], shared)[0])


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------------------
def test_random_background_on_seeded_draws_equals_the_restated_chain():
    """Seeds until every fired / unfired combination of the two steps and both directions of the matching came up."""
    dev = _dev()
    T, h, w = 2, 21, 35
    fg, a, bg = R.clip(T, h, w, 11), R.alphas(T, h, w, 12), R.image(50, 71, 13, 'band')
    dfg, da, dbg = _T(fg, dev), _T(a, dev), _T(bg, dev)
    seen = set()
    for seed in range(40):
        rs, rs2 = np.random.RandomState(seed), np.random.RandomState(seed)
        bd, hd = B.draw_window(rs, bg.shape[:2], (h, w)), B.draw_histmatch(rs, 0.6 if seed % 4 else 1.0)
        if seed % 4 == 0 and hd is not None:
            hd = B.HistDraws(hd.ratio, True)                                # the 5 % direction
        blur, x, y = R.window_calls(rs2, bg.shape[:2], (h, w))
        hist = None if hd is None else (hd.ratio, hd.match_bg)
        key = (blur is not None, None if hist is None else hist[1])
        if key in seen and len(seen) < 6:
            continue
        seen.add(key)
        want, f2, b2 = R.chain(fg, a, bg, blur, x, y, hist)
        on_dev = seed % 2 == 1
        got, fo, bo = B.random_background(dfg, da, dbg, bd.to(dev) if on_dev else bd, hd.to(dev) if on_dev and hd else hd, return_fg_bg=True)
        assert _eq(got, want) and _eq(fo, f2) and _eq(bo, b2), (seed, key)
        assert _eq(B.random_background(fg, a, bg, bd, hd, device=dev), want)
        if len(seen) == 6:
            break
    assert len(seen) == 6


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_chain_equals_the_fixture(name):
    dev = _dev()
    g = load_golden('background_pinned.npz')
    ks, x, y, fired, match_bg = (int(v) for v in g[name + '.draws'])
    sigma, ratio = (float(v) for v in g[name + '.floats'])
    T, h, w = g[name + '.alphas'].shape
    bd = B.BackgroundDraws(B.gaussian_taps(ks, sigma) if ks else None, x, y, h, w)
    hd = B.HistDraws(ratio, bool(match_bg)) if fired else None
    out, fo, bo = B.random_background(g[name + '.fg'], g[name + '.alphas'], g[name + '.bg'], bd, hd, return_fg_bg=True, device=dev)
    assert _eq(out, g[name + '.frames']) and _eq(fo, g[name + '.fg_out']) and _eq(bo, g[name + '.bg_out'])
    win = B.blur_crop(g[name + '.bg'], bd, device=dev)
    assert _eq(B.match_luts(g[name + '.fg'], win, hd, device=dev), g[name + '.luts'])


def test_chain_feeds_the_training_item():
    """random_background -> DevicePreprocessor.train_item equals train_item on the restated frames."""
    dev = _dev()
    name = 'mean_vs_any'
    c = C.GOLDEN[name]
    frames, alphas, _ = C.golden_inputs(name)
    T, n, h, w = c['T'], c['n'], c['h'], c['w']
    alphas = alphas.reshape(T, n, h, w)
    union = alphas.max(axis=1)
    bg = R.image(h + 30, w + 50, 21, 'ramp')
    rs = np.random.RandomState(4)
    bd = B.draw_window(rs, bg.shape[:2], (h, w), blur_p=1.0)
    hd = B.draw_histmatch(rs, 1.0)
    assert bd.blurred and hd is not None
    win = R.window(bg, bd.taps.astype(np.int64), bd.x, bd.y, h, w)
    f2, tiled = R.histmatch_literal(frames, np.tile(win, (T, 1, 1, 1)), hd.ratio, hd.match_bg)
    want = R.compose_literal(f2, union, tiled[0])
    got = B.random_background(frames, union, bg, bd, hd, device=dev)
    assert _eq(got, want)
    pre = DevicePreprocessor(max_inst=6, device=dev)
    cd = crop.draw_on_device(np.random.RandomState(c['rs_seed']), alphas.reshape(T * n, h, w), c['crop'], c['pp'], c['fp']).to(dev)
    da = _T(alphas, dev)
    item = pre.train_item(got, da, da, cd, [4, 1][:n], transition=(3, 2))
    ref = pre.train_item(_T(want, dev), da, da, cd, [4, 1][:n], transition=(3, 2))
    assert list(item) == list(ref) and all(torch.equal(item[k], ref[k]) for k in ref)
    plain = pre.train_item(_T(frames, dev), da, da, cd, [4, 1][:n], transition=(3, 2))
    assert not torch.equal(item['image'], plain['image'])


# ---- a graph -----------------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_the_chain_with_resident_draws():
    dev = _dev()
    faulthandler.dump_traceback_later(120, exit=True)                      # the test's own time limit: a hung capture or replay ends the process
    try:
        T, h, w = 2, 21, 35
        fg, a, bg = _T(R.clip(T, h, w, 11), dev), _T(R.alphas(T, h, w, 12), dev), _T(R.image(50, 71, 13, 'band'), dev)
        bd = B.BackgroundDraws(B.gaussian_taps(15, 3.0), 9, 4, h, w).to(dev)
        hd = B.HistDraws(0.33, False).to(dev)
        assert bd.on_device and hd.on_device
        eager = B.random_background(fg, a, bg, bd, hd).clone()              # also the warm-up off the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = B.random_background(fg, a, bg, bd, hd)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        del g
    finally:
        faulthandler.cancel_dump_traceback_later()


# ---- the errors --------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched():
    dev = _dev()
    lib, st = hip.lib(), hip.stream()
    bg = torch.zeros((10, 12, 3), dtype=torch.uint8, device=dev)
    win = _T(B.BackgroundDraws(None, 0, 0, 4, 5).win, dev)
    out = torch.full((4096,), 7, dtype=torch.uint8, device=dev)
    counts = torch.full((3, 256), 7, dtype=torch.int32, device=dev)
    wt = torch.zeros((256, 2), dtype=torch.float64, device=dev)
    draw = torch.zeros(4, dtype=torch.float32, device=dev)
    window = lambda b, bh, bw, t, o, h, w: lib.mg_bg_blur_crop(hip.ptr(b), c_int(bh), c_int(bw), hip.ptr(t), hip.ptr(o), c_int(h), c_int(w), st)   # noqa: E731
    assert window(bg, 10, 12, win, out, 11, 5) == -2 and window(bg, 10, 12, win, out, 4, 13) == -2 and window(bg, 10, 12, win, out, 0, 5) == -2
    assert window(None, 10, 12, win, out, 4, 5) == -2 and window(bg, 10, 12, None, out, 4, 5) == -2 and window(bg, 10, 12, win, None, 4, 5) == -2
    assert window(bg, 10, 32768, win, out, 4, 5) == -2 and window(bg, 10, 12, win, bg, 4, 5) == -2
    hist = lambda x, n, c: lib.mg_bg_hist(hip.ptr(x), c_long(n), hip.ptr(c), st)   # noqa: E731
    assert hist(bg, 0, counts) == -2 and hist(bg, 2 ** 31, counts) == -2 and hist(None, 4, counts) == -2 and hist(bg, 4, None) == -2
    assert lib.mg_bg_match_lut(hip.ptr(counts), None, hip.ptr(draw), hip.ptr(out), st) == -2
    assert lib.mg_bg_match_lut(hip.ptr(counts), hip.ptr(counts), None, hip.ptr(out), st) == -2
    comp = lambda f, a, b, bn, n, h, w, t, o: lib.mg_bg_compose(hip.ptr(f), hip.ptr(a), hip.ptr(b), c_long(bn), c_long(n), c_int(h), c_int(w), None,   # noqa: E731
                                                                hip.ptr(t), hip.ptr(o), None, None, st)
    assert comp(bg, bg, bg, 2, 3, 2, 2, wt, out) == -2 and comp(bg, bg, bg, 1, 1, 0, 2, wt, out) == -2 and comp(bg, bg, bg, 1, 1, 2, 2, None, out) == -2
    assert comp(None, bg, bg, 1, 1, 2, 2, wt, out) == -2 and comp(bg, bg, bg, 1, 70000, 2, 2, wt, out) == -3 and comp(bg, bg, bg, 1, 0, 2, 2, wt, out) == 0
    fg, a = np.zeros((2, 4, 5, 3), np.uint8), np.zeros((2, 4, 5), np.uint8)
    d = B.BackgroundDraws(B.gaussian_taps(5, 1.0), 3, 4, 4, 5)
    for call, err in ((lambda: B.blur_crop(bg.to(torch.int16), d), TypeError), (lambda: B.blur_crop(bg, B.BackgroundDraws(None, 8, 0, 4, 5)), ValueError),
                      (lambda: B.random_background(fg, a, bg, B.BackgroundDraws(None, 0, 0, 4, 6), None), ValueError),
                      (lambda: B.compose(fg, a, bg), ValueError), (lambda: B.histograms(a), ValueError),
                      (lambda: B.match_luts(fg, bg, 0.3), TypeError), (lambda: B.gaussian_taps(27, 1.0), ValueError)):
        with pytest.raises(err):
            call()
    torch.cuda.synchronize()
    assert (out == 7).all() and (counts == 7).all() and not bg.any()
