"""The host side of device compositing (maggie_amd.utils.compose) and the restatement the device is compared with
(tests/compose_restatement.py): the restatement against the live Pillow on every case tests/test_gpu_compose.py runs and against the fixture
Pillow wrote, the generator's three conditions on its inputs, the table builder, the drivers' host parts, the constants and the order of the
errors. No GPU is needed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import compose_restatement as R                                       # noqa: E402
from helpers import GOLDEN, load_golden                               # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import compose                                  # noqa: E402

_G = {}


def _golden():
    if not _G:
        g = load_golden('compose_pinned.npz')
        _G.update({k: g[k] for k in g.files})
    return _G


def _generator():
    pytest.importorskip('PIL')
    sys.path.insert(0, GOLDEN)
    import make_compose_golden
    return make_compose_golden


# ---- the restatement, live Pillow and the fixture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', (1, 3))
@pytest.mark.parametrize('index', range(len(R.RESIZE_CASES)))
def test_resize_restatement_equals_live_pillow_and_the_fixture(index, channels):
    Image = pytest.importorskip('PIL.Image')
    (h, w), (oh, ow), crop = R.RESIZE_CASES[index]
    src = R.resize_input(index, channels)
    for name, flt in (('bicubic', Image.BICUBIC), ('bilinear', Image.BILINEAR)):
        im = Image.fromarray(src)
        live = np.array((im if crop is None else im.crop(crop)).resize((ow, oh), flt))
        got = R.resize(src, (ow, oh), name, crop)
        assert got.shape == live.shape and (got == live).all(), name
        assert (got == R.resize_unpack(_golden()['resize/%d/%s' % (channels, name)], channels)[index]).all(), name


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    shapes = [(s, o) for s, o, _ in R.RESIZE_CASES]
    for need in (((37, 53), (20, 71)), ((64, 48), (150, 13)), ((9, 9), (9, 30)), ((100, 80), (17, 23)), ((5, 7), (40, 40)), ((33, 1), (8, 5))):
        assert need in shapes
    assert any(o == (1, 1) for _, o in shapes)                                                   # output size 1
    assert {o[1] for _, o in shapes} >= {1, 3, 4, 5, 67}                                         # widths of the vector and the edge stores
    assert any(c is not None and c[0] % 2 == 1 and c[1] % 2 == 1 for _, _, c in R.RESIZE_CASES)  # a crop at an odd offset
    taps = max(int(compose.resample_tables(s[1], o[1], 'bicubic')[:, 1].max()) for s, o in shapes)
    assert taps > 64 and max(s[1] / o[1] for s, o in shapes) >= 12                               # more taps than a wave is wide
    forms = {compose.ResizeTables((s[1], s[0]), (o[1], o[0])).regime for s, o in shapes}
    assert forms == {compose.FUSED, compose.TWO_PASS}                                            # both sides of the switch point


@pytest.mark.parametrize('channels', (1, 3))
def test_paste_restatement_equals_live_pillow_and_the_fixture(channels):
    Image = pytest.importorskip('PIL.Image')
    dst, src, mask = R.paste_input(channels)
    for k, (xy, _) in enumerate(R.PASTE_CASES):
        for masked in (0, 1):
            im = Image.fromarray(dst.copy())
            im.paste(Image.fromarray(src), xy, Image.fromarray(mask) if masked else None)
            got = R.paste(dst, src, xy, mask if masked else None)
            assert (got == np.array(im)).all() and (got == _golden()['paste/%d' % channels][k, masked]).all(), (xy, masked)


def test_the_generators_conditions_and_runs_hold_today():
    """Runs the generator's own Pillow runs again: its three input conditions (asserted inside `main`'s pieces) and equality with the fixture
    and the restatement."""
    G = _generator()
    g = _golden()
    kinds = set()
    for run in range(5):
        name, seed = str(g['image/%d/name' % run]), int(g['image/%d/seed' % run])
        fgs, alphas, bg = R.image_inputs(name)
        res, history, ratios, nxt = G.pil_image_run(seed, fgs, alphas, bg)
        want = R.synthesize_image(seed, fgs, alphas, bg)
        assert G.far(ratios, (0.7,))                                                             # condition 2
        assert nxt == int(g['image/%d/next' % run]) and (G.history_array(history) == g['image/%d/history' % run]).all()
        assert (res is None) == bool(g['image/%d/none' % run]) == (want is None)
        if any(len(t) >= 2 and not t[0][2] and t[-1][2] for t in history):
            kinds.add('rejected then accepted')
        if any(len(t) == 3 and not any(ok for _, _, ok in t) for t in history):
            kinds.add('dropped')
        if res is not None and any(t == [] for t in history):
            kinds.add('empty range')
        if res is None:
            kinds.add('none')
            continue
        assert want['history'] == history and want['ratios'] == ratios
        for key in ('image', 'alphas', 'fgs'):
            assert (res[key] == g['image/%d/%s' % (run, key)]).all() and (want[key] == res[key]).all(), (run, key)
    assert kinds == {'rejected then accepted', 'dropped', 'empty range', 'none'}                 # condition 3
    for level in R.VIDEO_LEVELS:
        fgrs, alphas, bg, boxes = R.video_inputs(level)
        plan = R.plan_video(np.random.RandomState(int(g['video/%s/seed' % level])), level, bg.shape[:2], boxes, n_bg_frames=7)
        frame, planes, occ, most, abort = G.pil_video_frame(bg, fgrs, alphas, plan, level)
        w_frame, w_planes, w_occ, w_most, w_abort = R.video_frame(bg, fgrs, alphas, plan, level)
        assert not abort and G.far(occ, (0.3, 0.85, 0.05, 0.5)) and G.far([most], (0.05, 0.5))
        assert (frame == g['video/%s/frame' % level]).all() and (w_frame == frame).all()
        assert (planes.view(np.int64) == w_planes.view(np.int64)).all() and occ == w_occ and most == w_most
        assert ((planes * 255).astype(np.uint8) == g['video/%s/planes' % level]).all()


def test_an_edge_image_needs_the_clamp_between_the_passes():
    """Condition 1 of the generator, on RESIZE_CASES[0] ((37, 53) -> (20, 71), bicubic): both passes clamp at 0 and at 255."""
    src = R.resize_input(0, 1)
    raw_h = R._pass(src[..., None], R.coeffs(53, 71, 'bicubic'), 1, clamp=False)
    raw_v = R._pass(np.clip(raw_h, 0, 255), R.coeffs(37, 20, 'bicubic'), 0, clamp=False)
    assert raw_h.min() < 0 and raw_h.max() > 255 and raw_v.min() < 0 and raw_v.max() > 255
    assert (R.resize(src, (71, 20), 'bicubic', clamp_between=False) != R.resize(src, (71, 20), 'bicubic')).any()


def test_the_fixture_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, 'compose_pinned.npz')) < 100 * 1024


# ---- the host side of the product ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.FILTERS)
def test_table_builder_properties_and_equality_with_the_restatement(name):
    for in_size, out_size in ((53, 71), (48, 13), (200, 12), (7, 40), (1, 5), (60, 1), (9, 9), (1080, 700)):
        t = compose.resample_tables(in_size, out_size, name)
        K = t.shape[1] - compose.TAB_HEADER
        assert t.dtype == np.int32 and t.shape[0] == out_size and K % 4 == 0
        assert K >= int(np.ceil(R.SUPPORT[name] * max(in_size / out_size, 1.0))) * 2 + 1
        for (lo, taps), row in zip(R.coeffs(in_size, out_size, name), t):
            n = len(taps)
            assert row[0] == lo and row[1] == n and (row[2:4] == 0).all()
            assert (row[compose.TAB_HEADER:compose.TAB_HEADER + n] == taps).all() and (row[compose.TAB_HEADER + n:] == 0).all()
            assert abs(int(taps.sum()) - (1 << 22)) <= n and lo + n <= in_size and n >= 1


def test_resize_tables_pick_the_form_from_the_vertical_span():
    t = compose.ResizeTables((20, 160), (24, 9))
    assert t.rows == 160 and t.regime == compose.TWO_PASS
    t = compose.ResizeTables((30, 9), (9, 9))                              # the vertical pass is skipped
    assert t.y is None and t.x is not None and t.rows == 9 and t.regime == compose.FUSED
    t = compose.ResizeTables((640, 1024), (400, 640))                      # the image tool's scale: 16 rows * 1.6 + the support
    assert t.regime == compose.FUSED and t.rows <= 16 * 1.6 + 2 * 2 * 1.6 + 3
    span = int(np.ceil(2.0 * 8.0)) * 2 + 1                                 # ceil(S fs) * 2 + 1 rows per output row at 8 x down
    assert compose.ResizeTables((64, 1024), (64, 128)).rows <= 15 * 8 + span


def test_constants_are_the_librarys():
    lib = hip.lib()
    v = [hip.ctypes.c_int() for _ in range(8)]
    assert lib.mg_compose_limits(*[hip.ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [compose.TILE_ROWS, compose.TILE_BYTES, compose.MAX_ROWS, compose.LDS_BYTES, compose.TAB_HEADER,
                                    compose.MAX_PLANES, compose.SUM_BLOCKS, compose.MAX_SIDE]
    assert lib.mg_compose_limits(*[None] * 8) == -2
    assert 8 * (2 * compose.MAX_PLANES + 1) == 168                          # the read-back of try_place


def test_c_entries_reject_bad_arguments_before_any_launch():
    lib = hip.lib()
    c_int, c_long, P = hip.c_int, hip.c_long, hip.ctypes.c_void_p
    one = P(16)                                                             # never dereferenced: every call below fails its checks
    rs = lambda **k: lib.mg_compose_resize(*[k.get(n, d) for n, d in (
        ('src', one), ('out', P(32)), ('tmp', None), ('xtab', None), ('ytab', None), ('n', c_long(1)), ('ps', c_int(1)), ('src_h', c_int(8)),
        ('src_w', c_int(8)), ('cx', c_int(0)), ('cy', c_int(0)), ('cw', c_int(8)), ('ch', c_int(8)), ('out_h', c_int(8)), ('out_w', c_int(8)),
        ('kx', c_int(0)), ('ky', c_int(0)), ('regime', c_int(0)), ('stream', None))])
    assert rs(ps=c_int(2)) == -2 and rs(cw=c_int(9)) == -2 and rs(cx=c_int(1)) == -2 and rs(regime=c_int(2)) == -2 and rs(n=c_long(-1)) == -2
    assert rs(out_w=c_int(5)) == -2                                         # a size change without a table
    assert rs(xtab=P(64), kx=c_int(6)) == -2 and rs(xtab=P(8), kx=c_int(8)) == -2      # taps not in fours; a table off 16 bytes
    assert rs(ytab=P(64), ky=c_int(8), regime=c_int(1)) == -2               # two launches need tmp
    assert rs(out=one) == -2 and rs(src=None) == -2 and rs(n=c_long(0)) == 0
    assert lib.mg_compose_paste(one, P(32), None, c_int(2), c_int(4), c_int(4), c_int(4), c_int(4), c_int(0), c_int(0), None) == -2
    assert lib.mg_compose_paste(one, one, None, c_int(1), c_int(4), c_int(4), c_int(4), c_int(4), c_int(0), c_int(0), None) == -2
    assert lib.mg_compose_paste(one, P(32), None, c_int(1), c_int(4), c_int(4), c_int(4), c_int(4), c_int(4), c_int(0), None) == 0   # outside: no launch
    place = lambda dtype, n_prev: lib.mg_compose_try_place(one, one, one, one, one, c_int(dtype), c_int(4), c_int(4), c_int(2), c_int(2), c_int(0),
                                                           c_int(0), c_int(n_prev), None)
    assert place(2, 1) == -2 and place(0, 11) == -2 and place(0, -1) == -2
    assert lib.mg_compose_commit(one, None, one, None, one, one, c_int(0), c_int(4), c_int(4), c_int(2), c_int(2), c_int(0), c_int(0), c_int(0),
                                 None) == -2                                 # an image without a foreground
    assert lib.mg_compose_commit(None, None, one, None, one, one, c_int(0), c_int(4), c_int(4), c_int(2), c_int(2), c_int(0), c_int(0), c_int(10),
                                 None) == -2
    assert lib.mg_compose_planes_u8(None, one, one, c_int(0), c_long(1), c_int(4), c_int(4), None) == -2
    assert lib.mg_compose_planes_u8(one, one, one, c_int(3), c_long(1), c_int(4), c_int(4), None) == -2
    assert lib.mg_compose_alpha_box(one, None, c_int(4), c_int(4), None) == -2 and lib.mg_compose_alpha_box(one, one, c_int(0), c_int(4), None) == -2


def test_argument_errors_come_before_the_no_gpu_error():
    u8 = np.zeros((8, 9), np.uint8)
    rgb = np.zeros((8, 9, 3), np.uint8)
    planes = torch.zeros((2, 8, 9))
    bad = [
        (TypeError, lambda: compose.pil_resize(u8.astype(np.float32), (4, 4))),
        (ValueError, lambda: compose.pil_resize(u8, (0, 4))),
        (ValueError, lambda: compose.pil_resize(u8, (4, 4), 'lanczos')),
        (ValueError, lambda: compose.pil_resize(u8, (4, 4), crop=(0, 0, 10, 8))),
        (ValueError, lambda: compose.pil_resize(u8, (4, 4), regime='shared')),
        (ValueError, lambda: compose.pil_resize(np.zeros((160, 4), np.uint8), (4, 9), regime='fused')),
        (ValueError, lambda: compose.pil_resize(u8, (4, 4), tables=compose.ResizeTables((9, 8), (5, 4)))),
        (TypeError, lambda: compose.pil_resize(u8, (4.0, 4))),
        (TypeError, lambda: compose.paste(u8, u8, (0, 0))),                                      # in place: a device tensor
        (ValueError, lambda: compose.paste(torch.zeros((8, 9), dtype=torch.uint8), rgb, (0, 0))),
        (ValueError, lambda: compose.paste(torch.zeros((8, 9), dtype=torch.uint8), u8, (0, 0), np.zeros((3, 3), np.uint8))),
        (TypeError, lambda: compose.try_place(planes.half(), u8, (0, 0), 1)),
        (TypeError, lambda: compose.try_place(planes, u8, (0, 0), 1, torch.float64)),
        (ValueError, lambda: compose.try_place(planes, u8, (0, 0), 3)),
        (ValueError, lambda: compose.commit(None, None, planes, None, u8, (0, 0), 2)),
        (ValueError, lambda: compose.commit(torch.zeros((8, 9, 3), dtype=torch.uint8), None, planes, None, u8, (0, 0), 1)),
        (ValueError, lambda: compose.commit(None, None, planes, np.zeros((4, 4, 3), np.uint8), u8, (0, 0), 1)),
        (TypeError, lambda: compose.planes_u8(planes.long())),
        (ValueError, lambda: compose.alpha_box(np.zeros((2, 8, 9), np.uint8))),
        (ValueError, lambda: compose.synthesize_image(0, [rgb], [u8, u8], rgb)),
        (ValueError, lambda: compose.synthesize_image(0, [rgb], [np.zeros((4, 4), np.uint8)], rgb)),
        (ValueError, lambda: compose.plan_video(np.random.RandomState(0), 'extreme', (48, 64), [(0, 0, 4, 4)])),
        (ValueError, lambda: compose.video_frame(rgb, [rgb], [u8, u8], {'boxes': [(0, 0, 4, 4)], 'placed': [(0, 0, 4, 4)]}, 'easy')),
    ]
    for err, call in bad:
        with pytest.raises(err):
            call()
    if not torch.cuda.is_available():
        for call in (lambda: compose.pil_resize(u8, (4, 4)), lambda: compose.paste(torch.zeros((8, 9), dtype=torch.uint8), u8, (0, 0)),
                     lambda: compose.try_place(planes, u8, (0, 0), 1), lambda: compose.commit(None, None, planes, None, u8, (0, 0), 1),
                     lambda: compose.planes_u8(planes), lambda: compose.alpha_box(u8), lambda: compose.synthesize_image(0, [rgb], [u8], rgb),
                     lambda: compose.video_frame(rgb, [rgb], [u8], {'boxes': [(0, 0, 4, 4)], 'placed': [(0, 0, 4, 4)]}, 'easy')):
            with pytest.raises(hip.MaggieHipError):
                call()


def test_draw_sources_makes_the_tools_two_draws():
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    fg, bg = compose.draw_sources(a, 40, 7)
    want_fg = b.choice(40, size=(b.randint(2, 5),), replace=False)
    want_bg = b.choice(7)
    assert list(fg) == list(want_fg) and bg == want_bg and 2 <= len(fg) <= 4 and len(set(fg)) == len(fg)
    assert a.randint(0, 2 ** 31 - 1) == b.randint(0, 2 ** 31 - 1)
    fg2, bg2 = R.draw_sources(np.random.RandomState(5), 40, 7)
    assert list(fg2) == list(fg) and bg2 == bg


def test_an_empty_draw_range_consumes_no_state():
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    for high in (0, -5):
        with pytest.raises(ValueError):
            a.randint(0, high)
    assert a.randint(0, 2 ** 31 - 1) == b.randint(0, 2 ** 31 - 1)


@pytest.mark.parametrize('level', compose.LEVELS)
def test_plan_video_is_the_restatements_and_consumes_the_same_state(level):
    boxes = [(6, 4, 20, 30), (30, 2, 24, 36), (8, 6, 60, 20)]
    for seed in range(20):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        got, want = compose.plan_video(a, level, (48, 64), boxes, n_bg_frames=1 + seed % 3), R.plan_video(b, level, (48, 64), boxes, 1 + seed % 3)
        assert got == want and a.randint(0, 2 ** 31 - 1) == b.randint(0, 2 ** 31 - 1)
        for (x1, y1, nw, nh), ratio, box in zip(got['placed'], got['ratios'], boxes):
            assert nw == int(box[2] * ratio) and nh == int(box[3] * ratio) and y1 == 48 - nh and x1 >= 0 and (x1 + nw <= 64 or x1 == 0)
    assert compose.OCCLUDED_ABORT == {'easy': None, 'medium': 0.3, 'hard': 0.85} and compose.OCCLUDED_KEEP == {'easy': None, 'medium': 0.05, 'hard': 0.5}
