"""The matting-loss kernels of csrc/losses.hip against float64 at their smallest plane sizes, end to end and one kernel at a time.

References, cases, operation counts and the comparison |got - ref| <= u32 k S live in tests/losses_reference.py;
tests/test_losses_reference_cpu.py proves on the host that this comparison rejects a dropped reflect pre-image, a clamped D^T, a shifted level
weight, sign(0) = 1, a lost factor 3, swapped Sobel kernels on a border column and a two-unit error, at 16 x 16 and 24 x 40.

Cases (H x W, planes as (N, slots)): 16x16 (1,3), 16x24 (1,3), 24x16 (1,3), 32x32 (2,2), 24x40 (1,4), 40x40 (1,3): level-2 planes of 4 .. 10 cells a
side, where pyr_upT has both reflect pre-images on one cell, ring_map degenerates to row-major and the quad kernels have 0 or 1 inner quad; and
264x256 (1,2): 67 584 cells per plane, a second, partial trip of the 256-workgroup reducing grid. 8-bit planes, weights in {0, 1, 2}, a 12 x 12
block with pred == target bit for bit under weight, a zero-weight block, a weightless plane per scale, a masked plane in the pvalid variants.
No cell of a small case lies in a sign band (asserted on the reference); the large case leaves the end-to-end gradient to the single-kernel
tests and drops the 3 x 3 neighbourhood of an undecided Sobel cell from mg_loss_point_bwd (at most 1 % of the weighted cells).

Measured err / (u32 S) on the MI355X (largest over all cases, both sum modes) and the derived k (losses_reference.K_*, sum_depth()):

    output                                      measured   k
    mg_pyr_down                                   1.12     K_DOWN 10
    mg_pyr_upT, with add                          1.10, 0.90   K_UPT 18
    mg_pyr_downT                                  1.16     K_DOWNT 12
    mg_pyr_lap_fwd sum |L| w_l                    0.53     K_LAPCELL 7 + 1 + sum_depth            (42 .. 82)
    mg_pyr_lap_fwd sum w_l, G                     exact    (G on decided cells; 0 on ties)
    mg_loss_point_bwd dp (264 x 256)              0.85     K_POINT_BWD 41
    matting_losses / _multi rec                   1.75     K_D 1 + 1 + sum_depth + 2              (38 .. 70)
    matting_losses / _multi lap                   0.27     k_level(l) + 1 + sum_depth + 5, max l  (78 .. 92)
    matting_losses / _multi grad                  0.15     K_MAGDIFF 5 + sum_depth + 2            (41 .. 73)
    matting_losses / _multi dpred (small cases)   0.68     K_DPRED 62
    first forms rec / lap / grad                  1.17 / 0.24 / 0.15   as above

Every k is an operation count of the longest fp32 path, written out next to its derivation in losses_reference.py, and none was fitted: the
per-cell outputs sit 9 to 90 times below their k because S already carries the size of every term and the counts follow the whole chain
(d -> three blur-decimations -> U -> L for the level-2 band; c G -> U^T -> three D^T for dpred), while the hardware contracts most
product-sum pairs into one rounding. sum_depth() follows the launch geometry (thread, wave, workgroup, then ordered slots or replicated
atomics): 34 at one workgroup per plane, 58 .. 66 at the large size.

The first forms (MG_LOSS_BATCHED=0) run once in a child process, on every case, and must return the per-pixel bits (G0..G2, dpred) of the
default forms; their loss values are held to the float64 reference.
Run time of the file on the MI355X: the 75 cases take 14 s together; the child process of the first forms is the slowest at 2.3 s, every other
case stays below 0.7 s. The float64 references are built once per case and shared by the sum modes.
"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_forms_worker
import losses_reference as LR

pytestmark = pytest.mark.gpu
F32 = torch.float32
MODES = [pytest.param(True, id='slots'), pytest.param(False, id='atomics')]
VALID = [pytest.param(False, id='all'), pytest.param(True, id='pvalid')]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


@contextlib.contextmanager
def _mode(det):
    from maggie_amd import hip
    was = hip.DETERMINISTIC
    hip.set_deterministic(det)
    try:
        yield
    finally:
        hip.set_deterministic(was)


_CACHE = {}


def _memo(key, build):
    """A case and its float64 references are built once and shared by the sum modes and tests that use them."""
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def _case(c):
    return _memo(('case', c), lambda: LR.make_case(*c))


def _refs(c, with_valid):
    return _memo(('refs', c, with_valid), lambda: LR.case_references(_case(c), with_valid))


def _check_values(got, ref, what):
    for i, name in enumerate(('rec', 'lap', 'grad')):
        LR.check(got[i], ref['values'][i], ref['S_values'][i], ref['k_values'][i], F32, '%s %s' % (what, name))


def _dead(ref, w):
    return (LR.planes(w).reshape(ref['pv'].numel(), -1).sum(1) == 0) | (ref['pv'] == 0)


def _check_scale(vals, dp, ref, w, small, what):
    _check_values(vals.cpu(), ref, what)
    dp = dp.cpu()
    dead = _dead(ref, w)
    assert float(dp[dead].abs().sum()) == 0.0, '%s: gradient on a weightless or masked plane' % what
    if small:
        LR.check(dp, ref['grad'], ref['S_grad'], LR.K_DPRED, F32, what + ' dpred')


# ----------------------------------------------------------------------------------------------------------------------
# end to end: MF.matting_losses (one C ABI call per kernel) and MF.matting_losses_multi (three scales per launch)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('det', MODES)
@pytest.mark.parametrize('with_valid', VALID)
@pytest.mark.parametrize('c', LR.SMALL + [LR.LARGE], ids=LR.case_id)
def test_losses_end_to_end_against_float64(c, with_valid, det):
    dev = _dev()
    case, refs = _case(c), _refs(c, with_valid)
    small = c != LR.LARGE
    if small:                # a condition on the reference alone (test_losses_reference_cpu.py checks it for every seed): no cell in a sign band
        assert not any(int(lv['undecided'].sum()) for r in refs for lv in r['levels']) and not any(int(r['sobel']['undecided'].sum()) for r in refs)
    with _mode(det):
        for s in range(3):
            vals, dp, Gs = loss_forms_worker.run_single(case, s, with_valid, dev)
            _check_scale(vals, dp, refs[s], case['weights'][s], small, 'matting_losses')
            live = LR.planes(case['weights'][s]).reshape(case['P'], -1).sum(1) > 0         # G is written wherever the plane has weight
            for l, lv in enumerate(refs[s]['levels']):
                keep = (~lv['undecided']) & live[:, None, None]
                assert torch.equal(Gs[l].cpu().double()[keep], lv['G'][keep]), 'G%d of scale %d' % (l, s)
        vals, dps, _ = loss_forms_worker.run_multi(case, with_valid, dev)
        for s in range(3):
            _check_scale(vals[s], dps[s], refs[s], case['weights'][s], small, 'matting_losses_multi')


# ----------------------------------------------------------------------------------------------------------------------
# one kernel at a time
# ----------------------------------------------------------------------------------------------------------------------
LINEAR_SIZES = [(4, 4), (4, 6), (6, 4), (8, 8), (6, 10), (8, 16), (10, 10), (12, 20), (16, 16), (16, 24), (24, 16), (20, 20), (32, 32), (24, 40),
                (40, 40), (264, 256)]
COEF = 0.8125


def _hw_id(hw):
    return '%dx%d' % tuple(hw[:2])


def _flags(dev, *on):
    return torch.tensor(on, dtype=torch.int32, device=dev)


@pytest.mark.parametrize('hw', LINEAR_SIZES, ids=_hw_id)
def test_pyramid_linear_kernels_against_float64(hw):
    """mg_pyr_down == D, mg_pyr_upT == add - c U^T (with and without add), mg_pyr_downT == c q + D^T, per element; the plane whose flag is 0 is
    not written."""
    from maggie_amd import kernels as K
    dev = _dev()
    h, w = hw
    P = 3
    ptr, ci, st = K.hip.ptr, K.c_int, K.hip.stream
    q, r, add = LR.random_planes((P, h, w), 11), LR.random_planes((P, h // 2, w // 2), 12), LR.random_planes((P, h // 2, w // 2), 13)
    flags = _flags(dev, 1, 0, 1)
    coef = torch.tensor([COEF], dtype=F32, device=dev)
    qd, rd, addd = q.to(dev), r.to(dev), add.to(dev)
    half = lambda: torch.full((P, h // 2, w // 2), 0x5A5A5A5A, dtype=torch.int32).view(F32).to(dev)      # noqa: E731
    full = lambda: torch.full((P, h, w), 0x5A5A5A5A, dtype=torch.int32).view(F32).to(dev)                # noqa: E731

    def compare(got, before, ref, what):
        val, S, k = ref
        got = got.cpu()
        assert torch.equal(LR.bits_of(got[1]), LR.bits_of(before[1].cpu())), what + ': wrote a plane whose flag is 0'
        LR.check(got[[0, 2]], val[[0, 2]], S[[0, 2]], k, F32, what)

    out = half()
    K.hip.call('mg_pyr_down', ptr(qd), ptr(flags), ci(P), ci(h), ci(w), ptr(out), st())
    compare(out, half(), LR.ref_down(q), 'mg_pyr_down')
    out = half()
    K.hip.call('mg_pyr_upT', ptr(qd), ptr(coef), None, ptr(flags), ci(P), ci(h), ci(w), ptr(out), st())
    compare(out, half(), LR.ref_upT(q, COEF), 'mg_pyr_upT')
    out = half()
    K.hip.call('mg_pyr_upT', ptr(qd), ptr(coef), ptr(addd), ptr(flags), ci(P), ci(h), ci(w), ptr(out), st())
    compare(out, half(), LR.ref_upT(q, COEF, add), 'mg_pyr_upT add')
    out = full()
    K.hip.call('mg_pyr_downT', ptr(rd), ptr(qd), ptr(coef), ptr(flags), ci(P), ci(h), ci(w), ptr(out), st())
    compare(out, full(), LR.ref_downT(r, q, COEF), 'mg_pyr_downT')


LAP_SIZES = [(4, 4, 2), (4, 6, 2), (6, 4, 2), (6, 10, 2), (10, 10, 2), (8, 8, 1), (12, 20, 1), (20, 20, 1), (16, 16, 0), (24, 40, 0), (40, 40, 0),
             (264, 256, 0)]


def _lap_inputs(h, w, lvl):
    """x: 8-bit planes, plane 3 all zero (a tie in every cell, under weight); weights in {0, 1, 2} at (h << lvl, w << lvl), plane 1 weightless."""
    rs = np.random.RandomState(100 * h + w)
    P = 4
    x = torch.from_numpy(((rs.randint(0, 256, size=(P, h, w)) - 128) / 255.0).astype(np.float32))
    x[3] = 0
    w0 = torch.from_numpy(rs.randint(0, 3, size=(P, h << lvl, w << lvl)).astype(np.float32))
    w0[1] = 0
    w0[3] = 1 + w0[3] % 2
    return x, w0


@pytest.mark.parametrize('det', MODES)
@pytest.mark.parametrize('hwl', LAP_SIZES, ids=lambda t: '%dx%d-lvl%d' % t)
def test_pyr_lap_fwd_against_float64(hwl, det):
    """mg_pyr_lap_fwd: sum |L| w_l within the bound, sum w_l exact, G == w_l sign(L) on every decided cell and exactly 0 on every tie."""
    from maggie_amd import kernels as K
    dev = _dev()
    h, w, lvl = hwl
    ptr, ci, st = K.hip.ptr, K.c_int, K.hip.stream
    x, w0 = _lap_inputs(h, w, lvl)
    P = x.shape[0]
    flags = _flags(dev, 1, 0, 1, 1)
    xd, w0d = x.to(dev), w0.to(dev)
    down = torch.zeros((P, h // 2, w // 2), dtype=F32, device=dev)
    K.hip.call('mg_pyr_down', ptr(xd), ptr(flags), ci(P), ci(h), ci(w), ptr(down), st())
    ref = _memo(('lap', hwl), lambda: LR.ref_lap_fwd(x, down.cpu(), w0, lvl))
    with _mode(det):
        sums = torch.zeros(32 * 16, dtype=F32, device=dev)
        G = torch.full((P, h, w), 7.0, dtype=F32, device=dev)
        K.hip.call('mg_pyr_lap_fwd', ptr(xd), ptr(down), ptr(w0d), ci(lvl), ci(h << lvl), ci(w << lvl), ptr(flags), ci(P), ci(h), ci(w), ptr(G),
                   ptr(sums), st())
        tot = sums.cpu().double().view(32, 16).sum(0)
    LR.check(tot[0], ref['sum'], ref['S_sum'], ref['k_sum'] + LR.sum_depth(h * w, 3), F32, 'mg_pyr_lap_fwd sum')
    assert float(tot[1]) == float(ref['sum_w'])
    G = G.cpu().double()
    assert float((G[1] - 7.0).abs().max()) == 0.0
    live = torch.tensor([True, False, True, True])[:, None, None]
    keep = (~ref['undecided']) & live
    assert int(ref['tie'][3].sum()) == h * w and int(ref['undecided'].sum()) <= 0.01 * h * w
    assert torch.equal(G[keep], (ref['wl'] * torch.sign(ref['L']))[keep])


@pytest.mark.parametrize('with_valid', VALID)
@pytest.mark.parametrize('with_dd', [False, True], ids=['nodd', 'dd'])
def test_point_bwd_at_the_large_size(with_dd, with_valid):
    """mg_loss_point_bwd at 264 x 256 (scale 2 of the large case: both planes carry weight) against autograd in float64; the 3 x 3
    neighbourhood of an undecided Sobel cell is left out, at most 1 % of the weighted cells."""
    from maggie_amd import kernels as K
    dev = _dev()
    case = _case(LR.LARGE)
    H, W, P = case['H'], case['W'], case['P']
    ptr, ci, st = K.hip.ptr, K.c_int, K.hip.stream
    p, t, w = LR.planes(case['preds'][2]), LR.planes(case['target']), LR.planes(case['weights'][2])
    dd = LR.random_planes((P, H, W), 21, -0.01, 0.01) if with_dd else None
    c_rec, c_grad = float(np.float32(1.3e-5)), float(np.float32(2.1e-5))
    val, S, k, dec = _memo(('pbwd', with_dd), lambda: LR.ref_point_bwd(p, t, w, c_rec, c_grad, dd))
    drop = LR.window_max(dec['undecided'].double()) > 0
    assert float((drop & (w > 0)).sum()) <= LR.MAX_LEFT_OUT * float((w > 0).sum())
    pd, td, wd = p.to(dev), t.to(dev), w.to(dev)
    flags = torch.zeros(P, dtype=torch.int32, device=dev)
    K.hip.call('mg_plane_flags', ptr(wd), ci(P), ci(H * W), ptr(flags), st())
    assert flags.cpu().tolist() == [1] * P
    coef = torch.tensor([c_rec, c_grad], dtype=F32, device=dev)
    A, B, dp = (torch.empty((P, H, W), dtype=F32, device=dev) for _ in range(3))
    pv = case['pvalid'].to(dev) if with_valid else None
    ddd = dd.to(dev) if with_dd else None
    K.hip.call('mg_loss_point_bwd', ptr(pd), ptr(td), ptr(wd), ptr(flags), ci(P), ci(H), ci(W), ptr(coef[0:1]), ptr(coef[1:2]),
               ptr(ddd), ptr(A), ptr(B), ptr(dp), ptr(pv), st())
    dp = dp.cpu()
    planes = [0] if with_valid else [0, 1]
    if with_valid:
        assert float(dp[P - 1].abs().sum()) == 0.0
    keep = ~drop
    LR.check(dp[planes][keep[planes]], val[planes][keep[planes]], S[planes][keep[planes]], k, F32, 'mg_loss_point_bwd')
    tie = dec['tie'][0, :LR.TIE - 2, :LR.TIE - 2]
    assert bool(tie.all())
    if not with_dd:
        assert float(dp[0, :LR.TIE - 2, :LR.TIE - 2].abs().sum()) == 0.0          # sign(0) = 0 in both terms: nothing on the inside of the tie block


# ----------------------------------------------------------------------------------------------------------------------
# the first forms of the four stencils (MG_LOSS_BATCHED=0), in a process of their own
# ----------------------------------------------------------------------------------------------------------------------
def test_first_forms_give_the_bits_of_the_batched_forms(tmp_path):
    _dev()
    assert 'MG_LOSS_BATCHED' not in os.environ, 'MG_LOSS_BATCHED is set: this process does not run the default forms'
    with _mode(True):
        mine = loss_forms_worker.outputs()
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'loss_forms_worker.py')
    path = str(tmp_path / 'first_forms.npz')
    pr = subprocess.run([sys.executable, worker, path], capture_output=True, text=True, timeout=180, env=dict(os.environ, MG_LOSS_BATCHED='0'))
    assert pr.returncode == 0 and 'DONE MG_LOSS_BATCHED=0' in pr.stdout, (pr.returncode, pr.stderr[-3000:])
    theirs = np.load(path)
    assert set(theirs.files) == set(mine)
    for name in sorted(mine):
        a, b = mine[name], theirs[name]
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if not name.endswith('values'):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), '%s differs from the default form' % name
    for c in loss_forms_worker.CASES:
        for wv in (0, 1):
            refs = _refs(c, bool(wv))
            tag = '%s_pv%d' % (LR.case_id(c), wv)
            _check_values(torch.from_numpy(theirs[tag + '_single_values']), refs[0], 'first forms')
            for s in range(3):
                _check_values(torch.from_numpy(theirs[tag + '_multi_values'][s]), refs[s], 'first forms')


# ----------------------------------------------------------------------------------------------------------------------
# the weight of the OS8 prediction at its thresholds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reweight', [True, False])
def test_os8_weight_at_the_band_edges(reweight):
    """mg_os8_weight_ex with gt and a8 on 1/255 and 254/255 and on their float32 neighbours on both sides == the weight_os8 statements of
    compute_loss (arch/maggie.py:271-281) on the CPU; a masked plane (pvalid == 0) whose a8 lies in the band counts as a8 == 0."""
    from maggie_amd import functional as MF
    dev = _dev()
    edge = []
    for thr in (1.0 / 255.0, 254.0 / 255.0):
        f = np.float32(thr)
        edge += [np.nextafter(f, np.float32(-1)), f, np.nextafter(f, np.float32(2))]
    edge = torch.from_numpy(np.array(edge, dtype=np.float32))
    n = edge.numel()
    alphas = torch.ones(1, 5, 8, 8)
    a8 = torch.zeros(1, 5, 8, 8)
    alphas[0, 0].view(-1)[:n] = edge                # gt on the edges, a8 outside the band
    a8[0, 1].view(-1)[:n] = edge                    # a8 on the edges, gt outside the band
    alphas[0, 2] = 0                                # a plane without ground truth, a8 on the edges
    a8[0, 2].view(-1)[:n] = edge
    a8[0, 3] = 0.5                                  # masked plane: a8 in the band and on its edges, gt outside
    a8[0, 3].view(-1)[:n] = edge
    alphas[0, 4].view(-1)[:n] = edge                # masked plane with gt on the edges
    a8[0, 4] = 0.25
    pvalid = torch.tensor([1, 1, 1, 0, 0], dtype=torch.int32)
    for pv in (None, pvalid):
        a8e = a8 if pv is None else a8 * pv.float().view(1, -1, 1, 1)
        w = torch.ones_like(a8e) * (alphas.sum((2, 3), keepdim=True) > 0)
        if reweight:
            w = (((alphas <= 254.0 / 255.0) & (alphas >= 1.0 / 255.0)) | ((a8e <= 254.0 / 255.0) & (a8e >= 1.0 / 255.0))).type(w.dtype) + w
        got = MF.os8_weight(alphas.to(dev), a8.to(dev), reweight, None if pv is None else pv.to(dev))
        assert torch.equal(got.cpu(), w), (reweight, pv)
        if reweight and pv is not None:
            assert float(w[0, 3].max()) == 1.0 and float(w[0, 1].view(-1)[:n].max()) == 2.0
