"""tests/losses_reference.py proven on the host: the restatement equals the oracle's losses, the operators U^T and D^T obtained from autograd
equal tap-by-tap matrices built here from the reflect rule alone, every case's seed meets its condition, and the comparison
|got - ref| <= u32 k S accepts the float32 torch run of the restatement and rejects, at 16 x 16 and at 24 x 40, each of the defects a
hand-derived adjoint can have: a dropped reflect pre-image of U^T (top, bottom), D^T with clamp for reflect at the bottom, the level
weight sampled one cell off, sign(0) = +1 on the tie block, the missing factor 3, the Sobel adjoint with kx and ky swapped on a border
column, and one element two units of its bound away."""
import pytest
import torch

import losses_reference as LR
from oracle import refmodel

F32, F64 = torch.float32, torch.float64
ALL = LR.SMALL + [LR.LARGE]
REJECT_AT = [(16, 16, 1, 3), (24, 40, 1, 4)]
_CACHE = {}


def _case(c):
    if c not in _CACHE:
        case = LR.make_case(*c)
        _CACHE[c] = (case, {wv: LR.case_references(case, wv) for wv in (False, True)})
    return _CACHE[c]


# ------------------------------------------------------------------------------------------------------------------
# the operators as matrices, from the padding rule alone
# ------------------------------------------------------------------------------------------------------------------
G5 = [1 / 16., 4 / 16., 6 / 16., 4 / 16., 1 / 16.]


def _refl(k, n):
    return -k if k < 0 else (2 * (n - 1) - k if k >= n else k)


def d_matrix(h, clamp_hi=False):
    """(h / 2, h): one axis of blur + decimate. clamp_hi: the defect -- indices past the end clamped instead of reflected."""
    M = torch.zeros((h // 2, h), dtype=F64)
    for a in range(h // 2):
        for i in range(5):
            k = 2 * a + i - 2
            M[a, (h - 1) if (clamp_hi and k >= h) else _refl(k, h)] += G5[i]
    return M


def u_matrix(h, drop_lo=False, drop_hi=False):
    """(h, h / 2): one axis of zero-stuff + 2 x blur. drop_lo / drop_hi: the defects -- the taps that reach a stuffed sample through the
    reflection at the top (they land on cell 1) / at the bottom (on cell h / 2 - 1) are left out."""
    M = torch.zeros((h, h // 2), dtype=F64)
    for y in range(h):
        for i in range(5):
            k = y + i - 2
            kk = _refl(k, h)
            if (kk & 1) or (drop_lo and k < 0) or (drop_hi and k >= h):
                continue
            M[y, kk // 2] += 2 * G5[i]
    return M


def lap_grad_matrices(G, c, **defect):
    """The Laplacian term of d/dpred from G_l and c_l with the matrix operators; a defect applies to the row axis of every level."""
    dd = None
    for l in (2, 1, 0):
        P, h, w = G[l].shape
        Uy, Ux = u_matrix(h, defect.get('drop_lo', False), defect.get('drop_hi', False)), u_matrix(w)
        Dy, Dx = d_matrix(h, defect.get('clamp_hi', False)), d_matrix(w)
        r = -c[l] * torch.einsum('ya,pyx,xb->pab', Uy, G[l], Ux)
        if dd is not None:
            r = r + dd
        dd = c[l] * G[l] + torch.einsum('ay,pab,bx->pyx', Dy, r, Dx)
    return dd


@pytest.mark.parametrize('hw', [(4, 4), (4, 6), (6, 4), (8, 8), (10, 6), (16, 24), (66, 64)])
def test_autograd_adjoints_equal_the_tap_matrices(hw):
    h, w = hw
    q, r = LR.random_planes((2, h, w), 1).double(), LR.random_planes((2, h // 2, w // 2), 2).double()
    Uy, Ux, Dy, Dx = u_matrix(h), u_matrix(w), d_matrix(h), d_matrix(w)
    assert torch.allclose(LR.U(r), torch.einsum('ya,pab,xb->pyx', Uy, r, Ux), rtol=0, atol=1e-14)
    assert torch.allclose(LR.D(q), torch.einsum('ay,pyx,bx->pab', Dy, q, Dx), rtol=0, atol=1e-14)
    assert torch.allclose(LR.UT(q), torch.einsum('ya,pyx,xb->pab', Uy, q, Ux), rtol=0, atol=1e-14)
    assert torch.allclose(LR.DT(r), torch.einsum('ay,pab,bx->pyx', Dy, r, Dx), rtol=0, atol=1e-14)
    # the defects change something at this size (at h == 4 both pre-images of U^T fall on the same cell)
    assert not torch.equal(u_matrix(h, drop_lo=True), Uy) and not torch.equal(u_matrix(h, drop_hi=True), Uy)
    assert not torch.equal(d_matrix(h, clamp_hi=True), Dy)


# ------------------------------------------------------------------------------------------------------------------
# the restatement against the oracle
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_valid', [False, True], ids=['all', 'pvalid'])
@pytest.mark.parametrize('c', ALL, ids=LR.case_id)
def test_restatement_in_float32_equals_the_oracle(c, with_valid):
    case, _ = _case(c)
    H, W = c[:2]
    pv = case['pvalid'] if with_valid else None
    for p, w in zip(case['preds'], case['weights']):
        mine, leaf = LR.restated(LR.planes(p), LR.planes(case['target']), LR.planes(w), pv, F32)
        pr = p.clone().requires_grad_(True)
        pe = pr if pv is None else pr * pv.float().reshape(p.shape[0], p.shape[1], 1, 1)
        v = lambda t: t.reshape(-1, 1, H, W)        # noqa: E731
        ref = torch.stack([refmodel.regression_loss(pe, case['target'], w), refmodel.lap_loss(v(pe), v(case['target']), v(w)),
                           refmodel.grad_loss(pe, case['target'], w)])
        assert torch.allclose(mine.detach(), ref.detach(), rtol=2e-6, atol=0), (mine, ref)
        g = torch.tensor(LR.GOUT)
        (mine * g).sum().backward()
        (ref * g).sum().backward()
        err = float((LR.planes(pr.grad) - leaf.grad).abs().max())
        assert err <= 2e-6 * float(pr.grad.abs().max()), (err, float(pr.grad.abs().max()))


@pytest.mark.parametrize('c', ALL, ids=LR.case_id)
def test_every_seed_meets_its_condition(c):
    case, refs = _case(c)
    ok, detail = LR.seed_condition(case, c != LR.LARGE)
    assert ok, detail
    T = LR.TIE
    for wv in (False, True):
        for ref, w in zip(refs[wv], case['weights']):
            w = LR.planes(w)
            assert float(w[0, :T, :T].min()) > 0 and float(ref['d'][0, :T, :T].abs().max()) == 0
            lv = ref['levels']
            assert bool(lv[0]['tie'][0, :T - 4, :T - 4].all()) and int(lv[1]['tie'].sum()) > 0       # L == 0 with every term zero
            for l in lv:
                assert float(l['L'][l['tie']].abs().sum()) == 0 and float(l['G'][l['tie']].abs().sum()) == 0
            sb = ref['sobel']
            assert bool(sb['tie'][0, :T - 1, :T - 1].all()) and bool(sb['tie'][0, c[0] - LR.ZERO_H + 1:, c[1] - LR.ZERO_W + 1:].all())
            assert float(sb['diff'][sb['tie']].abs().max()) == 0
            dead = (w.reshape(w.shape[0], -1).sum(1) == 0) | (ref['pv'] == 0)
            assert int(dead.sum()) >= (1 if (wv or ref is not refs[wv][2]) else 0) and float(ref['grad'][dead].abs().sum()) == 0
            # sign(0) = 0: no L1 term on the tie block, no Sobel term on it or under zero weight (the pyramid's D^T still reaches both)
            assert float(ref['g_l1'][0, :T, :T].abs().max()) == 0 and float(ref['g_sob'][0, :T - 2, :T - 2].abs().max()) == 0
            assert float(ref['g_sob'][w == 0].abs().max()) == 0 and float(ref['g_l1'][w == 0].abs().max()) == 0
            dec = ref['g_l1'] + ref['g_lap'] + ref['g_sob']
            assert float((dec - ref['grad']).abs().max()) <= 1e-15
            assert bool((ref['S_grad'] >= ref['grad'].abs() * (1 - 1e-12)).all())


# ------------------------------------------------------------------------------------------------------------------
# the comparison: accepts fp32, rejects the defects
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_valid', [False, True], ids=['all', 'pvalid'])
@pytest.mark.parametrize('c', ALL, ids=LR.case_id)
def test_comparison_accepts_the_float32_run(c, with_valid):
    case, refs = _case(c)
    pv = case['pvalid'] if with_valid else None
    for s, (p, w) in enumerate(zip(case['preds'], case['weights'])):
        ref = refs[with_valid][s]
        vals, leaf = LR.restated(LR.planes(p), LR.planes(case['target']), LR.planes(w), pv, F32)
        (vals * torch.tensor(LR.GOUT)).sum().backward()
        for i, name in enumerate(('rec', 'lap', 'grad')):
            LR.check(vals[i].detach(), ref['values'][i], ref['S_values'][i], ref['k_values'][i], F32, 'torch32 ' + name)
        keep = torch.ones_like(ref['grad'], dtype=torch.bool)
        if c == LR.LARGE:                        # the float32 run decides its own signs: leave out what the band leaves open
            keep, _ = LR.sobel_keep(ref, LR.planes(w))
            lap_open = sum(int(lv['undecided'].sum()) for lv in ref['levels'])
            if lap_open:
                continue
        LR.check(leaf.grad[keep], ref['grad'][keep], ref['S_grad'][keep], LR.K_DPRED, F32, 'torch32 dpred')


def _defects(case, ref, w):
    """name -> (got, ref, S, k) with the float64 result carrying one defect."""
    G, c = [lv['G'] for lv in ref['levels']], ref['coef'][2:]
    pv3 = ref['pv'][:, None, None]
    grad, S = ref['grad'], ref['S_grad']
    assert float((lap_grad_matrices(G, c) * pv3 - ref['g_lap']).abs().max()) <= 1e-15          # without a defect: the reference itself
    out = {}
    for name, kw in (('upT without the a == 1 pre-image', {'drop_lo': True}), ('upT without the ma == h pre-image', {'drop_hi': True}),
                     ('downT with clamp on the last two rows', {'clamp_hi': True})):
        out[name] = grad - ref['g_lap'] + lap_grad_matrices(G, c, **kw) * pv3
    Gs = [G[0]] + [w[:, 1::1 << l, 1::1 << l] * torch.sign(ref['levels'][l]['L']) for l in (1, 2)]
    out['level weight sampled at (y << lvl) + 1'] = grad - ref['g_lap'] + LR.lap_grad(Gs, c) * pv3
    out['sign(0) = +1 on the tie block'] = grad + ref['coef'][0] * w * (ref['d'] == 0) * pv3
    out['factor 3 missing'] = grad - ref['g_lap'] * (2.0 / 3.0)
    sb = ref['sobel']
    adj, swapped = LR.sobel_adjoint(sb['A'], sb['B']), LR.sobel_adjoint(sb['A'], sb['B'], kx=torch.tensor(LR.KX, dtype=F64).t().contiguous())
    col = torch.zeros_like(adj, dtype=torch.bool)
    col[:, :, 0] = True
    out['Sobel adjoint with kx and ky swapped on column 0'] = grad - ref['g_sob'] + ref['coef'][1] * w * torch.where(col, swapped, adj) * pv3
    off = grad.clone()
    i = int(torch.argmax(S))
    off.view(-1)[i] += 2 * LR.U32 * LR.K_DPRED * S.view(-1)[i]
    out['one element off by two units of its bound'] = off
    return out


@pytest.mark.parametrize('with_valid', [False, True], ids=['all', 'pvalid'])
@pytest.mark.parametrize('c', REJECT_AT, ids=LR.case_id)
def test_comparison_rejects_every_defect(c, with_valid):
    case, refs = _case(c)
    for s, w in enumerate(case['weights']):
        ref = refs[with_valid][s]
        assert LR.close(ref['grad'].float(), ref['grad'], ref['S_grad'], LR.K_DPRED, F32)       # the rounded reference passes
        for name, got in _defects(case, ref, LR.planes(w).double()).items():
            assert not LR.close(got, ref['grad'], ref['S_grad'], LR.K_DPRED, F32), (name, s)
        # the lost factor 3 in the value, and a value two units away
        v, S, k = ref['values'], ref['S_values'], ref['k_values']
        assert LR.close(v[1].float(), v[1], S[1], k[1], F32)
        assert not LR.close(v[1] / 3, v[1], S[1], k[1], F32)
        for i in range(3):
            assert not LR.close(v[i] + 2 * LR.U32 * k[i] * S[i], v[i], S[i], k[i], F32)


def test_sum_depth_counts():
    # one workgroup per plane, three planes: 4 cells per thread-trip, 6 + 4, slots 1 + 2 + 16 + 1
    assert LR.sum_depth(16 * 16, 3) == 4 + 10 + 20
    # the large plane: 256 workgroups, two trips; two planes: atomics 16 per replica + 32 replicas
    assert LR.sum_depth(264 * 256, 2) == 8 + 10 + 48
    assert [LR.k_level(l) for l in range(3)] == [18, 28, 38] and LR.K_DPRED == 62 and LR.K_POINT_BWD == 41
