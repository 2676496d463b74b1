"""Host-side proof for tests/test_gpu_tokens.py. No GPU needed.

1. Every float64 reference of tests/tokens_reference.py equals torch.autograd in float64 to 1e-12.
2. The same operation evaluated by plain float32 torch on the same inputs passes close() at k / 2, on the smallest and the largest device case of
   every kernel family.
3. Every planted fault fails close() by at least 16 x k on the smallest and the largest device case of its family. Where the smallest case of a
   family cannot express a fault at all (an id off by one needs two ids, the output-bias sum over one batch element needs two, a sum over the feature
   rows of a one-row case that is 0 whatever the kernel does, a softmax over one element), the smallest case that can express it stands in; FAULTS
   names the cases."""
import pytest
import torch
import torch.nn.functional as F

import rows_reference as R
import tokens_reference as TR

F32, F64 = torch.float32, torch.float64
TIGHT = 1e-12
A_SMALL, A_TWO, A_BATCH, A_LARGE = TR.ATTN_CASES[0], TR.ATTN_CASES[1], TR.ATTN_CASES[2], TR.ATTN_CASES[-1]
SA_SMALL, SA_TWO, SA_LARGE = TR.SA_CASES[0], TR.SA_CASES[1], TR.SA_CASES[4]
TL_SMALL, TL_LARGE = TR.TL_CASES[0], TR.TL_CASES[-1]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _leaf(t):
    return t.double().requires_grad_(True)


# ------------------------------------------------------------------------------------------------------------------
# 1. the references are right
# ------------------------------------------------------------------------------------------------------------------
def test_attn_tok_reference_equals_autograd():
    c = TR.attn_case(2, 37, 5)
    qk, btab, feat = _leaf(c['qk']), _leaf(c['btab']), _leaf(c['feat'])
    idx = c['ids'].long()[:, None, :].expand(2, TR.T_TOK, 37)
    s = (qk @ feat.transpose(1, 2) + btab.gather(2, idx)) * c['scale']
    p = torch.softmax(s, 2)
    ctx = p @ feat
    ((p * c['dp'].double()).sum() + (ctx * c['dctx'].double()).sum()).backward()
    f = TR.attn_tok_fwd(c['qk'], c['btab'], c['feat'], c['ids'], c['scale'])
    assert _rel(f['score'][0], s.detach()) < TIGHT and _rel(f['p'][0], p.detach()) < TIGHT and _rel(f['ctx'][0], ctx.detach()) < TIGHT
    b = TR.attn_tok_bwd(p.detach(), c['feat'], c['qk'], c['ids'], c['dctx'], c['dp'], c['scale'], 5)
    assert _rel(b['dqk'][0], qk.grad) < TIGHT and _rel(b['dbtab'][0], btab.grad) < TIGHT and _rel(b['dfeat'][0], feat.grad) < TIGHT


@pytest.mark.parametrize('tn', [False, True])
@pytest.mark.parametrize('pad_i', [0, 1, 2])
def test_attn_feat_reference_equals_autograd(tn, pad_i):
    c = TR.attn_case(3, 29, 4)
    pad = c['pads'][pad_i]
    b2 = c['b2'].transpose(1, 2).contiguous() if tn else c['b2']
    feat, kq, b2l, vp, ob = _leaf(c['feat']), _leaf(c['kq']), _leaf(b2), _leaf(c['vp']), _leaf(c['obias'])
    table = b2l if tn else b2l.transpose(1, 2)                              # (B, T, NID)
    idx = c['ids'].long()[:, None, :].expand(3, TR.T_TOK, 29)
    s = (feat @ kq.transpose(1, 2) + table.gather(2, idx).transpose(1, 2)) * c['scale']
    if pad is not None:
        s = s.masked_fill(pad.bool()[:, None, :], float('-inf'))
    p = torch.softmax(s, 2)
    out = p @ vp + ob
    (out * c['dout'].double()).sum().backward()
    f = TR.attn_feat_fwd(c['feat'], c['kq'], b2, c['vp'], c['obias'], pad, c['ids'], c['scale'], tn)
    assert _rel(f['out'][0], out.detach()) < TIGHT and _rel(f['p'][0], p.detach()) < TIGHT
    b = TR.attn_feat_bwd(c['dout'], p.detach(), c['feat'], c['kq'], c['vp'], c['ids'], c['scale'], 4, True, tn)
    for name, leaf in (('dfeat', feat), ('dkq', kq), ('dvp', vp), ('db2', b2l), ('dob', ob)):
        assert b[name][0].shape == leaf.grad.shape and _rel(b[name][0], leaf.grad) < TIGHT, name


@pytest.mark.parametrize('pad_i', [0, 1, 2])
def test_token_sa_reference_equals_autograd(pad_i):
    c = TR.sa_case(3, 7, 20)
    pad = c['pads'][pad_i]
    q, k, v = _leaf(c['q']), _leaf(c['k']), _leaf(c['v'])
    s = q @ k.transpose(1, 2) / 20 ** 0.5
    if pad is not None:
        s = s.masked_fill(pad[:, None, :], float('-inf'))
    p = torch.softmax(s, 2)
    out = p @ v
    (out * c['dout'].double()).sum().backward()
    f = TR.token_sa_fwd(c['q'], c['k'], c['v'], pad)
    assert _rel(f['out'][0], out.detach()) < TIGHT and _rel(f['p'][0], p.detach()) < TIGHT
    b = TR.token_sa_bwd(c['dout'], c['q'], c['k'], c['v'], p.detach())
    assert _rel(b['dq'][0], q.grad) < TIGHT and _rel(b['dk'][0], k.grad) < TIGHT and _rel(b['dv'][0], v.grad) < TIGHT


@pytest.mark.parametrize('wt', [False, True])
@pytest.mark.parametrize('xadd,bias,res,relu,ln', TR.TL_OPTIONS)
def test_token_linear_reference_equals_autograd(xadd, bias, res, relu, ln, wt):
    c = TR.tl_case(7, 12, 8, xadd, bias, res, ln, wt=wt)
    leaves = {n: (None if c[n] is None else _leaf(c[n])) for n in ('x', 'W', 'xadd', 'b', 'res', 'gamma', 'beta')}
    xs = leaves['x'] if not xadd else leaves['x'] + leaves['xadd']
    h = F.linear(xs, leaves['W'].t() if wt else leaves['W'], leaves['b'])
    if relu:
        h = F.relu(h)
    if res:
        h = h + leaves['res']
    y = F.layer_norm(h, (8,), leaves['gamma'], leaves['beta'], c['eps']) if ln else h
    (y * c['dy'].double()).sum().backward()
    f = TR.token_linear_fwd(c['x'], c['W'], c['b'], c['xadd'], c['res'], relu, c['gamma'], c['beta'], c['eps'], wt)
    assert _rel(f['y'][0], y.detach()) < TIGHT
    st = {n: f[n][0] for n in ('z', 'mean', 'rstd')} if ln else {}
    b = TR.token_linear_bwd(c['dy'], c['x'], c['W'], c['xadd'], bias, res, y.detach() if relu else None, c['gamma'], wt=wt, **st)
    want = {'dx': leaves['x'], 'dW': leaves['W'], 'db': leaves['b'], 'dres': leaves['res'], 'dgamma': leaves['gamma'], 'dbeta': leaves['beta']}
    for name, (val, _) in b.items():
        assert val.shape == want[name].grad.shape and _rel(val, want[name].grad) < TIGHT, name
    if xadd:
        assert _rel(b['dx'][0], leaves['xadd'].grad) < TIGHT
    assert set(b) == {n for n, l in want.items() if l is not None}


def test_pair_dx_reference_equals_autograd():
    g = torch.Generator().manual_seed(4)
    x = _leaf(torch.randn(5, 12, generator=g))
    W1, W2, d1, d2 = torch.randn(7, 12, generator=g), torch.randn(3, 12, generator=g), torch.randn(5, 7, generator=g), torch.randn(5, 3, generator=g)
    ((F.linear(x, W1.double()) * d1.double()).sum() + (F.linear(x, W2.double()) * d2.double()).sum()).backward()
    assert _rel(TR.pair_dx(d1, W1, d2, W2)[0], x.grad) < TIGHT


def test_imd_prep_restatement_equals_the_torch_expressions():
    """The numpy restatement against the torch expressions it restates (avg_pool2d > 0, (mask * id).max, max_pool2d > 0)."""
    B, NF, n_in, n_gt, n_i, h, w, s, gs = 2, 3, 4, 3, 6, 5, 7, 2, 4
    mask, gt = TR.imd_case(B, NF, n_in, n_gt, n_i, h, w, s, gs, 0)
    ids, guid, valid = TR.imd_prep(mask.numpy(), gt.numpy(), h, w, n_i)
    m8 = (F.avg_pool2d(mask.view(-1, n_in, h * s, w * s), s, s) > 0).float().view(B, NF, n_in, h, w)
    pos = torch.arange(1, n_in + 1)[None, None, :, None, None]
    want_ids = (m8 * pos).max(2)[0].long().view(B, -1)
    assert torch.equal(torch.from_numpy(ids).long(), want_ids)
    assert torch.equal(torch.from_numpy(valid[:, :n_in]).bool(), m8.amax((1, 3, 4)) > 0) and not valid[:, n_in:].any()
    g8 = (F.max_pool2d(gt.view(-1, n_gt, h * gs, w * gs), gs, gs) > 0).float().view(B, NF, n_gt, h, w).permute(0, 2, 1, 3, 4).reshape(B, n_gt, -1)
    assert torch.equal(torch.from_numpy(guid[:, :n_gt]), g8) and not guid[:, n_gt:].any()
    assert 0 < valid.sum() < valid.size and 0 < guid.mean() < 1 and len(set(ids.ravel().tolist())) > 2        # the case is not degenerate


# ------------------------------------------------------------------------------------------------------------------
# evaluations: family -> {output: (value, S)} in dt, with the stored probabilities / statistics of the fp32 forward as operands of the backward
# ------------------------------------------------------------------------------------------------------------------
def _attn(case, dt, fault=None, pad_i=2, tn=False):
    c = TR.attn_case(*case)
    pad = c['pads'][pad_i]
    out = {}
    f = TR.attn_tok_fwd(c['qk'], c['btab'], c['feat'], c['ids'], c['scale'], dt, fault)
    p32 = TR.attn_tok_fwd(c['qk'], c['btab'], c['feat'], c['ids'], c['scale'], F32)['p'][0]
    b = TR.attn_tok_bwd(p32, c['feat'], c['qk'], c['ids'], c['dctx'], c['dp'], c['scale'], c['NID'], dt, fault)
    out.update({'tok_' + n: v for n, v in list(f.items()) + list(b.items())})
    b2 = c['b2'].transpose(1, 2).contiguous() if tn else c['b2']
    f = TR.attn_feat_fwd(c['feat'], c['kq'], b2, c['vp'], c['obias'], pad, c['ids'], c['scale'], tn, dt, fault)
    p32 = TR.attn_feat_fwd(c['feat'], c['kq'], b2, c['vp'], c['obias'], pad, c['ids'], c['scale'], tn, F32)['p'][0]
    b = TR.attn_feat_bwd(c['dout'], p32, c['feat'], c['kq'], c['vp'], c['ids'], c['scale'], c['NID'], True, tn, dt, fault)
    out.update({'feat_' + n: v for n, v in list(f.items()) + list(b.items())})
    return out


def _attn_k(case):
    B, L, NID = case
    return {'tok_score': TR.K_SCORE, 'tok_p': TR.k_tok_p(L), 'tok_ctx': TR.k_tok_ctx(L), 'tok_dfeat': TR.k_tok_dfeat(L), 'tok_dqk': TR.k_tok_dqk(L),
            'tok_dbtab': TR.k_tok_dbtab(L), 'feat_out': TR.K_FEAT_OUT, 'feat_p': TR.K_FEAT_P, 'feat_dfeat': TR.K_FEAT_DFEAT, 'feat_dkq': TR.k_feat_dkq(L),
            'feat_dvp': TR.k_feat_dvp(L), 'feat_db2': TR.k_feat_db2(L), 'feat_dob': TR.k_feat_dob(B * L)}


def _sa(case, dt, fault=None, pad_i=2):
    c = TR.sa_case(*case)
    pad = c['pads'][min(pad_i, len(c['pads']) - 1)]
    f = TR.token_sa_fwd(c['q'], c['k'], c['v'], pad, dt, fault)
    p32 = TR.token_sa_fwd(c['q'], c['k'], c['v'], pad, F32)['p'][0]
    f.update(TR.token_sa_bwd(c['dout'], c['q'], c['k'], c['v'], p32, dt, fault))
    return f


def _sa_k(case):
    B, T, D = case
    return {'out': TR.k_sa_out(T, D), 'p': TR.k_sa_p(T, D), 'dq': TR.k_sa_dqk(T, D), 'dk': TR.k_sa_dqk(T, D), 'dv': TR.k_sa_dv(T)}


def _tl(case, opts, dt, fault=None):
    R_, K, N = case
    xadd, bias, res, relu, ln = opts
    c = TR.tl_case(R_, K, N, xadd, bias, res, ln)
    args = (c['x'], c['W'], c['b'], c['xadd'], c['res'], relu, c['gamma'], c['beta'], c['eps'], False)
    f = TR.token_linear_fwd(*args, dt, fault)
    f32 = TR.token_linear_fwd(*args, F32)
    st = {n: f32[n][0] for n in ('z', 'mean', 'rstd')} if ln else {}
    f.update(TR.token_linear_bwd(c['dy'], c['x'], c['W'], c['xadd'], bias, res, f32['y'][0] if relu else None, c['gamma'], wt=False, dt=dt, **st))
    return f


def _tl_k(case, opts):
    R_, K, N = case
    ln = opts[4]
    return {'y': TR.k_tl_y(K, ln), 'z': TR.k_tl_lin(K), 'mean': TR.k_tl_stat(K, 'mean'), 'rstd': TR.k_tl_stat(K, 'rstd'), 'dx': TR.k_tl_dx(N, ln),
            'dW': TR.k_tl_dw(R_, ln), 'db': TR.k_tl_db(R_, ln), 'dres': max(TR.k_tl_dz(ln), 1), 'dgamma': TR.k_tl_dgamma(R_), 'dbeta': TR.k_tl_dbeta(R_)}


def _pair(K, dt, fault=None):
    a, b = TR.tl_case(9, K, 40, False, False, False, False), TR.tl_case(9, K, 24, False, False, False, False, seed=1)
    return {'dx': TR.pair_dx(a['dy'], a['W'], b['dy'], b['W'], dt, fault)}, {'dx': TR.k_tl_dx(40, False, 24)}


# ------------------------------------------------------------------------------------------------------------------
# 2. float32 torch stays at or below k / 2
# ------------------------------------------------------------------------------------------------------------------
def _half_k(got, ref, ks, what):
    for name, (val, S) in ref.items():
        r = R.error_ratio(got[name][0], val, S, F32)
        print('F32 %-10s %-12s err/(u32*S) = %.3f (k / 2 = %s)' % (what, name, r, ks[name] / 2))
        assert R.close(got[name][0], val, S, ks[name] / 2, F32), (what, name, r, ks[name] / 2)


@pytest.mark.parametrize('case', [A_SMALL, A_LARGE], ids=str)
@pytest.mark.parametrize('tn', [False, True])
def test_float32_cross_attention_stays_within_half_k(case, tn):
    _half_k(_attn(case, F32, tn=tn), _attn(case, F64, tn=tn), _attn_k(case), 'attn')


@pytest.mark.parametrize('case', [SA_SMALL, SA_LARGE], ids=str)
def test_float32_self_attention_stays_within_half_k(case):
    _half_k(_sa(case, F32), _sa(case, F64), _sa_k(case), 'sa')


@pytest.mark.parametrize('case', [TL_SMALL, TL_LARGE], ids=str)
@pytest.mark.parametrize('opts', TR.TL_OPTIONS, ids=str)
def test_float32_token_linear_stays_within_half_k(case, opts):
    _half_k(_tl(case, opts, F32), _tl(case, opts, F64), _tl_k(case, opts), 'linear')


@pytest.mark.parametrize('K', [TR.PAIR_K[0], TR.PAIR_K[-1]])
def test_float32_pair_dx_stays_within_half_k(K):
    ref, ks = _pair(K, F64)
    _half_k(_pair(K, F32)[0], ref, ks, 'pair')


# ------------------------------------------------------------------------------------------------------------------
# 3. planted faults fail by at least 16 x k
# ------------------------------------------------------------------------------------------------------------------
# fault -> [(family, smallest case that can express the fault, largest case, outputs that must fail)]
FAULTS = {
    'drop_last_row': [('attn', A_SMALL, A_LARGE, ['tok_ctx', 'feat_dkq', 'feat_dvp', 'feat_dob']),
                      ('attn', A_TWO, A_LARGE, ['tok_dqk'])],                      # L = 1: dS = P (G - P G) = 0 whatever the kernel sums
    'drop_first_row_of_last_workgroup': [('attn', A_SMALL, A_LARGE, ['tok_ctx', 'feat_dkq', 'feat_dvp', 'feat_dob']),
                                         ('attn', A_TWO, A_LARGE, ['tok_dqk'])],
    'id_off_by_one': [('attn', A_TWO, A_LARGE, ['tok_p', 'tok_dbtab', 'feat_p', 'feat_out', 'feat_db2'])],     # needs NID > 1; one row of a thousand barely moves ctx: P shows it
    'other_layout': [('attn', A_TWO, A_LARGE, ['feat_p', 'feat_out']), ('attn_tn', A_TWO, A_LARGE, ['feat_p', 'feat_out'])],   # needs NID > 1
    'pad_ignored': [('attn', A_SMALL, A_LARGE, ['feat_p', 'feat_out']), ('sa', SA_TWO, SA_LARGE, ['p', 'out'])],               # a mask needs T > 1
    'scale_twice': [('attn', A_SMALL, A_LARGE, ['feat_p', 'feat_out', 'feat_dfeat', 'feat_dkq']),
                    ('attn', A_TWO, A_LARGE, ['tok_score', 'tok_p', 'tok_ctx', 'tok_dfeat', 'tok_dqk']),                         # L = 1: P = 1 whatever the score
                    ('sa', SA_TWO, SA_LARGE, ['p', 'out', 'dq', 'dk'])],
    'rowdot_short': [('attn', A_SMALL, A_LARGE, ['tok_dfeat', 'tok_dqk', 'tok_dbtab'])],
    'dob_one_batch': [('attn', A_BATCH, A_LARGE, ['feat_dob'])],                                                                 # needs B > 1
    'pair_twice': [('pair', TR.PAIR_K[0], TR.PAIR_K[-1], ['dx'])],
    'pair_missing': [('pair', TR.PAIR_K[0], TR.PAIR_K[-1], ['dx'])],
    'ln_divisor': [('linear', TL_SMALL, TL_LARGE, ['y'])],
}


def _family(family, case, dt, fault=None):
    if family == 'attn':
        return _attn(case, dt, fault), _attn_k(case)
    if family == 'attn_tn':
        return _attn(case, dt, fault, tn=True), _attn_k(case)
    if family == 'sa':
        return _sa(case, dt, fault), _sa_k(case)
    if family == 'linear':
        return _tl(case, TR.TL_OPTIONS[0], dt, fault), _tl_k(case, TR.TL_OPTIONS[0])
    res, ks = _pair(case, dt, fault)
    return res, ks


@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_planted_fault_fails_by_sixteen_k(fault):
    for family, small, large, outputs in FAULTS[fault]:
        for case in (small, large):
            ref, ks = _family(family, case, F64)
            bad, _ = _family(family, case, F64, fault)
            for name in outputs:
                r = R.error_ratio(bad[name][0], ref[name][0], ref[name][1], F32)
                print('FAULT %-34s %-8s %-16s %-10s err/(u32*S) = %.3g (16 k = %d)' % (fault, family, case, name, r, 16 * ks[name]))
                assert not R.close(bad[name][0], ref[name][0], ref[name][1], 16 * ks[name], F32), (fault, family, case, name, r, 16 * ks[name])


def test_the_rows_map_of_token_linear_bwd_is_injective_only_with_the_guard():
    """The thread -> (k, row) map of token_linear_bwd_rows (256 threads, cols = min(K, 128), groups = 256 // cols, thread t: c = t % cols,
    h = t // cols, k = c, c + cols, ..., rows h, h + groups, ... of a block of 4). Without the guard h < groups the surplus threads of 64 < K < 128
    own elements twice (K = 68 .. 124: 64 pairs at K = 96), which the accumulating form of dx_pair turns into a race; with it every element of every
    admissible K has exactly one owner."""
    dup_ks = []
    for K in range(4, 257, 4):
        cols = min(K, 128)
        groups = 256 // cols
        for guard in (False, True):
            owners = {}
            for t in range(256):
                c, h = t % cols, t // cols
                if guard and h >= groups:
                    continue
                for k in range(c, K, cols):
                    for rl in range(h, 4, groups):
                        owners[(k, rl)] = owners.get((k, rl), 0) + 1
            assert set(owners) == {(k, rl) for k in range(K) for rl in range(4)}, K
            if guard:
                assert max(owners.values()) == 1, K
            elif max(owners.values()) > 1:
                dup_ks.append(K)
                if K == 96:
                    assert sum(v > 1 for v in owners.values()) == 64
    assert dup_ks == list(range(68, 128, 4))
