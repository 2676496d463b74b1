"""tools/device_code_diff.py on hand-written assembly: the order of the functions and the compiler's per-function label index must not count, and
everything else must -- an instruction, the block or constant-pool entry a label names, a metadata field, a symbol that comes or goes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _fn(name, idx, body='\tv_mov_b32_e32 v0, 1', pool=0, target=2):
    return '''\t.section\t.text.%(n)s,"axG",@progbits,%(n)s,comdat
\t.globl\t%(n)s ; -- Begin function %(n)s
%(n)s:
\ts_getpc_b64 s[0:1]
\ts_add_u32 s0, s0, .LCPI%(i)d_%(p)d@rel32@lo+4
.LBB%(i)d_1:                                ; =>This Inner Loop Header: Depth=1
%(b)s
\ts_cbranch_scc1 .LBB%(i)d_%(t)d
.LBB%(i)d_2:%(pad)s;   in Loop: Header=BB%(i)d_1 Depth=1
\ts_endpgm
.Lfunc_end%(i)d:
\t.size\t%(n)s, .Lfunc_end%(i)d-%(n)s
                                        ; -- End function
''' % dict(n=name, i=idx, b=body, p=pool, t=target, pad=' ' * (30 - len(str(idx))))


def _meta(names, sgpr=10):
    return '\t.section\t.AMDGPU.gpr_maximums,"",@progbits\n\t.amdgpu_metadata\n---\namdhsa.kernels:\n' + ''.join(
        '  - .agpr_count:     0\n    .sgpr_count:     %d\n    .symbol:         %s.kd\n' % (sgpr, n) for n in names) + 'amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n'


def test_order_and_label_index_do_not_count_and_everything_else_does():
    import device_code_diff as D
    base = D.pieces(_fn('ka', 0) + _fn('kb', 1) + _meta(['ka', 'kb']))
    assert set(base) == {'<file>', 'ka', 'kb'}
    # swapped order, indices 11 and 3 (another digit count: the padding in front of the comment moves too), one __hip_cuid_ line
    assert D.pieces(_fn('kb', 3) + _fn('ka', 11) + '__hip_cuid_1234:\n' + _meta(['kb', 'ka'])) == base
    differs = lambda asm: sorted(k for k, v in D.pieces(asm).items() if base.get(k) != v)
    assert differs(_fn('ka', 0, body='\tv_mov_b32_e32 v0, 2') + _fn('kb', 1) + _meta(['ka', 'kb'])) == ['ka']
    assert differs(_fn('ka', 0) + _fn('kb', 1, pool=1) + _meta(['ka', 'kb'])) == ['kb']              # another constant-pool entry
    assert differs(_fn('ka', 0) + _fn('kb', 1, target=1) + _meta(['ka', 'kb'])) == ['kb']            # another branch target
    assert differs(_fn('ka', 0) + _fn('kb', 1) + _meta(['ka', 'kb'], sgpr=12)) == ['ka', 'kb']       # a metadata field
    assert set(D.pieces(_fn('ka', 0) + _meta(['ka']))) == {'<file>', 'ka'}                           # a symbol that went
