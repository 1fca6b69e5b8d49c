"""The entry points that answer an empty table (no node, or no pair) by clearing their record — the loss record, or the curvature
gradient — and launching nothing else: mm_spd_pdist_loss, mm_spd_pdist_loss_det, mm_spd_pdist_loss_subset and the two Stein loss
entries at n = 0, mm_sne_kl_loss, mm_sst_kl_loss and mm_stereo_pdist_bwd at n = 0 and n = 1.  That clear is a kernel node
(csrc/clear.hpp), as every clear of the library: a captured memset node zeroes its region on the first replay only
(profiles/replay.md).  Each entry is called eagerly, captured alone in a graph and replayed three times; the record is filled with
NaN before every call and must come back as +0 bit for bit, the words behind it untouched.  Everything goes through the C ABI."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DT = {'f32': torch.float32, 'f64': torch.float64}
D = 3                      # the smallest SPD size every entry takes (the Stein entries refuse d < 2)
WMIN, WMAX = 1e-8, 1e8     # the eigenvalue window of tests/test_replay_gpu.py; nothing is computed here
GUARD = 2                  # elements behind the record that the call must leave alone


def _B():
    from graphembed import _backend as B
    return B


def _spd(entry, det=False, subset=False, stein=False):
    """(record length, call): the SPD loss entries at an empty table; every buffer the argument check wants is a non-null dummy"""
    def call(dtc, rec, dummy):
        B = _B()
        p, st = B.ptr, B.stream_of(rec)
        x = p(dummy)
        shape = (0, D, None, 0, 0, 0) if subset else (0, D, 0, 0)      # n_total, d, idx, bs, rows | n, d, rows
        window = (WMIN, ) if stein else (WMIN, WMAX)
        ws = (x, x) if det else (x, )
        return B.lib().raw(entry)(dtc, B.LOSS_STRESS, x, None, x, *shape, 1.0, 1.0, 3, None, *window, p(rec), x, *ws, 0, st)
    return 2, call


def _kl(entry, n):
    def call(dtc, rec, dummy):
        B = _B()
        x = B.ptr(dummy)
        return B.lib().raw(entry)(dtc, 0, x, x, n, 1.3, x, B.ptr(rec), x, B.stream_of(rec))
    return 1, call


def _stereo(n):
    def call(dtc, rec, dummy):      # the record is grad_c; c_raw is read by no kernel here
        B = _B()
        x = B.ptr(dummy)
        return B.lib().raw('mm_stereo_pdist_bwd')(dtc, x, x, n, 4, 0, n, 1, x, 0, 0.001, x, B.ptr(rec), x, B.stream_of(rec))
    return 1, call


CASES = {
    'mm_spd_pdist_loss-n0': _spd('mm_spd_pdist_loss'),
    'mm_spd_pdist_loss_det-n0': _spd('mm_spd_pdist_loss_det', det=True),
    'mm_spd_pdist_loss_subset-n0': _spd('mm_spd_pdist_loss_subset', subset=True),
    'mm_spd_stein_pdiv_loss-n0': _spd('mm_spd_stein_pdiv_loss', stein=True),
    'mm_spd_stein_pdiv_loss_subset-n0': _spd('mm_spd_stein_pdiv_loss_subset', subset=True, stein=True),
    'mm_sne_kl_loss-n0': _kl('mm_sne_kl_loss', 0),
    'mm_sne_kl_loss-n1': _kl('mm_sne_kl_loss', 1),
    'mm_sst_kl_loss-n0': _kl('mm_sst_kl_loss', 0),
    'mm_sst_kl_loss-n1': _kl('mm_sst_kl_loss', 1),
    'mm_stereo_pdist_bwd-n0': _stereo(0),
    'mm_stereo_pdist_bwd-n1': _stereo(1),
}


def _check(name, stage, rec, words):
    bits = rec.view(torch.int32 if rec.dtype == torch.float32 else torch.int64).cpu().tolist()
    print(f'{name} {stage}: record bits {[hex(b) for b in bits[:words]]}')
    assert bits[:words] == [0] * words, (name, stage, [hex(b) for b in bits[:words]])
    assert bool(torch.isnan(rec[words:]).all()), (name, stage, 'the call wrote behind its record')


@pytest.mark.parametrize('dname', ('f32', 'f64'))
@pytest.mark.parametrize('name', list(CASES))
def test_the_record_of_an_empty_table_is_plus_zero_on_every_replay(name, dname):
    B = _B()
    words, call = CASES[name]
    dtc = B.MM_F32 if dname == 'f32' else B.MM_F64
    rec = torch.full((words + GUARD, ), float('nan'), dtype=DT[dname], device='cuda')
    dummy = torch.zeros(256, dtype=torch.uint8, device='cuda')
    assert call(dtc, rec, dummy) == 0      # eager (MM_OK)
    torch.cuda.synchronize()
    _check(name, 'eager', rec, words)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = call(dtc, rec, dummy)
    assert rc == 0
    for k in range(3):
        rec.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        _check(name, f'replay {k + 1}', rec, words)
