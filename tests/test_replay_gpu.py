"""Every accumulating entry point of the C ABI, captured alone in a graph and replayed three times with the inputs A, B, A of its
row of tests/replay_cases.py — each replay held on its own to the fp64 oracle of the case that was loaded, under the family
module's bound, and to the eager call of the same case: torch.equal for the rows without float atomics,
e_replay <= 2 e_eager + 64 eps max|oracle| (grass_cases.check's rule for reordered atomic sums) for the others.  Before each replay
the inputs are copied in place into the captured buffers, every output is filled with NaN and every workspace is put into the state
its header contract allows (0xFF bytes where it "may hold anything").  The third replay — A again, after B went through the same
buffers — is the one the recorded failure of profiles/vec_deterministic.md would have shown in.  One row per family is also
recorded twice in ONE graph on two sets of buffers and one workspace, as GraphedTrainStep(unroll=2) does.

Everything goes through the C ABI on one stream; the module runs in the environment it finds (the form switches are read once per
process).  Every comparison prints err / bound (-rA); the last test prints the worst ratio per family, dtype and stage:
profiles/replay.md."""
import numpy as np
import pytest
import torch

import replay_cases as R

pytestmark = pytest.mark.gpu
DT = {'f32': torch.float32, 'f64': torch.float64}
RECORDS = []      # (family, dname, stage, row id, quantity, err / bound, e_replay / allowance)
STAGES = ('eager', 'replay 1 (A)', 'replay 2 (B)', 'replay 3 (A)', 'unrolled 1', 'unrolled 2')


def _B():
    from graphembed import _backend as B
    return B


def plus_zero(t):
    """every element is +0 (torch.equal takes -0 for 0)"""
    return bool((t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64) == 0).all())


class Buffers:
    """The fixed device buffers of one row and its call into the library.  `ws`: the workspaces of another set to share."""

    def __init__(self, row, ws=None):
        B = _B()
        self.row, self.dt = row, DT[row['dname']]
        self.dtc = B.MM_F32 if row['dname'] == 'f32' else B.MM_F64
        self.g = row['geometry']
        a = R.inputs(row, 'a')
        self.inp = {k: (None if v is None else torch.from_numpy(np.array(v)).to(device='cuda', dtype=torch.int64 if k == 'idx' else self.dt))
                    for k, v in a.items()}
        self.grad = torch.empty_like(self.inp['x'])
        self.out = torch.empty(2, dtype=self.dt, device='cuda')
        self.has_loss = self.g['loss'] is not None
        self.has_scale = row['family'] not in ('sne', 'sst')      # (a KL objective's record is the loss alone)
        self.curv = row['family'] == 'stereo'                     # (out[0] is the curvature gradient)
        self.ws = ws if ws is not None else {name: torch.empty(self._ws_bytes(name), dtype=torch.uint8, device='cuda') for name in row['buffers'] if name != 'grad'}

    def _ws_bytes(self, name):
        raw, g, fam = _B().lib().raw, self.g, self.row['family']
        if fam in ('sne', 'sst'):
            return raw(f'mm_{fam}_kl_ws_bytes')(self.dtc, g['n'])
        if fam == 'stereo':
            return raw('mm_stereo_pdist_ws_bytes')(self.dtc, g['n'], g['m'])
        if fam == 'stein':
            return raw('mm_spd_pdist_ws_bytes')(self.dtc, g['n_total'], g['shape'][0])
        if fam == 'spd':
            return raw('mm_spd_pdist_det_ws_bytes' if name == 'det_ws' else 'mm_spd_pdist_ws_bytes')(self.dtc, g['n_total'], g['shape'][0])
        if fam == 'vec':
            if name == 'det_ws':
                return raw('mm_vec_pdist_det_ws_bytes')(self.dtc, R_KIND[g['kind']], g['n'], g['m'])
            return raw('mm_vec_pdist_ws_bytes')(self.dtc, g['n_total'], g['m'])
        loss = '_loss' if self.has_loss else ''
        if fam == 'so':
            return raw(f'mm_so_pdist{loss}_ws_bytes')(self.dtc, g['n_total'], g['shape'][0])
        return raw(f'mm_grass_pdist{loss}_ws_bytes')(self.dtc, g['n_total'], *g['shape'])

    def load(self, which):
        """the case's inputs, copied in place into the captured buffers"""
        for k, v in R.inputs(self.row, which).items():
            if v is not None:
                self.inp[k].copy_(torch.from_numpy(np.array(v)).to(self.inp[k].dtype))

    def dirty(self, keep_ws=False):
        """outputs full of NaN; workspaces in the state their contract allows"""
        contract = self.row['buffers'].get('grad', (R.ANY, ))[0]
        self.grad.fill_(0.0 if contract == R.ZERO else float('nan'))
        self.out.fill_(float('nan'))
        if not keep_ws:
            for name, t in self.ws.items():
                t.fill_(0 if self.row['buffers'][name][0] == R.ZERO else 0xFF)

    def enqueue(self):
        """the C call alone on the current stream: capture-safe; returns its code"""
        B = _B()
        g, p, i = self.g, B.ptr, self.inp
        fn, st = B.lib().raw(self.row['entry']), B.stream_of(i['x'])
        n, nt, rb, re = g['n'], g['n_total'], g['rows'][0], g['rows'][1]
        ws = [p(t) for t in self.ws.values()]
        if self.row['family'] in ('sne', 'sst'):      # (MM_SST_INCLUSIVE / _EXCLUSIVE are MM_SNE_'s codes)
            return fn(self.dtc, R.SNE_MODE[g['mode']], p(i['side']), p(i['x']), n, SNE_ALPHA, p(self.grad), p(self.out), *ws, st)
        if self.row['family'] == 'stereo':
            return fn(self.dtc, p(i['x']), p(i['side']), n, g['m'], rb, re, 1, p(i['scale']), g['c_mode'], STEREO_C_MIN, p(self.grad), p(self.out),
                      *ws, st)
        if self.row['family'] == 'stein':      # (flags = 0: the call prepares the per-node tables itself; no wmax)
            short, d = self.row['entry'].split('_pdiv_')[1], g['shape'][0]
            if short == 'bwd':
                return fn(self.dtc, p(i['x']), p(i['side']), n, d, rb, re, 1, SPD_WMIN, p(self.grad), *ws, 0, st)
            if short == 'bwd_subset':
                return fn(self.dtc, p(i['x']), p(i['side']), nt, d, p(i['idx']), n, rb, re, 1, SPD_WMIN, p(self.grad), *ws, 0, st)
            if short == 'loss':
                return fn(self.dtc, B.LOSS_STRESS, p(i['x']), p(i['side']), p(i['scale']), n, d, rb, re, 1.0, 1.0, 3, None, SPD_WMIN, p(self.out),
                          p(self.grad), *ws, 0, st)
            return fn(self.dtc, B.LOSS_STRESS, p(i['x']), p(i['side']), p(i['scale']), nt, d, p(i['idx']), n, rb, re, 1.0, 1.0, 3, None, SPD_WMIN,
                      p(self.out), p(self.grad), *ws, 0, st)
        short = self.row['entry'].split('_pdist_')[1]
        if self.row['family'] == 'spd':      # (flags = 0: the call prepares the per-node tables itself; ws, then det_ws)
            if short == 'loss_subset':
                return fn(self.dtc, B.LOSS_STRESS, p(i['x']), p(i['side']), p(i['scale']), nt, g['shape'][0], p(i['idx']), n, rb, re, 1.0, 1.0, 3,
                          None, SPD_WMIN, SPD_WMAX, p(self.out), p(self.grad), *ws, 0, st)
            if short in ('bwd', 'bwd_det'):
                return fn(self.dtc, p(i['x']), p(i['side']), n, g['shape'][0], rb, re, 1, SPD_WMIN, SPD_WMAX, p(self.grad), *ws, 0, st)
            return fn(self.dtc, B.LOSS_STRESS, p(i['x']), p(i['side']), p(i['scale']), n, g['shape'][0], rb, re, 1.0, 1.0, 3, None, SPD_WMIN,
                      SPD_WMAX, p(self.out), p(self.grad), *ws, 0, st)
        if self.row['family'] == 'vec':
            kind, m = R_KIND[g['kind']], g['m']
            if short in ('bwd', 'bwd_det', 'bwd_gram'):
                return fn(self.dtc, kind, p(i['x']), p(i['side']), n, m, rb, re, 1, p(self.grad), *ws, st)
            if short in ('loss', 'loss_det'):
                return fn(self.dtc, kind, B.LOSS_STRESS, p(i['x']), p(i['side']), p(i['scale']), n, m, rb, re, 1.0, 1.0, 3, None, p(self.out),
                          p(self.grad), *ws, st)
            return fn(self.dtc, kind, B.LOSS_STRESS, p(i['x']), p(i['side']), p(i['scale']), nt, m, p(i['idx']), n, rb, re, 1.0, 1.0, 3, None,
                      p(self.out), p(self.grad), *ws, st)
        shape = g['shape']
        if short == 'bwd':
            return fn(self.dtc, p(i['x']), p(i['side']), n, *shape, rb, re, 1, p(self.grad), *ws, st)
        if short == 'bwd_subset':
            return fn(self.dtc, p(i['x']), p(i['side']), nt, *shape, p(i['idx']), n, rb, re, 1, p(self.grad), *ws, st)
        if short == 'loss':
            return fn(self.dtc, B.LOSS_STRESS, p(i['x']), p(i['side']), p(i['scale']), n, *shape, rb, re, 1.0, 1.0, 3, None, p(self.out), p(self.grad),
                      *ws, st)
        return fn(self.dtc, B.LOSS_STRESS, p(i['x']), p(i['side']), p(i['scale']), nt, *shape, p(i['idx']), n, rb, re, 1.0, 1.0, 3, None, p(self.out),
                  p(self.grad), *ws, st)

    def device_result(self):
        if self.curv:
            return (self.out[:1].clone(), self.grad.clone())
        return (self.out[:2 if self.has_scale else 1].clone(), self.grad.clone()) if self.has_loss else (self.grad.clone(), )

    def result(self):
        """{quantity: fp64 array}"""
        out = {'grad': self.grad.double().cpu().numpy()}
        if self.curv:
            out['grad_c'] = self.out.double().cpu().numpy()[:1].copy()
        if self.has_loss:
            o = self.out.double().cpu().numpy()
            out['loss'] = o[:1].copy()
            if self.has_scale:
                out['scale_grad'] = o[1:].copy()
        return out


class ProductBuffers:
    """The same for a product row: one table (mm_product_loss: one vector of squared pair distances) and one gradient per factor,
    a loss record of 1 + nf values.  The pair entries are called with flags = 0: the call clears what it needs."""
    WMIN, WMAX = 1e-8, 1e8          # the SPD factor's eigenvalue clamps, never binding (tests/test_product_oracle_gpu.py)

    def __init__(self, row, ws=None):
        import ctypes
        B = _B()
        self.row, self.dt, self.g = row, DT[row['dname']], row['geometry']
        self.dtc = B.MM_F32 if row['dname'] == 'f32' else B.MM_F64
        dev = lambda v, dt: torch.from_numpy(np.array(v)).to(device='cuda', dtype=dt)      # noqa: E731
        a = R.inputs(row, 'a')
        k = self.k = len(self.g['factors'])
        self.xs = [dev(x, self.dt) for x in a['xs']]
        self.side = dev(a['side'], self.dt)
        self.scales = [dev(a['scales'][j:j + 1], self.dt) for j in range(k)]
        self.inp = {'idx': None if a['idx'] is None else dev(a['idx'], torch.int64)}
        self.grads = [torch.empty_like(x) for x in self.xs]
        self.out = torch.empty(1 + k, dtype=self.dt, device='cuda')
        self.kinds = (ctypes.c_int * k)(*[B.FACTOR_SPD if f == 'spd' else R_KIND[f] for f, _ in self.g['factors']])
        self.dims = (ctypes.c_int * k)(*[d for _, d in self.g['factors']])
        self.pairs_only = row['entry'] == 'mm_product_loss'
        if ws is None:
            raw = B.lib().raw
            nbytes = raw('mm_product_loss_ws_bytes')(self.dtc, k) if self.pairs_only else \
                raw('mm_product_pairs_ws_bytes')(self.dtc, k, self.kinds, self.dims, self.g['n'])
            ws = {'ws': torch.empty(nbytes, dtype=torch.uint8, device='cuda')}
        self.ws = ws

    def load(self, which):
        v = R.inputs(self.row, which)
        for t, x in zip(self.xs, v['xs']):
            t.copy_(torch.from_numpy(np.array(x)).to(t.dtype))
        self.side.copy_(torch.from_numpy(np.array(v['side'])).to(self.dt))
        for j, t in enumerate(self.scales):
            t.fill_(float(v['scales'][j]))

    def dirty(self, keep_ws=False):
        contract = self.row['buffers'].get('grad', (R.ANY, ))[0]
        for t in self.grads:
            t.fill_(0.0 if contract == R.ZERO else float('nan'))      # ("pass zero-filled": exactly that, and nothing more)
        self.out.fill_(float('nan'))
        if not keep_ws:
            self.ws['ws'].fill_(0xFF)

    def enqueue(self):
        B = _B()
        g, p, pa = self.g, B.ptr, B.ptr_array
        fn, st, n = B.lib().raw(self.row['entry']), B.stream_of(self.side), g['n']
        if self.pairs_only:
            return fn(self.dtc, B.LOSS_STRESS, self.k, pa(self.xs), p(self.side), pa(self.scales), n * (n - 1) // 2, 1.0, 1.0, 3, None,
                      pa(self.grads), p(self.out), p(self.ws['ws']), st)
        head = (self.dtc, B.LOSS_STRESS, self.k, self.kinds, self.dims, pa(self.xs), pa(self.scales), p(self.side))
        tail = (1.0, 1.0, 3, None, self.WMIN, self.WMAX, pa(self.grads), p(self.out), p(self.ws['ws']), 0, st)
        if self.row['minibatch']:
            return fn(*head, g['n_total'], p(self.inp['idx']), n, 0, n, *tail)
        return fn(*head, n, 0, n, *tail)

    def device_result(self):
        return (self.out.clone(), ) + tuple(t.clone() for t in self.grads)

    def result(self):
        gk, sk = R._product_keys(self.g['factors'])
        o = self.out.double().cpu().numpy()
        out = {'loss': o[:1].copy()}
        for j in range(self.k):
            out[gk[j]], out[sk[j]] = self.grads[j].double().cpu().numpy(), o[1 + j:2 + j].copy()
        return out


class StereoProductBuffers:
    """The same for a product of constant-curvature factors: per factor a table, a raw curvature, a gradient table and a one-element
    curvature gradient; the factor list is host memory read at call time (tests/test_stereo_product_gpu.py: abi_loss)."""

    def __init__(self, row, ws=None):
        B = _B()
        self.row, self.dt, self.g = row, DT[row['dname']], row['geometry']
        self.dtc = B.MM_F32 if row['dname'] == 'f32' else B.MM_F64
        dev = lambda v, dt: torch.from_numpy(np.array(v)).to(device='cuda', dtype=dt)      # noqa: E731
        a = R.inputs(row, 'a')
        self.k = len(self.g['ms'])
        self.xs = [dev(x, self.dt) for x in a['xs']]
        self.cs = [dev(a['scales'][j:j + 1], self.dt) for j in range(self.k)]
        self.side = dev(a['side'], self.dt)
        self.inp = {'idx': None if a['idx'] is None else dev(a['idx'], torch.int64)}
        self.grads = [torch.empty_like(x) for x in self.xs]
        self.gcs = [torch.empty(1, dtype=self.dt, device='cuda') for _ in self.xs]
        self.out = torch.empty(1, dtype=self.dt, device='cuda')
        self.ms = (B._c.c_int32 * self.k)(*self.g['ms'])
        if ws is None:
            ws = {'ws': torch.empty(B.lib().raw('mm_stereo_product_ws_bytes')(self.dtc, self.g['n'], self.k, self.ms), dtype=torch.uint8, device='cuda')}
        self.ws = ws

    def load(self, which):
        v = R.inputs(self.row, which)
        for t, x in zip(self.xs, v['xs']):
            t.copy_(torch.from_numpy(np.array(x)).to(t.dtype))
        self.side.copy_(torch.from_numpy(np.array(v['side'])).to(self.dt))
        for j, t in enumerate(self.cs):
            t.fill_(float(v['scales'][j]))

    def dirty(self, keep_ws=False):
        for t in self.grads + self.gcs + [self.out]:
            t.fill_(float('nan'))
        if not keep_ws:
            self.ws['ws'].fill_(0xFF)

    def enqueue(self):
        B = _B()
        g, p, n = self.g, B.ptr, self.g['n']
        fs = B.stereo_factors([(x, c, gx, gc, STEREO_C_MIN, m, md) for x, c, gx, gc, m, md in
                               zip(self.xs, self.cs, self.grads, self.gcs, g['ms'], g['c_modes'])])
        fn, st = B.lib().raw(self.row['entry']), B.stream_of(self.side)
        if self.row['minibatch']:
            return fn(self.dtc, B.LOSS_STRESS, fs, self.k, p(self.side), g['n_total'], p(self.inp['idx']), n, 0, n, 1.0, 0.5, 0, None, p(self.out),
                      p(self.ws['ws']), st)
        return fn(self.dtc, B.LOSS_STRESS, fs, self.k, p(self.side), n, 0, n, 1.0, 0.5, 0, None, p(self.out), p(self.ws['ws']), st)

    def device_result(self):
        return (self.out.clone(), ) + tuple(t.clone() for t in self.grads + self.gcs)

    def result(self):
        out = {'loss': self.out.double().cpu().numpy().copy()}
        for j in range(self.k):
            out[f'grad/{j}'], out[f'grad_c/{j}'] = self.grads[j].double().cpu().numpy(), self.gcs[j].double().cpu().numpy()
        return out


def stein_old_route(row, which):
    """{quantity: deviation from the oracle} of the route before the fused Stein kernels (the forward kernel, the loss in torch
    ops, autograd through the backward kernel: tests/test_stein_loss_gpu.py) on this GPU — the e_old of stein_cases' rule"""
    import stein_cases as T
    import test_stein_loss_gpu as TS
    g, regime, dname = row['geometry'], row[which]['regime'], row['dname']
    x = T.points(regime, g['n_total'], g['shape'][0])
    idx = T.batch_idx(g['n']) if row['minibatch'] else None
    if g['loss']:
        if idx is None:
            tg = T.targets(regime, g['n'], g['shape'][0])
        else:
            a, b = T.ref.triu_pairs(g['n'])
            tg = T.dense(regime, g['shape'][0], g['n'])[idx[a], idx[b]].double()
        old = dict(zip(('loss', 'grad', 'scale_grad'), TS.old_route(dname, x, tg, 'stress', idx=idx)))
    else:
        every = torch.arange(g['n']) if idx is None else idx
        old = {'grad': TS.old_pdiv(dname, x, every, True, T.upstream(g['n'] * (g['n'] - 1) // 2))[1]}
    torch.cuda.synchronize()
    want = R.want(row, which)
    return {q: float(np.abs(old[q].detach().double().cpu().numpy().reshape(-1) - want[q].reshape(-1)).max()) for q in want}


def make_buffers(row, ws=None):
    if row['family'] == 'stereo' and row['entry'] != 'mm_stereo_pdist_bwd':
        return StereoProductBuffers(row, ws)
    return (ProductBuffers if row['family'] == 'product' else Buffers)(row, ws)


R_KIND = {'euclidean': 0, 'lorentz': 1, 'sphere': 2}      # MM_EUCLIDEAN, MM_LORENTZ, MM_SPHERE
SPD_WMIN, SPD_WMAX = 1e-8, 1e8                             # spd_det_cases.WMIN, WMAX: the eigenvalue window, never binding
STEREO_C_MIN = 0.001                                       # stereo_cases.C_MIN
SNE_ALPHA = 1.3                                           # sne_cases.ALPHA, sst_cases.ALPHA


def _hold(row, which, stage, buf, eager, failures):
    """one result against the oracle of the case that was loaded and against the eager result of the same case; prints every
    figure before it judges"""
    got, dev = buf.result(), buf.device_result()
    tag = f"{row['id']} {stage} [{which.upper()}]"
    for q, t in got.items():
        if not np.isfinite(t).all():
            failures.append(f'{tag}: {q} holds {int((~np.isfinite(t)).sum())} non-finite elements of {t.size} (an output element left NaN)')
    errs = R.judge(row, which, got, getattr(buf, 'e_old', {}).get(which))
    e_now = R.deviations(row, which, got)
    ratios = {q: (e / b if b > 0 else (0.0 if e == 0 else float('inf'))) for q, (e, b) in errs.items()}
    ratios2 = dict.fromkeys(errs, 0.0)
    line = f'{tag}: ' + ', '.join(f'{q} {e:.3e} / {b:.3e} = {ratios[q]:.3f}' for q, (e, b) in errs.items())
    if eager is not None:
        e_eager, dev_eager = eager[which]
        if row['deterministic']:
            same = all(torch.equal(a, b) for a, b in zip(dev, dev_eager))
            line += ' | the same bits as the eager call' if same else ' | OTHER BITS than the eager call'
            if not same:
                failures.append(f'{tag}: a kernel without float atomics returns other bits replayed than eagerly')
        else:
            allow = R.replay_allowance(row, which, e_eager)
            ratios2 = {q: e_now[q] / max(allow[q], 1e-300) for q in e_now}
            line += ' | against eager: ' + ', '.join(f'{q} e {e_now[q]:.3e} e_eager {e_eager[q]:.3e} allowed {allow[q]:.3e}' for q in e_now)
            for q in e_now:
                if not e_now[q] <= allow[q]:
                    failures.append(f'{tag}: {q}: e_replay {e_now[q]:.3e} > 2 e_eager + 64 eps max|oracle| = {allow[q]:.3e}')
    print(line)
    for q, (e, b) in errs.items():
        if not e <= b:
            failures.append(f'{tag}: {q}: {e:.3e} > {b:.3e}, the bound of {row["module"]}')
        RECORDS.append((row['family'], row['dname'], stage, row['id'], q, ratios[q], ratios2[q]))
    if row['minibatch']:
        rest = torch.ones(buf.g['n_total'], dtype=torch.bool, device='cuda')
        rest[buf.inp['idx']] = False
        for outside in (t[rest] for t in getattr(buf, 'grads', None) or [buf.grad]):
            if not plus_zero(outside):
                failures.append(f'{tag}: gradient rows outside the batch are not exactly +0: {_bits(outside)}')
    return e_now, dev


def _bits(t):
    """how many elements are not +0, and the bit patterns of the first few"""
    words = t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).reshape(-1)
    bad = words[words != 0]
    width = 8 if t.dtype == torch.float32 else 16
    shown = ', '.join(f'0x{int(w) & ((1 << 4 * width) - 1):0{width}x}' for w in bad[:4].cpu().tolist())
    return f'{bad.numel()} of {words.numel()} elements are not +0; the first hold {shown}'


def _warm_up_and_capture(calls):
    """one warm-up of the calls on a side stream, then the calls alone in a graph on a single stream"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for c in calls:
            assert c.enqueue() == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        codes = [c.enqueue() for c in calls]
    assert codes == [0] * len(calls), codes      # the call returns 0 while capturing
    return graph


def run_row(row, failures):
    buf = make_buffers(row)
    if row['family'] == 'stein':
        buf.e_old = {which: stein_old_route(row, which) for which in ('a', 'b')}
    # 1. eager: both cases against their oracles; the eager errors and bits are kept
    eager = {}
    for which in ('a', 'b'):
        buf.load(which)
        buf.dirty()
        rc = buf.enqueue()
        torch.cuda.synchronize()
        assert rc == 0, (row['id'], rc)
        eager[which] = _hold(row, which, STAGES[0], buf, None, failures)
    # 2. capture the call alone
    buf.load('a')
    buf.dirty()
    graph = _warm_up_and_capture([buf])
    # 3. three replays: A, B, A
    for k, which in enumerate(('a', 'b', 'a')):
        buf.load(which)
        buf.dirty(keep_ws=row['keep_ws'] and k == 2)      # (SPD: A's call finds the workspace as B's replay left it)
        graph.replay()
        torch.cuda.synchronize()
        _hold(row, which, STAGES[1 + k], buf, eager, failures)
    del graph
    # 4. two consecutive calls in one graph: A's buffers, then a second set holding B; one workspace, cleared twice inside the graph
    if row['unroll']:
        second = make_buffers(row, ws=buf.ws)
        second.e_old = getattr(buf, 'e_old', {})
        buf.load('a')
        second.load('b')
        buf.dirty()
        second.dirty(keep_ws=True)
        graph = _warm_up_and_capture([buf, second])
        for k in range(2):
            buf.dirty()
            second.dirty(keep_ws=True)
            graph.replay()
            torch.cuda.synchronize()
            _hold(row, 'a', STAGES[4 + k], buf, eager, failures)
            _hold(row, 'b', STAGES[4 + k], second, eager, failures)
        del graph


@pytest.mark.parametrize('family,dname', R.GROUPS, ids=[f'{f}-{d}' for f, d in R.GROUPS])
def test_three_replays_against_the_oracle(family, dname):
    failures = []
    rows = [r for r in R.ROWS if (r['family'], r['dname']) == (family, dname)]
    assert rows
    for row in rows:
        run_row(row, failures)
    assert not failures, '\n'.join(failures)


def test_print_worst_ratios():
    """(last in the file) per family, dtype and stage the worst err / bound and the worst e_replay / (2 e_eager + 64 eps max|oracle|)"""
    worst = {}
    for family, dname, stage, rid, q, r1, r2 in RECORDS:
        w = worst.setdefault((family, dname, stage), [0.0, 0.0, 0, ''])
        if r1 > w[0]:
            w[3] = f'{rid} {q}'
        w[0], w[1], w[2] = max(w[0], r1), max(w[1], r2), w[2] + 1
    print('family | dtype | stage | comparisons | worst err / bound | worst e_replay / allowance | where')
    for (family, dname, stage), (r1, r2, count, where) in sorted(worst.items(), key=lambda kv: (kv[0][0], kv[0][1], STAGES.index(kv[0][2]))):
        print(f'{family} | {dname} | {stage} | {count} | {r1:.3f} | {r2:.3f} | {where}')
    assert all(w[0] <= 1.0 and w[1] <= 1.0 for w in worst.values()), {k: v for k, v in worst.items() if not (v[0] <= 1.0 and v[1] <= 1.0)}
