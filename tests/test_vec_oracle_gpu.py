"""Every instantiation of the vector-manifold pair kernels (csrc/vec.hip: vec_pdist_fwd_kernel, vec_pdist_bwd_kernel — ordered
pairs and node minibatches —, vec_pdist_finalize_kernel; csrc/vec_sym.hpp: vec_sym_prep_kernel, vec_pdist_bwd_sym_kernel;
csrc/vec_gram.hip, vec_gram_bwd64.hpp: the matrix-core forward and backward kernels) against the fp64 oracle (oracle/exact.c
through oracle.step), through the C ABI as a caller goes: mm_vec_pdist_fwd, _fwd_gram, _bwd, _bwd_gram, _loss and _loss_subset on
a workspace of mm_vec_pdist_ws_bytes.  The cases are the enumerated table of tests/vec_cases.py (every width class at both
ends; which instantiations a case launches under an environment is `vec_cases.route`, held equal to the library's kernel list by
tests/test_vec_cases_host.py); the tolerances are the project's existing ones (vec_cases.ABS / REL / GREL / TOL).

The library reads the switches that choose the form once per process, so the module tests the environment it finds itself in,
and one driver per environment of vec_cases.ENVS starts it again in a fresh child.  Every comparison prints `err / bound`;
-rA shows the ratios (profiles/vec_oracle.md)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import vec_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'f64': torch.float64}
CURRENT = {k: os.environ[k] for k in vc.ENV_KEYS if os.environ.get(k)}       # the environment this process runs under
GROUPS = [(entry, dname) for entry in vc.ENTRIES for dname in ('f32', 'f64')]
UNSUPPORTED = -2      # MM_ERR_UNSUPPORTED
# Float atomics decide the order of the sums in every backward form (ordered VALU: the accumulators; symmetric VALU and the
# matrix cores: the gradient itself; all: the loss slots): two calls agree within twice the bound.  The forward kernels have
# none: two calls give the same bits.
BITWISE = ('fwd', 'fwd_gram')


def _dev(a, dt):
    return torch.from_numpy(np.array(a)).to(device='cuda', dtype=dt)      # (a copy: the table's arrays are read-only)


class Call:
    """The device buffers of one case and its call into the library."""

    def __init__(self, c):
        from graphembed import _backend as B
        self.c, self.dt, self.inp = c, DT[c['dname']], vc.inputs(c)
        self.dtc = B.MM_F32 if c['dname'] == 'f32' else B.MM_F64
        self.x = _dev(self.inp['x'], self.dt)
        self.n = c['batch'] or c['n']
        self.ws = None
        if c['entry'] in ('bwd', 'loss', 'subset'):
            nbytes = B.lib().raw('mm_vec_pdist_ws_bytes')(self.dtc, self.x.shape[0], c['m'])
            self.ws = torch.full((nbytes, ), 255, dtype=torch.uint8, device='cuda')      # the library clears what it needs
        self.scale = torch.tensor([self.inp['scale']], dtype=self.dt, device='cuda') if c['loss'] and c['scale'] else None
        self.idx = None if self.inp['idx'] is None else torch.from_numpy(self.inp['idx']).cuda()
        self.side = {k: (None if self.inp[k] is None else _dev(self.inp[k], self.dt)) for k in ('g', 'target', 'dense')}

    def run(self):
        """(return code, what vec_cases.evaluate describes, as numpy fp64)"""
        from graphembed import _backend as B
        c, dt, lib, x = self.c, self.dt, B.lib(), self.x
        kind, m, sq = vc.KIND_CODE[c['kind']], c['m'], int(c['squared'])
        rb, re = c['rows'] or (0, self.n)
        stream = B.stream_of(x)
        some = lambda t: B.ptr(t) if t is not None and t.numel() else None      # noqa: E731
        if c['entry'] in ('fwd', 'fwd_gram'):
            lo, hi = (0, 0) if c['n'] > vc.GRAM_MAX_N else vc.pair_slice(c)      # (the refusals by size: no pair vector)
            out = torch.full((hi - lo, ), float('nan'), dtype=dt, device='cuda')      # a pair the kernel never wrote is seen
            rc = lib.raw('mm_vec_pdist_' + c['entry'])(self.dtc, kind, B.ptr(x), self.n, m, rb, re, sq, some(out), stream)
            torch.cuda.synchronize()
            return rc, out.double().cpu().numpy()
        if c['entry'] in ('bwd', 'bwd_gram'):
            grad = torch.full_like(x, float('nan'))      # a row the kernels never wrote is seen
            tail = (B.ptr(grad), B.ptr(self.ws), stream) if c['entry'] == 'bwd' else (B.ptr(grad), stream)
            rc = lib.raw('mm_vec_pdist_' + c['entry'])(self.dtc, kind, B.ptr(x), some(self.side['g']), self.n, m, rb, re, sq, *tail)
            torch.cuda.synchronize()
            return rc, grad.double().cpu().numpy()
        loss = vc.loss_of(c)
        code = vc.LOSS_CODE[loss['kind']]
        alpha, eps = float(loss.get('alpha', 1.0)), 1.0 / (loss.get('epoch', 0) + 1)
        out = torch.full((2, ), float('nan'), dtype=dt, device='cuda')
        if c['entry'] == 'subset':
            grad = torch.zeros_like(x)      # full-size, zero-filled: rows outside the batch must stay exactly zero
            rc = lib.raw('mm_vec_pdist_loss_subset')(self.dtc, kind, code, B.ptr(x), some(self.side['dense']), some(self.scale), x.shape[0], m,
                                                     some(self.idx), self.n, rb, re, alpha, eps, vc.terms_of(c), None, B.ptr(out),
                                                     B.ptr(grad), B.ptr(self.ws), stream)
        else:
            grad = torch.full_like(x, float('nan'))
            rc = lib.raw('mm_vec_pdist_loss')(self.dtc, kind, code, B.ptr(x), some(self.side['target']), some(self.scale), self.n, m, rb, re,
                                              alpha, eps, vc.terms_of(c), None, B.ptr(out), B.ptr(grad), B.ptr(self.ws), stream)
        torch.cuda.synchronize()
        o = out.double().cpu().numpy()
        return rc, (float(o[0]), grad.double().cpu().numpy(), float(o[1]))


def _compare(tag, c, want, got, failures, worst, scale=1.0, bounds=None):
    """Prints err / bound per quantity; `bounds`: {quantity: allowed} in place of the case's own; `scale` multiplies them."""
    errs = vc.errors(c, want, got)
    if bounds is not None:
        errs = {q: (e, bounds[q]) for q, (e, _) in errs.items()}
    errs = {q: (e, a * scale) for q, (e, a) in errs.items()}
    ratios = vc.worst(errs)
    print(f'{tag}: ' + ', '.join(f'{q} {r:.3f}' for q, r in ratios.items()))
    for q, r in ratios.items():
        worst[q] = max(worst.get(q, 0.0), r)
        if not r <= 1.0:
            failures.append(f'{tag}, {q}, {errs[q][0]:.3e} / {errs[q][1]:.3e}')


def _untouched(got):
    arrays = [got] if isinstance(got, np.ndarray) else [np.asarray(got[0]), got[1], np.asarray(got[2])]
    return all(np.isnan(a).all() or not a.any() for a in arrays)


@pytest.mark.parametrize('entry,dname', GROUPS, ids=[f'{e}-{d}' for e, d in GROUPS])
def test_vector_pair_kernels_vs_fp64_oracle(entry, dname):
    env = vc.env_id(CURRENT)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = [c for c in vc.cases_for(CURRENT) if (c['entry'], c['dname']) == (entry, dname)]
    failures, worst, results, calls = [], {}, {}, {}
    for c in cases:
        names = vc.route_of(c, CURRENT)
        form = vc.form_of(names)
        tag = f'[{env}] {c["id"]} -> {" + ".join(names) or "MM_ERR_UNSUPPORTED"}'
        call = Call(c)
        rc, got = call.run()
        if c['refuse']:      # a refusal is a refusal: the code, and nothing written
            print(f'{tag}: return code {rc}')
            if rc != UNSUPPORTED or not _untouched(got):
                failures.append(f'{tag}: return code {rc}, outputs {"untouched" if _untouched(got) else "written"}')
            continue
        if rc != 0:
            failures.append(f'{tag}: return code {rc}')
            continue
        results[c['id']] = got
        if c['primary'] and (c['n'] == vc.N or c['batch']) and c['rows'] is None:
            calls[c['id']] = call
        if entry == 'fwd':
            tag += f' (rows per tile {vc.fwd_tile_height(c["n"], *(c["rows"] or (0, c["n"])), cus)} on {cus} CUs)'
        _compare(tag, c, vc.expected(c), got, failures, worst.setdefault(form, {}))
        if c['batch']:      # rows outside the batch stay exactly zero
            rest = np.ones(vc.N_TABLE, dtype=bool)
            rest[call.inp['idx']] = False
            if got[1][rest].any():
                failures.append(f'{tag}: gradient rows outside the batch were written')
    for c in cases:
        if c['id'] not in calls:
            continue
        form = vc.form_of(vc.route_of(c, CURRENT))
        first = results[c['id']]
        # the same call again
        rc, again = calls[c['id']].run()
        assert rc == 0, (c['id'], rc)
        if entry in BITWISE:
            print(f'[{env}] {c["id"]} second call: {"the same bits" if np.array_equal(first, again) else "OTHER BITS"}')
            if not np.array_equal(first, again):
                failures.append(f'{c["id"]}: two calls of a kernel without atomics differ')
        else:
            own = {q: a for q, (_, a) in vc.errors(c, vc.expected(c), first).items()}
            _compare(f'[{env}] {c["id"]} second call against the first', c, first, again, failures, worst.setdefault(form + ' repeat / 2', {}),
                     scale=2.0, bounds=own)
        # the row shards against the whole: each is within its own bound of its own oracle, and the oracles add up exactly
        # (tests/test_vec_cases_host.py), so the device's sum is within the sum of the bounds of the device's whole
        if c['batch'] or not c['scale']:
            continue
        parts = vc.parts_of(c)
        if not all(p['id'] in results for p in parts):
            continue
        if entry in BITWISE:
            same = np.array_equal(np.concatenate([results[p['id']] for p in parts]), first)
            print(f'[{env}] {c["id"]} shards concatenated: {"the same bits" if same else "OTHER BITS"}')
            if not same:
                failures.append(f'{c["id"]}: the shards of the forward are not the whole')
            continue
        bound = {q: sum(vc.errors(p, vc.expected(p), results[p['id']])[q][1] for p in parts + [c]) for q in vc.errors(c, vc.expected(c), first)}
        if c['loss']:
            summed = tuple(sum(results[p['id']][k] for p in parts) for k in range(3))
        else:
            summed = sum(results[p['id']] for p in parts)
        _compare(f'[{env}] {c["id"]} shards summed against the whole', c, first, summed, failures, worst.setdefault(form + ' shards', {}),
                 bounds=bound)
    for form, w in sorted(worst.items()):
        print(f'[worst] {env} {entry} {dname} {form}: ' + ', '.join(f'{q} {r:.3f}' for q, r in sorted(w.items())))
    assert not failures, '\n'.join(failures)


# ------------------------------------------------------------------------------------------- the other environments, in children
# Seconds a child may take.  First run on an MI355X (profiles/vec_oracle.md): 3.9 ... 5.4 s per child, of which ~1 s are the
# tests and the rest the interpreter's start (torch, the library, the oracle).  Ten times that is under the floor of 60 s: a
# child that hangs still ends within a minute.
CHILD_TIMEOUT = {vc.env_id(e): 60 for e in vc.ENVS}
_DIED = []      # a child that aborted, crashed or hung: no further child is started


@pytest.mark.parametrize('env', vc.ENVS, ids=[vc.env_id(e) for e in vc.ENVS])
def test_vector_pair_kernels_vs_fp64_oracle_in_a_fresh_child(env):
    """This module again under `env` (its direct tests only: `-k 'not fresh_child'`), one child after another."""
    if env == CURRENT:
        return      # this process IS that environment: the direct tests above are its run
    if _DIED:
        pytest.fail(f'not started: an earlier child died ({_DIED[0]})')
    e = {k: v for k, v in os.environ.items() if k not in vc.ENV_KEYS}
    e.update(env)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-x', '-q', '-rA', '-m', 'gpu', '-k', 'not fresh_child',
                            '-p', 'no:cacheprovider'], env=e, capture_output=True, text=True, timeout=CHILD_TIMEOUT[vc.env_id(env)], cwd=ROOT)
    except subprocess.TimeoutExpired:
        _DIED.append(f'{vc.env_id(env)}: no end within {CHILD_TIMEOUT[vc.env_id(env)]} s')
        pytest.fail(_DIED[0])
    print(f'child {vc.env_id(env)}: {time.time() - t0:.1f} s, exit status {r.returncode}')
    print('\n'.join(ln for ln in r.stdout.splitlines() if ln.startswith('[worst]') or ' passed' in ln or ' failed' in ln))
    if r.returncode in (134, 139, 124, 137) or r.returncode < 0:
        _DIED.append(f'{vc.env_id(env)}: exit status {r.returncode}')
        pytest.fail(_DIED[0] + '\n' + r.stdout[-3000:] + r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'skipped' not in r.stdout.splitlines()[-1], r.stdout[-500:]
