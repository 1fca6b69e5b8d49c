"""Every instantiation of the mixed-manifold pair kernels (csrc/product_pairs.hip: product_pair_kernel<T, NV, SD, LOSS, PW, IDX,
KC>; csrc/product_sym.hip: product_sym_kernel<T, NV, SD, LOSS, KC>) against the fp64 oracle (oracle.step.objective: oracle/exact.c
per factor), through the C ABI as a caller goes: mm_product_pairs_loss and mm_product_pairs_loss_subset on a workspace of
mm_product_pairs_ws_bytes.  The cases are the enumerated table of tests/product_cases.py (one per instantiation; which one a
case takes under an environment is `product_cases.route`, held equal to the library's kernel list by
tests/test_product_cases_host.py); the tolerances are step_cases.TOL.

The library reads the switches that choose the form once per process, so the module tests the environment it finds itself in,
and one driver per environment of product_cases.ENVS starts it again in a fresh child.  Every comparison prints
`err / bound`; -rA shows the ratios (profiles/product_oracle.md)."""
import ctypes
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

import product_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'f64': torch.float64}
CURRENT = {k: os.environ[k] for k in pc.ENV_KEYS if os.environ.get(k)}       # the environment this process runs under
GROUPS = sorted({(c['nv'], c['sd'], c['dname']) for c in pc.CASES})
WMIN, WMAX = 1e-8, 1e8          # the SPD manifold's eigenvalue clamps (never binding here), as the oracle's
WS_PREPARED, WS_CLEAN = 1, 2    # MM_WS_PREPARED, MM_WS_CLEAN


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device='cuda', dtype=dt)


class Call:
    """The device buffers of one case and its call into the library."""

    def __init__(self, c):
        from graphembed import _backend as B
        self.c, self.dt, self.inp = c, DT[c['dname']], pc.inputs(c)
        k = len(c['factors'])
        self.kinds = (ctypes.c_int * k)(*[B.FACTOR_SPD if f == 'spd' else pc.KIND_CODE[f] for f, _ in c['factors']])
        self.dims = (ctypes.c_int * k)(*[d for _, d in c['factors']])
        self.xs = [_dev(x, self.dt) for x in self.inp['xs']]
        self.scales = [torch.tensor([s], dtype=self.dt, device='cuda') for s in self.inp['scales']]
        self.n = c['batch'] or c['n']
        nbytes = B.lib().raw('mm_product_pairs_ws_bytes')(B.MM_F32 if c['dname'] == 'f32' else B.MM_F64, k, self.kinds, self.dims, self.n)
        self.ws = torch.full((nbytes, ), 255, dtype=torch.uint8, device='cuda')      # flags = 0: the library clears what it needs
        self.idx = None if self.inp['idx'] is None else torch.from_numpy(self.inp['idx']).cuda()

    def run(self, flags, targets=None):
        """(loss, [gradient per factor], [d loss / d raw scale]) as numpy fp64; `targets`: those of another case on the same points"""
        from graphembed import _backend as B
        c, dt, lib = self.c, self.dt, B.lib()
        k = len(c['factors'])
        inp = targets or self.inp
        loss = pc.loss_of(c)
        code = pc.LOSS_CODE[loss['kind']]
        alpha, eps = float(loss.get('alpha', 1.0)), 1.0 / (loss.get('epoch', 0) + 1)
        dtc = B.MM_F32 if c['dname'] == 'f32' else B.MM_F64
        out = torch.full((1 + k, ), float('nan'), dtype=dt, device='cuda')
        stream = B.stream_of(self.xs[0])
        if c['batch']:
            dense = _dev(inp['dense'], dt)
            grads = [torch.zeros_like(x) for x in self.xs]      # full-size, zero-filled: the call writes the batch's rows
            rc = lib.raw('mm_product_pairs_loss_subset')(dtc, code, k, self.kinds, self.dims, B.ptr_array(self.xs), B.ptr_array(self.scales),
                                                         B.ptr(dense), pc.N_TABLE, B.ptr(self.idx), self.n, 0, self.n, alpha, eps,
                                                         pc.terms_of(c), None, WMIN, WMAX, B.ptr_array(grads), B.ptr(out), B.ptr(self.ws),
                                                         flags, stream)
        else:
            rb, re = c['rows'] or (0, c['n'])
            target = _dev(inp['target'], dt)
            grads = [torch.full_like(x, float('nan')) for x in self.xs]      # a row the kernels never wrote is seen
            rc = lib.raw('mm_product_pairs_loss')(dtc, code, k, self.kinds, self.dims, B.ptr_array(self.xs), B.ptr_array(self.scales),
                                                  B.ptr(target) if target.numel() else None, self.n, rb, re, alpha, eps, pc.terms_of(c), None,
                                                  WMIN, WMAX, B.ptr_array(grads), B.ptr(out), B.ptr(self.ws), flags, stream)
        assert rc == 0, (c['id'], rc)
        torch.cuda.synchronize()
        o = out.double().cpu().numpy()
        return float(o[0]), [g.double().cpu().numpy() for g in grads], [float(v) for v in o[1:]]


def _compare(tag, c, want, got, failures, worst):
    errs = pc.errors(c, want, got)
    ratios = pc.worst(errs)
    print(f'{tag}: ' + ', '.join(f'{q} {r:.3f}' for q, r in ratios.items()))
    for q, r in ratios.items():
        cls = q.split('/')[0] if not q.startswith('grad/') else ('grad_spd' if ':spd' in q else 'grad_vec')
        worst[cls] = max(worst.get(cls, 0.0), r)
        if not r <= 1.0:
            failures.append(f'{tag}, {q}, {errs[q][0]:.3e} / {errs[q][1]:.3e}')


def _finish(failures):
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('nv,sd,dname', GROUPS, ids=[f'nv{a}-sd{b}-{d}' for a, b, d in GROUPS])
def test_pair_kernels_vs_fp64_oracle(nv, sd, dname):
    env = pc.env_id(CURRENT)
    cases = [c for c in pc.cases_for(CURRENT) if (c['nv'], c['sd'], c['dname']) == (nv, sd, dname)]
    failures, worst, results = [], {}, {}
    for c in cases:
        if c['tdraw']:
            continue       # (the other targets of a workspace-contract case: run below, on the first draw's workspace)
        r = pc.route_of(c, CURRENT)
        w = worst.setdefault(r[0], {})
        tag = f'[{env}] {c["id"]} -> {pc.name(r)}'
        call = Call(c)
        got = results[c['id']] = call.run(0)
        _compare(tag, c, pc.expected(c), got, failures, w)
        if c['batch']:      # rows outside the batch stay exactly zero
            rest = np.ones(pc.N_TABLE, dtype=bool)
            rest[call.inp['idx']] = False
            if any(g[rest].any() for g in got[1]):
                failures.append(f'{tag}: gradient rows outside the batch were written')
        # the workspace contract (include/mm_manifolds.h): the same workspace again with other targets and MM_WS_CLEAN, then —
        # symmetric form: the node table is current — MM_WS_CLEAN | MM_WS_PREPARED; each call against its own oracle
        other = pc.BY_ID.get(pc.case(c['factors'], dname, c['loss'], c['epoch'], tdraw=1)['id'])
        if other is not None and c['primary'] and c['n'] == pc.N and c['rows'] is None and not c['batch'] and 'MM_PRODUCT_TI' not in CURRENT:
            second = pc.inputs(other)
            _compare(f'{tag} second call, MM_WS_CLEAN', other, pc.expected(other), call.run(WS_CLEAN, second), failures, w)
            third = WS_CLEAN | (WS_PREPARED if r[0] == 'sym' else 0)
            _compare(f'{tag} third call, flags {third}', other, pc.expected(other), call.run(third, second), failures, w)
    # the row shards sum to the whole: each is within its own bound of its own oracle, and the oracles add up exactly
    # (tests/test_product_cases_host.py), so the device's sum is within the sum of the bounds of the device's whole
    for c in cases:
        if not (c['primary'] and c['rows'] == pc.shards(pc.N)[0]) or 'MM_PRODUCT_TI' in CURRENT:
            continue
        parts = [pc.BY_ID[pc.case(c['factors'], dname, c['loss'], c['epoch'], rows=r)['id']] for r in pc.shards(pc.N)]
        whole = pc.whole_of(c)
        tot = results[whole['id']]
        bound = {q: sum(pc.errors(p, pc.expected(p), results[p['id']])[q][1] for p in parts + [whole]) for q in pc.errors(whole, pc.expected(whole), tot)}
        summed = (sum(results[p['id']][0] for p in parts), [sum(results[p['id']][1][k] for p in parts) for k in range(len(tot[1]))],
                  [sum(results[p['id']][2][k] for p in parts) for k in range(len(tot[2]))])
        for q, (e, _) in pc.errors(whole, tot, summed).items():
            print(f'[{env}] {whole["id"]} shards summed against the whole: {q} {e / bound[q]:.3f}')
            if not e <= bound[q]:
                failures.append(f'{whole["id"]} shards summed against the whole, {q}, {e:.3e} / {bound[q]:.3e}')
    for form, w in sorted(worst.items()):
        print(f'[worst] {env} {form} nv={nv} sd={sd} {dname}: ' + ', '.join(f'{q} {r:.3f}' for q, r in sorted(w.items())))
    _finish(failures)


# ------------------------------------------------------------------------------------------- the other environments, in children
# seconds a child may take.  First measured runs on an MI355X (profiles/product_oracle.md): 4.2 ... 5.8 s per child, of which
# ~2 s are the tests and the rest the interpreter's start (torch, the library, the oracle).  Ten times that: the start is disk
# and page cache, not the GPU, and varies by more than the tests do; a child that hangs still ends within a minute.
CHILD_TIMEOUT = {'default': 60, 'sym1': 60, 'rt_kinds1': 60, 'rt_kinds1+sym1': 60, 'ti16': 60}
_DIED = []      # a child that aborted, crashed or hung: no further child is started


@pytest.mark.parametrize('env', pc.ENVS, ids=[pc.env_id(e) for e in pc.ENVS])
def test_pair_kernels_vs_fp64_oracle_in_a_fresh_child(env):
    """This module again under `env` (its direct tests only: `-k 'not fresh_child'`), one child after another."""
    if env == CURRENT:
        return      # this process IS that environment: the direct tests above are its run
    if _DIED:
        pytest.fail(f'not started: an earlier child died ({_DIED[0]})')
    e = {k: v for k, v in os.environ.items() if k not in pc.ENV_KEYS}
    e.update(env)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-x', '-q', '-rA', '-m', 'gpu', '-k', 'not fresh_child',
                            '-p', 'no:cacheprovider'], env=e, capture_output=True, text=True, timeout=CHILD_TIMEOUT[pc.env_id(env)], cwd=ROOT)
    except subprocess.TimeoutExpired:
        _DIED.append(f'{pc.env_id(env)}: no end within {CHILD_TIMEOUT[pc.env_id(env)]} s')
        pytest.fail(_DIED[0])
    print(f'child {pc.env_id(env)}: {time.time() - t0:.1f} s, exit status {r.returncode}')
    print('\n'.join(ln for ln in r.stdout.splitlines() if ln.startswith('[worst]') or ' passed' in ln or ' failed' in ln))
    if r.returncode in (134, 139, 124, 137) or r.returncode < 0:
        _DIED.append(f'{pc.env_id(env)}: exit status {r.returncode}')
        pytest.fail(_DIED[0] + '\n' + r.stdout[-3000:] + r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'skipped' not in r.stdout.splitlines()[-1], r.stdout[-500:]
