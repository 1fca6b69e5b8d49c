"""Every (kernel, D, dtype) instantiation of the per-point SPD kernels — spd_dist_fwd_kernel, spd_dist_bwd_kernel, spd_map_kernel,
spd_norm_kernel, spd_eigvalsh_kernel (csrc/spd_pair.hpp), spd_stein_div_kernel (csrc/spd_stein.hpp) and the three optimizer
kernels, D = 2 .. 9, fp32 and fp64: 144 — against oracle.step.ExactSPD in fp64 on the CPU, through the C ABI as a caller goes
(mm_spd_map, mm_spd_norm, mm_spd_eigvalsh, mm_spd_dist_fwd / _bwd, mm_spd_stein_div, mm_spd_rsgd_step, mm_spd_rsgd_momentum_step,
mm_spd_radam_step), under the ABSOLUTE tolerance rule of tests/spd_point_cases.py — built from the reference alone, never from
another GPU route.  One test per (entry point, D, dtype); each also holds
  * the launch edges: m in {0, 1, 127, 128, 129, 130} on the 130-row buffers — rows < m carry the bits of the m = 130 call (these
    kernels have no atomics), rows >= m keep their fill bit for bit, m = 0 returns MM_OK and writes nothing;
  * class <-> ABI: SymmetricPositiveDefinite's exp / log / retr / projx / egrad2rgrad / norm / symeig / dist / stein_div and the
    autograd of the last two return the bits of the ABI call;
  * the optimizer entries in place (x_new == x) give the bits of the out-of-place call, and the Adam step counter advances by one
    per call with the ticket back at zero;
  * every matrix output equals its transpose bit for bit; eigenvalues ascend.
Every comparison prints `err / bound`; -rA shows them and the summary of the last test (profiles/spd_point_oracle.md)."""
import ctypes
import functools
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import spd_point_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

CNT = pc.CNT
GROUPS = [(kernel, D, dname) for kernel in pc.KERNELS for D in pc.DIMS for dname in pc.DNAMES]
assert len(GROUPS) == len(set(GROUPS)) == 144
WMIN, WMAX = 1e-8, 1e8
EDGE_REGIME = 'mid'      # the batch the launch edges, class <-> ABI and in-place runs use
_RAN, REACHED = set(), set()


def _B():
    from graphembed import _backend as B
    return B


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


@functools.lru_cache(maxsize=4)
def _bufs(regime, D, dname):
    dt = pc.DT[dname]
    b = {k: v.to(dt).cuda().contiguous() for k, v in pc.inputs(regime, D).items()}
    b['g'] = pc.upstream(CNT).to(dt).cuda()
    return b


class Call:
    """One variant of one entry point on the buffers of (regime, D, dtype).  launch(m) -> (return code, {output: tensor},
    {output: the tensor's content before the call}); `wants`: {output: (name of the quantity, Quantity, compared rows or None)}."""

    def __init__(self, label, launch, wants, matrices=(), adam=None):
        self.label, self.launch, self.wants, self.matrices, self.adam = label, launch, wants, matrices, adam


def _nan(dt, *shape):
    return torch.full(shape, float('nan'), dtype=dt, device='cuda')


def _calls(kernel, regime, D, dname):
    B = _B()
    raw, ptr = B.lib().raw(pc.KERNELS[kernel]), B.ptr
    dt, b = pc.DT[dname], _bufs(regime, D, dname)
    dtc = B.MM_F32 if dname == 'f32' else B.MM_F64
    stream = B.stream_of(b['x'])
    x, y, g = b['x'], b['y'], b['g']
    held = lambda name: pc.held(name, D, regime)      # noqa: E731
    out = []
    if kernel == 'spd_map_kernel':
        q = pc.map_quantities(regime, D)
        for op, name in enumerate(pc.MAP_OPS):
            first = b['a'] if name == 'projx' else x
            second = {'egrad2rgrad': b['un'], 'proju': b['un'], 'exp': b['ts'], 'retr': b['ts'], 'log': y, 'projx': None}[name]

            def launch(m, op=op, name=name, first=first, second=second):
                o = _nan(dt, CNT, D, D)
                return raw(dtc, op, ptr(first), ptr(second), m, D, WMIN, WMAX, ptr(o), stream), {name: o}, {name: o.clone()}
            out.append(Call(name, launch, {name: (f'map_{name}', q[name], None)}, (name, )))
    elif kernel == 'spd_norm_kernel':
        q = pc.map_quantities(regime, D)
        for squared, name in ((0, 'norm'), (1, 'norm2')):
            def launch(m, squared=squared, name=name):
                o = _nan(dt, CNT)
                return raw(dtc, ptr(x), ptr(b['ts']), m, D, squared, ptr(o), stream), {name: o}, {name: o.clone()}
            out.append(Call(name, launch, {name: (f'map_{name}', q[name], None)}))
    elif kernel == 'spd_eigvalsh_kernel':
        q = pc.map_quantities(regime, D)

        def launch(m):
            o = _nan(dt, CNT, D)
            return raw(dtc, ptr(b['a']), m, D, ptr(o), stream), {'eigvalsh': o}, {'eigvalsh': o.clone()}
        out.append(Call('eigvalsh', launch, {'eigvalsh': ('map_eigvalsh', q['eigvalsh'], None)}))
    elif kernel in ('spd_dist_fwd_kernel', 'spd_dist_bwd_kernel'):
        for windowed in (False, True) if regime in pc.REGIMES else (False, ):
            wmin, wmax = pc.window(regime, D) if windowed else (WMIN, WMAX)
            for squared in (1, 0):
                q = pc.dist_quantities(regime, D, bool(squared), windowed)
                keep = pc.keep_rows(regime, bool(squared))
                pre = f'{"wdist" if windowed else "dist"}_{"d2" if squared else "d"}'
                label = pre + (f' window {wmin:.4g}..{wmax:.4g}' if windowed else '')
                if kernel == 'spd_dist_fwd_kernel':
                    def launch(m, squared=squared, wmin=wmin, wmax=wmax):
                        o = _nan(dt, CNT)
                        return raw(dtc, ptr(x), ptr(y), m, D, squared, wmin, wmax, ptr(o), stream), {'val': o}, {'val': o.clone()}
                    out.append(Call(label, launch, {'val': (f'{pre}_val', q['val'], keep)}))
                else:
                    def launch(m, squared=squared, wmin=wmin, wmax=wmax):
                        gx, gy = _nan(dt, CNT, D, D), _nan(dt, CNT, D, D)
                        rc = raw(dtc, ptr(x), ptr(y), ptr(g), m, D, squared, wmin, wmax, ptr(gx), ptr(gy), stream)
                        return rc, {'grad_x': gx, 'grad_y': gy}, {'grad_x': gx.clone(), 'grad_y': gy.clone()}
                    wants = {n: (f'{pre}_{n}', q[n], keep) for n in ('grad_x', 'grad_y') if pc.held(f'{pre}_{n}', D, regime, windowed)}
                    out.append(Call(label, launch, wants, ('grad_x', 'grad_y')))
    elif kernel == 'spd_stein_div_kernel':
        for squared in (1, 0):
            q = pc.stein_quantities(regime, D, bool(squared))
            keep = pc.keep_rows(regime, bool(squared))
            pre = f'stein_{"d2" if squared else "d"}'

            def value(m, squared=squared):
                o = _nan(dt, CNT)
                return raw(dtc, ptr(x), ptr(y), None, m, D, squared, WMIN, ptr(o), None, None, stream), {'val': o}, {'val': o.clone()}

            def grads(m, squared=squared):
                gx, gy = _nan(dt, CNT, D, D), _nan(dt, CNT, D, D)
                rc = raw(dtc, ptr(x), ptr(y), ptr(g), m, D, squared, WMIN, None, ptr(gx), ptr(gy), stream)
                return rc, {'grad_x': gx, 'grad_y': gy}, {'grad_x': gx.clone(), 'grad_y': gy.clone()}
            out.append(Call(pre + ' value only', value, {'val': (f'{pre}_val', q['val'], keep)}))
            out.append(Call(pre + ' gradients only', grads,
                            {n: (f'{pre}_{n}', q[n], keep) for n in ('grad_x', 'grad_y') if held(f'{pre}_{n}')}, ('grad_x', 'grad_y')))
    else:
        kind = {'spd_rsgd_step_kernel': 'rsgd', 'spd_rsgd_momentum_kernel': 'momentum', 'spd_radam_step_kernel': 'radam'}[kernel]
        for case in pc.STEP_CASES:
            if case[0] != kind:
                continue
            _, exact, clip, t0, nc = case
            q = pc.step_quantities(regime, D, case)
            mgn = pc.step_clip(regime, D) if clip else -1.0

            def launch(m, inplace=False, exact=exact, mgn=mgn, t0=t0, nc=nc, steps=1):
                xin = x.clone() if inplace else x
                xn = xin if inplace else _nan(dt, CNT, D, D)
                outs, fills = {'x_new': xn}, {'x_new': xn.clone()}
                if kind == 'rsgd':
                    rc = raw(dtc, ptr(xin), ptr(b['eg']), m, D, pc.LR, mgn, exact, ptr(xn), stream)
                elif kind == 'momentum':
                    buf = b['buf'].clone()
                    outs['momentum_buffer'], fills['momentum_buffer'] = buf, buf.clone()
                    rc = raw(dtc, ptr(xin), ptr(b['eg']), ptr(buf), m, D, pc.LR, 0.9, 0.1, mgn, exact, ptr(xn), stream)
                else:
                    m1, v2 = b['buf'].clone(), b['v2'].clone()
                    outs.update(exp_avg=m1, exp_avg_sq=v2)
                    fills.update(exp_avg=m1.clone(), exp_avg_sq=v2.clone())
                    step = torch.tensor([float(t0)], dtype=torch.float64, device='cuda')
                    ticket = torch.zeros(1, dtype=torch.int32, device='cuda')
                    for _ in range(steps):
                        rc = raw(dtc, ptr(xin), ptr(b['eg']), ptr(m1), ptr(v2), ptr(step), ptr(ticket), m, D, pc.LR, pc.BETAS[0],
                                 pc.BETAS[1], nc, pc.ADAM_EPS, mgn, exact, ptr(xn), stream)
                    outs['_step'], outs['_ticket'] = step, ticket
                return rc, outs, fills
            wants = {n: (f'step_{kind}_{n}', q[n], pc.step_keep_rows(regime, case, n)) for n in pc.STEP_OUTPUTS[kind]}
            out.append(Call(pc.step_id(case), launch, wants, pc.STEP_OUTPUTS[kind], adam=t0))
    return out


def _through_the_class(kernel, D, dname, call_index):
    """{output: tensor} of the same variant through SymmetricPositiveDefinite, or None where the issue names no method"""
    import graphembed.manifolds as M
    b = _bufs(EDGE_REGIME, D, dname)
    x, y, g = b['x'], b['y'], b['g']
    man = M.SymmetricPositiveDefinite(D)
    if kernel == 'spd_map_kernel':
        name = pc.MAP_OPS[call_index]
        if name == 'proju':
            return None      # (the class forms sym(u) with torch ops)
        with torch.no_grad():
            args = {'egrad2rgrad': (x, b['un']), 'exp': (x, b['ts']), 'retr': (x, b['ts']), 'log': (x, y), 'projx': (b['a'], )}[name]
            return {name: getattr(man, name)(*args)}
    if kernel == 'spd_norm_kernel':
        name = ('norm', 'norm2')[call_index]
        return {name: man.norm(x, b['ts'], squared=bool(call_index))}
    if kernel == 'spd_eigvalsh_kernel':
        with torch.no_grad():
            return {'eigvalsh': man.symeig(b['a'])}
    if kernel in ('spd_dist_fwd_kernel', 'spd_dist_bwd_kernel'):
        windowed, squared = bool(call_index // 2), call_index % 2 == 0
        if windowed:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                wmin, wmax = pc.window(EDGE_REGIME, D)
                man = M.SymmetricPositiveDefinite(D, wmin=wmin, wmax=wmax)
        fn = lambda a, c: man.dist(a, c, squared=squared)      # noqa: E731
    elif kernel == 'spd_stein_div_kernel':
        squared = call_index // 2 == 0
        fn = lambda a, c: man.stein_div(a, c, squared=squared)      # noqa: E731
    else:
        return None
    xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    d = fn(xr, yr)
    gx, gy = torch.autograd.grad((d * g).sum(), [xr, yr])
    return {'val': d.detach(), 'grad_x': gx, 'grad_y': gy}


@pytest.mark.parametrize('kernel,D,dname', GROUPS, ids=[f'{pc.KERNELS[k]}-{D}-{d}' for k, D, d in GROUPS])
def test_point_kernels_vs_fp64_oracle(kernel, D, dname):
    _RAN.add((kernel, D, dname))
    entry = pc.KERNELS[kernel]
    failures = []
    for regime in pc.ALL_REGIMES:
        for ci, call in enumerate(_calls(kernel, regime, D, dname)):
            tag = f'{entry} spd({D}) {regime} {call.label}'
            rc, full, _ = call.launch(CNT)
            torch.cuda.synchronize()
            assert rc == 0, (tag, rc)
            for name, (what, q, keep) in call.wants.items():
                got = full[name] if keep is None else full[name][keep.cuda()]
                pc.check(tag, 'spd_pt_' + what, got, q, dname, failures)
            for name, t in full.items():
                if name.startswith('_'):
                    continue
                if not bool(torch.isfinite(t).all()) and not (regime == 'edge' and call.adam == 1 and 'nc' in call.label):
                    failures.append(f'{tag} {name} {dname}: not finite')      # (the rows left out of the comparison included)
                if name in call.matrices and not _same_bits(t, t.transpose(-1, -2)):
                    failures.append(f'{tag} {name} {dname}: not symmetric bit for bit')
                if name == 'eigvalsh' and not bool((t[:, 1:] >= t[:, :-1]).all()):
                    failures.append(f'{tag} {dname}: eigenvalues do not ascend')
            if call.adam is not None and (float(full['_step']) != call.adam + 1 or int(full['_ticket']) != 0):
                failures.append(f'{tag} {dname}: step {float(full["_step"])} ticket {int(full["_ticket"])} after one call from {call.adam}')
            if regime != EDGE_REGIME:
                continue
            REACHED.add((kernel, D, dname))
            # the launch edges
            for m in pc.M_EDGES:
                rc, part, fills = call.launch(m)
                torch.cuda.synchronize()
                if rc != 0:
                    failures.append(f'{tag} {dname} m = {m}: return code {rc}')
                    continue
                for name, t in part.items():
                    if name.startswith('_'):
                        want = call.adam + (1 if m else 0) if name == '_step' else 0
                        if float(t) != want:
                            failures.append(f'{tag} {dname} m = {m}: {name[1:]} is {float(t)}, not {want}')
                        continue
                    if not _same_bits(t[:m], full[name][:m]):
                        bad = int((_bits(t[:m]) != _bits(full[name][:m])).reshape(m, -1).any(1).sum())
                        failures.append(f'{tag} {name} {dname} m = {m}: {bad} of the rows [0, {m}) differ from those of m = {CNT}')
                    if not _same_bits(t[m:], fills[name][m:]):
                        failures.append(f'{tag} {name} {dname} m = {m}: rows >= {m} were written')
            # class <-> ABI
            cls = _through_the_class(kernel, D, dname, ci)
            for name in () if cls is None else call.wants if kernel != 'spd_dist_bwd_kernel' else ('grad_x', 'grad_y'):
                if not torch.equal(cls[name], full[name]):
                    failures.append(f'{tag} {name} {dname}: SymmetricPositiveDefinite and the ABI give different bits')
            # in place
            if call.adam is not None or kernel in ('spd_rsgd_step_kernel', 'spd_rsgd_momentum_kernel'):
                rc, same, _ = call.launch(CNT, inplace=True)
                torch.cuda.synchronize()
                assert rc == 0, (tag, rc)
                for name, t in same.items():
                    if not name.startswith('_') and not _same_bits(t, full[name]):
                        failures.append(f'{tag} {name} {dname}: x_new == x gives other bits than out of place')
            if call.adam is not None:
                rc, twice, _ = call.launch(CNT, steps=2)
                torch.cuda.synchronize()
                if rc != 0 or float(twice['_step']) != call.adam + 2 or int(twice['_ticket']) != 0:
                    failures.append(f'{tag} {dname}: step {float(twice["_step"])} ticket {int(twice["_ticket"])} after two calls from {call.adam}')
    assert not failures, '\n'.join(failures)


def test_every_instantiation_was_reached_and_summary():
    """Runs last: every (kernel, D, dtype) whose test ran has launched on a full batch — all 144 when the module runs whole — and
    the worst err / bound per quantity and dtype are printed (-rA)."""
    assert REACHED == _RAN, sorted(_RAN - REACHED)
    assert ctypes.c_int(_B().lib().raw('mm_spd_max_dim')()).value == pc.DIMS[-1]
    if len(_RAN) == len(GROUPS):
        assert len(REACHED) == 144
    for (what, dname), (ratio, tag) in sorted(pc.RATIOS.items()):
        if what.startswith('spd_pt_'):
            print(f'[worst] {what[7:]:28s} {dname}: {ratio:.3f}  ({tag})')
