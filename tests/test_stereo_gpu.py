"""The kappa-stereographic kernels (csrc/stereo.hip) against the long-double oracle of tests/stereo_cases.py, through the C ABI
and through graphembed.manifolds.Stereographic (which must agree bitwise), per case of the stated list.

Tolerance rule (stereo_cases.bound): fp64 <= 1e-11 of the scale - max d / max d^2, max |grad|, the MAGNITUDE sum of the pairs'
curvature-gradient terms, max |map| -; fp32 <= twice the recorded reference-fp32's own deviation from the same oracle on the same
case and quantity, never asked below 16 * 2^-24 of the scale.  `edge` cases compare projx and finiteness only."""
import functools

import numpy as np
import pytest
import torch

import stereo_cases as S
from graphembed import _backend as B

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
CASE_IDS = [S.case_id(c) for c in S.CASES]
MAPS = ('exp', 'exp_noproject', 'retr', 'projx', 'log', 'transp', 'egrad2rgrad')
FULL = [c for c in S.CASES if c[5] is None and c[4] != 'edge']


def dev():
    return torch.device('cuda', 0)


def cuda(a, dname):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=NP[dname])).to(dev())


def manifold(case, dname):
    from graphembed.manifolds import Stereographic
    n, m, c_init, fixed = case[:4]
    return Stereographic(m, c_init=c_init, c_min=S.C_MIN, keep_sign_fixed=fixed).to(device=dev(), dtype=DT[dname])


@functools.lru_cache(maxsize=None)
def oracle_pairs(base, squared):
    x, c_raw = S.make_inputs(base)
    return S.pdist(x, c_raw, S.mode_of(base[2], base[3]), squared)


@functools.lru_cache(maxsize=None)
def oracle_grads(case, squared):
    x, c_raw = S.make_inputs(case)
    lo, hi = S.pair_slice(case[0], S.rows_of(case))
    return S.pdist_grads(x, c_raw, S.mode_of(case[2], case[3]), squared, S.upstream(hi - lo), S.rows_of(case))


def check(failures, what, dname, got, want, scale, ref32=None):
    """one comparison under the tolerance rule; `ref32` is the recorded reference-fp32 result of the same quantity"""
    err = S.deviation(got, want)
    scale = float(scale)
    bound = S.bound(dname, 0.0 if ref32 is None else S.deviation(ref32, want), scale)
    print(f'{what} {dname}: err {err / scale if scale else 0:.2e} of scale, bound {bound / scale if scale else 0:.2e}, ratio {err / bound if bound else 0:.3f}')
    if not (np.isfinite(err) and err <= bound):
        failures.append(f'{what} {dname}: {err:.3e} > {bound:.3e} (scale {scale:.3e})')


def abi_fwd(x, c, mode, rows, squared):
    n, m = x.shape
    lo, hi = S.pair_slice(n, rows)
    out = torch.empty(hi - lo, dtype=x.dtype, device=x.device)
    B.lib().call('mm_stereo_pdist_fwd', B.dtype_code(x), B.ptr(x), n, m, rows[0], rows[1], int(squared), B.ptr(c), mode, S.C_MIN,
                 B.ptr(out), B.stream_of(x))
    return out


def abi_bwd(x, g, c, mode, rows, squared):
    n, m = x.shape
    dt = B.dtype_code(x)
    gx = torch.full_like(x, float('nan'))
    gc = torch.full((1, ), float('nan'), dtype=x.dtype, device=x.device)
    ws = torch.empty(B.lib().raw('mm_stereo_pdist_ws_bytes')(dt, n, m), dtype=torch.uint8, device=x.device)
    ws.fill_(0xFF)   # the workspace needs no initialisation: hand it over dirty (NaN patterns)
    B.lib().call('mm_stereo_pdist_bwd', dt, B.ptr(x), B.ptr(g), n, m, rows[0], rows[1], int(squared), B.ptr(c), mode, S.C_MIN,
                 B.ptr(gx), B.ptr(gc), B.ptr(ws), B.stream_of(x))
    return gx, gc


def abi_map(op, x, u, y, c, mode):
    out = torch.full_like(x, float('nan'))
    B.lib().call('mm_stereo_map', B.dtype_code(x), op, B.ptr(x), B.ptr(u), B.ptr(y), x.shape[0], x.shape[1], B.ptr(c), mode, S.C_MIN,
                 B.ptr(out), B.stream_of(x))
    return out


@pytest.mark.parametrize('case', S.CASES, ids=CASE_IDS)
def test_case_against_the_oracle(case):
    n, m, c_init, fixed, regime, _ = case
    R = S.recorded()
    tag, btag = S.case_id(case), S.case_id(S.base_of(case))
    x_np, c_raw = S.make_inputs(case)
    mode = S.mode_of(c_init, fixed)
    rows = S.rows_of(case)
    lo, hi = S.pair_slice(n, rows)
    failures = []
    for dname in ('f64', 'f32'):
        man = manifold(case, dname)
        x = cuda(x_np, dname)
        c = man.c.detach()
        if regime == 'edge':
            with torch.no_grad():
                px = man.projx(x)
            want = S.project(x_np.astype(S.LD), S.get_c(c_raw, mode)[0], dname)
            check(failures, f'{tag} projx', dname, px.cpu().numpy(), want, np.abs(want).max(), R[f'{btag}/projx_{dname}'])
            for squared in (False, True):
                d = man.pdist(px, squared=squared)
                assert bool(torch.isfinite(d).all()) and float(d.detach().min()) >= S.EPS * 0.99
            continue
        for sq, squared in (('d', False), ('sq', True)):
            want = oracle_pairs(S.base_of(case), squared)
            got = abi_fwd(x, c, mode, rows, squared)
            ref32 = R[f'{btag}/pdist_{sq}_f32'][lo:hi] if dname == 'f32' else None
            if hi > lo:
                check(failures, f'{tag} pdist_{sq}', dname, got.cpu().numpy(), want[lo:hi], want.max(), ref32)
            xr = x.clone().requires_grad_()
            man.c.grad = None
            d = man.pdist(xr, squared=squared, rows=None if case[5] is None else rows)
            assert torch.equal(d.detach(), got), 'the class and the C ABI disagree (forward)'
            g = cuda(S.upstream(hi - lo), dname)
            (d * g).sum().backward() if hi > lo else d.sum().backward()
            gx, gc = abi_bwd(x, g, c, mode, rows, squared)
            assert torch.equal(xr.grad, gx) and torch.equal(man.c.grad.to(gc.dtype), gc), 'the class and the C ABI disagree (backward)'
            if hi == lo:   # an empty range, or the last row: it has no pair
                assert d.shape == (0, ) and got.shape == (0, )
                assert not gx.any() and not gc.any() and not xr.grad.any() and not man.c.grad.any(), 'a range without pairs leaves zeros'
                assert not R[f'{tag}/gx_{sq}_{dname}'].any() and not R[f'{tag}/gc_{sq}_{dname}'].any()
                continue
            wx, wc, wcs = oracle_grads(case, squared)
            r32 = (R[f'{tag}/gx_{sq}_f32'], R[f'{tag}/gc_{sq}_f32']) if dname == 'f32' else (None, None)
            check(failures, f'{tag} grad_x_{sq}', dname, gx.cpu().numpy(), wx, np.abs(wx).max(), r32[0])
            check(failures, f'{tag} grad_c_{sq}', dname, gc.cpu().numpy()[0], wc, wcs, r32[1])
        if case[5] is not None:
            continue
        # maps, fused RSGD step, stabilize
        u_np = S.tangent(case, 1).astype(NP[dname]) * NP[dname](0.1)
        y_np = np.roll(x_np, 1, 0)
        want = S.maps(x_np, u_np, y_np, c_raw, mode, dname)
        u, y = cuda(u_np, dname), cuda(y_np, dname)
        with torch.no_grad():
            got = {'exp': man.exp(x, u), 'exp_noproject': man.exp(x, u, project=False), 'retr': man.retr(x, u), 'projx': man.projx(x),
                   'log': man.log(x, y), 'transp': man.transp(x, y, u), 'egrad2rgrad': man.egrad2rgrad(x, u)}
            assert man.proju(x, u) is u
        for k in MAPS:
            check(failures, f'{tag} {k}', dname, got[k].cpu().numpy(), want[k], np.abs(want[k]).max(), R[f'{btag}/{k}_{dname}'] if dname == 'f32' else None)
        ops = {'exp': (B.STEREO_EXP, u, None), 'exp_noproject': (B.STEREO_EXP_NOPROJECT, u, None), 'retr': (B.STEREO_RETR, u, None),
               'projx': (B.STEREO_PROJX, None, None), 'log': (B.STEREO_LOG, None, y), 'transp': (B.STEREO_TRANSP, u, y),
               'egrad2rgrad': (B.STEREO_EGRAD2RGRAD, u, None)}
        for k, (op, uu, yy) in ops.items():
            assert torch.equal(abi_map(op, x, uu, yy, c, mode), got[k]), f'the class and the C ABI disagree ({k})'
        assert torch.equal(abi_map(B.STEREO_PROJU, x, u, None, c, mode), u)
        check(failures, f'{tag} norm', dname, man.norm(x, u).cpu().numpy(), want['norm'], want['norm'].max(),
              R[f'{btag}/norm_{dname}'] if dname == 'f32' else None)
        eg_np = S.tangent(case, 2).astype(NP[dname]) * NP[dname](40)
        eg = cuda(eg_np, dname)
        for exact in (0, 1):
            for clip in (None, 20):
                ws = S.rsgd_step(x_np, eg_np, c_raw, mode, dname, 0.01, clip, exact)
                new = man.rsgd_step(x, eg, lr=0.01, max_grad_norm=clip, exact=bool(exact))
                check(failures, f'{tag} rsgd_{exact}_{clip}', dname, new.cpu().numpy(), ws, np.abs(ws).max(),
                      R[f'{btag}/rsgd_{exact}_{clip}_{dname}'] if dname == 'f32' else None)
                out = torch.empty_like(x)
                B.lib().call('mm_stereo_rsgd_step', B.dtype_code(x), B.ptr(x), B.ptr(eg), n, m, B.ptr(c), mode, S.C_MIN, 0.01,
                             -1.0 if clip is None else float(clip), exact, B.ptr(out), B.stream_of(x))
                assert torch.equal(out, new)
        big = cuda(x_np * np.float32(40 if regime == 'init' else 9), dname)
        wst = S.stabilize(big.cpu().numpy(), c_raw, mode, dname, 0.05 if regime == 'init' else 5.0)
        st = man.stabilize_(big.clone(), 0.05 if regime == 'init' else 5.0)
        out = torch.empty_like(big)
        B.lib().call('mm_stereo_stabilize', B.dtype_code(big), B.ptr(big), n, m, B.ptr(c), mode, S.C_MIN, 0.05 if regime == 'init' else 5.0,
                     B.ptr(out), B.stream_of(big))
        assert torch.equal(out, st), 'the class and the C ABI disagree (stabilize)'
        check(failures, f'{tag} stabilize', dname, st.cpu().numpy(), wst, np.abs(wst).max())
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_element_wise_dist_matches_the_pair_kernels(dname):
    case = (65, 8, 1.0, False, 'spread', None)
    x_np, c_raw = S.make_inputs(case)
    man = manifold(case, dname)
    x = cuda(x_np, dname)
    i, j = np.triu_indices(65, 1)
    it, jt = torch.from_numpy(i).to(dev()), torch.from_numpy(j).to(dev())
    failures = []
    for sq, squared in (('d', False), ('sq', True)):
        xa, xb = x[it].clone().requires_grad_(), x[jt].clone().requires_grad_()
        man.c.grad = None
        d = man.dist(xa, xb, squared=squared)
        want = oracle_pairs(case, squared)
        check(failures, f'dist_{sq}', dname, d.detach().cpu().numpy(), want, want.max(), S.recorded()[f'{S.case_id(case)}/pdist_{sq}_f32'])
        g = cuda(S.upstream(len(i)), dname)
        (d * g).sum().backward()
        # the same two calls through the C ABI: bitwise equal
        xa_c, xb_c, cr = xa.detach().contiguous(), xb.detach().contiguous(), man.c.detach()
        o, ga, gb = torch.empty_like(d), torch.empty_like(xa_c), torch.empty_like(xb_c)
        gcc = torch.empty(1, dtype=x.dtype, device=x.device)
        ws = torch.full((8 * ((len(i) + 127) // 128 + 1), ), 0xFF, dtype=torch.uint8, device=x.device)
        B.lib().call('mm_stereo_dist', B.dtype_code(x), B.ptr(xa_c), B.ptr(xb_c), None, len(i), 8, int(squared), B.ptr(cr), 0, S.C_MIN,
                     B.ptr(o), None, None, None, None, B.stream_of(x))
        B.lib().call('mm_stereo_dist', B.dtype_code(x), B.ptr(xa_c), B.ptr(xb_c), B.ptr(g), len(i), 8, int(squared), B.ptr(cr), 0, S.C_MIN,
                     None, B.ptr(ga), B.ptr(gb), B.ptr(gcc), B.ptr(ws), B.stream_of(x))
        assert torch.equal(o, d.detach()) and torch.equal(ga, xa.grad) and torch.equal(gb, xb.grad) and torch.equal(gcc, man.c.grad)
        gx = torch.zeros_like(x).index_add_(0, it, xa.grad).index_add_(0, jt, xb.grad)
        wx, wc, wcs = oracle_grads(case, squared)
        r32 = S.recorded()
        check(failures, f'dist grad_x_{sq}', dname, gx.cpu().numpy(), wx, np.abs(wx).max(), r32[f'{S.case_id(case)}/gx_{sq}_f32'])
        check(failures, f'dist grad_c_{sq}', dname, man.c.grad.cpu().numpy()[0], wc, wcs, r32[f'{S.case_id(case)}/gc_{sq}_f32'])
    assert d.shape == (len(i), ) and man.dist(x[:4], x[1:5], keepdim=True).shape == (4, 1)
    assert not failures, '\n'.join(failures)


def test_zero_curvature_gives_the_euclidean_limit():
    """c = 0 exactly (free sign, c_raw = 0): 4 |x_i - x_j|^2 where the reference returns NaN; the value only."""
    from graphembed.manifolds import Stereographic
    x_np = np.random.RandomState(3).uniform(-1, 1, size=(9, 4)).astype(np.float32)
    i, j = np.triu_indices(9, 1)
    q = ((x_np[i].astype(np.float64) - x_np[j]) ** 2).sum(-1)
    for dname, tol in (('f32', 1e-6), ('f64', 1e-14)):
        man = Stereographic(4, c_init=0.0, c_min=0.0).to(device=dev(), dtype=DT[dname])
        d2 = man.pdist(cuda(x_np, dname), squared=True)
        assert S.deviation(d2.detach().cpu().numpy(), 4 * q) <= tol * 4 * q.max()


@pytest.mark.parametrize('case', [c for c in FULL if c[0] in (65, 129, 257) and c[1] in (5, 8)][:4] + [(129, 13, -1.0, False, 'spread', None)],
                         ids=S.case_id)
def test_shards_sum_to_the_full_launch(case):
    n, m, c_init, fixed = case[:4]
    x_np, c_raw = S.make_inputs(case)
    mode = S.mode_of(c_init, fixed)
    failures = []
    for dname in ('f64', 'f32'):
        man = manifold(case, dname)
        x, c = cuda(x_np, dname), man.c.detach()
        for sq, squared in (('d', False), ('sq', True)):
            g = cuda(S.upstream(n * (n - 1) // 2), dname)
            full_x, full_c = abi_bwd(x, g, c, mode, (0, n), squared)
            cuts = [0, n // 5, n // 2, n]
            sx, sc = torch.zeros_like(full_x), torch.zeros_like(full_c)
            fw = []
            for rb, re in zip(cuts[:-1], cuts[1:]):
                lo, hi = S.pair_slice(n, (rb, re))
                px, pc = abi_bwd(x, g[lo:hi].contiguous(), c, mode, (rb, re), squared)
                sx += px
                sc += pc
                fw.append(abi_fwd(x, c, mode, (rb, re), squared))
            assert torch.equal(torch.cat(fw), abi_fwd(x, c, mode, (0, n), squared))
            wx, wc, wcs = oracle_grads(case, squared)
            r32x = S.recorded().get(f'{S.case_id(case)}/gx_{sq}_f32') if dname == 'f32' else None
            r32c = S.recorded().get(f'{S.case_id(case)}/gc_{sq}_f32') if dname == 'f32' else None
            check(failures, f'{S.case_id(case)} shard sum grad_x_{sq}', dname, sx.cpu().numpy(), wx, np.abs(wx).max(), r32x)
            check(failures, f'{S.case_id(case)} shard sum grad_c_{sq}', dname, sc.cpu().numpy()[0], wc, wcs, r32c)
            check(failures, f'{S.case_id(case)} full launch grad_x_{sq}', dname, full_x.cpu().numpy(), wx, np.abs(wx).max(), r32x)
            check(failures, f'{S.case_id(case)} full launch grad_c_{sq}', dname, full_c.cpu().numpy()[0], wc, wcs, r32c)
            ex, ec = abi_bwd(x, g[:0], c, mode, (7, 7), squared)
            assert not ex.any() and not ec.any()
    assert not failures, '\n'.join(failures)


def test_degenerate_node_counts():
    for dname in ('f32', 'f64'):
        man = manifold((1, 5, 0.01, False), dname)
        x = torch.zeros(1, 5, dtype=DT[dname], device=dev(), requires_grad=True)
        d = man.pdist(x)
        assert d.shape == (0, )
        d.sum().backward()
        assert not x.grad.any() and float(man.c.grad) == 0.0


def product(dname, n, c1=None):
    from graphembed.modules import StereographicProductEmbedding
    emb = StereographicProductEmbedding(n, [5, 5]).to(device=dev(), dtype=DT[dname])
    if c1 is not None:
        with torch.no_grad():
            emb.manifolds[1].c.fill_(float(np.float32(c1)))
    return emb


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_product_embedding_against_the_recorded_embedding(dname):
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import QuotientLoss, StochasticNeighborLoss, StressLoss
    R = S.recorded()
    emb = product(dname, 33, -0.3)
    assert all(p.is_cuda and p.manifold is man for p, man in zip(emb.xs, emb.manifolds)) and emb.device.type == 'cuda'
    failures = []
    with torch.no_grad():
        for k, x in enumerate(emb.xs):
            x.copy_(cuda(R[f'product33/x{k}'], dname))
    emb.stabilize()
    for k, c in ((0, 0.01), (1, -0.3)):
        want = S.stabilize(R[f'product33/x{k}'], np.float32(c), 0, dname, 5.0)
        check(failures, f'stabilize factor {k}', dname, emb.xs[k].detach().cpu().numpy(), want, 5.0, R[f'product33/stabilized{k}_{dname}'])
    xs = [R[f'product33/stabilized{k}_{dname}'] for k in (0, 1)]
    with torch.no_grad():
        for x, v in zip(emb.xs, xs):
            x.copy_(cuda(v, dname))
    want = S.pdist(xs[0], np.float32(0.01), 0, True) + S.pdist(xs[1], np.float32(-0.3), 0, True)
    check(failures, 'compute_dists', dname, emb.compute_dists().detach().cpu().numpy(), want, want.max(), R[f'product33/dists_{dname}'])
    idx = torch.from_numpy(R['product33/idx'])
    wi = S.pdist(xs[0][idx], np.float32(0.01), 0, True) + S.pdist(xs[1][idx], np.float32(-0.3), 0, True)
    check(failures, 'compute_dists(indices)', dname, emb.compute_dists(idx).detach().cpu().numpy(), wi, want.max(), R[f'product33/dists_idx_{dname}'])
    assert not failures, '\n'.join(failures)

    class Pairs:   # the dataset protocol of BatchedObjective: pair distances of a node subset
        def __init__(self, n):
            self.n = n
            self.full = torch.from_numpy(np.random.RandomState(1).randint(1, 7, size=n * (n - 1) // 2).astype(NP[dname]))

        def __getitem__(self, i):
            if i is None:
                return self.full
            dense = torch.zeros(self.n, self.n, dtype=self.full.dtype)
            a, b = torch.triu_indices(self.n, self.n, 1)
            dense[a, b] = self.full
            dense = dense + dense.T
            p, q = torch.triu_indices(len(i), len(i), 1)
            return dense[i[p], i[q]]

    for loss_fn in (StressLoss(), QuotientLoss(), StochasticNeighborLoss()):
        for indices in (None, idx):
            emb.zero_grad()
            loss = BatchedObjective(loss_fn, Pairs(33), emb)(indices, epoch=1, alpha=1.0)
            loss.backward()
            assert bool(torch.isfinite(loss))
            for x in emb.xs:
                assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())
                if indices is not None:
                    rest = torch.ones(33, dtype=torch.bool)
                    rest[indices] = False
                    assert not x.grad[rest.to(dev())].any()
            for c in emb.curvature_params:
                assert c.grad is not None and bool(torch.isfinite(c.grad).all()) and float(c.grad) != 0.0


def train_setup(dname):
    from graphembed.optim import RiemannianSGD
    R = S.recorded()
    emb = product(dname, 40)
    with torch.no_grad():
        for k, x in enumerate(emb.xs):
            x.copy_(cuda(R[f'train40/x{k}'], dname))
    # the curvatures are plain Euclidean parameters (a group of their own: plain SGD, as in the reference's grid)
    opt = RiemannianSGD([dict(params=list(emb.xs), lr=0.01, exact=True, max_grad_norm=20),
                         dict(params=list(emb.curvature_params), lr=0.001, exact=False, max_grad_norm=None)], lr=0.01)
    return emb, opt, cuda(R['train40/target'], dname)


def train_step(emb, opt, target):
    opt.zero_grad(set_to_none=True)
    loss = (emb.compute_dists() - target).pow(2).sum()
    loss.backward()
    opt.step()
    emb.stabilize()
    return loss.detach()


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_training_follows_the_oracle_trace(dname):
    R = S.recorded()
    emb, opt, target = train_setup(dname)
    want, _ = S.train_trace([R['train40/x0'], R['train40/x1']], [np.float32(0.01)] * 2, [0, 0], R['train40/target'], dname, 5)
    trace = [float(train_step(emb, opt, target)) for _ in range(20)]
    failures = []
    for e in range(5):
        check(failures, f'epoch {e} loss', dname, trace[e], want[e], want[e], R[f'train40/loss_{dname}'][e])
    assert not failures, '\n'.join(failures)
    assert all(b < a for a, b in zip(trace, trace[1:])) and trace[-1] < 0.8 * trace[0], trace
    for man in emb.manifolds:
        assert float(man.c.detach()) != float(np.float32(0.01)), 'the curvature did not move'
    assert all(bool(torch.isfinite(x).all()) for x in emb.xs)


def test_captured_step_follows_the_curvature_without_recapture():
    """One training step captured once (one stream, no parallel branches) and replayed 3 times equals 3 eager steps: the kernels
    read c from device memory - a value baked in at capture would freeze the geometry at the first step's curvature."""
    dname = 'f32'
    eager = train_setup(dname)
    for _ in range(3):
        train_step(*eager)
    emb, opt, target = train_setup(dname)
    start = [x.detach().clone() for x in emb.xs] + [c.detach().clone() for c in emb.curvature_params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture: allocator pools, lazy initialisation
        train_step(emb, opt, target)
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for p, v in zip(list(emb.xs) + list(emb.curvature_params), start):
            p.copy_(v)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        train_step(emb, opt, target)
    with torch.no_grad():            # (capturing does not execute)
        for p, v in zip(list(emb.xs) + list(emb.curvature_params), start):
            p.copy_(v)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(list(emb.xs) + list(emb.curvature_params), list(eager[0].xs) + list(eager[0].curvature_params)):
        scale = float(want.detach().abs().max())
        assert float((got.detach() - want.detach()).abs().max()) <= S.FLOOR32 * scale
    assert float(emb.manifolds[0].c.detach()) != float(start[2])


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_momentum_and_adam_take_the_generic_route(dname):
    """RiemannianSGD with momentum and RiemannianAdam have no fused kernel for these points: they run on egrad2rgrad, the
    reference's norm, exp and transp of the class.  One step each from fresh state, against the same update assembled from the
    oracle's maps (optim/rsgd.py:56-80 and optim/radam.py:62-98 of the reference)."""
    from graphembed.modules import ManifoldParameter
    from graphembed.optim import RiemannianAdam, RiemannianSGD
    case = (65, 8, 1.0, False, 'spread', None)
    x_np, c_raw = S.make_inputs(case)
    eg_np = S.tangent(case, 2).astype(NP[dname]) * NP[dname](40)
    man = manifold(case, dname)
    LD = S.LD
    c = S.get_c(c_raw, 0)[0]
    xl, el = x_np.astype(LD), eg_np.astype(LD)
    lam1 = 2 / S._den(xl, LD(1))

    def clipped(r):   # Universal.norm: the conformal factor at c = 1
        nrm = lam1 * np.sqrt((r * r).sum(-1, keepdims=True))
        return r * np.minimum(LD(20) / nrm, LD(1))

    r0 = el / (2 / S._den(xl, c)) ** 2
    r = clipped(r0)
    failures = []
    # a step chains three kernels (egrad2rgrad, exp, transp) and half a dozen element-wise torch ops, each good to a few ulp: the
    # scale handed to the single-kernel rule is four times max |value|
    lr = 0.001
    # heavy ball, first step: the buffer starts as the EUCLIDEAN gradient (rsgd.py:53-54), then buf = momentum buf + (1 - dampening) r
    buf = LD(0.9) * el + r
    new = S.project(S.expmap(xl, -LD(lr) * buf, c), c, dname)
    carried = S.maps(xl, buf, new, c_raw, 0, dname)['transp']
    p = ManifoldParameter(cuda(x_np, dname), manifold=man)
    p.grad = cuda(eg_np, dname)
    opt = RiemannianSGD([p], lr=lr, momentum=0.9, exact=True, max_grad_norm=20)
    opt.step()
    assert float(np.abs(new - xl).max()) > 1e-3 and float((lam1 * np.sqrt((r0 * r0).sum(-1, keepdims=True))).max()) > 20   # it moves, the clip acts
    check(failures, 'momentum step', dname, p.detach().cpu().numpy(), new, 4 * np.abs(new).max())
    check(failures, 'momentum buffer', dname, opt.state[p]['momentum_buffer'].cpu().numpy(), carried, 4 * np.abs(carried).max())
    # Adam, first step (radam.py:62-98): exp_avg = (1 - b1) r, exp_avg_sq = (1 - b2) ||r||^2 with the norm BEFORE clipping,
    # bias-corrected stride, first moment transported
    m1 = LD(0.1) * r
    v1 = LD(0.001) * (lam1 * np.sqrt((r0 * r0).sum(-1, keepdims=True))) ** 2
    stride = -LD(lr) * np.sqrt(LD(1) - LD(0.999)) / (LD(1) - LD(0.9))
    direction = m1 / (np.sqrt(v1) + LD(1e-8)) * stride
    new = S.project(S.expmap(xl, direction, c), c, dname)
    carried = S.maps(xl, m1, new, c_raw, 0, dname)['transp']
    p = ManifoldParameter(cuda(x_np, dname), manifold=man)
    p.grad = cuda(eg_np, dname)
    opt = RiemannianAdam([p], lr=lr, exact=True, max_grad_norm=20)
    opt.step()
    check(failures, 'adam step', dname, p.detach().cpu().numpy(), new, 4 * np.abs(new).max())
    check(failures, 'adam first moment', dname, opt.state[p]['exp_avg'].cpu().numpy(), carried, 4 * np.abs(carried).max())
    assert not failures, '\n'.join(failures)
