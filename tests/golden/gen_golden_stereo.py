"""Golden vectors of the kappa-stereographic manifold from the REAL reference (development container only).
    PYTHONDONTWRITEBYTECODE=1 PYTHONHASHSEED=0 python tests/golden/gen_golden_stereo.py
`Universal` (manifolds/universal.py, manifolds/impl/math.py) on the CPU, in fp64 and in fp32, for the case list of
tests/stereo_cases.py.  Per base case (a case without its row range): pdist with both `squared` settings; per case: x.grad and
c.grad of sum(g * pdist) over the case's row range; per base case the maps exp, retr, projx, log, transp, egrad2rgrad, norm
and one RSGD step for exact in {F, T} x max_grad_norm in {None, 20} (the reference's optim/rsgd.py).  `edge` cases record projx
only (their points lie outside the ball until projected).  Then products/embedding.py's Embedding for ds = [5, 5]: stabilize
and then compute_dists (all nodes and a node minibatch) at n = 33, and a 20-epoch RSGD training trace at n = 40 (lr 0.01, exact, max_grad_norm 20, curvature SGD lr 0.001,
stabilize every epoch, stress loss against a fixed target).

The pair vectors do not compress, so the records are sharded below the size limit of a committed file: stereo_<k>.npz, filled
in case order, array by array, up to 800 KB each."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import stereo_cases as S  # noqa: E402  (host code: the case list and its inputs)

ref_shim.install()
from graphembed.manifolds import Universal  # noqa: E402
from graphembed.modules import ManifoldParameter  # noqa: E402
from graphembed.optim import RiemannianSGD  # noqa: E402
from graphembed.products.embedding import Embedding  # noqa: E402

DT = (('f64', torch.float64), ('f32', torch.float32))
LIMIT = 800 * 1024


def manifold(case, dt):
    n, m, c_init, fixed = case[:4]
    man = Universal(m, c_init=c_init, c_min=S.C_MIN, keep_sign_fixed=fixed)
    return man.to(dt)


def record_case(case, out, done):
    tag = S.case_id(case)
    base = S.base_of(case)
    btag = S.case_id(base)
    n, m, c_init, fixed, regime, _ = case
    x, c_raw = S.make_inputs(case)
    rows = S.rows_of(case)
    lo, hi = S.pair_slice(n, rows)
    for dname, dt in DT:
        man = manifold(case, dt)
        assert np.float32(man.c.item()) == c_raw
        xt = torch.from_numpy(x).to(dt)
        if regime == 'edge':
            with torch.no_grad():
                out[f'{btag}/projx_{dname}'] = man.projx(xt.clone(), inplace=True).numpy().copy()
            continue
        for squared in (False, True):
            sq = 'sq' if squared else 'd'
            xr = xt.clone().requires_grad_()
            man.c.grad = None
            d = man.pdist(xr, squared=squared)
            if btag not in done:
                out[f'{btag}/pdist_{sq}_{dname}'] = d.detach().numpy().copy()
            g = torch.from_numpy(S.upstream(hi - lo)).to(dt)
            (d[lo:hi] * g).sum().backward()
            out[f'{tag}/gx_{sq}_{dname}'] = xr.grad.numpy().copy()
            out[f'{tag}/gc_{sq}_{dname}'] = man.c.grad.numpy().copy()
        if btag in done:
            continue
        with torch.no_grad():
            u = torch.from_numpy(S.tangent(case, 1)).to(dt) * 0.1
            y = torch.roll(xt, 1, 0)
            out[f'{btag}/exp_{dname}'] = man.exp(xt, u).numpy().copy()
            out[f'{btag}/exp_noproject_{dname}'] = man.exp(xt, u, project=False).numpy().copy()
            out[f'{btag}/retr_{dname}'] = man.retr(xt, u).numpy().copy()
            out[f'{btag}/projx_{dname}'] = man.projx(xt.clone(), inplace=True).numpy().copy()
            out[f'{btag}/log_{dname}'] = man.log(xt, y).numpy().copy()
            out[f'{btag}/transp_{dname}'] = man.transp(xt, y, u).numpy().copy()
            out[f'{btag}/egrad2rgrad_{dname}'] = man.egrad2rgrad(xt, u).numpy().copy()
            out[f'{btag}/norm_{dname}'] = man.norm(xt, u).numpy().copy()
        eg = torch.from_numpy(S.tangent(case, 2)).to(dt) * 40
        for exact in (False, True):
            for clip in (None, 20):
                p = ManifoldParameter(xt.clone(), manifold=man)
                p.grad = eg.clone()
                RiemannianSGD([p], lr=0.01, exact=exact, max_grad_norm=clip).step()
                out[f'{btag}/rsgd_{int(exact)}_{clip}_{dname}'] = p.detach().numpy().copy()
    done.add(btag)


def product_records(out):
    for dname, dt in DT:
        torch.manual_seed(5)
        emb = Embedding(33, [5, 5]).to(dt)
        with torch.no_grad():
            for k, x in enumerate(emb.xs):
                x0 = np.random.RandomState(40 + k).uniform(-2, 2, size=(33, 5)).astype(np.float32)
                x0[::4] *= np.float32(3.0)     # some rows beyond r_max = 5
                x.copy_(torch.from_numpy(x0).to(dt))
                out[f'product33/x{k}'] = x.detach().float().numpy().copy()
            emb.manifolds[1].c.fill_(float(np.float32(-0.3)))
        emb.stabilize()
        for k, x in enumerate(emb.xs):
            out[f'product33/stabilized{k}_{dname}'] = x.detach().numpy().copy()
        out[f'product33/dists_{dname}'] = emb.compute_dists().detach().numpy().copy()
        idx = torch.tensor([3, 30, 7, 8, 21, 0, 14])
        out['product33/idx'] = idx.numpy()
        out[f'product33/dists_idx_{dname}'] = emb.compute_dists(idx).detach().numpy().copy()
    # training trace
    n = 40
    rng = np.random.RandomState(9)
    target = rng.randint(1, 9, size=n * (n - 1) // 2).astype(np.float32) ** 2 * np.float32(1e-3)
    out['train40/target'] = target
    for dname, dt in DT:
        emb = Embedding(n, [5, 5]).to(dt)
        with torch.no_grad():
            for k, x in enumerate(emb.xs):
                x.copy_(torch.from_numpy(np.random.RandomState(60 + k).uniform(-1e-2, 1e-2, size=(n, 5)).astype(np.float32)).to(dt))
                out[f'train40/x{k}'] = x.detach().float().numpy().copy()
        opt = RiemannianSGD(list(emb.xs), lr=0.01, exact=True, max_grad_norm=20)
        copt = torch.optim.SGD(list(emb.curvature_params), lr=0.001)
        tg = torch.from_numpy(target).to(dt)
        trace, curv = [], []
        for _ in range(20):
            opt.zero_grad()
            copt.zero_grad()
            loss = (emb.compute_dists() - tg).pow(2).sum()
            loss.backward()
            opt.step()
            copt.step()
            emb.stabilize()
            trace.append(loss.item())
            curv.append([man.c.item() for man in emb.manifolds])
        out[f'train40/loss_{dname}'] = np.array(trace)
        out[f'train40/c_{dname}'] = np.array(curv)


def main():
    shards, cur, size, done = [], {}, 0, set()
    for case in S.CASES:
        rec = {}
        record_case(case, rec, done)
        for key, v in rec.items():   # (array by array: one n = 257 case alone is above the limit)
            if cur and size + v.nbytes > LIMIT:
                shards.append(cur)
                cur, size = {}, 0
            cur[key] = v
            size += v.nbytes
    shards.append(cur)
    prod = {}
    product_records(prod)
    shards.append(prod)
    for old in os.listdir(HERE):
        if old.startswith('stereo_') and old.endswith('.npz'):
            os.remove(os.path.join(HERE, old))
    for k, out in enumerate(shards):
        path = os.path.join(HERE, f'stereo_{k}.npz')
        np.savez_compressed(path, **out)
        print(os.path.basename(path), len(out), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
