"""Golden vectors of the fused objective of a product of constant-curvature factors, from the REAL reference (development
container only).
    PYTHONDONTWRITEBYTECODE=1 PYTHONHASHSEED=0 python tests/golden/gen_golden_stereo_product.py
`products.Embedding` (products/embedding.py) + the objective (objectives.py) + autograd on the CPU for the case list and the six
objective settings of tests/stereo_product_cases.py.  Per base case: the summed pair vector `compute_dists()`; per case and
setting: the loss, every x_k.grad and every c_k.grad over the case's row range (the objective is applied to that slice of the
pair vector).  Every case is recorded in fp32; the nodes sweep and the factor-shapes cases also in fp64.  Keys carry the prefix
`prod/`; the records are sharded below the size limit of a committed file: stereo_product_<k>.npz, filled in case order, array
by array, up to 800 KB each."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import stereo_cases as S  # noqa: E402
import stereo_product_cases as P  # noqa: E402  (host code: the case list, its inputs and targets)

ref_shim.install()
from graphembed.objectives import QuotientLoss, StressLoss  # noqa: E402
from graphembed.products.embedding import Embedding  # noqa: E402

DT = {'f64': torch.float64, 'f32': torch.float32}
LIMIT = 800 * 1024


def dtypes_of(case):
    """fp32 always; fp64 for the nodes sweep and the factor-shapes cases"""
    n, ds, cs, fixed, regime, rows = case
    both = rows is None and not any(fixed)
    return ('f64', 'f32') if both else ('f32', )


def embedding(case, dt):
    n, ds, cs, fixed, regime, _ = case
    xs, craws = P.make_inputs(case)
    emb = Embedding(n, list(ds), c_min=S.C_MIN).to(dt)
    with torch.no_grad():
        for man, p, x, c_raw, c_init, fx in zip(emb.manifolds, emb.xs, xs, craws, cs, fixed):
            man.c.fill_(float(c_raw))
            man.sign = None if not fx else 1 if c_init > 0 else -1
            p.copy_(torch.from_numpy(x).to(dt))
    return emb


def record_case(case, out, done):
    n = case[0]
    lo, hi = S.pair_slice(n, P.rows_of(case))
    btag = P.case_id(P.base_of(case))
    for dname in dtypes_of(case):
        dt = DT[dname]
        _, target = P.pairs_of(P.base_of(case))
        tg = torch.from_numpy(target[lo:hi]).to(dt)
        for setting in P.SETTINGS:
            name, kind, terms, alpha, epoch = setting
            emb = embedding(case, dt)
            d = emb.compute_dists()
            if (btag, dname) not in done:
                out[f'prod/{btag}/dists_{dname}'] = d.detach().numpy().copy()
                done.add((btag, dname))
            if kind == 0:
                loss = (d[lo:hi] * torch.from_numpy(S.upstream(hi - lo)).to(dt)).sum()
            elif kind == 1:
                loss = StressLoss()(tg, d[lo:hi])
            else:
                loss = QuotientLoss(inc_l1=bool(terms & 1), inc_l2=bool(terms & 2))(tg, d[lo:hi], epoch=epoch, alpha=alpha)
            loss.backward()
            out[P.key(case, name, 'loss', dname)] = np.array(loss.item())
            for k, (x, man) in enumerate(zip(emb.xs, emb.manifolds)):
                out[P.key(case, name, f'gx{k}', dname)] = x.grad.numpy().copy()
                out[P.key(case, name, f'gc{k}', dname)] = man.c.grad.numpy().copy()


def main():
    shards, cur, size, done = [], {}, 0, set()
    for case in P.CASES:
        rec = {}
        record_case(case, rec, done)
        for key, v in rec.items():
            if cur and size + v.nbytes > LIMIT:
                shards.append(cur)
                cur, size = {}, 0
            cur[key] = v
            size += v.nbytes
    shards.append(cur)
    for old in os.listdir(HERE):
        if old.startswith('stereo_product_') and old.endswith('.npz'):
            os.remove(os.path.join(HERE, old))
    for k, out in enumerate(shards):
        path = os.path.join(HERE, f'stereo_product_{k}.npz')
        np.savez_compressed(path, **out)
        print(os.path.basename(path), len(out), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
