"""Golden vectors of a NODE MINIBATCH of a product of constant-curvature factors, from the REAL reference (development
container only).
    PYTHONDONTWRITEBYTECODE=1 PYTHONHASHSEED=0 python tests/golden/gen_golden_stereo_subset.py
`products.Embedding.compute_dists(idx)` (products/embedding.py) on the full tables, the targets gathered as GraphDataset does
(`dense[idx][:, idx]`, upper triangle; data/dataset.py:19-27), the objective (objectives.py) on the case's batch row range and
autograd on the CPU, for the case list of tests/stereo_subset_cases.py.  The tables hold NaN outside the batch, as in the tests;
the recorded gradients are the batch's rows x_k.grad[idx], in idx order - every other row of the reference's gradient is
asserted to be zero here.
fp32: every case and setting.  fp64: the settings stress, q3 and q3b of the cases over their whole batch, the (16,) * 8 shape
left out, and the summed pair vector `compute_dists(idx)` of the batches up to 65 nodes (the record stays below the size limit of
a committed file).  Keys carry the prefix `sub/`; output stereo_subset.npz."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import stereo_cases as S  # noqa: E402
import stereo_subset_cases as C  # noqa: E402  (host code: the case list, its inputs and targets)

ref_shim.install()
from graphembed.objectives import QuotientLoss, StressLoss  # noqa: E402
from graphembed.products.embedding import Embedding  # noqa: E402

DT = {'f64': torch.float64, 'f32': torch.float32}


def in_fp64(case):
    return case[6] is None and case[2] != (16, ) * 8


def embedding(case, dt):
    n_total, bs, ds, cs, fixed, regime, _ = case
    xs, craws, idx = C.make_inputs(case)
    emb = Embedding(n_total, list(ds), c_min=S.C_MIN).to(dt)
    with torch.no_grad():
        for man, p, x, c_raw, c_init, fx in zip(emb.manifolds, emb.xs, xs, craws, cs, fixed):
            man.c.fill_(float(c_raw))
            man.sign = None if not fx else 1 if c_init > 0 else -1
            p.copy_(torch.from_numpy(C.poisoned(x, idx)).to(dt))
    return emb


def record_case(case, out):
    bs = case[1]
    lo, hi = S.pair_slice(bs, C.rows_of(case))
    idx = torch.from_numpy(C.batch_of(case))
    dense = torch.from_numpy(np.nan_to_num(C.dense_of(case), nan=-1.0))
    a, b = torch.triu_indices(bs, bs, 1)
    for dname in ('f64', 'f32') if in_fp64(case) else ('f32', ):
        dt = DT[dname]
        tg = dense[idx][:, idx][a, b].to(dt)[lo:hi]
        assert bool((tg > 0).all())
        for setting in C.SETTINGS:
            name, kind, terms, alpha, epoch = setting
            if dname == 'f64' and name not in C.RECORDED:
                continue
            emb = embedding(case, dt)
            d = emb.compute_dists(idx)
            if name == 'stress' and dname == 'f64' and bs <= 65:   # the pair vector: fp64 only, the small batches
                out[f'sub/{C.case_id(case)}/dists_{dname}'] = d.detach().numpy().copy()
            if kind == 1:
                loss = StressLoss()(tg, d[lo:hi])
            else:
                loss = QuotientLoss(inc_l1=bool(terms & 1), inc_l2=bool(terms & 2))(tg, d[lo:hi], epoch=epoch, alpha=alpha)
            loss.backward()
            out[C.key(case, name, 'loss', dname)] = np.array(loss.item())
            rest = torch.ones(case[0], dtype=torch.bool)
            rest[idx] = False
            for k, (x, man) in enumerate(zip(emb.xs, emb.manifolds)):
                assert not bool(x.grad[rest].any())
                out[C.key(case, name, f'gx{k}', dname)] = x.grad[idx].numpy().copy()
                out[C.key(case, name, f'gc{k}', dname)] = man.c.grad.numpy().copy()


def main():
    out = {}
    for case in C.CASES:
        record_case(case, out)
    path = os.path.join(HERE, 'stereo_subset.npz')
    np.savez_compressed(path, **out)
    print(os.path.basename(path), len(out), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
