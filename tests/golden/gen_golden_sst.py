"""Golden vectors of the spanning-tree KL objective from the REAL reference (development container only).
    PYTHONDONTWRITEBYTECODE=1 PYTHONHASHSEED=0 python tests/golden/gen_golden_sst.py
KLDiveregenceLoss('sste', inclusive) (graphembed/objectives.py:48-76, inference/stochastic_trees.py) on the CPU, alpha = 1.3,
for the case list of tests/sst_cases.py: per case the inputs (g = k^2 / 36, m rounded to fp32 so that both precisions see the
same numbers) and, per setting of `inclusive`, the reference's loss and gradient computed in fp64 and in fp32.  The `offset`
cases are recorded in fp64 only: exp(-m) underflows in fp32 there and the reference's Cholesky fails.

The gradients do not compress, so the records are sharded to stay below the size limit of a committed file: tests/golden/sst.npz
holds every case with n <= 66, sst_n129.npz and sst_n130.npz those of one size, sst_n257_<regime>.npz one case each."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
from sst_cases import ALPHA, CASES, REF_MODES, make_inputs, shard_of  # noqa: E402  (host code: the case list and its inputs)

ref_shim.install()
from graphembed.objectives import KLDiveregenceLoss  # noqa: E402


def main():
    shards = {}
    for n, regime in CASES:
        g, m = make_inputs(n, regime)
        out = shards.setdefault(shard_of(n, regime), {})
        tag = f'n{n}/{regime}'
        out[f'{tag}/g'] = g
        out[f'{tag}/m'] = m
        for mode in REF_MODES:
            fn = KLDiveregenceLoss('sste', inclusive=mode == 'incl')
            for dname, dt in (('f64', torch.float64), ('f32', torch.float32)):
                if regime == 'offset' and dname == 'f32':
                    continue
                gt = torch.from_numpy(g).to(dt)
                mt = torch.from_numpy(m).to(dt).requires_grad_()
                loss = fn(gt, mt, alpha=ALPHA)
                gr, = torch.autograd.grad(loss, mt)
                assert torch.isfinite(loss) and torch.isfinite(gr).all(), (tag, mode, dname)
                out[f'{tag}/{mode}/loss_{dname}'] = loss.detach().numpy()
                out[f'{tag}/{mode}/grad_{dname}'] = gr.numpy()
    for name, out in shards.items():
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        print(name, len(out), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
