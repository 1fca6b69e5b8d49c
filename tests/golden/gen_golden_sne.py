"""Golden vectors of the stochastic-neighbour KL objective from the REAL reference (development container only).
    PYTHONDONTWRITEBYTECODE=1 PYTHONHASHSEED=0 python tests/golden/gen_golden_sne.py
KLDiveregenceLoss('sne', inclusive) (graphembed/objectives.py:48-76, inference/stochastic_neighbors.py:8-24) on the CPU,
alpha = 1.3, for the case list of tests/sne_cases.py: per case the inputs (g: integers 1..6, m rounded to fp32 so that both
precisions see the same numbers) and, per mode, the reference's loss and gradient computed in fp64 and in fp32.

The gradients do not compress (3.7 MB over the case list), so the records are sharded to stay below the size limit of a
committed file: tests/golden/sne.npz holds every case with n <= 65, sne_n129.npz those of n = 129, sne_n257_<regime>.npz one case each."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
from sne_cases import ALPHA, CASES, MODES, make_inputs, shard_of  # noqa: E402  (host code: the case list and its inputs)

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
        for mode in MODES:
            fn = KLDiveregenceLoss('sne', inclusive=mode == 'incl')
            for dname, dt in (('f64', torch.float64), ('f32', torch.float32)):
                gt = torch.from_numpy(g.astype(np.float64)).to(dt)
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
