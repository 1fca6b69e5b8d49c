"""Golden RiemannianAdam traces on the reference's `Universal` manifold, from the REAL reference (development container only).
    PYTHONDONTWRITEBYTECODE=1 PYTHONHASHSEED=0 python tests/golden/gen_golden_stereo_radam.py
(run it after gen_golden_stereo.py, which clears every stereo_*.npz before it writes its own.)
Three consecutive steps of optim/radam.py on n = 17 points for m in {1, 5, 16}, (c_init, keep_sign_fixed) in {(0.01, F), (-0.3, F),
(1.0, T), (-1.0, T)} and the (exact, clip, nc) settings of gen_golden_radam.py, lr = 0.05, betas = (0.9, 0.99), in fp64 and fp32.
Points and gradients are those of tests/stereo_radam_cases.py (deterministic, not stored): the `spread` points of stereo_cases -
at |c| = 0.01 some lie at |x| > 1, where Universal.norm's conformal factor (taken at c = 1) sits on its 1e-15 clamp - and
gradients whose rows ZERO_ROWS vanish from the second step on (the rows outside a minibatch: zero gradient, non-zero moments).
fp64: the points after every step and the final moments.  fp32: points and both moments after every step (exp_avg_sq as its one
scalar per point: column 0), and only where the reference's own fp32 trace is finite - a trace that is not has no fp32 keys, and the tests
then hold the kernel to the floor of the tolerance rule.  Keys carry the prefix `radam/`; output stereo_radam.npz."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import stereo_cases as S  # noqa: E402
import stereo_radam_cases as A  # noqa: E402  (host code: the case list and its inputs)

ref_shim.install()
from graphembed.manifolds import Universal  # noqa: E402
from graphembed.modules import ManifoldParameter  # noqa: E402
from graphembed.optim import RiemannianAdam  # noqa: E402

DT = {'f64': torch.float64, 'f32': torch.float32}


def main():
    out, dropped = {}, []
    for case in A.CASES:
        m, c_init, fixed = case
        x0, c_raw, gs = A.make_inputs(case)
        for dname, dt in DT.items():
            torch.set_default_dtype(dt)
            for exact, clip, nc in A.SETTINGS:
                man = Universal(m, c_init=c_init, c_min=S.C_MIN, keep_sign_fixed=fixed)
                with torch.no_grad():
                    man.c.fill_(float(c_raw))
                p = ManifoldParameter(torch.from_numpy(x0).to(dt), manifold=man)
                opt = RiemannianAdam([p], lr=A.LR, betas=A.BETAS, nc=nc, max_grad_norm=clip, exact=exact)
                rec = {}
                for k, g in enumerate(gs):
                    p.grad = torch.from_numpy(g).to(dt)
                    opt.step()
                    rec[f'x{k + 1}'] = p.data.numpy().copy()
                    if dname == 'f32' or k == 2:
                        rec[f'exp_avg{k + 1}'] = opt.state[p]['exp_avg'].numpy().copy()
                        v = opt.state[p]['exp_avg_sq'].numpy()
                        assert np.allclose(v, v[:, :1], rtol=1e-6, atol=0, equal_nan=True)   # (torch's vectorised CPU loop: the last column may differ by an ulp)
                        rec[f'exp_avg_sq{k + 1}'] = v[:, 0].copy()
                assert opt.state[p]['step'] == 4
                if dname == 'f32' and not all(np.isfinite(v).all() for v in rec.values()):
                    dropped.append(A.key(case, (exact, clip, nc), 'x3', dname))
                    continue
                assert all(np.isfinite(v).all() for v in rec.values()), (case, exact, clip, nc, dname)
                for name, v in rec.items():
                    out[A.key(case, (exact, clip, nc), name, dname)] = v
    torch.set_default_dtype(torch.float32)
    path = os.path.join(HERE, 'stereo_radam.npz')
    np.savez_compressed(path, **out)
    print(os.path.basename(path), len(out), 'arrays', os.path.getsize(path), 'bytes; fp32 traces left out:', dropped)


if __name__ == '__main__':
    main()
