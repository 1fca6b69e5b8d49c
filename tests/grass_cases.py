"""Inputs, fp64 oracles and the tolerance rule shared by tests/test_grass_loss_gpu.py and tests/test_mat_step_gpu.py.

Every expected value comes from oracle/ref_port.py evaluated in fp64 on the CPU (never from an fp32 port: it yields NaN
gradients wherever 2p > N and in most of the reference-init regime).  Inputs are generated on the CPU with fixed seeds.

The tolerance is measured, not fixed: a case also runs the route the package took before the fused kernels (on the GPU, same
inputs), and with e_old / e_new the largest absolute deviations of the two routes from the oracle it requires

    e_new <= 2 e_old + 64 eps(dtype) max|oracle|

(the factor 2: the symmetric kernel sums half as many, differently ordered terms through atomics; the floor: cases where
the old route happens to be exact).  e_old is measured, never bounded, and both routes run the same device functions of
csrc/mat_common.hpp: a defect there shows up in e_old and e_new alike and this rule passes.  What holds the old route (and the
fused kernels) to an absolute answer is tests/test_mat_oracle_gpu.py — the rule of tests/mat_cases.py, built from the fp64 port
alone — at all 26 shapes of mat_cases.SHAPES (every (NP, P) instantiation at N = NP and at a padded N < NP, every N = p), both
kinds, fp32 and fp64; the golden vectors of tests/test_mat_gpu.py cover Gr(5,2), Gr(6,3) and St(5,2) at n = 33."""
import functools
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import ref_port as ref  # noqa: E402

DT = {'f32': torch.float32, 'f64': torch.float64}
SCALE_RAW = 0.3
QUOTIENT = dict(epoch=3, alpha=0.7)
REGIMES = {'f32': ('uniform', 'spread'), 'f64': ('uniform', 'spread', 'init')}

RATIOS = {}   # test id -> largest e_new / max(e_old, floor) seen (printed by the tests: -rA)


def _seed(*key):
    return zlib.crc32('/'.join(str(k) for k in key).encode())


@functools.lru_cache(maxsize=None)
def frames(regime, n, N, p):
    """n points of Gr(N,p) / St(N,p), fp64, CPU: `uniform` = Q of the QR of a Gaussian (pair distances O(1)); `spread` /
    `init` = exp from one base point along tangents of norm 0.3 / 1e-2 (the latter is the reference's own initialisation)."""
    g = torch.Generator().manual_seed(_seed('frames', regime, n, N, p))
    z = torch.randn(n, N, p, dtype=torch.float64, generator=g)
    if regime == 'uniform':
        return torch.linalg.qr(z)[0].contiguous()
    man = ref.Grassmann(N, p)
    base = torch.eye(N, p, dtype=torch.float64).expand(n, N, p)
    u = man.proju(base, z)
    u = u / u.norm(dim=(-2, -1), keepdim=True) * {'spread': 0.3, 'init': 1e-2}[regime]
    return man.exp(base, u).contiguous()


@functools.lru_cache(maxsize=None)
def targets(n):
    g = torch.Generator().manual_seed(_seed('targets', n))
    return torch.rand(n * (n - 1) // 2, dtype=torch.float64, generator=g) * 3.0 + 0.5


def oracle_loss(loss_name, gd, md):
    if loss_name == 'stress':
        return ref.stress_loss(gd, md)
    return ref.quotient_loss(gd, md, **QUOTIENT)


@functools.lru_cache(maxsize=None)
def objective_oracle(regime, n, N, p, loss_name):
    """(loss, grad_x [n,N,p], d loss / d scale_raw) of the full pair list in fp64 — computed once, shared, never modified."""
    x = frames(regime, n, N, p).clone().requires_grad_(True)
    s = torch.tensor(SCALE_RAW, dtype=torch.float64, requires_grad=True)
    md = ref.compute_dists([ref.Grassmann(N, p)], [x], [s])
    loss = oracle_loss(loss_name, targets(n), md)
    gx, gs = torch.autograd.grad(loss, [x, s])
    assert torch.isfinite(loss) and torch.isfinite(gx).all() and torch.isfinite(gs)
    return loss.detach(), gx, gs


def eps_of(dt):
    return float(torch.finfo(dt).eps)


def deviation(got, want):
    return float((got.detach().double().cpu() - want).abs().max()) if want.numel() else 0.0


def check(tag, what, old, new, want, dt, failures):
    """The tolerance rule for one quantity; records the ratio and appends a line to `failures` when it is missed."""
    e_old, e_new = deviation(old, want), deviation(new, want)
    floor = 64 * eps_of(dt) * float(want.abs().max()) if want.numel() else 0.0
    bound = 2 * e_old + floor
    RATIOS[tag] = max(RATIOS.get(tag, 0.0), e_new / max(e_old, floor, 1e-300))
    line = f'{tag} {what}: e_old {e_old:.3e} e_new {e_new:.3e} bound {bound:.3e} max|oracle| {float(want.abs().max()) if want.numel() else 0:.3e}'
    print(line)
    if not e_new <= bound:
        failures.append(line)


def embedding(n, N, p, dt, x, retr='svd'):
    """A single-factor Grassmann embedding on the GPU holding the points `x` (fp64, CPU) and the raw scale SCALE_RAW."""
    import graphembed.manifolds as M
    from graphembed.modules import ManifoldEmbedding
    torch.set_default_dtype(dt)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, [M.Grassmann(N, p, retr=retr)])
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        emb.xs[0].copy_(x.to(dt).cuda())
        emb.scales[0].fill_(SCALE_RAW)
    return emb


def objective(loss_name):
    from graphembed.objectives import QuotientLoss, StressLoss
    return (StressLoss(), {}) if loss_name == 'stress' else (QuotientLoss(), dict(QUOTIENT))


class CallSpy:
    """Records the names of the library's entry points called inside the `with` block (as tests/test_step_oracle_gpu.py)."""

    def __enter__(self):
        from graphembed import _backend as B
        self.lib, self.calls = B.lib(), []
        orig = self.lib.call

        def spy(name, *a):
            self.calls.append(name)
            return orig(name, *a)
        self.lib.call = spy
        return self

    def __exit__(self, *exc):
        del self.lib.call
        return False
