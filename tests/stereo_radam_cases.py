"""Cases, deterministic inputs and the LONG-DOUBLE oracle of the fused Riemannian Adam step on the kappa-stereographic manifold
(mm_stereo_radam_step, csrc/stereo.hip).  Host code only: the update of optim/radam.py:62-98 of the reference assembled from the
maps of tests/stereo_cases.py (egrad2rgrad, Universal.norm with its conformal factor at c = 1, expmap, project, transp).

Cases: m in (1, 5, 16) x (c_init, keep_sign_fixed) in ((0.01, F), (-0.3, F), (1.0, T), (-1.0, T)), n = 17, each under the
(exact, clip, nc) settings of tests/golden/gen_golden_radam.py; three steps at lr = 0.05, betas = (0.9, 0.99).  Points are the
`spread` points of stereo_cases (sqrt|c| max |x| = 0.7: at |c| = 0.01 some points have |x| > 1, where the norm's conformal
factor sits on its 1e-15 clamp); the rows ZERO_ROWS of the second and third gradient are zero - the rows outside a minibatch,
which keep moving on their moments."""
import itertools

import numpy as np

import stereo_cases as S

LD = S.LD
N = 17
LR = 0.05
BETAS = (0.9, 0.99)
EPS = 1e-8               # graphembed.utils.EPS, both precisions
ZERO_ROWS = (3, 11, 16)
CASES = [(m, c, fixed) for m in (1, 5, 16) for c, fixed in ((0.01, False), (-0.3, False), (1.0, True), (-1.0, True))]
SETTINGS = list(itertools.product([False, True], [None, 2.0], [False, True]))   # (exact, clip, nc)


def case_id(case):
    m, c, fixed = case
    return f'm{m}-c{c:g}-{"fix" if fixed else "free"}'


def setting_id(setting):
    exact, clip, nc = setting
    return f'exact{int(exact)}_clip{0 if clip is None else 1}_nc{int(nc)}'


def key(case, setting, what, dname):
    return f'radam/{case_id(case)}/{setting_id(setting)}/{what}_{dname}'


def mode_of(case):
    return S.mode_of(case[1], case[2])


def make_inputs(case):
    """(x0 [17, m] float32, c_raw float32, [g_0, g_1, g_2] float32)"""
    m, c, fixed = case
    scase = (N, m, c, fixed, 'spread', None)
    x0, c_raw = S.make_inputs(scase)
    gs = [S.tangent(scase, 2 + k) * np.float32(3.0) for k in range(3)]
    for g in gs[1:]:
        g[list(ZERO_ROWS)] = 0
    return x0, c_raw, gs


def step(x, eg, m1, v, t, c_raw, mode, dname, setting):
    """one update in long double: (x_new, exp_avg, exp_avg_sq [n, 1], t + 1) from the state (x, exp_avg, exp_avg_sq [n, 1], t)"""
    exact, clip, nc = setting
    x, eg, m1, v = (np.asarray(a, dtype=LD) for a in (x, eg, m1, v))
    c = S.get_c(c_raw, mode)[0]
    b1, b2 = LD(BETAS[0]), LD(BETAS[1])
    if nc:
        b2 = 1 - 1 / LD(t)
    r = eg / (2 / S._den(x, c)) ** 2
    nrm = 2 / S._den(x, LD(1)) * np.sqrt((r * r).sum(-1, keepdims=True))   # Universal.norm: c = 1
    v = b2 * v + (1 - b2) * nrm ** 2                                       # the norm BEFORE clipping
    if clip is not None:
        with np.errstate(divide='ignore'):
            r = r * np.minimum(LD(clip) / nrm, LD(1))
    m1 = b1 * m1 + (1 - b1) * r
    alpha = LD(LR) * np.sqrt(1 - b2 ** LD(t)) / (1 - b1 ** LD(t))
    direction = -alpha * m1 / (np.sqrt(v) + LD(EPS))
    new = S.project(S.expmap(x, direction, c) if exact else x + direction, c, dname)
    carried = S.maps(x, m1, new, c_raw, mode, dname)['transp']
    return new, carried, v, t + 1


def trace(case, setting, dname):
    """the oracle's states [(x, exp_avg, exp_avg_sq, t)] before step 1 and after each of the three steps"""
    x0, c_raw, gs = make_inputs(case)
    state = (x0.astype(LD), np.zeros(x0.shape, dtype=LD), np.zeros((N, 1), dtype=LD), 1)
    out = [state]
    for g in gs:
        state = step(state[0], g, state[1], state[2], state[3], c_raw, mode_of(case), dname, setting)
        out.append(state)
    return out
