"""Cases, deterministic inputs and the LONG-DOUBLE oracle of the fused objective of a product of constant-curvature factors
(mm_stereo_product_*, csrc/stereo.hip; graphembed.modules.StereographicProductEmbedding).  Host code only: the distances and
gradients of a factor come from tests/stereo_cases.py (closed forms in long double), the objective on m = sum_k d_k^2 and
g = d loss / d m are evaluated here in long double.

The case list is stated, not a cross product (20 cases):
  nodes     n in N_SWEEP, ds = [5, 5], c_init = (0.01, -0.3), free sign, `init`                                6
  shapes    ds in SHAPES at n = 65, `spread`, c_init cycling through C_CYCLE, free sign                         6
  modes     ds = [8, 8, 8], (c_init, fixed) = (1.0, T), (-1.0, T), (-0.01, F), n = 65, `init` and `spread`      2
  rows      every range of stereo_cases._rows(129) at n = 129, ds = [5, 8], c_init = (0.01, -0.3), `spread`     6
and every case runs under the six objective SETTINGS.

Targets are float32(m_oracle * F[k mod 4]) with F = (0.5, 0.8, 1.25, 2.0) over the pair index k: the quotient loss's |.| stays
away from its kink by construction - `kink_margin` gives the distance, the host test asserts it at >= 1e-4 for every case and
setting (a case that misses it gets another seed through SALT; no pair is ever filtered out)."""
import functools

import numpy as np

import stereo_cases as S

LD = S.LD
N_SWEEP = (2, 3, 64, 65, 129, 257)
SHAPES = ((3, 4), (5, 8), (1, 16), (2, 3, 5, 8), (2, ) * 8, (16, ) * 8)
C_CYCLE = (1.0, -1.0, 0.01, -0.3)
F = (0.5, 0.8, 1.25, 2.0)
# (name, loss kind, terms, alpha, epoch): kind 0 = an upstream gradient per pair (S.upstream), 1 = stress, 2 = quotient
SETTINGS = (('up', 0, 0, 1.0, 1), ('stress', 1, 0, 1.0, 1), ('q1', 2, 1, 1.0, 1), ('q2', 2, 2, 1.0, 1), ('q3', 2, 3, 1.0, 1),
            ('q3b', 2, 3, 0.7, 9))
SETTING_IDS = [s[0] for s in SETTINGS]
KINK = 1e-4
SALT = {}   # case id -> seed offset, for a case whose first seed lands a pair within KINK of the quotient loss's kink


def _build():
    cases = [(n, (5, 5), (0.01, -0.3), (False, False), 'init', None) for n in N_SWEEP]
    cases += [(65, ds, tuple(C_CYCLE[k % 4] for k in range(len(ds))), (False, ) * len(ds), 'spread', None) for ds in SHAPES]
    cases += [(65, (8, 8, 8), (1.0, -1.0, -0.01), (True, True, False), regime, None) for regime in ('init', 'spread')]
    cases += [(129, (5, 8), (0.01, -0.3), (False, False), 'spread', r) for r in S._rows(129)]
    return cases


CASES = _build()


def case_id(case):
    n, ds, cs, fixed, regime, rows = case
    shape = 'x'.join(str(d) for d in ds) if len(set(ds)) > 1 or len(ds) < 4 else f'{ds[0]}^{len(ds)}'
    mode = ''.join('f' if f else 'v' for f in fixed) if any(fixed) else 'free'
    return f'n{n}-d{shape}-{mode}-{regime}' + ('' if rows is None else f'-r{rows[0]}_{rows[1]}')


CASE_IDS = [case_id(c) for c in CASES]


def base_of(case):
    return case[:5] + (None, )


def rows_of(case):
    return (0, case[0]) if case[5] is None else case[5]


def modes_of(case):
    return [S.mode_of(c, f) for c, f in zip(case[2], case[3])]


def make_inputs(case):
    """([x_k [n, d_k] float32], [c_raw_k float32]): every factor as stereo_cases.make_inputs builds a single one"""
    n, ds, cs, fixed, regime, _ = base_of(case)
    xs, craws = [], []
    for k, (d, c_init, fx) in enumerate(zip(ds, cs, fixed)):
        seed = 7000000 + 1000 * n + 10 * d + 97 * k + int(fx) + (3 if c_init < 0 else 0) + {'init': 0, 'spread': 100000}[regime] \
            + 1000003 * SALT.get(case_id(base_of(case)), 0)
        rng = np.random.RandomState(seed)
        c_raw = np.float32(c_init)
        c = float(S.get_c(c_raw, S.mode_of(c_init, fx))[0])
        if regime == 'init':
            x = rng.uniform(-1e-2, 1e-2, size=(n, d))
        else:
            x = rng.uniform(-0.5, 0.5, size=(n, d))
            x *= 0.699 / (np.sqrt(abs(c)) * np.sqrt((x * x).sum(-1)).max())
        xs.append(x.astype(np.float32))
        craws.append(c_raw)
    return xs, craws


@functools.lru_cache(maxsize=None)
def pairs_of(base):
    """the oracle's summed pair vector of the whole case (long double) and float32 targets"""
    xs, craws = make_inputs(base)
    m = sum(S.pdist(x, c, md, True) for x, c, md in zip(xs, craws, modes_of(base)))
    f = np.array(F, dtype=LD)[np.arange(len(m)) % 4]
    return m, (m * f).astype(np.float32)


def objective(m, target, setting):
    """(loss terms per pair, g = d loss / d m per pair) in long double"""
    _, kind, terms, alpha, epoch = setting
    m, t = np.asarray(m, dtype=LD), np.asarray(target, dtype=LD)
    if kind == 0:
        g = S.upstream(len(m)).astype(LD)
        return g * m, g
    if kind == 1:
        return (m - t) ** 2, 2 * (m - t)
    ag, eps = LD(alpha) * t, LD(1) / LD(epoch + 1)
    loss, g = np.zeros_like(m), np.zeros_like(m)
    if terms & 1:
        q = m / ag - 1
        loss += np.abs(q)
        g += np.sign(q) / ag
    if terms & 2:
        q = ag / (m + eps) - 1
        loss += np.abs(q)
        g -= np.sign(q) * ag / (m + eps) ** 2
    return loss, g


def kink_margin(case, setting):
    """min over the case's pairs of | |m / (alpha g) - 1| | and | |alpha g / (m + eps) - 1| | (inf where the setting has no |.|)"""
    _, kind, terms, alpha, epoch = setting
    if kind != 2:
        return float('inf')
    m, t = pairs_of(base_of(case))
    lo, hi = S.pair_slice(case[0], rows_of(case))
    m, ag = m[lo:hi], LD(alpha) * t[lo:hi].astype(LD)
    if hi == lo:
        return float('inf')
    eps = LD(1) / LD(epoch + 1)
    return float(min(np.abs(m / ag - 1).min(), np.abs(ag / (m + eps) - 1).min()))


@functools.lru_cache(maxsize=None)
def oracle(case, name):
    """everything a comparison needs, for the case's row range: m, target (float32; the upstream g for `up`), loss, loss_scale,
    gx [k], gc [k], gcs [k] (the magnitude sums of the curvature gradients' terms)"""
    setting = SETTINGS[SETTING_IDS.index(name)]
    n = case[0]
    rows = rows_of(case)
    lo, hi = S.pair_slice(n, rows)
    m_all, t_all = pairs_of(base_of(case))
    m, t = m_all[lo:hi], t_all[lo:hi]
    terms, g = objective(m, t, setting)
    xs, craws = make_inputs(case)
    gx, gc, gcs = [], [], []
    for x, c, md in zip(xs, craws, modes_of(case)):
        if hi > lo:
            a, b, s = S.pdist_grads(x, c, md, True, g, rows)
        else:
            a, b, s = np.zeros(x.shape, dtype=LD), LD(0), LD(0)
        gx.append(a)
        gc.append(b)
        gcs.append(s)
    given = S.upstream(hi - lo) if setting[1] == 0 else t
    return dict(m=m, m_max=m_all.max(), target=given, loss=terms.sum(), loss_scale=np.abs(terms).sum(), g=g, gx=gx, gc=gc, gcs=gcs)


def spec_of(setting):
    """(loss_kind, alpha, eps, terms) as the C ABI takes them"""
    _, kind, terms, alpha, epoch = setting
    return kind, float(alpha), 1.0 / (epoch + 1), terms


def key(case, name, what, dname):
    """the recorded reference's array of a case and setting: 'prod/<case id>/<setting>/<what>_<dname>'"""
    return f'prod/{case_id(case)}/{name}/{what}_{dname}'
