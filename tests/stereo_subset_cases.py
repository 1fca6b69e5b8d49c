"""Cases, deterministic inputs and the LONG-DOUBLE oracle of the in-kernel node minibatch of a product of constant-curvature
factors (mm_stereo_product_loss_subset, csrc/stereo.hip).  Host code only: tables come from stereo_product_cases.make_inputs at
n_total, the batch is a fixed-seed permutation slice, the oracle is that of stereo_cases / stereo_product_cases on the GATHERED
rows, its gradients scattered into zero tables.

The case list is stated, not a cross product (17 cases):
  sizes   n_total = 257, bs in (2, 3, 64, 65, 129, 257 - a full permutation), ds = (5, 5), c = (0.01, -0.3), `spread`      6
  shapes  n_total = 129, bs = 65, ds in SHAPES, c cycling through C_CYCLE, `spread`                                        4
  init    n_total = 129, bs = 65, ds = (5, 5), c = (0.01, -0.3), `init`                                                    1
  shards  n_total = 257, bs = 129, ds = (5, 8), c = (0.01, -0.3), `spread`, every BATCH row range of
          stereo_cases._rows(129): the last row, which has no pair, and an empty range are among them                     6
and every case runs under the objective SETTINGS (stress, q1, q2, q3, q3b; an upstream gradient per pair has no dense form).

Targets are float32(m_oracle * F[k mod 4]) over the BATCH's pair index k, written symmetrically into a dense [n_total, n_total]
matrix whose every other entry, the diagonal included, is NaN; `poisoned` makes the table rows outside the batch NaN too: a
wrong gather cannot go unnoticed.  The quotient loss's kink is kept at a distance >= KINK as in stereo_product_cases (another idx
seed through SALT for a case that misses it; no pair is filtered out)."""
import functools

import numpy as np

import stereo_cases as S
import stereo_product_cases as P

LD = S.LD
SIZES = (2, 3, 64, 65, 129, 257)
SHAPES = ((1, 16), (2, 3, 5, 8), (2, ) * 8, (16, ) * 8)
SETTINGS = tuple(s for s in P.SETTINGS if s[1] != 0)
SETTING_IDS = [s[0] for s in SETTINGS]
RECORDED = ('stress', 'q3', 'q3b')   # the settings the reference record holds in fp64 (fp32: every setting)
KINK = P.KINK
SALT = {}   # case id -> offset of the idx seed


def _build():
    """(n_total, bs, ds, c_init, fixed, regime, rows)"""
    pair = ((0.01, -0.3), (False, False))
    cases = [(257, bs, (5, 5), *pair, 'spread', None) for bs in SIZES]
    cases += [(129, 65, ds, tuple(P.C_CYCLE[k % 4] for k in range(len(ds))), (False, ) * len(ds), 'spread', None) for ds in SHAPES]
    cases += [(129, 65, (5, 5), *pair, 'init', None)]
    cases += [(257, 129, (5, 8), *pair, 'spread', r) for r in S._rows(129)]
    return cases


CASES = _build()
SHARD_BASE = CASES[11]   # the whole batch the shards are parts of


def case_id(case):
    n_total, bs, ds, cs, fixed, regime, rows = case
    return f'b{bs}of' + P.case_id((n_total, ds, cs, fixed, regime, rows))


CASE_IDS = [case_id(c) for c in CASES]


def base_of(case):
    return case[:6] + (None, )


def table_case(case):
    """the stereo_product_cases case of the full tables"""
    n_total, bs, ds, cs, fixed, regime, _ = case
    return (n_total, ds, cs, fixed, regime, None)


def rows_of(case):
    return (0, case[1]) if case[6] is None else case[6]


def modes_of(case):
    return P.modes_of(table_case(case))


def batch_of(case):
    """idx int64 [bs]: a fixed-seed permutation slice (distinct, not monotone)"""
    n_total, bs = case[0], case[1]
    seed = 424200 + 1000 * n_total + bs + 7 * sum(case[2]) + 1000003 * SALT.get(case_id(base_of(case)), 0)
    return np.random.RandomState(seed).permutation(n_total)[:bs].astype(np.int64)


def make_inputs(case):
    """([x_k [n_total, d_k] float32], [c_raw_k float32], idx int64 [bs])"""
    xs, craws = P.make_inputs(table_case(case))
    return xs, craws, batch_of(case)


@functools.lru_cache(maxsize=None)
def pairs_of(base):
    """(m long double, target float32) over the batch's pair list"""
    xs, craws, idx = make_inputs(base)
    m = sum(S.pdist(x[idx], c, md, True) for x, c, md in zip(xs, craws, modes_of(base)))
    f = np.array(P.F, dtype=LD)[np.arange(len(m)) % 4]
    return m, (m * f).astype(np.float32)


def dense_of(case):
    """float32 [n_total, n_total]: the batch's targets at (idx[a], idx[b]) and (idx[b], idx[a]), NaN everywhere else"""
    n_total, bs = case[0], case[1]
    idx = batch_of(case)
    _, t = pairs_of(base_of(case))
    dense = np.full((n_total, n_total), np.nan, dtype=np.float32)
    a, b = np.triu_indices(bs, 1)
    dense[idx[a], idx[b]] = t
    dense[idx[b], idx[a]] = t
    return dense


def poisoned(x, idx):
    """the table with NaN in every row outside the batch"""
    out = np.full_like(x, np.nan)
    out[idx] = x[idx]
    return out


def kink_margin(case, setting):
    _, kind, terms, alpha, epoch = setting
    m, t = pairs_of(base_of(case))
    lo, hi = S.pair_slice(case[1], rows_of(case))
    if hi == lo:
        return float('inf')
    m, ag = m[lo:hi], LD(alpha) * t[lo:hi].astype(LD)
    eps = LD(1) / LD(epoch + 1)
    return float(min(np.abs(m / ag - 1).min(), np.abs(ag / (m + eps) - 1).min()))


@functools.lru_cache(maxsize=None)
def oracle(case, name):
    """m, target, loss, loss_scale over the case's batch row range; gx [k] as FULL tables (zero outside the batch), gc [k], gcs [k]"""
    setting = SETTINGS[SETTING_IDS.index(name)]
    n_total, bs = case[0], case[1]
    rows = rows_of(case)
    lo, hi = S.pair_slice(bs, rows)
    m_all, t_all = pairs_of(base_of(case))
    m, t = m_all[lo:hi], t_all[lo:hi]
    terms, g = P.objective(m, t, setting)
    xs, craws, idx = make_inputs(case)
    gx, gc, gcs = [], [], []
    for x, c, md in zip(xs, craws, modes_of(case)):
        full = np.zeros(x.shape, dtype=LD)
        if hi > lo:
            a, b, s = S.pdist_grads(x[idx], c, md, True, g, rows)
            full[idx] = a
        else:
            b, s = LD(0), LD(0)
        gx.append(full)
        gc.append(b)
        gcs.append(s)
    return dict(m=m, m_max=m_all.max(), target=t, loss=terms.sum(), loss_scale=np.abs(terms).sum(), gx=gx, gc=gc, gcs=gcs)


def key(case, name, what, dname):
    """the recorded reference's array: 'sub/<case id>/<setting>/<what>_<dname>' (gradients: the batch's rows, in idx order)"""
    return f'sub/{case_id(case)}/{name}/{what}_{dname}'
