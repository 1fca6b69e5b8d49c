"""TEST INFRASTRUCTURE ONLY — ctypes wrapper of oracle/exact.c (fp64, OpenMP)."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PATH = os.path.join(_HERE, '_build', 'liboracle_exact.so')
_lib = None
KINDS = {'euclidean': 0, 'lorentz': 1, 'sphere': 2}


def lib():
    global _lib
    if _lib is None:
        if not os.path.isfile(_PATH):
            import subprocess
            subprocess.check_call(['make', '-C', _HERE])
        _lib = ctypes.CDLL(_PATH)
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _chk(rc):
    if rc == -3:
        raise np.linalg.LinAlgError('input not positive definite')
    assert rc == 0, rc


def spd_pdist(x, squared=True, wmin=1e-8, wmax=1e8):
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, d = x.shape[0], x.shape[-1]
    out = np.empty(n * (n - 1) // 2)
    _chk(lib().oracle_spd_pdist(_p(x), ctypes.c_long(n), d, int(squared), ctypes.c_double(wmin),
                                ctypes.c_double(wmax), _p(out)))
    return out


def spd_pdist_grad(x, g, squared=True, wmin=1e-8, wmax=1e8):
    x = np.ascontiguousarray(x, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    n, d = x.shape[0], x.shape[-1]
    grad = np.empty_like(x)
    _chk(lib().oracle_spd_pdist_grad(_p(x), _p(g), ctypes.c_long(n), d, int(squared), ctypes.c_double(wmin),
                                     ctypes.c_double(wmax), _p(grad)))
    return grad


def vec_pdist(kind, x, squared=True):
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, m = x.shape
    out = np.empty(n * (n - 1) // 2)
    _chk(lib().oracle_vec_pdist(KINDS[kind], _p(x), ctypes.c_long(n), m, int(squared), _p(out)))
    return out


def vec_pdist_grad(kind, x, g, squared=True):
    x = np.ascontiguousarray(x, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    n, m = x.shape
    grad = np.empty_like(x)
    _chk(lib().oracle_vec_pdist_grad(KINDS[kind], _p(x), _p(g), ctypes.c_long(n), m, int(squared), _p(grad)))
    return grad


def _pair_list(n, lo, hi):
    lo = np.ascontiguousarray(lo, dtype=np.int64)
    hi = np.ascontiguousarray(hi, dtype=np.int64)
    assert lo.shape == hi.shape and lo.ndim == 1, (lo.shape, hi.shape)
    if lo.size and not (lo.min() >= 0 and hi.max() < n and (lo < hi).all()):
        raise ValueError('pair list needs 0 <= lo < hi < n')
    return lo, hi


def spd_pairs(x, lo, hi, squared=True, wmin=1e-8, wmax=1e8):
    """d (squared: d^2) of the pairs (lo[k], hi[k]) — spd_pdist on a pair list."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, d = x.shape[0], x.shape[-1]
    lo, hi = _pair_list(n, lo, hi)
    out = np.empty(lo.size)
    _chk(lib().oracle_spd_pairs(_p(x), ctypes.c_long(n), d, _p(lo), _p(hi), ctypes.c_long(lo.size), int(squared),
                                ctypes.c_double(wmin), ctypes.c_double(wmax), _p(out)))
    return out


def spd_pairs_grad(x, lo, hi, g, squared=True, wmin=1e-8, wmax=1e8):
    """d/dx of sum_k g[k] d(lo[k], hi[k]) (symmetric part), full [n, d, d]; zero on the points no pair touches."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, d = x.shape[0], x.shape[-1]
    lo, hi = _pair_list(n, lo, hi)
    g = np.ascontiguousarray(g, dtype=np.float64)
    assert g.shape == lo.shape
    grad = np.empty_like(x)
    _chk(lib().oracle_spd_pairs_grad(_p(x), ctypes.c_long(n), d, _p(lo), _p(hi), _p(g), ctypes.c_long(lo.size), int(squared),
                                     ctypes.c_double(wmin), ctypes.c_double(wmax), _p(grad)))
    return grad


def vec_pairs(kind, x, lo, hi, squared=True):
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, m = x.shape
    lo, hi = _pair_list(n, lo, hi)
    out = np.empty(lo.size)
    _chk(lib().oracle_vec_pairs(KINDS[kind], _p(x), ctypes.c_long(n), m, _p(lo), _p(hi), ctypes.c_long(lo.size), int(squared),
                                _p(out)))
    return out


def vec_pairs_grad(kind, x, lo, hi, g, squared=True):
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, m = x.shape
    lo, hi = _pair_list(n, lo, hi)
    g = np.ascontiguousarray(g, dtype=np.float64)
    assert g.shape == lo.shape
    grad = np.empty_like(x)
    _chk(lib().oracle_vec_pairs_grad(KINDS[kind], _p(x), ctypes.c_long(n), m, _p(lo), _p(hi), _p(g), ctypes.c_long(lo.size),
                                     int(squared), _p(grad)))
    return grad


def pair_index(n, lo, hi):
    """Linear index of pair (lo, hi) in the row-major upper triangle (torch.triu_indices(n, n, 1))."""
    lo = np.asarray(lo, dtype=np.int64)
    hi = np.asarray(hi, dtype=np.int64)
    return lo * (2 * n - lo - 1) // 2 + (hi - lo - 1)


def pair_of_index(n, k):
    """Inverse of pair_index: (lo, hi) of linear pair indices k (exact integer arithmetic after a float guess)."""
    k = np.asarray(k, dtype=np.int64)
    b = 2.0 * n - 1
    lo = np.floor((b - np.sqrt(b * b - 8.0 * k)) / 2).astype(np.int64)
    lo = np.clip(lo, 0, n - 2)
    for _ in range(3):
        lo = np.where(pair_index(n, lo, lo + 1) > k, lo - 1, lo)
        lo = np.where((lo + 1 <= n - 2) & (pair_index(n, lo + 1, lo + 2) <= k), lo + 1, lo)
    hi = k - pair_index(n, lo, lo + 1) + lo + 1
    return lo, hi
