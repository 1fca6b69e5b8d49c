"""GPU parity at the sizes where the pair kernels' 32-bit offsets are argued safe: pair vectors past 2^31 elements and 2^32
bytes, backward slices cut by the 32-bit cap (the multi-pass branch of spd_pdist_bwd_kernel), the share table's ncb < 2^16
limit, and the node limits of the entry points.

Whole pdists of these sizes are out of the oracle's reach, so every check is exact on a SAMPLE:
* forward: a pair set S (chosen rows, the pairs around linear index 2^31 and byte offsets 2^31 / 2^32, random pairs) gathered
  from the device's pair vector and compared with oracle/exact.c's pair-list entry points;
* backward: the upstream gradient is zero except on S, so the gradient must equal the oracle's over S — and be exactly zero
  on every point no pair of S touches (an atomic into the wrong row shows there);
* row shards of a few rows at the node limit: the whole shard against the oracle.

Each case first asserts, with a host mirror of the launcher's arithmetic (spd_pair.hpp spd_pdist_bwd_launch_sq, spd_ws.hpp
ColWalk / WalkShares), that it is in the regime it names — a case that does not reach it fails instead of passing vacuously —
and records the regime in the test's output (-rA)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'f64': torch.float64}
# DESIGN.md §5 (tests/test_spd_gpu.py, tests/test_vec_gpu.py)
D2_TOL = {'f32': (1e-6, 2e-5), 'f64': (1e-7, 2e-6)}
GRAD_TOL = {'f32': 2e-5, 'f64': 5e-6}
VEC_ABS = {'f32': 1e-6, 'f64': 1e-12}
VEC_REL = {'f32': 2e-5, 'f64': 1e-10}
VEC_GREL = {'f32': 5e-4, 'f64': 1e-9}
SHARD_TOL = {'f32': 1e-5, 'f64': 1e-13}     # test_row_sharding_is_exact
MM_ERR_ARG, MM_ERR_UNSUPPORTED = -1, -2
SPD_MAX_NODES = 1 << 22
TWO31, TWO32 = 1 << 31, 1 << 32


def pair_off(n, r):
    return r * (2 * n - r - 1) // 2


def need_free(nbytes, what):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes * 1.1:
        pytest.skip(f'{what}: needs {nbytes / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free')


def regime(request, text):
    """Records the regime a case asserted (printed with -rA / -s)."""
    print(f'[regime] {request.node.name}: {text}')


# ----------------------------------------------------------------------------------- host mirror of the SPD backward launch
def spd_bwd_cols(d, dname, pairs, two_cols_env=None):
    """Columns per lane of the launch (spd_pair.hpp pair_cols_bwd / kSpd4TwoColPairs; full launches only)."""
    if dname == 'f64':
        return 1
    if d in (2, 3):
        return 2
    if d == 4:
        return 2 if two_cols_env == '1' or (two_cols_env is None and pairs >= 30000000) else 1
    return 1


def spd_bwd_waves(d, dname):
    s = 4 if dname == 'f32' else 8
    return 4 if s * d * d * 64 * 4 <= 65536 else (2 if s * d * d * 64 * 2 <= 65536 else 1)


class ColWalk:
    """spd_ws.hpp ColWalk, in Python integers."""

    def __init__(self, n, rb, re, bw):
        self.bw, self.rb = bw, rb
        self.re = max(min(re, n - 1), rb)
        self.ncb = (n + bw - 1) // bw
        self.c0 = min((rb + 1) // bw, self.ncb)
        self.c1 = min(max(self.re // bw, self.c0), self.ncb)

    def hi(self, c):
        return np.minimum(self.bw * c + self.bw - 1, self.re)

    def prefix(self, c):
        c = np.asarray(c, dtype=np.int64)
        m = np.minimum(c, self.c1)
        s = (self.bw // 2) * (m * (m - 1) - self.c0 * (self.c0 - 1)) + (m - self.c0) * (self.bw - 1 - self.rb)
        s = s + np.maximum(c - self.c1, 0) * (self.re - self.rb)
        return np.where((c <= self.c0) | (self.re == self.rb), 0, s)

    def total(self):
        return int(self.prefix(self.ncb))


def spd_bwd_slices(n, rb, re, d, dname, cols, grid=None, cus=256):
    """The backward's walk as launched: for every grid the launcher can choose (or `grid`), the largest number of rows one
    workgroup's share holds in one column block, against NW * slice_cap (more = the multi-pass branch of the slice loop)."""
    size = 4 if dname == 'f32' else 8
    bw = 64 * cols
    walk = ColWalk(n, rb, re, bw)
    units = walk.total()
    nw = spd_bwd_waves(d, dname)
    slice_cap = max(16, min(1 << 20, TWO31 // (n * size)))
    cross = 16 if size == 4 else 8
    if grid is not None:
        grids = [grid]
    else:   # resident_workgroups = per_cu * cus, per_cu in 1..7, then at most 4 per CU and the small-launch rule
        grids = []
        for per_cu in range(1, 8):
            g = min(per_cu * cus, 4 * cus)
            half = max(1, cus // 2)
            by_rows = (units // 32 + half // 2) // half * half if cols >= 2 else units // 48 // cus * cus
            if by_rows < g:
                g = max(cus, by_rows)
            grids.append(g)
    grids = sorted({max(1, min(g, (units + 7) // 8)) for g in grids})
    c = np.arange(walk.c0, walk.ncb + 1, dtype=np.int64)
    ap = walk.prefix(c) + cross * (c - walk.c0)                      # aprefix of blocks c0 .. ncb
    worst = []
    for g in grids:
        total_aug = units + cross * (walk.ncb - walk.c0)
        q, r = divmod(total_aug, g)
        w = np.arange(g + 1, dtype=np.int64)
        bounds = q * w + np.minimum(w, r)
        cuts = np.unique(np.concatenate([ap, ap[:-1] + cross, bounds]))
        cuts = cuts[(cuts >= 0) & (cuts <= total_aug)]
        starts, lens = cuts[:-1], np.diff(cuts)
        blk = np.searchsorted(ap, starts, side='right') - 1
        in_rows = starts >= ap[blk] + cross
        worst.append(int(lens[in_rows].max()) if in_rows.any() else 0)
    return dict(units=units, grids=grids, ncb=walk.ncb, cap_rows=nw * slice_cap, min_share_rows=min(worst),
                multipass=min(worst) > nw * slice_cap, share_table_usable=walk.ncb < (1 << 16))


# ------------------------------------------------------------------------------------------------------ inputs and samples
def spd_points(n, d, seed, device='cuda'):
    """SPD points representable in fp32 (one fp64 copy serves the fp32 and the fp64 launch): A A^T / d + I/2, A ~ N(0, 1/2)."""
    g = torch.Generator(device=device).manual_seed(seed)
    a = torch.randn(n, d, d, generator=g, device=device) * 0.5
    x = a @ a.transpose(1, 2) / d + 0.5 * torch.eye(d, device=device)
    return 0.5 * (x + x.transpose(1, 2))                              # fp32, exactly symmetric


def sample_pairs(n, dname, rows_extra=(), n_random=None, seed=0, window=256, full_rows=False):
    """S: for the first rows, the rows whose pairs cross element 2^31 and byte offsets 2^31 / 2^32, the last rows of a column
    block and of the matrix — every pair (full_rows: the forward's S) or the pairs next to the diagonal, the last `window`
    columns and `window` columns either side of every crossing (the backward's S: whole rows would touch every point and
    leave the zero check on untouched points nothing to check); the pairs at 2^31 - 1, 2^31, 2^32 / sizeof(T) +- 1 and the
    last index; random pairs — 1e5, or n for the backward's S when that is fewer (a share of the points stays untouched).
    Returns (lo, hi, linear index, crossing indices), sorted and unique."""
    if n_random is None:
        n_random = 100000 if full_rows else min(100000, n)
    from oracle import exact
    size = 4 if dname == 'f32' else 8
    total = n * (n - 1) // 2
    ks = [k for k in (TWO31 - 1, TWO31, TWO32 // size - 1, TWO32 // size, TWO32 // size + 1, TWO31 // size - 1,
                      TWO31 // size, total - 1) if 0 <= k < total]
    kl, kh = exact.pair_of_index(n, np.array(ks, np.int64))
    rows = {0, 1, 63, 64, 127, 128, n - 65, n - 64, n - 3, n - 2} | set(rows_extra) | {int(r) for r in kl}
    lo, hi = [], []
    for r in sorted(r for r in rows if 0 <= r <= n - 2):
        cols = [np.arange(r + 1, min(r + 1 + window, n)), np.arange(max(r + 1, n - window), n)]
        cols += [np.arange(max(r + 1, h - window), min(n, h + window)) for l_, h in zip(kl, kh) if l_ == r]
        if full_rows:
            cols = [np.arange(r + 1, n)]
        c = np.unique(np.concatenate(cols))
        lo.append(np.full(c.size, r, np.int64))
        hi.append(c.astype(np.int64))
    rng = np.random.default_rng(seed)
    kr = rng.integers(0, total, size=n_random, dtype=np.int64)
    l2, h2 = exact.pair_of_index(n, np.concatenate([np.array(ks, np.int64), kr]))
    lo = np.concatenate(lo + [l2])
    hi = np.concatenate(hi + [h2])
    k = np.unique(exact.pair_index(n, lo, hi))
    lo, hi = exact.pair_of_index(n, k)
    return lo, hi, k, ks


def check_d2(got, ref, dname, what):
    got = np.asarray(got, np.float64)
    a, r = D2_TOL[dname]
    bad = np.abs(got - ref) - (a + r * np.abs(ref))
    assert np.isfinite(got).all(), what
    assert bad.max() <= 0, f'{what}: worst excess {bad.max():.3e} at {int(bad.argmax())}'


def check_grad(got, ref, tol, what, touched=None):
    got = np.asarray(got, np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref).max() / scale
    assert err <= tol, f'{what}: {err:.3e} > {tol:.1e}'
    if touched is not None:
        mask = np.ones(got.shape[0], bool)
        mask[touched] = False
        if mask.any():
            nz = np.flatnonzero(np.any(got[mask].reshape(int(mask.sum()), -1) != 0, axis=1))
            assert nz.size == 0, f'{what}: {nz.size} points no pair of S touches have a nonzero gradient'


# -------------------------------------------------------------------------------------------------------- C-ABI launches
def _spd_ws(T, n, d):
    from graphembed import _backend as B
    dt = B.dtype_code(torch.zeros(1, dtype=T))
    return torch.zeros(B.lib().raw('mm_spd_pdist_ws_bytes')(dt, n, d), dtype=torch.uint8, device='cuda')


def spd_fwd(x, rows, squared, ws=None):
    from graphembed import _backend as B
    n, d = x.shape[0], x.shape[-1]
    ws = _spd_ws(x.dtype, n, d) if ws is None else ws
    out = torch.empty(pair_off(n, rows[1]) - pair_off(n, rows[0]), dtype=x.dtype, device='cuda')
    B.lib().call('mm_spd_pdist_fwd', B.dtype_code(x), B.ptr(x), n, d, rows[0], rows[1], int(squared), 1e-8, 1e8, B.ptr(out),
                 B.ptr(ws), 0, B.stream_of(x))
    return out


def spd_bwd(x, g, rows, squared, ws=None):
    from graphembed import _backend as B
    n, d = x.shape[0], x.shape[-1]
    ws = _spd_ws(x.dtype, n, d) if ws is None else ws
    grad = torch.empty_like(x)
    B.lib().call('mm_spd_pdist_bwd', B.dtype_code(x), B.ptr(x), B.ptr(g), n, d, rows[0], rows[1], int(squared), 1e-8, 1e8,
                 B.ptr(grad), B.ptr(ws), 0, B.stream_of(x))
    return grad


def spd_loss(x, target, rows, kind, ws=None):
    from graphembed import _backend as B
    n, d = x.shape[0], x.shape[-1]
    ws = _spd_ws(x.dtype, n, d) if ws is None else ws
    grad = torch.empty_like(x)
    lo = torch.zeros(2, dtype=x.dtype, device='cuda')
    B.lib().call('mm_spd_pdist_loss', B.dtype_code(x), kind, B.ptr(x), B.ptr(target), None, n, d, rows[0], rows[1],
                 1.0, 0.5, 3, None, 1e-8, 1e8, B.ptr(lo), B.ptr(grad), B.ptr(ws), 0, B.stream_of(x))
    return lo, grad


def sparse_g(n, k, gk, T):
    g = torch.zeros(n * (n - 1) // 2, dtype=T, device='cuda')
    g[torch.from_numpy(k).cuda()] = torch.from_numpy(gk).to(T).cuda()
    return g


def spd_full_case(request, n, d, dname, seed, expect_multipass):
    """Full launch at n: sampled forward (squared and not), sparse backward (squared and not), untouched points exactly zero."""
    from oracle import exact
    T = DT[dname]
    size = torch.zeros(1, dtype=T).element_size()
    total = n * (n - 1) // 2
    need_free(2 * total * size + 2 * SPD_MAX_NODES * 200, f'SPD({d}) {dname} n = {n}')
    cols = spd_bwd_cols(d, dname, total)
    sl = spd_bwd_slices(n, 0, n, d, dname, cols)
    assert total * size > TWO32, 'pair vector below 2^32 bytes'
    if expect_multipass:
        assert sl['multipass'], f'no share spans more than NW x slice_cap = {sl["cap_rows"]} rows of a block: {sl}'
    if d == 4 and dname == 'f32':
        assert cols == 2, 'SPD(4) fp32 launch below the two-column threshold'
    regime(request, f'SPD({d}) {dname} n={n}: pairs {total} ({"> 2^31" if total > TWO31 else "< 2^31"}), bytes {total * size} > 2^32, '
                    f'{cols} col(s)/lane, multi-pass slices {sl["multipass"]} (share rows >= {sl["min_share_rows"]} vs '
                    f'{sl["cap_rows"]}, grids {sl["grids"]}), ncb {sl["ncb"]}')
    x32 = spd_points(n, d, seed)
    x = x32.to(T)
    x64 = x32.double().cpu().numpy()
    lo, hi, k, ks = sample_pairs(n, dname, rows_extra=(n // 2,), seed=seed, full_rows=True)
    kd = torch.from_numpy(k).cuda()
    ws = _spd_ws(T, n, d)
    for squared in (True, False):
        out = spd_fwd(x, (0, n), squared, ws)
        got = out[kd].double().cpu().numpy()
        del out
        ref = exact.spd_pairs(x64, lo, hi, squared=squared)
        check_d2(got if squared else got ** 2, ref if squared else ref ** 2, dname, f'd2 on S (squared={squared})')
    lo, hi, k, ks = sample_pairs(n, dname, rows_extra=(n // 2,), seed=seed)
    rng = np.random.default_rng(seed + 1)
    gk = rng.standard_normal(k.size)
    gk32 = gk.astype(np.float32).astype(np.float64) if dname == 'f32' else gk
    g = sparse_g(n, k, gk32, T)
    touched = np.unique(np.concatenate([lo, hi]))
    assert n - touched.size >= 1000, 'S touches nearly every point'
    for squared in (True, False):
        gr = spd_bwd(x, g, (0, n), squared, ws).double().cpu().numpy()
        ref = exact.spd_pairs_grad(x64, lo, hi, gk32, squared=squared)
        check_grad(gr, ref, GRAD_TOL[dname], f'sparse backward (squared={squared})', touched)
    del g
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- cases
def test_a_spd3_fp32_full_past_2_31_pairs(request):
    spd_full_case(request, 65600, 3, 'f32', 1, expect_multipass=False)


@pytest.mark.parametrize('d,n,dname,multipass', [(3, 65600, 'f64', True), (4, 50000, 'f32', False)])
def test_b_spd_fp64_and_spd4_two_columns(request, d, n, dname, multipass):
    spd_full_case(request, n, d, dname, 2 + d, expect_multipass=multipass)


C_GRID = 64


def _case_c_child(out_path):
    """(child process, MM_SPD_BWD_GRID set) fp32 SPD(3) n = 50000, dense random g: the full backward and 8 row-shard
    launches, and the sparse oracle check."""
    from graphembed import _backend as B
    from oracle import exact
    n, d, T = 50000, 3, torch.float32
    x32 = spd_points(n, d, 7)
    gen = torch.Generator(device='cuda').manual_seed(8)
    g = torch.randn(n * (n - 1) // 2, generator=gen, device='cuda')
    ws = _spd_ws(T, n, d)
    full = spd_bwd(x32, g, (0, n), True, ws)
    gsum = torch.zeros_like(x32)
    for r in range(8):
        rb, re = B.shard_rows(n, 8, r)
        gsum += spd_bwd(x32, g[pair_off(n, rb):pair_off(n, re)], (rb, re), True, ws)
    err = float((gsum - full).abs().max() / full.abs().max())
    del g
    lo, hi, k, _ = sample_pairs(n, 'f32', seed=9)
    gk = np.random.default_rng(10).standard_normal(k.size).astype(np.float32).astype(np.float64)
    sp = spd_bwd(x32, sparse_g(n, k, gk, T), (0, n), True, ws).double().cpu().numpy()
    ref = exact.spd_pairs_grad(x32.double().cpu().numpy(), lo, hi, gk)
    untouched = np.ones(n, bool)
    untouched[np.unique(np.concatenate([lo, hi]))] = False
    np.savez(out_path, shard_err=err, oracle_err=np.abs(sp - ref).max() / np.abs(ref).max(),
             untouched_nonzero=int(np.any(sp[untouched] != 0, axis=(1, 2)).sum()))


def test_c_multipass_slices_fp32_dense_g(request, tmp_path):
    n, d = 50000, 3
    need_free(2 * n * (n - 1) // 2 * 4 + (1 << 30), 'SPD(3) fp32 n = 50000')
    sl = spd_bwd_slices(n, 0, n, d, 'f32', 2, grid=C_GRID)
    assert sl['multipass'], sl
    default = spd_bwd_slices(n, 0, n, d, 'f32', 2)
    regime(request, f'SPD(3) fp32 n={n} MM_SPD_BWD_GRID={C_GRID}: multi-pass slices (share rows {sl["min_share_rows"]} > '
                    f'{sl["cap_rows"]}); at the default grids {default["grids"]}: multi-pass {default["multipass"]}')
    out = tmp_path / 'c.npz'
    env = dict(os.environ, MM_SPD_BWD_GRID=str(C_GRID))
    r = subprocess.run(['timeout', '-k', '10', '600', sys.executable, os.path.abspath(__file__), 'case_c', str(out)],
                       env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out)
    assert float(z['shard_err']) <= SHARD_TOL['f32'], float(z['shard_err'])
    assert float(z['oracle_err']) <= GRAD_TOL['f32'], float(z['oracle_err'])
    assert int(z['untouched_nonzero']) == 0


@pytest.fixture(scope='module')
def limit_points():
    """Points at the SPD node limit, per d: fp32-representable, on the device (the fp64 launch casts them)."""
    cache = {}

    def get(d):
        if d not in cache:
            cache.clear()
            torch.cuda.empty_cache()
            x = spd_points(SPD_MAX_NODES, d, 40 + d)
            cache[d] = (x, x.double().cpu().numpy())
        return cache[d]
    return get


@pytest.mark.parametrize('d', [2, 3, 4])
def test_d_row_shards_at_the_spd_node_limit(request, limit_points, d):
    """Shards of two rows at n = 2^22 (ncb = 2^16 for the one-column walks: share table unusable) and n = 2^22 - 64
    (usable): forward on the whole shard, backward with dense random g, the fused stress and quotient losses, launch-to-launch
    agreement; n = 2^22 + 1 is refused."""
    from graphembed import _backend as B
    from oracle import exact
    lib = B.lib()
    xfull, x64full = limit_points(d)
    notes = []
    for n in (SPD_MAX_NODES, SPD_MAX_NODES - 64):
        x32 = xfull[:n]
        x64 = x64full[:n]
        for rb in (0, n // 2, n - 5):
            rows = (rb, rb + 2)
            lo_k, hi_k = pair_off(n, rows[0]), pair_off(n, rows[1])
            lo = np.concatenate([np.full(n - 1 - r, r, np.int64) for r in range(*rows)])
            hi = np.concatenate([np.arange(r + 1, n, dtype=np.int64) for r in range(*rows)])
            ref = exact.spd_pairs(x64, lo, hi)
            gk = np.random.default_rng(rb + n + d).standard_normal(lo.size).astype(np.float32).astype(np.float64)
            ref_g = exact.spd_pairs_grad(x64, lo, hi, gk)
            target = (ref * np.random.default_rng(rb + d).uniform(0.5, 1.5, ref.size)).astype(np.float32).astype(np.float64)
            stress = float(((ref - target) ** 2).sum())
            target1 = (ref * np.random.default_rng(rb + d + 1).uniform(0, 0.5, ref.size)).astype(np.float32).astype(np.float64)
            stress1 = float(((ref - target1) ** 2).sum())
            stress1_g = exact.spd_pairs_grad(x64, lo, hi, 2 * (ref - target1))
            for dname in ('f32', 'f64'):
                T = DT[dname]
                x = x32.to(T)
                cols = spd_bwd_cols(d, dname, hi_k - lo_k)
                sl = spd_bwd_slices(n, rows[0], rows[1], d, dname, cols)
                if cols == 1:
                    assert sl['share_table_usable'] == (n < SPD_MAX_NODES), sl
                notes.append(f'n={n} rb={rb} {dname}: ncb {sl["ncb"]} share table {"usable" if sl["share_table_usable"] else "UNUSABLE"}')
                ws = _spd_ws(T, n, d)
                out = spd_fwd(x, rows, True, ws)
                assert out.numel() == ref.size
                check_d2(out.double().cpu().numpy(), ref, dname, f'd2 n={n} rows={rows} {dname}')
                assert torch.equal(spd_fwd(x, rows, True, ws), out), 'forward not reproducible'
                g = torch.from_numpy(gk).to(T).cuda()
                g1 = spd_bwd(x, g, rows, True, ws)
                g2 = spd_bwd(x, g, rows, True, ws)                      # (the second launch may read the remembered starts)
                got = g1.double().cpu().numpy()
                check_grad(got, ref_g, GRAD_TOL[dname], f'grad n={n} rows={rows} {dname}',
                           touched=np.arange(rows[0], n))
                scale = float(g1.abs().max())
                # (not bit for bit: the row sums of a shard leave through float atomics from many workgroups, whose order
                # varies; the bound is test_share_table_in_the_workspace_is_self_validating's)
                assert float((g2 - g1).abs().max()) <= (5e-6 if dname == 'f32' else 1e-12) * scale
                tgt = torch.from_numpy(target).to(T).cuda()
                lv, _ = spd_loss(x, tgt, rows, 1, ws)
                assert abs(float(lv[0]) - stress) <= (1e-4 if dname == 'f32' else 1e-10) * abs(stress), (float(lv[0]), stress)
                # The stress weights 2 (d2 - t) of the target above cancel over a row of ~4 M pairs, so the row node's gradient
                # is ill-conditioned in d2: a relative d2 bias far inside the d2 tolerance (6e-8) moves it by ~5e-4 of
                # max|grad|, and the fused kernel evaluates d2 in its own loop, not bit-equal to the forward's (measured against
                # the forward kernel's d2: SPD(2) / SPD(4) within 2e-5, fp32 SPD(3) 3.7e-4).  The accumulation is therefore checked with a target whose weights do not cancel, t = d2 U(0, 1/2):
                # the row sums must then match the exact gradient to the stated tolerance — a dropped or misplaced slice of
                # the 4 M pairs could not.  The d2 are held to their own tolerance above; their bias is recorded.
                d2k = out.double().cpu().numpy()
                lv1, lg = spd_loss(x, torch.from_numpy(target1).to(T).cuda(), rows, 1, ws)
                assert abs(float(lv1[0]) - stress1) <= (1e-4 if dname == 'f32' else 1e-10) * abs(stress1)
                check_grad(lg.double().cpu().numpy(), stress1_g, GRAD_TOL[dname], f'stress grad n={n} rows={rows} {dname}',
                           np.arange(rows[0], n))
                bias = float(np.mean((d2k - ref) / ref))
                notes.append(f'd2 mean relative bias {dname} d={d}: {bias:+.1e}')
                m = ref
                quot = float((np.abs(m / target - 1) + np.abs(target / (m + 0.5) - 1)).sum())
                qv, _ = spd_loss(x, tgt, rows, 2, ws)
                assert abs(float(qv[0]) - quot) <= (1e-4 if dname == 'f32' else 1e-10) * abs(quot), (float(qv[0]), quot)
                del ws, out, g, g1, g2
                torch.cuda.empty_cache()
    # one node past the limit: refused before anything is launched (buffers sized for the launch the arguments describe, so
    # that a refusal that regressed would fail an assertion, not address outside a buffer)
    n = SPD_MAX_NODES + 1
    xb = torch.zeros(n, d, d, device='cuda')
    pv = torch.zeros(2 * n - 3, device='cuda')
    gb = torch.empty_like(xb)
    wsb = torch.zeros(max(lib.raw('mm_spd_pdist_ws_bytes')(0, n, d), lib.raw('mm_spd_pdist_ws_bytes')(0, SPD_MAX_NODES, d)),
                      dtype=torch.uint8, device='cuda')
    assert lib.raw('mm_spd_pdist_fwd')(0, B.ptr(xb), n, d, 0, 2, 1, 1e-8, 1e8, B.ptr(pv), B.ptr(wsb), 0,
                                       B.stream_of(xb)) == MM_ERR_ARG
    assert lib.raw('mm_spd_pdist_bwd')(0, B.ptr(xb), B.ptr(pv), n, d, 0, 2, 1, 1e-8, 1e8, B.ptr(gb), B.ptr(wsb), 0,
                                       B.stream_of(xb)) == MM_ERR_ARG
    del xb, pv, gb, wsb
    torch.cuda.synchronize()
    regime(request, '; '.join(sorted(set(notes))))


# ---------------------------------------------------------------------------------------------------------------- Stein
def _stein64(xl, xh):
    """Stein divergence of the pairs (fp64 torch restatement of include/mm_manifolds.h's formula, autograd-ready)."""
    return torch.logdet(0.5 * (xl + xh)) - 0.5 * (torch.logdet(xl) + torch.logdet(xh))


def test_e_stein_full_past_2_31_pairs(request):
    """mm_spd_stein_pdiv_fwd / _bwd, SPD(3) fp32 at n = 65 600: forward on S (whole rows), sparse backward against the fp64
    restatement on the gathered pairs (tolerances of test_stein_vs_oracle_seeded_and_shards)."""
    from graphembed import _backend as B
    n, d, T = 65600, 3, torch.float32
    total = n * (n - 1) // 2
    need_free(2 * total * 4 + (1 << 30), 'Stein SPD(3) fp32 n = 65600')
    assert total > TWO31 and total * 4 > TWO32
    x = spd_points(n, d, 21)
    x64 = x.double().cpu()
    ws = _spd_ws(T, n, d)
    lib = B.lib()
    out = torch.empty(total, dtype=T, device='cuda')
    lib.call('mm_spd_stein_pdiv_fwd', 0, B.ptr(x), n, d, 0, n, 1, 1e-8, B.ptr(out), B.ptr(ws), 0, B.stream_of(x))
    lo, hi, k, _ = sample_pairs(n, 'f32', seed=21, full_rows=True)
    got = out[torch.from_numpy(k).cuda()].double().cpu().numpy()
    del out
    ref = _stein64(x64[lo], x64[hi]).clamp_min(1e-8).numpy()
    err = np.abs(got - ref) - (2e-6 + 2e-5 * np.abs(ref))
    assert err.max() <= 0, f'Stein on S: worst excess {err.max():.3e}'
    lo, hi, k, _ = sample_pairs(n, 'f32', seed=22)
    gk = np.random.default_rng(23).standard_normal(k.size).astype(np.float32).astype(np.float64)
    g = sparse_g(n, k, gk, T)
    grad = torch.empty_like(x)
    lib.call('mm_spd_stein_pdiv_bwd', 0, B.ptr(x), B.ptr(g), n, d, 0, n, 1, 1e-8, B.ptr(grad), B.ptr(ws), 0, B.stream_of(x))
    del g
    lt, ht = torch.from_numpy(lo), torch.from_numpy(hi)
    xl, xh = x64[lt].clone().requires_grad_(), x64[ht].clone().requires_grad_()
    gl, gh = torch.autograd.grad((_stein64(xl, xh) * torch.from_numpy(gk)).sum(), [xl, xh])
    ref_g = torch.zeros_like(x64).index_add_(0, lt, gl).index_add_(0, ht, gh)
    ref_g = 0.5 * (ref_g + ref_g.transpose(1, 2))
    check_grad(grad.double().cpu().numpy(), ref_g.numpy(), 5e-5, 'Stein sparse grad', np.unique(np.concatenate([lo, hi])))
    torch.cuda.synchronize()
    regime(request, f'Stein SPD(3) fp32 n={n}: pairs {total} > 2^31, bytes {total * 4} > 2^32')


# ------------------------------------------------------------------------------------------------------- node minibatches
H_NTOTAL, H_BS = 50000, 512


@pytest.fixture(scope='module')
def dense_target():
    """A dense n_total x n_total fp32 target (10 GB: n_total^2 > 2^31 elements, > 2^33 bytes)."""
    need_free(H_NTOTAL * H_NTOTAL * 4 + (2 << 30), 'dense minibatch target')
    gen = torch.Generator(device='cuda').manual_seed(31)
    dense = torch.rand(H_NTOTAL, H_NTOTAL, generator=gen, device='cuda') * 2 + 0.1
    yield dense
    del dense
    torch.cuda.empty_cache()


def minibatch_idx():
    """512 distinct nodes, in batch order: first the rows whose dense row starts just below element 2^31 and byte offset
    2^32 (node * n_total + column crosses them), then random nodes, the first and last node among them."""
    n = H_NTOTAL
    r31, r32 = TWO31 // n, (TWO32 // 4) // n
    rng = np.random.default_rng(32)
    rest = rng.choice(np.setdiff1d(np.arange(n), [r31, r32, 0, n - 1]), H_BS - 4, replace=False)
    idx = np.concatenate([[r31, r32], rest[:100], [0, n - 1], rest[100:]]).astype(np.int64)
    assert np.unique(idx).size == H_BS
    a, b = np.triu_indices(H_BS, 1)
    elem = idx[a] * n + idx[b]                                       # dense element of each batch pair's target
    assert (elem < TWO31).any() and (elem >= TWO31).any(), 'no batch pair on either side of element 2^31'
    assert (elem < TWO32 // 4).any() and (elem >= TWO32 // 4).any(), 'no batch pair on either side of byte offset 2^32'
    assert (idx[a] == r31).any() and ((idx[a] == r31) & (elem >= TWO31)).any()
    return idx


@pytest.mark.parametrize('what', ['spd2', 'spd3', 'lorentz11'])
def test_h_node_minibatch_with_a_dense_target_past_2_31(request, dense_target, what):
    """mm_spd_pdist_loss_subset / mm_vec_pdist_loss_subset, fp32 stress loss: a 512-node batch of n_total = 50 000 whose
    targets lie on both sides of element 2^31 and byte offset 2^32 of the dense matrix, against the fp64 loss and gradient of
    the gathered 512-node problem (scattered into rows idx; every other row exactly zero)."""
    from graphembed import _backend as B
    from oracle import exact
    lib = B.lib()
    n, bs = H_NTOTAL, H_BS
    idx = minibatch_idx()
    idx_d = torch.from_numpy(idx).cuda()
    sub = dense_target[idx_d][:, idx_d].double().cpu().numpy()
    a, b = np.triu_indices(bs, 1)
    t = sub[a, b]
    lo_out = torch.zeros(2, device='cuda')
    if what.startswith('spd'):
        d = int(what[3:])
        x = spd_points(n, d, 33 + d)
        xb = x[idx_d].contiguous()
        d2k = spd_fwd(xb, (0, bs), True).double().cpu().numpy()     # the kernel's d2 of the batch (see case d)
        d2 = exact.spd_pdist(xb.double().cpu().numpy())
        gsub = exact.spd_pdist_grad(xb.double().cpu().numpy(), 2 * (d2k - t))
        ws = _spd_ws(torch.float32, n, d)
        grad = torch.empty_like(x)
        lib.call('mm_spd_pdist_loss_subset', 0, 1, B.ptr(x), B.ptr(dense_target), None, n, d, B.ptr(idx_d), bs, 0, bs,
                 1.0, 0.5, 3, None, 1e-8, 1e8, B.ptr(lo_out), B.ptr(grad), B.ptr(ws), 0, B.stream_of(x))
        check_d2(d2k, d2, 'f32', 'batch d2')
        tol = GRAD_TOL['f32']
    else:
        m = 11
        x = vec_points('lorentz', n, m, 34)
        xb = x[idx_d].contiguous()
        xb64 = xb.double().cpu().numpy()
        d2 = exact.vec_pdist('lorentz', xb64, True)
        gsub = exact.vec_pdist_grad('lorentz', xb64, 2 * (d2 - t), True)
        ws = torch.zeros(lib.raw('mm_vec_pdist_ws_bytes')(0, n, m), dtype=torch.uint8, device='cuda')
        grad = torch.empty_like(x)
        lib.call('mm_vec_pdist_loss_subset', 0, 1, 1, B.ptr(x), B.ptr(dense_target), None, n, m, B.ptr(idx_d), bs, 0, bs,
                 1.0, 0.5, 3, None, B.ptr(lo_out), B.ptr(grad), B.ptr(ws), B.stream_of(x))
        tol = VEC_GREL['f32']
    loss = float(((d2 - t) ** 2).sum())
    assert abs(float(lo_out[0]) - loss) <= 1e-4 * abs(loss), (float(lo_out[0]), loss)
    ref = np.zeros(grad.shape)
    ref[idx] = gsub
    check_grad(grad.double().cpu().numpy(), ref, tol, f'{what} minibatch grad', idx)
    torch.cuda.synchronize()
    regime(request, f'{what} fp32 n_total={n}, batch {bs}: dense target {n * n} > 2^31 elements ({n * n * 4} bytes); batch '
                    f'pairs on both sides of element 2^31 and byte offset 2^32')


# ------------------------------------------------------------------------------------------------------- vector manifolds
def vec_points(kind, n, m, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(n, m, generator=g, device='cuda')
    if kind == 'sphere':   # (a cap of the sphere: fp32 acos is ill-conditioned at antipodal pairs, which m = 2 meets often)
        x[:, 0] = x[:, 0].abs() + 3
        x = x / x.norm(dim=1, keepdim=True)
    elif kind == 'lorentz':
        x = x * 0.3
        x[:, 0] = torch.sqrt(1 + (x[:, 1:].double() ** 2).sum(1)).float()
    return x                                                          # fp32; the oracle reads the same values in fp64


VEC_KIND = {'euclidean': 0, 'lorentz': 1, 'sphere': 2}


def vec_fwd(kind, x, rows, squared):
    from graphembed import _backend as B
    n, m = x.shape
    out = torch.empty(pair_off(n, rows[1]) - pair_off(n, rows[0]), dtype=x.dtype, device='cuda')
    B.lib().call('mm_vec_pdist_fwd', B.dtype_code(x), VEC_KIND[kind], B.ptr(x), n, m, rows[0], rows[1], int(squared), B.ptr(out),
                 B.stream_of(x))
    return out


def vec_bwd_rc(kind, x, g, rows, squared):
    from graphembed import _backend as B
    n, m = x.shape
    dt = B.dtype_code(x)
    ws = torch.zeros(B.lib().raw('mm_vec_pdist_ws_bytes')(dt, n, m), dtype=torch.uint8, device='cuda')
    grad = torch.empty_like(x)
    rc = B.lib().raw('mm_vec_pdist_bwd')(dt, VEC_KIND[kind], B.ptr(x), B.ptr(g), n, m, rows[0], rows[1], int(squared),
                                         B.ptr(grad), B.ptr(ws), B.stream_of(x))
    return rc, grad


def check_vec(got, ref, dname, m, what):
    s = max(1, m // 8)
    bad = np.abs(np.asarray(got, np.float64) - ref) - s * (VEC_ABS[dname] + VEC_REL[dname] * np.abs(ref))
    assert bad.max() <= 0, f'{what}: worst excess {bad.max():.3e}'


VEC_CASES = [('lorentz', 11), ('sphere', 2), ('sphere', 11), ('sphere', 64), ('euclidean', 2), ('euclidean', 11),
             ('euclidean', 64)]
ORDERED_CASES = [('lorentz', 11), ('sphere', 64), ('euclidean', 2)]


def _vec_full(kind, m, dname, n, seed):
    """Sampled forward and sparse backward of a full launch; run in-process and by the ordered-backward child."""
    from oracle import exact
    T = DT[dname]
    x32 = vec_points(kind, n, m, seed)
    x = x32.to(T)
    x64 = x32.double().cpu().numpy()
    lo, hi, k, _ = sample_pairs(n, dname, seed=seed, full_rows=True)
    kd = torch.from_numpy(k).cuda()
    out = vec_fwd(kind, x, (0, n), True)
    got = out[kd].double().cpu().numpy()
    del out
    check_vec(got, exact.vec_pairs(kind, x64, lo, hi, True), dname, m, f'{kind}({m}) {dname} d2 on S')
    lo, hi, k, _ = sample_pairs(n, dname, seed=seed)
    touched = np.unique(np.concatenate([lo, hi]))
    assert n - touched.size >= 1000
    gk = np.random.default_rng(seed).standard_normal(k.size).astype(np.float32).astype(np.float64)
    g = sparse_g(n, k, gk, T)
    rc, gr = vec_bwd_rc(kind, x, g, (0, n), True)
    assert rc == 0, rc
    del g
    check_grad(gr.double().cpu().numpy(), exact.vec_pairs_grad(kind, x64, lo, hi, gk, True), VEC_GREL[dname],
               f'{kind}({m}) {dname} sparse grad', touched)


@pytest.mark.parametrize('kind,m', VEC_CASES)
@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_f_vector_full_launch_past_2_31_pairs(request, kind, m, dname):
    n = 70000
    total = n * (n - 1) // 2
    size = 4 if dname == 'f32' else 8
    need_free(2 * total * size + (1 << 30), f'{kind}({m}) {dname} n = {n}')
    assert total > TWO31 and total * size > TWO32
    regime(request, f'{kind}({m}) {dname} n={n}: pairs {total} > 2^31, bytes {total * size} > 2^32 (symmetric backward)')
    _vec_full(kind, m, dname, n, 60 + m)
    torch.cuda.synchronize()


def _case_f_ordered_child():
    for kind, m in ORDERED_CASES:
        _vec_full(kind, m, 'f32', 70000, 80 + m)
    torch.cuda.synchronize()


def test_f_vector_ordered_backward_past_2_31_pairs(request):
    """MM_VEC_BWD_ORDERED=1 (the ordered-pair fallback) at the same n, in a child process."""
    n = 70000
    need_free(2 * n * (n - 1) // 2 * 4 + (1 << 30), 'ordered vector backward n = 70000')
    regime(request, f'{ORDERED_CASES} fp32 n={n} ordered backward: pairs {n * (n - 1) // 2} > 2^31, grid y {(n + 63) // 64}')
    env = dict(os.environ, MM_VEC_BWD_ORDERED='1')
    r = subprocess.run(['timeout', '-k', '10', '600', sys.executable, os.path.abspath(__file__), 'case_f_ordered'],
                       env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize('kind,m', [('lorentz', 11), ('sphere', 2)])
def test_f_vector_row_shards_at_the_node_limits(request, kind, m):
    """Row shards at n = 2^22 (forward and symmetric backward) and forward-only shards at n = 2^24; the backward above 2^22
    nodes is refused (MM_ERR_UNSUPPORTED), not launched."""
    from oracle import exact
    for n, with_bwd in ((SPD_MAX_NODES, True),) + (((1 << 24, False),) if m <= 16 else ()):
        x32 = vec_points(kind, n, m, 90 + m)
        x64 = x32.double().cpu().numpy()
        for rb in (0, n // 2, n - 5):
            rows = (rb, rb + 2)
            lo = np.concatenate([np.full(n - 1 - r, r, np.int64) for r in range(*rows)])
            hi = np.concatenate([np.arange(r + 1, n, dtype=np.int64) for r in range(*rows)])
            ref = exact.vec_pairs(kind, x64, lo, hi, True)
            gk = np.random.default_rng(rb).standard_normal(lo.size).astype(np.float32).astype(np.float64)
            ref_g = exact.vec_pairs_grad(kind, x64, lo, hi, gk, True) if with_bwd else None
            for dname in ('f32', 'f64'):
                x = x32.to(DT[dname])
                out = vec_fwd(kind, x, rows, True)
                assert out.numel() == lo.size
                check_vec(out.double().cpu().numpy(), ref, dname, m, f'{kind}({m}) n={n} rows={rows} {dname}')
                if with_bwd:
                    rc, gr = vec_bwd_rc(kind, x, torch.from_numpy(gk).to(DT[dname]).cuda(), rows, True)
                    assert rc == 0, rc
                    check_grad(gr.double().cpu().numpy(), ref_g, VEC_GREL[dname], f'{kind}({m}) n={n} rows={rows} {dname} grad',
                               np.arange(rows[0], n))
                del out
        del x32
        torch.cuda.empty_cache()
    # the backward one node past 2^22: refused, nothing launched (the ordered fallback's grid height is n / 64; g sized for
    # the rows (0, 2) it names, so that a refusal that regressed fails here instead of reading outside a buffer)
    n = SPD_MAX_NODES + 1
    x = torch.zeros(n, m, device='cuda')
    rc, _ = vec_bwd_rc(kind, x, torch.zeros(2 * n - 3, device='cuda'), (0, 2), True)
    assert rc == MM_ERR_UNSUPPORTED, rc
    torch.cuda.synchronize()
    regime(request, f'{kind}({m}): shards at n = 2^22 (fwd + bwd) and 2^24 (fwd; pair offsets near 2^47); bwd at 2^22 + 1 refused')


# ------------------------------------------------------------------------------------------------------------ Gram kernels
@pytest.mark.parametrize('n', [32768, 32769])
def test_g_gram_kernels_at_their_limit(request, n):
    """mm_vec_pdist_fwd_gram / mm_vec_pdist_bwd_gram at n = 32768 against the oracle; at 32769 both refuse
    (MM_ERR_UNSUPPORTED) and the Python layer — Lorentz(24) fp32, which takes both matrix-core forms up to 32768 — takes the
    VALU kernels without a word, with the same numbers."""
    from graphembed import _backend as B
    from graphembed.manifolds import Lorentz
    from graphembed.manifolds.vector import _pdist_forms
    from oracle import exact
    kind, m = 'lorentz', 24
    forms = _pdist_forms(B.LORENTZ, m, n, True, True, True)
    assert forms == ((True, True) if n <= 32768 else (False, False)), forms
    x32 = vec_points(kind, n, m, 5)
    x64 = x32.double().cpu().numpy()
    lo, hi, k, _ = sample_pairs(n, 'f32', seed=5)
    kd = torch.from_numpy(k).cuda()
    ref = exact.vec_pairs(kind, x64, lo, hi, True)
    out = torch.empty(n * (n - 1) // 2, device='cuda')
    rc = B.lib().raw('mm_vec_pdist_fwd_gram')(0, 1, B.ptr(x32), n, m, 0, n, 1, B.ptr(out), B.stream_of(x32))
    if n <= 32768:
        assert rc == 0, rc
        check_vec(out[kd].double().cpu().numpy(), ref, 'f32', m, f'gram fwd n={n}')
    else:
        assert rc == MM_ERR_UNSUPPORTED, rc
    del out
    gk = np.random.default_rng(6).standard_normal(k.size).astype(np.float32).astype(np.float64)
    g = sparse_g(n, k, gk, torch.float32)
    grad = torch.empty_like(x32)
    rc = B.lib().raw('mm_vec_pdist_bwd_gram')(0, 1, B.ptr(x32), B.ptr(g), n, m, 0, n, 1, B.ptr(grad), B.stream_of(x32))
    ref_g = exact.vec_pairs_grad(kind, x64, lo, hi, gk, True)
    touched = np.unique(np.concatenate([lo, hi]))
    if n <= 32768:
        assert rc == 0, rc
        check_grad(grad.double().cpu().numpy(), ref_g, VEC_GREL['f32'], 'gram bwd', touched)
    else:
        assert rc == MM_ERR_UNSUPPORTED, rc
    man = Lorentz(m)
    assert man.use_gram
    xr = x32.clone().requires_grad_()
    d2 = man.pdist(xr, squared=True)
    check_vec(d2.detach()[kd].double().cpu().numpy(), ref, 'f32', m, f'pdist n={n}')
    gr, = torch.autograd.grad(d2, xr, g)
    check_grad(gr.double().cpu().numpy(), ref_g, VEC_GREL['f32'], f'pdist backward n={n}', touched)
    torch.cuda.synchronize()
    regime(request, f'Lorentz(24) fp32 n={n}: ' + ('matrix-core forward and backward' if n <= 32768 else
                                                   'matrix-core forms refused, the Python layer took the VALU kernels'))


# -------------------------------------------------------------------------------------------------------------- row sort
def test_j_graph_sort_rows_at_its_bound(request):
    from graphembed import _backend as B
    lib = B.lib()
    n = 46340
    assert n * n < TWO31 < (n + 1) * (n + 1)
    need_free((n + 1) * (n + 1) * 8 * 2 + (1 << 30), 'row sort n = 46340')
    gen = torch.Generator(device='cuda').manual_seed(3)
    # a few distinct values per row (ties: the sort is stable, ties in node order)
    dist = torch.randint(0, 1000, (n, n), generator=gen, device='cuda').float()
    nbytes = lib.raw('mm_graph_sort_rows_ws_bytes')(0, n)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    order = torch.empty(n, n, dtype=torch.int32, device='cuda')
    lib.call('mm_graph_sort_rows', 0, B.ptr(dist), n, B.ptr(order), B.ptr(ws), nbytes, B.stream_of(dist))
    rows = torch.tensor([0, 1, n // 2, 46339 - 1, 46339, (TWO31 // 4) // n, (TWO31 // 4) // n + 1], device='cuda')
    ref = torch.sort(dist[rows], dim=1, stable=True).indices.int()
    assert torch.equal(order[rows], ref)
    # one node more: refused by both calls (buffers sized for what the arguments describe); the Python caller turns the zero
    # workspace size into an error
    assert lib.raw('mm_graph_sort_rows_ws_bytes')(0, n + 1) == 0
    del order, dist
    dist1 = torch.zeros((n + 1) * (n + 1), device='cuda')
    order1 = torch.empty((n + 1) * (n + 1), dtype=torch.int32, device='cuda')
    assert lib.raw('mm_graph_sort_rows')(0, B.ptr(dist1), n + 1, B.ptr(order1), B.ptr(ws), nbytes,
                                         B.stream_of(dist1)) == MM_ERR_UNSUPPORTED
    del dist1, order1, ws
    torch.cuda.synchronize()
    regime(request, f'n={n}: n^2 = {n * n} < 2^31; n = {n + 1} refused')


if __name__ == '__main__':
    torch.cuda.init()
    if sys.argv[1] == 'case_c':
        _case_c_child(sys.argv[2])
    elif sys.argv[1] == 'case_f_ordered':
        _case_f_ordered_child()
