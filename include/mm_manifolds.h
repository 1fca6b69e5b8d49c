/* mm_manifolds.h — C ABI of libmm_manifolds.so (MI355X / gfx950).
 *
 * Drop-in boundary for graphembed's pairwise manifold-distance training path.
 * The reference has no FFI of its own: the interface these entry points
 * replace is the Python plugin class `Manifold`
 * (graphembed/graphembed/manifolds/base.py:7-81) and its callers
 * (optim/rsgd.py:40-82, modules.py:84-88).  Each entry point below cites the
 * reference method whose arithmetic it performs; INTEGRATION.md shows the
 * ctypes binding that plugs them back into that class.
 *
 * Rules of the ABI
 *   - plain C: pointers, sizes, scalars.  No torch / C++ types.
 *   - every `const void*` / `void*` data pointer is DEVICE memory (HBM),
 *     contiguous, row-major, batch-first; element type given by `dtype`.
 *   - the caller owns all buffers, including the workspace `ws`
 *     (size from the matching *_ws_bytes()); nothing is allocated inside.
 *   - kernels are enqueued on `stream` (a hipStream_t) and never synchronise;
 *     no call blocks the host.
 *   - return value: MM_OK, a negative MM_ERR_* for argument errors, or a
 *     positive hipError_t from the launch.  No exceptions cross the ABI.
 *   - pair order everywhere: k <-> (i,j), i<j, row-major upper triangle
 *     (torch.triu_indices(n,n,1); base.py:62, spd.py:179).
 *   - a row range [row_begin,row_end) selects the pairs (i,j) with
 *     row_begin <= i < row_end: a contiguous slice of the pair list starting at
 *     mm_pair_offset(n,row_begin).  This is the multi-GPU sharding unit.
 */
#ifndef MM_MANIFOLDS_H
#define MM_MANIFOLDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mm_stream_t; /* hipStream_t */

enum { MM_F32 = 0, MM_F64 = 1 };
enum { MM_OK = 0, MM_ERR_ARG = -1, MM_ERR_UNSUPPORTED = -2,
       MM_ERR_COMM = -3 /* RCCL missing or an RCCL call failed: text in mm_comm_last_error() */ };

/* vector-manifold kinds for mm_vec_* */
enum { MM_EUCLIDEAN = 0, MM_LORENTZ = 1, MM_SPHERE = 2 };

/* ---- library info -------------------------------------------------------- */
int mm_abi_version(void);
const char* mm_target_arch(void); /* "gfx950" */

/* ---- optional live kernel timing (HIP events on the launch stream) ---------- */
enum { MM_PROF_SPD_FWD = 0, MM_PROF_SPD_BWD = 1, MM_PROF_VEC_FWD = 2, MM_PROF_VEC_BWD = 3 };
/* When on, each pair-kernel launch is bracketed by hipEventRecord on its stream. */
int mm_prof_enable(int on);
/* Waits for the recorded events of kernel `id`; returns their count and summed
 * duration since the previous collect. */
int mm_prof_collect(int id, int64_t* launches, double* total_ms);
/* Shader clock at this moment of the stream: one wavefront runs `iters` dependent multiply-adds between two readings of
 * s_memtime (shader cycles) and s_memrealtime (the constant 100 MHz reference); out (device, 2 x uint64) receives the two
 * differences — clock [MHz] = 100 * out[0] / out[1].  Enqueued behind the kernels whose clock regime is to be read
 * (bench.py: behind a burst of replays of the timed step), so that an instruction budget can be priced in time. */
int mm_prof_clock_probe(void* out, int iters, mm_stream_t stream);

/* ---- pair-list geometry (host-side helpers, no GPU work) ----------------- */
/* number of pairs in rows < row:  row*(2n-row-1)/2 */
int64_t mm_pair_offset(int64_t n, int64_t row);
/* contiguous row range of shard `rank` of `world`, balanced by pair count */
int mm_shard_rows(int64_t n, int world, int rank, int64_t* row_begin, int64_t* row_end);

/* ---- SPD(d), affine-invariant metric ------------------------------------- */
/* Largest d the pairwise / per-node SPD kernels are instantiated for. */
int mm_spd_max_dim(void);

/* Workspace bytes for mm_spd_pdist_fwd/bwd on n points.  The workspace is the caller's and may hold anything when it is first
 * handed over (no memset is needed, ever): the per-node tables are written by the preparation, the accumulators are cleared by
 * it and by finalize, and the 64 KB behind them — where the backward's workgroups remember the start of their share of the
 * pair walk from one launch to the next (one 32-byte entry per workgroup: the walk's key and the start it leads to) — are
 * self-validating: an entry is used only if its whole key matches the launch, so stale or uninitialised contents cost a
 * recomputation, never a wrong result.  Keeping ONE workspace per embedding across steps (as the Python layer and bench.py
 * do) is what makes those entries hit; results do not depend on it.  One stream at a time may use a workspace. */
size_t mm_spd_pdist_ws_bytes(int dtype, int64_t n, int d);

/* flags for the pdist calls */
enum { MM_WS_PREPARED = 1 /* ws already holds the per-node factors of this x */ };

/* Fills ws with the per-node factors of x (Cholesky factor, its inverse, log det; the part of
 * _lult, manifolds/spd.py:108-111, that depends on one point only) and clears its accumulators and
 * status word; later pdist calls on the same x may then pass MM_WS_PREPARED. */
int mm_spd_prepare(int dtype, const void* x, int64_t n, int d, void* ws, mm_stream_t stream);

/* SymmetricPositiveDefinite.pdist — manifolds/spd.py:175-181 (+ _norm_log
 * 163-169, _lult 108-111).  out[k] = sum_m log^2 lambda_m(L_i^-1 X_j L_i^-T)
 * (sqrt of it if !squared), eigenvalues value-clamped to [wmin,wmax], result
 * value-clamped >= wmin.  d >= 3 (and the fused objectives of every d): windows narrower than
 * [1e-6, 1e6] return MM_ERR_UNSUPPORTED — the element-wise mm_spd_dist_fwd / _bwd take any window
 * (DESIGN.md section 6, item 11).
 *   x    [n,d,d]   out  [mm_pair_offset(n,row_end)-mm_pair_offset(n,row_begin)]
 * A non-positive-definite x[i] sets the status word (mm_spd_status).
 * n <= 2^22 in every SPD entry point (32-bit byte offsets into the node tables; 2^22 nodes are 8.8e12 pairs):
 * MM_ERR_ARG beyond, as for null pointers and row ranges outside [0, n]. */
int mm_spd_pdist_fwd(int dtype, const void* x, int64_t n, int d, int64_t row_begin,
                     int64_t row_end, int squared, double wmin, double wmax, void* out,
                     void* ws, int flags, mm_stream_t stream);

/* Backward of the above (what autograd computes in the reference; symmetric
 * part — SURVEY.md §8 a5).  g has the layout of `out`.  grad_x [n,d,d] is
 * OVERWRITTEN with this shard's partial gradient (full shape; sum the shards).
 * fp32 on ILL-CONDITIONED points: pairs whose matrix L_i^-1 X_j L_i^-T has lambda_max > 256 lambda_min are solved a second
 * time by a one-sided Jacobi on L_i^-1 L_j (d = 2..4) in EVERY form of the kernel — since round 6 also in the
 * two-columns-per-lane form of the SPD(4) backward that launches of >= 30 M pairs (n >= 7747) and row bands of >= 12 M pairs
 * take (there through an out-of-line call), so the gradient's accuracy does not depend on the launch size or on how a problem
 * is sharded: 8e-5 of its largest entry at cond(X) = 1e4, 1.5e-6 at 1e2 (measured, tools/illcond_probe.py; pinned by
 * tests/test_spd_gpu.py::test_ill_conditioned_points_fp32 in both forms).  MM_SPD4_BWD_TWO_COLS=0 / 1 in the environment
 * forces the one- / two-column form at every size (A/B builds only); fp64 needs no second solve. */
int mm_spd_pdist_bwd(int dtype, const void* x, const void* g, int64_t n, int d,
                     int64_t row_begin, int64_t row_end, int squared, double wmin,
                     double wmax, void* grad_x, void* ws, int flags, mm_stream_t stream);

/* Fused objective + gradients for a single-factor SPD embedding: ONE pass over the pairs
 * evaluates  m_k = softplus(*scale_raw) * d2_k  (ManifoldEmbedding.compute_dists,
 * modules.py:84-88), the loss against target[k] (objectives.py:16-45), and both gradients —
 * what `loss = objective_fn(gdists, compute_dists()); loss.backward()` computes in the reference
 * (train.py:213-217) without ever writing the pair vector of distances (4 B/pair of HBM traffic
 * instead of >= 40 B/pair through the framework's element-wise ops).
 *   loss_kind  MM_LOSS_STRESS    sum (m - target)^2                         objectives.py:39-45
 *              MM_LOSS_QUOTIENT  terms bit0: sum |m/(alpha target) - 1|
 *                                terms bit1: sum |alpha target/(m + eps) - 1|,  eps = 1/(epoch+1)
 *                                                                            objectives.py:16-36
 *   target     pair vector (layout of mm_spd_pdist_fwd's `out`) of squared graph distances
 *   scale_raw  device scalar (the raw scale parameter) or NULL for scale 1
 *   loss_params  NULL, or a device fp64 array {alpha, eps} that overrides the two by-value arguments
 *              (quotient loss): a captured graph of a step then follows eps = 1/(epoch+1) across epochs
 *              by updating that array, without being re-recorded.  Same argument in every *_loss entry.
 *   loss_out   device [2]: { loss of this shard, d loss / d scale_raw of this shard }
 *   grad_x     [n,d,d], OVERWRITTEN with this shard's partial d loss / d x. */
enum { MM_LOSS_NONE = 0, MM_LOSS_STRESS = 1, MM_LOSS_QUOTIENT = 2 };
int mm_spd_pdist_loss(int dtype, int loss_kind, const void* x, const void* target,
                      const void* scale_raw, int64_t n, int d, int64_t row_begin, int64_t row_end,
                      double alpha, double eps, int terms, const double* loss_params, double wmin, double wmax,
                      void* loss_out, void* grad_x, void* ws, int flags, mm_stream_t stream);

/* ---- SPD(d): the BIT-DETERMINISTIC mode of the two entries above (csrc/spd_det.hpp) ----------------
 * mm_spd_pdist_bwd and mm_spd_pdist_loss add their row sums, column sums and loss terms with float atomics: two runs on the
 * same inputs differ in the last bits.  The _det entries compute the same quantities without any atomic — a lane owns a COLUMN
 * node c and visits every r != c (both orders of a pair, so every logarithm is taken twice), its sums of one chunk of rows
 * leave with plain stores and a per-node kernel adds a node's chunk records in chunk order — and return the same bits for the
 * same (dtype, n, d, row range, inputs), on every call: eagerly or replayed from a graph, whatever det_ws held before.
 *
 * Geometry (host only, no GPU work): the n rows are cut into `chunks` chunks of `rows_per_chunk` rows,
 * (chunks - 1) rows_per_chunk < n <= chunks rows_per_chunk; both — and with them every order of summation — are a pure
 * function of (dtype, n, d): never of the row range, the device, an occupancy query or the environment.  chunks falls as n
 * grows (the grid is sized towards 1024 workgroups of 256 columns), so the scratch stays bounded:
 *   mm_spd_pdist_det_ws_bytes = chunks d^2 n sizeof(T)   the slab [chunks][d*d][n]
 *                             + 2 groups chunks sizeof(T) one {loss, dloss/dsoftplus} slot per workgroup, groups = ceil(n / 256)
 *   (each part rounded up to 64 bytes), and the slab is at most max(d^2 n sizeof(T), B) with B = 64 MiB.
 * mm_spd_pdist_det_geometry: MM_ERR_ARG for a dtype other than MM_F32 / MM_F64, n < 1, n > 2^22, d outside 2 ...
 * mm_spd_max_dim() or null outputs.
 *
 * mm_spd_pdist_bwd_det / mm_spd_pdist_loss_det take the arguments of mm_spd_pdist_bwd / mm_spd_pdist_loss plus `det_ws`
 * (mm_spd_pdist_det_ws_bytes(dtype, n, d) bytes) behind `ws`.  `ws` is the SAME workspace (mm_spd_pdist_ws_bytes): the same
 * preparation, MM_WS_PREPARED honoured, the status word set for non-PD points (mm_spd_status); its accumulators are not
 * touched and stay clean, so the same ws serves the atomic entries afterwards.  det_ws may hold anything on entry: every
 * record the per-node kernel reads is written by the same call.  Capture-safe, no allocation, no synchronisation.
 * Every d = 2 ... mm_spd_max_dim(), fp32 and fp64; squared and !squared; MM_LOSS_STRESS and MM_LOSS_QUOTIENT.
 * MM_ERR_ARG: null x / ws / det_ws / grad_x (/ loss_out), null g / target with a non-empty pair range, a row range outside
 * [0, n], n > 2^22; MM_ERR_UNSUPPORTED: eigenvalue windows narrower than [1e-6, 1e6] (d >= 3, and the fused objective of
 * every d), as for the atomic entries.  An empty row range: all-zero grad_x, zero loss record.
 * The loss record is summed per workgroup in a fixed order and over the workgroups' slots in fp64 (lane t of one wavefront
 * the slots t, t + 64, ... in index order, the 64 lane sums through a fixed butterfly).
 * Accuracy: the same gates and device functions per pair as the atomic kernel — the two modes agree to rounding. */
size_t mm_spd_pdist_det_ws_bytes(int dtype, int64_t n, int d);
int mm_spd_pdist_det_geometry(int dtype, int64_t n, int d, int64_t* chunks, int64_t* rows_per_chunk);
int mm_spd_pdist_bwd_det(int dtype, const void* x, const void* g, int64_t n, int d,
                         int64_t row_begin, int64_t row_end, int squared, double wmin,
                         double wmax, void* grad_x, void* ws, void* det_ws, int flags, mm_stream_t stream);
int mm_spd_pdist_loss_det(int dtype, int loss_kind, const void* x, const void* target,
                          const void* scale_raw, int64_t n, int d, int64_t row_begin, int64_t row_end,
                          double alpha, double eps, int terms, const double* loss_params, double wmin, double wmax,
                          void* loss_out, void* grad_x, void* ws, void* det_ws, int flags, mm_stream_t stream);

/* The same objective for a NODE MINIBATCH, with no gather or scatter launch around it (train.py:198-222 draws
 * idx = randperm(n)[a:b]; ManifoldEmbedding.compute_dists(idx) gathers x[idx], modules.py:86; GraphDataset.__getitem__
 * gathers dense[idx][:, idx], data/dataset.py:19-27; autograd's index backward scatters the gradient rows):
 *   x        the FULL table [n_total, d, d]; the `bs` points of the step are its rows idx[0..bs) (device int64, DISTINCT)
 *   dense    the dataset's dense n_total x n_total matrix of squared graph distances: target of pair (a, b) = dense[idx[a]][idx[b]]
 *   grad_x   [n_total, d, d], OVERWRITTEN: rows idx[.] with the gradient, every other row with zero — the dense
 *            gradient the reference's optimizers see
 *   ws       mm_spd_pdist_ws_bytes(dtype, n_total, d): the per-node tables are those of the FULL embedding (flags =
 *            MM_WS_PREPARED skips their preparation when they are current); row_begin / row_end shard the pair list of
 *            the BATCH (0 .. bs).  Every d of mm_spd_max_dim().
 *   idx      is caller data the kernels cannot validate: they read the low 32 bits of each index and CLAMP the node id into
 *            [0, n_total) — an out-of-range or negative index yields wrong numbers for that batch, never an access outside
 *            the buffers; repeated indices break the "each gradient row is written once" contract silently.  The Python
 *            layer checks host-side index tensors (graphembed.modules.distinct_in_range); device-side ones are the
 *            caller's responsibility.  The same holds for mm_vec_pdist_loss_subset, mm_product_pairs_loss_subset,
 *            mm_stereo_product_loss_subset, mm_pair_gather and mm_train_step.batch_idx. */
int mm_spd_pdist_loss_subset(int dtype, int loss_kind, const void* x, const void* dense, const void* scale_raw,
                             int64_t n_total, int d, const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end,
                             double alpha, double eps, int terms, const double* loss_params, double wmin, double wmax,
                             void* loss_out, void* grad_x, void* ws, int flags, mm_stream_t stream);

/* Stein divergence S(X,Y) = log det((X+Y)/2) - (log det X + log det Y)/2 — the second SPD "distance" of the
 * reference (SymmetricPositiveDefinite(use_stein_div=True): spd.py:183-194 stein_div / stein_pdiv,
 * 246-295 PairwiseSteinDivergence, linalg/torch_batch.py:173-197 PLogDet).  Value clamped >= wmin
 * (gradient-transparent), sqrt of it if !squared.  Layouts, workspace (mm_spd_pdist_ws_bytes), row ranges and
 * flags as mm_spd_pdist_fwd / mm_spd_pdist_bwd; mm_spd_stein_div is the element-wise form over m pairs
 * (out and/or both gradients may be requested; g is the upstream gradient of out). */
int mm_spd_stein_pdiv_fwd(int dtype, const void* x, int64_t n, int d, int64_t row_begin,
                          int64_t row_end, int squared, double wmin, void* out, void* ws, int flags,
                          mm_stream_t stream);
int mm_spd_stein_pdiv_bwd(int dtype, const void* x, const void* g, int64_t n, int d,
                          int64_t row_begin, int64_t row_end, int squared, double wmin,
                          void* grad_x, void* ws, int flags, mm_stream_t stream);
int mm_spd_stein_div(int dtype, const void* x, const void* y, const void* g, int64_t m, int d,
                     int squared, double wmin, void* out, void* grad_x, void* grad_y,
                     mm_stream_t stream);

/* Fused objective + gradients of a Stein-divergence embedding — the counterpart of mm_spd_pdist_loss (same loss kinds,
 * arguments and outputs; the comments there apply): with S = max(stein divergence of a pair, wmin) — the clamp is on the value
 * only, spd.py:188,193 — and m = softplus(*scale_raw) * S,
 *   loss_out = { sum of objective(target, m) over the pairs of rows [row_begin, row_end), d loss / d scale_raw },
 *   grad_x [n,d,d] OVERWRITTEN with this shard's partial gradient (symmetric; shards sum to the whole).
 * One pass over the pairs (csrc/spd_stein_loss.hpp): the Cholesky factor of (X_i + X_j)/2 and its inverse feed both points of
 * the pair, no pair vector is read or written besides `target`.  scale_raw may be NULL (scale 1, loss_out[1] = 0).  Any wmin is
 * honoured; there is no wmax (the divergence has no eigenvalue window).  ws: mm_spd_pdist_ws_bytes(dtype, n, d); flags /
 * MM_WS_PREPARED as mm_spd_stein_pdiv_bwd.  Every d = 2 ... mm_spd_max_dim(), fp32 and fp64.  MM_ERR_ARG: null x / ws / grad_x /
 * loss_out, a null target with a non-empty pair range, a bad row range, n > 2^22, a quotient loss with terms & 3 == 0;
 * MM_ERR_UNSUPPORTED: another loss kind, d out of range — all before anything is launched.  n == 0 zeroes loss_out; an empty
 * pair range gives a zero loss record and an all-zero grad_x.  Nothing allocates or synchronises: capture-safe. */
int mm_spd_stein_pdiv_loss(int dtype, int loss_kind, const void* x, const void* target, const void* scale_raw,
                           int64_t n, int d, int64_t row_begin, int64_t row_end, double alpha, double eps, int terms,
                           const double* loss_params, double wmin, void* loss_out, void* grad_x, void* ws, int flags,
                           mm_stream_t stream);
/* ... for a NODE MINIBATCH, the counterpart of mm_spd_pdist_loss_subset (the comment there applies, the paragraph on `idx`
 * included): x is the FULL table [n_total,d,d], the step's points are its rows idx[0 .. bs) (device int64, distinct; the kernel
 * reads the low 32 bits and clamps the node id into [0, n_total)), the target of batch pair (a, b), a < b, is
 * dense[idx[a]][idx[b]] — exactly that element of the contiguous n_total x n_total matrix, no symmetry assumed; row_begin /
 * row_end shard the pair list of the BATCH (0 <= row_begin <= row_end <= bs <= n_total).  grad_x [n_total,d,d] is OVERWRITTEN:
 * rows idx[.] with this shard's partial gradient, every other row with +0 — no gather, no scatter-add, no zero fill.
 * ws: mm_spd_pdist_ws_bytes(dtype, n_total, d).  bs < 2 or an empty row range: zero loss record, all-zero grad_x. */
int mm_spd_stein_pdiv_loss_subset(int dtype, int loss_kind, const void* x, const void* dense, const void* scale_raw,
                                  int64_t n_total, int d, const int64_t* idx, int64_t bs, int64_t row_begin,
                                  int64_t row_end, double alpha, double eps, int terms, const double* loss_params,
                                  double wmin, void* loss_out, void* grad_x, void* ws, int flags, mm_stream_t stream);
/* mm_spd_stein_pdiv_fwd / _bwd for a node minibatch of the full table (same addressing): `out` / `g` are the pair vector of
 * the BATCH's rows [row_begin, row_end) (bs (bs - 1) / 2 entries for the whole batch), grad_x [n_total,d,d] is OVERWRITTEN
 * (+0 outside the batch).  Repeated nodes are allowed HERE: gradients accumulate per node through atomics, and the pair of a
 * node with itself has S = 0 -> wmin and a gradient w (P - X^-1) / 2 that is zero to rounding (with squared = 0 that rounding is
 * amplified by 1 / (2 sqrt(wmin)), as in the reference's autograd). */
int mm_spd_stein_pdiv_fwd_subset(int dtype, const void* x, int64_t n_total, int d, const int64_t* idx, int64_t bs,
                                 int64_t row_begin, int64_t row_end, int squared, double wmin, void* out, void* ws,
                                 int flags, mm_stream_t stream);
int mm_spd_stein_pdiv_bwd_subset(int dtype, const void* x, const void* g, int64_t n_total, int d, const int64_t* idx,
                                 int64_t bs, int64_t row_begin, int64_t row_end, int squared, double wmin, void* grad_x,
                                 void* ws, int flags, mm_stream_t stream);

/* Counts the points whose Cholesky factorisation failed in the last prepare of `ws`
 * (n = the point count it was prepared for) into *host_status (0 = all succeeded).
 * Synchronises `stream` — the only blocking call of the ABI. */
int mm_spd_status(void* ws, int64_t n, int* host_status, mm_stream_t stream);

/* SymmetricPositiveDefinite.dist — spd.py:171-173, element-wise over m pairs
 * (x[k], y[k]).  x,y [m,d,d]; out [m]. */
int mm_spd_dist_fwd(int dtype, const void* x, const void* y, int64_t m, int d, int squared,
                    double wmin, double wmax, void* out, mm_stream_t stream);
int mm_spd_dist_bwd(int dtype, const void* x, const void* y, const void* g, int64_t m, int d,
                    int squared, double wmin, double wmax, void* grad_x, void* grad_y,
                    mm_stream_t stream);

/* Per-point maps used by RiemannianSGD (optim/rsgd.py:56-82); all [m,d,d]. */
enum {
  MM_SPD_EGRAD2RGRAD = 0, /* X sym(U) X                         spd.py:134-135 */
  MM_SPD_EXP = 1,         /* L expm(L^-1 U L^-T) L^T            spd.py:137-144 */
  MM_SPD_RETR = 2,        /* sym(X + U + 1/2 U X^-1 U)          spd.py:146-154 */
  MM_SPD_LOG = 3,         /* L logm(L^-1 Y L^-T) L^T  (U = Y)   spd.py:156-161 */
  MM_SPD_PROJX = 4,       /* V clamp(w) V^T of sym(X) (U unused) spd.py:126-132 */
  MM_SPD_PROJU = 5        /* sym(U)                             spd.py:119-124 */
};
int mm_spd_map(int dtype, int op, const void* x, const void* u, int64_t m, int d, double wmin,
               double wmax, void* out, mm_stream_t stream);
/* SymmetricPositiveDefinite.symeig — spd.py:35-41, 63-64 (linalg/fast.py:53-91 for n = 2, 3; LAPACK on the CPU
 * otherwise): eigenvalues of sym(x[k]), ascending.   x [m,d,d] -> w [m,d] */
int mm_spd_eigvalsh(int dtype, const void* x, int64_t m, int d, void* w, mm_stream_t stream);
/* graphembed/linalg/fast.py:25-159 by name — the closed forms for stacks of 2x2 / 3x3 matrices (spd.py:35-46 and
 * grassmann.py:29 pick them; monitor.py:39-45, tests/test_linalg.py:47-141 and tests/test_perf.py:14-81 call them directly),
 * with the derivative torch's autograd gives the reference's arithmetic (upper-triangle gradients, fast.py:5-10; the
 * `.data.clamp_` guards clamp the value and pass the derivative).  x [n,2,2] or [n,3,3]:
 *   op                      out              out2 (optional)     reference
 *   MM_FAST_SYMEIG2         w [n,2] asc.                         fast.py:53-70
 *   MM_FAST_SYMEIG3         w [n,3] asc.                         fast.py:75-91
 *   MM_FAST_CHOLESKY2       L [n,2,2]                            fast.py:94-107
 *   MM_FAST_INVCHOLESKY2    L^-1 [n,2,2]     L [n,2,2] or NULL   fast.py:110-135
 *   MM_FAST_SINGULAR2       s [n,2] desc.                        fast.py:138-159
 *   MM_FAST_DET2 / DET3 / SYMDET3   det [n]                      fast.py:25-50
 * mm_fast_bwd: grad_x [n,k,k] from the cotangents of out (and of out2, or NULL).  `eps` is the functions' `eps` argument. */
enum { MM_FAST_SYMEIG2 = 0, MM_FAST_SYMEIG3 = 1, MM_FAST_CHOLESKY2 = 2, MM_FAST_INVCHOLESKY2 = 3, MM_FAST_SINGULAR2 = 4,
       MM_FAST_DET2 = 5, MM_FAST_DET3 = 6, MM_FAST_SYMDET3 = 7 };
int mm_fast_fwd(int op, int dtype, const void* x, int64_t n, double eps, void* out, void* out2, mm_stream_t stream);
int mm_fast_bwd(int op, int dtype, const void* x, const void* grad_out, const void* grad_out2, int64_t n, double eps,
                void* grad_x, mm_stream_t stream);
/* SymmetricPositiveDefinite.norm — spd.py:113-117: ||L^-1 U L^-T||_F  -> out [m] */
int mm_spd_norm(int dtype, const void* x, const void* u, int64_t m, int d, int squared, void* out,
                mm_stream_t stream);
/* One fused RiemannianSGD update without momentum (rsgd.py:63-68, 82):
 *   r = X sym(G) X; r *= min(max_grad_norm/||r||_X, 1) (skipped if
 *   max_grad_norm <= 0); x_new = (exact ? exp : retr)(X, -lr r). */
int mm_spd_rsgd_step(int dtype, const void* x, const void* egrad, int64_t m, int d, double lr,
                     double max_grad_norm, int exact, void* x_new, mm_stream_t stream);

/* ---- vector manifolds: Euclidean R^m, Lorentz H^{m-1}, sphere S^{m-1} -------- */
/* `kind` is MM_EUCLIDEAN / MM_LORENTZ / MM_SPHERE; points are rows of x [n,m]. */
int mm_vec_max_dim(void);
/* (accumulators, loss slots, zero-padded points and — as for SPD — 64 KB of self-validating workgroup starts of the backward's walk) */
size_t mm_vec_pdist_ws_bytes(int dtype, int64_t n, int m);

/* Manifold.pdist default = gather + dist — manifolds/base.py:59-63 with
 *   Euclidean: max(sum (y-x)^2, 1e-8) [sqrt]                 base.py:29-33,56-57; euclidean.py:35-48
 *   Lorentz  : max(acosh(max(-<x,y>_L,1)),1e-8)^2            lorentz.py:72-77,101-138
 *   Sphere   : max(acos(clamp <x,y>),1e-8)^2                 sphere.py:68-74
 * out has the row-range layout described at the top. */
int mm_vec_pdist_fwd(int dtype, int kind, const void* x, int64_t n, int m, int64_t row_begin,
                     int64_t row_end, int squared, void* out, mm_stream_t stream);
/* Same, forward only, with the Gram matrix X J X^T formed on the matrix cores
 * (v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64) and the distance map fused
 * into the accumulator epilogue.  Lorentz and sphere (the reference evaluates
 * both from inner products); Euclidean uses the difference form above.  MM_ERR_UNSUPPORTED for n > 32768. */
int mm_vec_pdist_fwd_gram(int dtype, int kind, const void* x, int64_t n, int m, int64_t row_begin,
                          int64_t row_end, int squared, void* out, mm_stream_t stream);
/* Backward: grad_x [n,m] OVERWRITTEN with this shard's partial gradient.
 * (Sphere: the reference's 1/sqrt(1-c^2) is floored at 1e-8 instead of inf.)
 * n > 2^22 returns MM_ERR_UNSUPPORTED (the balanced symmetric form stops there, and the ordered fallback launches one row of
 * workgroups per 64 nodes of the whole problem whatever the row range); so does the ordered form (MM_VEC_BWD_ORDERED=1)
 * beyond the device's grid height. */
int mm_vec_pdist_bwd(int dtype, int kind, const void* x, const void* g, int64_t n, int m,
                     int64_t row_begin, int64_t row_end, int squared, void* grad_x, void* ws,
                     mm_stream_t stream);

/* Backward of mm_vec_pdist_fwd(_gram) on the matrix cores (fp32; Lorentz, sphere, and the SQUARED
 * Euclidean distance): W^T X with W = g * dout/dq(Gram) formed tile by tile in the MFMA accumulators
 * (csrc/vec_gram.hip; Euclidean: W = g, no Gram).  Same result as mm_vec_pdist_bwd; needs no
 * workspace.  MM_ERR_UNSUPPORTED for other dtypes / kinds / sizes (n > 32768, m > 32). */
int mm_vec_pdist_bwd_gram(int dtype, int kind, const void* x, const void* g, int64_t n, int m,
                          int64_t row_begin, int64_t row_end, int squared, void* grad_x,
                          mm_stream_t stream);

/* Fused objective + gradients for a single-factor vector-manifold embedding — the counterpart of
 * mm_spd_pdist_loss (same loss kinds, arguments and outputs; squared distances).  Where the symmetric pair kernel does
 * not cover (dtype, kind, m) — fp32 m > 32, fp64 m > 16 except Euclidean (m > 32) — the ordered fallback serves it, and
 * then n > 2^22 returns MM_ERR_UNSUPPORTED, as for mm_vec_pdist_bwd. */
int mm_vec_pdist_loss(int dtype, int kind, int loss_kind, const void* x, const void* target,
                      const void* scale_raw, int64_t n, int m, int64_t row_begin, int64_t row_end,
                      double alpha, double eps, int terms, const double* loss_params, void* loss_out, void* grad_x, void* ws,
                      mm_stream_t stream);
/* ... for a NODE MINIBATCH, the counterpart of mm_spd_pdist_loss_subset (same arguments: the FULL table x [n_total, m], the dense
 * target matrix, idx int64[bs] distinct, grad_x [n_total, m] OVERWRITTEN — zero rows outside the batch; ws as
 * mm_vec_pdist_ws_bytes(dtype, n_total, m)); every kind, every m <= mm_vec_max_dim(). */
int mm_vec_pdist_loss_subset(int dtype, int kind, int loss_kind, const void* x, const void* dense, const void* scale_raw,
                             int64_t n_total, int m, const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end,
                             double alpha, double eps, int terms, const double* loss_params, void* loss_out, void* grad_x,
                             void* ws, mm_stream_t stream);

/* ---- vector manifolds: the BIT-DETERMINISTIC mode of the three entries above (csrc/vec_det.hpp) ----
 * mm_vec_pdist_bwd, mm_vec_pdist_loss and mm_vec_pdist_loss_subset accumulate with float atomics in every one of their forms
 * (symmetric VALU, matrix cores, ordered pairs): two runs on the same inputs differ in the last bits.  The _det entries compute
 * the same quantities without any atomic — a lane owns a COLUMN node j and visits every i != j (both orders of a pair, the
 * per-pair arithmetic of the ordered atomic kernel), its sums of one chunk of rows leave with plain stores and a per-node
 * kernel adds a node's chunk records in chunk order — and return the same bits for the same (dtype, kind, n, m, row range,
 * inputs) on every call: eagerly or replayed from a graph, whatever det_ws held before, whatever MM_VEC_* / MM_GRAM_* say
 * (no environment switch selects or alters these kernels).
 *
 * Geometry (host only, no GPU work): the n rows are cut into `chunks` chunks of `rows_per_chunk` rows (a multiple of 8),
 * (chunks - 1) rows_per_chunk < n <= chunks rows_per_chunk; both — and with them every order of summation — are a pure
 * function of (dtype, kind, n, m): never of the row range, the device, an occupancy query or the environment.  The grid is
 * sized towards 1024 workgroups of 256 columns, so chunks falls as n grows and the scratch stays bounded:
 *   mm_vec_pdist_det_ws_bytes = chunks E n sizeof(T)       the slab [chunks][E][n], E = m (+ 1 for MM_EUCLIDEAN: the weights)
 *                             + 2 groups chunks sizeof(T)  one {loss, dloss/dsoftplus} slot per workgroup, groups = ceil(n / 256)
 *   (each part rounded up to 64 bytes), and the slab is at most max(E n sizeof(T), B) with B = 64 MiB.
 * mm_vec_pdist_det_geometry: MM_ERR_ARG for a dtype other than MM_F32 / MM_F64, an unknown kind, n < 1, n > 2^22, m outside
 * 1 ... mm_vec_max_dim() or null outputs.
 *
 * mm_vec_pdist_bwd_det / mm_vec_pdist_loss_det / mm_vec_pdist_loss_subset_det take the arguments of the atomic entries with
 * `ws` REPLACED by `det_ws` (mm_vec_pdist_det_ws_bytes(dtype, kind, n, m) bytes; the minibatch entry: of (dtype, kind, bs, m) —
 * the slab is addressed by batch position, with the geometry of a full batch of bs points).  det_ws may hold anything on
 * entry: every record the per-node kernel reads is written by the same call.  Capture-safe, no allocation, no
 * synchronisation.  Every kind, every m <= mm_vec_max_dim(), fp32 and fp64; squared and !squared; MM_LOSS_STRESS and
 * MM_LOSS_QUOTIENT.  The minibatch entry reads the target of batch pair (a, b), a < b by POSITION, at dense[idx[a]][idx[b]]
 * (no symmetry assumed), clamps node ids into the table, and OVERWRITES grad_x [n_total, m]: rows idx[.] (distinct) with the
 * gradient, every other row with +0.  On the gathered rows x[idx] with the targets dense[idx[a]][idx[b]] the full-batch entry
 * returns the same bits.
 * MM_ERR_ARG: null x / det_ws / grad_x (/ loss_out), null g / target / dense / idx with a non-empty pair range, a row range
 * outside [0, n], the quotient loss with terms & 3 == 0; MM_ERR_UNSUPPORTED: m > mm_vec_max_dim(), n (bs) > 2^22, another loss
 * kind.  All of them before anything touches the GPU.  An empty row range, or bs <= 1: all-zero grad_x, zero loss record.
 * The loss record is summed per workgroup in a fixed order and over the workgroups' slots in fp64 (lane t of one wavefront
 * the slots t, t + 64, ... in index order, the 64 lane sums through a fixed butterfly).  Offsets are 64-bit as in the ordered
 * atomic kernel (not exercised past 32 bits). */
size_t mm_vec_pdist_det_ws_bytes(int dtype, int kind, int64_t n, int m);
int mm_vec_pdist_det_geometry(int dtype, int kind, int64_t n, int m, int64_t* chunks, int64_t* rows_per_chunk);
int mm_vec_pdist_bwd_det(int dtype, int kind, const void* x, const void* g, int64_t n, int m,
                         int64_t row_begin, int64_t row_end, int squared, void* grad_x, void* det_ws,
                         mm_stream_t stream);
int mm_vec_pdist_loss_det(int dtype, int kind, int loss_kind, const void* x, const void* target,
                          const void* scale_raw, int64_t n, int m, int64_t row_begin, int64_t row_end,
                          double alpha, double eps, int terms, const double* loss_params, void* loss_out, void* grad_x,
                          void* det_ws, mm_stream_t stream);
int mm_vec_pdist_loss_subset_det(int dtype, int kind, int loss_kind, const void* x, const void* dense, const void* scale_raw,
                                 int64_t n_total, int m, const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end,
                                 double alpha, double eps, int terms, const double* loss_params, void* loss_out, void* grad_x,
                                 void* det_ws, mm_stream_t stream);

/* Element-wise dist over cnt pairs (x[k],y[k]).  out may be NULL (backward only);
 * grad_x/grad_y may both be NULL (forward only), else g [cnt] is required. */
int mm_vec_dist(int dtype, int kind, const void* x, const void* y, const void* g, int64_t cnt, int m,
                int squared, void* out, void* grad_x, void* grad_y, mm_stream_t stream);

/* Per-point maps (optim/rsgd.py:56-82 call sites); x,u,y,out are [cnt,m]. */
enum {
  MM_VEC_EGRAD2RGRAD = 0, /* lorentz.py:52-57, sphere.py:41-44, identity for Euclidean      */
  MM_VEC_PROJU = 1,       /* lorentz.py:39-42, sphere.py:41-44                              */
  MM_VEC_EXP = 2,         /* lorentz.py:59-62, sphere.py:51-56, x+u                         */
  MM_VEC_RETR = 3,        /* = exp for Lorentz/Euclidean (base.py:49-50); sphere.py:58-59   */
  MM_VEC_PROJX = 4,       /* lorentz.py:44-50, sphere.py:46-49 (u unused)                   */
  MM_VEC_TRANSP = 5,      /* u from x to y: lorentz.py:79-82; proju(y,u) (base.py:65-66)    */
  MM_VEC_LOG = 6          /* log_x(u): lorentz.py:64-70, sphere.py:61-66, u-x               */
};
int mm_vec_map(int dtype, int kind, int op, const void* x, const void* u, const void* y, int64_t cnt,
               int m, void* out, mm_stream_t stream);
/* Manifold.norm — base.py:29-33: sqrt(max(<u,u>, 1e-8)) with the manifold's inner product */
int mm_vec_norm(int dtype, int kind, const void* u, int64_t cnt, int m, int squared, void* out,
                mm_stream_t stream);
/* Fused momentum-free RiemannianSGD update (rsgd.py:63-68,82). */
int mm_vec_rsgd_step(int dtype, int kind, const void* x, const void* egrad, int64_t cnt, int m,
                     double lr, double max_grad_norm, int exact, void* x_new, mm_stream_t stream);
/* The same update for `count` (<= mm_vec_rsgd_multi_max()) parameters of one optimizer group in one
 * launch — the loop over group['params'] of rsgd.py:52-82 for parameters that share lr / max_grad_norm /
 * exact.  kinds, xs, egrads, cnts, ms, x_new are HOST arrays; x_new[t] may equal xs[t]. */
int mm_vec_rsgd_multi_max(void);
int mm_vec_rsgd_step_multi(int dtype, int count, const int* kinds, const void* const* xs,
                           const void* const* egrads, const int64_t* cnts, const int* ms, double lr,
                           double max_grad_norm, int exact, void* const* x_new, mm_stream_t stream);

/* The heavy-ball variant of the RSGD update (rsgd.py:70-80): momentum_buffer = momentum * momentum_buffer +
 * (1 - dampening) * rgrad (clipped), x_new = exp/retr(x, -lr * momentum_buffer), and the buffer is transported
 * to x_new — updated IN PLACE (SPD: identity transport, the buffer is kept symmetric).  x_new may equal x. */
int mm_vec_rsgd_momentum_step(int dtype, int kind, const void* x, const void* egrad, void* momentum_buffer,
                              int64_t cnt, int m, double lr, double momentum, double dampening,
                              double max_grad_norm, int exact, void* x_new, mm_stream_t stream);
int mm_spd_rsgd_momentum_step(int dtype, const void* x, const void* egrad, void* momentum_buffer, int64_t m,
                              int d, double lr, double momentum, double dampening, double max_grad_norm,
                              int exact, void* x_new, mm_stream_t stream);

/* One fused RiemannianAdam update (radam.py:62-98): Riemannian gradient, second moment from its norm
 * BEFORE clipping (one scalar per point, stored broadcast over the point as the reference does), clipping,
 * first moment, step size lr sqrt(1-beta2^t)/(1-beta1^t) (nc != 0: beta2 = 1 - 1/t), exp (exact) or
 * retr, transport of the first moment to the new point.  exp_avg / exp_avg_sq are updated in place;
 * x_new may equal x.  `step` is state['step'] as a DEVICE fp64 scalar (>= 1), advanced by the kernel;
 * `ticket` is a device uint32 that is zero between calls (the last block to finish advances `step`), so a
 * captured graph of a training step keeps counting when replayed. */
int mm_vec_radam_step(int dtype, int kind, const void* x, const void* egrad, void* exp_avg,
                      void* exp_avg_sq, double* step, unsigned* ticket, int64_t cnt, int m, double lr,
                      double beta1, double beta2, int nc, double eps, double max_grad_norm, int exact,
                      void* x_new, mm_stream_t stream);
/* ... for `count` (<= mm_vec_rsgd_multi_max()) vector-space parameters of one group in one launch; every
 * parameter has its own moments, step counter and ticket (HOST arrays of device pointers; cnts[t] >= 1). */
int mm_vec_radam_step_multi(int dtype, int count, const int* kinds, const void* const* xs,
                            const void* const* egrads, void* const* exp_avg, void* const* exp_avg_sq,
                            double* const* steps, unsigned* const* tickets, const int64_t* cnts,
                            const int* ms, double lr, double beta1, double beta2, int nc, double eps,
                            double max_grad_norm, int exact, void* const* x_new, mm_stream_t stream);
int mm_spd_radam_step(int dtype, const void* x, const void* egrad, void* exp_avg, void* exp_avg_sq,
                      double* step, unsigned* ticket, int64_t m, int d, double lr, double beta1,
                      double beta2, int nc, double eps, double max_grad_norm, int exact, void* x_new,
                      mm_stream_t stream);

/* ---- Grassmann Gr(N,p) / Stiefel St(N,p): points are [cnt,N,p], N <= 9, p <= 4 ---- */
enum { MM_GRASSMANN = 0, MM_STIEFEL = 1 };
enum {
  MM_MAT_PROJU = 0,    /* u - x x^T u (grassmann.py:49-53) / u - x sym(x^T u) (stiefel.py:40-45)   */
  MM_MAT_PROJX = 1,    /* Q of QR(x) (grassmann.py:55-61); Stiefel: sign-fixed (stiefel.py:47-57)  */
  MM_MAT_RETR_SVD = 2, /* polar factor U V^T of x+u (grassmann.py:76-80, stiefel.py:66-69); St(N, N), the
                          orthogonal group: followed by one Newton-Schulz step o (3 I - o^T o) / 2       */
  MM_MAT_RETR_QR = 3,  /* Q of QR(x+u) (grassmann.py:71-74); Stiefel sign-fixed (stiefel.py:62-63) */
  MM_MAT_EXP = 4,      /* x V cos(S) V^T + U sin(S) V^T, u = U S V^T (grassmann.py:63-69)          */
  MM_MAT_LOG = 5       /* log_x(u) (grassmann.py:82-89)                                            */
};
int mm_mat_max_rows(void);
int mm_mat_max_cols(void);
int mm_mat_map(int dtype, int kind, int op, const void* x, const void* u, int64_t cnt, int N, int p,
               void* out, mm_stream_t stream);
/* Grassmann.dist — grassmann.py:91-96: sum_k acos^2 sigma_k(x^T y) [sqrt]; element-wise over
 * cnt pairs; out / (grad_x,grad_y) optional as in mm_vec_dist.  (acos'(1), where the
 * reference yields NaN, is replaced by its finite limit.) */
int mm_grass_dist(int dtype, const void* x, const void* y, const void* g, int64_t cnt, int N, int p,
                  int squared, void* out, void* grad_x, void* grad_y, mm_stream_t stream);
/* Manifold.pdist default (base.py:59-63) with Grassmann.dist, row-range layout as above.  The backward OVERWRITES grad_x [n,N,p];
 * its ws: mm_grass_pdist_ws_bytes(dtype, n, N, p) bytes, may hold anything: cleared by the call. */
size_t mm_grass_pdist_ws_bytes(int dtype, int64_t n, int N, int p);
int mm_grass_pdist_fwd(int dtype, const void* x, int64_t n, int N, int p, int64_t row_begin,
                       int64_t row_end, int squared, void* out, mm_stream_t stream);
int mm_grass_pdist_bwd(int dtype, const void* x, const void* g, int64_t n, int N, int p,
                       int64_t row_begin, int64_t row_end, int squared, void* grad_x, void* ws,
                       mm_stream_t stream);
/* Fused objective + gradients for a single-factor Grassmann embedding — the counterpart of mm_vec_pdist_loss and
 * mm_spd_pdist_loss (same loss kinds, arguments and outputs; the header comments there apply): with d2 the squared
 * principal-angle distance of a pair (the p = 2 closed form and its eps clamps included) and m = softplus(*scale_raw) * d2,
 *   loss_out = { sum of objective(target, m) over the pairs of rows [row_begin, row_end), d loss / d scale_raw },
 *   grad_x [n,N,p] OVERWRITTEN with this shard's partial gradient (shards sum to the whole).
 * `target` is the slice of squared graph distances for those rows of the pair list.  One pass over the pairs: every
 * unordered pair is visited once, its p x p SVD runs once and feeds both of its points (csrc/grass_loss.hip) — no pair
 * vector is read or written besides `target`.  ws: mm_grass_pdist_loss_ws_bytes(dtype, n, N, p), cleared by the call itself.
 * Nothing is allocated and nothing synchronises: the call can be captured in a HIP graph.  An empty row range writes a zero
 * gradient and {0, 0}.  Limits as mm_grass_pdist_bwd (N <= 9, p <= 4, p <= N, n <= 2^30; MM_ERR_ARG / MM_ERR_UNSUPPORTED
 * before anything touches the GPU; a row range of more than 2^31 - 1 tiles of 16 rows x 64 columns is MM_ERR_UNSUPPORTED).
 * mm_grass_pdist_loss_form: how (dtype, N, p) walks the pairs — 1: every unordered pair once; 0: ordered pairs (for an
 * instantiation whose symmetric form would need scratch: none today); < 0: unsupported, with the codes above. */
size_t mm_grass_pdist_loss_ws_bytes(int dtype, int64_t n, int N, int p);
int mm_grass_pdist_loss_form(int dtype, int N, int p);
int mm_grass_pdist_loss(int dtype, int loss_kind, const void* x, const void* target, const void* scale_raw,
                        int64_t n, int N, int p, int64_t row_begin, int64_t row_end, double alpha, double eps,
                        int terms, const double* loss_params, void* loss_out, void* grad_x, void* ws,
                        mm_stream_t stream);
/* mm_grass_pdist_loss for a NODE MINIBATCH, the counterpart of mm_spd_pdist_loss_subset / mm_vec_pdist_loss_subset (the header
 * comment there applies word for word): x is the FULL table [n_total, N, p]; the points of the step are its rows idx[0..bs)
 * (device int64, DISTINCT; the kernel reads the low 32 bits and clamps the node id into [0, n_total)); the target of batch pair
 * (a, b), a < b, is dense[idx[a]][idx[b]] — exactly that element of the contiguous n_total x n_total matrix, no symmetry
 * assumed; row_begin / row_end shard the pair list of the BATCH (positions 0 .. bs); grad_x [n_total, N, p] is OVERWRITTEN:
 * rows idx[.] with this shard's partial gradient, every other row with +0; loss_out = { loss, d loss / d scale_raw }.
 * ws: mm_grass_pdist_loss_ws_bytes(dtype, n_total, N, p) — sized by the table, not by the batch, so one buffer serves every
 * batch of an epoch and a captured step; the call clears it itself.  A step is a memset, the pair kernel (the accumulators are
 * addressed by node) and the finalize launch over n_total; nothing allocates and nothing synchronises.  bs = 0, bs = 1 or an
 * empty row range writes a zero gradient and {0, 0} without a pair kernel.  Limits as mm_grass_pdist_loss (N <= 9, p <= 4,
 * p <= N, n_total <= 2^30, bs <= n_total, the tile count in one grid dimension), errors before anything touches the GPU.
 * mm_grass_pdist_loss_subset_form: 1 when (dtype, N, p) is built (every one is today); MM_ERR_UNSUPPORTED for an instantiation
 * left out because it would need scratch inside the row loop (the entry point then returns the same); MM_ERR_ARG as above. */
int mm_grass_pdist_loss_subset_form(int dtype, int N, int p);
int mm_grass_pdist_loss_subset(int dtype, int loss_kind, const void* x, const void* dense, const void* scale_raw,
                               int64_t n_total, int N, int p, const int64_t* idx, int64_t bs, int64_t row_begin,
                               int64_t row_end, double alpha, double eps, int terms, const double* loss_params,
                               void* loss_out, void* grad_x, void* ws, mm_stream_t stream);
/* Fused RiemannianSGD update of Grassmann / Stiefel points (rsgd.py:40-82), one launch: rgrad = proju(x, egrad), clipped by
 * max_grad_norm / sqrt(max(||rgrad||_F^2, 1e-8)) capped at 1 when max_grad_norm > 0, x_new = step(x, -lr * rgrad) with
 * step = retr_op (MM_MAT_RETR_SVD or MM_MAT_RETR_QR) or, with `exact`, MM_MAT_EXP (Grassmann only: Stiefel returns
 * MM_ERR_UNSUPPORTED, as mm_mat_map does).  The heavy-ball variant: momentum_buffer = momentum * momentum_buffer +
 * (1 - dampening) * rgrad, x_new = step(x, -lr * momentum_buffer), and the buffer is transported to x_new
 * (proju(x_new, .), base.py:65-66) IN PLACE.  x, egrad, momentum_buffer, x_new are [cnt,N,p]; x_new may equal x. */
int mm_mat_rsgd_step(int dtype, int kind, int retr_op, const void* x, const void* egrad, int64_t cnt, int N, int p,
                     double lr, double max_grad_norm, int exact, void* x_new, mm_stream_t stream);
int mm_mat_rsgd_momentum_step(int dtype, int kind, int retr_op, const void* x, const void* egrad,
                              void* momentum_buffer, int64_t cnt, int N, int p, double lr, double momentum,
                              double dampening, double max_grad_norm, int exact, void* x_new, mm_stream_t stream);
/* Fused RiemannianAdam update of Grassmann / Stiefel points (radam.py:62-98), one launch, one thread per point, in the
 * reference's order: rgrad = proju(x, egrad); gn^2 = max(||rgrad||_F^2, 1e-8), taken BEFORE the clip by min(max_grad_norm / gn,
 * 1) (max_grad_norm > 0); exp_avg = beta1 exp_avg + (1 - beta1) rgrad; exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) gn^2 — ONE
 * scalar per point, stored broadcast over it, as mm_spd_radam_step does; x_new = step(x, -alpha exp_avg / (sqrt(exp_avg_sq) +
 * eps)) with alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t), beta2 = 1 - 1/t when `nc`, and step = retr_op or, with `exact`,
 * MM_MAT_EXP (Grassmann only: Stiefel returns MM_ERR_UNSUPPORTED); exp_avg is then transported to x_new (proju(x_new, .),
 * base.py:65-66) IN PLACE.  `step` (device fp64 scalar t >= 1) is advanced by the kernel and `ticket` (device counter, zero
 * between launches) re-armed, as in mm_vec_radam_step: a captured graph keeps counting.  1 - beta is formed in fp64 from the
 * fp64 arguments.  Grassmann at N = p (a single point, no tangent directions): `exact` moves with retr_op, which keeps the frame
 * orthonormal where exp would carry normalised rounding noise into x_new^T x_new.  All tensors are [cnt,N,p]; x_new may equal x.  A point with a zero gradient and a zero first moment comes
 * out as itself (exp: bit for bit; the retractions: polar(x) / Q(x), x to rounding). */
int mm_mat_radam_step(int dtype, int kind, int retr_op, const void* x, const void* egrad, void* exp_avg, void* exp_avg_sq,
                      double* step, unsigned* ticket, int64_t cnt, int N, int p, double lr, double beta1, double beta2,
                      int nc, double eps, double max_grad_norm, int exact, void* x_new, mm_stream_t stream);

/* ---- special orthogonal group SO(N): points are [cnt,N,N], 2 <= N <= mm_so_max_dim() = 4 ---- */
/* The metric part of the reference's OrthogonalGroup / SpecialOrthogonalGroup (manifolds/orthogonal.py); proju, projx, the
 * retractions and the fused optimizer steps are those of St(N, N): mm_mat_map and mm_mat_*_step with MM_STIEFEL, p = N.
 * The distance (orthogonal.py:13-21: sum of the squared arguments of all eigenvalues of x^T y, = ||log(x^T y)||_F^2) is
 * computed as, and for inputs orthogonal only to rounding DEFINED as, the ambient function
 *   d2(x, y) = tr psi((y - x)^T (y - x) / 2) = sum_k 4 asin^2(sigma_k / 2),  sigma_k the singular values of y - x,
 * smooth wherever sigma_k < 2, with the gradient d d2 / dy = B diag(psi'_k) V^T = -d d2 / dx, (y - x) V = B from a one-sided
 * Jacobi, psi' = 2 theta / sin theta; proju(y, d d2 / dy) = -2 log_y(x).  At the cut locus (a rotation angle of pi: sigma = 2, or
 * a pair in different components of O(N)) sigma / 2 is clamped to 1 — d2 stays finite — and cos^2(theta / 2) is floored at
 * 1e-12, so the gradient, undefined there, comes out finite.  The reference's connected-component check (orthogonal.py:14-16)
 * would synchronise and is not made.
 * Every entry point validates its arguments before anything touches the GPU: MM_ERR_ARG for null pointers, bad counts or row
 * ranges and unknown dtypes / ops / loss kinds; MM_ERR_UNSUPPORTED for N outside 2 .. 4.  Nothing allocates, nothing
 * synchronises: the calls can be captured in a HIP graph. */
enum {
  MM_SO_LOG = 0, /* log_x(u), u a point: x skew(x^T D) V diag(theta_k / sin theta_k) V^T, D = u - x (orthogonal.py:26-37, where it
                    is a loop of scipy.linalg.logm on the CPU) */
  MM_SO_EXP = 1  /* exp_x(u) = x (V cos(S) V^T + B (sin(S) / S) V^T), skew(x^T u) V = B, S = diag ||b_k|| (the reference has none:
                    stiefel.py:59-60) */
};
int mm_so_max_dim(void);
int mm_so_map(int dtype, int op, const void* x, const void* u, int64_t cnt, int N, void* out, mm_stream_t stream);
/* OrthogonalGroup.dist — orthogonal.py:13-21 [sqrt unless squared]; element-wise over cnt pairs; out / (grad_x, grad_y) optional
 * as in mm_grass_dist (g: upstream gradient per pair, needed with the gradients).  The non-squared gradient of a pair at distance
 * 0 is 0. */
int mm_so_dist(int dtype, const void* x, const void* y, const void* g, int64_t cnt, int N, int squared, void* out,
               void* grad_x, void* grad_y, mm_stream_t stream);
/* Manifold.pdist default (base.py:59-63) with the distance above, pair order and row-range layout as for mm_grass_pdist_*.
 * The backward visits every unordered pair of the row range once (csrc/so.hip) and OVERWRITES grad_x [n,N,N] with this shard's
 * partial gradient; ws: mm_so_pdist_ws_bytes(dtype, n, N), cleared by the call.  n <= 2^30; a forward row range of 2^20 rows or
 * more is MM_ERR_UNSUPPORTED. */
size_t mm_so_pdist_ws_bytes(int dtype, int64_t n, int N);
int mm_so_pdist_fwd(int dtype, const void* x, int64_t n, int N, int64_t row_begin, int64_t row_end, int squared, void* out,
                    mm_stream_t stream);
int mm_so_pdist_bwd(int dtype, const void* x, const void* g, int64_t n, int N, int64_t row_begin, int64_t row_end,
                    int squared, void* grad_x, void* ws, mm_stream_t stream);
/* Fused objective + gradients of a single-factor SO(N) embedding: mm_grass_pdist_loss without `p` (its header comment applies:
 * loss kinds, target slice, loss_out = {loss, d loss / d scale_raw}, grad_x overwritten, empty ranges) on m =
 * softplus(*scale_raw) * d2 with the d2 above — what modules.py:84-88 and objectives.py:16-45 compute for the reference's `so`
 * factors (experiments/utils.py:3-40), which its own dist cannot differentiate.  ws: mm_so_pdist_loss_ws_bytes(dtype, n, N). */
size_t mm_so_pdist_loss_ws_bytes(int dtype, int64_t n, int N);
int mm_so_pdist_loss(int dtype, int loss_kind, const void* x, const void* target, const void* scale_raw, int64_t n, int N,
                     int64_t row_begin, int64_t row_end, double alpha, double eps, int terms, const double* loss_params,
                     void* loss_out, void* grad_x, void* ws, mm_stream_t stream);
/* The three pair-list entry points above for a NODE MINIBATCH, inside the pair kernels (csrc/so.hip, SUB): x is the FULL table
 * [n_total, N, N]; the points of the step are its rows idx[0..bs) (device int64; the kernels read the low 32 bits and clamp the
 * node id into [0, n_total)); the pairs are those of the BATCH POSITIONS 0 .. bs in this library's pair order, and row_begin /
 * row_end shard those positions.  No gather, no scatter-add, no zero fill.
 *   mm_so_pdist_fwd_subset   writes the batch's pair vector (the slice of the row range) to `out`.
 *   mm_so_pdist_bwd_subset   g: the upstream gradient of that slice, by batch pair position; grad_x [n_total, N, N] is
 *                            OVERWRITTEN: rows idx[.] with this shard's partial gradient, every other row with +0.
 *   mm_so_pdist_loss_subset  mm_grass_pdist_loss_subset without `p` (its header comment applies): the target of batch pair
 *                            (a, b), a < b, is dense[idx[a]][idx[b]] — exactly that element of the contiguous n_total x n_total
 *                            matrix, no symmetry assumed; grad_x as above; loss_out = { loss, d loss / d scale_raw }.
 * For the loss the nodes of a batch must be DISTINCT and bs <= n_total.  For the two pdist entry points REPEATED nodes are allowed
 * and correct, 0 <= bs <= 2^30: the accumulators are per node and summed with atomics, and a pair of a node with itself has
 * y - x = 0, hence d = 0 and a zero gradient in the squared and the non-squared form.
 * ws: mm_so_pdist_ws_bytes / mm_so_pdist_loss_ws_bytes (dtype, n_total, N) — sized by the table, not by the batch, so one buffer
 * serves every batch and a captured step; each call clears it itself.  A backward / loss call is a memset, the pair kernel (the
 * accumulators are addressed by node) and the finalize launch over n_total; nothing allocates and nothing synchronises.  bs = 0,
 * bs = 1 or a row range without pairs launches no pair kernel: the forward writes nothing, the backward a zero gradient, the loss
 * a zero gradient and {0, 0}.  Errors before anything touches the GPU: MM_ERR_ARG for null pointers (idx, dense, g, out only when
 * there are pairs), bad counts or row ranges, n_total > 2^30, unknown dtypes / loss kinds and MM_LOSS_NONE as a loss;
 * MM_ERR_UNSUPPORTED for N outside 2 .. 4, more tiles than one grid dimension holds and a forward row range of 2^20 rows or more. */
int mm_so_pdist_fwd_subset(int dtype, const void* x, int64_t n_total, int N, const int64_t* idx, int64_t bs,
                           int64_t row_begin, int64_t row_end, int squared, void* out, mm_stream_t stream);
int mm_so_pdist_bwd_subset(int dtype, const void* x, const void* g, int64_t n_total, int N, const int64_t* idx, int64_t bs,
                           int64_t row_begin, int64_t row_end, int squared, void* grad_x, void* ws, mm_stream_t stream);
int mm_so_pdist_loss_subset(int dtype, int loss_kind, const void* x, const void* dense, const void* scale_raw,
                            int64_t n_total, int N, const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end,
                            double alpha, double eps, int terms, const double* loss_params, void* loss_out,
                            void* grad_x, void* ws, mm_stream_t stream);

/* ---- stochastic-neighbour KL objective ---------------------------------------- */
/* The reference's KLDiveregenceLoss('sne', inclusive) (objectives.py:48-76, inference/stochastic_neighbors.py:8-24) on
 * pair vectors in this library's order (pair i < j at mm_pair_offset(n, i) + j - i - 1): with
 *   Z_i(theta) = sum_{j != i} exp theta_ij,  A(theta) = sum_i log Z_i,  P_ij(theta) = exp(theta_ij) / Z_i,
 *   loss = A(theta_z) - A(theta_x) - sum_{i<j} (P_ij + P_ji)(theta_x) (theta_z - theta_x)_ij  = sum_i KL(P_i(theta_x) || P_i(theta_z)),
 *   MM_SNE_INCLUSIVE: theta_x = -alpha * target, theta_z = -m;   MM_SNE_EXCLUSIVE: theta_x = -m, theta_z = -alpha * target.
 * target, m: [n (n - 1) / 2] squared graph / manifold distances.  loss_out[0] = loss (one value of `dtype`); grad_out, when
 * not null, is OVERWRITTEN with d loss / d m, one value per pair.  Three passes (csrc/sne_loss.hip): per-tile node
 * statistics with a per-node shift of the exponentials, a per-node merge, the gradient (skipped when grad_out is null);
 * no n x n array and no float atomics, so the results are bitwise reproducible from call to call.
 * ws: mm_sne_kl_ws_bytes(dtype, n) bytes (0 for an unknown dtype, n < 0 or n above the limit); it needs no clearing.
 * Nothing is allocated and nothing synchronises: the call can be captured in a HIP graph.
 * MM_ERR_ARG for an unknown dtype or mode, n < 0, a null loss_out and, for n >= 2, a null target, m or ws — before anything
 * touches the GPU.  n < 2: loss_out[0] = 0, nothing else is read or written.  n > 32768 returns MM_ERR_UNSUPPORTED (pair
 * offsets stay below 2^31 elements up to there, and the fp64 workspace is 0.8 GB at the limit). */
enum { MM_SNE_INCLUSIVE = 0, MM_SNE_EXCLUSIVE = 1 };
size_t mm_sne_kl_ws_bytes(int dtype, int64_t n);
int mm_sne_kl_loss(int dtype, int mode, const void* target, const void* m, int64_t n, double alpha,
                   void* grad_out /* may be null */, void* loss_out, void* ws, mm_stream_t stream);

/* ---- spanning-tree KL objective ------------------------------------------------ */
/* The reference's KLDiveregenceLoss('sste', inclusive) (objectives.py:48-76, inference/stochastic_trees.py) on pair vectors
 * in this library's order: with w = exp theta, L(theta) the weighted graph Laplacian without the row and column of node 0,
 * G = L^-1 (zero row and column for node 0) and q(S)_ij = S_ii + S_jj - 2 S_ij,
 *   A(theta) = log det L(theta),  mu(theta)_ij = w_ij q(G)_ij,  delta = theta_z - theta_x,
 *   loss = A(theta_z) - A(theta_x) - mu(theta_x) . delta  = KL(trees(theta_x) || trees(theta_z)),
 *   MM_SST_INCLUSIVE: theta_x = -alpha * target, theta_z = -m;   d loss / d m = mu(theta_x) - mu(theta_z)
 *   MM_SST_EXCLUSIVE: theta_x = -m, theta_z = -alpha * target;   d loss / d m_ij = mu_ij delta_ij - w_ij q(G M G)_ij, M the
 *                     reduced Laplacian of the weights w delta, all at theta_x (the gradient of the loss above)
 *   MM_SST_EXCLUSIVE_REFERENCE: the same loss;                   d loss / d m_ij = mu_ij delta_ij — what the reference
 *                     returns: its PLogDet.backward forms L^-1 outside the graph, so d G / d theta is dropped.
 * target, m: [n (n - 1) / 2] squared graph / manifold distances.  loss_out[0] = loss (one value of `dtype`); grad_out, when
 * not null, is OVERWRITTEN with d loss / d m, one value per pair.  Passes (csrc/sst_loss.hip): both models are shifted by
 * their largest theta (the loss and the first two gradients do not change when a constant is added to every m), the two
 * (n - 1) x (n - 1) Laplacians are factored by a blocked Cholesky in `dtype` with log det accumulated in fp64, the inverse
 * is formed only for a model whose marginals are needed (theta_x always, theta_z for the inclusive gradient), products run on
 * the matrix cores (exact f32 / f64).  No float atomics and every sum in a fixed order: bitwise reproducible from call to call.
 * A pivot that is not finite and positive (a disconnected graph, m = +inf on every pair of a node) gives a non-finite loss
 * and gradient; the call still returns MM_OK and the next call on the same workspace is unaffected.
 * ws: mm_sst_kl_ws_bytes(dtype, n) bytes = 5 (n - 1)^2 elements (each matrix rounded up to 256 bytes) + 2 x 256 elements +
 * 8 (2 ceil((n - 1) / 32) + n - 1) bytes, every part rounded up to 256 (0 for an unknown dtype, n < 2 or n above the limit);
 * it needs no clearing.  Nothing is allocated and nothing synchronises: the call can be captured in a HIP graph.
 * MM_ERR_ARG for an unknown dtype or mode, n < 0, a null loss_out and, for n >= 2, a null target, m or ws — before anything
 * touches the GPU.  n < 2: loss_out[0] = 0, nothing else is read or written.  n > 4096 returns MM_ERR_UNSUPPORTED (the fp64
 * workspace is 0.67 GB at the limit). */
enum { MM_SST_INCLUSIVE = 0, MM_SST_EXCLUSIVE = 1, MM_SST_EXCLUSIVE_REFERENCE = 2 };
size_t mm_sst_kl_ws_bytes(int dtype, int64_t n);
int mm_sst_kl_loss(int dtype, int mode, const void* target, const void* m, int64_t n, double alpha,
                   void* grad_out /* may be null */, void* loss_out, void* ws, mm_stream_t stream);

/* ---- constant curvature: the kappa-stereographic model ------------------------ */
/* The reference's `Universal` manifold (manifolds/universal.py, manifolds/impl/math.py): the Poincare ball for c > 0, the
 * stereographic projection of the sphere for c < 0, curvature K = -c, with c a TRAINABLE parameter.  Points are rows of
 * x [n, m], 1 <= m <= 16.  The curvature is passed as (c_raw, c_mode, c_min): c_raw is ONE element of `dtype` in DEVICE
 * memory, and the kernels apply get_c (universal.py:27-31) themselves,
 *   MM_STEREO_C_FREE      c = sign(c_raw) c_min + c_raw                 (keep_sign_fixed = False)
 *   MM_STEREO_C_POSITIVE  c =   c_min + softplus(c_raw)                  (keep_sign_fixed, c_init > 0)
 *   MM_STEREO_C_NEGATIVE  c = -(c_min + softplus(c_raw))                 (keep_sign_fixed, c_init < 0)
 * so a captured graph follows the optimizer's updates of c_raw without re-capture and the host never reads c.
 * Curvature gradients are with respect to c_raw (chain rule applied in the kernel).
 *
 * Distance (csrc/stereo.hip has the derivation): with q = |x_i - x_j|^2, D = (1 - c|x_i|^2)(1 - c|x_j|^2) + c q, t = q / D,
 *   d = 2 sqrt(t) phi(c t),  phi(w) = artanh(sqrt w)/sqrt w (w > 0), atan(sqrt -w)/sqrt -w (w < 0), phi(0) = 1,
 * the value clamped at 1e-8 after squaring (universal.py:79-84; the clamp is transparent to the gradient), D at 1e-15
 * (impl/math.py:345).  phi is one analytic function: c = 0 EXACTLY gives the Euclidean limit d^2 = 4 q, where the
 * reference returns NaN.
 *
 * mm_stereo_pdist_fwd / _bwd: pair vector in the row-range layout described at the top.  grad_x [n, m] and grad_c [1] are
 * OVERWRITTEN with this shard's partial gradients; an empty row range leaves zeros; n < 2 writes nothing but a zero
 * grad_c.  Every unordered pair is visited once, nothing is accumulated with float atomics (results are bitwise
 * reproducible), the curvature gradient is summed in fp64.  ws: mm_stereo_pdist_ws_bytes(dtype, n, m) bytes (0 for
 * arguments the library refuses); it needs no clearing.  It holds one record of m + 1 values per node and tile row /
 * tile column: 4 (m + 1) n (ceil(n / 64) * 2) bytes in fp32, 8 (m + 1) n (ceil(n / 32) + ceil(n / 64)) in fp64 — 23 MB
 * at n = 4039, m = 10 in fp32, 2.3 GB (fp32) / 6.8 GB (fp64) at the node limit with m = 16 — plus 8 bytes per tile.
 * mm_stereo_dist: element-wise over cnt pairs (x[k], y[k]); out may be NULL (backward only); grad_x / grad_y / grad_c
 * all NULL (forward only) or all given, then g [cnt] and ws of 8 * ((cnt + 127) / 128 + 1) bytes are required.
 * MM_ERR_ARG for null pointers, bad row ranges, m < 1, an unknown dtype, c_mode or op, c_min < 0 — before anything
 * touches the GPU; MM_ERR_UNSUPPORTED for m > 16 and n > 32768 (pair offsets stay below 2^31 elements up to there).
 * Nothing is allocated and nothing synchronises: every call can be captured in a HIP graph. */
enum { MM_STEREO_C_FREE = 0, MM_STEREO_C_POSITIVE = 1, MM_STEREO_C_NEGATIVE = 2 };
size_t mm_stereo_pdist_ws_bytes(int dtype, int64_t n, int m);
int mm_stereo_pdist_fwd(int dtype, const void* x, int64_t n, int m, int64_t row_begin, int64_t row_end, int squared,
                        const void* c_raw, int c_mode, double c_min, void* out, mm_stream_t stream);
int mm_stereo_pdist_bwd(int dtype, const void* x, const void* g, int64_t n, int m, int64_t row_begin, int64_t row_end,
                        int squared, const void* c_raw, int c_mode, double c_min, void* grad_x, void* grad_c, void* ws,
                        mm_stream_t stream);
int mm_stereo_dist(int dtype, const void* x, const void* y, const void* g, int64_t cnt, int m, int squared,
                   const void* c_raw, int c_mode, double c_min, void* out, void* grad_x, void* grad_y, void* grad_c,
                   void* ws, mm_stream_t stream);
/* Per-point maps; x, u, y, out are [cnt, m]. */
enum {
  MM_STEREO_EGRAD2RGRAD = 0,   /* u / lambda_x^2                         impl/math.py:1452-1453              */
  MM_STEREO_PROJU = 1,         /* u                                      universal.py:54-55                  */
  MM_STEREO_EXP = 2,           /* project(exp_x(u))                      universal.py:66-71, math.py:720-727 */
  MM_STEREO_EXP_NOPROJECT = 3, /* exp_x(u)                               (project=False)                     */
  MM_STEREO_RETR = 4,          /* project(x + u)                         universal.py:73-74                  */
  MM_STEREO_PROJX = 5,         /* c > 0 only, BALL_EPS 4e-3 / 1e-5       impl/math.py:142-156 (u unused)     */
  MM_STEREO_LOG = 6,           /* log_x(y)                               impl/math.py:835-841 (u unused)     */
  MM_STEREO_TRANSP = 7         /* u from x to y, gyration form           impl/math.py:1282-1298, 1359-1362   */
};
int mm_stereo_map(int dtype, int op, const void* x, const void* u, const void* y, int64_t cnt, int m, const void* c_raw,
                  int c_mode, double c_min, void* out, mm_stream_t stream);
/* Fused momentum-free RiemannianSGD update (rsgd.py:63-68, 82): r = egrad / lambda_x^2; r *= min(max_grad_norm / ||r||, 1)
 * (skipped if max_grad_norm <= 0) with the norm the reference's class computes — Universal.norm calls math.norm without c,
 * so ITS conformal factor is taken at c = 1 (universal.py:48-52) —; x_new = exact ? project(exp_x(-lr r)) :
 * project(x - lr r).  x_new may equal x. */
int mm_stereo_rsgd_step(int dtype, const void* x, const void* egrad, int64_t cnt, int m, const void* c_raw, int c_mode,
                        double c_min, double lr, double max_grad_norm, int exact, void* x_new, mm_stream_t stream);
/* Fused RiemannianAdam update (optim/radam.py:62-98 of the reference on Universal) in one launch, one thread per point:
 *   r = egrad / lambda_c(x)^2;  nrm = lambda_1(x) |r|  (Universal.norm: the conformal factor at c = 1, clamped at 1e-15, as in
 *   mm_stereo_rsgd_step);  exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) nrm^2  (ONE scalar per point, the norm BEFORE clipping,
 *   stored broadcast over the point's m entries);  r *= min(max_grad_norm / nrm, 1) if max_grad_norm > 0 (a zero gradient stays
 *   zero);  exp_avg = beta1 exp_avg + (1 - beta1) r;  u = -alpha exp_avg / (sqrt(exp_avg_sq) + eps) with
 *   alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t) and, if nc, beta2 = 1 - 1 / t (AdamNc);
 *   x_new = exact ? project(exp_x(u)) : project(x + u);  exp_avg = transp(x -> x_new, exp_avg), MM_STEREO_TRANSP's arithmetic.
 * 1 - beta1 and 1 - beta2 are formed in fp64 from the fp64 arguments and then rounded to `dtype`, as the reference forms them.
 * exp_avg / exp_avg_sq [cnt, m] are updated IN PLACE; x_new may equal x.  `step` (device fp64 scalar t >= 1, state['step'])
 * is read by every workgroup and advanced by the last one through `ticket` (device counter, zero between launches), as
 * mm_vec_radam_step does: a captured graph keeps counting.  Argument errors as mm_stereo_rsgd_step; step and ticket must
 * not be NULL. */
int mm_stereo_radam_step(int dtype, const void* x, const void* egrad, void* exp_avg, void* exp_avg_sq, double* step,
                         unsigned* ticket, int64_t cnt, int m, const void* c_raw, int c_mode, double c_min, double lr,
                         double beta1, double beta2, int nc, double eps, double max_grad_norm, int exact, void* x_new,
                         mm_stream_t stream);
/* products/embedding.py:37-46 in one launch: x / max(|x| / r_max, 1), then projx.  x_new may equal x. */
int mm_stereo_stabilize(int dtype, const void* x, int64_t cnt, int m, const void* c_raw, int c_mode, double c_min,
                        double r_max, void* x_new, mm_stream_t stream);
/* Products of nf constant-curvature factors (products/embedding.py:8-60 of the reference): m = sum_k max(d_k^2, 1e-8), the
 * factors' squared distances summed in factor order WITHOUT scales, every factor with its own (c_raw, c_mode, c_min).  The
 * factor list `f` is HOST memory, read at call time and passed to the kernels by value; x, c_raw, grad_x, grad_c are
 * device memory.
 * mm_stereo_product_pdist_fwd: the summed pair vector of the rows [row_begin, row_end) in ONE launch (grad_x / grad_c of
 * the factors are not touched and may be NULL).
 * mm_stereo_product_loss: one pass over every unordered pair and all factors that evaluates the objective on m and writes
 * grad_x [n, m_k] and grad_c [1] of EVERY factor (both OVERWRITTEN with this shard's partial gradients, with respect to
 * c_raw) and loss_out [1].  loss_kind MM_LOSS_STRESS / MM_LOSS_QUOTIENT: target, alpha, eps, terms and loss_params
 * {alpha, eps} (device, may be NULL) as for mm_grass_pdist_loss, without a scale.  MM_LOSS_NONE: `target` is the upstream
 * gradient d L / d m per pair (the backward of the forward above), nothing is written to loss_out (may be NULL).
 * Three launches whatever nf is: the pair kernel, one finalize over (node, factor), one fixed-order fp64 reduction of the
 * loss and curvature partials.  No float atomics: results are bitwise reproducible; shards of the row range sum to the whole.
 * An empty row range, a range without pairs or n < 2 writes zero gradients, zero grad_c and a zero loss.
 * ws: mm_stereo_product_ws_bytes(dtype, n, nf, m) bytes (0 for arguments the library refuses): the factors' slabs, each as
 * mm_stereo_pdist_ws_bytes describes, plus (nf + 1) fp64 partials per tile; it needs no clearing.
 * 1 <= nf <= 8 (more: MM_ERR_UNSUPPORTED), 1 <= m <= 16 and n <= 32768 as above; MM_ERR_ARG (null pointers, bad row ranges,
 * nf < 1, m < 1, an unknown dtype, loss_kind or c_mode, c_min < 0) is reported first, both before anything touches the
 * GPU.  Nothing is allocated and nothing synchronises: every call can be captured in a HIP graph, and a captured step
 * follows the optimizer's updates of every c_raw. */
typedef struct mm_stereo_factor {
  const void* x;     /* [n, m] */
  const void* c_raw; /* one element of `dtype`, device memory */
  void* grad_x;      /* [n, m], OVERWRITTEN (may be NULL for the forward) */
  void* grad_c;      /* [1],    OVERWRITTEN (may be NULL for the forward) */
  double c_min;
  int32_t m, c_mode;
} mm_stereo_factor;
size_t mm_stereo_product_ws_bytes(int dtype, int64_t n, int nf, const int32_t* m);
int mm_stereo_product_pdist_fwd(int dtype, const mm_stereo_factor* f, int nf, int64_t n, int64_t row_begin,
                                int64_t row_end, void* out, mm_stream_t stream);
int mm_stereo_product_loss(int dtype, int loss_kind, const mm_stereo_factor* f, int nf, const void* target, int64_t n,
                           int64_t row_begin, int64_t row_end, double alpha, double eps, int terms,
                           const double* loss_params, void* loss_out /* [1]; may be NULL for MM_LOSS_NONE */, void* ws,
                           mm_stream_t stream);
/* mm_stereo_product_loss for a NODE MINIBATCH, the counterpart of mm_spd_pdist_loss_subset: f[k].x is the FULL table
 * [n_total, m_k], the step's bs points are its rows idx[0 .. bs) (device int64, distinct, any order; see the paragraph on `idx`
 * at mm_spd_pdist_loss_subset), the target of batch pair (a, b), a < b, is dense[idx[a]][idx[b]] (dense: contiguous
 * [n_total, n_total] of `dtype`), row_begin / row_end shard the pair list of the BATCH (0 <= row_begin <= row_end <= bs).
 * f[k].grad_x [n_total, m_k] is OVERWRITTEN: rows idx[.] with this shard's partial gradient, every other row with exact zeros;
 * f[k].grad_c [1] and loss_out [1] as above.  MM_LOSS_STRESS and MM_LOSS_QUOTIENT only (an upstream gradient per pair has no
 * dense form: MM_LOSS_NONE is MM_ERR_ARG).  The pair tiles run over batch positions with the arithmetic, the tile shape and the
 * summation order of mm_stereo_product_loss: the result is BITWISE that of mm_stereo_product_loss on the gathered tables
 * x_k[idx] with the condensed targets of the same pairs.  Four launches whatever nf is: one that clears the gradient tables,
 * the pair kernel, the finalize over (batch position, factor), the reduction.
 * ws: mm_stereo_product_ws_bytes(dtype, bs, nf, m) - the BATCH's size; it needs no clearing.
 * Limits and error order as above with n = bs (nf <= 8, m <= 16, bs <= 32768); bs > n_total, bs < 0, a null idx or dense are
 * MM_ERR_ARG, n_total >= 2^31 is MM_ERR_UNSUPPORTED.  bs < 2 or a range without pairs writes zero gradients, zero grad_c and a
 * zero loss.  No float atomics, nothing allocated, no synchronisation: capturable, and the contents of idx may change between
 * replays. */
int mm_stereo_product_loss_subset(int dtype, int loss_kind, const mm_stereo_factor* f, int nf, const void* dense,
                                  int64_t n_total, const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end,
                                  double alpha, double eps, int terms, const double* loss_params, void* loss_out, void* ws,
                                  mm_stream_t stream);

/* ---- product embeddings ---------------------------------------------------- */
/* Objective of a product embedding in one pass over the pair vectors (the element-wise part of
 * train.py:213-217 for several factors): with d2[k] the squared pair distances of factor k,
 *   m = sum_k softplus(*scale_raw[k]) * d2[k]      (modules.py:84-88)
 *   loss = objective(target, m)                    (objectives.py:16-45; kinds as mm_spd_pdist_loss)
 * writes g_out[k] = dloss/dm * softplus(scale_k) (the upstream gradient of factor k's pdist backward)
 * and loss_out = { loss, dloss/dscale_raw[0], ..., dloss/dscale_raw[nf-1] }.
 * d2, scale_raw, g_out are HOST arrays of nf device pointers (nf <= mm_product_max_factors()). */
int mm_product_max_factors(void);
size_t mm_product_loss_ws_bytes(int dtype, int nf);
int mm_product_loss(int dtype, int loss_kind, int nf, const void* const* d2, const void* target,
                    const void* const* scale_raw, int64_t npairs, double alpha, double eps, int terms, const double* loss_params,
                    void* const* g_out, void* loss_out, void* ws, mm_stream_t stream);

/* The same objective in ONE pair kernel over all factors (the csphd configuration: Lorentz x sphere x
 * SPD(2) — one launch computes every factor's squared distance, the weighted sum, the loss term and all
 * gradients; ManifoldEmbedding.compute_dists modules.py:84-88 + objectives.py:16-45 + their backward).
 *   kinds[k]   MM_EUCLIDEAN / MM_LORENTZ / MM_SPHERE (xs[k] = [n, dims[k]], dims[k] <= 16) or
 *              MM_FACTOR_SPD (xs[k] = [n, d, d] with d = dims[k] in {2, 3}; the Cholesky factors are
 *              formed inside the pair kernel — no workspace, no preparation launch)
 *   grads[k]   Euclidean gradient of the loss w.r.t. xs[k] (same shape), rows [row_begin,row_end) of the
 *              pair list only — summed over shards it is the full gradient
 *   loss_out   { loss, dloss/dscale_raw[0..nf-1] }
 *   ws         mm_product_pairs_ws_bytes; every successful call leaves its accumulators zero, so a
 *              workspace that is reused for the same (dtype, factor list, n) may be passed with
 *              flags = MM_WS_CLEAN from the second call on (saves the clearing launches); | MM_WS_PREPARED only when the
 *              workspace's node table (symmetric pair kernel, large n) holds the CURRENT points — mm_train_step_run leaves
 *              it so after a fused product step; a caller that does not know passes neither and the table is rebuilt
 * At most 3 vector factors and one SPD factor; otherwise MM_ERR_UNSUPPORTED (use mm_product_loss around
 * the per-factor kernels).  kinds, dims, xs, scale_raw, grads are HOST arrays. */
enum { MM_FACTOR_SPD = 16 };
enum { MM_WS_CLEAN = 2 /* flag: the workspace's accumulators are already zero */ };
size_t mm_product_pairs_ws_bytes(int dtype, int nf, const int* kinds, const int* dims, int64_t n);
int mm_product_pairs_loss(int dtype, int loss_kind, int nf, const int* kinds, const int* dims,
                          const void* const* xs, const void* const* scale_raw, const void* target,
                          int64_t n, int64_t row_begin, int64_t row_end, double alpha, double eps,
                          int terms, const double* loss_params, double wmin, double wmax, void* const* grads, void* loss_out,
                          void* ws, int flags, mm_stream_t stream);

/* The same for a node minibatch (train.py:198-222, batch_size = 512 in the paper grid) without any gather or
 * scatter launch around it: the `bs` points of the step are rows idx[0..bs) (device int64) of the factors'
 * FULL tables xs[k] = [n_total, ...]; the target of pair (a, b) is dense[idx[a]][idx[b]] (the dense
 * n_total x n_total matrix of GraphDataset, data/dataset.py:19-27); gradients are written to rows idx[.] of
 * the full-size grads[k] — the other rows are NOT touched: pass zero-filled buffers.  row_begin/row_end
 * shard the pair list of the batch; ws as mm_product_pairs_ws_bytes(..., n = bs). */
int mm_product_pairs_loss_subset(int dtype, int loss_kind, int nf, const int* kinds, const int* dims,
                                 const void* const* xs, const void* const* scale_raw, const void* dense,
                                 int64_t n_total, const int64_t* idx, int64_t bs, int64_t row_begin,
                                 int64_t row_end, double alpha, double eps, int terms, const double* loss_params, double wmin,
                                 double wmax, void* const* grads, void* loss_out, void* ws, int flags,
                                 mm_stream_t stream);

/* Targets of a node minibatch: out[pair (a,b), a<b] = dense[idx[a]][idx[b]] in pair-vector order
 * (GraphDataset.__getitem__, data/dataset.py:19-27).  dense [n,n]; idx int64[bs] (device); out [bs(bs-1)/2]. */
int mm_pair_gather(int dtype, const void* dense, int64_t n, const int64_t* idx, int64_t bs, void* out,
                   mm_stream_t stream);

/* ---- graph-reconstruction metric --------------------------------------------- */
/* Per-node average precision of the embedding's neighbour ranking — what
 * FastPrecision::MeanAveragePrecision (pyx/impl/precision.cpp) and py_mean_average_precision
 * (metrics.py:61-96) average into the MAP score.
 *   dist          [n,n] dense symmetric embedding distances (zeros on the diagonal)
 *   indptr/indices  CSR adjacency of the (unweighted) graph, int32, device memory
 *   rank_scratch  int[nnz] device scratch
 *   ap_out        [n]: AP(u) = 1/deg(u) sum_{v in N(u)} (#neighbours ranked <= v) / rank(v); 0 for a node of degree 0.
 * THE ORDER (the contract of this entry and of mm_graph_sort_rows): one total order on (distance, node) — numbers
 * ascending with -0.0 == +0.0, then every NaN of either sign and any payload, ties by node index.  It is the order of
 * numpy.argsort(kind='stable') and torch.sort(stable=True).  rank(v) is the position of v in that order of row u with u
 * itself removed (1 = closest), so the ranks of a row are distinct; on return rank_scratch[e] holds rank(indices[e]). */
int mm_graph_average_precision(int dtype, const void* dist, int64_t n, const int* indptr,
                               const int* indices, int* rank_scratch, void* ap_out,
                               mm_stream_t stream);

/* Layer-wise F1 scores of the embedding's ordering against the shortest-path trees of the graph —
 * FastPrecision::LayerMeanF1Scores / LayerMeanAverageF1Scores (pyx/impl/precision.cpp:300-429), unweighted
 * AND weighted graphs.  order [n,n] int32: row u = all nodes sorted by embedding distance to u (stable: ties by node id);
 * hops [n,n] int32: the LAYER of v in the shortest-path tree rooted at u = the dense rank of the graph distance d(u,v)
 * among the distinct distances from u (precision.cpp:150-166; for unweighted graphs that is the hop distance); indptr CSR row pointers (degrees, for the min/max filter);
 * num_layers = diameter + 1 (<= 2048).  ACCUMULATES into the device arrays m1, m2, counts (double[num_layers-1],
 * zeroed by the caller): per layer the sum of F1, of F1^2 and the number of terms (per_tree_average = 0), or
 * the same over per-tree layer means (per_tree_average = 1). */
int mm_graph_layer_f1(const int* order, const int* hops, int64_t n, const int* indptr, int min_degree,
                      int max_degree, int per_tree_average, int num_layers, double* m1, double* m2,
                      double* counts, mm_stream_t stream);

/* Row-wise stable argsort of the dense embedding-distance matrix: order[u][k] = the node with the k-th smallest
 * distance to u, ties in node order (SortNodeDists, pyx/impl/precision.cpp:107-121) — the input of mm_graph_layer_f1.
 * The order is the total order stated at mm_graph_average_precision: numbers ascending with -0.0 == +0.0, then every NaN
 * of either sign, ties by node index (the keys are copied into ws with every NaN made the one canonical NaN; dist is
 * only read).  dist [n,n] (device), order int32 [n,n], ws of mm_graph_sort_rows_ws_bytes bytes; n <= 46340: a larger n
 * makes mm_graph_sort_rows_ws_bytes return 0 and mm_graph_sort_rows MM_ERR_UNSUPPORTED, before anything is launched. */
size_t mm_graph_sort_rows_ws_bytes(int dtype, int64_t n);
int mm_graph_sort_rows(int dtype, const void* dist, int64_t n, int* order, void* ws, size_t ws_bytes,
                       mm_stream_t stream);

/* ---- all-pairs graph distances (csrc/graph_paths.hip) ----------------------------- */
/* What data/graph.py:15-87 (targets) and pyx/impl/precision.cpp:44-92 (the evaluator's shortest-path trees) compute before
 * the first step.  The graph is a CSR adjacency in device memory, int32: row v of indptr / indices lists the OUT-neighbours
 * of v (metrics.graph_csr); self-loops and repeated neighbours are allowed and change nothing, neighbour ids outside
 * [0, n) are skipped.  Everywhere dist [n,n] int32 holds dist[v][s] = d(v -> s), 0 on the diagonal and -1 where s cannot
 * be reached from v; n <= mm_graph_max_nodes() = 46340 (n * n < 2^31, as mm_graph_sort_rows).  The entries issue kernel
 * launches only — no allocation, no synchronisation, no memset node — and check their arguments before anything touches
 * the GPU (MM_ERR_ARG); n == 0 does nothing.
 *
 * mm_graph_hops: hop distances of an unweighted graph, directed or not, every source at once with one BIT per source:
 * R_L[v] = {s : d(v -> s) <= L} = R_{L-1}[v] u U_{u in N(v)} R_{L-1}[u], one launch per level.  The call issues the levels
 * level_begin + 1 ... level_begin + level_count.  level_begin == 0 first initialises ws and dist (identity bits; 0 on the
 * diagonal, -1 elsewhere): both may hold anything on entry.  level_begin == k > 0 continues from the state that the call
 * which issued level k left in ws and dist.  new_bits int32[level_count] (device) is cleared and written by the call:
 * new_bits[j] = 1 if level level_begin + j + 1 found a new pair (v, s), else 0 — the caller reads it whenever it likes and
 * decides when to stop; the hop diameter is the last level whose flag is 1.  Levels issued after the frontier has emptied
 * change nothing.  ws: mm_graph_hops_ws_bytes(n) bytes, 8-byte aligned — three bit matrices [n][ceil(n / 64)] of 64-bit
 * words (reached, and two frontiers used alternately); 0 for n outside [0, mm_graph_max_nodes()].
 * MM_ERR_ARG: n < 0 or n > mm_graph_max_nodes(), level_begin < 0, level_count < 1, level_begin + level_count >= 2^31, and
 * for n > 0 a null pointer, ws_bytes too small or ws not 8-byte aligned. */
int64_t mm_graph_max_nodes(void);
size_t mm_graph_hops_ws_bytes(int64_t n);
int mm_graph_hops(const int* indptr, const int* indices, int64_t n, int level_begin, int level_count, int* dist,
                  int* new_bits, void* ws, size_t ws_bytes, mm_stream_t stream);

/* Cost distances: costs int32[nnz] (device) holds the cost of edge indices[e]; of parallel edges the cheapest counts.
 * Blocked Floyd-Warshall over (min, +) in int32 on dist itself: 3 ceil(n / 64) + 3 launches (4 for n <= 64), a function of n alone, so the
 * call is asynchronous end to end.  dist may hold anything on entry.  PRECONDITION (not checked on the device; the Python
 * layer checks it on the host graph): costs are integers >= 0 and (n - 1) * max cost < 2^30 - 1, the in-kernel sentinel for
 * "no route" — every finite distance then stays below it and no sum of two entries overflows.
 * MM_ERR_ARG: n < 0 or n > mm_graph_max_nodes(), a null pointer with n > 0. */
int mm_graph_cost_paths(const int* indptr, const int* indices, const int* costs, int64_t n, int* dist, mm_stream_t stream);

/* The targets of GraphDataset (data/dataset.py:16-19) straight from dist: over the upper triangle (i < j, pair-vector order,
 * pair (i, j) at mm_pair_offset(n, i) + j - i - 1) the value T(d) * T(d) / (T(dmax) * T(dmax)), T = float (MM_F32) or double
 * (MM_F64), one correctly rounded multiply and one correctly rounded divide per element, written as the condensed vector
 * [n(n-1)/2] and / or the dense symmetric matrix [n,n] with zero diagonal (either may be NULL).  stats int64[2] (device,
 * 8-byte aligned, cleared by the call): the largest finite distance of the upper triangle — dmax, read by the scaling kernel
 * from device memory: no host round trip — and its number of -1 entries.  A -1 yields +inf in the outputs.
 * MM_ERR_ARG: an unknown dtype, n < 0 or n > mm_graph_max_nodes(), a null or misaligned stats, a null dist with n > 0. */
int mm_graph_targets(int dtype, const int* dist, int64_t n, int64_t* stats, void* condensed, void* dense,
                     mm_stream_t stream);

/* ---- the collective of the sharded path ----------------------------------------- */
/* One process per GPU; the embedding is replicated, the pair list is cut into row ranges (mm_shard_rows) and every
 * step ends with ONE all-reduce(sum) of {point gradients, loss, scale gradients} over a process-lifetime RCCL
 * communicator (xGMI).  Replaces the reference's only parallel call site, torch.nn.DataParallel around
 * BatchedObjective (graphembed/graphembed/train.py:107-109: broadcast + gather + reduce-add per step); SURVEY.md §8b
 * "allreduce_grad(buf)".  RCCL is bound at run time (dlopen; MM_RCCL_LIB overrides the search), so the library loads
 * without it; every entry below then returns MM_ERR_COMM.
 *   rendezvous: rank 0 calls mm_comm_unique_id and hands the MM_COMM_ID_BYTES token to the other ranks through any
 *               host channel (file, socket, MPI, a torch.distributed store); every rank then calls mm_comm_init with
 *               the same token — collective, blocks until all `world` ranks have arrived.  `device` = HIP device
 *               ordinal of this rank (made current).  world = 1 is valid (a one-rank communicator).
 *   mm_allreduce_sum: in place, buf [count] of `dtype` in device memory, enqueued on `stream`, never synchronises —
 *               capturable into a HIP graph together with the kernels around it (after one uncaptured call).
 *   mm_comm_last_error: text of this thread's last MM_ERR_COMM. */
typedef struct mm_comm* mm_comm_t;
enum { MM_COMM_ID_BYTES = 128 };
int mm_comm_available(void);          /* 1 if RCCL could be bound */
int mm_comm_rccl_version(void);       /* NCCL_VERSION_CODE of the bound RCCL, 0 if none */
int mm_comm_unique_id(void* id_out /* host, MM_COMM_ID_BYTES */);
int mm_comm_init(mm_comm_t* comm, int rank, int world, const void* unique_id, int device);
int mm_comm_rank(mm_comm_t comm);
int mm_comm_world(mm_comm_t comm);
int mm_allreduce_sum(mm_comm_t comm, int dtype, void* buf, int64_t count, mm_stream_t stream);
int mm_comm_destroy(mm_comm_t comm);
const char* mm_comm_last_error(void);

/* ---- one training step per call ------------------------------------------------ */
/* The body of the reference's training loop for one full batch (graphembed/graphembed/train.py:198-222:
 * objective(dataset[idx], embedding.compute_dists(idx)) -> backward -> optimizer.step() for the point and the
 * scale parameter groups), issued by ONE call: the fused objective kernel of the embedding (mm_spd_pdist_loss /
 * mm_vec_pdist_loss / mm_product_pairs_loss) followed by the fused optimizer kernels of every parameter
 * (mm_*_rsgd_step, mm_*_rsgd_momentum_step, mm_*_radam_step[_multi]).  Nothing is allocated, nothing synchronises;
 * a caller whose loop is not captured in a HIP graph pays one foreign-function call per step instead of ~15.
 * Parameters are updated IN PLACE; gradients are left in the `grad` buffers (the scales' gradients in
 * loss_out[1 + k]); loss_out[0] is the loss BEFORE the update, as the reference logs it.
 * A single SPD factor is issued as TWO launches: the pair kernel (loss + gradient sums) and one per-point kernel that
 * finishes the gradient, applies the optimizer rule, writes the new point and its tables for the next step, closes the
 * loss record and updates a momentum-free RSGD scale — instead of prepare + pair + finalize + point update + scale update.
 * So is a single vector factor where mm_vec_fused_step_supports says so (the per-point kernel there moves the pair kernel's
 * sums into the gradient, steps the points and writes their zero-padded copy for the next pair kernel).
 * Multi-GPU: with a row range and a communicator the same call issues objective (this rank's pairs) -> one
 * all-reduce -> optimizer, still without touching the host in between (capturable as one HIP graph). */
enum { MM_OPT_NONE = -1 /* frozen: read by the objective, never stepped (a scale during burn-in) */,
       MM_OPT_RSGD = 0, MM_OPT_RADAM = 1 };
typedef struct mm_step_param {
  int kind;              /* MM_EUCLIDEAN / MM_LORENTZ / MM_SPHERE, or MM_FACTOR_SPD; flat parameters: MM_EUCLIDEAN */
  int dim;               /* m of a vector point, d of an SPD(d) point, 1 for a scalar                              */
  int64_t count;         /* points                                                                                */
  void* x;               /* the parameter (device), updated in place                                              */
  void* grad;            /* its Euclidean gradient (device): written by the objective, read by the optimizer       */
  int optimizer;         /* MM_OPT_RSGD (optim/rsgd.py:10-82) or MM_OPT_RADAM (optim/radam.py:12-98)               */
  double lr, momentum, dampening, max_grad_norm /* <= 0: no clipping */, beta1, beta2, adam_eps;
  int nc, exact;
  void* state0;          /* RSGD: momentum buffer (NULL when momentum == 0); Adam: exp_avg                         */
  void* state1;          /* Adam: exp_avg_sq                                                                       */
  double* step;          /* Adam: state['step'], device fp64                                                       */
  unsigned* ticket;      /* Adam: device counter, zero between calls                                               */
} mm_step_param;
typedef struct mm_train_step {
  size_t struct_size;            /* sizeof(mm_train_step) of the CALLER's header (mm_abi_version() >= 4): the library reads
                                    exactly that many bytes and takes every later field as zero, so a caller compiled against an
                                    older header of this layout keeps working when fields are appended; a value that is not a
                                    plausible size of this struct (below the ABI-4 base, or a caller of ABI <= 3 whose first
                                    member was `dtype`) is MM_ERR_ARG, and a LONGER struct whose extra tail is not all zero —
                                    a feature this library does not have — MM_ERR_UNSUPPORTED.  `mm_train_step s = {0};
                                    s.struct_size = sizeof s;` */
  int dtype, loss_kind, terms;
  double alpha, eps;             /* quotient loss: target scale and 1 / (epoch + 1)                                */
  const double* loss_params;     /* optional device {alpha, eps} overriding the two values above                   */
  double wmin, wmax;             /* SPD eigenvalue clamps (spd.py:29-30)                                           */
  int64_t n;                     /* points per factor                                                              */
  int nf;                        /* factors of the product manifold, 1..4                                          */
  mm_step_param points[4];       /* one per factor                                                                 */
  mm_step_param scales[4];       /* the factors' raw scale parameters (kind MM_EUCLIDEAN, dim 1, count 1;
                                    .grad is ignored: the gradient is loss_out[1 + k])                             */
  const void* target;            /* squared graph distances, pair-vector order [n(n-1)/2]                          */
  void* loss_out;                /* [1 + nf]                                                                       */
  void* ws;                      /* workspace of the embedding's objective kernel (mm_*_ws_bytes)                  */
  int ws_flags;                  /* MM_WS_CLEAN when a product workspace is known to be clean; MM_WS_PREPARED when a
                                    single SPD factor's workspace holds the tables of the CURRENT points: a step with an
                                    optimizer on the SPD points writes the tables of the new points itself (the optimizer
                                    kernel does what mm_spd_prepare does), so from the second consecutive step on the
                                    caller passes MM_WS_PREPARED — unless it changed the points in between.  The same
                                    holds for a single vector factor that takes the two-launch form
                                    (mm_vec_fused_step_supports) and its padded copy of the points, and for a product
                                    embedding on one GPU (the node table of its symmetric pair kernel); ignored elsewhere.
                                    A node-minibatch step (batch_idx) of a VECTOR factor does not rewrite the padded copy:
                                    the next full-batch step must not pass MM_WS_PREPARED (an SPD factor's does rewrite its tables) */
  /* -- sharded step (mm_abi_version() >= 2); all zero = the whole pair list on one GPU ------------------------- */
  int64_t row_begin, row_end;    /* this rank's rows of the pair list (mm_shard_rows); row_end <= 0 means n.  `target`
                                    is then this rank's SLICE: the targets of the pairs from mm_pair_offset(n,row_begin) on */
  mm_comm_t comm;                /* NULL: no collective.  Else ONE mm_allreduce_sum of reduce_buf between the objective
                                    and the optimizer kernels, on the same stream: afterwards every rank holds the full
                                    gradients and loss and applies the identical update — replicas stay equal, no broadcast */
  void* reduce_buf;              /* [reduce_count] of `dtype`: ONE allocation that contains every points[k].grad and
                                    loss_out (MM_ERR_ARG otherwise) — the message of the collective                 */
  int64_t reduce_count;
  /* -- node minibatch (mm_abi_version() >= 3); NULL / 0 = full batch -------------------------------------------------
     train.py:198-222 with batch_size set: the step's pair list is that of the `batch` nodes batch_idx[.] (device int64,
     distinct); `target` is then the DENSE n x n matrix of squared graph distances (GraphDataset.pdists), row_begin /
     row_end shard the batch's pair list, and the optimizer still steps all n points — those outside the batch with a
     zero gradient (the reference's dense x.grad; momentum and Adam state keep moving them).  Single SPD(d) or vector
     factor; MM_ERR_UNSUPPORTED for products (mm_product_pairs_loss_subset + the optimizer entry points serve those). */
  const int64_t* batch_idx;
  int64_t batch;
} mm_train_step;
int mm_train_step_run(const mm_train_step* step, mm_stream_t stream);
/* Largest d for which a single SPD(d) factor takes the two-launch form above (and therefore leaves the workspace holding
 * the tables of the new points: MM_WS_PREPARED on the next call); wider matrices are stepped by separate launches. */
int mm_spd_fused_step_max_dim(void);
/* 1 if a single vector factor (kind, dimension m) takes the two-launch form: the sizes at which the symmetric VALU pair
 * kernel is the fused objective (every Euclidean size it is built for; Lorentz / sphere up to m = 16). */
int mm_vec_fused_step_supports(int dtype, int kind, int m);

#ifdef __cplusplus
}
#endif
#endif /* MM_MANIFOLDS_H */
