/* include/pogs_amd.h -- C ABI of the MI355X-native POGS graph-form ADMM engine.
 *
 *   minimize  sum_i f_i(y_i) + sum_j g_j(x_j)   subject to  y = A x
 *   f_i(v) = c_i h_i(a_i v - b_i) + d_i v + e_i v^2 / 2      (same for g_j)
 *
 * Part 1 is the drop-in boundary: the four graph-form entry points of the
 * reference's C interface, with identical names, argument order, argument
 * meaning, enum values and return codes, so that the reference's own
 * python/pogs/graph.py (ctypes) or a C caller can be pointed at libpogs_amd.so
 * instead of libpogs_cpu.so.  Every pointer in part 1 is a HOST pointer owned
 * by the caller; the library copies what it needs and writes exactly n, m, m
 * elements to x, y, l (reference: src/interface_c/pogs_c.cpp:19-52).
 *
 * Part 2 is an additive extension for what the one-shot ABI cannot express on
 * a GPU: a persistent handle (equilibration + factorisation reused across
 * solves; the reference offers this only through its C++ API,
 * src/cpu/pogs.cpp:113-114), device-resident inputs, row-sharded multi-GPU
 * solves over RCCL, iteration stepping for benchmarks, and statistics.
 *
 * All functions are extern "C", take plain pointers and sizes, and never throw.
 */
#ifndef POGS_AMD_H_
#define POGS_AMD_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * Part 1 -- drop-in graph-form ABI
 * ------------------------------------------------------------------------- */

/* replaces: src/interface_c/pogs_c.h:51 */
enum ORD { COL_MAJ, ROW_MAJ };

/* replaces: src/interface_c/pogs_c.h:54-69 (order pinned by
 * tests/test_c_interface.cpp:149-154: ABS == 0, SQUARE == 14, ZERO == 15) */
enum FUNCTION { ABS, EXP, HUBER, IDENTITY, INDBOX01, INDEQ0, INDGE0, INDLE0,
                LOGISTIC, MAXNEG0, MAXPOS0, NEGENTR, NEGLOG, RECIPR, SQUARE, ZERO };

/* Return codes: the reference's PogsStatus (src/include/pogs.h:31-37).
 * NB 3 (not 1) means "max_iter reached"; *final_iter is the 0-based index of
 * the last iteration executed (src/cpu/pogs.cpp:391-393). */
enum POGS_STATUS { POGS_SUCCESS = 0, POGS_INFEASIBLE = 1, POGS_UNBOUNDED = 2,
                   POGS_MAX_ITER = 3, POGS_NAN_FOUND = 4, POGS_INVALID_CONE = 5,
                   POGS_ERROR = 6 };

/* replaces: src/interface_c/pogs_c.h:75-82 (PogsD).  Dense A, direct projector
 * (src/interface_c/pogs_c.cpp:19-20). */
int PogsD(enum ORD ord, size_t m, size_t n, const double *A,
          const double *f_a, const double *f_b, const double *f_c,
          const double *f_d, const double *f_e, const enum FUNCTION *f_h,
          const double *g_a, const double *g_b, const double *g_c,
          const double *g_d, const double *g_e, const enum FUNCTION *g_h,
          double rho, double abs_tol, double rel_tol, unsigned int max_iter,
          unsigned int verbose, int adaptive_rho, int gap_stop,
          double *x, double *y, double *l, double *optval, unsigned int *final_iter);

/* replaces: src/interface_c/pogs_c.h:84-91 (PogsS) */
int PogsS(enum ORD ord, size_t m, size_t n, const float *A,
          const float *f_a, const float *f_b, const float *f_c,
          const float *f_d, const float *f_e, const enum FUNCTION *f_h,
          const float *g_a, const float *g_b, const float *g_c,
          const float *g_d, const float *g_e, const enum FUNCTION *g_h,
          float rho, float abs_tol, float rel_tol, unsigned int max_iter,
          unsigned int verbose, int adaptive_rho, int gap_stop,
          float *x, float *y, float *l, float *optval, unsigned int *final_iter);

/* replaces: src/interface_c/pogs_c.h:99-108 (PogsSparseD).  ROW_MAJ = CSR with
 * ptr of length m+1, COL_MAJ = CSC with ptr of length n+1; int32 indices; CGLS
 * projector (src/interface_c/pogs_c.cpp:69-73). */
int PogsSparseD(enum ORD ord, size_t m, size_t n, size_t nnz,
                const double *data, const int *ptr, const int *ind,
                const double *f_a, const double *f_b, const double *f_c,
                const double *f_d, const double *f_e, const enum FUNCTION *f_h,
                const double *g_a, const double *g_b, const double *g_c,
                const double *g_d, const double *g_e, const enum FUNCTION *g_h,
                double rho, double abs_tol, double rel_tol, unsigned int max_iter,
                unsigned int verbose, int adaptive_rho, int gap_stop,
                double *x, double *y, double *l, double *optval,
                unsigned int *final_iter);

/* replaces: src/interface_c/pogs_c.h:110-119 (PogsSparseS) */
int PogsSparseS(enum ORD ord, size_t m, size_t n, size_t nnz,
                const float *data, const int *ptr, const int *ind,
                const float *f_a, const float *f_b, const float *f_c,
                const float *f_d, const float *f_e, const enum FUNCTION *f_h,
                const float *g_a, const float *g_b, const float *g_c,
                const float *g_d, const float *g_e, const enum FUNCTION *g_h,
                float rho, float abs_tol, float rel_tol, unsigned int max_iter,
                unsigned int verbose, int adaptive_rho, int gap_stop,
                float *x, float *y, float *l, float *optval,
                unsigned int *final_iter);

/* ---------------------------------------------------------------------------
 * Part 2 -- MI355X extension: persistent handle, device inputs, multi-GPU
 * ------------------------------------------------------------------------- */

typedef struct PogsAmdSolver PogsAmdSolver; /* opaque */

enum POGS_AMD_DTYPE { POGS_AMD_F32 = 0, POGS_AMD_F64 = 1 };
enum POGS_AMD_MEM { POGS_AMD_HOST = 0, POGS_AMD_DEVICE = 1 };
enum POGS_AMD_PROJECTOR { POGS_AMD_PROJ_DEFAULT = 0, /* dense: direct; sparse: CGLS by default, DIRECT for
                                                        min(m, n) <= POGS_AMD_SPARSE_DIRECT_MAX, one GPU */
                          POGS_AMD_PROJ_DIRECT = 1, POGS_AMD_PROJ_CGLS = 2,
                          POGS_AMD_PROJ_CGLS_FUSED = 3 /* dense, one GPU: CGLS with one pass over A per CG step and
                                                          one host poll per ADMM iteration (PogsAmdCreateDense) */ };
/* largest min(m, n) of a sparse handle with the direct projector (its factor is two dense K x K matrices) */
#define POGS_AMD_SPARSE_DIRECT_MAX 16384

#define POGS_AMD_UNIQUE_ID_BYTES 128

/* Row-sharding descriptor.  world == 1 (or a NULL pointer) means single GPU.
 * Every rank holds m_local consecutive rows of A and the matching slices of
 * f, y, l; x-sized data (g, x) is replicated.  The only collectives are sum
 * all-reduces of n-vectors / n*n Gram / a few scalars over RCCL. */
typedef struct PogsAmdDist {
  int rank;
  int world;
  size_t m_global;                              /* total rows over all ranks  */
  char unique_id[POGS_AMD_UNIQUE_ID_BYTES];     /* from PogsAmdDistUniqueId() */
} PogsAmdDist;

typedef struct PogsAmdOptions {
  int device;          /* HIP device ordinal; -1 = current device                   */
  int projector;       /* enum POGS_AMD_PROJECTOR                                   */
  int profile;         /* 1: bracket the dominant kernels with HIP events; k > 1:
                          every k-th such launch only (an event record costs the
                          stream a few microseconds of idle time)                   */
  int reserved[5];     /* reserved[POGS_AMD_OPT_STORAGE] (= reserved[0]): the `storage` option, enum
                          POGS_AMD_STORAGE, 0 = as dtype; reserved[1..4]: zero.  The array keeps
                          its declaration so that an initialiser written for it --
                          {dev, proj, prof, {0, 0, 0, 0, 0}} -- compiles and means what it meant
                          (in strict C99 a struct has no second name for an array's element);
                          zeroed options give the behaviour they always gave                 */
} PogsAmdOptions;
#define POGS_AMD_OPT_STORAGE 0
#define PogsAmdOptStorage(opt) ((opt)->reserved[POGS_AMD_OPT_STORAGE])   /* lvalue: PogsAmdOptStorage(&o) = POGS_AMD_STORE_F32 */
/* How a dense handle stores its matrix.  STORE_SAME: in the handle's dtype.  STORE_F32 (an fp64 handle): the
 * equilibrated matrix is rounded to float and the one-pass iteration reads the float copy (PogsAmdCreateDense). */
enum POGS_AMD_STORAGE { POGS_AMD_STORE_SAME = 0, POGS_AMD_STORE_F32 = 1 };

typedef struct PogsAmdStats {
  /* last solve / iterate call */
  double t_total_s, t_init_s, t_loop_s, t_h2d_s;
  unsigned int iterations;        /* executed (= final_iter + 1)                    */
  unsigned int exact_iters;       /* iterations that evaluated exact residuals      */
  unsigned int norm_est_iters;    /* power iterations used by the norm estimate     */
  unsigned int rho_updates;
  unsigned long long cg_iters;    /* total CGLS inner iterations                    */
  unsigned long long matvecs;     /* passes over A (dense) / SpMVs (sparse), loop   */
  unsigned long long matvecs_init;/* the same for the one-time setup                */
  double rho_final, nrmA;
  /* HIP-event timing of the dominant kernel (options.profile = 1), loop only */
  double stream_ms;               /* sum of durations of the A-streaming launches   */
  unsigned long long stream_launches;
  double stream_bytes;            /* algorithmic bytes those launches had to move   */
  /* one-time setup pieces, HIP-event timed */
  double equil_ms, normest_ms, gram_ms, chol_ms, trtri_ms;
  double gram_flops;
  double reserved[8];             /* [0] / [1]: one-pass iteration, rho predictions hit / missed;
                                     [2]: all-reduce calls issued by the handle so far;
                                     [3]: ranks of the handle's communicator as RCCL reports
                                          them (ncclCommCount; 0 without row shards);
                                     [4]: after PogsAmdSolveBatchFn, the sum over its problems
                                          of the iterations each one executed (`iterations` then
                                          counts batch iterations, `matvecs` multi-vector passes
                                          over A);
                                     [5] / [6] / [7]: with options.profile, the same batch's
                                          HIP-event time (ms), launch count and algorithmic bytes
                                          of its multi-vector passes over A;
                                     after PogsAmdSolveBatchSparseFn the same, with `matvecs`
                                          counting multi-vector products with A or A^T and
                                          `cg_iters` batched CG steps                             */
} PogsAmdStats;

/* Fill `out` (POGS_AMD_UNIQUE_ID_BYTES) with a fresh RCCL unique id (rank 0
 * calls this and ships the bytes to the other ranks by any means). */
int PogsAmdDistUniqueId(char *out);

/* Create a solver for a dense m x n matrix.  `A` is a host or device pointer
 * (mem), row- or column-major (ord), of type dtype.  The matrix is copied,
 * equilibrated (reference: src/cpu/matrix/matrix_dense.cpp:116-200), its norm
 * estimated (src/cpu/include/equil_helper.h:107-135) and the projector set up
 * (src/cpu/projector/projector_direct_dense.cpp:45-84,116-121).  With dist,
 * m is the LOCAL row count.
 * opt->projector: DEFAULT and DIRECT factor the Gram matrix.  CGLS (one GPU, any shape) builds no factor and runs the
 * reference's CGLS loop (projector_cgls.cpp:52-88): two passes over A and one host poll per CG step.
 * CGLS_FUSED (one GPU, any shape, both types, both orderings, host or device A) stores A and estimates the norm as
 * CGLS does, builds no factor, and runs the same arithmetic as a device-resident loop: q = A p and the column sums of
 * A^T q come from ONE pass over A, s = A^T r - x is kept by the recurrence s -= alpha (A^T q + p) inside a projection
 * (formed explicitly at its start), and the host polls once per ADMM iteration (csrc/dense_cg_fused.h).  y = A x comes
 * from the recurrence y_warm + sum alpha q, and from the product every POGS_AMD_YSYNC-th iteration (default 16).
 * stats: matvecs counts the launches that read A (per projection 1 + the CG steps; a row wider than one register
 * tile is read twice per step), cg_iters the CG steps.  Every sum has one fixed order: two runs give the same bytes.
 * With dist->world > 1 both CGLS values are refused.  On a handle of either CGLS value PogsAmdSolveBatchFn,
 * PogsAmdSolveBatchWarmFn and PogsAmdGetFactor return POGS_ERROR and the handle stays usable.  PogsAmdCreateSparse
 * refuses CGLS_FUSED before anything is built.
 * PogsAmdOptStorage(opt) = POGS_AMD_STORE_F32 (mixed storage; the option lives in opt->reserved[0]): an fp64 handle
 * over an fp32 copy of the matrix.  After the
 * equilibration the stored matrix is rounded, entry by entry and to nearest, to values representable in float -- call
 * it A^ -- and EVERYTHING in the handle is then defined on A^: the norm estimate, Gram matrix, factor, every product,
 * the residuals and the epilogue.  The handle solves, in fp64 arithmetic throughout, the graph-form problem of the
 * matrix D^-1 A^ E^-1, which differs from the caller's A by at most 2^-24 relative per entry; it is not an approximate
 * projector on the unrounded matrix (d, e are those of the equilibration as it ran; PogsAmdGetEquil returns A^).  Two
 * copies with equal values are kept: the fp64 one and a float one (rows of round_up(n, 4) floats, zero padding), so
 * the matrix takes 1.5 x the memory of a plain fp64 handle's.  The hot launches of the one-pass iteration (lasso-like
 * and logistic f: PogsAmdSolve, PogsAmdIterate) read the float copy, 4 bytes per entry instead of 8 (stats:
 * stream_bytes counts such a launch as m n 4); every other pass -- set-up, the two-pass iteration, the pass after a
 * missed rho prediction, the exact-residual pass of the lean form, PogsAmdMul, PogsAmdProject, the batch entries --
 * reads the fp64 copy with its existing kernel.  Both copies hold the same numbers, so only the order of some sums
 * differs.  POGS_AMD_MIXED_PASS=0 in the environment, read at create, keeps the rounding and both copies but runs
 * every pass on the fp64 copy (the A / B leg of a measurement).  (The multi-vector kernels that would let the batch
 * entries read the float copy exist and are tested on their own -- PogsAmdBatchRowsMixedCheck below -- but the batch
 * entries do not call them yet.)
 * Honoured for: dtype F64, m > n, projector DEFAULT or DIRECT, no dist, n <= 10240 (the row fits a one-pass shape of
 * the mixed plan: not windowed and no wider than the fp64 one-pass iteration reaches).  Refused before anything is
 * built -- POGS_ERROR, *out NULL, PogsAmdLastError names the reason: dtype F32, m <= n, either CGLS value, row shards,
 * a wider or windowed row, an unknown storage value.  PogsAmdCreateSparse refuses any non-zero storage (a sparse fp64
 * handle over float non-zeros: PogsAmdCreateSparseMixed). */
int PogsAmdCreateDense(PogsAmdSolver **out, int dtype, enum ORD ord, size_t m,
                       size_t n, const void *A, int mem,
                       const PogsAmdOptions *opt, const PogsAmdDist *dist);

/* Create a solver for a sparse matrix (CSR if ord == ROW_MAJ, else CSC);
 * data/ptr/ind are host or device pointers (mem).  With dist (may be NULL) the
 * matrix is this rank's block of m consecutive rows, given as CSR (SURVEY.md
 * section 8 f.3): CGLS with the A^T products and row sums all-reduced.
 * opt->projector: DEFAULT and CGLS run CGLS.  DIRECT (single GPU, min(m, n) <= POGS_AMD_SPARSE_DIRECT_MAX) forms
 * I + A_eq^T A_eq (m > n) or I + A_eq A_eq^T from the sparse copies after the equilibration, factors and inverts it
 * as a dense handle does and keeps W = L^-1 and U = W^T (2 K^2 elements, K = min(m, n)): every projection is then
 * two products with A / A^T and two triangular mat-vecs, exact, with no inner loop (stats: cg_iters stays 0, matvecs
 * counts 2 products per iteration and 2 more on an iteration with exact residuals; gram_ms, chol_ms, trtri_ms the
 * set-up).  DIRECT with a larger short side or with dist is refused before anything is built: POGS_ERROR, *out NULL,
 * PogsAmdLastError says why. */
int PogsAmdCreateSparse(PogsAmdSolver **out, int dtype, enum ORD ord, size_t m,
                        size_t n, size_t nnz, const void *data, const int *ptr,
                        const int *ind, int mem, const PogsAmdOptions *opt,
                        const PogsAmdDist *dist);

/* Create a MIXED-STORAGE solver for a sparse matrix: an fp64 handle over float non-zeros (one GPU).  The arguments are
 * those of PogsAmdCreateSparse with dtype POGS_AMD_F64 implied and no dist; opt->projector DEFAULT, CGLS or DIRECT as
 * there.  PogsAmdCreateSparse itself keeps refusing a non-zero storage: the capability lives in this entry.
 * The set-up runs as a plain fp64 handle's on the fp64 values -- structure, both CSR copies, both tiled copies,
 * Sinkhorn-Knopp, D A E, the division by the norm -- so d and e are the plain handle's bytes.  Then every value of BOTH
 * CSR copies is rounded to the nearest float and stored back as that double, val = (double)(float)val -- call the
 * matrix A^ -- and EVERYTHING after that is defined on A^: the norm estimate, the sparse Gram matrix and factor of a
 * DIRECT handle, every product, the residuals, the epilogue, PogsAmdGetEquil, PogsAmdMul, PogsAmdProject and the batch
 * entries.  The handle solves, in fp64 arithmetic throughout, the graph-form problem of the matrix D^-1 A^ E^-1, which
 * differs from the caller's A by at most 2^-24 relative per entry; it is not an approximate projector on the unrounded
 * matrix.  The VALUES of the tiled copies are then written as floats (the fp64 arrays are released first, so the peak
 * does not grow; local columns, row ids, tile table and plan are untouched) and every solo product -- the ADMM
 * iteration, both CGLS loops, the norm estimate, warm start, PogsAmdMul, PogsAmdProject, PogsAmdSparseCgCheck, the
 * direct projector's two products -- streams 4 instead of 8 bytes per value and widens it on use.  Both CSR copies hold
 * bitwise-equal values, a float converts to double exactly and the order of every sum is fixed by the tile plan, so a
 * product over the float values is BIT FOR BIT the fp64 product over A^.  The CSR copies stay fp64 with the rounded
 * values: the plain CSR kernel (a copy that did not get tiled, POGS_AMD_SPMV=plain), the batched sparse kernels and the
 * sparse Gram kernel read them, unchanged.  stats: stream_bytes counts a product on a float tiled copy with 4 instead
 * of 8 in its nnz (s + 4) term; the vectors stay 8.  The handle holds 4 bytes less per stored element on each tiled copy.
 * POGS_AMD_MIXED_PASS=0 in the environment, read at create, keeps the rounding but leaves the tiled values as doubles,
 * the existing kernel over A^ (the A / B leg of a measurement; same bytes out).
 * Refused before anything is built -- POGS_ERROR, *out NULL, PogsAmdLastError names the reason: a NULL argument (opt may
 * be NULL), an unknown ord or mem, bad dimensions, projector CGLS_FUSED, DIRECT with min(m, n) >
 * POGS_AMD_SPARSE_DIRECT_MAX, a storage field other than 0 or POGS_AMD_STORE_F32 (both mean float non-zeros here).
 * Every entry that takes a sparse handle works on the result. */
int PogsAmdCreateSparseMixed(PogsAmdSolver **out, enum ORD ord, size_t m, size_t n, size_t nnz,
                             const double *data, const int *ptr, const int *ind, int mem,
                             const PogsAmdOptions *opt);

/* Create a MIXED-STORAGE dense solver with the one-pass CGLS projector: an fp64 POGS_AMD_PROJ_CGLS_FUSED handle over a
 * float copy of the matrix (one GPU, no row shards, any m, tall or wide, 1 <= n <= 10240: the row fits a one-pass shape
 * of the mixed plan, not windowed).  The arguments are those of PogsAmdCreateDense with dtype POGS_AMD_F64 implied and
 * no dist.  opt is required: opt->projector must be POGS_AMD_PROJ_CGLS_FUSED and the storage field 0 or
 * POGS_AMD_STORE_F32 (both mean the float copy here).  PogsAmdCreateDense itself keeps refusing POGS_AMD_STORE_F32 with
 * either CGLS value and with m <= n: the capability lives in this entry.
 * The equilibrated matrix is rounded to float once, at the end of the equilibration and before the norm estimate, by
 * the code a POGS_AMD_STORE_F32 handle of PogsAmdCreateDense runs -- call it A^ -- and EVERYTHING after that is defined
 * on A^: the norm estimate, every product, the CG loop, the residuals, the epilogue, PogsAmdGetEquil, PogsAmdMul and
 * PogsAmdProject.  It is not an approximate projector on the unrounded matrix.  Both copies are kept (1.5 x the matrix).
 * The RECURRING launches of the projector read the float copy, 4 bytes per entry instead of 8: u = A^T r at the start
 * of every projection, the one pass of every CG step (q = A p with the column sums of A^T q), and the product y = A x
 * of every POGS_AMD_YSYNC-th projection.  Every other pass -- set-up, warm start, the exact-residual pass, PogsAmdMul,
 * the two set-up products of PogsAmdProject -- keeps its fp64 kernel on the fp64 copy; both hold the same numbers, so
 * only the order of some sums differs.  stats: matvecs and cg_iters count as on a plain CGLS_FUSED handle; with
 * profiling on, stream_bytes counts a launch over the float copy as m n 4.  POGS_AMD_MIXED_PASS=0 in the environment,
 * read at create, keeps the rounding and both copies and runs every pass on the fp64 copy (the A / B leg).
 * Refused before anything is built and with no device needed -- POGS_ERROR, *out NULL, PogsAmdLastError names the
 * reason: a NULL argument (out, A, opt), an unknown ord or mem, bad dimensions, any projector but CGLS_FUSED,
 * n > 10240 or a windowed row, a storage field other than 0 or POGS_AMD_STORE_F32.
 * Every entry that takes a dense CGLS_FUSED handle works on the result, PogsAmdDenseCgCheck included; the batch entries
 * and PogsAmdGetFactor refuse as on any CGLS handle. */
int PogsAmdCreateDenseMixed(PogsAmdSolver **out, enum ORD ord, size_t m, size_t n, const double *A, int mem,
                            const PogsAmdOptions *opt);

/* Cold-start solve (reference: PogsImplementation::Solve, src/cpu/pogs.cpp:91-581).
 * Coefficient and output pointers are HOST pointers of the solver's dtype
 * (f_*: m_local, g_*: n; x: n, y/l: m_local).  mu (length n) may be NULL. */
int PogsAmdSolve(PogsAmdSolver *s,
                 const void *f_a, const void *f_b, const void *f_c, const void *f_d,
                 const void *f_e, const int *f_h,
                 const void *g_a, const void *g_b, const void *g_c, const void *g_d,
                 const void *g_e, const int *g_h,
                 double rho, double abs_tol, double rel_tol, unsigned int max_iter,
                 unsigned int verbose, int adaptive_rho, int gap_stop,
                 void *x, void *y, void *l, void *mu, double *optval,
                 unsigned int *final_iter);

/* The same solve with BROADCAST coefficients: a field of f or g whose pointer is NULL holds one value (a0 .. e0, h0) for
 * every element and is filled on the device -- the caller neither builds nor converts nor uploads an array for it.  A
 * lasso's f is (h = SQUARE, a = 1, b = b_i, c = 1, d = 0, e = 0) and its g (h = ABS, a = 1, b = 0, c = lambda, d = e = 0):
 * one per-element array out of twelve (python/pogs/graph.py:428,431 builds m + n objects for them; at 2.5e6 elements
 * the twelve arrays are 60 MB of host work per solve).  Everything else as PogsAmdSolve / PogsAmdBeginRun. */
typedef struct PogsAmdFn {
  const void *a, *b, *c, *d, *e;   /* HOST arrays of the solver's dtype, or NULL */
  const int *h;                    /* HOST array of enum FUNCTION values, or NULL */
  double a0, b0, c0, d0, e0;       /* the value of a field whose pointer is NULL  */
  int h0;
} PogsAmdFn;
int PogsAmdSolveFn(PogsAmdSolver *s, const PogsAmdFn *f, const PogsAmdFn *g,
                   double rho, double abs_tol, double rel_tol, unsigned int max_iter,
                   unsigned int verbose, int adaptive_rho, int gap_stop,
                   void *x, void *y, void *l, void *mu, double *optval,
                   unsigned int *final_iter);
int PogsAmdBeginRunFn(PogsAmdSolver *s, const PogsAmdFn *f, const PogsAmdFn *g,
                      double rho, double abs_tol, double rel_tol, unsigned int max_iter,
                      int adaptive_rho, int gap_stop);

/* Batched solves: k problems (1 <= k <= POGS_AMD_BATCH_MAX) on the handle's matrix, every pass over A shared by all
 * of them.  f[j], g[j] as in PogsAmdSolveFn; rho: k values or NULL (1.0 each); tolerances, max_iter, adaptive_rho and
 * gap_stop are shared, every problem starts cold, and a problem that stops is frozen while the others go on.
 * Outputs are HOST arrays, problem j at offset j*n (x, mu) / j*m (y, l) / j (optval, final_iter, status);
 * y, l, mu, optval may be NULL.  Returns 0 when the batch ran (status[j] holds each PogsStatus),
 * POGS_ERROR when refused (PogsAmdLastError says why): k out of range, a sparse handle, m <= n, the CGLS projector,
 * row shards, or a NULL x, final_iter or status.  The handle's solo state (a pending warm start included) is kept.
 * Members that start from a given (x0, l0): PogsAmdSolveBatchWarmFn. */
#define POGS_AMD_BATCH_MAX 16
int PogsAmdSolveBatchFn(PogsAmdSolver *s, int k, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho,
                        double abs_tol, double rel_tol, unsigned int max_iter, unsigned int verbose,
                        int adaptive_rho, int gap_stop, void *x, void *y, void *l, void *mu,
                        double *optval, unsigned int *final_iter, int *status);

/* Batched solves on a sparse handle: as PogsAmdSolveBatchFn (same arguments, output layout, shared parameters and
 * per-problem rho), for a single-GPU sparse handle of any shape (m > n or m <= n), built from CSR or CSC, from host or
 * device memory.  Every product with A or A^T reads the equilibrated matrix once for all active problems.  The
 * projection is a batched CGLS: each problem runs its own CG (shift 1, at most 500 steps, its own tolerance,
 * warm-started from its previous x) and leaves the product's slot list when its CG stops.  A problem's outputs do not
 * depend on k, on its position or on the other problems.  On a handle with the direct projector the projection is
 * exact instead -- two shared products and the two triangular row passes over W and U, no inner loop and no host poll
 * inside it -- `cg_iters` is 0, and the same independence holds.  Stats: `iterations` batch iterations, `matvecs`
 * multi-vector products, `cg_iters` batched CG steps, reserved[4] problem-iterations, reserved[5..7] with
 * options.profile the products' HIP-event time (ms), launch count and algorithmic bytes.
 * Returns 0 when the batch ran (status[j] holds each PogsStatus), POGS_ERROR when refused (PogsAmdLastError says
 * why): k out of range, a dense handle, row shards, or a NULL x, final_iter or status; the handle stays usable.  The
 * handle's solo state (the last solo solve's stats but those above, its iterate, a pending warm start) is kept.
 * Here too every problem starts cold; members that start from a given (x0, l0): PogsAmdSolveBatchWarmFn. */
int PogsAmdSolveBatchSparseFn(PogsAmdSolver *s, int k, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho,
                              double abs_tol, double rel_tol, unsigned int max_iter, unsigned int verbose,
                              int adaptive_rho, int gap_stop, void *x, void *y, void *l, void *mu,
                              double *optval, unsigned int *final_iter, int *status);

/* Batched solves whose members may start warm, on either kind of handle: a dense handle runs the batch of
 * PogsAmdSolveBatchFn, a sparse one that of PogsAmdSolveBatchSparseFn (CGLS or direct projector).  Arguments, output
 * layout, stats and refusals are those of the two entries (a wide or CGLS dense handle, row shards, k out of range,
 * a NULL x, final_iter or status), and in addition:
 * x0 (k*n), l0 (k*m): HOST arrays of the handle's dtype, problem j at offset j*n / j*m.  Both NULL: every problem
 *    starts cold.  Both given: see `warm`.  One without the other is refused (src/cpu/pogs.cpp:159-179).
 * warm: NULL (every problem is warm when x0 is given), or k flags: problem j starts warm where warm[j] != 0 and cold
 *    elsewhere -- a cold problem's part of x0 / l0 is never read.  Flags together with a NULL x0 are refused.
 * A warm problem starts as a solo solve does after PogsAmdSetWarmStart (SetInitX + SetInitLambda,
 *    src/cpu/pogs.cpp:144-156) at its own rho[j]: x = x0 / e, y = A x, t = l0 / d, xt = (A^T t) (1 / rho[j]),
 *    yt = t (-1 / rho[j]).  The two products are shared by the warm problems and are counted in `matvecs`.  A cold
 *    problem returns the bytes the cold entries return for it, and a problem's outputs depend neither on k, nor on
 *    its position, nor on the other problems, nor on which of them are warm.  The sparse CGLS batch starts its first
 *    CG from that x.
 * rho_final: NULL, or k doubles: each problem's rho when it stopped -- with x and l, the start of a neighbouring
 *    problem (a warm start at rho = 1 loses most of what the warm start gains).
 * A refused call returns POGS_ERROR, writes nothing and leaves the handle usable; the solo state is kept. */
int PogsAmdSolveBatchWarmFn(PogsAmdSolver *s, int k, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho,
                            const void *x0, const void *l0, const int *warm,
                            double abs_tol, double rel_tol, unsigned int max_iter, unsigned int verbose,
                            int adaptive_rho, int gap_stop, void *x, void *y, void *l, void *mu,
                            double *optval, unsigned int *final_iter, int *status, double *rho_final);

/* Many small problems, each with its own matrix: k independent graph-form problems, problem j with its own
 * m x n matrix A_j and its own f[j], g[j], rho[j].  Each one is solved exactly as the one-shot PogsD / PogsS call
 * solves it: cold start, equilibration, norm estimate, direct projector (m > n factors I + A^T A, m <= n factors
 * I + A A^T), the reference's stopping rule and adaptive rho.  The whole solve of a problem runs on the device, one
 * workgroup per problem; a problem's outputs do not depend on k, on its position, on the other problems or on how
 * the call was split into chunks.
 * A: the k matrices back to back, matrix j at element offset j*m*n, each in `ord`.  Host or device memory (mem),
 *    dtype POGS_AMD_F32 / F64.  A device-resident A is never written.
 * opt: only opt->device and opt->projector are read (NULL = current device, direct projector).  CGLS is refused.
 * rho: k values, or NULL (1.0 each).  Tolerances, max_iter, adaptive_rho and gap_stop are shared.
 * Outputs are HOST arrays, laid out as in PogsAmdSolveBatchFn: problem j at offset j*n (x, mu) / j*m (y, l) /
 *    j (optval, final_iter, status).  y, l, mu, optval may be NULL.
 * Envelope: 1 <= min(m, n) <= POGS_AMD_MANY_MIN_DIM_MAX and max(m, n) <= POGS_AMD_MANY_MAX_DIM_MAX; any k >= 1.
 * Memory: the problems run in chunks whose device workspace (equilibrated A_j, W_j = L_j^-1, work vectors) stays
 *    under POGS_AMD_MANY_WORKSPACE_MB (environment, read at every call; default 1/8 of the device's memory; a
 *    chunk holds at least one problem).  A host A is uploaded chunk by chunk.
 * verbose > 0 prints ONE summary for the call (per-iteration lines mean nothing across k problems): k, the count
 *    of problems per status, the range of iterations, setup and loop time, launches.
 * Returns 0 when the problems ran (status[j] holds each PogsStatus).  Returns POGS_ERROR when refused:
 *    PogsAmdLastError says why, and no output has been written. */
#define POGS_AMD_MANY_MIN_DIM_MAX 512
#define POGS_AMD_MANY_MAX_DIM_MAX 16384
int PogsAmdSolveManyFn(int dtype, enum ORD ord, int k, size_t m, size_t n, const void *A, int mem,
                       const PogsAmdOptions *opt, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho,
                       double abs_tol, double rel_tol, unsigned int max_iter, unsigned int verbose,
                       int adaptive_rho, int gap_stop, void *x, void *y, void *l, void *mu,
                       double *optval, unsigned int *final_iter, int *status);

/* A persistent many-problem handle: the k problems of PogsAmdSolveManyFn set up ONCE and re-solved with new f, g.
 * PogsAmdManyCreate: arguments, envelope and refusals of PogsAmdSolveManyFn (dtype, ord, k >= 1, the two dimension
 *    caps, CGLS refused).  It runs the one-shot call's setup and keeps resident, for all k problems, the equilibrated
 *    A_j, d, e, the norm estimate, W_j = L_j^-1, the work vectors and each problem's last un-scaled x and l.  A host A
 *    is uploaded in chunks whose staging stays under POGS_AMD_MANY_WORKSPACE_MB; a device A is read during create,
 *    never written and never referenced afterwards.  There is no chunked handle: if the resident footprint cannot be
 *    allocated, create returns POGS_ERROR, *out is NULL and nothing is left allocated (PogsAmdSolveManyFn remains).
 * PogsAmdManySolveFn: f, g, tolerances, outputs (layout, NULL-able y, l, mu, optval) and per-problem status as in
 *    PogsAmdSolveManyFn.  rho_final: NULL or k doubles, each problem's rho when it stopped.  Every call states its
 *    start (the warm start is not sticky):
 *    POGS_AMD_MANY_COLD        z = zt = 0; rho NULL = 1.0 each.  A problem's bytes are those PogsAmdSolveManyFn
 *                              returns for it, however many solves preceded.
 *    POGS_AMD_MANY_WARM_GIVEN  x0 (k*n) and l0 (k*m), HOST arrays of the handle's dtype, both required.  Per problem
 *                              the reference's SetInitX + SetInitLambda (src/cpu/pogs.cpp:144-156): x = x0 / e,
 *                              y = A x, t = l0 / d, xt = (-A^T t) (-1 / rho), yt = t (-1 / rho) with this call's rho
 *                              of the problem; rho NULL = 1.0 each.
 *    POGS_AMD_MANY_WARM_LAST   the same initialisation from each problem's own last x, l kept on the device (nothing
 *                              is uploaded); rho NULL = each problem's last final rho.  Refused before the handle's
 *                              first solve.  A problem whose last status was neither POGS_SUCCESS nor POGS_MAX_ITER
 *                              starts cold at rho = 1.
 *    (WARM_GIVEN uploads x0, l0 into the kept buffers and then takes the WARM_LAST path.)
 *    verbose > 0 prints the one-line summary of PogsAmdSolveManyFn with the start mode.
 *    Returns 0 when the problems ran, POGS_ERROR when refused (PogsAmdLastError says why): a NULL handle, f, g, x,
 *    final_iter or status, an unknown start, and the cases above.  A refused call writes no output and leaves the
 *    handle as it was.
 * PogsAmdManyGetInfo: the handle's shape, its resident bytes, create's setup time and the last solve's counters. */
typedef struct PogsAmdMany PogsAmdMany; /* opaque */
enum POGS_AMD_MANY_START { POGS_AMD_MANY_COLD = 0, POGS_AMD_MANY_WARM_GIVEN = 1, POGS_AMD_MANY_WARM_LAST = 2 };
typedef struct PogsAmdManyInfo {
  int k, dtype;
  size_t m, n;
  size_t resident_bytes;              /* device memory the handle holds                      */
  double setup_s;                     /* PogsAmdManyCreate: upload and setup, wall clock     */
  /* last PogsAmdManySolveFn */
  double loop_s;                      /* begin and loop launches, wall clock                 */
  unsigned long long launches;        /* kernel launches                                     */
  unsigned long long problem_iters;   /* sum over the problems of the iterations executed    */
  double reserved[8];
} PogsAmdManyInfo;
int PogsAmdManyCreate(PogsAmdMany **out, int dtype, enum ORD ord, int k, size_t m, size_t n, const void *A, int mem,
                      const PogsAmdOptions *opt);
int PogsAmdManySolveFn(PogsAmdMany *h, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho, int start,
                       const void *x0, const void *l0, double abs_tol, double rel_tol, unsigned int max_iter,
                       unsigned int verbose, int adaptive_rho, int gap_stop, void *x, void *y, void *l, void *mu,
                       double *optval, unsigned int *final_iter, int *status, double *rho_final);
int PogsAmdManyGetInfo(const PogsAmdMany *h, PogsAmdManyInfo *out);
void PogsAmdManyDestroy(PogsAmdMany *h);

/* Ragged many-problem solves: the k problems of PogsAmdSolveManyFn, problem j with its own shape m[j] x n[j].  The
 * same kernels solve them, one workgroup per problem, and problem j's outputs are the bytes PogsAmdSolveManyFn
 * returns for it alone (k = 1), whatever its position, its neighbours and the chunks.
 * PogsAmdSolveManyRaggedFn: m, n: HOST arrays of k shapes.  Every packed array holds the problems back to back:
 *    A: matrix j at element offset sum_{i<j} m[i] n[i], each in `ord`, host or device (mem); the offset may have any
 *       element alignment; a device A is never written.
 *    f[j] describes m[j] entries and g[j] n[j] entries: a caller that packs its coefficient arrays puts problem j's
 *       at row offset sum_{i<j} m[i] (f) / column offset sum_{i<j} n[i] (g) and points f[j], g[j] there.
 *    Outputs (HOST): x, mu at the column offset; y, l at the row offset; optval, final_iter, status at j.
 *    Every other argument as in PogsAmdSolveManyFn.  Envelope, per problem: 1 <= min(m[j], n[j]) <=
 *    POGS_AMD_MANY_MIN_DIM_MAX and max(m[j], n[j]) <= POGS_AMD_MANY_MAX_DIM_MAX.  Chunks are packed by each
 *    problem's own footprint under POGS_AMD_MANY_WORKSPACE_MB; a chunk holds at least one problem.
 *    Refused with POGS_ERROR before any device work, no output written, PogsAmdLastError naming the argument and, for
 *    a shape, the problem's index: k < 1; NULL m, n, A, f, g, x, final_iter or status; an unknown ord, dtype or mem;
 *    a problem outside the envelope; CGLS.
 * PogsAmdManyCreateRagged: PogsAmdManyCreate over ragged problems (arguments and refusals as above).  The handle is
 *    a PogsAmdMany: PogsAmdManySolveFn (all three starts, rho_final), PogsAmdManyGetInfo and PogsAmdManyDestroy work
 *    on it with the ragged layouts above (x0 at the column offsets, l0 at the row offsets).  PogsAmdManyInfo.m / .n
 *    report the largest m[j] / n[j].
 * PogsAmdManyGetShapes: the k shapes of a handle of either kind into m and n (k values each). */
int PogsAmdSolveManyRaggedFn(int dtype, enum ORD ord, int k, const size_t *m, const size_t *n, const void *A, int mem,
                             const PogsAmdOptions *opt, const PogsAmdFn *f, const PogsAmdFn *g, const double *rho,
                             double abs_tol, double rel_tol, unsigned int max_iter, unsigned int verbose,
                             int adaptive_rho, int gap_stop, void *x, void *y, void *l, void *mu,
                             double *optval, unsigned int *final_iter, int *status);
int PogsAmdManyCreateRagged(PogsAmdMany **out, int dtype, enum ORD ord, int k, const size_t *m, const size_t *n,
                            const void *A, int mem, const PogsAmdOptions *opt);
int PogsAmdManyGetShapes(const PogsAmdMany *h, size_t *m, size_t *n);

/* Benchmark stepping.  PogsAmdBeginRun loads f/g and the solve parameters and
 * resets the ADMM state to the cold start; PogsAmdIterate then advances exactly
 * `iters` ADMM iterations of real solves (restarting from the cold start each
 * time a solve converges or hits max_iter), and returns the elapsed seconds
 * measured with HIP events on the solver's stream. */
int PogsAmdBeginRun(PogsAmdSolver *s,
                    const void *f_a, const void *f_b, const void *f_c, const void *f_d,
                    const void *f_e, const int *f_h,
                    const void *g_a, const void *g_b, const void *g_c, const void *g_d,
                    const void *g_e, const int *g_h,
                    double rho, double abs_tol, double rel_tol, unsigned int max_iter,
                    int adaptive_rho, int gap_stop);
int PogsAmdIterate(PogsAmdSolver *s, unsigned int iters, double *seconds,
                   unsigned int *solves_completed);

/* Warm start for the NEXT PogsAmdSolve / PogsAmdBeginRun call only (reference: C++-only
 * SetInitX / SetInitLambda, src/include/pogs.h:112-119, consumed at src/cpu/pogs.cpp:144-180;
 * as there, x0 and l0 must be given together).  HOST pointers: x0 (n), l0 (m_local). */
int PogsAmdSetWarmStart(PogsAmdSolver *s, const void *x0, const void *l0);

int PogsAmdGetStats(const PogsAmdSolver *s, PogsAmdStats *out);
int PogsAmdResetStats(PogsAmdSolver *s);
void PogsAmdDestroy(PogsAmdSolver *s);

/* Last error message of the calling thread ("" if none). */
const char *PogsAmdLastError(void);

/* Device memory pool.  The reference builds and destroys its solver inside every one-shot call
 * (src/interface_c/pogs_c.cpp:19-20, 67-68), i.e. its working set is allocated and freed per
 * call; on the GPU that costs map / first-touch / unmap stalls of 0.1-0.3 s at 5 GB.  The
 * library therefore keeps the device blocks of destroyed handles (and of finished PogsD/PogsS
 * calls) in a per-device cache and hands them to the next handle.  At most POGS_AMD_POOL_MB
 * (environment; default a quarter of the device's memory, 0 = no caching) stay idle per device;
 * an allocation that fails is retried after the cache has been emptied. */
typedef struct PogsAmdPoolInfo {
  unsigned long long mallocs;   /* blocks taken from the HIP runtime                    */
  unsigned long long reuses;    /* blocks taken from the cache                          */
  unsigned long long frees;     /* blocks given back to the HIP runtime                 */
  double malloc_ms, free_ms;    /* host time spent inside hipMalloc / hipFree           */
  size_t cached_bytes;          /* idle in the cache now                                */
  size_t live_bytes;            /* in use by handles now                                */
  size_t peak_cached_bytes;
} PogsAmdPoolInfo;
int PogsAmdPoolStats(int device, PogsAmdPoolInfo *out);
/* Gives the idle blocks of `device` (-1: every device) back to the HIP runtime. */
int PogsAmdPoolTrim(int device, size_t *freed_bytes);

/* ---------------------------------------------------------------------------
 * Part 3 -- building blocks exported for parity tests (device pointers unless
 * noted).  Not needed by a drop-in caller.
 * ------------------------------------------------------------------------- */

/* out[i] = Prox{f_i}(in[i]) with penalty rho; SoA coefficients; all HOST
 * pointers of type dtype (reference: ProxEval, src/include/prox_lib.h:207-230,
 * 503-511).  The evaluation runs on the GPU. */
int PogsAmdProxEval(int dtype, size_t n, const int *h, const void *a, const void *b,
                    const void *c, const void *d, const void *e, double rho,
                    const void *in, void *out);
/* sum_i f_i(in[i])  (reference: FuncEval, src/include/prox_lib.h:326-349,520-529) */
int PogsAmdFuncEval(int dtype, size_t n, const int *h, const void *a, const void *b,
                    const void *c, const void *d, const void *e, const void *in,
                    double *out);
/* v_out[i] = ProjSubgrad{f_i}(v_in[i]) at x_in[i]: the point of the subdifferential of f_i at
 * x_in[i] closest to v_in[i] (reference: ProjSubgradEval, src/include/prox_lib.h:468-493,
 * 538-546; unused by the reference's solvers, part of its prox library).  HOST pointers. */
int PogsAmdProjSubgradEval(int dtype, size_t n, const int *h, const void *a, const void *b,
                           const void *c, const void *d, const void *e, const void *x_in,
                           const void *v_in, void *v_out);
/* Equilibrated matrix, scalings and norm estimate of a solver (HOST outputs,
 * any may be NULL): A_eq (m*n row-major), d (m), e (n). */
int PogsAmdGetEquil(const PogsAmdSolver *s, void *A_eq, void *d, void *e, double *nrmA);
/* Projection onto {y = A_eq x}: (x, y) = argmin |x-x0|^2 + |y-y0|^2 (HOST ptrs).  tol: the relative tolerance of
 * a CGLS handle's loop; a handle with the direct projector (dense or sparse) projects exactly and ignores it. */
int PogsAmdProject(PogsAmdSolver *s, const void *x0, const void *y0, double tol,
                   void *x, void *y);
/* y = alpha * op(A_eq) x + beta * y on the solver's operator (HOST ptrs);
 * trans = 'n' or 't' (reference: Matrix::Mul). */
int PogsAmdMul(PogsAmdSolver *s, char trans, double alpha, const void *x, double beta,
               void *y);
/* Diagnostic: GB/s at which `device` (-1: current) reads `bytes` of device memory with nothing else to
 * do -- the better of two read-only kernels (all workgroups side by side, 16-byte non-temporal loads; the
 * row-block shape of the dense pass), `reps` timed launches each.  bench.py prints it as
 * roofline.peak_measured next to the data-sheet peak.  *pattern (may be NULL): 0 or 1, which one won. */
int PogsAmdReadBandwidth(int device, size_t bytes, int reps, double *gb_per_s, int *pattern);
/* Diagnostic: the 64-lane wavefront sums of the engine formed in the vector ALU (dev::wave_sum_valu:
 * v_permlane32_swap / v_permlane16_swap / DPP, csrc/reduce.h) in the order of the butterfly
 * `v += shfl_xor(v, 32, 16, 8, 4, 2, 1)` -- the fp32 tree of the streaming row dots and the fp64 tree of every
 * scalar sum.  For n (a multiple of 64) HOST values this returns, per value, its wavefront's total formed that way
 * (alu) and by the butterfly through the LDS crossbar (lds): the two must agree bit for bit
 * (tests/test_gpu_dense.py). */
int PogsAmdWaveSumCheck(int dtype, size_t n, const void *in_host, void *alu_host, void *lds_host);
/* Diagnostic: the logical workgroup ids of the dense one-pass iteration kernels (csrc/stream.h: logical_block_id),
 * which deal rows and partial-sum slots by them.  Launches `grid` workgroups and returns ids_host[b] = the id that
 * block b computed: a permutation of 0 .. grid - 1 for every grid.  *group: blocks whose index agrees modulo this
 * number take consecutive ids (0: built with blockIdx.x as the id).  tests/test_gpu_block_ids.py. */
int PogsAmdBlockIdCheck(int grid, int *ids_host, int *group);

/* Diagnostics of the batched and many-problem kernels.  Every array is a HOST pointer of type dtype (0 fp32,
 * 1 fp64) unless noted; each entry uploads its inputs, runs the launch functions and geometry the solvers call, and
 * downloads the results.  k (1 <= k <= POGS_AMD_BATCH_MAX) problems are stored at stride ld in X / Y / U / Z;
 * act[0 .. nact) (1 <= nact <= k, distinct, in [0, k)) lists the problems of the launch, slot q running problem
 * act[q].  Output arrays are uploaded before the launch and downloaded after it, so entries a launch does not write
 * come back as they were.  VEC = 16 / sizeof(element) (4 fp32, 2 fp64), cols_pad = round_up(cols, VEC).  Invalid
 * arguments are refused before any device work: POGS_ERROR, and PogsAmdLastError says why. */
/* Y[p][r] = sum_c M[r][c] X[p][c] for r < rows and the problems p of act (the batched solve's launch_batch_rows).
 * M: rows x ldm row-major; ldm, ldx: multiples of VEC, >= cols_pad; ldy >= rows.  tri: 0 full, 1 lower (c <= r),
 * 2 upper (c >= r) triangle of a square M (rows == cols); entries outside the triangle and M's columns >= cols are
 * never used.  Contract of the caller (batch_admm.h's vectors keep it): X[p][c] == 0 for cols <= c < cols_pad. */
int PogsAmdBatchRowsCheck(int dtype, int tri, int rows, int cols, const void *M, size_t ldm, int k, const int *act,
                          int nact, const void *X, size_t ldx, void *Y, size_t ldy);
/* Z[p][c] = sum_r M[r][c] U[p][r] (+ add[p][c] when add is not NULL) for c < cols, Z[p][c] = 0 for
 * cols <= c < cols_pad (launch_batch_cols over the row-block partition of the batched solve, then
 * launch_batch_cols_reduce).  M: rows x ldm row-major, ldm a multiple of VEC, >= cols_pad; ldu >= rows;
 * ldz >= cols_pad (also add's).  *nrb_used and *rpb report the partition: row blocks and rows per block. */
int PogsAmdBatchColsCheck(int dtype, int rows, int cols, const void *M, size_t ldm, int k, const int *act, int nact,
                          const void *U, size_t ldu, const void *add, void *Z, size_t ldz, int *nrb_used, int *rpb);
/* The two entries above for a matrix stored as floats -- the kernels with which a batched solve on a mixed-storage
 * handle (POGS_AMD_STORE_F32) can read the float copy (launch_batch_rows_mixed, launch_batch_cols_mixed over the fp64
 * row-block partition, then launch_batch_cols_reduce): dtype fp64 is implied and the full form only.  M is a HOST
 * array of FLOATS, rows x ldm row-major, ldm a multiple of 4 and >= round_up(cols, 4); X / U / Y / Z / add are doubles
 * under the fp64 entries' constraints (ldx, ldz multiples of 2 and >= round_up(cols, 2); ldy, ldu >= rows).  The
 * results are, bit for bit, those of the fp64 entries on M widened to doubles, *nrb_used and *rpb included; what M
 * holds from column cols to ldm is never used (tests/test_gpu_batch_mixed_kernels.py). */
int PogsAmdBatchRowsMixedCheck(int rows, int cols, const float *M, size_t ldm, int k, const int *act, int nact,
                               const double *X, size_t ldx, double *Y, size_t ldy);
int PogsAmdBatchColsMixedCheck(int rows, int cols, const float *M, size_t ldm, int k, const int *act, int nact,
                               const double *U, size_t ldu, const double *add, double *Z, size_t ldz, int *nrb_used,
                               int *rpb);
/* Y[p][r] = sum_q val[q] X[p][ind[q]] over ptr[r] <= q < ptr[r+1] (+ beta yin[p][r] when yin is not NULL), the
 * batched sparse solve's product (sp_batch_geometry, launch_sp_batch_pack, launch_sp_batch_spmv).  CSR of
 * nrows x ncols: ptr (nrows + 1, ptr[0] == 0, non-decreasing), ind in [0, ncols) (int32).  ldx >= ncols,
 * ldy >= nrows, ldin >= nrows.  part (doubles, may be NULL): part[p * grid + w] = the sum of the squares of the Y
 * values of workgroup w; it must hold k * max(1, ceil(nrows / 4)) doubles (>= k * grid).  num_cu: the CU count the
 * geometry is chosen for (0: the device's).  geom (3 ints) = {log2 lanes per row, rows per workgroup, grid}. */
int PogsAmdSpBatchSpmvCheck(int dtype, int nrows, int ncols, const int *ptr, const int *ind, const void *val, int k,
                            const int *act, int nact, const void *X, size_t ldx, double beta, const void *yin,
                            size_t ldin, void *Y, size_t ldy, double *part, int num_cu, int *geom);
/* The setup of PogsAmdSolveManyFn on k problems in one chunk (its launch sequence: copy, Sinkhorn-Knopp, scale,
 * norm estimate, Gram tiles, Cholesky, W = L^-1); arguments and refusals as there.  Per problem j (HOST outputs,
 * any may be NULL): A_eq + j m n (m x n row-major), d + j m, e + j n, nrmA[j], and W + j K^2 with K = min(m, n):
 * K x K row-major, W = L^-1 in its lower triangle for L L^T = I + A_eq^T A_eq (m > n) or I + A_eq A_eq^T. */
int PogsAmdManySetupCheck(int dtype, enum ORD ord, int k, size_t m, size_t n, const void *A, int mem, void *A_eq,
                          void *d, void *e, double *nrmA, void *W);
/* Diagnostics of the dense factorisation (DenseSolver::factor: Gram product, Cholesky, L^-1).  HOST arrays of type
 * dtype, row-major; invalid arguments are refused before any device work, as above. */
/* G = P^T P for a K-major operand P (kdim rows of k columns, leading dimension lda: what a tall handle stores, and a
 * wide one, which keeps A^T), by the very function factor() calls, which picks the product from (kdim, k, CU count):
 * native fp32 / fp64 MFMA tiles, split-K into slabs, two-level accumulation, or the fp16 split on the 128 or 256 tile.
 * (The row-major operand form of the native product cannot be reached from factor() and is not offered.)  lda: a
 * multiple of VEC, >= k; P's columns >= k are never read.  num_cu: 0 = the device's.  force: 0 = as a solve would
 * choose (the environment included), 1 = POGS_AMD_GRAM=fp32, 128 / 256 = POGS_AMD_GRAM_TILE (like the variable it
 * only picks the tile where the fp16 split is the product of the shape).  G: k x ldg (ldg >= k), uploaded before and
 * downloaded after: the lower 128-tiles are written (whole diagonal tiles, so G is symmetric inside them), entries
 * above them come back as they were.  info (8 ints) = {path (0 native, 1 fp16 split), tile, ksplit, kchunk, kacc,
 * K units, rows per unit, 1 if the tiles ran in gram_tile_order}; ksplit, kchunk and kacc are 0 on path 1. */
int PogsAmdGramCheck(int dtype, int kdim, int k, const void *P, size_t lda, int num_cu, int force, void *G, size_t ldg,
                     int *info);
/* For a symmetric positive definite H (n x ldh, n >= 1; only the lower triangle is read) the sequence of factor()
 * after the diagonal shift: four zeroed slabs of n x ld, ld = round_up(n, VEC), H into the first, cholesky_lower,
 * trtri_lower, launch_transpose.  L (L L^T = H), W = L^-1 and U = W^T come back as the slabs hold them, rows of
 * min(ldo, ld) columns at stride ldo (ldo >= n): the strict upper triangle of L is what H held there, that of W and
 * the strict lower one of U are zero, and so are the columns n .. ld.  An H that is not positive definite is no
 * error: the square root of the bad pivot is NaN, and NaN spreads from there (the reference's
 * linalg_cholesky_decomp reports an error instead). */
int PogsAmdCholCheck(int dtype, int n, const void *H, size_t ldh, void *L, void *W, void *U, size_t ldo);
/* Diagnostic of the solo sparse solver's product.  HOST arrays; invalid arguments are refused before any device work, as
 * above.  The entry builds what the constructor of a sparse handle builds before its equilibration, by the same
 * functions: both CSR copies (the second transposed on the device), and of each the tiled lane-stream copy the product
 * streams, or the row blocks of the plain CSR kernel where that copy is not built.  The matrix (nrows x ncols) is given
 * as PogsAmdCreateSparse takes it: ord = ROW_MAJ: CSR (ptr: nrows + 1), COL_MAJ: CSC (ptr: ncols + 1); ptr[0] == 0,
 * indices need not be sorted and entries may repeat (they add up).  A matrix without entries is refused.
 *   num_cu: the CU count the geometry is chosen for (0: the device's).
 *   format: 0 as a solve chooses (POGS_AMD_SELL_FORMAT and POGS_AMD_SPMV included), 1 a row tag per element, 2 two id
 *     slots per batch, 3 the plain CSR kernel on both copies.
 *   force_rr_rows, force_ncg: 0, or the rows per row range (a multiple of 64 in [512, 16384 fp32 / 6144 fp64]) and the
 *     number of column groups (1 .. min(column blocks, 32)) that replace the solver's choice on the copy the product
 *     runs on (A for trans = 'n', A^T for 't'); the other copy is built as a solve builds it.
 *   scale: after the build every value of both CSR copies is multiplied by it and the tiled values are written a second
 *     time from the CSR copy, through the table of positions the first fill recorded (what a handle does with the
 *     equilibrated values); scale = 1 takes the same way.
 *   Then one product with the functor of the norm estimate:  y = alpha op(A)' x' + beta y,  op = A (trans 'n') or A^T
 *   ('t'), every entry of A squared when sq != 0, x' = x / sqrt(x_nrm2) (x_nrm2 = 0: x itself, no scalar is read);
 *   *sumsq = the sum of the squares of the new y, added up in fp64 by the launches a solve uses.
 *   x: xlen >= (columns of op) elements, all uploaded; y: ylen >= (rows of op) elements, uploaded before and downloaded
 *   after, so that what lies behind the vectors must come back as it was.
 *   info (16 ints), 8 for A and 8 for A^T: {1 if tiled, 1 if two id slots, rows per row range, row ranges, column
 *     blocks, column groups, stored 64-element units, why not tiled}; the last is 0 on a tiled copy, else 1 no
 *     non-zeros (a handle's code; this entry refuses such a matrix), 2 the plan (6 to 10 bytes per (row, column block)) too large, 3 a stream offset of the planner out of
 *     range, 4 padding beyond 4 nnz + 2^22 stored elements, 5 a row holds more than 65535 entries in one column block
 *     (repeated entries), 6 the plain kernel pinned.  The geometry fields are 0 on a copy that is not tiled.
 *   t_ptr, t_ind, t_val (each may be NULL): the CSR copy built on the device (A^T for CSR input, A for CSC input) as
 *     the build leaves it, before `scale`: rows sorted by index, equal indices by the value's bit pattern as unsigned. */
int PogsAmdSpmvCheck(int dtype, enum ORD ord, int nrows, int ncols, const int *ptr, const int *ind, const void *val,
                     int num_cu, int format, int force_rr_rows, int force_ncg, double scale, char trans, int sq,
                     double x_nrm2, double alpha, double beta, const void *x, size_t xlen, void *y, size_t ylen,
                     double *sumsq, int *info, int *t_ptr, int *t_ind, void *t_val);
/* The same diagnostic for the product of a mixed-storage handle (PogsAmdCreateSparseMixed), fp64: the copies are built as
 * PogsAmdSpmvCheck builds them for POGS_AMD_F64 and multiplied by `scale`; then every value of both CSR copies is rounded
 * to the nearest float (kept as that double), the tiled values are written as FLOATS through the table of positions,
 * and one product with the functor of the norm estimate runs on them (format 3: the plain CSR kernel on the rounded
 * doubles).  There is no `sq`: the mixed kernel has no squared form.  Arguments, refusals and info as PogsAmdSpmvCheck. */
int PogsAmdSpmvMixedCheck(enum ORD ord, int nrows, int ncols, const int *ptr, const int *ind, const double *val,
                          int num_cu, int format, int force_rr_rows, int force_ncg, double scale, char trans,
                          double x_nrm2, double alpha, double beta, const double *x, size_t xlen,
                          double *y, size_t ylen, double *sumsq, int *info);
/* Diagnostic of the sparse solver's projection: one run of its CGLS loop on given vectors, on a live sparse handle (one
 * GPU), by the member functions and launches an ADMM iteration uses, without the prox step.  HOST arrays of the handle's
 * type; n-sized: x0, x_warm, x_prev, x12, x, xtemp, p, sv; m-sized: y0, y_warm, y12, y_new, ytemp, r.  A is the handle's
 * equilibrated matrix (PogsAmdGetEquil).  The projection of (x0, y0) onto {y = A x} is started from x_warm, and y_warm
 * stands for A x_warm (inside a solve: the previous iterate, whose y is also the y_prev of the bookkeeping, so y_warm is
 * both here).  The entry uploads x0 / y0 into the solver's xtemp / ytemp, y_warm, x_prev, x12 and y12 into the previous
 * iterate and the prox point, and then, by `loop`:
 *   0  the device-resident loop (csrc/cg_fused.h): r = y0 - y_warm and x = x_warm - x0 as the prox launch leaves them,
 *      the done flag and the step count cleared, then the loop with `ahead` (>= 1) steps enqueued before the first host
 *      poll, at most max_steps (>= 1; a solve: 500) steps in all, the closing launch (x += x0, the sums of
 *      (x_prev - x)^2, (x12 - x)^2, xtemp -= x, and the same of the y half from the recurrence y_warm + sum alpha q);
 *      ysync = 1: y_new = A x by the product instead, with the y half's bookkeeping in that launch.
 *   1  the host-polled loop (cgls_project) warm-started with x_warm and A x_warm = y_warm, then y_new = A x with the
 *      y half's bookkeeping and the x half's launch; 2: the same loop as PogsAmdProject runs it, from x = x_warm with
 *      both products of the start taken (y_warm only serves as y_prev).  max_steps, ahead and ysync are not used.
 * tol: the relative tolerance of cgls.h:301-305.  Outputs: x, y_new; xtemp, ytemp as the closing launches leave them; the
 * loop's r, p, s (sv); slots (17 doubles): the scalar block's kFcDone, kFcSteps, kFcNorms0, kFcGamma0, kFcGamma1,
 * kFcAlpha, kFcBeta, kFcDelta, kFcIndef (loop 0 only; csrc/vec_kernels.h), kCgQ2, kCgP2, kCgS2, kCgX2 (the last step's
 * |q|^2, |p|^2 before it, |s|^2, |x|^2), kDXprev2, kDX12, kDYprev2, kDY12; rec_x (512 doubles, loop 0): the per-block
 * |x|^2 records of the last step, set to NaN before the loop, so that a record no block wrote comes back as NaN (the
 * first ceil(n / 1024) are written); info (16 ints): the geometry words of PogsAmdSpmvCheck for A and A^T; *enqueued:
 * the steps the host enqueued (loop 0) or ran (1, 2).
 * POGS_ERROR, before any device work: a null argument, ahead < 1, max_steps < 1, loop or ysync out of range, a dense or
 * row-sharded handle, a sparse handle with the direct projector (it has no CGLS loop), and with loop 0 a handle whose copies are not both tiled or that was created with POGS_AMD_CG=h.
 * The handle solves afterwards as if the call had not been made (its step prediction and its statistics are put back);
 * a run begun with PogsAmdBeginRun is lost, PogsAmdIterate is refused until the next PogsAmdBeginRun / PogsAmdSolve. */
int PogsAmdSparseCgCheck(PogsAmdSolver *s, const void *x0, const void *y0, const void *x_warm, const void *y_warm,
                         const void *x_prev, const void *x12, const void *y12, double tol, int max_steps, int ahead,
                         int ysync, int loop, void *x, void *y_new, void *xtemp, void *ytemp, void *r, void *p, void *sv,
                         double *slots, double *rec_x, int *info, int *enqueued);
/* Diagnostic of the dense fused CGLS projector: one projection on given vectors, on a live handle created with
 * POGS_AMD_PROJ_CGLS_FUSED, by the member an ADMM iteration calls, without the prox step.  HOST arrays of the handle's
 * type; n-sized: x0, x_warm, x, p, sv; m-sized: y0, y_warm, y_new, r.  A is the handle's equilibrated matrix
 * (PogsAmdGetEquil).  The projection of (x0, y0) onto {y = A x} is started from x_warm, and y_warm stands for A x_warm.
 * The entry puts r = y0 - y_warm and x = x_warm - x0 in place as the prox launch leaves them, clears the done flag and
 * the step count, and runs the loop with `ahead` (>= 1) steps enqueued before the first host poll and at most
 * max_steps (>= 1; a solve: 500) in all, then the closing launch (x += x0).  ysync = 0: y_new = y_warm + sum alpha q;
 * 1: y_new = A x by the product.  tol: the relative tolerance of cgls.h:301-305.  Outputs: x, y_new; the loop's r, p,
 * s (sv); slots (17 doubles) as PogsAmdSparseCgCheck returns them; *enqueued: the steps the host enqueued; *steps: the
 * steps the loop took; *matvecs: the launches that read A (what the call added to stats.matvecs).
 * POGS_ERROR, before any device work: a null argument, ahead < 1, max_steps < 1, ysync out of range, any other kind of
 * handle.  The handle solves afterwards as if the call had not been made (its step prediction and its statistics are
 * put back); a run begun with PogsAmdBeginRun is lost, PogsAmdIterate is refused until the next PogsAmdBeginRun /
 * PogsAmdSolve. */
int PogsAmdDenseCgCheck(PogsAmdSolver *s, const void *x0, const void *y0, const void *x_warm, const void *y_warm,
                        double tol, int max_steps, int ahead, int ysync, void *x, void *y_new, void *r, void *p, void *sv,
                        double *slots, int *enqueued, int *steps, unsigned long long *matvecs);
/* W = L^-1 and U = W^T of a handle with the direct projector (dense, or sparse created with POGS_AMD_PROJ_DIRECT),
 * L L^T = I + A_eq^T A_eq (m > n) or I + A_eq A_eq^T: HOST outputs of k x k, k = min(m, n), either may be NULL.  On
 * row shards every rank holds the factor of the whole matrix.  POGS_ERROR on a handle that runs the CGLS projector
 * (a sparse one: "needs a dense handle"). */
int PogsAmdGetFactor(const PogsAmdSolver *s, void *W, void *U);
/* Diagnostics of the sparse direct projector (csrc/sparse_direct.h).  HOST arrays of type dtype; invalid arguments are
 * refused before any device work, as above. */
/* The lower triangle of the Gram matrix a direct sparse handle factors, G = A^T A (nrows > ncols, K = ncols) or A A^T
 * (K = nrows), by the launch its set-up runs, on copies built as a handle builds them (the matrix as PogsAmdSpmvCheck
 * takes it: CSR or CSC, indices unsorted and entries repeated allowed, no empty matrix; the values are used as given,
 * without equilibration).  Sums are formed in double for both types and rounded once; the result depends on the
 * matrix alone (not on window, num_cu or the run).  K <= POGS_AMD_SPARSE_DIRECT_MAX.  num_cu: 0 = the device's.
 * window: the columns of a row a wavefront accumulates in LDS at a time: 0 = the solver's choice, else a multiple of
 * 64 in [64, 2048].  G: K x ldg row-major (ldg >= K), uploaded before and downloaded after: every G[i][j], j <= i, is
 * written (zeros included), the strict upper triangle and the columns >= K come back as given.  info (8 ints) = {K,
 * 1 if nrows > ncols, window used, windows of the last row, workgroups, leading dimension on the device, 0, 0}. */
int PogsAmdSparseGramCheck(int dtype, enum ORD ord, int nrows, int ncols, const int *ptr, const int *ind,
                           const void *val, int num_cu, int window, void *G, size_t ldg, int *info);
/* y = tri(M) x by the solo solve's triangular mat-vec: M n x ldm row-major (ldm a multiple of VEC, >= n), tri 1: the
 * lower triangle (columns 0 .. i of row i), 2: the upper one (columns i .. n - 1); x, y: n elements.  Nothing outside
 * the triangle and nothing in columns n .. ldm is read. */
int PogsAmdTriMatvecCheck(int dtype, int tri, int n, const void *M, size_t ldm, const void *x, void *y);
/* Diagnostic of the dense streaming passes (csrc/stream.h) and of the column side between two passes
 * (csrc/fused_cols.h): ONE pass over a stored matrix and its second stage on caller-supplied HOST arrays, by the
 * launch functions and kernel instantiations a dense solve uses (the per-shape objects of csrc/dense_plan.hip).  No
 * iteration is modelled: every output is a function of this call's inputs alone.
 *   M: rows x ldm row-major, ldm a multiple of VEC and >= n_pad = round_up(n, VEC).  Contract of the caller, as the
 *   solver's buffers keep it: M's columns n .. n_pad and the entries n .. n_pad of x0 / x1 are ZERO; nothing in columns
 *   n_pad .. ldm is read.  W_SWEEP (rows == n, the lower triangle of M): a row is read in whole 16-byte vectors up to
 *   and including the vector that holds its diagonal, so the entries right of the diagonal inside that vector must be
 *   zero; no vector wholly right of the diagonal is read.
 *   The shape is make_stream_plan(n_pad, num_cu) (num_cu = 0: the device's; POGS_AMD_XL_LIMIT is honoured), or the shape
 *   (force_tpb, force_nv) of POGS_STREAM_PLANS when force_tpb != 0: it must hold n_pad (tpb nv VEC >= n_pad).  The
 *   per-solve tuning of the one-pass kernel (workgroups per CU, the prefetching kernel of fp32 256 x 5 with the logistic
 *   functor) is applied as a solve applies it.
 *   form / functor (pass, then second stage):
 *     PRE_ACC    the column-sum-only pass.  functor CHEAP: u0 = ytemp, u1 = y12 + zs yt - ycur (PreAccOp); XSIDE:
 *                u0 = ytemp, u1 = y12 (PreAcc2Op).
 *     ITER_FULL  the one-pass iteration's pass, two dots (x0, x1) and two column sums, functor FusedIterOp with the
 *                inlined cheap prox (CHEAP), the logistic prox (LOGISTIC) or the m <= n mirror (XSIDE: yt is the old
 *                dual vector, c_old its scale).  Row outputs ynew, ytemp (in / out), y12s, ytemps; scalars[0..6).
 *     ITER_LEAN  the same with one dot and one column sum (fp64 only: POGS_ERROR in fp32); scalars[2] stays 0.
 *     EXACT      the exact-residual pass: dot with x0, ExactRowOp (y12, yt, ycur, zs) -> scalars[0]; second stage
 *                ExactColOp (x12 as INPUT, xt, x_cur, zs) -> col_scalars[0]; tot0 = the raw column totals.  This is
 *                the form that runs on windowed plans.
 *     W_SWEEP    tot0 = M^T (M (x0 + x1)) over the lower triangle (x1 may be NULL), IdentRowOp.
 *   cols (second stage of PRE_ACC / ITER_*): REDUCE: tot0 / tot1 = the totals (reduce_cols, StoreColOp; padding columns
 *   zero); PRE: pre_cols_kernel with both partial sets, PRE_ONE: with the second set absent (the only one of the two a
 *   lean pass may take): g (g_h .. g_e), x_cur, xt, zt_scale = zs, rho, alpha -> x12, xtemp, rhs (n_pad entries
 *   written) and col_scalars[0..4); PACK: pack (2 n_pad + 6 doubles) = both totals as doubles, then scalars[0..6) as
 *   the extra workgroup of pack_cols_kernel sums them (not for ITER_LEAN).
 *   Scalar partials are added by launch_sum_jobs with the strides and offsets the iteration uses.
 *   Vectors: every row-side array (ycur, y12, yt, ytemp, ynew, y12s, ytemps, f_*) has row_len >= rows elements, every
 *   column-side one (x0, x1, tot0, tot1, x_cur, xt, x12, xtemp, rhs, g_*) col_len >= n_pad; dots (may be NULL) has
 *   2 row_len: M x0 and M x1 (W_SWEEP: M (x0 + x1) over the triangle, once) by the solver's plain row-dot launch.  An
 *   array a form does not use may be NULL.  Output arrays are uploaded before and downloaded after the launches, so what
 *   a launch does not write comes back as it was.  The device's partial-sum buffers start as NaN.
 *   info (8 ints) = {tpb, nv, rows per workgroup step, grid of the pass, windows, kernel (0 plain, 1 triangular,
 *   2 prefetching), partial sets' count handed to the second stage, 1 if windowed}.
 * Invalid arguments are refused before any device work: POGS_ERROR, and PogsAmdLastError names the argument. */
enum { POGS_AMD_PASS_PRE_ACC = 0, POGS_AMD_PASS_ITER_FULL = 1, POGS_AMD_PASS_ITER_LEAN = 2, POGS_AMD_PASS_EXACT = 3,
       POGS_AMD_PASS_W_SWEEP = 4 };
enum { POGS_AMD_PASS_FN_CHEAP = 0, POGS_AMD_PASS_FN_LOGISTIC = 1, POGS_AMD_PASS_FN_XSIDE = 2 };
enum { POGS_AMD_PASS_COLS_REDUCE = 0, POGS_AMD_PASS_COLS_PRE = 1, POGS_AMD_PASS_COLS_PRE_ONE = 2,
       POGS_AMD_PASS_COLS_PACK = 3 };
typedef struct PogsAmdDensePassArgs {
  int dtype, form, functor, cols;
  int rows, n;
  const void *M;
  size_t ldm;
  int num_cu, force_tpb, force_nv;
  size_t row_len, col_len;
  const void *x0, *x1;
  const void *ycur, *y12, *yt;
  void *ytemp;
  const int *f_h;
  const void *f_a, *f_b, *f_c, *f_d, *f_e;
  double rho, alpha, zs, c_old;
  void *ynew, *y12s, *ytemps, *dots;
  double *scalars;       /* 6 */
  void *tot0, *tot1;
  double *pack;
  const int *g_h;
  const void *g_a, *g_b, *g_c, *g_d, *g_e;
  const void *x_cur, *xt;
  void *x12, *xtemp, *rhs;
  double *col_scalars;   /* 4 */
  int *info;             /* 8 */
} PogsAmdDensePassArgs;
int PogsAmdDensePassCheck(const PogsAmdDensePassArgs *args);
/* The same diagnostic for the mixed-storage pass (csrc/stream_mixed.h: an fp64 one-pass iteration's pass over a FLOAT
 * matrix), by the launch functions a POGS_AMD_STORE_F32 handle calls.  Same struct, with these differences: dtype must
 * be POGS_AMD_F64 (the type of every vector); M is float, rows x ldm, ldm a multiple of 4 and >= round_up(n, 4), its
 * columns n .. round_up(n, 4) zero; forms ITER_FULL and ITER_LEAN, functors CHEAP and LOGISTIC, cols as above;
 * force_tpb / force_nv name a one-pass shape of the MIXED plan (the 64- and 256-thread shapes of POGS_STREAM_PLANS,
 * in float4 vectors: tpb nv 4 >= round_up(n, 4)), default make_stream_plan<float>(round_up(n, 4)); n <= 10240; dots
 * must be NULL.  All vectors are doubles with the length contract above (col_len >= round_up(n, 2)); info as above
 * (kernel = 3).  Invalid arguments are refused before any device work. */
int PogsAmdDensePassMixedCheck(const PogsAmdDensePassArgs *args);
/* Diagnostic of the single-vector streaming pass over a FLOAT matrix (csrc/stream_mixed.h: stream_rows_mixed_kernel,
 * what the recurring launches of a PogsAmdCreateDenseMixed handle's projector run): ONE launch and its second stage
 * on caller-supplied HOST arrays, through the launch functions and with the functors the solver uses.
 *   form ACC      (GemvTOp)     tot = M^T u                       (reduce_cols of the column partials); q, scalars untouched
 *   form DOT_ACC  (DcgQRowOp)   q = M x, tot = M^T q, scalars[0] = |q|^2 (the [grid] records added in order); guarded
 *   form DOT      (ProjTailOp)  q = M x, scalars[0] = scalars[1] = |q|^2 (its two sums against zero vectors); tot untouched
 * M is float, rows x ldm, ldm a multiple of 4 and >= round_up(n, 4), its columns n .. round_up(n, 4) zero; columns past
 * round_up(n, 4) are never read.  x and tot have round_up(n, 2) doubles, u and q `rows`, scalars 2.  num_cu (0: the
 * device's), force_tpb / force_nv (0 / 0: the plan of n) as PogsAmdDensePassMixedCheck reads them.  `done` is placed in
 * the guard's slot of a device scalar block before the launch: non-zero, the DOT_ACC launch returns before any load or
 * store and its second stage is not run, as every launch of an ended CG loop returns at the same flag.
 * q, tot and scalars are uploaded before the launch and downloaded after it, so what a launch does not write comes
 * back as given.  The partial buffers start as NaN; `partials` (may be NULL; ACC forms; partials_len
 * doubles, at least grid * round_up(n, 2) -- checked before the launch) receives the column partials as the launch
 * left them.  info (8 ints) = {tpb, nv, rows per step, grid, execution tpb,
 * execution nv, scalar sums per record, workgroups per CU}.  An argument a form does not name may be NULL.  Invalid
 * arguments are refused before any device work. */
enum POGS_AMD_STREAM_MIXED_FORM { POGS_AMD_STREAM_MIXED_ACC = 0, POGS_AMD_STREAM_MIXED_DOT_ACC = 1, POGS_AMD_STREAM_MIXED_DOT = 2 };
int PogsAmdStreamMixedCheck(int form, int rows, int n, const float *M, size_t ldm, int num_cu, int force_tpb, int force_nv,
                            const double *x, const double *u, double done, double *q, double *tot, double *scalars,
                            double *partials, size_t partials_len, int *info);
/* Diagnostic of the kernels that do not read the matrix (csrc/vec_kernels.hip) and of the scalar block's way to the host
 * (csrc/engine.h: Ctx::queue_sum / fetch_scalars): ONE launch (plus the sum launch that follows it in a solve) on
 * caller-supplied HOST arrays, through the launch functions and block-count helpers the solvers call.  Every x-side array
 * (g_*, x_in[], x_out[]) has len_x >= n_x elements of dtype, every y-side one (f_*, y_in[], y_out[]) len_y >= n_y; every
 * array given is uploaded before the launch and every output array downloaded after it, so what the launch does not
 * write comes back as it was.  An array an op does not name may be NULL.  The device's partial-sum buffer starts as NaN
 * (ops that write partials) and is returned whole in `partials` (partials_len doubles, at least what the op writes).
 * `scalars` (64 doubles, in / out) is the device scalar block: slot numbers are those of csrc/vec_kernels.h (Slot).
 * `s0`, `s1`, `rho`, `alpha`, `zs` are cast to dtype.  A sum job is 6 ints {first, nparts, ns, stride, offset, slot}:
 * partial records start at partials[first], the ns sums go to scalars[slot ..].
 *   SCALE_OBJECTIVE  launch_scale_objective: g, scale = x_in[0], mode 1 divide / 0 multiply; a, c, d, e -> x_out[0..4).
 *   PROBE_UNIFORM    probe_uniform(g, n_x): info[0] = mask, info[1] = h; scalars[0..3) = c, d, e.
 *   ADMM_PRE         launch_admm_pre: g, f; x_in = {x_cur, xt}, y_in = {y_cur, yt}; x_out = {x12, xtemp, x_aux or NULL},
 *                    y_out likewise; cg (2 doubles, may be NULL) = cg_reset; cheap 0 / 1 as given (1 is refused when a
 *                    function is outside is_cheap_prox); probe 1: ug / uf from probe_uniform, 0: from u_mask / u_h / u_cde
 *                    ([0] g, [1] f).  partials = [pre_blocks(n_x) + pre_blocks(n_y)][3]; then launch_sum_jobs with the
 *                    two jobs of the dense iteration: scalars[kGapX ..+3) and scalars[kGapY ..+3).
 *                    info = {blocks_x, blocks_y, ug.mask, uf.mask}.
 *   ADMM_TAIL        launch_admm_tail(n_x): x_in = {znew, zprev, z12}, x_out[0] = ztemp (in / out); partials
 *                    [vec_blocks(n_x)][2], summed into scalars[kDXprev2 ..+2).  info[0] = blocks.
 *   UNSCALE          launch_unscale: x_in = {x12, xt, xprev, e}, y_in = {y12, yt, yprev, d}; x_out = {x, mu or NULL},
 *                    y_out = {y, l}.
 *   EXACT_U          launch_exact_u(n_x): x_in = {y12, yt, yprev}, c = s0, u = x_out[0].
 *   SCALE_BY         launch_scale_by: alpha = s0, x_in = {in, sc}, mode 1 divide / 0 multiply, x_out[0].
 *   AXPBY            launch_axpby: a = s0, x = x_in[0], b = s1, y = x_out[0] (in / out).
 *   SCAL, SQRT, FILL launch_scal (alpha = s0), launch_sqrt_inplace, launch_fill (v = s0) on x_out[0].
 *   SUM_JOBS         launch_sum_jobs on the records in `partials` (input), njobs (1 .. 8) jobs.
 *   MAX_PARTIALS     launch_max_partials(partials, partials_len) -> scalars[0].
 *   SUM_CG           launch_sum_cg: jobs[0], scalars, cg (5 doubles, in / out), mode 1 / 2 / 3, shift = s0, eps = s1.
 *   PUBLISH          on a context of the entry's own whose device block starts as `scalars`: njobs jobs are queued, the
 *                    overlay (ov_src, ov_slot, ov_n; ov_src has ov_n[0] + ov_n[1] doubles) is set, fetch_scalars();
 *                    then njobs2 jobs (jobs2) are queued and fetched with no overlay.  mode 0: the polling path, 1: the
 *                    copying path (launch_apply_overlay, then a copy).  pub (4 x 64 doubles) = host block 1, device
 *                    block 1, host block 2, device block 2; info = {counter word after fetch 1, after fetch 2,
 *                    poll_fetch after fetch 1, after fetch 2}.
 * Invalid arguments are refused before any device work: POGS_ERROR, and PogsAmdLastError names the argument. */
enum { POGS_AMD_VEC_SCALE_OBJECTIVE = 0, POGS_AMD_VEC_PROBE_UNIFORM = 1, POGS_AMD_VEC_ADMM_PRE = 2,
       POGS_AMD_VEC_ADMM_TAIL = 3, POGS_AMD_VEC_UNSCALE = 4, POGS_AMD_VEC_EXACT_U = 5, POGS_AMD_VEC_SCALE_BY = 6,
       POGS_AMD_VEC_AXPBY = 7, POGS_AMD_VEC_SCAL = 8, POGS_AMD_VEC_SQRT = 9, POGS_AMD_VEC_FILL = 10,
       POGS_AMD_VEC_SUM_JOBS = 11, POGS_AMD_VEC_MAX_PARTIALS = 12, POGS_AMD_VEC_SUM_CG = 13, POGS_AMD_VEC_PUBLISH = 14 };
#define POGS_AMD_VEC_SCALARS 64
typedef struct PogsAmdVecArgs {
  int dtype, op, mode;
  int n_x, n_y;
  size_t len_x, len_y;
  int cheap, probe;
  int u_mask[2], u_h[2];
  double u_cde[6];
  double rho, alpha, zs, s0, s1;
  const int *g_h;
  const void *g_a, *g_b, *g_c, *g_d, *g_e;
  const int *f_h;
  const void *f_a, *f_b, *f_c, *f_d, *f_e;
  const void *x_in[4], *y_in[4];
  void *x_out[4], *y_out[4];
  double *partials;
  size_t partials_len;
  const int *jobs, *jobs2;
  int njobs, njobs2;
  double *scalars;       /* 64 */
  double *cg;            /* 5 (ADMM_PRE: 2) */
  const double *ov_src;
  int ov_slot[2], ov_n[2];
  double *pub;           /* 4 x 64 */
  int *info;             /* 4 */
} PogsAmdVecArgs;
int PogsAmdVecCheck(const PogsAmdVecArgs *args);
/* The Norm2Est start vector (reference: gsl::rand, src/cpu/include/gsl/gsl_rand.h:8-16). */
int PogsAmdRandUniform(int dtype, size_t n, void *out_host);

#ifdef __cplusplus
}
#endif
#endif /* POGS_AMD_H_ */
