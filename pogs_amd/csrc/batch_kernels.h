// Kernels of the batched solves: multi-vector passes over a stored row-major matrix on the matrix cores (dense batch,
// dense_batch.h), and the element-wise stages and sums of the loop both batches share (batch_admm.h).  Their own
// translation unit (batch_kernels.hip), so that the per-shape code objects of the solo solver stay small.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pogs_amd.h"
#include "common.h"
#include "prox.h"

namespace pogs_amd {

constexpr int kBatchMax = POGS_AMD_BATCH_MAX;

// slot -> problem index of the problems a launch works on (slots >= nact are zero columns)
struct BatchSlots {
  int nact = 0;
  int act[kBatchMax] = {};
};

constexpr int kBRowGroups = 4;
constexpr int kBRowsPerWg = 16 * kBRowGroups;

template <typename T>
struct BatchVecArgs {
  int n, m, bx, by;            // bx, by: vec_blocks(n), vec_blocks(m)
  size_t ldx, ldy;
  const FnView<T> *fg;         // [2 kb]: f of problem p at 2p, g at 2p + 1 (scaled)
  BatchSlots sl;
  T rho[kBatchMax], zs[kBatchMax];   // by problem index
  T alpha;
  const T *x_cur, *y_cur, *xt, *yt;
  T *x12, *y12, *xtemp, *ytemp;
  const T *x_new, *y_new;      // tail / exact stages
  const T *zx, *zy;            // exact stage: A^T u (n), A x12 (m)
  T *u;                        // exact prep: y12 + zs yt - yprev
  double *part;                // [kb][bx + by][ns]
};

// Scalar sums of the problems of the slots: job q (blockIdx.x) adds records [b0, b1) of ns values from
// part[p][nblk][ns] into out[p * kBatchRec + slot .. + ns).  Fixed order: thread stride, then dev::block_sum.
constexpr int kBatchRec = 16;   // doubles per problem in the batch scalar block
struct BatchSumJob {
  const double *part;
  int nblk, ns, b0, b1, slot;
};
struct BatchSumJobs {
  BatchSumJob j[4];
};
// record layout of the batch scalar block (per problem)
enum BatchRec : int { kBrPreX = 0, kBrPreY = 3, kBrTailX = 6, kBrTailY = 8, kBrExS = 10, kBrExR = 11, kBrFval = 12 };

// Y[p][row] = sum_c M[row][c] X[p][c] for the problems p of sl (tri: kFull / kLower / kUpper of stream.h's Tri)
template <typename T>
void launch_batch_rows(int tri, const T *M, size_t ldm, int rows, int cols, int cols_pad, const T *X, size_t ldx, T *Y,
                       size_t ldy, const BatchSlots &sl, hipStream_t s);
// part[rb][p][c] = sum over the rows of row block rb of M[row][c] U[p][row]  (grid: column slabs x nrb row blocks)
template <typename T>
void launch_batch_cols(const T *M, size_t ldm, int rows, int cols_pad, int rows_per_block, int nrb, const T *U,
                       size_t ldu, T *part, int kb, const BatchSlots &sl, hipStream_t s);
// columns per slab of launch_batch_cols
template <typename T>
constexpr int batch_cols_slab() { return 64 / static_cast<int>(sizeof(T)) * 4; }
// Row-block partition of launch_batch_cols over a rows x cols_pad matrix: from the shape only (the same for every k
// and slot).  rpb: rows per block, a multiple of 16; nrb_used: the blocks that hold rows.
template <typename T>
inline void batch_cols_partition(int rows, int cols_pad, int &rpb, int &nrb_used) {
  constexpr int SLAB = batch_cols_slab<T>();
  const int ncs = (cols_pad + SLAB - 1) / SLAB;
  const int nrb = std::max(1, std::min((rows + 63) / 64, (4096 + ncs - 1) / ncs));
  rpb = static_cast<int>(round_up(static_cast<size_t>((rows + nrb - 1) / nrb), 16));
  nrb_used = (rows + rpb - 1) / rpb;
}
// Z[p][c] = sum_rb part[rb][p][c] in row-block order (+ add[p][c]); columns >= cols are zero
template <typename T>
void launch_batch_cols_reduce(const T *part, int nrb, int kb, int cols, int cols_pad, const T *add, T *Z, size_t ldz,
                              const BatchSlots &sl, hipStream_t s);
// Mixed storage (DenseSolver's float copy of A, stream_mixed.h): launch_batch_rows<double>(kFull, ...) and
// launch_batch_cols<double> over a matrix stored as floats, rows of round_up(cols, 4) floats at stride ldm (a multiple
// of 4).  Vectors, partials and arithmetic are fp64, cols_pad = round_up(cols, 2), and the row-block partition is
// batch_cols_partition<double>'s: the results are, bit for bit, those of the fp64 launches on the widened matrix
// (launch_batch_cols_reduce<double> is the second stage of both).
constexpr int kBatchColsMixedSlab = 64;   // columns per slab of launch_batch_cols_mixed
void launch_batch_rows_mixed(const float *M, size_t ldm, int rows, int cols, int cols_pad, const double *X, size_t ldx,
                             double *Y, size_t ldy, const BatchSlots &sl, hipStream_t s);
void launch_batch_cols_mixed(const float *M, size_t ldm, int rows, int cols_pad, int rows_per_block, int nrb,
                             const double *U, size_t ldu, double *part, int kb, const BatchSlots &sl, hipStream_t s);
// element-wise stages over x blocks (vec_blocks(n)) and y blocks (vec_blocks(m)), one grid row per slot
template <typename T> void launch_batch_pre(const BatchVecArgs<T> &a, hipStream_t s);
template <typename T> void launch_batch_tail(const BatchVecArgs<T> &a, hipStream_t s);
template <typename T> void launch_batch_exact_u(const BatchVecArgs<T> &a, hipStream_t s);
template <typename T> void launch_batch_exact(const BatchVecArgs<T> &a, hipStream_t s);
void launch_batch_sums(const BatchSumJobs &jobs, int njobs, const BatchSlots &sl, double *out, hipStream_t s);

// The warm begin of the listed problems (BatchAdmm::warm_begin; pogs.cpp:144-156), around the two products
// zy = A x12, zx = A^T u.  x0 / l0: the caller's start, problem p at p * ldx / p * ldy.  Elements below n / m only:
// the padding of every vector stays zero.
template <typename T>
struct BatchWarmArgs {
  int n, m, bx, by;
  size_t ldx, ldy;
  BatchSlots sl;
  const T *x0, *l0, *d, *e;
  T *x12, *u;                        // scale: x12 = x0 / e, u = l0 / d
  const T *zx, *zy;                  // close: A^T u, A x12
  T *x_cur, *y_cur, *xt, *yt;        // close: x = x12, y = zy, xt = zx * pos, yt = u * neg
  T pos[kBatchMax], neg[kBatchMax];  // T(1) / rho and T(-1) / rho, by problem index
};
template <typename T> void launch_batch_warm_scale(const BatchWarmArgs<T> &a, hipStream_t s);
template <typename T> void launch_batch_warm_close(const BatchWarmArgs<T> &a, hipStream_t s);

// The slots of the diagnostic entries (PogsAmdBatchRowsCheck, ...): k problems, nact of them active, act without
// repeats and inside [0, k).  Throws Error otherwise.
inline BatchSlots checked_batch_slots(int k, const int *act, int nact) {
  POGS_CHECK(k >= 1 && k <= kBatchMax, "k must be in [1, POGS_AMD_BATCH_MAX]");
  POGS_CHECK(nact >= 1 && nact <= k, "nact must be in [1, k]");
  POGS_CHECK(act != nullptr, "null act");
  BatchSlots sl;
  bool seen[kBatchMax] = {};
  for (int q = 0; q < nact; ++q) {
    POGS_CHECK(act[q] >= 0 && act[q] < k, "act entry out of range [0, k)");
    POGS_CHECK(!seen[act[q]], "act entry repeats");
    seen[act[q]] = true;
    sl.act[q] = act[q];
  }
  sl.nact = nact;
  return sl;
}
// Diagnostics behind PogsAmdBatchRowsCheck / PogsAmdBatchColsCheck (HOST arrays; include/pogs_amd.h): argument checks,
// upload, the solver's launches, download.
template <typename T>
void batch_rows_check(int tri, int rows, int cols, const T *M, size_t ldm, int k, const int *act, int nact, const T *X,
                      size_t ldx, T *Y, size_t ldy);
template <typename T>
void batch_cols_check(int rows, int cols, const T *M, size_t ldm, int k, const int *act, int nact, const T *U,
                      size_t ldu, const T *add, T *Z, size_t ldz, int *nrb_used, int *rpb);
// Behind PogsAmdBatchRowsMixedCheck / PogsAmdBatchColsMixedCheck: the same for the mixed launches (M: floats).
void batch_rows_mixed_check(int rows, int cols, const float *M, size_t ldm, int k, const int *act, int nact,
                            const double *X, size_t ldx, double *Y, size_t ldy);
void batch_cols_mixed_check(int rows, int cols, const float *M, size_t ldm, int k, const int *act, int nact,
                            const double *U, size_t ldu, const double *add, double *Z, size_t ldz, int *nrb_used,
                            int *rpb);

}  // namespace pogs_amd
