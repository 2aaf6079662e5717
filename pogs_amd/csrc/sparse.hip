// Sparse graph-form ADMM solver with the CGLS projector and, for a short side (min(m, n) <= POGS_AMD_SPARSE_DIRECT_MAX,
// one GPU), the direct one: I + A^T A (or I + A A^T) formed from the sparse copies, factored and inverted once on the
// matrix cores, applied as two triangular mat-vecs per iteration (sparse_direct.h).
//
// Reference call stack being replaced:
//   PogsSparseD/S -> PogsSparse<T,O> (src/interface_c/pogs_c.cpp:57-108)
//     MatrixSparse::Init/Mul/Equil (src/cpu/matrix/matrix_sparse.cpp:97-302,
//       gsl_spblas.h:10-40, gsl_spmat.h:32-93): CSR plus its transpose, both
//       used as row-gather SpMVs
//     ProjectorCgls::Project (src/cpu/projector/projector_cgls.cpp:52-88)
//       -> cgls::Solve (src/cpu/include/cgls.h:200-323)
//     PogsImplementation::Solve (src/cpu/pogs.cpp:91-581)
//
// HBM layout: two CSR structures (A by rows, A^T by rows; int32 indices) -- kept for GetEquil,
// as the source of the tiled copies and as the fallback (POGS_AMD_SPMV=plain): "row blocks" of
// consecutive rows whose non-zeros fit one LDS tile, streamed with coalesced loads, products
// staged in LDS, rows reduced from there.  The solver itself runs on a tiled sliced-ELL copy of
// each (sell.h): x slices and row sums in LDS, uint16 local columns, no partial-sum traffic.
//
// One translation unit in four files: sparse_kernels.h (row functors, the plain SpMV and its companions),
// sparse_operator.h (SparseOperator<T>: both copies, their build and their products), sparse_direct.h (the direct
// projector's kernels: sparse Gram product, triangular mat-vec) and this one -- SparseSolver<T> (equilibration, norm
// estimate, CGLS, the direct projector's factor and solves, the ADMM iteration, warm start; the solve around them is
// SoloSolver<T>, solo_solver.h),
// PogsAmdSpmvCheck's spmv_check(), which runs one product on a SparseOperator of its own, without a solver, and the
// same for the direct projector's kernels: sparse_gram_check() and tri_matvec_check().
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <limits>
#include <optional>
#include <type_traits>
#include <vector>

#include "batch_admm.h"
#include "cg_fused.h"
#include "cg_kernels.h"
#include "engine.h"
#include "gemm.h"
#include "reduce.h"
#include "sell.h"
#include "solo_solver.h"
#include "sparse_batch_kernels.h"
#include "sparse_direct.h"
#include "sparse_operator.h"
#include "spmv_check.h"
#include "vec_kernels.h"

namespace pogs_amd {

void rand_uniform_host(float *x, size_t n);
void rand_uniform_host(double *x, size_t n);

namespace {

#define POGS_STR2(x) #x
#define POGS_STR(x) POGS_STR2(x)

template <typename T>
class SparseSolver final : public SoloSolver<T> {
  using B = SoloSolver<T>;
  using B::begin_destroy, B::ctx_, B::m_, B::n_, B::multi_, B::d_, B::e_, B::nrmA_, B::x_, B::y_, B::xt_, B::yt_, B::xtemp_,
      B::ytemp_, B::x12_, B::y12_, B::xout_, B::yout_, B::lout_, B::muout_, B::f_, B::g_, B::fs_, B::gs_, B::ctl_, B::loaded_,
      B::cur_, B::zt_scale_, B::pre_cheap_, B::warm_pending_, B::warm_x_, B::warm_l_, B::fview, B::gview, B::alloc_iterate,
      B::load_functions, B::arm_control, B::reset_iterate, B::pre_args, B::advance, B::reduce_y_scalars, B::log_iteration,
      B::collect_timer_head;

 public:
  SparseSolver(int ord, size_t m, size_t n, size_t nnz, const void *data, const int *ptr, const int *ind, int mem,
               const PogsAmdOptions *opt, const PogsAmdDist *dist, bool mixed = false) {
    const double t0 = wall_s();
    // mixed storage (PogsAmdCreateSparseMixed; what it is honoured for is checked in abi.hip before anything is built):
    // the equilibrated values are rounded to float and the tiled copies store them as floats.  POGS_AMD_MIXED_PASS=0
    // keeps the rounding and leaves the tiled values as doubles (the A / B leg, the bit-for-bit yardstick).
    mixed_ = mixed;
    if (mixed_) {
      POGS_CHECK((std::is_same<T, double>::value) && !(dist && dist->world >= 1), "mixed storage needs an fp64 handle on one GPU");
      const char *mp = std::getenv("POGS_AMD_MIXED_PASS");
      mixed_pass_ = !(mp && mp[0] == '0');
    }
    // the direct projector (ProjectorDirect, projector_direct_dense.cpp, on a sparse A): refused before anything is built
    direct_ = opt && opt->projector == POGS_AMD_PROJ_DIRECT;
    if (direct_) {
      POGS_CHECK(!(dist && dist->world >= 1), "the sparse direct projector is single-GPU (the handle would have row shards)");
      POGS_CHECK(std::min(m, n) <= static_cast<size_t>(POGS_AMD_SPARSE_DIRECT_MAX),
                 "the sparse direct projector needs min(m, n) <= POGS_AMD_SPARSE_DIRECT_MAX = "
                 POGS_STR(POGS_AMD_SPARSE_DIRECT_MAX) "; use POGS_AMD_PROJ_CGLS");
    }
    ctx_.init(opt ? opt->device : -1, opt ? opt->profile : 0);
    POGS_CHECK(m > 0 && n > 0 && m < (1u << 31) && n < (1u << 31) && nnz < (1ull << 31), "bad dimensions");
    m_ = static_cast<int>(m);
    n_ = static_cast<int>(n);
    nnz_ = nnz;
    // row shards: this rank holds m consecutive rows as CSR; y-sized
    // state is local, x-sized state replicated, A^T products and row sums are all-reduced
    if (dist && dist->world >= 1) {
      POGS_CHECK(ord == ROW_MAJ, "a row shard must be given as CSR (ROW_MAJ)");
      ctx_.dist.init(dist->rank, dist->world, dist->unique_id);
      ctx_.m_global = dist->m_global;
    } else {
      ctx_.m_global = m;
    }
    multi_ = ctx_.dist.active();
    op_.emplace(ctx_, ord, m_, n_, nnz_, data, ptr, ind, mem);
    ctx_.stats.t_h2d_s = wall_s() - t0;
    alloc_state();
    op_->print_stamps();
    equilibrate();
    norm_est();
    if (direct_) factor_direct();
    ctx_.sync();
    ctx_.stats.t_init_s = wall_s() - t0;
  }

  ~SparseSolver() override { begin_destroy(ctx_); }

  // k problems on the handle's matrix, every product with A / A^T shared (the loop: batch_admm.h; the
  // products and the batched CGLS: sparse_batch.h); w: the members that start warm, cold by default
  void solve_batch_sparse(int kb, const FnHost *f, const FnHost *g, const double *rho0, const SolveParams &p,
                          const BatchOut &out, const BatchWarm &w) override;
  void solve_batch_any(int kb, const FnHost *f, const FnHost *g, const double *rho0, const SolveParams &p,
                       const BatchOut &out, const BatchWarm &w) override {
    solve_batch_sparse(kb, f, g, rho0, p, out, w);
  }

  void get_equil(void *A_eq, void *d, void *e, double *nrmA) override {
    ctx_.sync();
    // A_eq: the equilibrated CSR values of the first copy, length nnz
    if (A_eq) POGS_HIP_CHECK(hipMemcpy(A_eq, op_->A().val.p, nnz_ * sizeof(T), hipMemcpyDeviceToHost));
    if (d) POGS_HIP_CHECK(hipMemcpy(d, d_.p, m_ * sizeof(T), hipMemcpyDeviceToHost));
    if (e) POGS_HIP_CHECK(hipMemcpy(e, e_.p, n_ * sizeof(T), hipMemcpyDeviceToHost));
    if (nrmA) *nrmA = nrmA_;
  }

  // W = L^-1 and U = W^T of a direct handle: K x K row-major on the host, K = min(m, n)
  void get_factor(void *W, void *U) override {
    if (!direct_) SolverBase::get_factor(W, U);
    ctx_.sync();
    const size_t row = static_cast<size_t>(k_) * sizeof(T), pitch = kld_ * sizeof(T);
    if (W) POGS_HIP_CHECK(hipMemcpy2D(W, row, Wp_, pitch, row, k_, hipMemcpyDeviceToHost));
    if (U) POGS_HIP_CHECK(hipMemcpy2D(U, row, Up_, pitch, row, k_, hipMemcpyDeviceToHost));
  }

  void project(const void *x0, const void *y0, double tol, void *x, void *y) override {
    hipStream_t s = ctx_.stream;
    POGS_HIP_CHECK(hipMemcpyAsync(xtemp_.p, x0, n_ * sizeof(T), hipMemcpyHostToDevice, s));
    POGS_HIP_CHECK(hipMemcpyAsync(ytemp_.p, y0, m_ * sizeof(T), hipMemcpyHostToDevice, s));
    if (direct_) {
      // exact: tol is not used
      direct_project_x(xtemp_.p, ytemp_.p, x_[1].p, false);
      if (tall_) {
        spmv<false>(op_->A(), x_[1].p, nullptr, SpAxpbyOp<T>{1, 0, nullptr, y_[1].p}, nullptr);
      } else {
        launch_axpby<T>(m_, static_cast<T>(1), ytemp_.p, static_cast<T>(0), y_[1].p, s);   // y = y0 + t
        launch_axpby<T>(m_, static_cast<T>(1), dr_.p, static_cast<T>(1), y_[1].p, s);
      }
    } else {
    x_[1].zero(s);  // cold start: x = 0
    cgls_project(xtemp_.p, ytemp_.p, x_[1].p, static_cast<T>(tol));
    spmv<false>(op_->A(), x_[1].p, nullptr, SpAxpbyOp<T>{1, 0, nullptr, y_[1].p}, nullptr);
    }
    POGS_HIP_CHECK(hipMemcpyAsync(x, x_[1].p, n_ * sizeof(T), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipMemcpyAsync(y, y_[1].p, m_ * sizeof(T), hipMemcpyDeviceToHost, s));
    ctx_.sync();
  }

  // PogsAmdSparseCgCheck: one projection on given vectors, by cg_loop_fused (loop 0) or cgls_project (1 warm, 2 cold)
  // with the launches iteration() puts around it, minus the prox step
  void sparse_cg_check(const SparseCgCheckArgs &a) override {
    POGS_CHECK(!multi_, "PogsAmdSparseCgCheck: a row-sharded handle is not supported");
    POGS_CHECK(!direct_, "PogsAmdSparseCgCheck: the handle runs the direct projector (no CGLS loop to check)");
    if (a.loop == 0) {
      POGS_CHECK(op_->A().sell_ready && op_->At().sell_ready,
                 "PogsAmdSparseCgCheck: the device-resident loop needs both copies tiled");
      POGS_CHECK(fused_cg_, "PogsAmdSparseCgCheck: the handle does not run the device-resident loop");
    }
    hipStream_t s = ctx_.stream;
    ctx_.sync();
    const PogsAmdStats stats0 = ctx_.stats;
    const int pred0 = cg_pred_;
    const unsigned long long timed0 = timed_spmvs_;
    double *S = ctx_.S.p;
    const int nw = cur_ ^ 1;
    T *x = x_[nw].p, *xw = xout_.p;   // (xout_: free between solves)
    double *rec_x = ctx_.spart.p + sp_cgx_off_;
    auto up = [&](T *dst, const void *src, int cnt) {
      POGS_HIP_CHECK(hipMemcpyAsync(dst, src, static_cast<size_t>(cnt) * sizeof(T), hipMemcpyHostToDevice, s));
    };
    auto down = [&](void *dst, const T *src, int cnt) {
      POGS_HIP_CHECK(hipMemcpyAsync(dst, src, static_cast<size_t>(cnt) * sizeof(T), hipMemcpyDeviceToHost, s));
    };
    up(xtemp_.p, a.x0, n_); up(ytemp_.p, a.y0, m_); up(xw, a.x_warm, n_); up(y_[cur_].p, a.y_warm, m_);
    up(x_[cur_].p, a.x_prev, n_); up(x12_.p, a.x12, n_); up(y12_.p, a.y12, m_);
    int enq = 0;
    if (a.loop == 0) {
      // what admm_pre_kernel leaves: r = y0 - y_warm, x = x_warm - x0, the done flag and the step count cleared
      hipLaunchKernelGGL(sub_norm_kernel<T>, dim3(vec_blocks(m_)), dim3(kVecTpb), 0, s, m_, ytemp_.p, y_[cur_].p, cg_r_.p,
                         ctx_.spart.p);
      hipLaunchKernelGGL(sub_norm_kernel<T>, dim3(vec_blocks(n_)), dim3(kVecTpb), 0, s, n_, xw, xtemp_.p, x, ctx_.spart.p);
      static_assert(kFcSteps == kFcDone + 1, "slot order");
      POGS_HIP_CHECK(hipMemsetAsync(S + kFcDone, 0, 2 * sizeof(double), s));
      launch_fill<double>(rec_x, std::numeric_limits<double>::quiet_NaN(), kCgfBlocks, s);
      cg_loop_fused(x, nw, a.ysync != 0, a.ahead, a.max_steps, a.tol, nullptr, &enq);
    } else {
      const unsigned long long cg0 = ctx_.stats.cg_iters;
      if (a.loop == 1) {
        cgls_project(xtemp_.p, ytemp_.p, x, static_cast<T>(a.tol), y_[cur_].p, xw);
      } else {
        POGS_HIP_CHECK(hipMemcpyAsync(x, xw, n_ * sizeof(T), hipMemcpyDeviceToDevice, s));
        cgls_project(xtemp_.p, ytemp_.p, x, static_cast<T>(a.tol));
      }
      spmv<false>(op_->A(), x, nullptr, SpTailOp<T>{y_[nw].p, y_[cur_].p, y12_.p, ytemp_.p}, S + kDYprev2, true);
      launch_admm_tail<T>(n_, x, x_[cur_].p, x12_.p, xtemp_.p, ctx_.spart.p, s);
      ctx_.queue_sum(SumJob{ctx_.spart.p, vec_blocks(n_), 2, S + kDXprev2});
      ctx_.fetch_scalars();
      enq = static_cast<int>(ctx_.stats.cg_iters - cg0);
    }
    POGS_HIP_CHECK(hipGetLastError());
    down(a.x, x, n_); down(a.y_new, y_[nw].p, m_); down(a.xtemp, xtemp_.p, n_); down(a.ytemp, ytemp_.p, m_);
    down(a.r, cg_r_.p, m_); down(a.p, cg_p_.p, n_); down(a.s, cg_s_.p, n_);
    double hS[kNumSlots];
    POGS_HIP_CHECK(hipMemcpyAsync(hS, S, kNumSlots * sizeof(double), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipMemcpyAsync(a.rec_x, rec_x, kCgfBlocks * sizeof(double), hipMemcpyDeviceToHost, s));
    ctx_.sync();
    int k = 0;
    for (int slot = kFcDone; slot <= kFcIndef; ++slot) a.slots[k++] = hS[slot];
    for (int slot : {kCgQ2, kCgP2, kCgS2, kCgX2, kDXprev2, kDX12, kDYprev2, kDY12}) a.slots[k++] = hS[slot];
    for (int c = 0; c < 2; ++c) op_->describe(c, a.info + 8 * c);
    *a.enqueued = enq;
    // the handle as it was, for the next solve: the prediction, the counters, no timed launch kept; the vectors of a
    // run in progress (PogsAmdBeginRun / PogsAmdIterate) are gone
    ctx_.stats = stats0;
    cg_pred_ = pred0;
    timed_spmvs_ = timed0;
    if (ctx_.stream_timer.enabled()) {
      unsigned long long cnt = 0;
      (void)ctx_.stream_timer.collect_ms(&cnt);
    }
    loaded_ = false;
  }

  void mul(char trans, double alpha, const void *x, double beta, void *y) override {
    hipStream_t s = ctx_.stream;
    const bool tr = (trans == 't' || trans == 'T');
    const int nin = tr ? m_ : n_, nout = tr ? n_ : m_;
    DevBuf<T> vin(nin), vout(nout);
    POGS_HIP_CHECK(hipMemcpyAsync(vin.p, x, nin * sizeof(T), hipMemcpyHostToDevice, s));
    POGS_HIP_CHECK(hipMemcpyAsync(vout.p, y, nout * sizeof(T), hipMemcpyHostToDevice, s));
    const SpAxpbyOp<T> op{static_cast<T>(alpha), static_cast<T>(beta), vout.p, vout.p};
    if (tr) spmv_t<false>(vin.p, op, nullptr);   // summed over the row shards
    else spmv<false>(op_->A(), vin.p, nullptr, op, nullptr);
    POGS_HIP_CHECK(hipMemcpyAsync(y, vout.p, nout * sizeof(T), hipMemcpyDeviceToHost, s));
    ctx_.sync();
  }

 private:
  void alloc_state() {
    hipStream_t s = ctx_.stream;
    alloc_iterate(n_, m_);
    cg_p_.alloc(n_); cg_s_.alloc(n_); cg_q_.alloc(m_); cg_r_.alloc(m_); cg_b_.alloc(m_); u_.alloc(m_);
    cg_.alloc(kCgNumSlots);
    cg_.zero(s);
    if (multi_) { tsum_.alloc(n_); cg_u_.alloc(n_); cg_u_.zero(s); tsum_.zero(s); }
    const size_t vb = vec_blocks(n_) + vec_blocks(m_);
    const size_t sg = op_->partials_needed();
    const DevCsr<T> &A = op_->A(), &At = op_->At();
    // [SpMV / vector-kernel partials | |x|^2 partials of a CG step | |p|^2 partials]: the last two
    // are summed by the launch that publishes the scalars, so they keep regions of their own
    sp_cgx_off_ = std::max<size_t>(sg * 4 + 64, vb * 3 + 64);
    const size_t cgreg = static_cast<size_t>(std::max(vec_blocks(n_), kCgfBlocks)) + 8;   // (cg_fused.h: up to kCgfBlocks records)
    sp_cgp_off_ = sp_cgx_off_ + cgreg;
    sp_pre_off_ = sp_cgp_off_ + cgreg;   // prox-step sums (deferred on one GPU)
    ctx_.ensure_spart(sp_pre_off_ + vb * 3 + 8);
    // device-resident CGLS loop (cg_fused.h): both copies in the tiled layout; POGS_AMD_CG=h keeps
    // round 2's host-polled loop (cgls_project), which is also what the plain-CSR fallback runs
    const char *cg_env = std::getenv("POGS_AMD_CG");
    fused_cg_ = !direct_ && A.sell_ready && At.sell_ready && !(cg_env && cg_env[0] == 'h') && ctx_.poll_fetch;
    if (multi_) {
      // every rank must take the same path (the collectives of the two loops differ): all or none
      DevBuf<double> flag(1);
      const double mine = fused_cg_ ? 0.0 : 1.0;
      POGS_HIP_CHECK(hipMemcpyAsync(flag.p, &mine, sizeof(double), hipMemcpyHostToDevice, s));
      ctx_.dist.allreduce(flag.p, 1, s);
      double any = 0;
      POGS_HIP_CHECK(hipMemcpyAsync(&any, flag.p, sizeof(double), hipMemcpyDeviceToHost, s));
      POGS_HIP_CHECK(hipStreamSynchronize(s));
      if (any != 0.0) fused_cg_ = false;
    }
    if (fused_cg_) {
      // scalar records of the loop's products: one region for A^T products, one for A products
      cg_rec_cap_ = static_cast<size_t>(std::max({A.nrr * A.ncg, At.nrr * At.ncg, kCgfBlocks})) * 2;
      if (multi_) {
        // row shards: the |q|^2 records of the ranks are summed record by record (one all-reduce of the
        // record array, no folding launch), so the ranks agree on its length -- the largest -- and a
        // rank's unused tail stays zero; the sums land in a third region
        DevBuf<double> caps(static_cast<size_t>(ctx_.dist.world()));
        caps.zero(s);
        const double mine = static_cast<double>(cg_rec_cap_);
        POGS_HIP_CHECK(hipMemcpyAsync(caps.p + ctx_.dist.rank(), &mine, sizeof(double), hipMemcpyHostToDevice, s));
        ctx_.dist.allreduce(caps.p, caps.n, s);
        std::vector<double> all(caps.n);
        POGS_HIP_CHECK(hipMemcpyAsync(all.data(), caps.p, caps.n * sizeof(double), hipMemcpyDeviceToHost, s));
        POGS_HIP_CHECK(hipStreamSynchronize(s));
        for (double v : all) cg_rec_cap_ = std::max(cg_rec_cap_, static_cast<size_t>(v));
      }
      cg_rec_.alloc(cg_rec_cap_ * (multi_ ? 4 : 2));   // row shards: + the summed |q|^2 records, + |s|^2 records of U1
      cg_rec_.zero(s);
      const char *ys = std::getenv("POGS_AMD_YSYNC");
      if (ys) ysync_ = std::max(0, std::atoi(ys));
    }
  }

  // the operator's product on copy M, with the CGLS scalar block bound; a timed one counts as a matvec of the solve
  template <bool SQ, typename Op>
  void spmv(const DevCsr<T> &M, const T *x, const double *x_nrm2, const Op &op, double *scalar_out, bool timed = false,
            int cg_mode = 0) {
    op_->template spmv<SQ>(M, x, x_nrm2, op, scalar_out, timed, cg_mode, cg_.p);
    if (timed) ++timed_spmvs_;
  }
  // A^T product: with row shards the n partial sums are all-reduced before the row functor runs
  template <bool SQ, typename Op>
  void spmv_t(const T *xin, const Op &op, double *scalar_out, bool timed = false, int cg_mode = 0) {
    if (!multi_) {
      spmv<SQ>(op_->At(), xin, nullptr, op, scalar_out, timed, cg_mode);
      return;
    }
    hipStream_t s = ctx_.stream;
    spmv<SQ>(op_->At(), xin, nullptr, SpAxpbyOp<T>{1, 0, nullptr, tsum_.p}, nullptr, timed);
    ctx_.dist.allreduce(tsum_.p, n_, s);
    const int grid = std::max(1, std::min((n_ + 255) / 256, op_->grid_cap()));
    hipLaunchKernelGGL((apply_rows_kernel<T, Op>), dim3(grid), dim3(256), 0, s, tsum_.p, n_, op, ctx_.spart.p);
    if (Op::NS > 0 && scalar_out) {
      SumJob j{ctx_.spart.p, grid, Op::NS, scalar_out};
      launch_sum_jobs(&j, 1, s);
    }
  }

  // MatrixSparse::Equil (matrix_sparse.cpp:158-242): Sinkhorn-Knopp on the squared
  // entries (squared on the fly), D A E on both copies, Frobenius norm of the first.
  void equilibrate() {
    hipStream_t s = ctx_.stream;
    PhaseTimer pt(s);
    const double mg = static_cast<double>(ctx_.m_global), nn = n_;
    const T ce = static_cast<T>(1e-4) * static_cast<T>(mg + nn) / static_cast<T>(mg);
    const T cd = static_cast<T>(1e-4) * static_cast<T>(mg + nn) / static_cast<T>(nn);
    launch_fill<T>(d_.p, static_cast<T>(1), m_, s);
    launch_fill<T>(e_.p, static_cast<T>(1), n_, s);
    // 50 iterations in the reference (equil_helper.h:147).  As in DenseSolver::equilibrate (fp32):
    // once an iteration changes every entry of e (replicated, so the ranks of a sharded solve
    // agree) by one common ratio 1 + gamma -- the slow drift of the common factor (d * a, e / a)
    // -- the loop ends after its d update and the remaining iterations are applied in closed
    // form.  POGS_AMD_SK_FULL=1: all 50.
    const char *sk_env = std::getenv("POGS_AMD_SK_FULL");
    const bool sk_probe = std::is_same<T, float>::value && !(sk_env && sk_env[0] == '1');
    double *mark = sk_probe ? ctx_.S.p + kSkMark : nullptr;
    const T sk_tol = 16 * std::numeric_limits<T>::epsilon();
    double r_ref = 0, gamma = 0;
    bool extrapolate = false;
    int k = 0;
    while (k < 50) {
      spmv_t<true>(d_.p, SpSkOp<T>{static_cast<T>(mg), ce, e_.p, mark, k + 1.0, sk_tol, static_cast<T>(r_ref)},
                   ctx_.S.p + kSkRatio);
      spmv<true>(op_->A(), e_.p, nullptr, SpSkOp<T>{static_cast<T>(nn), cd, d_.p}, nullptr);
      ++k;
      if (mark && k >= 2) {
        const double *S = ctx_.fetch_scalars();
        const double r_mean = S[kSkRatio] / n_;
        const bool uniform = k >= 3 && S[kSkMark] < static_cast<double>(k) && r_mean > 0.5 && r_mean < 2.0;
        r_ref = r_mean;
        gamma = r_mean - 1.0;
        if (uniform) { extrapolate = true; break; }
      }
    }
    if (extrapolate) {
      // state (e_{k-1}, d_k) after k iterations; the reference ends with (e_49, d_50)
      const double f = std::pow(1.0 + gamma, 50 - k);
      launch_scal<T>(e_.p, static_cast<T>(f), n_, s);
      launch_scal<T>(d_.p, static_cast<T>(1.0 / f), m_, s);
    }
    ctx_.stats.matvecs_init += 2 * k;
    launch_sqrt_inplace<T>(d_.p, m_, s);
    launch_sqrt_inplace<T>(e_.p, n_, s);
    const int g = op_->grid_cap();
    double *pa = ctx_.spart.p, *pb = ctx_.spart.p + g;
    op_->scale(d_.p, e_.p, pa, pb);
    SumJob j{op_->first_is_A() ? pa : pb, g, 1, ctx_.S.p + kFro2};   // first nnz only (matrix_sparse.cpp:257)
    launch_sum_jobs(&j, 1, s);
    reduce_y_scalars(ctx_.S.p + kFro2, 1);
    const double *S = ctx_.fetch_scalars();
    const T normA = static_cast<T>(std::sqrt(S[kFro2])) /
                    static_cast<T>(std::sqrt(std::min(mg, nn)));
    op_->scal(static_cast<T>(1) / normA);
    // mixed storage: from here on the matrix is the rounded one -- norm estimate, Gram matrix and factor, every product
    // (d, e are those of the equilibration as it ran)
    if (mixed_) op_->round_values();
    op_->finalize_values(mixed_ && mixed_pass_);
    const T invs = static_cast<T>(1) / std::sqrt(normA);
    launch_scal<T>(d_.p, invs, m_, s);
    launch_scal<T>(e_.p, invs, n_, s);
    ctx_.stats.equil_ms = pt.stop_ms();
  }

  // Norm2Est (equil_helper.h:107-135)
  void norm_est() {
    hipStream_t s = ctx_.stream;
    PhaseTimer pt(s);
    std::vector<T> x0(n_);
    rand_uniform_host(x0.data(), n_);
    POGS_HIP_CHECK(hipMemcpyAsync(xtemp_.p, x0.data(), n_ * sizeof(T), hipMemcpyHostToDevice, s));
    ctx_.sync();
    const T kTol = static_cast<T>(1e-4);
    T norm_est = 0, last;
    unsigned i = 0;
    for (i = 0; i < 50; ++i) {
      last = norm_est;
      // Sx = A (x / |x|);  x' = A^T Sx
      spmv<false>(op_->A(), xtemp_.p, (i == 0) ? nullptr : ctx_.S.p + kPowX2,
                  SpAxpbyNormOp<T>{1, 0, nullptr, cg_q_.p}, ctx_.S.p + kPowSx2);
      reduce_y_scalars(ctx_.S.p + kPowSx2, 1);
      spmv_t<false>(cg_q_.p, SpAxpbyNormOp<T>{1, 0, nullptr, xtemp_.p}, ctx_.S.p + kPowX2);
      const double *S = ctx_.fetch_scalars();
      const T normx = static_cast<T>(std::sqrt(S[kPowX2]));
      const T normSx = static_cast<T>(std::sqrt(S[kPowSx2]));
      norm_est = normx / normSx;
      ctx_.stats.matvecs_init += 2;
      if (std::abs(last - norm_est) < kTol * norm_est) { ++i; break; }
    }
    nrmA_ = norm_est;
    ctx_.stats.nrmA = nrmA_;
    ctx_.stats.norm_est_iters = i;
    xtemp_.zero(s);
    ctx_.stats.normest_ms = pt.stop_ms();
  }

  // ---- direct projector -------------------------------------------------------
  // ProjectorDirect::Init and the first-call factorisation (projector_direct_dense.cpp:45-84, 116-121; s = 1 always):
  // G = A^T A (m > n) or A A^T from the equilibrated copies (sparse_direct.h), L L^T = G + I, W = L^-1, U = W^T
  // (gemm.h).  W and U stay; G / L and the scratch slab go back to the pool.
  void factor_direct() {
    hipStream_t s = ctx_.stream;
    tall_ = m_ > n_;
    k_ = std::min(m_, n_);
    kld_ = round_up(static_cast<size_t>(k_), Vec16<T>::N);
    const size_t slab = static_cast<size_t>(k_) * kld_;
    fac_.alloc(slab * 2);
    fac_.zero(s);
    Wp_ = fac_.p;
    Up_ = fac_.p + slab;
    dr_.alloc(kld_); dt_.alloc(kld_);
    dr_.zero(s); dt_.zero(s);
    std::optional<DevicePool::QuiescedScope> drained;   // from the sync on: the work slabs go back as idle
    DevBuf<T> work(slab * 2);
    work.zero(s);
    T *G = work.p, *tmp = work.p + slab;
    {
      PhaseTimer pt(s);
      const DevCsr<T> &O = tall_ ? op_->At() : op_->A(), &I = tall_ ? op_->A() : op_->At();
      launch_sparse_gram<T>(SparseGramArgs<T>{O.val.p, O.ind.p, O.ptr.p, I.val.p, I.ind.p, I.ptr.p, k_, 0, G, kld_},
                            ctx_.num_cu, s);
      POGS_HIP_CHECK(hipGetLastError());
      ctx_.stats.gram_ms = pt.stop_ms();
    }
    launch_add_diag<T>(G, kld_, k_, static_cast<T>(1), s);                // projector_direct_dense.cpp:118-119
    {
      PhaseTimer pt(s);
      cholesky_lower<T>(G, kld_, k_, Wp_, kld_, s);
      ctx_.stats.chol_ms = pt.stop_ms();
    }
    {
      PhaseTimer pt(s);
      trtri_lower<T>(G, kld_, k_, Wp_, kld_, tmp, s);
      launch_transpose<T>(Wp_, kld_, k_, k_, Up_, kld_, s);
      ctx_.stats.trtri_ms = pt.stop_ms();
    }
    POGS_HIP_CHECK(hipGetLastError());
    ctx_.sync();
    drained.emplace();
  }

  // out = U (W rhs): the two triangular products that replace linalg_cholesky_svx (gsl_linalg.h:57-61); out may be rhs
  void direct_solve(const T *rhs, T *out) {
    launch_tri_matvec<T>(kTriLower, Wp_, kld_, k_, rhs, dt_.p, ctx_.stream);
    launch_tri_matvec<T>(kTriUpper, Up_, kld_, k_, dt_.p, out, ctx_.stream);
  }

  // ProjectorDirect::Project up to the y half (projector_direct_dense.cpp:122-135): the projected x from (x0, y0).
  //   m > n:   x = (I + A^T A)^-1 (x0 + A^T y0); the caller forms y = A x
  //   m <= n:  t = (I + A A^T)^-1 (A x0 - y0), x = x0 - A^T t; t is left in dr_ and the caller forms y = y0 + t
  void direct_project_x(const T *x0, const T *y0, T *x, bool timed) {
    if (tall_) {
      spmv_t<false>(y0, SpAxpbyOp<T>{1, 1, x0, dr_.p}, nullptr, timed);
      direct_solve(dr_.p, x);
    } else {
      spmv<false>(op_->A(), x0, nullptr, SpAxpbyOp<T>{1, static_cast<T>(-1), y0, dr_.p}, nullptr, timed);
      direct_solve(dr_.p, dr_.p);
      spmv_t<false>(dr_.p, SpAxpbyOp<T>{static_cast<T>(-1), 1, x0, x}, nullptr, timed);
    }
  }

  // ---- per solve: the hooks of SoloSolver<T> ----------------------------------
  void load_problem(const FnHost &f, const FnHost &g, const SolveParams &p) override {
    load_functions(f, g);
    // coefficient arrays that hold one value throughout (a lasso: h, c, d, e of both halves) are not streamed by the
    // prox step: 16 of its 44 bytes per element
    uni_f_ = probe_uniform<T>(fview(), m_, ctx_.stream);
    uni_g_ = probe_uniform<T>(gview(), n_, ctx_.stream);
    arm_control(p);
  }

  void cold_start() override {
    reset_iterate();
    proj_count_ = 0;
    cg_pred_ = 1;
  }

  void sum_vec_partials(int blocks, double *out) {
    SumJob j{ctx_.spart.p, blocks, 1, out};
    launch_sum_jobs(&j, 1, ctx_.stream);
  }

  // ProjectorCgls::Project up to (not including) the final y = A x
  // (projector_cgls.cpp:59-75): x holds the warm start on entry, the projected x
  // on exit.
  // `Ax_warm` (optional): A times the warm-start x, if the caller already has it.  The
  // reference forms b = y0 - A x0 and r = b - A (x - x0) with two SpMVs (:65-68,
  // cgls.h:226-233); their sum is r = y0 - A x_warm, and inside the ADMM loop A x_warm is the
  // previous iteration's y (the projection always ends with y = A x), so both SpMVs vanish.
  // `x_warm` (with Ax_warm): where the warm start is read from -- x itself by default; the ADMM
  // loop passes the previous iterate, which saves the 2 MB device-to-device copy into x per
  // iteration (30 us at C4 through the runtime's blit kernel).
  void cgls_project(const T *x0, const T *y0, T *x, T tol, const T *Ax_warm = nullptr, const T *x_warm = nullptr) {
    hipStream_t s = ctx_.stream;
    const int bx = vec_blocks(n_);
    const double shift = 1.0;
    const double kEps = std::numeric_limits<T>::epsilon();
    if (Ax_warm) {
      // r = y0 - A x_warm ; x <- x - x0                                       (:62)
      hipLaunchKernelGGL(sub_norm_kernel<T>, dim3(vec_blocks(m_)), dim3(kVecTpb), 0, s, m_, y0, Ax_warm, cg_r_.p,
                         ctx_.spart.p);
      hipLaunchKernelGGL(sub_norm_kernel<T>, dim3(bx), dim3(kVecTpb), 0, s, n_, x_warm ? x_warm : x, x0, x, ctx_.spart.p);
    } else {
      // x <- x - x0, |x|^2                                                    (:62)
      hipLaunchKernelGGL(sub_norm_kernel<T>, dim3(bx), dim3(kVecTpb), 0, s, n_, x, x0, x, ctx_.spart.p);
      sum_vec_partials(bx, ctx_.S.p + kCgX2);
      // b = y0 - A x0                                                         (:65-68)
      spmv<false>(op_->A(), x0, nullptr, SpAxpbyOp<T>{static_cast<T>(-1), static_cast<T>(1), y0, cg_b_.p}, nullptr, true);
      const double *S0 = ctx_.fetch_scalars();
      // r = b - A x (only if x != 0)                                          (cgls.h:226-233)
      if (std::sqrt(S0[kCgX2]) > 0.0) {
        spmv<false>(op_->A(), x, nullptr, SpAxpbyOp<T>{static_cast<T>(-1), static_cast<T>(1), cg_b_.p, cg_r_.p}, nullptr,
                    true);
      } else {
        POGS_HIP_CHECK(hipMemcpyAsync(cg_r_.p, cg_b_.p, m_ * sizeof(T), hipMemcpyDeviceToDevice, s));
      }
    }
    const double *S;
    double normx;
    // Single GPU: the scalar sum after an SpMV and the one-thread CGLS update that consumes it are
    // one launch (launch_sum_cg), and |x|^2, |p|^2 -- needed by the host only -- are summed by the
    // launch that publishes the scalar block: 9 launches per CG step instead of 13.
    const bool fuse = !multi_;
    double *px = ctx_.spart.p + sp_cgx_off_, *pp = ctx_.spart.p + sp_cgp_off_;
    // s = A^T r - shift x ; p = s ; gamma = |s|^2                             (cgls.h:236-245)
    spmv_t<false>(cg_r_.p, SpAxpbyNormOp<T>{1, static_cast<T>(-shift), x, cg_s_.p}, ctx_.S.p + kCgS2, true, fuse ? 3 : 0);
    if (!fuse) hipLaunchKernelGGL(set_gamma_kernel, dim3(1), dim3(1), 0, s, ctx_.S.p, cg_.p);
    hipLaunchKernelGGL(cg_update_p_kernel<T>, dim3(bx), dim3(kVecTpb), 0, s, n_, cg_.p, cg_s_.p, cg_p_.p,
                       fuse ? pp : ctx_.spart.p, true);
    if (fuse) ctx_.queue_sum(SumJob{pp, bx, 1, ctx_.S.p + kCgP2});
    else sum_vec_partials(bx, ctx_.S.p + kCgP2);
    S = ctx_.fetch_scalars();
    const double norms0 = std::sqrt(S[kCgS2]);
    double norms = norms0;
    const int maxit = (norms < kEps) ? 0 : 500;                               // flag 1 / projector_cgls.cpp:17
    for (int k = 0; k < maxit; ++k) {
      // q = A p, |q|^2 ; alpha                                               (cgls.h:257-271)
      spmv<false>(op_->A(), cg_p_.p, nullptr, SpAxpbyNormOp<T>{1, 0, nullptr, cg_q_.p}, ctx_.S.p + kCgQ2, true, fuse ? 1 : 0);
      if (!fuse) {
        reduce_y_scalars(ctx_.S.p + kCgQ2, 1);
        hipLaunchKernelGGL(cg_alpha_kernel, dim3(1), dim3(1), 0, s, ctx_.S.p, cg_.p, shift, kEps);
      }
      // x += alpha p ; r -= alpha q ; |x|^2                                  (:274-277)
      const int bm = vec_blocks(m_);
      hipLaunchKernelGGL(cg_update_xr_kernel<T>, dim3(bx + bm), dim3(kVecTpb), 0, s, n_, m_, cg_.p, cg_p_.p, x,
                         cg_q_.p, cg_r_.p, fuse ? px : ctx_.spart.p, bx, static_cast<const T *>(nullptr),
                         static_cast<T *>(nullptr));
      if (fuse) ctx_.queue_sum(SumJob{px, bx, 1, ctx_.S.p + kCgX2});
      else sum_vec_partials(bx, ctx_.S.p + kCgX2);
      // s = A^T r - shift x ; |s|^2 ; beta ; p = s + beta p ; |p|^2          (:281-296)
      spmv_t<false>(cg_r_.p, SpAxpbyNormOp<T>{1, static_cast<T>(-shift), x, cg_s_.p}, ctx_.S.p + kCgS2, true, fuse ? 2 : 0);
      if (!fuse) hipLaunchKernelGGL(cg_beta_kernel, dim3(1), dim3(1), 0, s, ctx_.S.p, cg_.p);
      hipLaunchKernelGGL(cg_update_p_kernel<T>, dim3(bx), dim3(kVecTpb), 0, s, n_, cg_.p, cg_s_.p, cg_p_.p,
                         fuse ? pp : ctx_.spart.p, false);
      if (fuse) ctx_.queue_sum(SumJob{pp, bx, 1, ctx_.S.p + kCgP2});
      else sum_vec_partials(bx, ctx_.S.p + kCgP2);
      S = ctx_.fetch_scalars();
      norms = std::sqrt(S[kCgS2]);
      normx = std::sqrt(S[kCgX2]);
      ++ctx_.stats.cg_iters;
      const bool converged = (norms <= norms0 * static_cast<double>(tol)) || (normx * static_cast<double>(tol) >= 1.0);
      if (converged) break;                                                   // :301-305
    }
    // x <- x + x0                                                            (projector_cgls.cpp:75)
    launch_axpby<T>(n_, static_cast<T>(1), x0, static_cast<T>(1), x, s);
  }

  void apply_warm_start() override {
    if (!warm_pending_) return;
    warm_pending_ = false;
    hipStream_t s = ctx_.stream;
    const T rho = ctl_.rho;
    POGS_HIP_CHECK(hipMemcpyAsync(xtemp_.p, warm_x_.data(), n_ * sizeof(T), hipMemcpyHostToDevice, s));
    POGS_HIP_CHECK(hipMemcpyAsync(ytemp_.p, warm_l_.data(), m_ * sizeof(T), hipMemcpyHostToDevice, s));
    launch_scale_by<T>(n_, static_cast<T>(1), xtemp_.p, e_.p, true, x_[cur_].p, s);
    spmv<false>(op_->A(), x_[cur_].p, nullptr, SpAxpbyOp<T>{1, 0, nullptr, y_[cur_].p}, nullptr);
    launch_scale_by<T>(m_, static_cast<T>(1), ytemp_.p, d_.p, true, yt_.p, s);
    spmv_t<false>(yt_.p, SpAxpbyOp<T>{static_cast<T>(1) / rho, 0, nullptr, xt_.p}, nullptr);
    launch_scal<T>(yt_.p, static_cast<T>(-1) / rho, m_, s);
    ctx_.sync();
    xtemp_.zero(s);
    ytemp_.zero(s);
  }

  // The prox step and the projection of one iteration with the device-resident CGLS loop
  // (cg_fused.h): 6 launches per CG step, one host poll.  Returns the published block.
  const double *prox_and_project_fused(const AdmmPreArgs<T> &pa0, int nw) {
    T *x = x_[nw].p;
    // y = A x by the recurrence, except every ysync_-th projection (and the first), which takes the
    // product itself
    const bool ysync = ysync_ <= 0 || (proj_count_ % static_cast<unsigned long long>(ysync_)) == 0;
    ++proj_count_;
    // prox, sums, over-relaxation; r = y0 - A x_warm (A x_warm is the previous y, see cgls_project),
    // x <- x_warm - x0                                                        (projector_cgls.cpp:62)
    AdmmPreArgs<T> pa = pa0;
    pa.x_aux = x;
    pa.y_aux = cg_r_.p;
    pa.cg_reset = ctx_.S.p + kFcDone;
    launch_admm_pre<T>(pa, ctx_.stream);
    // at most 500 steps (projector_cgls.cpp:17), as many as the previous projection took enqueued ahead
    return cg_loop_fused(x, nw, ysync, cg_pred_, 500, static_cast<double>(ctl_.proj_tol()), pa.partials);
  }

  // The loop proper: on entry x = x_warm - x0 (x: x_[nw]), cg_r_ = y0 - A x_warm, xtemp_ / ytemp_ = x0 / y0, x_[cur_] /
  // y_[cur_] the previous iterate (y_[cur_] = A x_warm starts the y recurrence) and S[kFcDone] = S[kFcSteps] = 0.
  // `ahead_steps` steps are enqueued before the first poll, at most `max_steps` in all.  pre_part: the prox step's partial
  // sums, summed with the closing launch's (null, one GPU only: there was no prox step -- sparse_cg_check).
  // *enqueued (optional): the steps the host enqueued.
  const double *cg_loop_fused(T *x, int nw, bool ysync, int ahead_steps, int max_steps, double tol, double *pre_part,
                              int *enqueued = nullptr) {
    hipStream_t s = ctx_.stream;
    const int bx = pre_blocks(n_), bm = pre_blocks(m_);
    double *S = ctx_.S.p;
    double *rec_t = cg_rec_.p, *rec_a = cg_rec_.p + cg_rec_cap_;          // A^T products, A products
    double *rec_x = ctx_.spart.p + sp_cgx_off_, *rec_p = ctx_.spart.p + sp_cgp_off_;
    double *cpart = ctx_.spart.p;   // closing launch: [bx + bm][2]
    const double shift = 1.0, kEps = std::numeric_limits<T>::epsilon();
    std::vector<size_t> &ev = fused_events_;
    ev.clear();
    size_t e;
    // Row shards: q = A p and r are this rank's rows; x, p, s and
    // u = A^T r (summed over the ranks) are replicated.  A CG step needs two sums over all ranks, |q|^2
    // and A^T r_new = u - alpha A^T q: with t = A^T q formed BEFORE alpha is known, both travel at the
    // same point -- t as the n-vector of local column sums, |q|^2 as the array of per-block records
    // (summed record by record; every block of U1 then adds the records up as on one GPU) -- in ONE
    // grouped RCCL launch per step, on the stream, between the launches that produce and consume
    // them: 0 host polls.  u is set by the explicit product at the start of every projection, so the
    // recurrence u -= alpha t runs over the few steps of one projection only.
    double *rec_a_sum = multi_ ? cg_rec_.p + 2 * cg_rec_cap_ : rec_a;
    double *rec_s2 = multi_ ? cg_rec_.p + 3 * cg_rec_cap_ : rec_t;
    const int nrec_a_sum = static_cast<int>(cg_rec_cap_);
    const int gv = cgf_blocks(std::max(n_, m_)), gp = cgf_blocks(n_);
    // s = A^T r - shift x ; p = s ; |s_0|^2 records                           (cgls.h:236-245)
    int nrec_s0;
    if (!multi_) {
      nrec_s0 = op_->spmv_cg(op_->At(), cg_r_.p, SpCgInitOp<T>{static_cast<T>(shift), x, cg_s_.p, cg_p_.p}, rec_t, -1, &e);
    } else {
      op_->spmv_cg(op_->At(), cg_r_.p, SpStoreOp<T>{tsum_.p}, rec_t, -1, &e);
      ctx_.dist.allreduce(tsum_.p, n_, s);
      nrec_s0 = cgf_blocks(n_);
      SpCgInitOp<T> init{static_cast<T>(shift), x, cg_s_.p, cg_p_.p};
      init.u = cg_u_.p;
      hipLaunchKernelGGL((cgf_reduce_kernel<T, SpCgInitOp<T>>), dim3(nrec_s0), dim3(kCgfTpb), 0, s, tsum_.p, n_, 1, init,
                         rec_t, S, -1);
    }
    int enq = 0;
    auto step = [&]() {
      // q = A p, |q|^2 records                                               (cgls.h:257-260)
      int nrec_q = op_->spmv_cg(op_->A(), cg_p_.p, SpAxpbyNormOp<T>{1, 0, nullptr, cg_q_.p}, rec_a, 0, &e);
      ev.push_back(e);
      if (multi_) {
        // t = A^T q (this rank's rows), then t and the |q|^2 records over all ranks
        op_->spmv_cg(op_->At(), cg_q_.p, SpStoreOp<T>{tsum_.p}, rec_s2, 0, &e);
        ev.push_back(e);
        {
          DistComm::Group grp(ctx_.dist);   // one RCCL launch; closed on every way out (also by an exception)
          ctx_.dist.allreduce(tsum_.p, n_, s);
          ctx_.dist.allreduce(rec_a, rec_a_sum, static_cast<size_t>(nrec_a_sum), s);
        }
        nrec_q = nrec_a_sum;
      }
      // alpha ; x += alpha p ; r -= alpha q ; y_new += alpha q ; |x|^2        (:262-277, 298)
      // (row shards: also u -= alpha t ; s = u - shift x ; |s|^2, :281-286)
      CgfStepA<T> a;
      a.n = n_; a.m = m_; a.S = S;
      a.first = enq == 0; a.gslot = enq & 1;
      a.rec_s0 = rec_t; a.nrec_s0 = nrec_s0;
      a.rec_p = rec_p; a.nrec_p = gp;
      a.rec_q = rec_a_sum; a.nrec_q = nrec_q;
      a.shift = shift; a.eps = kEps;
      a.p = cg_p_.p; a.x = x; a.q = cg_q_.p; a.r = cg_r_.p;
      a.ycur = y_[cur_].p; a.ynew = ysync ? nullptr : y_[nw].p;
      a.rec_x = rec_x;
      a.u = multi_ ? cg_u_.p : nullptr; a.t = tsum_.p; a.s = cg_s_.p; a.rec_s = rec_s2;
      a.nb_n = gp;
      hipLaunchKernelGGL(cgf_step_a_kernel<T>, dim3(gv), dim3(kCgfTpb), 0, s, a);
      int nrec_s = gp;
      if (!multi_) {
        // s = A^T r - shift x ; |s|^2 records                                (:281-286)
        nrec_s = op_->spmv_cg(op_->At(), cg_r_.p, SpAxpbyNormOp<T>{1, static_cast<T>(-shift), x, cg_s_.p}, rec_t, 0, &e);
        ev.push_back(e);
      }
      // beta, gamma, the stopping test ; p = s + beta p ; |p|^2              (:288-305)
      CgfStepB<T> b;
      b.n = n_; b.S = S; b.k = enq;
      b.rec_s = rec_s2; b.nrec_s = nrec_s;
      b.rec_x = rec_x; b.nrec_x = gp;
      b.tol = tol; b.maxit = max_steps;
      b.s = cg_s_.p; b.p = cg_p_.p; b.rec_p = rec_p;
      hipLaunchKernelGGL(cgf_step_b_kernel<T>, dim3(gp), dim3(kCgfTpb), 0, s, b);
      ++enq;
    };
    auto close = [&]() {
      // x <- x + x0 (projector_cgls.cpp:75), the bookkeeping of both halves (y_new from the
      // recurrence), the iteration's sums and the publish
      CgfClose<T> c;
      c.n = n_; c.m = m_; c.S = S;
      c.x = x; c.xprev = x_[cur_].p; c.x12 = x12_.p; c.xtemp = xtemp_.p;
      c.ynew = ysync ? nullptr : y_[nw].p; c.yprev = y_[cur_].p; c.y12 = y12_.p; c.ytemp = ytemp_.p;
      c.part = cpart; c.blocks_x = bx;
      hipLaunchKernelGGL(cgf_close_kernel<T>, dim3(ysync ? bx : bx + bm), dim3(kVecTpb), 0, s, c);
      if (pre_part) ctx_.queue_sum(SumJob{pre_part, bx, 3, S + kGapX});
      ctx_.queue_sum(SumJob{cpart, bx, 2, S + kDXprev2});
      if (!multi_) {
        if (pre_part) ctx_.queue_sum(SumJob{pre_part + static_cast<size_t>(bx) * 3, bm, 3, S + kGapY});
        if (!ysync) ctx_.queue_sum(SumJob{cpart + static_cast<size_t>(bx) * 2, bm, 2, S + kDYprev2});
      } else {
        // the y-side sums are over this rank's rows: slots kGapY .. kDY12 are adjacent, one all-reduce
        static_assert(kWY2 == kGapY + 1 && kHY2 == kGapY + 2 && kDYprev2 == kGapY + 3 && kDY12 == kGapY + 4, "slot order");
        SumJob j[2] = {{pre_part + static_cast<size_t>(bx) * 3, bm, 3, S + kGapY},
                       {cpart + static_cast<size_t>(bx) * 2, bm, 2, S + kDYprev2}};
        launch_sum_jobs(j, ysync ? 1 : 2, s);
        ctx_.dist.allreduce(S + kGapY, ysync ? 3 : 5, s);
      }
      return ctx_.fetch_scalars();
    };
    const int ahead = std::max(1, std::min(ahead_steps, max_steps));
    for (int k = 0; k < ahead; ++k) step();
    const double *Sh = close();
    int more = 1;
    while (Sh[kFcDone] == 0.0) {   // the loop needed more steps than the previous projection
      for (int k = 0; k < more && enq < max_steps; ++k) step();
      Sh = close();
      more = std::min(2 * more, 64);   // a growing chunk per host poll, not one step per poll
    }
    const int steps = static_cast<int>(Sh[kFcSteps]);
    cg_pred_ = std::max(1, steps);
    ctx_.stats.cg_iters += static_cast<unsigned long long>(steps);
    // launches that found the loop ended were no-ops
    for (size_t k = 2 * static_cast<size_t>(steps); k < ev.size(); ++k) ctx_.stream_timer.drop(ev[k]);
    timed_spmvs_ += 1 + 2 * static_cast<unsigned long long>(steps);
    if (ysync) {
      // y = A x fused with the y-half bookkeeping                             (projector_cgls.cpp:78)
      spmv<false>(op_->A(), x, nullptr, SpTailOp<T>{y_[nw].p, y_[cur_].p, y12_.p, ytemp_.p}, S + kDYprev2, true);
      reduce_y_scalars(S + kDYprev2, 2);
      Sh = ctx_.fetch_scalars();
    }
    if (enqueued) *enqueued = enq;
    return Sh;
  }

  bool iteration(unsigned verbose) override {
    hipStream_t s = ctx_.stream;
    const int nw = cur_ ^ 1;
    AdmmPreArgs<T> pa = pre_args();
    pa.uf = uni_f_; pa.ug = uni_g_;
    pa.partials = ctx_.spart.p + sp_pre_off_;
    const double *S;
    if (fused_cg_) {
      S = prox_and_project_fused(pa, nw);
    } else {
    launch_admm_pre<T>(pa, s);
    {
      SumJob j[2] = {{pa.partials, pa.blocks_x, 3, ctx_.S.p + kGapX},
                     {pa.partials + static_cast<size_t>(pa.blocks_x) * 3, pre_blocks(m_), 3, ctx_.S.p + kGapY}};
      if (!multi_) {
        // one GPU: summed by the launch that publishes the scalar block next (the first fetch of the
        // projection); the partials have a region of their own until then
        ctx_.queue_sum(j[0]);
        ctx_.queue_sum(j[1]);
      } else {
        launch_sum_jobs(j, 2, s);
        reduce_y_scalars(ctx_.S.p + kGapY, 3);
      }
    }
    if (direct_) direct_project_x(xtemp_.p, ytemp_.p, x_[nw].p, true);
    // warm start with the previous x (pogs.cpp:281), then CGLS
    else cgls_project(xtemp_.p, ytemp_.p, x_[nw].p, ctl_.proj_tol(), y_[cur_].p, x_[cur_].p);   // y_cur == A x_cur
    if (direct_ && !tall_) {
      // y = y0 + t as the reference forms it (projector_direct_dense.cpp:134), with the y-half bookkeeping
      double *yp = ctx_.spart.p + static_cast<size_t>(vec_blocks(n_)) * 2;   // (the x half's partials come first)
      hipLaunchKernelGGL(direct_wide_y_kernel<T>, dim3(vec_blocks(m_)), dim3(256), 0, s, m_, dr_.p, y_[cur_].p, y12_.p,
                         ytemp_.p, y_[nw].p, yp);
      ctx_.queue_sum(SumJob{yp, vec_blocks(m_), 2, ctx_.S.p + kDYprev2});
    } else {
    // y = A x fused with the y-half bookkeeping; x-half element-wise        (projector_cgls.cpp:78)
    spmv<false>(op_->A(), x_[nw].p, nullptr, SpTailOp<T>{y_[nw].p, y_[cur_].p, y12_.p, ytemp_.p}, ctx_.S.p + kDYprev2, true);
    reduce_y_scalars(ctx_.S.p + kDYprev2, 2);
    }
    launch_admm_tail<T>(n_, x_[nw].p, x_[cur_].p, x12_.p, xtemp_.p, ctx_.spart.p, s);
    ctx_.queue_sum(SumJob{ctx_.spart.p, vec_blocks(n_), 2, ctx_.S.p + kDXprev2});   // x side: no exchange; summed by the fetch below
    S = ctx_.fetch_scalars();
    }
    ctl_.set_pre(S);
    bool exact = false;
    if (ctl_.set_approx(S, nrmA_)) {
      spmv<false>(op_->A(), x12_.p, nullptr, SpExactROp<T>{y12_.p}, ctx_.S.p + kExactR2, true);
      reduce_y_scalars(ctx_.S.p + kExactR2, 1);
      hipLaunchKernelGGL(exact_u_kernel<T>, dim3((m_ + 255) / 256), dim3(256), 0, s, m_, y12_.p, yt_.p, y_[cur_].p,
                         zt_scale_, u_.p);
      spmv_t<false>(u_.p, SpExactSOp<T>{x12_.p, xt_.p, x_[cur_].p, zt_scale_}, ctx_.S.p + kExactS2, true);
      S = ctx_.fetch_scalars();
      ctl_.set_exact(S);
      exact = true;
    }
    const bool stop = ctl_.check_stop(exact);
    log_iteration(verbose);
    if (stop) return true;
    advance(nw);
    return false;
  }

  void collect_timer() override {
    ctx_.stats.matvecs += timed_spmvs_;
    if (const unsigned long long cnt = collect_timer_head()) {
      // algorithmic bytes of one SpMV: nnz (s + 4) + 4 (rows + 1) + s (rows + cols)
      // (a mixed tiled copy streams 4-byte values; the products alternate between the copies, as the row term assumes)
      const double vbytes = 0.5 * (op_->A().mixed ? 4.0 : sizeof(T)) + 0.5 * (op_->At().mixed ? 4.0 : sizeof(T));
      const double per = static_cast<double>(nnz_) * (vbytes + 4) + 4.0 * (0.5 * (m_ + n_) + 1) +
                         static_cast<double>(sizeof(T)) * (m_ + n_);
      ctx_.stats.stream_bytes += static_cast<double>(cnt) * per;
    }
    timed_spmvs_ = 0;
  }

  void print_solver_line(int status) override {
    const PogsAmdStats &st = ctx_.stats;
    std::printf("POGS-AMD sparse/%s: status %d, iter %u, init %.3e s, loop %.3e s, cg %llu, spmv %llu\n",
                direct_ ? "direct" : "cgls", status, ctl_.k, st.t_init_s, st.t_loop_s, st.cg_iters, st.matvecs);
  }

  size_t nnz_ = 0;
  bool mixed_ = false, mixed_pass_ = false;   // mixed storage: values rounded to float; the tiled copies store floats
  std::optional<SparseOperator<T>> op_;   // A and A^T (built once ctx_ is initialised)
  DevBuf<T> tsum_;   // row shards: this rank's A^T partial sums before the all-reduce
  DevBuf<T> cg_u_;   // row shards, device-resident CG loop: A^T r over all ranks, kept by recurrence
  size_t sp_cgx_off_ = 0, sp_cgp_off_ = 0, sp_pre_off_ = 0;   // regions of ctx_.spart (alloc_state)
  unsigned long long timed_spmvs_ = 0;
  std::vector<size_t> fused_events_;
  DevBuf<T> cg_p_, cg_s_, cg_q_, cg_r_, cg_b_, u_;
  DevBuf<double> cg_;
  // direct projector (POGS_AMD_PROJ_DIRECT; factor_direct)
  bool direct_ = false, tall_ = true;
  int k_ = 0;                    // min(m, n)
  size_t kld_ = 0;               // leading dimension of W and U
  DevBuf<T> fac_;                // [W = L^-1 | U = W^T], k_ x kld_ each
  T *Wp_ = nullptr, *Up_ = nullptr;
  DevBuf<T> dr_, dt_;            // right-hand side (wide: then t) and W rhs
  // device-resident CGLS loop (cg_fused.h)
  bool fused_cg_ = false;
  int cg_pred_ = 1;              // CG steps enqueued ahead: what the previous projection took
  DevBuf<double> cg_rec_;        // scalar records of its products: [A^T products | A products]
  size_t cg_rec_cap_ = 0;
  int ysync_ = 16;               // y = A x explicitly every ysync_-th iteration (0: always), else by recurrence
  unsigned long long proj_count_ = 0;
  FnUniform<T> uni_f_, uni_g_;   // coefficient arrays of f / g that hold one value throughout (load_problem)
};

#include "sparse_batch.h"

}  // namespace

SolverBase *make_sparse_solver(int dtype, int ord, size_t m, size_t n, size_t nnz, const void *data, const int *ptr,
                               const int *ind, int mem, const PogsAmdOptions *opt, const PogsAmdDist *dist) {
  if (dtype == POGS_AMD_F32) return new SparseSolver<float>(ord, m, n, nnz, data, ptr, ind, mem, opt, dist);
  if (dtype == POGS_AMD_F64) return new SparseSolver<double>(ord, m, n, nnz, data, ptr, ind, mem, opt, dist);
  throw Error("unknown dtype");
}

// PogsAmdCreateSparseMixed: an fp64 handle over float non-zeros (include/pogs_amd.h)
SolverBase *make_sparse_solver_mixed(int ord, size_t m, size_t n, size_t nnz, const double *data, const int *ptr,
                                     const int *ind, int mem, const PogsAmdOptions *opt) {
  return new SparseSolver<double>(ord, m, n, nnz, data, ptr, ind, mem, opt, nullptr, true);
}

namespace {
// PogsAmdSpmvCheck: the copies as a solve builds them (SparseOperator, with the switches a solve reads from the
// environment and the planner's two geometry choices as arguments), the second write of the values as equilibrate()
// ends (scale, finalize_values), then one product with the functor of the norm estimate
template <typename T>
void spmv_check_t(const SpmvCheckArgs &a) {
  std::optional<DevicePool::QuiescedScope> drained;   // from the last sync on: blocks go back to the pool as idle
  Ctx ctx;
  ctx.init(-1, 0);
  if (a.num_cu > 0) ctx.num_cu = a.num_cu;
  hipStream_t s = ctx.stream;
  const int m = a.nrows, n = a.ncols;
  const size_t nnz = static_cast<size_t>(a.ptr[(a.ord == ROW_MAJ) ? m : n]);
  SparseOperator<T> op(ctx, a.ord, m, n, nnz, a.val, a.ptr, a.ind, POGS_AMD_HOST,
                       SpmvChoice{a.format, a.force_rr_rows, a.force_ncg, (a.trans == 'n') ? 0 : 1});
  ctx.ensure_spart(op.partials_needed() * 4 + 64);
  const DevCsr<T> &built = op.first_is_A() ? op.At() : op.A();   // the copy the operator transposed on the device
  if (a.t_ptr) POGS_HIP_CHECK(hipMemcpyAsync(a.t_ptr, built.ptr.p, (built.nrows + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
  if (a.t_ind && nnz) POGS_HIP_CHECK(hipMemcpyAsync(a.t_ind, built.ind.p, nnz * sizeof(int), hipMemcpyDeviceToHost, s));
  if (a.t_val && nnz) POGS_HIP_CHECK(hipMemcpyAsync(a.t_val, built.val.p, nnz * sizeof(T), hipMemcpyDeviceToHost, s));
  {
    // one factor throughout, given as the row factors of A (and so the column factors of A^T)
    const size_t mx = static_cast<size_t>(std::max(m, n));
    DevBuf<T> sc(mx), one(mx);
    launch_fill<T>(sc.p, static_cast<T>(a.scale), mx, s);
    launch_fill<T>(one.p, static_cast<T>(1), mx, s);
    op.scale(sc.p, one.p, ctx.spart.p, ctx.spart.p + op.grid_cap());
    if (a.mixed) op.round_values();   // PogsAmdSpmvMixedCheck: rounded, then the tiled values as floats
    op.finalize_values(a.mixed != 0);
    ctx.sync();   // sc / one are freed at scope exit
  }
  const DevCsr<T> &M = a.trans == 't' ? op.At() : op.A();
  DevBuf<T> vin(a.xlen), vout(a.ylen);
  POGS_HIP_CHECK(hipMemcpyAsync(vin.p, a.x, a.xlen * sizeof(T), hipMemcpyHostToDevice, s));
  POGS_HIP_CHECK(hipMemcpyAsync(vout.p, a.y, a.ylen * sizeof(T), hipMemcpyHostToDevice, s));
  const double *x_nrm2 = nullptr;
  if (a.x_nrm2 != 0.0) {
    POGS_HIP_CHECK(hipMemcpyAsync(ctx.S.p + kPowX2, &a.x_nrm2, sizeof(double), hipMemcpyHostToDevice, s));
    x_nrm2 = ctx.S.p + kPowX2;
  }
  const SpAxpbyNormOp<T> fn{static_cast<T>(a.alpha), static_cast<T>(a.beta), vout.p, vout.p};
  if (a.sq) op.template spmv<true>(M, vin.p, x_nrm2, fn, ctx.S.p + kPowSx2);
  else op.template spmv<false>(M, vin.p, x_nrm2, fn, ctx.S.p + kPowSx2);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipMemcpyAsync(a.y, vout.p, a.ylen * sizeof(T), hipMemcpyDeviceToHost, s));
  POGS_HIP_CHECK(hipMemcpyAsync(a.sumsq, ctx.S.p + kPowSx2, sizeof(double), hipMemcpyDeviceToHost, s));
  ctx.sync();
  drained.emplace();
  for (int c = 0; c < 2; ++c) op.describe(c, a.info + 8 * c);
}
}  // namespace

namespace {
// PogsAmdSparseGramCheck: the copies as a handle builds them, values as given, then the launch factor_direct() runs
template <typename T>
void sparse_gram_check_t(const SparseGramCheckArgs &a) {
  std::optional<DevicePool::QuiescedScope> drained;
  Ctx ctx;
  ctx.init(-1, 0);
  if (a.num_cu > 0) ctx.num_cu = a.num_cu;
  hipStream_t s = ctx.stream;
  const int m = a.nrows, n = a.ncols, K = std::min(m, n);
  const bool tall = m > n;
  const size_t nnz = static_cast<size_t>(a.ptr[(a.ord == ROW_MAJ) ? m : n]);
  SparseOperator<T> op(ctx, a.ord, m, n, nnz, a.val, a.ptr, a.ind, POGS_AMD_HOST);
  const size_t ld = round_up(static_cast<size_t>(K), Vec16<T>::N), row = static_cast<size_t>(K) * sizeof(T);
  DevBuf<T> G(static_cast<size_t>(K) * ld);
  G.zero(s);
  POGS_HIP_CHECK(hipMemcpy2DAsync(G.p, ld * sizeof(T), a.G, a.ldg * sizeof(T), row, K, hipMemcpyHostToDevice, s));
  const DevCsr<T> &O = tall ? op.At() : op.A(), &I = tall ? op.A() : op.At();
  const SparseGramInfo gi = launch_sparse_gram<T>(
      SparseGramArgs<T>{O.val.p, O.ind.p, O.ptr.p, I.val.p, I.ind.p, I.ptr.p, K, a.window, G.p, ld}, ctx.num_cu, s);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipMemcpy2DAsync(a.G, a.ldg * sizeof(T), G.p, ld * sizeof(T), row, K, hipMemcpyDeviceToHost, s));
  ctx.sync();
  drained.emplace();
  const int out[8] = {K, tall ? 1 : 0, gi.window, gi.windows, gi.grid, static_cast<int>(ld), 0, 0};
  for (int i = 0; i < 8; ++i) a.info[i] = out[i];
}

template <typename T>
void tri_matvec_check_t(int tri, int n, const T *M, size_t ldm, const T *x, T *y) {
  POGS_CHECK(ldm % Vec16<T>::N == 0, "ldm must be a multiple of the 16-byte vector");
  hipStream_t s = nullptr;
  const size_t nm = static_cast<size_t>(n) * ldm;
  DevBuf<T> dM(nm), dx(static_cast<size_t>(n)), dy(static_cast<size_t>(n));
  POGS_HIP_CHECK(hipMemcpy(dM.p, M, nm * sizeof(T), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dx.p, x, static_cast<size_t>(n) * sizeof(T), hipMemcpyHostToDevice));
  POGS_HIP_CHECK(hipMemcpy(dy.p, y, static_cast<size_t>(n) * sizeof(T), hipMemcpyHostToDevice));
  launch_tri_matvec<T>(tri, dM.p, ldm, n, dx.p, dy.p, s);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipMemcpy(y, dy.p, static_cast<size_t>(n) * sizeof(T), hipMemcpyDeviceToHost));
  POGS_HIP_CHECK(hipDeviceSynchronize());
}
}  // namespace

void sparse_gram_check(const SparseGramCheckArgs &a) {
  // every refusal comes before the first HIP call
  POGS_CHECK(a.dtype == POGS_AMD_F32 || a.dtype == POGS_AMD_F64, "unknown dtype");
  POGS_CHECK(a.ord == ROW_MAJ || a.ord == COL_MAJ, "unknown ord (ROW_MAJ: CSR, COL_MAJ: CSC)");
  POGS_CHECK(a.ptr && a.ind && a.val && a.G && a.info, "null argument");
  POGS_CHECK(a.nrows >= 1 && a.ncols >= 1, "nrows and ncols must be >= 1");
  POGS_CHECK(std::min(a.nrows, a.ncols) <= POGS_AMD_SPARSE_DIRECT_MAX,
             "min(nrows, ncols) must be <= POGS_AMD_SPARSE_DIRECT_MAX");
  POGS_CHECK(a.num_cu >= 0, "num_cu must be >= 0");
  POGS_CHECK(a.window == 0 || (a.window % 64 == 0 && a.window >= 64 && a.window <= kSgWindowMax),
             "window must be 0 (the solver's choice) or a multiple of 64 in [64, 2048]");
  POGS_CHECK(a.ldg >= static_cast<size_t>(std::min(a.nrows, a.ncols)), "ldg must be >= min(nrows, ncols)");
  const int r1 = (a.ord == ROW_MAJ) ? a.nrows : a.ncols;
  POGS_CHECK(a.ptr[0] == 0, "ptr[0] must be 0");
  POGS_CHECK(a.ptr[r1] >= 1, "ptr must end at the number of non-zeros (>= 1: an empty matrix has no product to check)");
  if (a.dtype == POGS_AMD_F32) sparse_gram_check_t<float>(a);
  else sparse_gram_check_t<double>(a);
}

void tri_matvec_check(int dtype, int tri, int n, const void *M, size_t ldm, const void *x, void *y) {
  POGS_CHECK(dtype == POGS_AMD_F32 || dtype == POGS_AMD_F64, "unknown dtype");
  POGS_CHECK(tri == kTriLower || tri == kTriUpper, "unknown tri (1 lower, 2 upper)");
  POGS_CHECK(n >= 1, "n must be >= 1");
  POGS_CHECK(M && x && y, "null argument");
  POGS_CHECK(ldm >= static_cast<size_t>(n), "ldm must be >= n");
  if (dtype == POGS_AMD_F32)
    tri_matvec_check_t<float>(tri, n, static_cast<const float *>(M), ldm, static_cast<const float *>(x), static_cast<float *>(y));
  else
    tri_matvec_check_t<double>(tri, n, static_cast<const double *>(M), ldm, static_cast<const double *>(x),
                               static_cast<double *>(y));
}

void spmv_check(const SpmvCheckArgs &a) {
  // every refusal comes before the first HIP call
  POGS_CHECK(a.dtype == POGS_AMD_F32 || a.dtype == POGS_AMD_F64, "unknown dtype");
  POGS_CHECK(!a.mixed || (a.dtype == POGS_AMD_F64 && !a.sq), "the mixed product is fp64 and has no squared form");
  POGS_CHECK(a.ord == ROW_MAJ || a.ord == COL_MAJ, "unknown ord (ROW_MAJ: CSR, COL_MAJ: CSC)");
  POGS_CHECK(a.ptr && a.ind && a.val && a.x && a.y && a.sumsq && a.info, "null argument");
  POGS_CHECK(a.nrows >= 1 && a.ncols >= 1, "nrows and ncols must be >= 1");
  POGS_CHECK(a.trans == 'n' || a.trans == 't', "trans must be 'n' or 't'");
  POGS_CHECK(a.num_cu >= 0, "num_cu must be >= 0");
  POGS_CHECK(a.format >= kSpmvFormatAuto && a.format <= kSpmvFormatPlain,
             "unknown format (0 as a solve chooses, 1 tags, 2 two id slots, 3 plain CSR kernel)");
  const int r1 = (a.ord == ROW_MAJ) ? a.nrows : a.ncols;
  POGS_CHECK(a.ptr[0] == 0, "ptr[0] must be 0");
  POGS_CHECK(a.ptr[r1] >= 1, "ptr must end at the number of non-zeros (>= 1: an empty matrix has no product to check)");
  const bool f32 = a.dtype == POGS_AMD_F32;
  const int nin = a.trans == 'n' ? a.ncols : a.nrows, nout = a.trans == 'n' ? a.nrows : a.ncols;
  const int bw = f32 ? SellCfg<float>::BW : SellCfg<double>::BW, rrmax = f32 ? SellCfg<float>::RR : SellCfg<double>::RR;
  POGS_CHECK(a.force_rr_rows == 0 || (a.force_rr_rows % 64 == 0 && a.force_rr_rows >= 512 && a.force_rr_rows <= rrmax),
             "force_rr_rows must be 0 or a multiple of 64 in [512, the LDS-limit height of the type]");
  POGS_CHECK(a.force_ncg == 0 || (a.force_ncg >= 1 && a.force_ncg <= std::min((nin + bw - 1) / bw, 32)),
             "force_ncg must be 0 or in [1, min(column blocks of the copy the product runs on, 32)]");
  POGS_CHECK(a.xlen >= static_cast<size_t>(nin) && a.ylen >= static_cast<size_t>(nout), "xlen / ylen shorter than the vectors");
  if (f32) spmv_check_t<float>(a);
  else spmv_check_t<double>(a);
}

}  // namespace pogs_amd
