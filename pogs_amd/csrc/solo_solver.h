// The part of a solo solve that does not touch the matrix, once for DenseSolver<T, Tag> and SparseSolver<T>: the
// iterate and its control block, the solve / begin_run / iterate entries around the iteration, loading f and g,
// the objective, the epilogue and the head of the timer collection (PogsImplementation::Solve, src/cpu/pogs.cpp:91-581,
// minus the projection).  Whatever reads A -- the iteration, the warm start, what a cold start resets beyond the
// iterate, what loading a problem decides from it -- is a hook the subclass fills; nothing here asks which one it serves.
#pragma once
#include <cstdio>
#include <utility>
#include <vector>

#include "engine.h"
#include "vec_kernels.h"

namespace pogs_amd {

template <typename T>
class SoloSolver : public SolverBase {
 public:
  int dtype() const override { return sizeof(T) == 4 ? POGS_AMD_F32 : POGS_AMD_F64; }
  int device() const override { return ctx_.device; }
  void on_entry() override { ctx_.on_entry(); }
  void on_error() override { ctx_.on_error(); }
  PogsAmdStats &stats() override { return ctx_.stats; }

  int solve(const FnHost &f, const FnHost &g, const SolveParams &p, void *x, void *y, void *l, void *mu,
            double *optval, unsigned *final_iter) override {
    const double t0 = wall_s();
    begin_run(f, g, p);
    const double t1 = wall_s();
    if (ctx_.dist.rank() == 0) print_banner(p.verbose);
    while (!iteration(p.verbose)) {}
    ctx_.sync();
    const double t2 = wall_s();
    const int status = epilogue(x, y, l, mu, optval);
    *final_iter = ctl_.k;
    PogsAmdStats &st = ctx_.stats;
    st.t_loop_s = t2 - t1;
    st.t_total_s = st.t_init_s + (wall_s() - t0);
    st.iterations = ctl_.k + 1;
    st.exact_iters = ctl_.exact_iters;
    st.rho_updates = ctl_.rho_updates;
    st.rho_final = ctl_.rho;
    collect_timer();
    if (p.verbose > 0 && ctx_.dist.rank() == 0) {
      print_summary(status, st.t_total_s, st.t_init_s, ctl_);
      if (p.verbose > 3) print_timing_breakdown(st.t_loop_s, st.iterations);
      print_solver_line(status);
    }
    return status;
  }

  void begin_run(const FnHost &f, const FnHost &g, const SolveParams &p) override {
    load_problem(f, g, p);
    cold_start();
    apply_warm_start();
    ctx_.sync();
  }

  void set_warm_start(const void *x0, const void *l0) override {
    warm_x_.assign(static_cast<const T *>(x0), static_cast<const T *>(x0) + n_);
    warm_l_.assign(static_cast<const T *>(l0), static_cast<const T *>(l0) + m_);
    warm_pending_ = true;
  }

  void iterate(unsigned iters, double *seconds, unsigned *solves) override {
    POGS_CHECK(loaded_, "PogsAmdIterate before PogsAmdBeginRun / PogsAmdSolve: no problem is loaded");
    unsigned done = 0;
    ctx_.sync();
    const double t0 = wall_s();
    for (unsigned i = 0; i < iters; ++i) {
      if (ctl_.finished) {
        cold_start();
        ++done;
      }
      iteration(0);
    }
    ctx_.sync();
    const double t1 = wall_s();
    if (seconds) *seconds = t1 - t0;
    if (solves) *solves = done;
    ctx_.stats.t_loop_s += t1 - t0;
    ctx_.stats.iterations += iters;
    collect_timer();
  }

 protected:
  // ---- what differs between the solvers ---------------------------------------
  // One ADMM iteration (pogs.cpp:253-470).  Returns true when the solve stops.
  virtual bool iteration(unsigned verbose) = 0;
  // z = 0, zt = 0 (pogs.cpp:71-73,121-126): reset_iterate() and the projector's own per-solve state
  virtual void cold_start() = 0;
  // (x0, lambda0) -> (z, z~): z = [x0 / e | A (x0 / e)], z~ = -(1/rho) [-A^T (l0 / d) | l0 / d]
  // (pogs.cpp:144-156).  Consumed once.
  virtual void apply_warm_start() = 0;
  // load_functions(), what the solver decides from the functions, arm_control()
  virtual void load_problem(const FnHost &f, const FnHost &g, const SolveParams &p) = 0;
  // collect_timer_head() and the bytes its passes streamed
  virtual void collect_timer() = 0;
  // the closing line of a verbose solve (rank 0)
  virtual void print_solver_line(int status) = 0;

  // ---- shared pieces ----------------------------------------------------------
  // The iterate, the equilibration vectors, the output and function buffers.  nx / ny: the lengths of the x- / y-sized
  // vectors the iteration reads (padded where its kernels load whole vectors); the iterate starts at zero.
  void alloc_iterate(size_t nx, size_t ny) {
    hipStream_t s = ctx_.stream;
    for (int i = 0; i < 2; ++i) { x_[i].alloc(nx); y_[i].alloc(ny); x_[i].zero(s); y_[i].zero(s); }
    xt_.alloc(nx); yt_.alloc(ny); xtemp_.alloc(nx); ytemp_.alloc(ny); x12_.alloc(nx); y12_.alloc(ny);
    xt_.zero(s); yt_.zero(s); xtemp_.zero(s); ytemp_.zero(s); x12_.zero(s); y12_.zero(s);
    d_.alloc(ny); e_.alloc(nx);
    xout_.alloc(nx); yout_.alloc(m_); lout_.alloc(m_); muout_.alloc(nx);
    f_.alloc(m_); g_.alloc(n_); fs_.alloc(m_); gs_.alloc(n_);
  }

  void load_functions(const FnHost &f, const FnHost &g) {
    hipStream_t s = ctx_.stream;
    upload_fn<T>(f_, f, m_, s);
    upload_fn<T>(g_, g, n_, s);
    warn_negative_coeffs<T>(f, m_);   // prox_lib.h:62-69 (the clamp is in scale_objective_kernel)
    warn_negative_coeffs<T>(g, n_);
    pre_cheap_ = all_h(f, m_, [](int h) { return is_cheap_prox(h); }) && all_h(g, n_, [](int h) { return is_cheap_prox(h); });
    // scaled copies: h and b shared with the originals (pogs.cpp:608-617)
    launch_scale_objective<T>(f_.view(), fs_.a.p, fs_.c.p, fs_.d.p, fs_.e.p, d_.p, m_, true, s);
    launch_scale_objective<T>(g_.view(), gs_.a.p, gs_.c.p, gs_.d.p, gs_.e.p, e_.p, n_, false, s);
  }
  void arm_control(const SolveParams &p) {
    ctl_ = make_admm_control<T>(p, p.rho, ctx_.m_global, n_);
    ctl_.say_rho = p.verbose > 3 && ctx_.dist.rank() == 0;
    loaded_ = true;
    ctx_.sync();  // the host coefficient arrays may be freed by the caller afterwards
  }
  FnView<T> fview() const { return FnView<T>{f_.h.p, fs_.a.p, f_.b.p, fs_.c.p, fs_.d.p, fs_.e.p}; }
  FnView<T> gview() const { return FnView<T>{g_.h.p, gs_.a.p, g_.b.p, gs_.c.p, gs_.d.p, gs_.e.p}; }

  void reset_iterate() {
    hipStream_t s = ctx_.stream;
    for (int i = 0; i < 2; ++i) { x_[i].zero(s); y_[i].zero(s); }
    xt_.zero(s); yt_.zero(s); xtemp_.zero(s); ytemp_.zero(s);
    cur_ = 0;
    zt_scale_ = 1;
    ctl_.reset();
  }

  // The prox step's arguments for both halves at the current iterate, partial sums at the head of the scalar scratch;
  // the caller changes what its pass does differently.
  AdmmPreArgs<T> pre_args() const {
    AdmmPreArgs<T> pa;
    pa.n_x = n_; pa.n_y = m_;
    pa.g = gview(); pa.f = fview();
    pa.x_cur = x_[cur_].p; pa.y_cur = y_[cur_].p;
    pa.xt = xt_.p; pa.yt = yt_.p;
    pa.zt_scale = zt_scale_;
    pa.x12 = x12_.p; pa.y12 = y12_.p;
    pa.xtemp = xtemp_.p; pa.ytemp = ytemp_.p;
    pa.rho = ctl_.rho; pa.alpha = ctl_.alpha(); pa.cheap = pre_cheap_;
    pa.partials = ctx_.spart.p;
    pa.blocks_x = pre_blocks(n_);
    return pa;
  }

  // End of an iteration that goes on: the dual update already sits in xtemp / ytemp (the projection's tail), so the
  // buffers swap roles; nw becomes the current iterate, rho adapts.
  void advance(int nw) {
    std::swap(xt_, xtemp_);
    std::swap(yt_, ytemp_);
    cur_ = nw;
    zt_scale_ = ctl_.adapt();
    ++ctl_.k;
  }

  // sums of a y-sized quantity: add the other ranks' rows
  void reduce_y_scalars(double *slot, int count) {
    if (multi_) ctx_.dist.allreduce(slot, count, ctx_.stream);
  }

  // launches that leave sum f(y12) in S[kFvalF] and sum g(x12) in S[kFvalG]
  void launch_objective() {
    hipStream_t s = ctx_.stream;
    const int by = vec_blocks(m_), bx = vec_blocks(n_);
    launch_func_eval<T>(m_, fview(), y12_.p, ctx_.spart.p, s);
    launch_func_eval<T>(n_, gview(), x12_.p, ctx_.spart.p + by, s);
    SumJob j[2] = {{ctx_.spart.p, by, 1, ctx_.S.p + kFvalF}, {ctx_.spart.p + by, bx, 1, ctx_.S.p + kFvalG}};
    launch_sum_jobs(j, 2, s);
    reduce_y_scalars(ctx_.S.p + kFvalF, 1);
  }
  static double objective_of(const double *S) {
    return static_cast<double>(static_cast<T>(S[kFvalF]) + static_cast<T>(S[kFvalG]));
  }
  // sum f(y12) + sum g(x12) at the current prox point (pogs.cpp:385, 473)
  double eval_objective() {
    launch_objective();
    return objective_of(ctx_.fetch_scalars());
  }
  // the reference's per-iteration line (pogs.cpp:382-388); every rank evaluates (the objective
  // sum is a collective on row shards), rank 0 prints
  void log_iteration(unsigned verbose) {
    if (!wants_iter_line(verbose, ctl_)) return;
    const double obj = eval_objective();
    if (ctx_.dist.rank() == 0) print_iter_line(ctl_, obj);
  }

  // optval, status, un-scaling, copy out (pogs.cpp:473-482, 510-518, 567-570).
  int epilogue(void *x, void *y, void *l, void *mu, double *optval) {
    hipStream_t s = ctx_.stream;
    launch_objective();
    UnscaleArgs<T> u;
    u.n_x = n_; u.n_y = m_;
    u.x12 = x12_.p; u.y12 = y12_.p; u.xt = xt_.p; u.yt = yt_.p;
    u.xprev = x_[cur_].p; u.yprev = y_[cur_].p; u.d = d_.p; u.e = e_.p;
    u.zt_scale = zt_scale_; u.rho = ctl_.rho;
    u.x_out = xout_.p; u.y_out = yout_.p; u.l_out = lout_.p; u.mu_out = muout_.p;
    launch_unscale<T>(u, s);
    POGS_HIP_CHECK(hipMemcpyAsync(x, xout_.p, n_ * sizeof(T), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipMemcpyAsync(y, yout_.p, m_ * sizeof(T), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipMemcpyAsync(l, lout_.p, m_ * sizeof(T), hipMemcpyDeviceToHost, s));
    if (mu) POGS_HIP_CHECK(hipMemcpyAsync(mu, muout_.p, n_ * sizeof(T), hipMemcpyDeviceToHost, s));
    *optval = objective_of(ctx_.fetch_scalars());
    // the polled sequence word says the kernels are done; the D2H copies into the caller's
    // (pageable) buffers are only guaranteed complete after a synchronizing call
    POGS_HIP_CHECK(hipStreamSynchronize(s));
    return ctl_.status();
  }

  // The communicator's counters and, in profile mode, the time of the bracketed passes since the last call.
  // Returns how many passes that was (0 with the timer off).
  unsigned long long collect_timer_head() {
    ctx_.stats.reserved[2] = static_cast<double>(ctx_.dist.collectives());   // all-reduce calls since creation
    ctx_.stats.reserved[3] = static_cast<double>(ctx_.dist.comm_nranks());   // ranks as the communicator reports them
    if (!ctx_.stream_timer.enabled()) return 0;
    unsigned long long cnt = 0;
    ctx_.stats.stream_ms += ctx_.stream_timer.collect_ms(&cnt);
    ctx_.stats.stream_launches += cnt;
    return cnt;
  }

  Ctx ctx_;   // first: outlives every buffer below and every member of the subclasses
  int m_ = 0, n_ = 0;
  bool multi_ = false;
  DevBuf<T> d_, e_;
  T nrmA_ = 0;
  DevBuf<T> x_[2], y_[2], xt_, yt_, xtemp_, ytemp_, x12_, y12_;
  DevBuf<T> xout_, yout_, lout_, muout_;
  FnBuf<T> f_, g_, fs_, gs_;
  AdmmControl<T> ctl_;
  bool loaded_ = false;   // load_problem has run: f, g and the control block are valid
  int cur_ = 0;
  T zt_scale_ = 1;
  bool pre_cheap_ = false;      // every f_i, g_j has a few-operation prox (admm_pre_kernel inlines it)
  bool warm_pending_ = false;
  std::vector<T> warm_x_, warm_l_;
};

}  // namespace pogs_amd
