// DenseSolver: the one-pass, device-resident CGLS projector (POGS_AMD_PROJ_CGLS_FUSED).
//
// Reference: ProjectorCgls::Project (src/cpu/projector/projector_cgls.cpp:52-88) -> cgls::Solve with shift 1
// (src/cpu/include/cgls.h:200-323).  cgls_project (dense_factor.h) runs that loop literally: two passes over A per CG
// step (q = A p, then s = A^T r - x), about nine launches and one host poll per step.  Here a CG step reads A ONCE and
// never involves the host -- s is carried by the recurrence the row-sharded sparse loop uses (cg_fused.h), with
// t = A^T q formed by the pass that forms q:
//
//   start  u = A^T r (one column-sum pass), s = u - x, p = s, |s_0|^2 records        reduce_cols_kernel<DcgInitColOp>
//   L1     q = A p, |q|^2 records, column partials of t = A^T q                      stream_rows_kernel DOT + ACC, DcgQRowOp
//   L2     alpha (every block adds up the |q|^2 and |p|^2 records itself, cgf_sum's fixed order);
//          x blocks: t_j (second stage of the column partials), s_j -= alpha (t_j + p_j), x_j += alpha p_j,
//                    |s|^2 and |x|^2 records;  y blocks: r -= alpha q, y_new += alpha q    dcg_step_a_kernel
//   L3     beta, gamma, the stopping test of cgls.h:301-305 -> S[kFcDone]; p = s + beta p, |p|^2 records, the step
//          count                                                                     cgf_step_b_kernel (cg_fused.h)
//   close  x += x0 and the iteration's bookkeeping, only when S[kFcDone] is set       cgf_close_kernel (cg_fused.h)
//
// s = A^T r - x is formed explicitly at the start of every projection, so the recurrence
// s_new = A^T (r - alpha q) - (x + alpha p) = s - alpha (t + p) spans the steps of one projection only.
// Every launch of a step returns at once when S[kFcDone] is set (the streaming kernel through the StreamOpGuarded
// trait of its row functor, stream.h).  The host enqueues as many steps as the previous projection took, the closing
// launch and the publish, and polls once per ADMM iteration; on a miss a growing chunk (1, 2, 4, ...) of steps and the
// closing launches again -- the rule and the scalar slots (kFc*, vec_kernels.h) of the sparse loop.  No atomics, every
// sum in one fixed order: two runs of one solve give the same bytes.
//
// Windowed plans (StreamPlan::xl): launch_stream splits L1 into window dot passes and window column passes, so a step
// reads A twice there -- correct results, no saving.
//
// Member definitions of the class template declared in dense_solver.h, which includes this file once, right after the
// class, inside its namespaces (no include guard, no namespace of its own); the kernels and functors of the loop first.

// (L1's row functor, DcgQRowOp, is in stream_mixed.h: the mixed launch functions name it)

// start: s_j = (A^T r)_j - shift x_j ; p_j = s_j ; |s_0|^2                  (cgls.h:236-245)
template <typename T>
struct DcgInitColOp {
  static constexpr int NS = 1;
  const T *x;
  T shift;
  T *s, *p;
  int n;
  template <int N>
  __device__ __forceinline__ void col(int j, T total, double (&acc)[N]) const {
    T v = 0;
    if (j < n) {
      v = total - shift * x[j];
      dev::prod_acc(acc[0], v, v);
    }
    s[j] = v;
    p[j] = v;
  }
};

constexpr int kDcgCols = 32;                    // column vectors per x block of L2
constexpr int kDcgGroups = kCgfTpb / kDcgCols;  // groups of partials per column vector
inline int dcg_blocks_x(int n_pad, int vec) { return (n_pad / vec + kDcgCols - 1) / kDcgCols; }

template <typename T>
struct DcgStepA {
  int n, n_pad, m;
  double *S;
  int first;                 // step 0: gamma = |s_0|^2 from rec_s0 (and |p|^2 = gamma), else gamma from S
  int gslot;                 // gamma slot to read (not first)
  const double *rec_s0; int nrec_s0;
  const double *rec_p; int nrec_p;
  const double *rec_q; int nrec_q;
  double shift, eps;
  const T *colpart; int nparts;   // L1's column partials [nparts][n_pad]
  const T *p; T *x; T *s;
  const T *q; T *r;
  const T *ycur; T *ynew;    // ynew == nullptr: the y recurrence is off (explicit product at the end)
  double *rec_x, *rec_s;     // [blocks_x]
  int blocks_x, blocks_y;
};
// L2: alpha = gamma / (|q|^2 + shift |p|^2) (cgls.h:262-271).  x blocks: t_j = sum of the column partials (groups of
// partials side by side, then the groups in order: the order depends on nparts alone), s_j -= alpha (t_j + shift p_j),
// x_j += alpha p_j (:274), |s|^2 and |x|^2 records.  y blocks: r -= alpha q (:277), y_new = (first ? y_warm : y_new)
// + alpha q.
template <typename T>
__global__ void __launch_bounds__(kCgfTpb) dcg_step_a_kernel(DcgStepA<T> a) {
  using V = typename Vec16<T>::type;
  constexpr int VEC = Vec16<T>::N;
  __shared__ double s_sum[kCgfWaves];
  __shared__ double s_red[2 * kCgfWaves];
  __shared__ V s_v[kDcgGroups][kDcgCols];
  if (cgf_skip(a.S, 0)) return;
  double gamma, p2;
  if (a.first) {
    double g[1];
    cgf_sum<1>(a.rec_s0, a.nrec_s0, g, s_sum);
    gamma = g[0];
    p2 = g[0];
  } else {
    double g[1];
    cgf_sum<1>(a.rec_p, a.nrec_p, g, s_sum);
    gamma = a.S[kFcGamma0 + a.gslot];
    p2 = g[0];
  }
  if (a.first && sqrt(gamma) < a.eps) {   // flag 1 (cgls.h:247-252): nothing to do, x stays
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      a.S[kFcGamma0] = gamma;
      a.S[kFcNorms0] = gamma;
      a.S[kFcDone] = 1.0;   // (a block that starts after this store returns at the guard: same outcome)
    }
    return;
  }
  double q2[1];
  cgf_sum<1>(a.rec_q, a.nrec_q, q2, s_sum);
  double delta = q2[0] + a.shift * p2;
  const bool indef = delta <= 0.0;
  if (delta == 0.0) delta = a.eps;
  const double alpha_d = gamma / delta;
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // (slots nobody reads in this launch)
    if (a.first) {
      a.S[kFcGamma0] = gamma;
      a.S[kFcNorms0] = gamma;
      a.S[kFcIndef] = 0.0;
    }
    if (indef) a.S[kFcIndef] = 1.0;
    a.S[kCgQ2] = q2[0];
    a.S[kCgP2] = p2;
    a.S[kFcDelta] = delta;
    a.S[kFcAlpha] = alpha_d;
  }
  const T alpha = static_cast<T>(alpha_d), neg_alpha = static_cast<T>(-alpha_d), sh = static_cast<T>(a.shift);
  if (static_cast<int>(blockIdx.x) >= a.blocks_x) {   // (uniform per block) the y side
    const int stride = a.blocks_y * kCgfTpb;
    const int t0 = (static_cast<int>(blockIdx.x) - a.blocks_x) * kCgfTpb + threadIdx.x;
    if (a.ynew) {
      const T *ysrc = a.first ? a.ycur : a.ynew;
      for (int i = t0; i < a.m; i += stride) {
        const T qi = a.q[i];
        a.r[i] += neg_alpha * qi;
        a.ynew[i] = ysrc[i] + alpha * qi;
      }
    } else {
      for (int i = t0; i < a.m; i += stride) a.r[i] += neg_alpha * a.q[i];
    }
    return;
  }
  const int cx = threadIdx.x % kDcgCols, g = threadIdx.x / kDcgCols;
  const int col = (blockIdx.x * kDcgCols + cx) * VEC;
  V sum = dev::vzero<V>();
  if (col < a.n_pad) {
    int b = g;
    for (; b + 3 * kDcgGroups < a.nparts; b += 4 * kDcgGroups) {   // four independent loads in flight
      V v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        v[k] = *reinterpret_cast<const V *>(a.colpart + static_cast<size_t>(b + k * kDcgGroups) * a.n_pad + col);
#pragma unroll
      for (int k = 0; k < 4; ++k) dev::vadd(sum, v[k]);
    }
    for (; b < a.nparts; b += kDcgGroups)
      dev::vadd(sum, *reinterpret_cast<const V *>(a.colpart + static_cast<size_t>(b) * a.n_pad + col));
  }
  s_v[g][cx] = sum;
  __syncthreads();
  double acc[2] = {0.0, 0.0};
  if (g == 0 && col < a.n_pad) {
    V tot = s_v[0][cx];
#pragma unroll 4
    for (int k = 1; k < kDcgGroups; ++k) dev::vadd(tot, s_v[k][cx]);
    V pv = *reinterpret_cast<const V *>(a.p + col);
    V sv = *reinterpret_cast<const V *>(a.s + col);
    V xv = *reinterpret_cast<const V *>(a.x + col);
    const T *tp = reinterpret_cast<const T *>(&tot), *pp = reinterpret_cast<const T *>(&pv);
    T *sp = reinterpret_cast<T *>(&sv), *xp = reinterpret_cast<T *>(&xv);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      if (col + i < a.n) {   // (padding columns stay zero)
        const T sn = sp[i] + neg_alpha * (tp[i] + sh * pp[i]);
        const T xn = xp[i] + alpha * pp[i];
        sp[i] = sn;
        xp[i] = xn;
        dev::prod_acc(acc[0], sn, sn);
        dev::prod_acc(acc[1], xn, xn);
      }
    }
    *reinterpret_cast<V *>(a.s + col) = sv;
    *reinterpret_cast<V *>(a.x + col) = xv;
  }
  dev::block_sum<2, kCgfTpb>(acc, s_red);
  if (threadIdx.x == 0) {
    a.rec_s[blockIdx.x] = acc[0];
    a.rec_x[blockIdx.x] = acc[1];
  }
}

// Regions of cgf_rec_ (doubles), sized once in alloc_state.
template <typename T, typename Tag>
void DenseSolver<T, Tag>::alloc_cg_fused() {
  const size_t nbx = static_cast<size_t>(dcg_blocks_x(n_pad_, Vec16<T>::N));
  const size_t pb = static_cast<size_t>(pre_blocks(n_)) + pre_blocks(m_);
  size_t off = 0;
  auto take = [&](size_t cnt) { const size_t o = off; off += cnt + 8; return o; };
  // (the |q|^2 records are the launch's own grid: the larger of planA_'s and, on a mixed-storage handle, the mixed plan's)
  cgo_q_ = take(std::max<size_t>(planA_.grid_max, mixed_store_ ? mixed1_grid_max(planM_) : 0));
  cgo_p_ = take(kCgfBlocks);
  cgo_x_ = take(nbx);
  cgo_s_ = take(nbx);
  cgo_s0_ = take(static_cast<size_t>(reduce_cols_grid(n_pad_, Vec16<T>::N)));
  cgo_pre_ = take(pb * 3);
  cgo_close_ = take(pb * 2);
  cgf_rec_.alloc(off);
  cgf_rec_.zero(ctx_.stream);
}

// The loop proper.  On entry x = x_warm - x0, cg_r_ = y0 - A x_warm, xtemp_ / ytemp_ = x0 / y0, S[kFcDone] = S[kFcSteps] = 0.
// xprev: the previous x of the bookkeeping.  ynew != null: y_new = ycur + sum alpha_k q_k (ycur = A x_warm, also the previous
// y of the bookkeeping) and the y half's bookkeeping in the closing launch; null: the caller takes y = A x itself.
// `ahead_steps` steps are enqueued before the first poll, at most `max_steps` in all.  pre_part: the prox step's partial sums
// ([pre_blocks(n) + pre_blocks(m)][3]), summed with the closing launch's (null: there was no prox step).
// *enqueued (optional): the steps the host enqueued.  Returns the published scalar block.
template <typename T, typename Tag>
const double *DenseSolver<T, Tag>::cg_loop_fused(T *x, const T *xprev, const T *ycur, T *ynew, int ahead_steps, int max_steps,
                                                 double tol, const double *pre_part, int *enqueued) {
  hipStream_t s = ctx_.stream;
  constexpr int VEC = Vec16<T>::N;
  const int bx = pre_blocks(n_), bm = pre_blocks(m_);
  double *S = ctx_.S.p;
  double *rec_q = cgf_rec_.p + cgo_q_, *rec_p = cgf_rec_.p + cgo_p_, *rec_x = cgf_rec_.p + cgo_x_;
  double *rec_s = cgf_rec_.p + cgo_s_, *rec_s0 = cgf_rec_.p + cgo_s0_, *cpart = cgf_rec_.p + cgo_close_;
  const double shift = 1.0, kEps = std::numeric_limits<T>::epsilon();
  const int gp = cgf_blocks(n_), gy = cgf_blocks(m_), gxa = dcg_blocks_x(n_pad_, VEC);
  // mixed storage: the start's column-sum pass and L1 read the float copy (stream_mixed.h) -- their own grids
  const bool mixed = mixed_cg();
  const int gridQ = cg_grid(true, true);
  const unsigned long long reads_per_step = (planA_.xl && !mixed) ? 2 : 1;   // windowed: dot windows, then column windows
  // u = A^T r ; s = u - shift x ; p = s ; |s_0|^2 records                     (cgls.h:236-245)
  cg_gemv_t_partials(cg_r_.p);
  launch_reduce_cols<T, DcgInitColOp<T>>(colpart_.p, cg_grid(false, true), n_pad_,
                                         DcgInitColOp<T>{x, static_cast<T>(shift), cg_s_.p, cg_p_.p, n_}, rec_s0, s);
  ctx_.stats.matvecs += 1;
  const int nrec_s0 = reduce_cols_grid(n_pad_, VEC);
  std::vector<size_t> &ev = cgf_events_;
  ev.clear();
  int enq = 0;
  auto step = [&]() {
    // L1: q = A p, |q|^2 records, column partials of t = A^T q                (cgls.h:257-260)
    StreamArgs<T> sa = argsA();
    sa.xin = cg_p_.p;
    sa.scalar_partials = rec_q;
    ev.push_back(cg_tbegin(kCgFormL1));
    bool done = false;
    if constexpr (std::is_same<T, double>::value) {
      if (mixed) {
        launch_stream_mixed(planM_, argsM(cg_p_.p, rec_q), DcgQRowOp<double>{cg_q_.p, S}, s);
        done = true;
      }
    }
    if (!done) launch_stream<T, true, true, false, kFull, Tag>(planA_, sa, DcgQRowOp<T>{cg_q_.p, S}, s);
    ctx_.stream_timer.end(s);
    // L2
    DcgStepA<T> a;
    a.n = n_; a.n_pad = n_pad_; a.m = m_; a.S = S;
    a.first = enq == 0; a.gslot = enq & 1;
    a.rec_s0 = rec_s0; a.nrec_s0 = nrec_s0;
    a.rec_p = rec_p; a.nrec_p = gp;
    a.rec_q = rec_q; a.nrec_q = gridQ;
    a.shift = shift; a.eps = kEps;
    a.colpart = colpart_.p; a.nparts = gridQ;
    a.p = cg_p_.p; a.x = x; a.s = cg_s_.p; a.q = cg_q_.p; a.r = cg_r_.p;
    a.ycur = ycur; a.ynew = ynew;
    a.rec_x = rec_x; a.rec_s = rec_s;
    a.blocks_x = gxa; a.blocks_y = gy;
    hipLaunchKernelGGL(dcg_step_a_kernel<T>, dim3(gxa + gy), dim3(kCgfTpb), 0, s, a);
    // L3: beta, gamma, the stopping test ; p = s + beta p ; |p|^2             (:288-305)
    CgfStepB<T> b;
    b.n = n_; b.S = S; b.k = enq;
    b.rec_s = rec_s; b.nrec_s = gxa;
    b.rec_x = rec_x; b.nrec_x = gxa;
    b.tol = tol; b.maxit = max_steps;
    b.s = cg_s_.p; b.p = cg_p_.p; b.rec_p = rec_p;
    hipLaunchKernelGGL(cgf_step_b_kernel<T>, dim3(gp), dim3(kCgfTpb), 0, s, b);
    ++enq;
  };
  auto close = [&]() {
    // x <- x + x0 (projector_cgls.cpp:75), the bookkeeping of both halves, the iteration's sums and the publish
    CgfClose<T> c;
    c.n = n_; c.m = m_; c.S = S;
    c.x = x; c.xprev = xprev; c.x12 = x12_.p; c.xtemp = xtemp_.p;
    c.ynew = ynew; c.yprev = ycur; c.y12 = y12_.p; c.ytemp = ytemp_.p;
    c.part = cpart; c.blocks_x = bx;
    hipLaunchKernelGGL(cgf_close_kernel<T>, dim3(ynew ? bx + bm : bx), dim3(kVecTpb), 0, s, c);
    if (pre_part) {
      ctx_.queue_sum(SumJob{pre_part, bx, 3, S + kGapX});
      ctx_.queue_sum(SumJob{pre_part + static_cast<size_t>(bx) * 3, bm, 3, S + kGapY});
    }
    ctx_.queue_sum(SumJob{cpart, bx, 2, S + kDXprev2});
    if (ynew) ctx_.queue_sum(SumJob{cpart + static_cast<size_t>(bx) * 2, bm, 2, S + kDYprev2});
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
  // launches that found the loop ended were no-ops: they read nothing
  ctx_.stats.matvecs += reads_per_step * static_cast<unsigned long long>(steps);
  for (size_t k = static_cast<size_t>(steps); k < ev.size(); ++k) ctx_.stream_timer.drop(ev[k]);
  if (mixed)   // (the bracketed launches that ran read the float copy: collect_timer)
    for (size_t k = 0; k < ev.size() && k < static_cast<size_t>(steps); ++k) mixed_timed_ += ev[k] != EventTimer::npos;
  if (enqueued) *enqueued = enq;
  return Sh;
}

// Steps (1) and (2c) of iteration() with the device-resident loop: prox, over-relaxation and the start of the projection
// in one launch (r = y0 - y_warm, x = x_warm - x0: the previous iterate is the warm start and its y is A x_warm), the loop,
// y = A x by the recurrence or -- every ysync_-th projection -- by the product.  Returns the published scalar block.
template <typename T, typename Tag>
const double *DenseSolver<T, Tag>::project_cg_fused(int nw, bool ysync, int ahead, int max_steps, double tol,
                                                    const double *pre_part, int *enqueued) {
  hipStream_t s = ctx_.stream;
  const double *Sh = cg_loop_fused(x_[nw].p, x_[cur_].p, y_[cur_].p, ysync ? nullptr : y_[nw].p, ahead, max_steps, tol,
                                   pre_part, enqueued);
  if (ysync) {
    // y = A x fused with the y half's bookkeeping                             (projector_cgls.cpp:78)
    StreamArgs<T> a = argsA();
    a.xin = x_[nw].p;
    const bool timed = cg_tbegin(kCgFormYsync) != EventTimer::npos;
    bool done = false;
    if constexpr (std::is_same<T, double>::value) {
      if (mixed_cg()) {
        launch_stream_mixed(planM_, argsM(x_[nw].p, ctx_.spart.p), ProjTailOp<double>{y_[nw].p, y_[cur_].p, y12_.p, ytemp_.p}, s);
        mixed_timed_ += timed;
        done = true;
      }
    }
    if (!done) launch_stream<T, true, false, false, kFull, Tag>(planA_, a, ProjTailOp<T>{y_[nw].p, y_[cur_].p, y12_.p, ytemp_.p}, s);
    ctx_.stream_timer.end(s);
    sum_row_scalars(cg_grid(true, false), 2, ctx_.S.p + kDYprev2);
    ctx_.stats.matvecs += 1;
    Sh = ctx_.fetch_scalars();
  }
  return Sh;
}

template <typename T, typename Tag>
const double *DenseSolver<T, Tag>::prox_and_project_fused(const AdmmPreArgs<T> &pa0, int nw) {
  const bool ysync = ysync_ <= 0 || (proj_count_ % static_cast<unsigned long long>(ysync_)) == 0;
  ++proj_count_;
  AdmmPreArgs<T> pa = pa0;
  pa.partials = cgf_rec_.p + cgo_pre_;
  pa.x_aux = x_[nw].p;
  pa.y_aux = cg_r_.p;
  pa.cg_reset = ctx_.S.p + kFcDone;
  launch_admm_pre<T>(pa, ctx_.stream);
  // at most 500 steps (projector_cgls.cpp:17), as many as the previous projection took enqueued ahead
  return project_cg_fused(nw, ysync, cg_pred_, 500, static_cast<double>(ctl_.proj_tol()), pa.partials, nullptr);
}

// PogsAmdProject on a fused handle: the start as cgls_project takes it without A x_warm (b = y0 - A x0, r = b - A x with
// x = x_warm - x0, x_warm = 0), the loop, x in x_[0]; the caller takes y = A x.
template <typename T, typename Tag>
void DenseSolver<T, Tag>::project_start_fused(double tol) {
  hipStream_t s = ctx_.stream;
  T *x = x_[0].p;
  double *vp = ctx_.spart.p + static_cast<size_t>(planA_.grid_max) * 6;
  x_[0].zero(s);
  hipLaunchKernelGGL(sub_norm_kernel<T>, dim3(vec_blocks(n_)), dim3(kVecTpb), 0, s, n_, x, xtemp_.p, x, vp);
  StreamArgs<T> a = argsA();
  a.xin = xtemp_.p;
  launch_stream<T, true, false, false, kFull, Tag>(planA_, a, SubDotOp<T>{ytemp_.p, cg_q_.p}, s);   // b = y0 - A x0
  a.xin = x;
  launch_stream<T, true, false, false, kFull, Tag>(planA_, a, SubDotOp<T>{cg_q_.p, cg_r_.p}, s);    // r = b - A x
  ctx_.stats.matvecs += 2;
  static_assert(kFcSteps == kFcDone + 1, "slot order");
  POGS_HIP_CHECK(hipMemsetAsync(ctx_.S.p + kFcDone, 0, 2 * sizeof(double), s));
  const int pred0 = cg_pred_;
  cg_loop_fused(x, x_[1].p, y_[1].p, nullptr, 1, 500, tol, nullptr, nullptr);
  cg_pred_ = pred0;   // (a projection from zero says nothing about the next iteration's)
}

// PogsAmdDenseCgCheck: one projection on given vectors by project_cg_fused, the member iteration() calls, with what the
// prox launch leaves put in place by hand.
template <typename T, typename Tag>
void DenseSolver<T, Tag>::dense_cg_check(const DenseCgCheckArgs &a) {
  POGS_CHECK(cg_fused_, "PogsAmdDenseCgCheck needs a dense handle created with POGS_AMD_PROJ_CGLS_FUSED");
  hipStream_t s = ctx_.stream;
  ctx_.sync();
  const PogsAmdStats stats0 = ctx_.stats;
  const int pred0 = cg_pred_;
  const int nw = cur_ ^ 1;
  auto up = [&](T *dst, const void *src, int cnt) {
    POGS_HIP_CHECK(hipMemcpyAsync(dst, src, static_cast<size_t>(cnt) * sizeof(T), hipMemcpyHostToDevice, s));
  };
  auto down = [&](void *dst, const T *src, int cnt) {
    POGS_HIP_CHECK(hipMemcpyAsync(dst, src, static_cast<size_t>(cnt) * sizeof(T), hipMemcpyDeviceToHost, s));
  };
  up(xtemp_.p, a.x0, n_); up(ytemp_.p, a.y0, m_); up(x_[cur_].p, a.x_warm, n_); up(y_[cur_].p, a.y_warm, m_);
  x12_.zero(s); y12_.zero(s);
  // what admm_pre_kernel leaves: r = y0 - y_warm, x = x_warm - x0, the done flag and the step count cleared
  double *vp = ctx_.spart.p + static_cast<size_t>(planA_.grid_max) * 6;
  hipLaunchKernelGGL(sub_norm_kernel<T>, dim3(vec_blocks(m_)), dim3(kVecTpb), 0, s, m_, ytemp_.p, y_[cur_].p, cg_r_.p, vp);
  hipLaunchKernelGGL(sub_norm_kernel<T>, dim3(vec_blocks(n_)), dim3(kVecTpb), 0, s, n_, x_[cur_].p, xtemp_.p, x_[nw].p, vp);
  static_assert(kFcSteps == kFcDone + 1, "slot order");
  POGS_HIP_CHECK(hipMemsetAsync(ctx_.S.p + kFcDone, 0, 2 * sizeof(double), s));
  int enq = 0;
  const unsigned long long mv0 = ctx_.stats.matvecs;
  const double *Sh = project_cg_fused(nw, a.ysync != 0, a.ahead, a.max_steps, a.tol, nullptr, &enq);
  const int steps = static_cast<int>(Sh[kFcSteps]);
  const unsigned long long mv = ctx_.stats.matvecs - mv0;
  POGS_HIP_CHECK(hipGetLastError());
  down(a.x, x_[nw].p, n_); down(a.y_new, y_[nw].p, m_);
  down(a.r, cg_r_.p, m_); down(a.p, cg_p_.p, n_); down(a.s, cg_s_.p, n_);
  double hS[kNumSlots];
  POGS_HIP_CHECK(hipMemcpyAsync(hS, ctx_.S.p, kNumSlots * sizeof(double), hipMemcpyDeviceToHost, s));
  ctx_.sync();
  int k = 0;
  for (int slot = kFcDone; slot <= kFcIndef; ++slot) a.slots[k++] = hS[slot];
  for (int slot : {kCgQ2, kCgP2, kCgS2, kCgX2, kDXprev2, kDX12, kDYprev2, kDY12}) a.slots[k++] = hS[slot];
  *a.enqueued = enq;
  *a.steps = steps;
  *a.matvecs = mv;
  // the handle as it was, for the next solve: the prediction and the counters; the vectors of a run in progress
  // (PogsAmdBeginRun / PogsAmdIterate) are gone
  ctx_.stats = stats0;
  cg_pred_ = pred0;
  if (ctx_.stream_timer.enabled()) {
    unsigned long long cnt = 0;
    (void)ctx_.stream_timer.collect_ms(&cnt);
  }
  loaded_ = false;
}
