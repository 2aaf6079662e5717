// The ADMM loop of the batched solves: up to kBatchMax graph-form problems (own f, g, rho) on one handle's matrix,
// advanced side by side.  Shared by the dense batch (dense_batch.h) and the sparse batch (sparse_batch.h), which
// supply the two steps that touch the matrix:
//   project(slots, nw)         x[nw], y[nw] of the listed problems from xtemp, ytemp (warm start: x[cur], y[cur]);
//   residual_products(slots)   zy = A x12, zx = A^T u of the listed problems.
// Everything else is here, once: the per-problem vectors (problem j at offset j * ld, zero padding throughout), the
// function tables, the controls, the element-wise stages (batch_kernels.hip), the one poll per iteration, and the
// rule that keeps a member's bytes independent of its batch and slot: a problem that stops is finished from the
// iterate of that iteration and leaves the slot list; nothing of it is touched again.
// Members may start warm (warm_begin, between the constructor and run()): from a caller's (x0, l0) at their own rho,
// through the same residual_products.
#pragma once
#include <algorithm>
#include <array>
#include <cstdio>
#include <utility>
#include <vector>

#include "batch_kernels.h"
#include "engine.h"
#include "vec_kernels.h"

namespace pogs_amd {

template <typename T>
struct BatchAdmm {
  Ctx &ctx;
  const hipStream_t s;
  const int kb, m, n;
  const size_t ldx, ldy;
  const T *const d, *const e;   // the handle's equilibration
  const T nrmA;
  const char *const label;      // "dense" / "sparse" in the verbose lines
  const SolveParams &p;
  const BatchOut &out;
  const double t0;
  double t1 = 0;
  const int vbx, vby;
  DevBuf<T> x[2], y[2], xt, yt, xtemp, ytemp, x12, y12, zx, zy, u;
  // functions: originals (h, b used as they are) and equilibrated copies, per problem
  std::vector<FnBuf<T>> fo, go, fsc, gsc;
  std::vector<FnView<T>> views;
  DevBuf<FnView<T>> dviews;
  DevBuf<double> vpart, tpart, epart, bS;
  PinnedBuf<double> hS;
  std::vector<AdmmControl<T>> ctl;
  std::vector<T> zs;
  int cur = 0;
  unsigned long long batch_iters = 0, prob_iters = 0;
  EventTimer timer;   // the batch's own stopwatch: the solo stats stay those of the last solo solve
  DevBuf<T> ox, oy, ol, omu;
  DevBuf<double> fpart, fval;

  // Refuses a bad k / out before anything is allocated or launched.
  BatchAdmm(Ctx &c, int m_, int n_, size_t ldx_, size_t ldy_, const T *d_, const T *e_, T nrmA_, const char *label_,
            int k, const FnHost *f, const FnHost *g, const double *rho0, const SolveParams &p_, const BatchOut &out_)
      : ctx(c), s(c.stream), kb(checked_k(k, out_)), m(m_), n(n_), ldx(ldx_), ldy(ldy_), d(d_), e(e_), nrmA(nrmA_),
        label(label_), p(p_), out(out_), t0(wall_s()), vbx(vec_blocks(n_)), vby(vec_blocks(m_)), fo(k), go(k), fsc(k),
        gsc(k), views(2 * k), dviews(2 * k), vpart(static_cast<size_t>(k) * (vbx + vby) * 3),
        tpart(static_cast<size_t>(k) * (vbx + vby) * 2), epart(static_cast<size_t>(k) * (vbx + vby)),
        bS(static_cast<size_t>(k) * kBatchRec), hS(static_cast<size_t>(k) * kBatchRec), zs(k, static_cast<T>(1)),
        ox(ldx_), oy(ldy_), ol(ldy_), omu(ldx_), fpart(static_cast<size_t>(vbx + vby)), fval(2) {
    DevBuf<T> *xs[] = {&x[0], &x[1], &xt, &xtemp, &x12, &zx}, *ys[] = {&y[0], &y[1], &yt, &ytemp, &y12, &zy, &u};
    for (DevBuf<T> *b : xs) { b->alloc(ldx * kb); b->zero(s); }
    for (DevBuf<T> *b : ys) { b->alloc(ldy * kb); b->zero(s); }
    for (int j = 0; j < kb; ++j) {
      fo[j].alloc(m); go[j].alloc(n); fsc[j].alloc(m); gsc[j].alloc(n);
      upload_fn<T>(fo[j], f[j], m, s);
      upload_fn<T>(go[j], g[j], n, s);
      warn_negative_coeffs<T>(f[j], m);
      warn_negative_coeffs<T>(g[j], n);
      launch_scale_objective<T>(fo[j].view(), fsc[j].a.p, fsc[j].c.p, fsc[j].d.p, fsc[j].e.p, d, m, true, s);
      launch_scale_objective<T>(go[j].view(), gsc[j].a.p, gsc[j].c.p, gsc[j].d.p, gsc[j].e.p, e, n, false, s);
      views[2 * j] = FnView<T>{fo[j].h.p, fsc[j].a.p, fo[j].b.p, fsc[j].c.p, fsc[j].d.p, fsc[j].e.p};
      views[2 * j + 1] = FnView<T>{go[j].h.p, gsc[j].a.p, go[j].b.p, gsc[j].c.p, gsc[j].d.p, gsc[j].e.p};
      ctl.push_back(make_admm_control<T>(p, rho0 ? rho0[j] : 1.0, ctx.m_global, n));
    }
    POGS_HIP_CHECK(hipMemcpyAsync(dviews.p, views.data(), views.size() * sizeof(FnView<T>), hipMemcpyHostToDevice, s));
    bS.zero(s);
    timer.enable(ctx.stream_timer.enabled());
  }

  static int checked_k(int k, const BatchOut &o) {
    POGS_CHECK(k >= 1 && k <= kBatchMax, "batched solve: k must be in [1, POGS_AMD_BATCH_MAX]");
    POGS_CHECK(o.x && o.final_iter && o.status, "batched solve: x, final_iter and status must not be NULL");
    return k;
  }
  static BatchSlots slots_of(const std::vector<int> &idx) {
    BatchSlots sl;
    sl.nact = static_cast<int>(idx.size());
    for (int q = 0; q < sl.nact; ++q) sl.act[q] = idx[q];
    return sl;
  }
  // the sums of `jobs` into the scalar block `dev`, the block to its pinned mirror `host`; waits for the stream
  void fetch(double *dev, double *host, const BatchSumJobs &jobs, int njobs, const BatchSlots &sl) {
    launch_batch_sums(jobs, njobs, sl, dev, s);
    POGS_HIP_CHECK(hipGetLastError());
    POGS_HIP_CHECK(hipMemcpyAsync(host, dev, static_cast<size_t>(kb) * kBatchRec * sizeof(double),
                                  hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipStreamSynchronize(s));
  }
  BatchVecArgs<T> vec_args(const BatchSlots &sl) const {
    BatchVecArgs<T> a;
    a.n = n; a.m = m; a.bx = vbx; a.by = vby; a.ldx = ldx; a.ldy = ldy;
    a.fg = dviews.p; a.sl = sl;
    for (int j = 0; j < kBatchMax; ++j) { a.rho[j] = j < kb ? ctl[j].rho : 0; a.zs[j] = j < kb ? zs[j] : 0; }
    a.alpha = ctl[0].alpha();
    a.x_cur = x[cur].p; a.y_cur = y[cur].p; a.xt = xt.p; a.yt = yt.p;
    a.x12 = x12.p; a.y12 = y12.p; a.xtemp = xtemp.p; a.ytemp = ytemp.p;
    a.x_new = x[cur ^ 1].p; a.y_new = y[cur ^ 1].p;
    a.zx = zx.p; a.zy = zy.p; a.u = u.p;
    a.part = nullptr;
    return a;
  }
  // optval and the un-scaled outputs of problem j from the current iterate (pogs.cpp:473-482, 510-518)
  void finish(int j) {
    const size_t xo = static_cast<size_t>(j) * ldx, yo = static_cast<size_t>(j) * ldy;
    launch_func_eval<T>(m, views[2 * j], y12.p + yo, fpart.p, s);
    launch_func_eval<T>(n, views[2 * j + 1], x12.p + xo, fpart.p + vby, s);
    SumJob sj[2] = {{fpart.p, vby, 1, fval.p}, {fpart.p + vby, vbx, 1, fval.p + 1}};
    launch_sum_jobs(sj, 2, s);
    UnscaleArgs<T> a;
    a.n_x = n; a.n_y = m;
    a.x12 = x12.p + xo; a.y12 = y12.p + yo; a.xt = xt.p + xo; a.yt = yt.p + yo;
    a.xprev = x[cur].p + xo; a.yprev = y[cur].p + yo; a.d = d; a.e = e;
    a.zt_scale = zs[j]; a.rho = ctl[j].rho;
    a.x_out = ox.p; a.y_out = oy.p; a.l_out = ol.p; a.mu_out = omu.p;
    launch_unscale<T>(a, s);
    double fv[2];
    POGS_HIP_CHECK(hipMemcpyAsync(fv, fval.p, sizeof(fv), hipMemcpyDeviceToHost, s));
    auto to_host = [&](void *dst, const DevBuf<T> &src, int cnt) {   // a null output is not wanted
      if (!dst) return;
      POGS_HIP_CHECK(hipMemcpyAsync(static_cast<T *>(dst) + static_cast<size_t>(j) * cnt, src.p, cnt * sizeof(T),
                                    hipMemcpyDeviceToHost, s));
    };
    to_host(out.x, ox, n);
    to_host(out.y, oy, m);
    to_host(out.l, ol, m);
    to_host(out.mu, omu, n);
    POGS_HIP_CHECK(hipStreamSynchronize(s));
    if (out.optval) out.optval[j] = static_cast<double>(static_cast<T>(fv[0]) + static_cast<T>(fv[1]));
    out.final_iter[j] = ctl[j].k;
    out.status[j] = ctl[j].status();
    if (p.verbose > 0)
      std::printf("POGS-AMD %s batch: problem %d, status %d, iter %u, rho %.3e\n", label, j, out.status[j], ctl[j].k,
                  static_cast<double>(ctl[j].rho));
  }

  // The warm begin, between the constructor and run(): every member j that w lists starts from the caller's
  // (x0, l0) at its own rho as a solo solve does after SetInitX + SetInitLambda (pogs.cpp:144-156; dense_iter.h
  // apply_warm_start): x = x0 / e, y = A x, t = l0 / d, xt = (A^T t) (1 / rho_j), yt = t (-1 / rho_j); xtemp and
  // ytemp stay zero.  One scaling launch, the back end's two shared products over the warm members only, one closing
  // launch.  A cold member's vectors are not touched and its x0 / l0 are not read; the padding stays zero.
  template <typename Products>
  void warm_begin(const BatchWarm &w, Products &&residual_products) {
    std::vector<int> warm;
    for (int j = 0; j < kb; ++j)
      if (w.is_warm(j)) warm.push_back(j);
    if (warm.empty()) return;
    DevBuf<T> x0(ldx * kb), l0(ldy * kb);
    const T *hx = static_cast<const T *>(w.x0), *hl = static_cast<const T *>(w.l0);
    // one strided copy per run of consecutive warm members (two in all when every member is warm)
    for (size_t q = 0; q < warm.size();) {
      size_t r = q + 1;
      while (r < warm.size() && warm[r] == warm[r - 1] + 1) ++r;
      const size_t j0 = static_cast<size_t>(warm[q]), cnt = r - q;
      POGS_HIP_CHECK(hipMemcpy2DAsync(x0.p + j0 * ldx, ldx * sizeof(T), hx + j0 * n, n * sizeof(T), n * sizeof(T), cnt,
                                      hipMemcpyHostToDevice, s));
      POGS_HIP_CHECK(hipMemcpy2DAsync(l0.p + j0 * ldy, ldy * sizeof(T), hl + j0 * m, m * sizeof(T), m * sizeof(T), cnt,
                                      hipMemcpyHostToDevice, s));
      q = r;
    }
    BatchWarmArgs<T> a;
    a.n = n; a.m = m; a.bx = vbx; a.by = vby; a.ldx = ldx; a.ldy = ldy;
    a.sl = slots_of(warm);
    a.x0 = x0.p; a.l0 = l0.p; a.d = d; a.e = e;
    a.x12 = x12.p; a.u = u.p; a.zx = zx.p; a.zy = zy.p;
    a.x_cur = x[cur].p; a.y_cur = y[cur].p; a.xt = xt.p; a.yt = yt.p;
    for (int j = 0; j < kBatchMax; ++j) {
      a.pos[j] = j < kb ? static_cast<T>(1) / ctl[j].rho : 0;
      a.neg[j] = j < kb ? static_cast<T>(-1) / ctl[j].rho : 0;
    }
    launch_batch_warm_scale<T>(a, s);
    POGS_HIP_CHECK(hipGetLastError());
    residual_products(a.sl);   // zy = A x12, zx = A^T u
    launch_batch_warm_close<T>(a, s);
    POGS_HIP_CHECK(hipGetLastError());
    POGS_HIP_CHECK(hipStreamSynchronize(s));   // x0 and l0 are freed at scope exit
  }
  // each member's rho at its stop (nothing of a member changes after it)
  void rho_out(double *rho_final) const {
    if (!rho_final) return;
    for (int j = 0; j < kb; ++j) rho_final[j] = static_cast<double>(ctl[j].rho);
  }

  // Runs every problem to its stop; leaves iterations and reserved[4..6] in the handle's stats (matvecs, cg_iters and
  // reserved[7] are the back end's to add).
  template <typename Project, typename Products>
  void run(Project &&project, Products &&residual_products) {
    std::vector<int> active(kb);
    for (int j = 0; j < kb; ++j) active[j] = j;
    ctx.sync();
    t1 = wall_s();
    while (!active.empty()) {
      const BatchSlots sl = slots_of(active);
      const int nw = cur ^ 1;
      BatchVecArgs<T> va = vec_args(sl);
      // (1) prox + over-relaxation, all active problems
      va.part = vpart.p;
      launch_batch_pre<T>(va, s);
      // (2) projection of (xtemp, ytemp) onto y = A x
      project(sl, nw);
      va.part = tpart.p;
      launch_batch_tail<T>(va, s);
      // (3) one poll for every problem's sums
      BatchSumJobs jobs;
      jobs.j[0] = BatchSumJob{vpart.p, vbx + vby, 3, 0, vbx, kBrPreX};
      jobs.j[1] = BatchSumJob{vpart.p, vbx + vby, 3, vbx, vbx + vby, kBrPreY};
      jobs.j[2] = BatchSumJob{tpart.p, vbx + vby, 2, 0, vbx, kBrTailX};
      jobs.j[3] = BatchSumJob{tpart.p, vbx + vby, 2, vbx, vbx + vby, kBrTailY};
      fetch(bS.p, hS.p, jobs, 4, sl);
      // (4) per-problem bounds; (5) exact residuals for the problems whose bounds ask for them
      std::vector<int> exact;
      std::vector<std::array<double, kNumSlots>> S(kb);
      for (int j : active) {
        double *Sj = S[j].data();
        std::fill(Sj, Sj + kNumSlots, 0.0);
        const double *r = hS.p + static_cast<size_t>(j) * kBatchRec;
        for (int q = 0; q < 3; ++q) { Sj[kGapX + q] = r[kBrPreX + q]; Sj[kGapY + q] = r[kBrPreY + q]; }
        Sj[kDXprev2] = r[kBrTailX]; Sj[kDX12] = r[kBrTailX + 1];
        Sj[kDYprev2] = r[kBrTailY]; Sj[kDY12] = r[kBrTailY + 1];
        ctl[j].set_pre(Sj);
        if (ctl[j].set_approx(Sj, nrmA)) exact.push_back(j);
      }
      if (!exact.empty()) {
        const BatchSlots se = slots_of(exact);
        BatchVecArgs<T> ve = vec_args(se);
        launch_batch_exact_u<T>(ve, s);
        residual_products(se);
        ve.part = epart.p;
        launch_batch_exact<T>(ve, s);
        BatchSumJobs ej;
        ej.j[0] = BatchSumJob{epart.p, vbx + vby, 1, 0, vbx, kBrExS};
        ej.j[1] = BatchSumJob{epart.p, vbx + vby, 1, vbx, vbx + vby, kBrExR};
        fetch(bS.p, hS.p, ej, 2, se);
        for (int j : exact) {
          const double *r = hS.p + static_cast<size_t>(j) * kBatchRec;
          S[j][kExactS2] = r[kBrExS];
          S[j][kExactR2] = r[kBrExR];
          ctl[j].set_exact(S[j].data());
        }
      }
      ++batch_iters;
      std::vector<int> still;
      for (int j : active) {
        const bool ex = std::find(exact.begin(), exact.end(), j) != exact.end();
        ++prob_iters;
        if (ctl[j].check_stop(ex)) {
          finish(j);   // frozen: its outputs from this iteration, and it leaves the active list
          continue;
        }
        zs[j] = ctl[j].adapt();
        ++ctl[j].k;
        still.push_back(j);
      }
      active.swap(still);
      // (dual update already in xtemp / ytemp: swap roles)
      std::swap(xt, xtemp);
      std::swap(yt, ytemp);
      cur = nw;
    }
    ctx.sync();
    PogsAmdStats &st = ctx.stats;
    st.iterations = static_cast<unsigned>(batch_iters);
    st.reserved[4] = static_cast<double>(prob_iters);
    if (timer.enabled()) {
      unsigned long long cnt = 0;
      st.reserved[5] = timer.collect_ms(&cnt);
      st.reserved[6] = static_cast<double>(cnt);
    }
  }
  // the closing verbose line; `extra` goes between the iteration count and the times ("" or ", 12 CG steps")
  void say_done(const char *extra) const {
    if (p.verbose > 0)
      std::printf("POGS-AMD %s batch: %d problems, %llu batch iterations%s, loop %.3e s, total %.3e s\n", label, kb,
                  batch_iters, extra, wall_s() - t1, wall_s() - t0);
  }
};

}  // namespace pogs_amd
