// SparseSolver: batched solves -- up to kBatchMax problems (own f, g, rho) on the handle's sparse matrix, every
// product with A or A^T shared by all of them (one GPU, tall or wide, CSR or CSC input).
//
// The equilibration and the norm estimate depend on A only, so K graph-form problems on one matrix can run their
// ADMM iterations side by side.  Each product reads the handle's equilibrated plain CSR copy (A_ for A v, At_ for
// A^T v) once and forms the K dot products of every row from it (sparse_batch_kernels.hip); the K operands are packed
// interleaved, [col][Kp], so the K values of a column are one gather.  The projection is a batched CGLS: every
// member runs its own CG (shift 1, at most 500 steps, its own AdmmControl::proj_tol(), warm-started from its previous
// x), a member whose CG has stopped leaves the slot list for the rest of that projection, and the host polls once
// per CG step.  The element-wise stages are those of the dense batch (batch_kernels.hip).
//
// Every product a problem takes part in is formed the same way whatever the other problems and its slot: problem j
// alone, in slot 15 of a 16-problem batch, or next to any other problems gives the same bytes.
//
// Member definition of the class template in sparse.hip, which includes this file once, right after the class,
// inside its namespaces (no include guard, no namespace of its own).

template <typename T>
void SparseSolver<T>::solve_batch_sparse(int kb, const FnHost *f, const FnHost *g, const double *rho0,
                                         const SolveParams &p, const BatchOut &out) {
  POGS_CHECK(kb >= 1 && kb <= kBatchMax, "batched solve: k must be in [1, POGS_AMD_BATCH_MAX]");
  POGS_CHECK(!multi_, "batched sparse solves are single-GPU (the handle has row shards)");
  POGS_CHECK(out.x && out.final_iter && out.status, "batched solve: x, final_iter and status must not be NULL");
  const double t0 = wall_s();
  hipStream_t s = ctx_.stream;
  const int n = n_, m = m_;
  const size_t ldx = round_up(static_cast<size_t>(n), 64), ldy = round_up(static_cast<size_t>(m), 64);
  const size_t nx = ldx * kb, ny = ldy * kb;
  // per-problem vectors, problem p at offset p * ld; zero padding throughout
  DevBuf<T> bx[2], by[2], bxt(nx), byt(ny), bxtemp(nx), bytemp(ny), bx12(nx), by12(ny), bzx(nx), bzy(ny), bu(ny),
      cr(ny), cq(ny), cp(nx), cs(nx);
  for (int q = 0; q < 2; ++q) { bx[q].alloc(nx); by[q].alloc(ny); }
  DevBuf<T> *all[] = {&bx[0], &bx[1], &by[0], &by[1], &bxt, &byt, &bxtemp, &bytemp, &bx12, &by12, &bzx, &bzy, &bu,
                      &cr, &cq, &cp, &cs};
  for (DevBuf<T> *b : all) b->zero(s);
  DevBuf<T> pk(static_cast<size_t>(std::max(m, n)) * kBatchMax);   // interleaved operands [col][Kp]
  // functions: originals (h, b used as they are) and equilibrated copies, per problem
  std::vector<FnBuf<T>> fo(kb), go(kb), fsc(kb), gsc(kb);
  std::vector<FnView<T>> views(2 * kb);
  for (int j = 0; j < kb; ++j) {
    fo[j].alloc(m); go[j].alloc(n); fsc[j].alloc(m); gsc[j].alloc(n);
    upload_fn<T>(fo[j], f[j], m, s);
    upload_fn<T>(go[j], g[j], n, s);
    warn_negative_coeffs<T>(f[j], m);
    warn_negative_coeffs<T>(g[j], n);
    launch_scale_objective<T>(fo[j].view(), fsc[j].a.p, fsc[j].c.p, fsc[j].d.p, fsc[j].e.p, d_.p, m, true, s);
    launch_scale_objective<T>(go[j].view(), gsc[j].a.p, gsc[j].c.p, gsc[j].d.p, gsc[j].e.p, e_.p, n, false, s);
    views[2 * j] = FnView<T>{fo[j].h.p, fsc[j].a.p, fo[j].b.p, fsc[j].c.p, fsc[j].d.p, fsc[j].e.p};
    views[2 * j + 1] = FnView<T>{go[j].h.p, gsc[j].a.p, go[j].b.p, gsc[j].c.p, gsc[j].d.p, gsc[j].e.p};
  }
  DevBuf<FnView<T>> dviews(2 * kb);
  POGS_HIP_CHECK(hipMemcpyAsync(dviews.p, views.data(), views.size() * sizeof(FnView<T>), hipMemcpyHostToDevice, s));
  // product geometry: from the matrix only (the same for every k and slot)
  const SpBatchCsr<T> MA = sp_batch_geometry(A_.val.p, A_.ind.p, A_.ptr.p, m, nnz_, ctx_.num_cu);
  const SpBatchCsr<T> MT = sp_batch_geometry(At_.val.p, At_.ind.p, At_.ptr.p, n, nnz_, ctx_.num_cu);
  const int vbx = vec_blocks(n), vby = vec_blocks(m);
  DevBuf<double> vpart(static_cast<size_t>(kb) * (vbx + vby) * 3), tpart(static_cast<size_t>(kb) * (vbx + vby) * 2),
      epart(static_cast<size_t>(kb) * (vbx + vby)), bS(static_cast<size_t>(kb) * kBatchRec);
  DevBuf<double> qpart(static_cast<size_t>(kb) * MA.grid), spart(static_cast<size_t>(kb) * MT.grid),
      xpart(static_cast<size_t>(kb) * vbx), ppart(static_cast<size_t>(kb) * vbx), bC(static_cast<size_t>(kb) * kBatchRec),
      bcg(static_cast<size_t>(kb) * kSbCg);
  PinnedBuf<double> hS(static_cast<size_t>(kb) * kBatchRec), hC(static_cast<size_t>(kb) * kBatchRec);
  bS.zero(s);
  bC.zero(s);
  bcg.zero(s);

  std::vector<AdmmControl<T>> ctl(kb);
  std::vector<T> zs(kb, static_cast<T>(1));
  for (int j = 0; j < kb; ++j) {
    AdmmControl<T> &c = ctl[j];
    c.abs_tol = static_cast<T>(p.abs_tol);
    c.rel_tol = static_cast<T>(p.rel_tol);
    c.max_iter = p.max_iter;
    c.adaptive_rho = p.adaptive_rho;
    c.gap_stop = p.gap_stop;
    c.rho0 = static_cast<T>(rho0 ? rho0[j] : 1.0);
    c.m_glob = ctx_.m_global;
    c.n = n_;
    c.reset();
  }
  int cur = 0;
  unsigned long long products = 0, batch_iters = 0, prob_iters = 0, cg_steps = 0;
  double prod_bytes = 0;
  EventTimer timer;   // the batch's own stopwatch: the solo stats stay those of the last solo solve
  timer.enable(ctx_.stream_timer.enabled());
  auto slots_of = [&](const std::vector<int> &idx) {
    BatchSlots sl;
    sl.nact = static_cast<int>(idx.size());
    for (int q = 0; q < sl.nact; ++q) sl.act[q] = idx[q];
    return sl;
  };
  // Y = M X (+ beta yin) over the problems of sl; X has M's column count of elements per problem
  auto product = [&](const SpBatchCsr<T> &M, int cols, const T *X, size_t ldin, T *Y, size_t ldout, const T *yin,
                     T beta, double *part, const BatchSlots &sl) {
    launch_sp_batch_pack<T>(X, ldin, cols, sl, pk.p, s);
    timer.begin(s);
    launch_sp_batch_spmv<T>(M, pk.p, sl, Y, ldout, yin, ldout, beta, part, s);
    timer.end(s);
    POGS_HIP_CHECK(hipGetLastError());
    ++products;
    if (timer.enabled())   // algorithmic bytes: the CSR once, K operand and K result vectors
      prod_bytes += static_cast<double>(nnz_) * (sizeof(T) + 4) + 4.0 * (M.nrows + 1) +
                    static_cast<double>(sizeof(T)) * sl.nact * (static_cast<double>(cols) + M.nrows);
  };
  auto fetch = [&](double *dev, double *host, const BatchSumJobs &jobs, int njobs, const BatchSlots &sl) {
    launch_batch_sums(jobs, njobs, sl, dev, s);
    POGS_HIP_CHECK(hipGetLastError());
    POGS_HIP_CHECK(hipMemcpyAsync(host, dev, static_cast<size_t>(kb) * kBatchRec * sizeof(double),
                                  hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipStreamSynchronize(s));
  };
  auto sum_only = [&](const BatchSumJob &job, const BatchSlots &sl) {
    BatchSumJobs jobs;
    jobs.j[0] = job;
    launch_batch_sums(jobs, 1, sl, bC.p, s);
  };
  auto vec_args = [&](const BatchSlots &sl) {
    BatchVecArgs<T> a;
    a.n = n; a.m = m; a.bx = vbx; a.by = vby; a.ldx = ldx; a.ldy = ldy;
    a.fg = dviews.p; a.sl = sl;
    for (int j = 0; j < kBatchMax; ++j) { a.rho[j] = j < kb ? ctl[j].rho : 0; a.zs[j] = j < kb ? zs[j] : 0; }
    a.alpha = ctl[0].alpha();
    a.x_cur = bx[cur].p; a.y_cur = by[cur].p; a.xt = bxt.p; a.yt = byt.p;
    a.x12 = bx12.p; a.y12 = by12.p; a.xtemp = bxtemp.p; a.ytemp = bytemp.p;
    a.x_new = bx[cur ^ 1].p; a.y_new = by[cur ^ 1].p;
    a.zx = bzx.p; a.zy = bzy.p; a.u = bu.p;
    a.part = nullptr;
    return a;
  };
  const double shift = 1.0, kEps = std::numeric_limits<T>::epsilon();
  // ProjectorCgls::Project for the problems of sl (projector_cgls.cpp:59-78, cgls.h:200-323): x_new from
  // (xtemp, ytemp), warm-started from x_cur with A x_cur = y_cur; then y_new = A x_new
  auto project = [&](const BatchSlots &sl, int nw) {
    SpBatchCgArgs<T> c;
    c.n = n; c.m = m; c.bx = vbx; c.by = vby; c.ldx = ldx; c.ldy = ldy; c.sl = sl;
    c.cg = bcg.p; c.x = bx[nw].p; c.r = cr.p; c.p = cp.p; c.q = cq.p; c.sv = cs.p;
    c.x0 = bxtemp.p; c.y0 = bytemp.p; c.xw = bx[cur].p; c.yw = by[cur].p;
    c.part = nullptr; c.first = false;
    // r = y0 - A x_warm ; x <- x_warm - x0
    launch_sp_batch_cg_init<T>(c, s);
    // s = A^T r - shift x ; gamma = |s|^2 ; p = s                          (cgls.h:236-245)
    product(MT, m, cr.p, ldy, cs.p, ldx, bx[nw].p, static_cast<T>(-shift), spart.p, sl);
    sum_only(BatchSumJob{spart.p, MT.grid, 1, 0, MT.grid, kSbS2}, sl);
    launch_sp_batch_cg_scalars(0, sl, bC.p, bcg.p, shift, kEps, s);
    c.part = ppart.p; c.first = true;
    launch_sp_batch_cg_p<T>(c, s);
    c.first = false;
    BatchSumJobs j0;
    j0.j[0] = BatchSumJob{ppart.p, vbx, 1, 0, vbx, kSbP2};
    fetch(bC.p, hC.p, j0, 1, sl);
    std::vector<double> norms0(kb, 0.0);
    std::vector<int> cgk(kb, 0), live;
    for (int q = 0; q < sl.nact; ++q) {
      const int j = sl.act[q];
      norms0[j] = std::sqrt(hC.p[static_cast<size_t>(j) * kBatchRec + kSbS2]);
      if (!(norms0[j] < kEps)) live.push_back(j);                       // flag 1 / projector_cgls.cpp:17
    }
    while (!live.empty()) {
      const BatchSlots cl = slots_of(live);
      c.sl = cl;
      // q = A p, |q|^2 ; alpha                                               (cgls.h:257-271)
      product(MA, n, cp.p, ldx, cq.p, ldy, nullptr, static_cast<T>(0), qpart.p, cl);
      sum_only(BatchSumJob{qpart.p, MA.grid, 1, 0, MA.grid, kSbQ2}, cl);
      launch_sp_batch_cg_scalars(1, cl, bC.p, bcg.p, shift, kEps, s);
      // x += alpha p ; r -= alpha q ; |x|^2                                   (:274-277)
      c.part = xpart.p;
      launch_sp_batch_cg_xr<T>(c, s);
      // s = A^T r - shift x ; |s|^2 ; beta ; p = s + beta p ; |p|^2           (:281-296)
      product(MT, m, cr.p, ldy, cs.p, ldx, bx[nw].p, static_cast<T>(-shift), spart.p, cl);
      sum_only(BatchSumJob{spart.p, MT.grid, 1, 0, MT.grid, kSbS2}, cl);
      launch_sp_batch_cg_scalars(2, cl, bC.p, bcg.p, shift, kEps, s);
      c.part = ppart.p;
      launch_sp_batch_cg_p<T>(c, s);
      BatchSumJobs jobs;
      jobs.j[0] = BatchSumJob{xpart.p, vbx, 1, 0, vbx, kSbX2};
      jobs.j[1] = BatchSumJob{ppart.p, vbx, 1, 0, vbx, kSbP2};
      fetch(bC.p, hC.p, jobs, 2, cl);
      ++cg_steps;
      std::vector<int> still;
      for (int j : live) {
        const double *r = hC.p + static_cast<size_t>(j) * kBatchRec;
        const double norms = std::sqrt(r[kSbS2]), normx = std::sqrt(r[kSbX2]);
        const double tol = static_cast<double>(ctl[j].proj_tol());
        const bool converged = (norms <= norms0[j] * tol) || (normx * tol >= 1.0);   // :301-305
        if (!converged && ++cgk[j] < 500) still.push_back(j);                     // maxit, projector_cgls.cpp:17
      }
      live.swap(still);
    }
    c.sl = sl;
    // x <- x + x0 (projector_cgls.cpp:75); y = A x (:78)
    launch_sp_batch_cg_close<T>(c, s);
    product(MA, n, bx[nw].p, ldx, by[nw].p, ldy, nullptr, static_cast<T>(0), nullptr, sl);
  };
  // optval and the un-scaled outputs of problem j from the current iterate (pogs.cpp:473-482, 510-518)
  DevBuf<T> ox(ldx), oy(ldy), ol(ldy), omu(ldx);
  DevBuf<double> fpart(static_cast<size_t>(vbx + vby)), fval(2);
  auto finish = [&](int j) {
    const size_t xo = static_cast<size_t>(j) * ldx, yo = static_cast<size_t>(j) * ldy;
    launch_func_eval<T>(m, views[2 * j], by12.p + yo, fpart.p, s);
    launch_func_eval<T>(n, views[2 * j + 1], bx12.p + xo, fpart.p + vby, s);
    SumJob sj[2] = {{fpart.p, vby, 1, fval.p}, {fpart.p + vby, vbx, 1, fval.p + 1}};
    launch_sum_jobs(sj, 2, s);
    UnscaleArgs<T> u;
    u.n_x = n; u.n_y = m;
    u.x12 = bx12.p + xo; u.y12 = by12.p + yo; u.xt = bxt.p + xo; u.yt = byt.p + yo;
    u.xprev = bx[cur].p + xo; u.yprev = by[cur].p + yo; u.d = d_.p; u.e = e_.p;
    u.zt_scale = zs[j]; u.rho = ctl[j].rho;
    u.x_out = ox.p; u.y_out = oy.p; u.l_out = ol.p; u.mu_out = omu.p;
    launch_unscale<T>(u, s);
    double fv[2];
    POGS_HIP_CHECK(hipMemcpyAsync(fv, fval.p, sizeof(fv), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipMemcpyAsync(static_cast<T *>(out.x) + static_cast<size_t>(j) * n, ox.p, n * sizeof(T),
                                  hipMemcpyDeviceToHost, s));
    if (out.y) POGS_HIP_CHECK(hipMemcpyAsync(static_cast<T *>(out.y) + static_cast<size_t>(j) * m, oy.p, m * sizeof(T),
                                             hipMemcpyDeviceToHost, s));
    if (out.l) POGS_HIP_CHECK(hipMemcpyAsync(static_cast<T *>(out.l) + static_cast<size_t>(j) * m, ol.p, m * sizeof(T),
                                             hipMemcpyDeviceToHost, s));
    if (out.mu) POGS_HIP_CHECK(hipMemcpyAsync(static_cast<T *>(out.mu) + static_cast<size_t>(j) * n, omu.p,
                                              n * sizeof(T), hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipStreamSynchronize(s));
    if (out.optval) out.optval[j] = static_cast<double>(static_cast<T>(fv[0]) + static_cast<T>(fv[1]));
    out.final_iter[j] = ctl[j].k;
    out.status[j] = ctl[j].status();
    if (p.verbose > 0)
      std::printf("POGS-AMD sparse batch: problem %d, status %d, iter %u, rho %.3e\n", j, out.status[j], ctl[j].k,
                  static_cast<double>(ctl[j].rho));
  };

  std::vector<int> active(kb);
  for (int j = 0; j < kb; ++j) active[j] = j;
  ctx_.sync();
  const double t1 = wall_s();
  while (!active.empty()) {
    const BatchSlots sl = slots_of(active);
    const int nw = cur ^ 1;
    BatchVecArgs<T> va = vec_args(sl);
    // (1) prox + over-relaxation, all active problems
    va.part = vpart.p;
    launch_batch_pre<T>(va, s);
    // (2) projection: batched CGLS, then y = A x
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
      if (ctl[j].set_approx(Sj, nrmA_)) exact.push_back(j);
    }
    if (!exact.empty()) {
      const BatchSlots se = slots_of(exact);
      BatchVecArgs<T> ve = vec_args(se);
      launch_batch_exact_u<T>(ve, s);
      product(MA, n, bx12.p, ldx, bzy.p, ldy, nullptr, static_cast<T>(0), nullptr, se);   // A x12
      product(MT, m, bu.p, ldy, bzx.p, ldx, nullptr, static_cast<T>(0), nullptr, se);     // A^T u
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
    std::swap(bxt, bxtemp);
    std::swap(byt, bytemp);
    cur = nw;
  }
  ctx_.sync();
  PogsAmdStats &st = ctx_.stats;
  st.iterations = static_cast<unsigned>(batch_iters);
  st.matvecs = products;
  st.cg_iters = cg_steps;
  st.reserved[4] = static_cast<double>(prob_iters);
  if (timer.enabled()) {
    unsigned long long cnt = 0;
    st.reserved[5] = timer.collect_ms(&cnt);
    st.reserved[6] = static_cast<double>(cnt);
    st.reserved[7] = prod_bytes;
  }
  if (p.verbose > 0)
    std::printf("POGS-AMD sparse batch: %d problems, %llu batch iterations, %llu CG steps, loop %.3e s, total %.3e s\n",
                kb, batch_iters, cg_steps, wall_s() - t1, wall_s() - t0);
}
