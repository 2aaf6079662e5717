// DenseSolver: batched solves -- up to kBatchMax problems (own f, g, rho) on the handle's matrix, every pass over A
// shared by all of them (m > n, direct projector, one GPU).
//
// The projector (I + A^T A)^-1, the equilibration and the factorisation depend on A only, so K graph-form problems
// on one matrix can run their ADMM iterations side by side: each pass over a stored matrix (A, W = L^-1, U = W^T)
// reads a row tile once and forms K dot products (or K column accumulations) with it on the matrix cores.  The
// pass stays bound by HBM; the K vectors are a few MB and come through L2.
//
// The kernels live in batch_kernels.hip.  Every product a problem takes part in is formed the same way whatever the
// other problems and its slot (batch_kernels.hip): problem j alone, in slot 15 of a 16-problem batch, or next to any
// other problems gives the same bytes.
//
// Member definitions of the class template declared in dense_solver.h, which includes this file once, right after
// the class, inside its namespaces (no include guard, no namespace of its own).

template <typename T, typename Tag>
void DenseSolver<T, Tag>::solve_batch(int kb, const FnHost *f, const FnHost *g, const double *rho0,
                                      const SolveParams &p, const BatchOut &out) {
  POGS_CHECK(kb >= 1 && kb <= kBatchMax, "batched solve: k must be in [1, POGS_AMD_BATCH_MAX]");
  POGS_CHECK(!multi_, "batched solves are single-GPU (the handle has row shards)");
  POGS_CHECK(!use_cgls_, "batched solves need the direct projector (the handle uses CGLS)");
  POGS_CHECK(tall_ && !tmode_, "batched solves need m > n (the handle stores A^T)");
  POGS_CHECK(out.x && out.final_iter && out.status, "batched solve: x, final_iter and status must not be NULL");
  const double t0 = wall_s();
  hipStream_t s = ctx_.stream;
  const int n = n_, m = m_;
  const size_t ldx = static_cast<size_t>(n_pad_), ldy = static_cast<size_t>(round_up(m, Vec16<T>::N));
  const size_t nx = ldx * kb, ny = ldy * kb;
  // per-problem vectors, problem p at offset p * ld; zero padding throughout
  DevBuf<T> bx[2], by[2], bxt(nx), byt(ny), bxtemp(nx), bytemp(ny), bx12(nx), by12(ny), brhs(nx), btv(nx), bzy(ny),
      bu(ny);
  for (int q = 0; q < 2; ++q) { bx[q].alloc(nx); by[q].alloc(ny); }
  DevBuf<T> *all[] = {&bx[0], &bx[1], &by[0], &by[1], &bxt, &byt, &bxtemp, &bytemp, &bx12, &by12, &brhs, &btv, &bzy, &bu};
  for (DevBuf<T> *b : all) b->zero(s);
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
  // column-sum partials: row blocks chosen from the shape only (the same for every k and slot)
  int rpb = 0, nrb_used = 0;
  batch_cols_partition<T>(m, n_pad_, rpb, nrb_used);
  DevBuf<T> bpart(static_cast<size_t>(nrb_used) * kb * n_pad_);
  const int vbx = vec_blocks(n), vby = vec_blocks(m);
  DevBuf<double> vpart(static_cast<size_t>(kb) * (vbx + vby) * 3), tpart(static_cast<size_t>(kb) * (vbx + vby) * 2),
      epart(static_cast<size_t>(kb) * (vbx + vby)), bS(static_cast<size_t>(kb) * kBatchRec);
  PinnedBuf<double> hS(static_cast<size_t>(kb) * kBatchRec);
  bS.zero(s);

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
  unsigned long long passes = 0, batch_iters = 0, prob_iters = 0;
  EventTimer timer;   // the batch's own stopwatch: the solo stats stay those of the last solo solve
  timer.enable(ctx_.stream_timer.enabled());
  auto slots_of = [&](const std::vector<int> &idx) {
    BatchSlots sl;
    sl.nact = static_cast<int>(idx.size());
    for (int q = 0; q < sl.nact; ++q) sl.act[q] = idx[q];
    return sl;
  };
  auto rows_pass = [&](int tri, const T *M, size_t ldm, int rows, int cols, int cols_pad, const T *X, T *Y,
                       size_t ldin, size_t ldout, const BatchSlots &sl, bool timed) {
    if (timed) timer.begin(s);
    launch_batch_rows<T>(tri, M, ldm, rows, cols, cols_pad, X, ldin, Y, ldout, sl, s);
    if (timed) timer.end(s);
    POGS_HIP_CHECK(hipGetLastError());
  };
  // Z = A^T U (+ add) over the problems of sl
  auto cols_pass = [&](const T *U, const T *add, T *Z, const BatchSlots &sl) {
    timer.begin(s);
    launch_batch_cols<T>(A_.p, lda_, m, n_pad_, rpb, nrb_used, U, ldy, bpart.p, kb, sl, s);
    timer.end(s);
    launch_batch_cols_reduce<T>(bpart.p, nrb_used, kb, n, n_pad_, add, Z, ldx, sl, s);
    POGS_HIP_CHECK(hipGetLastError());
  };
  auto fetch = [&](const BatchSumJobs &jobs, int njobs, const BatchSlots &sl) {
    launch_batch_sums(jobs, njobs, sl, bS.p, s);
    POGS_HIP_CHECK(hipGetLastError());
    POGS_HIP_CHECK(hipMemcpyAsync(hS.p, bS.p, static_cast<size_t>(kb) * kBatchRec * sizeof(double),
                                  hipMemcpyDeviceToHost, s));
    POGS_HIP_CHECK(hipStreamSynchronize(s));
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
    a.zx = btv.p; a.zy = bzy.p; a.u = bu.p;
    a.part = nullptr;
    return a;
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
      std::printf("POGS-AMD dense batch: problem %d, status %d, iter %u, rho %.3e\n", j, out.status[j], ctl[j].k,
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
    // (2) rhs = xtemp + A^T ytemp
    cols_pass(bytemp.p, bxtemp.p, brhs.p, sl);
    // (3) x = U (W rhs)
    rows_pass(kLower, Wp_, k_pad_, n, n, k_pad_, brhs.p, btv.p, ldx, ldx, sl, false);
    rows_pass(kUpper, Up_, k_pad_, n, n, k_pad_, btv.p, bx[nw].p, ldx, ldx, sl, false);
    // (4) y = A x
    rows_pass(kFull, A_.p, lda_, m, n, n_pad_, bx[nw].p, by[nw].p, ldx, ldy, sl, true);
    va.part = tpart.p;
    launch_batch_tail<T>(va, s);
    passes += 2;
    // (5) one poll for every problem's sums
    BatchSumJobs jobs;
    jobs.j[0] = BatchSumJob{vpart.p, vbx + vby, 3, 0, vbx, kBrPreX};
    jobs.j[1] = BatchSumJob{vpart.p, vbx + vby, 3, vbx, vbx + vby, kBrPreY};
    jobs.j[2] = BatchSumJob{tpart.p, vbx + vby, 2, 0, vbx, kBrTailX};
    jobs.j[3] = BatchSumJob{tpart.p, vbx + vby, 2, vbx, vbx + vby, kBrTailY};
    fetch(jobs, 4, sl);
    // (6) per-problem bounds; (7) exact residuals for the problems whose bounds ask for them
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
      rows_pass(kFull, A_.p, lda_, m, n, n_pad_, bx12.p, bzy.p, ldx, ldy, se, true);
      cols_pass(bu.p, nullptr, btv.p, se);
      ve.part = epart.p;
      launch_batch_exact<T>(ve, s);
      passes += 2;
      BatchSumJobs ej;
      ej.j[0] = BatchSumJob{epart.p, vbx + vby, 1, 0, vbx, kBrExS};
      ej.j[1] = BatchSumJob{epart.p, vbx + vby, 1, vbx, vbx + vby, kBrExR};
      fetch(ej, 2, se);
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
  st.matvecs = passes;
  st.reserved[4] = static_cast<double>(prob_iters);
  if (timer.enabled()) {
    unsigned long long cnt = 0;
    st.reserved[5] = timer.collect_ms(&cnt);
    st.reserved[6] = static_cast<double>(cnt);
    st.reserved[7] = static_cast<double>(cnt) * m * n * sizeof(T);
  }
  if (p.verbose > 0)
    std::printf("POGS-AMD dense batch: %d problems, %llu batch iterations, loop %.3e s, total %.3e s\n", kb, batch_iters,
                wall_s() - t1, wall_s() - t0);
}
