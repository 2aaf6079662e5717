// SparseSolver: batched solves -- up to kBatchMax problems (own f, g, rho) on the handle's sparse matrix, every
// product with A or A^T shared by all of them (one GPU, tall or wide, CSR or CSC input).
//
// The equilibration and the norm estimate depend on A only, so K graph-form problems on one matrix can run their
// ADMM iterations side by side.  Each product reads the operator's equilibrated plain CSR copy (A() for A v, At() for
// A^T v) once and forms the K dot products of every row from it (sparse_batch_kernels.hip); the K operands are packed
// interleaved, [col][Kp], so the K values of a column are one gather.  The projection is a batched CGLS: every
// member runs its own CG (shift 1, at most 500 steps, its own AdmmControl::proj_tol(), warm-started from its previous
// x), a member whose CG has stopped leaves the slot list for the rest of that projection, and the host polls once
// per CG step.  On a handle with the direct projector the projection is exact instead: two shared products and the two
// triangular row passes of the dense batch (launch_batch_rows over W = L^-1 and U = W^T), no inner loop and no poll.
//
// The loop and the element-wise stages are BatchAdmm's (batch_admm.h), shared with the dense batch; here are the
// handle check, the product, the projection and the two products of the exact residuals.
//
// Every product a problem takes part in is formed the same way whatever the other problems and its slot: problem j
// alone, in slot 15 of a 16-problem batch, or next to any other problems gives the same bytes.
//
// Member definition of the class template in sparse.hip, which includes this file once, right after the class,
// inside its namespaces (no include guard, no namespace of its own).

template <typename T>
void SparseSolver<T>::solve_batch_sparse(int kb, const FnHost *f, const FnHost *g, const double *rho0,
                                         const SolveParams &p, const BatchOut &out, const BatchWarm &w) {
  POGS_CHECK(!multi_, "batched sparse solves are single-GPU (the handle has row shards)");
  hipStream_t s = ctx_.stream;
  const int n = n_, m = m_;
  const size_t ldx = round_up(static_cast<size_t>(n), 64), ldy = round_up(static_cast<size_t>(m), 64);
  BatchAdmm<T> B(ctx_, m, n, ldx, ldy, d_.p, e_.p, nrmA_, "sparse", kb, f, g, rho0, p, out);
  const size_t nx = ldx * kb, ny = ldy * kb;
  DevBuf<T> cr(ny), cq(ny), cp(nx), cs(nx);   // the CG vectors, laid out as the driver's
  for (DevBuf<T> *b : {&cr, &cq, &cp, &cs}) b->zero(s);
  DevBuf<T> pk(static_cast<size_t>(std::max(m, n)) * kBatchMax);   // interleaved operands [col][Kp]
  // product geometry: from the matrix only (the same for every k and slot)
  const DevCsr<T> &A = op_->A(), &At = op_->At();
  const SpBatchCsr<T> MA = sp_batch_geometry(A.val.p, A.ind.p, A.ptr.p, m, nnz_, ctx_.num_cu);
  const SpBatchCsr<T> MT = sp_batch_geometry(At.val.p, At.ind.p, At.ptr.p, n, nnz_, ctx_.num_cu);
  const int vbx = B.vbx, vby = B.vby;
  DevBuf<double> qpart(static_cast<size_t>(kb) * MA.grid), spart(static_cast<size_t>(kb) * MT.grid),
      xpart(static_cast<size_t>(kb) * vbx), ppart(static_cast<size_t>(kb) * vbx), bC(static_cast<size_t>(kb) * kBatchRec),
      bcg(static_cast<size_t>(kb) * kSbCg);
  PinnedBuf<double> hC(static_cast<size_t>(kb) * kBatchRec);
  bC.zero(s);
  bcg.zero(s);
  unsigned long long products = 0, cg_steps = 0;
  double prod_bytes = 0;
  // Y = M X (+ beta yin) over the problems of sl; X has M's column count of elements per problem
  auto product = [&](const SpBatchCsr<T> &M, int cols, const T *X, size_t ldin, T *Y, size_t ldout, const T *yin,
                     T beta, double *part, const BatchSlots &sl) {
    launch_sp_batch_pack<T>(X, ldin, cols, sl, pk.p, s);
    B.timer.begin(s);
    launch_sp_batch_spmv<T>(M, pk.p, sl, Y, ldout, yin, ldout, beta, part, s);
    B.timer.end(s);
    POGS_HIP_CHECK(hipGetLastError());
    ++products;
    if (B.timer.enabled())   // algorithmic bytes: the CSR once, K operand and K result vectors
      prod_bytes += static_cast<double>(nnz_) * (sizeof(T) + 4) + 4.0 * (M.nrows + 1) +
                    static_cast<double>(sizeof(T)) * sl.nact * (static_cast<double>(cols) + M.nrows);
  };
  auto sum_only = [&](const BatchSumJob &job, const BatchSlots &sl) {
    BatchSumJobs jobs;
    jobs.j[0] = job;
    launch_batch_sums(jobs, 1, sl, bC.p, s);
  };
  const double shift = 1.0, kEps = std::numeric_limits<T>::epsilon();
  // ProjectorCgls::Project for the problems of sl (projector_cgls.cpp:59-78, cgls.h:200-323): x_new from
  // (xtemp, ytemp), warm-started from x_cur with A x_cur = y_cur; then y_new = A x_new
  auto project = [&](const BatchSlots &sl, int nw) {
    SpBatchCgArgs<T> c;
    c.n = n; c.m = m; c.bx = vbx; c.by = vby; c.ldx = ldx; c.ldy = ldy; c.sl = sl;
    c.cg = bcg.p; c.x = B.x[nw].p; c.r = cr.p; c.p = cp.p; c.q = cq.p; c.sv = cs.p;
    c.x0 = B.xtemp.p; c.y0 = B.ytemp.p; c.xw = B.x[B.cur].p; c.yw = B.y[B.cur].p;
    c.part = nullptr; c.first = false;
    // r = y0 - A x_warm ; x <- x_warm - x0
    launch_sp_batch_cg_init<T>(c, s);
    // s = A^T r - shift x ; gamma = |s|^2 ; p = s                          (cgls.h:236-245)
    product(MT, m, cr.p, ldy, cs.p, ldx, B.x[nw].p, static_cast<T>(-shift), spart.p, sl);
    sum_only(BatchSumJob{spart.p, MT.grid, 1, 0, MT.grid, kSbS2}, sl);
    launch_sp_batch_cg_scalars(0, sl, bC.p, bcg.p, shift, kEps, s);
    c.part = ppart.p; c.first = true;
    launch_sp_batch_cg_p<T>(c, s);
    c.first = false;
    BatchSumJobs j0;
    j0.j[0] = BatchSumJob{ppart.p, vbx, 1, 0, vbx, kSbP2};
    B.fetch(bC.p, hC.p, j0, 1, sl);
    std::vector<double> norms0(kb, 0.0);
    std::vector<int> cgk(kb, 0), live;
    for (int q = 0; q < sl.nact; ++q) {
      const int j = sl.act[q];
      norms0[j] = std::sqrt(hC.p[static_cast<size_t>(j) * kBatchRec + kSbS2]);
      if (!(norms0[j] < kEps)) live.push_back(j);                       // flag 1 / projector_cgls.cpp:17
    }
    while (!live.empty()) {
      const BatchSlots cl = B.slots_of(live);
      c.sl = cl;
      // q = A p, |q|^2 ; alpha                                               (cgls.h:257-271)
      product(MA, n, cp.p, ldx, cq.p, ldy, nullptr, static_cast<T>(0), qpart.p, cl);
      sum_only(BatchSumJob{qpart.p, MA.grid, 1, 0, MA.grid, kSbQ2}, cl);
      launch_sp_batch_cg_scalars(1, cl, bC.p, bcg.p, shift, kEps, s);
      // x += alpha p ; r -= alpha q ; |x|^2                                   (:274-277)
      c.part = xpart.p;
      launch_sp_batch_cg_xr<T>(c, s);
      // s = A^T r - shift x ; |s|^2 ; beta ; p = s + beta p ; |p|^2           (:281-296)
      product(MT, m, cr.p, ldy, cs.p, ldx, B.x[nw].p, static_cast<T>(-shift), spart.p, cl);
      sum_only(BatchSumJob{spart.p, MT.grid, 1, 0, MT.grid, kSbS2}, cl);
      launch_sp_batch_cg_scalars(2, cl, bC.p, bcg.p, shift, kEps, s);
      c.part = ppart.p;
      launch_sp_batch_cg_p<T>(c, s);
      BatchSumJobs jobs;
      jobs.j[0] = BatchSumJob{xpart.p, vbx, 1, 0, vbx, kSbX2};
      jobs.j[1] = BatchSumJob{ppart.p, vbx, 1, 0, vbx, kSbP2};
      B.fetch(bC.p, hC.p, jobs, 2, cl);
      ++cg_steps;
      std::vector<int> still;
      for (int j : live) {
        const double *r = hC.p + static_cast<size_t>(j) * kBatchRec;
        const double norms = std::sqrt(r[kSbS2]), normx = std::sqrt(r[kSbX2]);
        const double tol = static_cast<double>(B.ctl[j].proj_tol());
        const bool converged = (norms <= norms0[j] * tol) || (normx * tol >= 1.0);   // :301-305
        if (!converged && ++cgk[j] < 500) still.push_back(j);                     // maxit, projector_cgls.cpp:17
      }
      live.swap(still);
    }
    c.sl = sl;
    // x <- x + x0 (projector_cgls.cpp:75); y = A x (:78)
    launch_sp_batch_cg_close<T>(c, s);
    product(MA, n, B.x[nw].p, ldx, B.y[nw].p, ldy, nullptr, static_cast<T>(0), nullptr, sl);
  };
  auto residual_products = [&](const BatchSlots &sl) {
    product(MA, n, B.x12.p, ldx, B.zy.p, ldy, nullptr, static_cast<T>(0), nullptr, sl);   // A x12
    product(MT, m, B.u.p, ldy, B.zx.p, ldx, nullptr, static_cast<T>(0), nullptr, sl);     // A^T u
  };
  // ProjectorDirect::Project for the problems of sl (projector_direct_dense.cpp:122-135).  The operands of the row
  // passes keep zeros in their padding columns (launch_batch_rows multiplies them by zeros of the matrix): the products
  // and the passes write rows below their count only.
  const size_t ldk = tall_ ? ldx : ldy;
  DevBuf<T> brhs, btv;
  if (direct_) {
    brhs.alloc(ldk * kb); btv.alloc(ldk * kb);
    brhs.zero(s); btv.zero(s);
  }
  auto rows_pass = [&](int tri, const T *M, const T *X, T *Y, const BatchSlots &sl) {
    launch_batch_rows<T>(tri, M, kld_, k_, k_, static_cast<int>(kld_), X, ldk, Y, ldk, sl, s);
    POGS_HIP_CHECK(hipGetLastError());
  };
  auto project_direct = [&](const BatchSlots &sl, int nw) {
    if (tall_) {
      // rhs = xtemp + A^T ytemp ; x = U (W rhs) ; y = A x
      product(MT, m, B.ytemp.p, ldy, brhs.p, ldx, B.xtemp.p, static_cast<T>(1), nullptr, sl);
      rows_pass(kTriLower, Wp_, brhs.p, btv.p, sl);
      rows_pass(kTriUpper, Up_, btv.p, B.x[nw].p, sl);
      product(MA, n, B.x[nw].p, ldx, B.y[nw].p, ldy, nullptr, static_cast<T>(0), nullptr, sl);
    } else {
      // s = A xtemp - ytemp ; t = U (W s) ; x = xtemp - A^T t ; y = ytemp + t
      product(MA, n, B.xtemp.p, ldx, brhs.p, ldy, B.ytemp.p, static_cast<T>(-1), nullptr, sl);
      rows_pass(kTriLower, Wp_, brhs.p, btv.p, sl);
      rows_pass(kTriUpper, Up_, btv.p, brhs.p, sl);
      T *const z = B.zx.p;   // free here: A^T u of the exact residuals at another time
      product(MT, m, brhs.p, ldy, z, ldx, nullptr, static_cast<T>(0), nullptr, sl);
      hipLaunchKernelGGL(direct_wide_batch_kernel<T>, dim3(vbx + vby, sl.nact), dim3(256), 0, s, n, m, vbx, ldx, ldy,
                         B.xtemp.p, z, B.x[nw].p, B.ytemp.p, brhs.p, B.y[nw].p, sl);
      POGS_HIP_CHECK(hipGetLastError());
    }
  };
  B.warm_begin(w, residual_products);   // (the batched CGLS then starts from x[cur] with y[cur] = A x[cur])
  if (direct_) B.run(project_direct, residual_products);
  else B.run(project, residual_products);
  B.rho_out(w.rho_final);
  PogsAmdStats &st = ctx_.stats;
  st.matvecs = products;
  st.cg_iters = cg_steps;
  if (B.timer.enabled()) st.reserved[7] = prod_bytes;
  B.say_done(direct_ ? ", direct projector" : (", " + std::to_string(cg_steps) + " CG steps").c_str());
}
