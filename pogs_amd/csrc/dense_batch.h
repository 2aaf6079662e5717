// DenseSolver: batched solves -- up to kBatchMax problems (own f, g, rho) on the handle's matrix, every pass over A
// shared by all of them (m > n, direct projector, one GPU).
//
// The projector (I + A^T A)^-1, the equilibration and the factorisation depend on A only, so K graph-form problems
// on one matrix can run their ADMM iterations side by side: each pass over a stored matrix (A, W = L^-1, U = W^T)
// reads a row tile once and forms K dot products (or K column accumulations) with it on the matrix cores.  The
// pass stays bound by HBM; the K vectors are a few MB and come through L2.
//
// The loop is BatchAdmm's (batch_admm.h); here are the handle checks and the two steps that pass over the stored
// matrices.  The kernels live in batch_kernels.hip.  Every product a problem takes part in is formed the same way
// whatever the other problems and its slot (batch_kernels.hip): problem j alone, in slot 15 of a 16-problem batch, or
// next to any other problems gives the same bytes.
//
// Member definitions of the class template declared in dense_solver.h, which includes this file once, right after
// the class, inside its namespaces (no include guard, no namespace of its own).

template <typename T, typename Tag>
void DenseSolver<T, Tag>::solve_batch(int kb, const FnHost *f, const FnHost *g, const double *rho0,
                                      const SolveParams &p, const BatchOut &out, const BatchWarm &w) {
  POGS_CHECK(!multi_, "batched solves are single-GPU (the handle has row shards)");
  POGS_CHECK(!use_cgls_, "batched solves need the direct projector (the handle uses CGLS)");
  POGS_CHECK(tall_ && !tmode_, "batched solves need m > n (the handle stores A^T)");
  hipStream_t s = ctx_.stream;
  const int n = n_, m = m_;
  const size_t ldx = static_cast<size_t>(n_pad_), ldy = static_cast<size_t>(round_up(m, Vec16<T>::N));
  BatchAdmm<T> B(ctx_, m, n, ldx, ldy, d_.p, e_.p, nrmA_, "dense", kb, f, g, rho0, p, out);
  DevBuf<T> brhs(ldx * kb);
  brhs.zero(s);
  T *const tv = B.zx.p;   // between the two triangular passes; A^T u of the exact residuals at another time
  // column-sum partials: row blocks chosen from the shape only (the same for every k and slot)
  int rpb = 0, nrb_used = 0;
  batch_cols_partition<T>(m, n_pad_, rpb, nrb_used);
  DevBuf<T> bpart(static_cast<size_t>(nrb_used) * kb * n_pad_);
  unsigned long long passes = 0;
  auto rows_pass = [&](int tri, const T *M, size_t ldm, int rows, int cols, int cols_pad, const T *X, T *Y,
                       size_t ldin, size_t ldout, const BatchSlots &sl, bool timed) {
    if (timed) B.timer.begin(s);
    launch_batch_rows<T>(tri, M, ldm, rows, cols, cols_pad, X, ldin, Y, ldout, sl, s);
    if (timed) B.timer.end(s);
    POGS_HIP_CHECK(hipGetLastError());
  };
  // Z = A^T U (+ add) over the problems of sl
  auto cols_pass = [&](const T *U, const T *add, T *Z, const BatchSlots &sl) {
    B.timer.begin(s);
    launch_batch_cols<T>(A_.p, lda_, m, n_pad_, rpb, nrb_used, U, ldy, bpart.p, kb, sl, s);
    B.timer.end(s);
    launch_batch_cols_reduce<T>(bpart.p, nrb_used, kb, n, n_pad_, add, Z, ldx, sl, s);
    POGS_HIP_CHECK(hipGetLastError());
  };
  // rhs = xtemp + A^T ytemp ; x = U (W rhs) ; y = A x
  auto project = [&](const BatchSlots &sl, int nw) {
    cols_pass(B.ytemp.p, B.xtemp.p, brhs.p, sl);
    rows_pass(kLower, Wp_, k_pad_, n, n, k_pad_, brhs.p, tv, ldx, ldx, sl, false);
    rows_pass(kUpper, Up_, k_pad_, n, n, k_pad_, tv, B.x[nw].p, ldx, ldx, sl, false);
    rows_pass(kFull, A_.p, lda_, m, n, n_pad_, B.x[nw].p, B.y[nw].p, ldx, ldy, sl, true);
    passes += 2;
  };
  auto residual_products = [&](const BatchSlots &sl) {
    rows_pass(kFull, A_.p, lda_, m, n, n_pad_, B.x12.p, B.zy.p, ldx, ldy, sl, true);
    cols_pass(B.u.p, nullptr, B.zx.p, sl);
    passes += 2;
  };
  B.warm_begin(w, residual_products);
  B.run(project, residual_products);
  B.rho_out(w.rho_final);
  PogsAmdStats &st = ctx_.stats;
  st.matvecs = passes;
  if (B.timer.enabled()) st.reserved[7] = st.reserved[6] * m * n * sizeof(T);
  B.say_done("");
}
