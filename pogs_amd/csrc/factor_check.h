#pragma once
// PogsAmdGramCheck / PogsAmdCholCheck (include/pogs_amd.h, Part 3): the Gram phase and the Cholesky / inverse /
// transpose sequence of DenseSolver::factor() on HOST arrays, through the functions factor() calls.
#include <cmath>

#include "common.h"
#include "gemm.h"
#include "gram_phase.h"

namespace pogs_amd {

// what gram_product needs of the solver's Ctx, on the null stream
struct CheckHost {
  hipStream_t stream = nullptr;
  void sync() { POGS_HIP_CHECK(hipStreamSynchronize(stream)); }
  void tmark(const char *) {}
};

template <typename T>
void gram_check(int kdim, int k, const T *P, size_t lda, int num_cu, int force, T *G, size_t ldg, int *info) {
  constexpr size_t VEC = Vec16<T>::N;
  POGS_CHECK(kdim >= 1 && k >= 1, "kdim and k must be >= 1");
  POGS_CHECK(P && G && info, "null argument");
  POGS_CHECK(lda >= static_cast<size_t>(k) && lda % VEC == 0, "lda must be a multiple of VEC and >= k");
  POGS_CHECK(ldg >= static_cast<size_t>(k), "ldg must be >= k");
  POGS_CHECK(force == 0 || force == kGramForceNative || force == 128 || force == 256,
             "unknown force (0 as the solver chooses, 1 native product, 128 / 256 tile of the fp16 split)");
  POGS_CHECK(num_cu >= 0, "num_cu must be >= 0");
  if (num_cu == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    POGS_HIP_CHECK(hipGetDevice(&dev));
    POGS_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  double amax = 0;   // as the equilibration leaves it: the largest |entry| of the stored matrix
  for (int r = 0; r < kdim; ++r)
    for (int c = 0; c < k; ++c) amax = std::fmax(amax, std::fabs(static_cast<double>(P[static_cast<size_t>(r) * lda + c])));
  const size_t ld = round_up(static_cast<size_t>(k), VEC), slab = static_cast<size_t>(k) * ld;
  const size_t np = static_cast<size_t>(kdim) * lda, row = static_cast<size_t>(k) * sizeof(T);
  DevBuf<T> dP(np), fac(slab * 4);
  CheckHost host;
  POGS_HIP_CHECK(hipMemcpy(dP.p, P, np * sizeof(T), hipMemcpyHostToDevice));
  fac.zero(host.stream);
  POGS_HIP_CHECK(hipMemcpy2D(fac.p, ld * sizeof(T), G, ldg * sizeof(T), row, k, hipMemcpyHostToDevice));
  const GramInfo gi = gram_product<T>(dP.p, lda, kdim, k, true, amax, num_cu, fac.p, ld, force, host);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipMemcpy2D(G, ldg * sizeof(T), fac.p, ld * sizeof(T), row, k, hipMemcpyDeviceToHost));
  POGS_HIP_CHECK(hipDeviceSynchronize());
  const int out[8] = {gi.path, gi.tile, gi.ksplit, gi.kchunk, gi.kacc, gi.units, gi.unit_rows, gi.tile_map};
  for (int i = 0; i < 8; ++i) info[i] = out[i];
}

template <typename T>
void chol_check(int n, const T *H, size_t ldh, T *L, T *W, T *U, size_t ldo) {
  constexpr size_t VEC = Vec16<T>::N;
  POGS_CHECK(n >= 1, "n must be >= 1");
  POGS_CHECK(H && L && W && U, "null argument");
  POGS_CHECK(ldh >= static_cast<size_t>(n) && ldo >= static_cast<size_t>(n), "ldh and ldo must be >= n");
  // the leading dimension and the four slabs of factor(): [H -> L | scratch | W | U], zero before H arrives
  const size_t ld = round_up(static_cast<size_t>(n), VEC), slab = static_cast<size_t>(n) * ld;
  const size_t row = static_cast<size_t>(n) * sizeof(T), back = (ldo < ld ? ldo : ld) * sizeof(T);
  DevBuf<T> fac(slab * 4);
  hipStream_t s = nullptr;
  fac.zero(s);
  T *G = fac.p, *tmp = fac.p + slab, *Wp = fac.p + 2 * slab, *Up = fac.p + 3 * slab;
  POGS_HIP_CHECK(hipMemcpy2D(G, ld * sizeof(T), H, ldh * sizeof(T), row, n, hipMemcpyHostToDevice));
  cholesky_lower<T>(G, ld, n, Wp, ld, s);
  trtri_lower<T>(G, ld, n, Wp, ld, tmp, s);
  launch_transpose<T>(Wp, ld, n, n, Up, ld, s);
  POGS_HIP_CHECK(hipGetLastError());
  POGS_HIP_CHECK(hipMemcpy2D(L, ldo * sizeof(T), G, ld * sizeof(T), back, n, hipMemcpyDeviceToHost));
  POGS_HIP_CHECK(hipMemcpy2D(W, ldo * sizeof(T), Wp, ld * sizeof(T), back, n, hipMemcpyDeviceToHost));
  POGS_HIP_CHECK(hipMemcpy2D(U, ldo * sizeof(T), Up, ld * sizeof(T), back, n, hipMemcpyDeviceToHost));
  POGS_HIP_CHECK(hipDeviceSynchronize());
}

}  // namespace pogs_amd
