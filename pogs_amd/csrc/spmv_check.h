#pragma once
// PogsAmdSpmvCheck (include/pogs_amd.h, Part 3): one product of the solo sparse solver on HOST arrays, on copies built
// by the solver's own SparseOperator (sparse_operator.h: structure, tiled copies, scale, finalize_values), with no solver
// and no equilibration around it.  spmv_check() itself is in sparse.hip.
#include <cstddef>

namespace pogs_amd {

// `format`: the switches a solve reads from POGS_AMD_SELL_FORMAT / POGS_AMD_SPMV, as an argument
// (info[7], why a copy runs the plain CSR kernel: the kSellWhy* codes of sell.h)
constexpr int kSpmvFormatAuto = 0, kSpmvFormatTags = 1, kSpmvFormatTwo = 2, kSpmvFormatPlain = 3;

struct SpmvCheckArgs {
  int dtype, ord, nrows, ncols;
  const int *ptr, *ind;
  const void *val;
  int num_cu, format, force_rr_rows, force_ncg;
  double scale;
  char trans;
  int sq;
  double x_nrm2, alpha, beta;
  const void *x;
  size_t xlen;
  void *y;
  size_t ylen;
  double *sumsq;
  int *info;
  int *t_ptr, *t_ind;
  void *t_val;
  int mixed;   // PogsAmdSpmvMixedCheck (dtype F64, sq 0): the values rounded to float and the tiled copies' values stored as floats
};

void spmv_check(const SpmvCheckArgs &a);

}  // namespace pogs_amd
