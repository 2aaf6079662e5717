// Many small dense problems, each with its own matrix (PogsAmdSolveManyFn, include/pogs_amd.h): the host driver's
// entry.  The kernels and the driver live in many_kernels.hip; DESIGN.md section 3.7 describes the design.
#pragma once
#include <vector>

#include "engine.h"

namespace pogs_amd {

// k problems of one shape (m x n, matrix j at element offset j*m*n of A, in `ord`, host or device memory `mem`),
// f[j], g[j], rho[j] (rho may be null: 1.0 each).  Throws Error on a refusal, before any output is written.
void solve_many(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem, int device, const FnHost *f,
                const FnHost *g, const double *rho, const SolveParams &p, const BatchOut &out);

// PogsAmdManySetupCheck (include/pogs_amd.h): the setup of a solve on k problems in one chunk, HOST outputs (any may
// be null).  Refusals as solve_many's, before any device work.
void many_setup_check(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem, void *A_eq, void *d,
                      void *e, double *nrmA, void *W);

}  // namespace pogs_amd
