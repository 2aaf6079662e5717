// Many small dense problems, each with its own matrix (PogsAmdSolveManyFn, include/pogs_amd.h): the host driver's
// entries.  One translation unit, many_kernels.hip, holds the driver: ManySet<T>, the device buffers of a set of
// resident problems (one per one-shot solve, sized to its largest chunk; one per handle, for all k), the staging of A
// and the launch sequences.  It includes many_device.h (the kernels and their argument structs) and many_plan.h (the
// arithmetic on shapes: workspace layout, prefix sums, chunks; plain C++).  DESIGN.md section 3.7 describes the design.
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

// The argument checks solve_many and many_create share (k, dtype, ord, mem, A, the envelope); host only.
void many_check_args(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem);

// How a solve on a ManyHandle starts (PogsAmdManySolveFn): start is an enum POGS_AMD_MANY_START; x0, l0 HOST arrays
// (WARM_GIVEN only); rho and rho_final may be null.
struct ManyStart {
  int start;
  const void *x0, *l0;
  const double *rho;
  double *rho_final;
};

// The persistent many-problem handle (PogsAmdMany): k problems set up once, resident on the device.
struct ManyHandle {
  virtual ~ManyHandle() {}
  virtual int device() const = 0;
  virtual int count() const = 0;
  // Throws Error on a refusal, before any output is written or any state of the handle is changed.
  virtual void solve(const FnHost *f, const FnHost *g, const ManyStart &st, const SolveParams &p,
                     const BatchOut &out) = 0;
  virtual PogsAmdManyInfo info() const = 0;
  // the count() shapes (PogsAmdManyGetShapes); a uniform handle repeats its one shape
  virtual void shapes(size_t *m, size_t *n) const = 0;
};

// Checks as solve_many's (many_check_args), before any device work; then upload, setup, and the resident buffers.
ManyHandle *many_create(int dtype, int ord, int k, size_t m, size_t n, const void *A, int mem, int device);

// The ragged forms (PogsAmdSolveManyRaggedFn, PogsAmdManyCreateRagged): problem j is m[j] x n[j], its matrix at
// element offset sum_{i<j} m[i] n[i] of A, its rows / columns at sum_{i<j} m[i] / n[i] of every packed array.  The
// same driver, kernels and handle class; refusals name the argument and, for a shape, the problem.
void many_check_ragged(int dtype, int ord, int k, const size_t *m, const size_t *n, const void *A, int mem);
void solve_many_ragged(int dtype, int ord, int k, const size_t *m, const size_t *n, const void *A, int mem, int device,
                       const FnHost *f, const FnHost *g, const double *rho, const SolveParams &p, const BatchOut &out);
ManyHandle *many_create_ragged(int dtype, int ord, int k, const size_t *m, const size_t *n, const void *A, int mem,
                               int device);

}  // namespace pogs_amd
