// of2d_solvers.h — per-regularisation device buffers and kernel launchers
// beyond Horn-Schunck (Demons, Fluid, Elastic, Curvature).
#pragma once

#include "of2d_host.h"

namespace of2d {
namespace solvers {

// allocate the solver-specific fields of a level (IterativeSolver / OpticalFlow /
// Demons / OpticalFlowFluid constructors)
void alloc_level(Level &L, int reg);
// largest number of per-block Logger partials one iteration writes at this level
int max_partial_blocks(const Level &L, int reg);

// Curvature's per-level tables (eigenvalues; per axis the cosine matrices of
// the GEMM path or the twiddles of the fast path).  dct = 1 takes the fast
// line transforms on every axis whose length qualifies (dct_fast_length), 0
// the GEMMs on both.  Rebuilt when the choice differs from the level's last.
void build_curvature(Level &L, float alpha, float tau, int dct, hipStream_t st);
// REDFT10 (inverse = false; times E when E != nullptr) or REDFT01 of the plane
// pair in `cur`, axis y then axis x, by the level's paths (L.cpath); `other`
// is the second buffer of the level.  Returns the buffer that holds the result.
double *curvature_dct2d(const Level &L, bool inverse, double *cur, double *other, const double *E,
                        hipStream_t st);

}  // namespace solvers
}  // namespace of2d
